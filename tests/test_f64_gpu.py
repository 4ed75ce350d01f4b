"""The f32 path against float64 references (util.assert_f64_close): the oracle evaluated in float64 on the GPU
through torch's own ops, with the same oracle in float32 (TF32 off) on the same inputs as the unit of error. The
HIP result must be within F64_K = 4 of the float32 evaluation's error, elementwise and normwise. Decoder outputs
are compared as logits (util.inv_out_act); gradient checks give rows at a leaky-ReLU / clamp kink (util.kink_rows)
zero upstream gradient on both sides; arg-max selections are fed to the references as the product made them
and checked on their own against the float64 logits."""
import gc

import pytest
import torch

from util import (K_BIAS, assert_f64_close, check_selection, inv_out_act, k_for as _k, kink_rows, make_module,
                  make_pointnet, oracle_grads, orc, run_query, tf32_off, to_dev)

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _full_precision_references():
    with tf32_off():
        yield
    gc.collect()
    torch.cuda.empty_cache()


def _dev(p, dev, dt):
    return {k: v.to(dev, dt) for k, v in p.items()}


def _logits(v, sig):
    return v.double() if sig else inv_out_act(v)


def _check_decoder_out(what, got, r64, r32, sig, report=None):
    assert_f64_close(what, _logits(got, sig), _logits(r64, sig), _logits(r32, sig), report=report)


# ---------------------------------------------------------------------------------------------------------------
# decoders: forward
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n,sig", [("IMNET", 5000, False), ("IEF", 5000, False), ("IEF", 160000, False),
                                        ("IMNET", 160000, True), ("IEF", 2500, True)])
def test_decoder_module_forward(cuda, kind, n, sig):
    d = 385
    p = orc.randomize_biases(orc.init_decoder(kind, d, 11, 5.0), 12)
    m = make_module(kind, p, d, cuda, use_sigmoid=sig)
    x = torch.randn(n, d, generator=torch.Generator().manual_seed(n)).to(cuda)
    with torch.no_grad():
        got = m(x)
        r64 = orc.decoder_forward(_dev(p, cuda, torch.float64), x.double(), kind, 2, sig)
        r32 = orc.decoder_forward(_dev(p, cuda, torch.float32), x, kind, 2, sig)
    _check_decoder_out("%s n=%d" % (kind, n), got, r64, r32, sig)


def test_decoders_pair_and_strided_rows_forward(cuda):
    """decoders_forward with both decoders (the pair launch), rows given as a view with a row stride > D."""
    from implicit_depth_amd import decoders_forward
    d, n = 385, 65536
    pp = orc.randomize_biases(orc.init_decoder("IMNET", d, 1, 5.0), 2)
    po = orc.randomize_biases(orc.init_decoder("IEF", d, 3, 5.0), 4)
    big = torch.randn(n, 400, generator=torch.Generator().manual_seed(6)).to(cuda)
    x = big[:, :d]
    with torch.no_grad():
        gp, go = decoders_forward(x, make_module("IMNET", pp, d, cuda), make_module("IEF", po, d, cuda))
        xc = x.contiguous()
        for what, got, p, kind in (("prob", gp, pp, "IMNET"), ("off", go, po, "IEF")):
            r64 = orc.decoder_forward(_dev(p, cuda, torch.float64), xc.double(), kind)
            r32 = orc.decoder_forward(_dev(p, cuda, torch.float32), xc, kind)
            _check_decoder_out(what, got, r64, r32, False)


# ---------------------------------------------------------------------------------------------------------------
# decoders: backward (dense random upstream gradient, kink rows masked)
# ---------------------------------------------------------------------------------------------------------------
def _masked_weights(p, x, kind, n, gen, cuda, sig=False):
    bad = kink_rows(_dev(p, cuda, torch.float64), x.double(), kind, use_sigmoid=sig)
    frac = bad.float().mean().item() if n else 0.0
    print("%s: %d of %d rows masked (%.3f %%)" % (kind, int(bad.sum()), n, 100 * frac))
    assert n < 1000 or frac < 0.01, frac
    w = torch.randn(n, generator=gen).to(cuda)
    return torch.where(bad, torch.zeros_like(w), w)


def _cdiv(a, b):
    return -(-a // b)


def _wgrad_plan(M, N, n, scratch=True):
    """lidf_train.hip wgrad2_launch's plan for the (M x N) weight gradient over n rows, restated: returns (plan,
    swapped, capped) with plan "one-slice" (n <= 320, added straight into C), "slab" (partial blocks in the scratch
    area and a fixed-order reduce) or "atomics" (no scratch area, or the partial blocks do not fit it); capped: the
    slice count is at the budget of 512 slabs per product."""
    swap = M > 128 and N <= 128 and n > 320
    if swap:
        M, N = N, M
    mb, nb = _cdiv(M, 128), _cdiv(N, 256)
    budget = (512 if scratch else 1024) // (mb * nb)
    splits = max(1, min(budget, _cdiv(n, 64) if scratch else _cdiv(n, 1024)))
    one_slice = scratch and n <= 320
    if one_slice:
        splits = 1
    rs = 16 if (not swap and M <= 64 and N <= 128 and mb == 1 and nb == 1) else 8
    rows_per_split = _cdiv(_cdiv(n, splits), rs) * rs
    sp = _cdiv(n, rows_per_split)
    slab = scratch and not one_slice and sp * mb * nb <= 512       # the scratch area holds 512 slabs
    return ("one-slice" if one_slice else "slab" if slab else "atomics"), swap, splits == budget


# the decoders' weight gradients as lidf_launch_wgrad splits them: layer 3 (64 x 128), layer 2 (128 x 256), layer 1's
# 385 input columns as [256] + [128 + 1]
DECODER_WGRADS = [(64, 128), (128, 256), (256, 256), (256, 128)]
# n = 1 and 320: one slice; 321 / 5,000: slab reduction below the slice cap; 160,000 / 614,400 (the train record's
# row count): at the cap; above 320 rows layer 1's [128 + 1] block is the swapped orientation
ROWS = [1, 320, 321, 5000, 160000, 614400]


def _assert_plans(n):
    plans = [_wgrad_plan(M, N, n) for M, N in DECODER_WGRADS]
    want = "one-slice" if n <= 320 else "slab"
    assert all(p == want for p, _, _ in plans), (n, plans)
    assert [sw for _, sw, _ in plans] == [False, False, False, n > 320], (n, plans)
    assert all(c == (n >= 160000) for p, _, c in plans if p == "slab"), (n, plans)


@pytest.mark.parametrize("scratch", [True, False])
@pytest.mark.parametrize("n", [320, 5000, 160000])
def test_wgrad_plans(cuda, n, scratch):
    """lidf_wgrad_f32 at the decoders' layer-1 shape (256 x 385 = [256] + [128 + 1]): one slice, slab reduction
    and, without the scratch area, the atomics fallback — weight and bias gradients against float64."""
    from implicit_depth_amd import _lib
    M, N = 256, 385
    plans = [_wgrad_plan(M, c, n, scratch) for c in (256, 128)]
    if not scratch:
        assert all(p == "atomics" for p, _, _ in plans), plans
    else:
        assert all(p == ("one-slice" if n <= 320 else "slab") for p, _, _ in plans), plans
    L = _lib.lib()
    g = torch.Generator().manual_seed(n)
    a = torch.randn(n, M, generator=g).to(cuda)
    b = torch.randn(n, N, generator=g).to(cuda)
    ws = torch.empty((L.lidf_wgrad_workspace_bytes() if scratch else 0,), dtype=torch.uint8, device=cuda)
    c, db = torch.zeros(M, N, device=cuda), torch.zeros(M, device=cuda)
    _lib.check(L.lidf_wgrad_f32(_lib.ptr(a), M, M, _lib.ptr(b), N, N, n, _lib.ptr(c), N, _lib.ptr(db),
                                _lib.ptr(ws) if scratch else None, ws.numel(), _lib.current_stream(cuda)))
    tag = "wgrad n=%d %s" % (n, "scratch" if scratch else "atomics")
    assert_f64_close(tag + " dW", c, a.double().t() @ b.double(), a.t() @ b)
    assert_f64_close(tag + " db", db, a.double().sum(0), a.sum(0), k=K_BIAS)


@pytest.mark.parametrize("n", ROWS)
def test_decoder_module_backward(cuda, n):
    d = 385
    p = orc.randomize_biases(orc.init_decoder("IEF", d, 31, 5.0), 32)
    m = make_module("IEF", p, d, cuda).train()
    _assert_plans(n)
    gen = torch.Generator().manual_seed(n)
    x = torch.randn(n, d, generator=gen).to(cuda)
    w = _masked_weights(p, x, "IEF", n, gen, cuda)
    for q in m.parameters():
        q.grad = None
    xg = x.clone().requires_grad_(True)
    (m(xg).reshape(-1) * w).sum().backward()
    got = {k: q.grad for k, q in m.named_parameters()}
    got["input"] = xg.grad
    _, g64 = oracle_grads(p, x, "IEF", w, torch.float64)
    _, g32 = oracle_grads(p, x, "IEF", w, torch.float32)
    for k in g64:
        assert_f64_close("IEF n=%d d%s" % (n, k), got[k], g64[k], g32[k], k=_k(k))


@pytest.mark.parametrize("n", ROWS)
def test_decoder_pair_node_backward(cuda, n):
    """decoders_forward_train: both decoders as one autograd node, the rows' gradient one product over both."""
    from implicit_depth_amd import decoders_forward_train
    d = 385
    pp = orc.randomize_biases(orc.init_decoder("IMNET", d, 21, 5.0), 22)
    po = orc.randomize_biases(orc.init_decoder("IEF", d, 23, 5.0), 24)
    prob = make_module("IMNET", pp, d, cuda).train()
    off = make_module("IEF", po, d, cuda).train()
    _assert_plans(n)
    gen = torch.Generator().manual_seed(n + d)
    x = torch.randn(n, d, generator=gen).to(cuda)
    wp = _masked_weights(pp, x, "IMNET", n, gen, cuda)
    wo = _masked_weights(po, x, "IEF", n, gen, cuda)
    xg = x.clone().requires_grad_(True)
    yp, yo = decoders_forward_train(xg, prob, off)
    ((yp.reshape(-1) * wp).sum() + (yo.reshape(-1) * wo).sum()).backward()
    refs = {}
    for dt in (torch.float64, torch.float32):
        yp_r, gp = oracle_grads(pp, x, "IMNET", wp, dt)
        yo_r, go = oracle_grads(po, x, "IEF", wo, dt)
        g = {"prob." + k: v for k, v in gp.items() if k != "input"}
        g.update({"off." + k: v for k, v in go.items() if k != "input"})
        g["input"] = gp["input"] + go["input"]
        refs[dt] = (yp_r, yo_r, g)
        del gp, go
    _check_decoder_out("pair n=%d prob" % n, yp.detach(), refs[torch.float64][0], refs[torch.float32][0], False)
    _check_decoder_out("pair n=%d off" % n, yo.detach(), refs[torch.float64][1], refs[torch.float32][1], False)
    got = {"prob." + k: q.grad for k, q in prob.named_parameters()}
    got.update({"off." + k: q.grad for k, q in off.named_parameters()})
    got["input"] = xg.grad
    for k in refs[torch.float64][2]:
        assert_f64_close("pair n=%d d%s" % (n, k), got[k], refs[torch.float64][2][k], refs[torch.float32][2][k],
                         k=_k(k))


# ---------------------------------------------------------------------------------------------------------------
# the query: forward
# ---------------------------------------------------------------------------------------------------------------
def _oracle_query_on(scene, dev, dt, max_pair_id, **kw):
    s = to_dev(scene, dev)
    c = lambda v: v.to(dt)  # noqa: E731
    return orc.query(c(s["ray_dir"]), s["ray_pix"], s["ray_bid"], s["pair_ray"].long(), s["pair_vox"].long(),
                     c(s["pair_t"]), s["pair_off"], c(s["feat_grid"]), c(s["vox_feat"]), _dev(scene["prob_p"], dev, dt),
                     _dev(scene["off_p"], dev, dt), fast_roi=True, max_pair_id=max_pair_id, **kw)


def _check_query(scene, cuda, **kw):
    got = run_query(scene, cuda, **kw)
    mid = got["max_pair_id"].long()
    r64 = _oracle_query_on(scene, cuda, torch.float64, mid)
    r32 = _oracle_query_on(scene, cuda, torch.float32, mid)
    for k in ("pred_offset", "pred_prob_end"):
        assert_f64_close(k + " logit", inv_out_act(got[k]), inv_out_act(r64[k]), inv_out_act(r32[k]))
    for k in ("pair_pred_pos", "pred_pos", "pred_prob_end_softmax"):
        assert_f64_close(k, got[k], r64[k], r32[k])
    check_selection(scene, got, r64, r32)


@pytest.mark.parametrize("ragged", [False, True])
def test_query_config0_whole_frame(cuda, ragged):
    _check_query(orc.synthetic_scene(1, 64, 64, 16, seed=1234, ragged=ragged), cuda)


def test_query_full_size_ragged_whole_frame(cuda):
    """240x320 rays with 0-64 candidates each (P ~ 2.46 M), the whole frame."""
    scene = orc.synthetic_scene(1, 240, 320, 64, seed=4321, ragged=True)
    assert scene["P"] > 2_000_000
    _check_query(scene, cuda)


# ---------------------------------------------------------------------------------------------------------------
# the query: training (the reference's loss structure, as bench.py --workload train-query, plus dense terms)
# ---------------------------------------------------------------------------------------------------------------
def _query_rows(scene, dev):
    """The float64 decoder input rows of orc.query, from the oracle itself (its rows list), for the kink mask."""
    rows = []
    with torch.no_grad():
        _oracle_query_on(scene, dev, torch.float64, torch.zeros(scene["R"], dtype=torch.long, device=dev), rows=rows)
    return torch.cat(rows, 0)


@pytest.mark.parametrize("B,h,w,N,factorised,offsets", [
    (1, 64, 96, 8, True, "all"), (1, 64, 96, 8, False, "all"),                 # 49,152 pairs
    (1, 240, 320, 8, True, "all"), (1, 240, 320, 8, True, "selected"),        # the train-query record shape
    (1, 240, 320, 8, False, "all")])
def test_query_train_gradients(cuda, B, h, w, N, factorised, offsets):
    from implicit_depth_amd.query import lidf_query_train
    scene = orc.synthetic_scene(B, h, w, N, seed=1235)
    R, P, D = scene["R"], scene["P"], scene["D"]
    s = to_dev(scene, cuda)
    gen = torch.Generator().manual_seed(99)
    gt_pos = (torch.rand(R, 3, generator=gen) * 2 - 1).to(cuda)
    label = torch.randint(0, N, (R, 1), generator=gen).to(cuda)
    w_off = torch.randn(P, generator=gen).to(cuda) * 1e-3
    # kink rows of both decoders (float64 rows): zero upstream gradient on both sides
    with torch.no_grad():
        rows = _query_rows(scene, cuda)
        bad_p = kink_rows(_dev(scene["prob_p"], cuda, torch.float64), rows, "IMNET")
        bad_o = kink_rows(_dev(scene["off_p"], cuda, torch.float64), rows, "IEF")
        del rows
    print("masked rows: prob %d, offset %d of %d" % (int(bad_p.sum()), int(bad_o.sum()), P))
    assert bad_p.float().mean().item() < 0.01 and bad_o.float().mean().item() < 0.01

    def loss(o, wr):
        l = o["pred_prob_end"][:, 0]
        l = torch.where(bad_p, l.detach(), l)
        lsm = torch.log_softmax(l.view(-1, N), dim=1)
        po = torch.where(bad_o, o["pred_offset"][:, 0].detach(), o["pred_offset"][:, 0])
        return (((o["pred_pos"] - gt_pos.to(l.dtype)).abs() * wr[:, None]).mean() - lsm.gather(1, label).mean()
                + (po * w_off.to(l.dtype)).sum())

    prob = make_module("IMNET", scene["prob_p"], D, cuda).train()
    off = make_module("IEF", scene["off_p"], D, cuda).train()
    fg = s["feat_grid"].clone().requires_grad_(True)
    vf = s["vox_feat"].clone().requires_grad_(True)
    out = lidf_query_train(s["ray_dir"], s["ray_pix"], s["ray_bid"], s["pair_off"], s["pair_ray"], s["pair_vox"],
                           s["pair_t"], fg, vf, prob, off, factorised=factorised, offsets=offsets)
    mid = out["max_pair_id"].long()
    wr = (~bad_o[mid]).to(torch.float32)          # a ray whose selected pair sits at a kink: no position loss
    if offsets == "selected":                     # pred_offset exists at the selected pairs only
        w_off.zero_()
    loss(out, wr).backward()
    got = {"feat_grid": fg.grad, "vox_feat": vf.grad}
    got.update({"prob." + k: q.grad for k, q in prob.named_parameters()})
    got.update({"off." + k: q.grad for k, q in off.named_parameters()})
    refs = {}
    for dt in (torch.float64, torch.float32):
        pp = {k: v.to(cuda, dt, copy=True).requires_grad_(True) for k, v in scene["prob_p"].items()}
        pq = {k: v.to(cuda, dt, copy=True).requires_grad_(True) for k, v in scene["off_p"].items()}
        fr = s["feat_grid"].to(dt, copy=True).requires_grad_(True)
        vr = s["vox_feat"].to(dt, copy=True).requires_grad_(True)
        ref = orc.query(s["ray_dir"].to(dt), s["ray_pix"], s["ray_bid"], s["pair_ray"].long(), s["pair_vox"].long(),
                        s["pair_t"].to(dt), s["pair_off"], fr, vr, pp, pq, fast_roi=True, max_pair_id=mid)
        loss(ref, wr.to(dt)).backward()
        g = {"feat_grid": fr.grad, "vox_feat": vr.grad}
        g.update({"prob." + k: v.grad for k, v in pp.items()})
        g.update({"off." + k: v.grad for k, v in pq.items()})
        refs[dt] = (g, {k: ref[k].detach() for k in ("pred_prob_end", "pred_pos")})
        del ref
    tag = "%dx%dx%d %s %s" % (h, w, N, "factorised" if factorised else "rows", offsets)
    assert_f64_close(tag + " pred_prob_end logit", inv_out_act(out["pred_prob_end"]),
                     inv_out_act(refs[torch.float64][1]["pred_prob_end"]),
                     inv_out_act(refs[torch.float32][1]["pred_prob_end"]))
    assert_f64_close(tag + " pred_pos", out["pred_pos"], refs[torch.float64][1]["pred_pos"],
                     refs[torch.float32][1]["pred_pos"])
    for k in refs[torch.float64][0]:
        assert_f64_close("%s d%s" % (tag, k), got[k], refs[torch.float64][0][k], refs[torch.float32][0][k], k=_k(k))


# ---------------------------------------------------------------------------------------------------------------
# PointNet inference, below and above the LDS pooling table's 288 voxels
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,V", [(20000, 200), (70000, 1000)])
def test_pointnet_forward(cuda, n, V):
    p = orc.init_pointnet(3, 1.5)
    gen = torch.Generator().manual_seed(V)
    inp = torch.randn(n, 6, generator=gen).to(cuda)
    vox = torch.randint(0, V, (n,), generator=gen).to(cuda)
    with torch.no_grad():
        got = make_pointnet(p, cuda)(inp, vox, V)
        r64 = orc.pointnet2stage(_dev(p, cuda, torch.float64), inp.double(), vox, V)
        r32 = orc.pointnet2stage(_dev(p, cuda, torch.float32), inp, vox, V)
    assert_f64_close("pointnet n=%d V=%d" % (n, V), got, r64, r32)
