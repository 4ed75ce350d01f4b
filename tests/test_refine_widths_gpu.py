"""Stage-2 training at widths other than the shipped configuration: generic.refine_train behind
query.lidf_refine_train, the two per-ray entries (lidf_refine_step_forward_f32 / _backward_f32) and the whole step,
held to float64 / float32 autograd through the oracle (tests/refine_widths_ref.py; util.assert_f64_close)."""
import gc
import zlib

import pytest
import torch

import pointnet_ref as ref
import refine_widths_ref as rw
import stream_order as so
import ws_poison
from entry_cases import Entry, same
from test_f64_stage2_gpu import REFINE_KEYS, _check_all
from util import assert_f64_close, orc, tf32_off

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _full_precision_references():
    with tf32_off():
        yield
    gc.collect()
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------------
# the whole route
# ------------------------------------------------------------------------------------------------------------------
def _modules(case, dev, use_sigmoid=False):
    from implicit_depth_amd import IEF, IMNet, PointNet2Stage
    _, _, pnet_out, pnet_gf, gf, kind, n_iter, _, _ = case["cfg"]
    D = rw.inp_dim(case["cfg"])
    pnet = PointNet2Stage(6, pnet_out, pnet_gf)
    dec = IEF(dev, D, 1, gf, n_iter=n_iter, use_sigmoid=use_sigmoid) if kind == "IEF" else \
        IMNet(D, 1, gf, use_sigmoid=use_sigmoid)
    pnet.load_state_dict({k: v.clone() for k, v in case["pnet_p"].items()})
    dec.load_state_dict({k: v.clone() for k, v in case["off_p"].items()})
    return pnet.to(dev).train(), dec.to(dev).train()


def _step(case, t, pnet, dec, forward_times, pos_rel, pnet_pos_rel, w, **kw):
    """One forward + backward of lidf_refine_train on the live tensors t: {leaf: gradient, "pos", "end_voxel"}."""
    from implicit_depth_amd.query import lidf_refine_train
    _, roi_out, _, _, _, _, _, Lm, Lv = case["cfg"]
    for m in (pnet, dec):
        for q in m.parameters():
            q.grad = None
    pp = t["pred_pos"].detach().clone().requires_grad_(True)
    fg = t["feat_grid"].detach().clone().requires_grad_(True)
    args = [pp if k == "pred_pos" else fg if k == "feat_grid" else t[k] for k in REFINE_KEYS]
    pos, ev = lidf_refine_train(*args, pnet, dec, forward_times=forward_times, multires=Lm, multires_views=Lv,
                                roi_out_bbox=roi_out, pos_rel=pos_rel, pnet_pos_rel=pnet_pos_rel,
                                perturb_noise=case["noise"], **kw)
    (pos * w).sum().backward()
    got = {"pnet." + k: q.grad for k, q in pnet.named_parameters()}
    got.update({"dec." + k: q.grad for k, q in dec.named_parameters()})
    got.update({"pred_pos": pp.grad, "feat_grid": fg.grad, "pos": pos.detach(), "end_voxel": ev})
    return got


def _hold(cuda, cfg, forward_times, pos_rel, pnet_pos_rel, use_sigmoid=False, use_grid=False, **kw):
    case, keep_ray, keep_valid, _ = rw.conditioned(cfg, pos_rel, pnet_pos_rel, use_sigmoid)
    (p64, e64, g64), (p32, e32, g32) = rw.refs(cfg, forward_times, pos_rel, pnet_pos_rel, use_sigmoid)
    assert torch.equal(e64, e32)
    t = {k: case[k].to(cuda) for k in REFINE_KEYS}
    pnet, dec = _modules(case, cuda, use_sigmoid)
    if use_grid:
        kw["grid"] = dict(case["grid"], voxel_coord=case["grid"]["voxel_coord"].to(cuda))
    got = _step(case, t, pnet, dec, forward_times, pos_rel, pnet_pos_rel, rw.upstream(case).to(cuda), **kw)
    assert torch.equal(got.pop("end_voxel").cpu().long(), e64)
    assert all(v is not None for v in got.values())
    tag = "refine_train %s x%d%s%s%s %s" % (rw.cfg_id(cfg), forward_times, " pos_rel" if pos_rel else "",
                                             " grid" if use_grid else "", " sigmoid" if use_sigmoid else "", kw.get("factorised"))
    _check_all(tag, got, dict(g64, pos=p64), dict(g32, pos=p32))


@pytest.mark.parametrize("forward_times", [1, 2])
@pytest.mark.parametrize("pos_rel,pnet_pos_rel", rw.SETTINGS)
@pytest.mark.parametrize("cfg", rw.NEW_ONLY, ids=rw.cfg_id)
def test_refine_train_at_other_widths(cuda, cfg, pos_rel, pnet_pos_rel, forward_times):
    """Positions, end voxels (equal) and the gradient of every PointNet and decoder parameter, of pred_pos and of
    feat_grid against the float64 / float32 chain. factorised=None: configurations 1-3 have no other route; 4 and 5
    (gf_dim 128 / pnet_out 256) — 4 is served by the composed path by default, so the route is named."""
    _hold(cuda, cfg, forward_times, pos_rel, pnet_pos_rel, factorised=True if cfg[:3] == (32, 2, 128) else None)


def test_refine_train_through_the_cell_table(cuda):
    _hold(cuda, rw.CONFIGS[0], 2, False, True, use_grid=True)


@pytest.mark.parametrize("route", ["today", "factorised"])
@pytest.mark.parametrize("cfg", rw.BOTH_ROUTES + [rw.SHIPPED], ids=rw.cfg_id)
def test_configurations_both_routes_take(cuda, cfg, route):
    """Today's route (composed; the fused node for the shipped configuration) and generic.refine_train under
    factorised=True, both held to the same references."""
    _hold(cuda, cfg, 2, False, True, factorised=True if route == "factorised" else None)


def test_refine_train_use_sigmoid(cuda):
    _hold(cuda, rw.CONFIGS[0], 2, False, True, use_sigmoid=True)


def test_two_identical_steps_give_the_same_bits(cuda):
    cfg = rw.CONFIGS[0]
    case = rw.conditioned(cfg)[0]
    flat = (case["ray_bid"].long() * 20 + case["ray_pix"][:, 1].long()) * 24 + case["ray_pix"][:, 0].long()
    assert torch.unique(flat).numel() == flat.numel()            # the scene's rays are distinct pixels
    t = {k: case[k].to(cuda) for k in REFINE_KEYS}
    pnet, dec = _modules(case, cuda)
    w = rw.upstream(case).to(cuda)
    first = _step(case, t, pnet, dec, 2, False, True, w)
    second = _step(case, t, pnet, dec, 2, False, True, w)
    for k in first:
        assert first[k] is not None and torch.equal(first[k], second[k]), k + ": a second identical step differs"


def test_whole_refine_step_at_other_widths(cuda):
    """pipeline.train_refine_step with rgb_out 16 / roi_out_bbox 3 / pnet_out 64 / pnet_gf 16 / gf_dim 32 in both
    stages: finite, non-zero, repeatable."""
    import numpy as np
    from implicit_depth_amd import IEF, IMNet, LidfOptions, PointNet2Stage
    from implicit_depth_amd.pipeline import train_refine_step
    from implicit_depth_amd.synthetic import synthetic_batch
    from test_train_widths_gpu import _pointnet_params
    Cr, Co, gf = 16, 64, 32
    D1, D2 = Co + Cr * 9 + 2 * 51 + 27, Co + Cr * 9 + 51 + 27
    batch, feat = synthetic_batch(2, 24, 32, seed=31)
    batch = {k: (v.to(cuda) if torch.is_tensor(v) else v) for k, v in batch.items()}
    pnet, pnet_r = PointNet2Stage(6, Co, 16), PointNet2Stage(6, Co, 16)
    pnet.load_state_dict(_pointnet_params(6, Co, 16, 3)), pnet_r.load_state_dict(_pointnet_params(6, Co, 16, 5))
    prob, off, off_r = IMNet(D1, 1, gf), IEF(cuda, D1, 1, gf, n_iter=2), IEF(cuda, D2, 1, gf, n_iter=2)
    prob.load_state_dict(orc.init_decoder("IMNET", D1, 7, 5.0, gf=gf))
    off.load_state_dict(orc.init_decoder("IEF", D1, 8, 5.0, gf=gf))
    off_r.load_state_dict(orc.randomize_biases(orc.init_decoder("IEF", D2, 77, 5.0, gf=gf), 78))
    frozen = [m.to(cuda).eval() for m in (pnet, prob, off)]
    mods = [m.to(cuda).train() for m in (pnet_r, off_r)]
    opt = LidfOptions(roi_out_bbox=3, miss_sample_num=-1, maxpool_label_epo=0)

    def step():
        for m in mods:
            for q in m.parameters():
                q.grad = None
        np.random.seed(77)
        ok, dd, _, loss = train_refine_step(batch, feat[:, :Cr].contiguous().to(cuda), *frozen, *mods, opt=opt)
        assert ok and bool(torch.isfinite(loss["loss_net"]))
        loss["loss_net"].backward()
        torch.cuda.synchronize()
        return {"m%d.%s" % (i, n): q.grad for i, m in enumerate(mods) for n, q in m.named_parameters()}, dd

    first, dd = step()
    assert dd["pred_pos_refine"].shape == dd["pred_pos"].shape and bool(torch.isfinite(dd["pred_pos_refine"]).all())
    for k, g in first.items():
        assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0.0, k
    second, _ = step()
    for k in first:
        assert torch.equal(first[k], second[k]), k + ": a second identical step differs"


# ------------------------------------------------------------------------------------------------------------------
# routing and refusals
# ------------------------------------------------------------------------------------------------------------------
def _call(cuda, cfg, pnet=None, dec=None, **kw):
    from implicit_depth_amd.query import lidf_refine_train
    case = rw.widths_case(cfg)
    t = {k: case[k].to(cuda) for k in REFINE_KEYS}
    mp, md = _modules(case, cuda)
    kw.setdefault("roi_out_bbox", cfg[1])
    return lidf_refine_train(*[t[k] for k in REFINE_KEYS], pnet or mp, dec or md, forward_times=1, multires=cfg[7],
                             multires_views=cfg[8], **kw)


def test_routing(cuda, monkeypatch):
    from implicit_depth_amd import generic, query
    entered = []
    real_generic, real_composed = generic.refine_train, query._lidf_refine_train_composed
    monkeypatch.setattr(generic, "refine_train", lambda *a, **k: entered.append("generic") or real_generic(*a, **k))
    monkeypatch.setattr(query, "_lidf_refine_train_composed",
                        lambda *a, **k: entered.append("composed") or real_composed(*a, **k))
    _call(cuda, rw.SHIPPED)                          # the fused node: neither
    _call(cuda, rw.SHIPPED, factorised=False)
    assert entered == []
    for cfg in rw.BOTH_ROUTES:
        _call(cuda, cfg)
        _call(cuda, cfg, factorised=False)
    assert entered == ["composed"] * (2 * len(rw.BOTH_ROUTES))
    del entered[:]
    for cfg in (rw.SHIPPED, rw.BOTH_ROUTES[0], rw.NEW_ONLY[0]):
        _call(cuda, cfg, factorised=True)
    _call(cuda, rw.NEW_ONLY[0])
    _call(cuda, rw.NEW_ONLY[4])                      # pnet_out 256 at rgb_out 32 / roi_out_bbox 2
    assert entered == ["generic"] * 5
    del entered[:]
    with pytest.raises(RuntimeError):                # factorised=False never takes it: today's refusal
        _call(cuda, rw.NEW_ONLY[0], factorised=False)
    assert "generic" not in entered


def test_refusals(cuda):
    from implicit_depth_amd import IEF, IMNet, PointNet2Stage
    cfg = rw.NEW_ONLY[0]
    D = rw.inp_dim(cfg)
    with pytest.raises(RuntimeError, match="out_dim == 1"):
        _call(cuda, cfg, dec=IMNet(D, 2, 32).to(cuda).train())
    with pytest.raises(RuntimeError, match="input_channels must be 6"):
        _call(cuda, cfg, pnet=PointNet2Stage(7, 64, 16).to(cuda).train())
    with pytest.raises(RuntimeError, match="inp_dim must be %d" % (D - 16 * 9 + 16 * 4)):
        _call(cuda, cfg, roi_out_bbox=2)
    with pytest.raises(RuntimeError, match="inp_dim must be %d" % D):
        _call(cuda, cfg, dec=IEF(cuda, D + 1, 1, 32).to(cuda).train())


def test_no_rays_still_carry_a_graph(cuda):
    from implicit_depth_amd.query import lidf_refine_train
    cfg = rw.NEW_ONLY[0]
    case = rw.widths_case(cfg)
    t = {k: case[k].to(cuda) for k in REFINE_KEYS}
    for k in ref.RAY_KEYS:
        t[k] = t[k][:0].contiguous()
    pnet, dec = _modules(case, cuda)
    pos, ev = lidf_refine_train(*[t[k] for k in REFINE_KEYS], pnet, dec, multires=cfg[7], multires_views=cfg[8],
                                roi_out_bbox=cfg[1])
    assert pos.shape == (0, 3) and ev.shape == (0,) and ev.dtype == torch.int32 and pos.requires_grad
    pos.sum().backward()
    assert all(q.grad is not None and not bool(q.grad.any()) for m in (pnet, dec) for q in m.parameters())


# ------------------------------------------------------------------------------------------------------------------
# the two entries alone
# ------------------------------------------------------------------------------------------------------------------
EMBED_TOL = 1e-6     # the embedder's bound against float64 (tests/test_edge_gpu.py): the matrix-free sin / cos of
#                      lidf_device.h are within 4.2e-7 of exact at every octave, the value itself is rounded once


def _ray_scene(R, seed):
    """R random rays on refine_case()'s voxel list (every cell of the 9 x 9 x 9 grid of two frames): positions inside
    and around the grid, arg-max pairs with every fifth ray on the dummy row, random pixels. Host tensors."""
    base = ref.refine_case()
    g = torch.Generator().manual_seed(seed)
    V, h, w, P, Nv = base["voxel_bound"].shape[0], 20, 24, 300, 37
    pos = torch.rand(R, 3, generator=g) * torch.tensor([2.6, 2.6, 2.6]) + torch.tensor([-1.3, -1.3, -0.3])
    mid = torch.randint(0, P, (R,), generator=g)
    mid[::5] = P
    return {"pos": pos.contiguous(), "max_pair_id": mid, "pair_vox": torch.randint(0, V, (P,), generator=g).int(),
            "voxel_bound": base["voxel_bound"], "voxel_bid": base["voxel_bid"],
            "ray_bid": torch.randint(0, 2, (R,), generator=g).int(),
            "ray_flat": torch.randint(0, h * w, (R,), generator=g).int(),
            "rgb_img": torch.randn(2, 3, h, w, generator=g), "ray_dir": torch.randn(R, 3, generator=g),
            "valid_inp": torch.randn(Nv, 6, generator=g), "valid_vox": torch.randint(0, V, (Nv,), generator=g).int(),
            "voxel_coord": base["grid"]["voxel_coord"], "g_pos": torch.randn(R, 3, generator=g),
            "d_rows": torch.randn(Nv + R, 6, generator=g)}


def _constants(s, L_, pos_rel, pnet_pos_rel, use_grid):
    from implicit_depth_amd.query import _cell_lookup
    base = ref.refine_case()
    st = {k: s[k] for k in ("max_pair_id", "pair_vox", "voxel_bound", "voxel_bid", "ray_bid", "ray_flat", "rgb_img",
                            "ray_dir", "valid_inp", "valid_vox")}
    st.update(multires=L_, pos_rel=pos_rel, pnet_pos_rel=pnet_pos_rel, offset_range=(-0.2, 0.3), cells=None)
    if use_grid:
        st["cells"] = _cell_lookup(dict(base["grid"], voxel_coord=s["voxel_coord"]), s["voxel_bound"].shape[0], 2,
                                   s["pos"].device, s["voxel_bound"])
    return st


def _forward_wide(s, st, pad, misalign=0):
    """The forward entry with pe at a row stride of E + pad (NaN behind the E columns), its base `misalign` floats off a
    16-byte boundary: the pe block [R, E] and the whole buffer."""
    from implicit_depth_amd import _lib
    dev = s["pos"].device
    R, Nv, E = s["pos"].shape[0], s["valid_inp"].shape[0], 3 + 6 * st["multires"]
    buf = torch.full((R * (E + pad) + 4,), float("nan"), device=dev)
    pe = buf[misalign:misalign + R * (E + pad)].view(R, E + pad)
    pn_inp = torch.empty((Nv + R, 6), device=dev)
    pn_vox = torch.empty((Nv + R,), dtype=torch.int32, device=dev)
    ev = torch.empty((R,), dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().lidf_refine_step_forward_f32(
        _lib.ptr(s["pos"]), _lib.ptr(s["max_pair_id"]), _lib.ptr(s["pair_vox"]), s["pair_vox"].shape[0],
        _lib.ptr(s["voxel_bound"]), _lib.ptr(s["voxel_bid"]), s["voxel_bound"].shape[0], _lib.ptr(s["ray_bid"]),
        _lib.ptr(s["ray_flat"]), _lib.ptr(s["rgb_img"]), 2, 20, 24, R, Nv, 1 if st["pnet_pos_rel"] else 0,
        1 if st["pos_rel"] else 0, st["multires"], None, None, None, 0.0, 0, _lib.ptr(ev), _lib.ptr(pn_inp),
        _lib.ptr(pn_vox), _lib.ptr(pe), E + pad, None, 0, _lib.current_stream(dev)))
    return pe, ev


def _entry_refs(s, L_, pos_rel, pnet_pos_rel, end, dt):
    """embed, PointNet rows and d_pos at dtype dt from the float32 operand x = pos (- centre): the operand is an
    input of the embedding (its rounding is the subtraction's, the same float32 operation on both sides)."""
    vb = s["voxel_bound"][end.long()]
    centre = (vb[:, :3] + vb[:, 3:]) / 2.0
    E = 3 + 6 * L_
    x = ((s["pos"] - centre) if pos_rel else s["pos"]).to(dt, copy=True).requires_grad_(True)
    rows = ((s["pos"] - centre) if pnet_pos_rel else s["pos"]).to(dt, copy=True).requires_grad_(True)
    pe = orc.embed(x, L_)
    Nv = s["valid_inp"].shape[0]
    d_pe = torch.randn(x.shape[0], E, generator=torch.Generator().manual_seed(E)).to(x.device)
    ((pe * d_pe.to(dt)).sum() + (rows * s["d_rows"][Nv:, :3].to(dt)).sum()).backward()
    d_pos = s["g_pos"].to(dt) + x.grad + rows.grad
    d_off = 0.5 * (s["g_pos"].to(dt) * s["ray_dir"].to(dt)).sum(1)
    return pe.detach(), rows.detach(), d_pos, d_off, d_pe


@pytest.mark.parametrize("L_", [0, 1, 8, 16])
@pytest.mark.parametrize("R", [1, 33, 129, 2049])
def test_step_entries(cuda, R, L_):
    from implicit_depth_amd import generic
    from implicit_depth_amd.extensions import pcl_aabb
    E = 3 + 6 * L_
    for pos_rel, pnet_pos_rel in rw.SETTINGS:
        s = {k: v.to(cuda) for k, v in _ray_scene(R, 100 * R + L_).items()}
        Nv = s["valid_inp"].shape[0]
        st = _constants(s, L_, pos_rel, pnet_pos_rel, False)
        ev, pn_inp, pn_vox, pe = generic.refine_step_forward(s["pos"], st)
        # end voxels: max(the arg-max pair's voxel, the last containing voxel), the dummy row -> voxel 0
        P = s["pair_vox"].shape[0]
        first = torch.cat((s["pair_vox"].long(), torch.zeros(1, dtype=torch.long, device=cuda)))[s["max_pair_id"]]
        assert int((s["max_pair_id"] == P).sum()) >= 1
        last = pcl_aabb.last_voxel(s["pos"], s["voxel_bound"], s["ray_bid"], s["voxel_bid"]).long()
        want = torch.maximum(first, last)
        assert torch.equal(ev.long(), want)
        assert R < 129 or (bool((last > first).any()) and bool((last < 0).any()))
        # the cell table gives the same, twice (the second call reuses the table)
        stg = _constants(s, L_, pos_rel, pnet_pos_rel, True)
        for ready in (False, True):
            ev_g, pn_g, pv_g, pe_g = generic.refine_step_forward(s["pos"], stg, ready)
            assert torch.equal(ev_g, ev) and torch.equal(pn_g, pn_inp) and torch.equal(pv_g, pn_vox)
            assert torch.equal(pe_g, pe)
        # the rows behind the valid points, the valid points in front
        assert torch.equal(pn_inp[:Nv], s["valid_inp"]) and torch.equal(pn_vox[:Nv], s["valid_vox"])
        assert torch.equal(pn_vox[Nv:], ev)
        r64, r32 = (_entry_refs(s, L_, pos_rel, pnet_pos_rel, ev, dt) for dt in (torch.float64, torch.float32))
        assert torch.equal(pn_inp[Nv:, :3], r32[1])                     # one float32 subtraction: the same bits
        rgb = s["rgb_img"].permute(0, 2, 3, 1).reshape(-1, 3)[s["ray_bid"].long() * 480 + s["ray_flat"].long()]
        assert torch.equal(pn_inp[Nv:, 3:], rgb)
        err = float((pe.double() - r64[0]).abs().max())
        print("R=%d L=%d%s: embed max error against float64 %.3g" % (R, L_, " pos_rel" if pos_rel else "", err))
        assert pe.shape == (R, E) and err <= EMBED_TOL and torch.equal(pe[:, :3], r32[0][:, :3])
        # a row stride wider than E (aligned rows: 16-byte pieces; odd and off a 16-byte boundary: single stores)
        for pad, mis in ((1, 0), (5, 0), (2, 1), (0, 1)):
            wide, ev_w = _forward_wide(s, st, pad, mis)
            assert torch.equal(wide[:, :E], pe) and torch.equal(ev_w, ev), (pad, mis)
            assert bool(torch.isnan(wide[:, E:]).all())                 # nothing is written behind a row's E columns
        # backward
        d_pe = r64[4]
        d_off, d_pos = generic.refine_step_backward(s["g_pos"], st, d_off=True, pos=s["pos"], end_voxel=ev, d_pe=d_pe,
                                                    d_rows=s["d_rows"], d_pos=True)
        tag = "step backward R=%d L=%d%s" % (R, L_, " pos_rel" if pos_rel else "")
        assert_f64_close(tag + " d_pos", d_pos, r64[2], r32[2])
        assert_f64_close(tag + " d_off", d_off, r64[3], r32[3])
        only_off, none = generic.refine_step_backward(s["g_pos"], st, d_off=True)
        assert none is None and torch.equal(only_off, d_off)
        _, plain = generic.refine_step_backward(s["g_pos"], st, d_pos=True)
        assert torch.equal(plain, s["g_pos"])                           # neither term: the pass-through alone


# ------------------------------------------------------------------------------------------------------------------
# the library's standing contracts: arbitrary workspace contents, the caller's stream
# ------------------------------------------------------------------------------------------------------------------
def entry_refine_train_widths(dev):
    """generic.refine_train at (16, 3, 64, 16, 32, IEF) through the cell table, forward + backward, held to float64."""
    cfg = rw.CONFIGS[0]
    case = rw.conditioned(cfg)[0]
    pnet, dec = _modules(case, dev)
    coord = case["grid"]["voxel_coord"]

    def call(live):
        grid = dict(case["grid"], voxel_coord=live["voxel_coord"])
        got = _step(case, live, pnet, dec, 2, False, True, live["w"], grid=grid)
        return {k: v for k, v in got.items() if v is not None}

    def check(got):
        with tf32_off():
            (p64, e64, g64), (p32, e32, g32) = rw.refs(cfg, 2)
        got = dict(got)
        assert torch.equal(got.pop("end_voxel").cpu().long(), e64)
        _check_all("entry refine_train", got, dict(g64, pos=p64), dict(g32, pos=p32))

    inputs = {k: case[k] for k in REFINE_KEYS}
    inputs.update(voxel_coord=coord, w=rw.upstream(case))
    return Entry(inputs, call, check, modules=(pnet, dec))


def _step_entry(dev, backward):
    R, L_ = 2049, 8
    s = _ray_scene(R, 7)

    def call(live):
        from implicit_depth_amd import generic
        st = _constants(live, L_, True, True, True)
        ev, pn_inp, pn_vox, pe = generic.refine_step_forward(live["pos"], st)
        if not backward:
            return {"end_voxel": ev, "pnet_inp": pn_inp, "pnet_vox": pn_vox, "pe": pe}
        d_off, d_pos = generic.refine_step_backward(live["g_pos"], st, d_off=True, pos=live["pos"], end_voxel=ev,
                                                    d_pe=live["d_pe"], d_rows=live["d_rows"], d_pos=True)
        return {"d_off": d_off, "d_pos": d_pos}

    def check(got):
        from implicit_depth_amd.extensions import pcl_aabb
        sd = {k: v.to(dev) for k, v in s.items()}
        first = torch.cat((sd["pair_vox"].long(), torch.zeros(1, dtype=torch.long, device=dev)))[sd["max_pair_id"]]
        ev = torch.maximum(first, pcl_aabb.last_voxel(sd["pos"], sd["voxel_bound"], sd["ray_bid"],
                                                      sd["voxel_bid"]).long())
        r64, r32 = (_entry_refs(sd, L_, True, True, ev, dt) for dt in (torch.float64, torch.float32))
        if backward:
            assert_f64_close("entry step backward d_pos", got["d_pos"], r64[2], r32[2])
            assert_f64_close("entry step backward d_off", got["d_off"], r64[3], r32[3])
            return
        Nv = sd["valid_inp"].shape[0]
        assert torch.equal(got["end_voxel"].long(), ev) and torch.equal(got["pnet_vox"][Nv:].long(), ev)
        assert torch.equal(got["pnet_inp"][Nv:, :3], r32[1]) and torch.equal(got["pnet_inp"][:Nv], sd["valid_inp"])
        assert float((got["pe"].double() - r64[0]).abs().max()) <= EMBED_TOL

    inputs = dict(s)
    inputs["d_pe"] = torch.randn(R, 3 + 6 * L_, generator=torch.Generator().manual_seed(3 + 6 * L_))
    return Entry(inputs, call, check)


ENTRIES = {"refine_train_widths": entry_refine_train_widths,
           "refine_step_forward": lambda dev: _step_entry(dev, False),
           "refine_step_backward": lambda dev: _step_entry(dev, True)}


@pytest.mark.parametrize("name", list(ENTRIES))
def test_workspace_contents_do_not_matter(cuda, monkeypatch, request, name):
    """Zero-filled workspaces, then the four poisons of ws_poison: bit-equal results."""
    with tf32_off():
        poison = ws_poison.Poisoner("zeros", seed=zlib.crc32(request.node.nodeid.encode())).install(monkeypatch)
        entry = ENTRIES[name](cuda)
        live = {k: v.to(cuda).contiguous() for k, v in entry.inputs.items()}

        def run():
            out = so.tree_map(lambda t: t.detach().clone(), entry.call(live))
            torch.cuda.synchronize()
            return out
        assert ws_poison.MODES[0] == "zeros" and len(ws_poison.MODES) == 5
        poison.begin("zeros")
        base = run()
        assert poison.handed, "the entry took no workspace from _lib.workspace"
        entry.check(base)
        for mode in ws_poison.MODES[1:]:
            if mode == "replay":
                poison.begin("zeros")
                run()
                assert poison.snapshot()
            poison.begin(mode)
            same(run(), base, "%s [%s]" % (name, mode))


@pytest.mark.parametrize("name", list(ENTRIES))
def test_caller_stream_with_late_inputs(cuda, monkeypatch, name):
    with tf32_off():
        rec = so.Recorder().install(monkeypatch)
        entry = ENTRIES[name](cuda)
        base = so.baseline(entry, cuda)
        entry.check(base)
        host_ms, fresh = so.enqueue_ms(entry, cuda)
        so.compare(fresh, base, entry, name + " on a fresh stream, no delay")
        ms = so.delay_ms(host_ms, name, "late inputs")
        got, running = so.late_inputs(entry, cuda, ms, rec)
        so.compare(got, base, entry, name + " with late inputs")
        assert running, "inconclusive: the %g ms delay had ended when the enqueue of %s returned" % (ms, name)
