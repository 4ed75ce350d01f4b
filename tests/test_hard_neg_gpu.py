"""GPU: hard-negative mining on the device — losses.topk_mean (csrc/lidf_select.hip) against the numpy twin of
tests/hard_neg_ref.py, exactly: the selected set, the weights' bits and the mean to one float32 rounding; then the
"device" route of lidf_loss / refine_loss against the float64 restatements, the fixtures and the torch route."""
import ctypes as C

import numpy as np
import pytest
import torch

import hard_neg_ref as hn
import refine_loss_ref as rl
import train_loss_ref as tl
from util import assert_f64_close

pytestmark = pytest.mark.gpu

# the smallest sizes at which a lane, wavefront, workgroup or slab (4096 values) boundary can go wrong; the shipped
# 8 x 20,000 rays; more than 2^20 values, odd
SIZES = [1, 9, 10, 63, 64, 65, 255, 256, 257, 1023, 1025, 4097, 160000, 1000003]


def _pattern(name, n):
    """float32 values of one pattern (numpy, seeded by the size)."""
    rng = np.random.default_rng(1000 + n)
    if name == "uniform":          # tie-free
        v = rng.permutation(n).astype(np.float32) / np.float32(max(n, 1)) - np.float32(0.25)
    elif name == "all_equal":      # the first k indices must win
        v = np.full(n, 0.375, dtype=np.float32)
    elif name == "five_values":    # ties straddle every slab boundary
        v = ((np.arange(n, dtype=np.int64) * 7919) % 5).astype(np.float32)
    elif name == "last_digit":     # the top 21+ bits shared: the last radix digit decides, with heavy ties
        v = (1.0 + rng.integers(0, 256, n) * 2.0 ** -23).astype(np.float32)
    elif name == "special":        # NaN of both signs, +-inf, +-0, denormals, negatives
        pool = np.array([np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-45, 3e-39, -2.5, 7.0, 1.5],
                        dtype=np.float32)
        # 4 % NaN, 3 % +inf, 5 % of 7.0: at ratio 0.1 the k-th place lies among the 7.0s, below the NaNs and +inf
        p = np.array([0.02, 0.02, 0.03, 0.11, 0.11, 0.11, 0.11, 0.11, 0.11, 0.11, 0.05, 0.11])
        v = pool[rng.choice(pool.shape[0], n, p=p / p.sum())]
    elif name == "signed_zeros":   # 5 % positive, 2 % positive denormals, 10 % of +-0 across the k-th place, negatives
        u = rng.random(n)
        v = -rng.random(n).astype(np.float32) - np.float32(0.5)
        v[u < 0.17] = np.where(rng.random(n) < 0.5, 0.0, -0.0).astype(np.float32)[u < 0.17]
        v[u < 0.07] = np.float32(3e-39)
        v[u < 0.05] = (rng.random(n).astype(np.float32) + np.float32(0.5))[u < 0.05]
    else:
        raise KeyError(name)
    return np.ascontiguousarray(v, dtype=np.float32)


def _check(got_mean, got_w, v, ratio, count=None, what=""):
    """The exact checks of one job against the twin."""
    ref = hn.topk_mean_ref(v, ratio, count)
    k = ref["k"]
    w = got_w.cpu().numpy()
    mean = float(got_mean)
    assert w.shape == v.shape and w.dtype == np.float32
    sel = np.nonzero(w)[0]
    assert sel.shape[0] == k, "%s: %d selected, k = %d" % (what, sel.shape[0], k)
    assert np.array_equal(sel, ref["sel"]), what
    assert np.array_equal(w.view(np.uint32), ref["weights"].view(np.uint32)), what   # 1 / k bit for bit, 0 as +0
    m64 = ref["mean64"]
    print("%s n %d k %d mean %r mean64 %r bound %.3g" % (what, v.shape[0], k, mean, m64, 2.0 ** -23 * ref["scale"]))
    if np.isnan(m64):
        assert np.isnan(mean), what
    elif np.isinf(m64):
        assert mean == m64, what
    else:
        # the double accumulation of fewer than 2^31 terms plus one rounding to float
        assert abs(mean - m64) <= 2.0 ** -23 * ref["scale"], (what, mean, m64)
    return ref


PATTERNS = ["uniform", "all_equal", "five_values", "last_digit", "special", "signed_zeros"]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", PATTERNS)
def test_patterns_against_the_twin(cuda, name, n):
    from implicit_depth_amd import topk_mean
    v = _pattern(name, n)
    mean, w = topk_mean(torch.from_numpy(v).to(cuda), 0.1)
    assert mean.dim() == 0 and mean.dtype == torch.float32 and w.dtype == torch.float32
    _check(mean, w, v, 0.1, what="%s" % name)


@pytest.mark.parametrize("ratio", [0.0, 1.0])
@pytest.mark.parametrize("name", PATTERNS)
def test_ratio_zero_and_one(cuda, name, ratio):
    from implicit_depth_amd import topk_mean
    v = _pattern(name, 257)
    mean, w = topk_mean(torch.from_numpy(v).to(cuda), ratio)
    ref = _check(mean, w, v, ratio, what="%s ratio %g" % (name, ratio))
    assert ref["k"] == (257 if ratio else 0)


@pytest.mark.parametrize("n", [10, 257, 4097, 160000, 1000003])
def test_prob_unreduced_lookalike_with_a_device_count(cuda, n):
    """-inf at about 80 % of the positions, k from the number of finite entries, which stays on the device."""
    from implicit_depth_amd import topk_mean
    rng = np.random.default_rng(n)
    v = (rng.random(n) * 9.0).astype(np.float32)
    v[rng.random(n) < 0.8] = -np.inf
    finite = int(np.isfinite(v).sum())
    cnt = torch.tensor(finite, dtype=torch.int32, device=cuda)
    mean, w = topk_mean(torch.from_numpy(v).to(cuda), 0.1, cnt)
    ref = _check(mean, w, v, 0.1, finite, what="prob look-alike")
    assert ref["k"] == int(finite * 0.1) and (ref["k"] == 0 or np.isfinite(v[ref["sel"]]).all())
    # count 0: a NaN mean and no weight, whatever the values
    zero = torch.zeros((1,), dtype=torch.int32, device=cuda)
    mean, w = topk_mean(torch.from_numpy(v).to(cuda), 0.1, zero)
    assert torch.isnan(mean) and not bool(w.any())


def test_no_value_at_all(cuda):
    """n == 0: a NaN mean (torch.mean of an empty tensor) and an empty weight vector."""
    from implicit_depth_amd import topk_mean
    mean, w = topk_mean(torch.empty((0,), device=cuda), 0.1)
    assert torch.isnan(mean) and tuple(w.shape) == (0,)
    mean, w = topk_mean(torch.empty((0,), device=cuda), 1.0, torch.zeros((), dtype=torch.int32, device=cuda))
    assert torch.isnan(mean) and tuple(w.shape) == (0,)


@pytest.mark.parametrize("ratio,k", [(0.29, 28), (0.57, 56)])
def test_k_is_a_double_product(cuda, ratio, k):
    from implicit_depth_amd import topk_mean
    v = _pattern("uniform", 100)
    mean, w = topk_mean(torch.from_numpy(v).to(cuda), ratio)
    assert int((w != 0).sum()) == k
    _check(mean, w, v, ratio, what="ratio %g" % ratio)
    cnt = torch.tensor([100], dtype=torch.int32, device=cuda)
    mean, w = topk_mean(torch.from_numpy(v).to(cuda), ratio, cnt)
    assert int((w != 0).sum()) == k


@pytest.mark.parametrize("off", [1, 2, 3])
@pytest.mark.parametrize("n", [1, 10, 257, 4093, 4097, 8192])
def test_values_off_the_16_byte_boundary(cuda, n, off):
    """An unaligned head and tail: the values start 4, 8 or 12 bytes past a 16-byte boundary."""
    from implicit_depth_amd import topk_mean
    v = _pattern("five_values", n)
    buf = torch.full((n + 8,), float("nan"), device=cuda)
    buf[off:off + n] = torch.from_numpy(v).to(cuda)
    view = buf[off:off + n]
    assert view.data_ptr() % 16 == 4 * off
    mean, w = topk_mean(view, 0.3)
    _check(mean, w, v, 0.3, what="offset %d" % off)


def _raw_jobs(cuda, specs, ratio):
    """One lidf_topk_mean_f32 call over `specs` = [(values tensor, count tensor or None, weights tensor or None)]:
    ([means], the weights as given)."""
    from implicit_depth_amd import _lib
    L = _lib.lib()
    means = torch.full((len(specs),), 123.0, device=cuda)
    jobs = (_lib.LidfTopkJob * len(specs))()
    for i, (v, cnt, w) in enumerate(specs):
        jobs[i] = _lib.LidfTopkJob(v.data_ptr(), v.shape[0], None if cnt is None else cnt.data_ptr(),
                                   means[i:].data_ptr(), None if w is None else w.data_ptr())
    wsb = L.lidf_topk_mean_workspace_bytes(len(specs), max(v.shape[0] for v, _, _ in specs))
    ws = _lib.workspace(wsb, cuda)
    with torch.cuda.device(cuda):
        _lib.check(L.lidf_topk_mean_f32(jobs, len(specs), ratio, _lib.ptr(ws), wsb, _lib.current_stream(cuda)))
    torch.cuda.synchronize(cuda)
    return means


def test_five_jobs_in_one_call(cuda):
    """Different n, one job without weights, one with a device count, one whose values and weights both start off
    the 16-byte boundary: bit-equal to five single-job calls, and from run to run."""
    ns = [1, 257, 4097, 10000, 65]
    pats = ["uniform", "five_values", "last_digit", "uniform", "signed_zeros"]
    vals = [_pattern(p, n) for p, n in zip(pats, ns)]
    vals[3][np.random.default_rng(5).random(ns[3]) < 0.8] = -np.inf
    counts = [None, None, None, int(np.isfinite(vals[3]).sum()), None]
    ratio = 0.3
    runs = []
    for _ in range(2):
        dv = [torch.from_numpy(v).to(cuda) for v in vals]
        shifted = torch.zeros((ns[1] + 4,), device=cuda)
        shifted[1:1 + ns[1]] = dv[1]
        dv[1] = shifted[1:1 + ns[1]]
        dc = [None if c is None else torch.tensor([c], dtype=torch.int32, device=cuda) for c in counts]
        wbuf = torch.full((ns[1] + 4,), 5.0, device=cuda)
        dw = [torch.full((n,), 5.0, device=cuda) for n in ns]
        dw[1] = wbuf[1:1 + ns[1]]
        dw[4] = None
        means = _raw_jobs(cuda, list(zip(dv, dc, dw)), ratio)
        assert float(wbuf[0]) == 5.0 and bool((wbuf[1 + ns[1]:] == 5.0).all())   # nothing beside the job's weights
        runs.append((means, dw))
    for i in range(5):
        assert torch.equal(runs[0][0][i], runs[1][0][i]) or (torch.isnan(runs[0][0][i]) and torch.isnan(runs[1][0][i]))
        if runs[0][1][i] is not None:
            assert torch.equal(runs[0][1][i], runs[1][1][i])
    from implicit_depth_amd import topk_mean
    for i in range(5):
        cnt = None if counts[i] is None else torch.tensor(counts[i], dtype=torch.int32, device=cuda)
        mean, w = topk_mean(torch.from_numpy(vals[i]).to(cuda), ratio, cnt)
        assert mean.view(torch.int32).item() == runs[0][0][i].view(torch.int32).item(), i
        if runs[0][1][i] is not None:
            assert torch.equal(w, runs[0][1][i]), i
            _check(mean, w, vals[i], ratio, counts[i], what="job %d" % i)


def test_graph_capture_and_replay(cuda):
    """One call with a device count captured on one stream; replayed on new values and a new count it gives what an
    eager call gives. That the capture succeeds is the evidence that nothing is read back."""
    from implicit_depth_amd import topk_mean
    n = 5000
    a, b = _pattern("uniform", n), _pattern("last_digit", n)
    vals = torch.from_numpy(a).to(cuda)
    cnt = torch.tensor([3000], dtype=torch.int32, device=cuda)
    topk_mean(vals, 0.1, cnt)                      # eager warm-up
    torch.cuda.synchronize(cuda)
    st = torch.cuda.Stream(cuda)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        mean, w = topk_mean(vals, 0.1, cnt)
    g.replay()
    torch.cuda.synchronize(cuda)
    _check(mean, w, a, 0.1, 3000, what="replay 1")
    vals.copy_(torch.from_numpy(b).to(cuda))
    cnt.fill_(4321)
    g.replay()
    torch.cuda.synchronize(cuda)
    _check(mean, w, b, 0.1, 4321, what="replay 2")
    mean2, w2 = topk_mean(vals.clone(), 0.1, cnt.clone())
    assert torch.equal(mean, mean2) and torch.equal(w, w2)


# ----------------------------------------------------------------------------------------------
# Through the losses
# ----------------------------------------------------------------------------------------------
def _refine_dd(d, dev):
    """refine_loss's data_dict from a restatement dict (pix2ray as compute_gt builds it, a fresh leaf)."""
    lin = d["miss_bid"] * (d["h"] * d["w"]) + d["miss_flat"]
    table = torch.full((d["bs"] * d["h"] * d["w"],), -1, dtype=torch.int32)
    table[lin] = torch.arange(lin.shape[0], dtype=torch.int32)
    return {"bs": d["bs"], "h": d["h"], "w": d["w"], "xyz_flat": d["xyz_flat"].to(dev),
            "ray_bid": d["miss_bid"].int().to(dev), "ray_flat": d["miss_flat"].int().to(dev),
            "gt_pos": d["gt_pos"].to(dev), "pix2ray": table.to(dev),
            "pred_pos_refine": d["pred_pos_refine"].to(dev).requires_grad_(True)}


def _stage1_dd(d, dev):
    """lidf_loss's data_dict from a restatement dict: the pairs ray-major, voxels ascending inside a ray. Returns
    (dd, order) with ray_major = reference[order]."""
    R, V = d["miss_bid"].shape[0], d["voxel_bound"].shape[0]
    order = torch.argsort(d["pair_ray"] * V + d["pair_vox"], stable=True)
    pair_ray, pair_vox = d["pair_ray"][order], d["pair_vox"][order]
    pair_off = torch.zeros(R + 1, dtype=torch.int64)
    pair_off[1:] = torch.cumsum(torch.bincount(pair_ray, minlength=R), 0)
    dd = {"bs": d["bs"], "h": d["h"], "w": d["w"], "xyz_flat": d["xyz_flat"].to(dev),
          "ray_bid": d["miss_bid"].int().to(dev), "ray_flat": d["miss_flat"].int().to(dev),
          "pair_off": pair_off.int().to(dev), "pair_ray": pair_ray.int().to(dev), "pair_vox": pair_vox.int().to(dev),
          "voxel_bound": d["voxel_bound"].to(dev),
          "pred_pos": d["pred_pos"].to(dev).requires_grad_(True),
          "pred_prob_end": d["pred_prob_end"][order].contiguous().to(dev).requires_grad_(True)}
    return dd, order


def _f32(x):
    return np.float32(float(x))


def test_refine_loss_device_route_on_the_fixture(cuda):
    from implicit_depth_amd import LidfLossOptions, refine_loss
    g, _ = rl.g10_files()
    d, ref = rl.g10_case(g, "hn")
    epoch, opt = int(g["epoch"]), rl.G10_CASES["hn"]
    dd = _refine_dd(d, cuda)
    out = refine_loss(dd, LidfLossOptions(hard_neg_select="device", **opt), "train", epoch)
    assert tuple(out) == rl.REFINE_LOSS_KEYS and all(v.dim() == 0 and v.is_cuda for v in out.values())
    assert out["loss_net"].requires_grad
    out["loss_net"].backward()
    loss64, gp64 = rl.loss_and_grad(d, torch.float64, epoch, 1.0, **opt)
    for i, k in enumerate(rl.REFINE_LOSS_KEYS):
        assert_f64_close("g10 hn device %s" % k, out[k].detach().cpu().reshape(1), loss64[i].reshape(1),
                         ref["loss"][i].reshape(1))
    assert_f64_close("g10 hn device g_pred_pos_refine", dd["pred_pos_refine"].grad.cpu(), gp64,
                     ref["g_pred_pos_refine"])
    # the torch route on the same inputs: the fixture keeps every top-k boundary clear of ties, so the weights and
    # with them the gradient are identical
    dt = _refine_dd(d, cuda)
    out_t = refine_loss(dt, LidfLossOptions(**opt), "train", epoch)
    out_t["loss_net"].backward()
    assert torch.equal(dd["pred_pos_refine"].grad, dt["pred_pos_refine"].grad)
    for k in ("err", "angle_err"):
        assert torch.equal(out[k], out_t[k])
    # loss_net from the returned means, in float, in the forward's order (the fixture's epoch has both gates' state)
    o = LidfLossOptions(**opt)
    net = _f32(o.pos_w) * _f32(out["pos_loss"])
    if o.surf_norm_w > 0 and epoch >= o.surf_norm_epo:
        net = net + _f32(o.surf_norm_w) * _f32(out["surf_norm_loss"])
    if o.smooth_w > 0 and epoch >= o.smooth_epo:
        net = net + _f32(o.smooth_w) * _f32(out["smooth_loss"])
    assert np.float32(net).tobytes() == _f32(out["loss_net"].detach()).tobytes()
    # bit-identical from run to run
    d2 = _refine_dd(d, cuda)
    out2 = refine_loss(d2, LidfLossOptions(hard_neg_select="device", **opt), "train", epoch)
    assert all(torch.equal(out[k].detach(), out2[k].detach()) for k in rl.REFINE_LOSS_KEYS)


@pytest.mark.parametrize("name", [n for n in sorted(tl.G9_CASES) if tl.G9_CASES[n][1]])
def test_lidf_loss_device_route_on_the_fixture(cuda, name):
    from implicit_depth_amd import LidfLossOptions, lidf_loss
    from implicit_depth_amd.losses import compute_gt
    g, _ = tl.g9_files()
    d, ref = tl.g9_case(g, name)
    epoch, opt = tl.g9_opt(name)
    assert opt["hard_neg"]
    dd, order = _stage1_dd(d, cuda)
    compute_gt(dd)
    out = lidf_loss(dd, LidfLossOptions(hard_neg_select="device", **opt), "train", epoch)
    assert tuple(out) == tl.LOSS_KEYS and all(v.dim() == 0 and v.is_cuda for v in out.values())
    out["loss_net"].backward()
    loss64, gp64, gl64 = tl.loss_and_grads(d, torch.float64, epoch, **opt)
    inv = torch.empty_like(order)
    inv[order] = torch.arange(order.shape[0])
    for i, k in enumerate(tl.LOSS_KEYS):
        assert_f64_close("g9 %s device %s" % (name, k), out[k].detach().cpu().reshape(1), loss64[i].reshape(1),
                         ref["loss"][i].reshape(1))
    assert_f64_close("g9 device g_pred_pos", dd["pred_pos"].grad.cpu(), gp64, ref["g_pred_pos"])
    assert_f64_close("g9 device g_pred_prob_end", dd["pred_prob_end"].grad.cpu()[inv], gl64, ref["g_pred_prob_end"])
    dt, _ = _stage1_dd(d, cuda)
    compute_gt(dt)
    out_t = lidf_loss(dt, LidfLossOptions(**opt), "train", epoch)
    out_t["loss_net"].backward()
    assert torch.equal(dd["pred_pos"].grad, dt["pred_pos"].grad)
    assert torch.equal(dd["pred_prob_end"].grad, dt["pred_prob_end"].grad)
    for k in ("acc", "err", "angle_err"):
        assert torch.equal(out[k], out_t[k])
    o = LidfLossOptions(**opt)
    net = _f32(o.pos_w) * _f32(out["pos_loss"]) + _f32(o.prob_w) * _f32(out["prob_loss"])
    if o.surf_norm_w > 0 and epoch >= o.surf_norm_epo:
        net = net + _f32(o.surf_norm_w) * _f32(out["surf_norm_loss"])
    if o.smooth_w > 0 and epoch >= o.smooth_epo:
        net = net + _f32(o.smooth_w) * _f32(out["smooth_loss"])
    assert np.float32(net).tobytes() == _f32(out["loss_net"].detach()).tobytes()


def test_smooth_term_enters_loss_net_on_the_device_route(cuda):
    """Both gates on: smooth_loss = the dx mean + the dy mean in float, and loss_net takes it last."""
    from implicit_depth_amd import LidfLossOptions, refine_loss
    d = rl.random_case(257)
    kw = dict(hard_neg=True, hard_neg_ratio=0.1, smooth_w=0.5)
    dd, dt = _refine_dd(d, cuda), _refine_dd(d, cuda)
    out = refine_loss(dd, LidfLossOptions(hard_neg_select="device", **kw))
    out_t = refine_loss(dt, LidfLossOptions(**kw))
    net = _f32(100.0) * _f32(out["pos_loss"])
    net = net + _f32(10.0) * _f32(out["surf_norm_loss"])
    net = net + _f32(0.5) * _f32(out["smooth_loss"])
    assert np.float32(net).tobytes() == _f32(out["loss_net"].detach()).tobytes()
    for k in rl.REFINE_LOSS_KEYS:   # the means of two routes: the same elements summed in another order
        a, b = float(out[k].detach()), float(out_t[k].detach())
        assert abs(a - b) <= 4 * 2.0 ** -23 * abs(b), (k, a, b)


def test_k_zero_end_to_end(cuda):
    """R < 10 at ratio 0.1: NaN means, finite metrics, the torch route's gradient."""
    from implicit_depth_amd import LidfLossOptions, refine_loss
    d = rl.random_case(7)
    kw = dict(hard_neg=True, hard_neg_ratio=0.1, smooth_w=0.5)
    dd, dt = _refine_dd(d, cuda), _refine_dd(d, cuda)
    out = refine_loss(dd, LidfLossOptions(hard_neg_select="device", **kw))
    out_t = refine_loss(dt, LidfLossOptions(**kw))
    out["loss_net"].backward(), out_t["loss_net"].backward()
    for k in ("pos_loss", "surf_norm_loss", "smooth_loss", "loss_net"):
        assert torch.isnan(out[k]) and torch.isnan(out_t[k])
    for k in ("err", "angle_err"):
        assert torch.isfinite(out[k]) and torch.equal(out[k], out_t[k])
    assert torch.equal(dd["pred_pos_refine"].grad, dt["pred_pos_refine"].grad)


def test_stage1_without_a_labelled_pair(cuda):
    """The label count 0 stays on the device: NaN prob_loss, the other terms finite, no gradient on the logits."""
    from implicit_depth_amd import LidfLossOptions, lidf_loss
    from implicit_depth_amd.losses import compute_gt
    g, _ = tl.g9_files()
    d, _ = tl.g9_case(g, "e0")
    d["voxel_bound"] = d["voxel_bound"] + 50.0
    dd, _ = _stage1_dd(d, cuda)
    compute_gt(dd)
    assert int(dd["n_label"]) == 0 and int(dd["pcl_label"].sum()) == 0
    out = lidf_loss(dd, LidfLossOptions(hard_neg=True, hard_neg_ratio=0.1, hard_neg_select="device"))
    out["loss_net"].backward()
    assert torch.isnan(out["prob_loss"]) and torch.isnan(out["loss_net"])
    assert all(torch.isfinite(out[k]) for k in ("pos_loss", "surf_norm_loss", "smooth_loss", "acc", "err", "angle_err"))
    assert torch.isfinite(dd["pred_pos"].grad).all() and bool((dd["pred_prob_end"].grad == 0).all())
