"""Float64 references for PointNet2Stage and the stage-2 refine chain (tests only; CPU, plain torch ops).

PointNet2Stage has hard ReLUs and two max-poolings: where a pre-activation sits within rounding of 0, or a pooled
maximum has a runner-up within rounding of it, rounding decides which route the gradient takes, in any precision —
the float32 oracle then differs from the float64 one by a whole entry, and its error stops being a unit. Behind a
pooling such rows cannot simply be given zero upstream gradient (util.kink_rows does that for the decoders), so
the inputs are CONDITIONED instead: the float64 evaluation is repeated, dropping the points that sit at a kink or
at a near-tie, until none is left. On the conditioned inputs float32 and float64 take the same routes and
util.assert_f64_close applies as it does to the decoders.

Exact ties (duplicated rows) are a different matter: there the route is a definition. torch_scatter, and the
kernels (lidf_pointnet_train.hip: 64-bit maximum of value bits << 32 | ~row over a stable sort), give the whole
gradient to the lowest input row; the oracle's amax autograd splits it evenly. pointnet2stage_argrouted is the
oracle's function with torch_scatter's gradient."""
import functools

import torch
import torch.nn.functional as F

from util import kink_rows_of, orc

# About 5 x the float32 oracle's largest pre-activation error against float64, relative to its layer's max|z|
# (6.0-6.5e-7 at n = 70000, V = 300, vox_lin2, depending on the CPU's summation order; tests/test_pointnet_ref.py
# measures it again and asserts REL >= 4 x it): above the 4 x (util.F64_K) a kernel is conceded, so that neither
# the float32 oracle nor a kernel within the criterion takes another route than float64 on conditioned inputs.
REL = 3e-6
FACE_EPS = 1e-6      # a position this close to a voxel's face may fall on either side of it in float32
POINT_LAYERS = ("point_lin1", "point_lin2", "point_lin3", "point_lin4")
LAYERS = ("point_lin1", "point_lin2", "vox_lin1", "point_lin3", "point_lin4", "vox_lin2")


def _near_zero(z, rel):
    """[rows, F] bool: |z| < rel x max|z| of the layer."""
    if z.numel() == 0:
        return torch.zeros(z.shape, dtype=torch.bool, device=z.device)
    return z.abs() < rel * z.abs().max()


def pool_args(x, vox, V):
    """Max-pooling of the rows x [n, F] (post-ReLU) into V voxels with torch_scatter's arg: (mx [V, F], arg [V, F])
    — arg is the lowest row holding the maximum, n where the maximum is 0 (no row: empty voxel or nothing positive)."""
    n = x.shape[0]
    idx = vox.view(-1, 1).expand_as(x)
    mx = torch.zeros(V, x.shape[1], dtype=x.dtype, device=x.device).scatter_reduce(0, idx, x, reduce="amax",
                                                                                   include_self=True)
    rows = torch.arange(n, device=x.device).view(-1, 1).expand_as(x)
    cand = torch.where((x == mx[vox]) & (x > 0), rows, torch.full_like(rows, n))
    arg = torch.full((V, x.shape[1]), n, dtype=torch.long, device=x.device)
    return mx, arg.scatter_reduce(0, idx, cand, reduce="amin", include_self=True)


def runner_up(x, vox, V, arg):
    """[V, F]: the largest value of the voxel's rows other than the arg row (0, the pooling's floor, if none)."""
    n = x.shape[0]
    idx = vox.view(-1, 1).expand_as(x)
    rest = torch.cat((x, x.new_zeros(1, x.shape[1])), 0)
    rest.scatter_(0, arg, float("-inf"))
    return x.new_zeros(V, x.shape[1]).scatter_reduce(0, idx, rest[:n], reduce="amax", include_self=True)


def _gather_pool(x, vox, V):
    """The pooled rows by gathering the arg row: the oracle's values bit for bit, torch_scatter's gradient."""
    _, arg = pool_args(x.detach(), vox, V)
    return torch.gather(torch.cat((x, x.new_zeros(1, x.shape[1])), 0), 0, arg)


def rowwise_linear(x, w, b):
    """F.linear as one product-and-sum per output entry. A matrix product may round equal rows differently
    depending on where in the batch they stand (a BLAS blocks the rows; seen in float64 on one CPU at a batch of
    2 x 257); here a row's result depends on that row alone, so equal rows stay equal bit for bit."""
    return (x.unsqueeze(1) * w.unsqueeze(0)).sum(-1) + b


def pointnet_forward(p, inp, vox, V, pool=_gather_pool, spread=lambda g1, vox: g1[vox], linear=F.linear):
    """orc.pointnet2stage's operations in its order, with the two poolings (pool(x, vox, V) -> [V, F]), the
    voxel-to-point gather (spread(g1, vox) -> [n, 64]) and the linear map replaceable: pointnet2stage_argrouted
    below, and the deliberately wrong variants of tests/test_pointnet_ref.py."""
    lin = lambda x, k: linear(x, p[k + ".weight"], p[k + ".bias"])  # noqa: E731
    f1 = F.relu(lin(inp, "point_lin1"))
    f2 = F.relu(lin(f1, "point_lin2"))
    g1 = F.relu(lin(pool(f2, vox, V), "vox_lin1"))
    f3 = torch.cat((spread(g1, vox), f2), -1)
    f4 = F.relu(lin(f3, "point_lin3"))
    f5 = F.relu(lin(f4, "point_lin4"))
    return F.relu(lin(pool(f5, vox, V), "vox_lin2"))


def pointnet2stage_argrouted(p, inp, vox, V):
    """orc.pointnet2stage with torch_scatter's scatter-max gradient: among equal maxima the lowest input row gets
    all of it; an entry whose maximum is 0 has no row. Equal to the oracle in value bit for bit, and in gradient
    wherever no two rows of a voxel tie exactly."""
    return pointnet_forward(p, inp, vox, V)


def pointnet_grads(fn, p, inp, vox, V, w, dt, device=None):
    """Output and gradients of sum(fn(p, inp, vox, V) * w) at dtype dt: (out, {param: grad, "inp": grad}); fresh
    leaves per call."""
    dev = device if device is not None else inp.device
    pc = {k: v.detach().to(dev, dt, copy=True).requires_grad_(True) for k, v in p.items()}
    xc = inp.detach().to(dev, dt, copy=True).requires_grad_(True)
    out = fn(pc, xc, vox.to(dev), V)
    (out * w.to(dev, dt)).sum().backward()
    g = {k: v.grad for k, v in pc.items()}
    g["inp"] = xc.grad
    return out.detach(), g


# ----------------------------------------------------------------------------------------------------------------
# conditioning
# ----------------------------------------------------------------------------------------------------------------
def pointnet_flags(tr, V, rel):
    """From one orc.pointnet2stage trace (float64): (bad [n] bool, out_mask [V, 128] bool).
    bad: (a) a per-point pre-activation within rel x max|z| of 0 for its layer; (b) the arg row of a pooled entry
    with a positive maximum whose runner-up in the same voxel is within rel x max of it; (c) the first row of a
    voxel that has a vox_lin1 pre-activation within rel x max|z| of 0.
    out_mask: vox_lin2 pre-activations within rel x max|z| of 0."""
    vox = tr["pool1"][1]
    n = vox.shape[0]
    bad = torch.zeros(n, dtype=torch.bool)
    for k in POINT_LAYERS:
        bad |= _near_zero(tr[k], rel).any(1)
    for key in ("pool1", "pool2"):
        x, vx = tr[key]
        mx, arg = pool_args(x, vx, V)
        near = (mx > 0) & (mx - runner_up(x, vx, V, arg) <= rel * mx)
        bad[arg[near]] = True
    first = torch.full((V,), n, dtype=torch.long).scatter_reduce(0, vox, torch.arange(n), reduce="amin",
                                                                 include_self=True)
    near = _near_zero(tr["vox_lin1"], rel).any(1) & (first < n)
    bad[first[near]] = True
    return bad, _near_zero(tr["vox_lin2"], rel)


def condition_pointnet(p64, inp, vox, V, rel=REL, max_passes=50):
    """(keep [n] bool, out_mask [V, 128] bool, passes): the float64 evaluation iterated to a fixed point, every
    pass dropping the points pointnet_flags marks (a dropped point changes the pooled values, hence the
    re-evaluation); passes counts the evaluations that dropped something. Rows with vox < 0 are not kept.
    The test zeroes the upstream gradient at out_mask."""
    x = inp.detach().double()
    vox = vox.long()
    keep = vox >= 0
    passes = 0
    while True:
        ids = torch.nonzero(keep)[:, 0]
        tr = []
        with torch.no_grad():
            orc.pointnet2stage(p64, x[ids], vox[ids], V, trace=tr)
        bad, out_mask = pointnet_flags(tr[0], V, rel)
        if not bool(bad.any()):
            return keep, out_mask, passes
        keep[ids[bad]] = False
        passes += 1
        assert passes <= max_passes, "conditioning does not settle"


# the shapes of tests/test_f64_stage2_gpu.py, each for the path of lidf_pointnet_train.hip it takes: under one
# 128-point tile; two tiles plus one row; inside the 32-row pooling window (PNT_WINDOW); one voxel in four
# PNT_CH = 256 chunks; ~4 points per voxel (a tile spans more voxels than the window: the global 64-bit maxima;
# V above the inference table's 288; empty voxels); more tiles than workgroups
SHAPES = [(5, 3), (257, 9), (3000, 40), (1000, 1), (20000, 5000), (70000, 300)]


@functools.lru_cache(maxsize=None)
def pointnet_case(n, V, left_out=0.0):
    """Parameters, inputs and upstream gradient of test_train_gpu.py::test_pointnet_gradients at (n, V), conditioned:
    a dict with p, inp [n, 6], vox [n] (left_out: that share of the rows at -1 from the start), keep [n], w [V, 128]
    (zero at out_mask), passes, masked. Computed once per shape and shared; nobody writes to it."""
    g = torch.Generator().manual_seed(n + V)
    p = orc.init_pointnet(7, 1.5)
    inp = torch.randn(n, 6, generator=g)
    vox = torch.randint(0, V, (n,), generator=g)
    w = torch.randn(V, 128, generator=g)
    if left_out:
        vox[torch.rand(n, generator=g) < left_out] = -1
    keep, out_mask, passes = condition_pointnet({k: v.double() for k, v in p.items()}, inp, vox, V)
    return {"p": p, "inp": inp, "vox": vox, "keep": keep, "w": torch.where(out_mask, torch.zeros_like(w), w),
            "passes": passes, "masked": int(out_mask.sum()), "V": V}


RAY_KEYS = ("ray_dir", "ray_pix", "ray_bid", "ray_flat", "pred_pos", "max_pair_id")


def refine_case(frames=2, h=20, w=24, n_valid=1500, noise=0.03):
    """The stage-2 scene of the float64 refine tests: orc.synthetic_scene(frames, h, w, 5, seed=31, ragged=True)
    with the 0.25-wide voxel boxes, image, valid points and parameters of
    test_train_gpu.py::test_refine_train_gradients_vs_oracle; pred_pos / max_pair_id from the oracle's query."""
    scene = orc.synthetic_scene(frames, h, w, 5, seed=31, ragged=True)
    with torch.no_grad():
        s1 = orc.query(scene["ray_dir"], scene["ray_pix"], scene["ray_bid"], scene["pair_ray"].long(),
                       scene["pair_vox"].long(), scene["pair_t"], scene["pair_off"], scene["feat_grid"],
                       scene["vox_feat"], scene["prob_p"], scene["off_p"], fast_roi=True)
    g = torch.Generator().manual_seed(9)
    V = scene["V"]
    per = V // frames
    case = {k: scene[k] for k in ("ray_dir", "ray_pix", "ray_bid", "ray_flat", "pair_vox", "feat_grid")}
    case["pred_pos"], case["max_pair_id"] = s1["pred_pos"].contiguous(), s1["max_pair_id"].long()
    case["voxel_bound"] = torch.cat((scene["vox_center"] - 0.125, scene["vox_center"] + 0.125), 1)
    case["voxel_bid"] = torch.arange(frames).repeat_interleave(per).int()
    case["rgb_img"] = torch.randn(frames, 3, h, w, generator=g)
    case["valid_inp"] = torch.randn(n_valid, 6, generator=g) * 0.2
    case["valid_vox"] = torch.randint(0, V, (n_valid,), generator=g).int()
    case["noise"] = noise
    case["pnet_p"] = orc.init_pointnet(5, 1.5)
    case["off_p"] = orc.randomize_biases(orc.init_decoder("IEF", 334, 77, 5.0), 78)
    # the voxel list as cells of its grid (query.get_occ_vox_bound's entries): every cell of the 9 x 9 x 9 grid
    ci = torch.arange(9)
    coord = torch.stack(torch.meshgrid(ci, ci, ci, indexing="ij"), -1).reshape(-1, 3)
    case["grid"] = {"xmin": (-1.125, -1.125, -0.125), "grid_dims": (9, 9, 9), "part_size": 0.25,
                    "voxel_coord": coord.repeat(frames, 1).int().contiguous()}
    return case


@functools.lru_cache(maxsize=None)
def conditioned_refine_case(pos_rel=False, pnet_pos_rel=True):
    """refine_case() conditioned for two iterations (which covers one: the first iteration is the same):
    (case, keep_ray, keep_valid, passes). Computed once per position type and shared; nobody writes to it."""
    case = refine_case()
    keep_ray, keep_valid, passes = condition_refine(case, 2, pos_rel, pnet_pos_rel)
    return subset_case(case, keep_ray, keep_valid), keep_ray, keep_valid, passes


def subset_case(case, keep_ray, keep_valid):
    out = dict(case)
    for k in RAY_KEYS:
        out[k] = case[k][keep_ray].contiguous()
    out["valid_inp"] = case["valid_inp"][keep_valid].contiguous()
    out["valid_vox"] = case["valid_vox"][keep_valid].contiguous()
    return out


def refine_chain(case, dt, forward_times, pos_rel=False, pnet_pos_rel=True, leaves=None, trace=None):
    """forward_times iterations of orc.refine_step at dtype dt from pred_pos + noise x ray_dir, the per-ray RoIAlign
    rows through orc.roi_align_fast (differentiable, follows dt). leaves: a dict that receives the tensors a
    gradient is taken of ("pnet." / "dec." parameters, "pred_pos", "feat_grid"), as fresh leaves.
    Returns (pos, [end voxels of every iteration])."""
    c = lambda t: t.detach().to(dt, copy=True)  # noqa: E731
    pn = {k: c(v) for k, v in case["pnet_p"].items()}
    of = {k: c(v) for k, v in case["off_p"].items()}
    pp, fg = c(case["pred_pos"]), c(case["feat_grid"])
    if leaves is not None:
        for t in list(pn.values()) + list(of.values()) + [pp, fg]:
            t.requires_grad_(True)
        leaves.update({"pnet." + k: v for k, v in pn.items()})
        leaves.update({"dec." + k: v for k, v in of.items()})
        leaves["pred_pos"], leaves["feat_grid"] = pp, fg
    ray_dir = case["ray_dir"].to(dt)
    R = ray_dir.shape[0]
    boxes = orc.roi_boxes(case["ray_pix"].long(), case["ray_bid"].long(), fg.shape[2], fg.shape[3], 8)
    ray_rgb = orc.roi_align_fast(fg, boxes).reshape(R, -1)
    pos = pp + case["noise"] * ray_dir
    evs = []
    for _ in range(forward_times):
        pos, ev, _ = orc.refine_step(pos, ray_dir, case["ray_pix"], case["ray_bid"], case["ray_flat"],
                                     case["max_pair_id"], case["pair_vox"], case["voxel_bound"].to(dt),
                                     case["voxel_bid"], case["rgb_img"].to(dt), fg, case["valid_inp"].to(dt),
                                     case["valid_vox"], pn, of, pos_rel=pos_rel, pnet_pos_rel=pnet_pos_rel,
                                     ray_rgb=ray_rgb, trace=trace)
        evs.append(ev)
    return pos, evs


def refine_grads(case, dt, forward_times, w, **kw):
    """(pos, end voxels of the last iteration, {leaf: gradient of sum(pos * w)}) of refine_chain at dtype dt."""
    leaves = {}
    pos, evs = refine_chain(case, dt, forward_times, leaves=leaves, **kw)
    (pos * w.to(dt)).sum().backward()
    return pos.detach(), evs[-1], {k: v.grad for k, v in leaves.items()}


def _near_face(pos, bid, voxel_bound, voxel_bid, eps):
    """[R] bool: a coordinate of pos within eps of a face plane of any voxel of the ray's frame."""
    bad = torch.zeros(pos.shape[0], dtype=torch.bool)
    for b in torch.unique(bid).tolist():
        rows = torch.nonzero(bid == b)[:, 0]
        vb = voxel_bound[voxel_bid == b].double()
        for a in range(3):
            planes = torch.unique(torch.cat((vb[:, a], vb[:, 3 + a])))
            d = (pos[rows, a].double().view(-1, 1) - planes.view(1, -1)).abs().min(1).values
            bad[rows[d < eps]] = True
    return bad


def condition_refine(case, forward_times, pos_rel=False, pnet_pos_rel=True, rel=REL, max_passes=50):
    """(keep_ray [R] bool, keep_valid [Nv] bool, passes): condition_pointnet's rules over the whole forward_times-
    iteration chain of orc.refine_step in float64. A flagged valid point is dropped; a flagged predicted point
    drops its ray from the scene (subset_case), and so does a decoder row at a kink in any iteration
    (util.kink_rows' rule, output clamp included) and a position entering an iteration within FACE_EPS of a
    face of a voxel of its frame (the end voxel is a discrete choice). vox_lin2 feeds the decoder rows of the
    rays that end in the voxel: an entry of it at a kink drops those rays."""
    R, Nv = case["ray_dir"].shape[0], case["valid_inp"].shape[0]
    V = case["voxel_bound"].shape[0]
    keep_ray, keep_valid = torch.ones(R, dtype=torch.bool), torch.ones(Nv, dtype=torch.bool)
    passes = 0
    while True:
        rid, vid = torch.nonzero(keep_ray)[:, 0], torch.nonzero(keep_valid)[:, 0]
        sub = subset_case(case, keep_ray, keep_valid)
        tr = []
        with torch.no_grad():
            refine_chain(sub, torch.float64, forward_times, pos_rel, pnet_pos_rel, trace=tr)
        bad_ray = torch.zeros(rid.numel(), dtype=torch.bool)
        bad_valid = torch.zeros(vid.numel(), dtype=torch.bool)
        for it in tr:
            bad, out_mask = pointnet_flags(it["pnet"], V, rel)
            bad_valid |= bad[:vid.numel()]
            bad_ray |= bad[vid.numel():]
            bad_ray |= out_mask.any(1)[it["end_voxel"]]
            bad_ray |= kink_rows_of(it["preacts"][:-1], it["preacts"][-1], rel=rel)
            bad_ray |= _near_face(it["pos"], sub["ray_bid"], case["voxel_bound"], case["voxel_bid"], FACE_EPS)
        if not bool(bad_ray.any() or bad_valid.any()):
            return keep_ray, keep_valid, passes
        keep_ray[rid[bad_ray]] = False
        keep_valid[vid[bad_valid]] = False
        passes += 1
        assert passes <= max_passes, "conditioning does not settle"
