"""The small scenes of the entry-point sweeps, once (tests only).

tests/test_workspace_gpu.py (arbitrary workspace contents) and tests/test_streams_gpu.py (arbitrary caller streams)
drive the same inventory of entry points on the same scenes — the smallest shapes at which the kernels take their
multi-block, ragged and two-launch paths. This module holds
  * `same()`, the bit-for-bit comparison of two runs,
  * the scene builders with their cached references, and
  * for the stream sweep, every entry split into an `Entry`: the device inputs it reads (`inputs`, host tensors the
    harness stages), the modules whose parameters it reads (`modules`), `call(live) -> results` (launches only: no
    upload from host memory, no host read except the ones listed in `reads_back`) and `check(results)`, which holds
    the results to the reference of the entry's existing test with that test's bound (imported, not restated).
"""
import functools

import numpy as np
import torch

from util import TOL, assert_f64_close, k_for, make_module, make_pointnet, oracle_grads, oracle_query, orc


# ------------------------------------------------------------------------------------------------------------------
# Comparison
# ------------------------------------------------------------------------------------------------------------------
def _bits(t):
    t = t.detach().contiguous().reshape(-1)
    if t.is_floating_point():
        return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])
    return t


def same(got, base, what="out", ref="the zero-filled run"):
    """Bit for bit (NaN payloads included): tensors, and dicts / lists / tuples of them."""
    if torch.is_tensor(base):
        assert torch.is_tensor(got) and got.shape == base.shape and got.dtype == base.dtype, what
        if not torch.equal(_bits(got), _bits(base)):
            d = (got.double() - base.double()).abs()
            raise AssertionError("%s differs from %s: %d of %d entries, max |d| %g"
                                 % (what, ref, int((_bits(got) != _bits(base)).sum()), base.numel(),
                                    float(d[d == d].max()) if bool((d == d).any()) else float("nan")))
    elif isinstance(base, dict):
        assert set(got) == set(base), what
        for k in base:
            same(got[k], base[k], "%s[%r]" % (what, k), ref)
    elif isinstance(base, (list, tuple)):
        assert len(got) == len(base), what
        for i, (a, b) in enumerate(zip(got, base)):
            same(a, b, "%s[%d]" % (what, i), ref)
    else:
        assert got == base or (got != got and base != base), (what, got, base)


def close_rel(a, b, what, rel, floor):
    scale = max(floor, b.abs().max().item())
    err = (a - b).abs().max().item()
    assert err <= rel * scale, (what, err, scale)


# ------------------------------------------------------------------------------------------------------------------
# Scenes
# ------------------------------------------------------------------------------------------------------------------
def scan_values(m):
    return torch.randint(0, 30, (m,), generator=torch.Generator().manual_seed(m), dtype=torch.int32)


def voxel_points(n, B):
    g = torch.Generator().manual_seed(n + B)                          # test_voxelize_random's points
    xyz = (torch.rand(n, 3, generator=g) - 0.5) * 3.0 + torch.tensor([0.0, 0.0, 1.0])
    xyz[:5] = torch.tensor([-1.125, -1.125, -0.125])
    xyz[5:8] = torch.tensor([1.125, 0.0, 1.0])
    return xyz, torch.randint(0, B, (n,), generator=g)


@functools.lru_cache(maxsize=None)
def voxel_ref(n, B):
    return orc.occupied_voxels(*voxel_points(n, B))


def mask_2x16x24(seed=1624, p=0.5):
    return (np.random.default_rng(seed).random((2, 16, 24)) < p).astype(np.uint8)


def intr(bs, h, w, dev):
    from test_miss_window_gpu import _intr
    return _intr(bs, h, w, dev)


QUERY_KEYS = ("pred_offset", "pred_prob_end", "pair_pred_pos", "pred_pos", "pred_prob_end_softmax", "max_pair_id",
              "depth", "rayfeat")


@functools.lru_cache(maxsize=None)
def query_scene():
    scene = orc.synthetic_scene(2, 13, 17, 6, seed=1317, ragged=True)
    return scene, oracle_query(scene)


def check_query(scene, ref, got):
    for k in ("pred_offset", "pred_prob_end", "pair_pred_pos", "pred_pos"):
        err = (got[k].cpu() - ref[k]).abs().max().item()
        assert err <= TOL, (k, err)
    assert (got["pred_prob_end_softmax"].cpu() - ref["pred_prob_end_softmax"]).abs().max().item() <= 1e-5
    gid, rid, sm, P = got["max_pair_id"].cpu(), ref["max_pair_id"], ref["pred_prob_end_softmax"], scene["P"]
    for r in (gid != rid).nonzero().flatten().tolist():     # only float-noise ties may differ
        assert gid[r] < P and rid[r] < P and abs(sm[gid[r]] - sm[rid[r]]) <= 1e-6
    depth_ref = ref["pred_pos"][:, 2].reshape(scene["B"], scene["h"], scene["w"])
    assert (got["depth"].cpu() - depth_ref).abs().mean().item() <= TOL


@functools.lru_cache(maxsize=None)
def query_scene_gf32():
    scene = dict(query_scene()[0])
    D = scene["D"]
    scene["prob_p"], scene["off_p"] = orc.init_decoder("IMNET", D, 7, 5.0, gf=32), orc.init_decoder("IEF", D, 8, 5.0, gf=32)
    return scene, oracle_query(scene)


@functools.lru_cache(maxsize=None)
def query_train_case(pos_loss_only):
    """tests/test_query_train_gpu.py::test_query_gradients' scene with oracle autograd on the CPU."""
    scene = orc.synthetic_scene(2, 12, 16, 8, seed=71, ragged=True)
    R, P = scene["R"], scene["P"]
    gen = torch.Generator().manual_seed(72)
    w = {"prob": torch.randn(P, generator=gen), "off": torch.randn(P, generator=gen), "pos": torch.randn(R, 3, generator=gen)}
    if pos_loss_only:      # offsets="selected": pred_offset exists at the selected pairs only (_ref_loss)
        w["off"] = torch.zeros(P)
    pp = {k: v.clone().requires_grad_(True) for k, v in scene["prob_p"].items()}
    po = {k: v.clone().requires_grad_(True) for k, v in scene["off_p"].items()}
    fg = scene["feat_grid"].clone().requires_grad_(True)
    vf = scene["vox_feat"].clone().requires_grad_(True)
    ref = orc.query(scene["ray_dir"], scene["ray_pix"], scene["ray_bid"], scene["pair_ray"].long(),
                    scene["pair_vox"].long(), scene["pair_t"], scene["pair_off"], fg, vf, pp, po, fast_roi=True,
                    vox_center=scene["vox_center"], pos_rel=True, offset_range=(-0.2, 0.2), part_size=0.25)
    query_loss(ref, w, pos_loss_only).backward()
    g = {"feat_grid": fg.grad, "vox_feat": vf.grad}
    g.update({"prob." + k: v.grad for k, v in pp.items()})
    g.update({"off." + k: v.grad for k, v in po.items()})
    return scene, w, {k: ref[k].detach() for k in ("pred_offset", "pred_prob_end", "pair_pred_pos", "pred_pos")}, g


def query_loss(out, w, pos_loss_only):
    loss = (out["pred_prob_end"][:, 0] * w["prob"]).sum() + (out["pred_pos"] * w["pos"]).sum()
    return loss if pos_loss_only else loss + (out["pred_offset"][:, 0] * w["off"]).sum()


@functools.lru_cache(maxsize=None)
def pointnet_case(n, v):
    g = torch.Generator().manual_seed(n + v)
    p = orc.init_pointnet(7, 1.5)
    inp = torch.randn(n, 6, generator=g)
    vox = torch.randint(0, v, (n,), generator=g)
    return p, inp, vox, orc.pointnet2stage(p, inp, vox, v)


@functools.lru_cache(maxsize=None)
def pointnet_train_case(n, v):
    g = torch.Generator().manual_seed(n + v)
    p = orc.init_pointnet(7, 1.5)
    inp = torch.randn(n, 6, generator=g)
    vox = torch.randint(0, v, (n,), generator=g)
    wgt = torch.randn(v, 128, generator=g)
    pr = {k: t.clone().requires_grad_(True) for k, t in p.items()}
    xi = inp.clone().requires_grad_(True)
    ref = orc.pointnet2stage(pr, xi, vox, v)
    (ref * wgt).sum().backward()
    grads = {k: t.grad for k, t in pr.items()}
    grads["inp"] = xi.grad
    return p, inp, vox, wgt, ref.detach(), grads


@functools.lru_cache(maxsize=None)
def refine_case():
    """tests/test_refine_gpu.py::test_refine_synthetic_vs_oracle's scene."""
    scene = orc.synthetic_scene(2, 12, 16, 6, seed=21, ragged=True)
    g = torch.Generator().manual_seed(3)
    vb = torch.cat((scene["vox_center"] - 0.125, scene["vox_center"] + 0.125), 1)
    vbid = torch.arange(2).repeat_interleave(729).int()
    rgb = torch.randn(2, 3, 12, 16, generator=g)
    valid_inp = torch.randn(500, 6, generator=g) * 0.2
    valid_vox = torch.randint(0, scene["V"], (500,), generator=g).int()
    pnet_p = orc.init_pointnet(5, 1.5)
    offr_p = orc.randomize_biases(orc.init_decoder("IEF", 334, 77, 5.0), 78)
    return scene, vb, vbid, rgb, valid_inp, valid_vox, pnet_p, offr_p


_REFINE_ORACLE = {}


def refine_oracle(pos, mid):
    """Two oracle iterations from the product's own stage 1 (the same tensors in every case: computed once)."""
    if "out" not in _REFINE_ORACLE or not torch.equal(_REFINE_ORACLE["in"], pos):
        scene, vb, vbid, rgb, valid_inp, valid_vox, pnet_p, offr_p = refine_case()
        start = pos
        for _ in range(2):
            pos, ev, _ = orc.refine_step(pos, scene["ray_dir"], scene["ray_pix"], scene["ray_bid"], scene["ray_flat"],
                                         mid, scene["pair_vox"], vb, vbid, rgb, scene["feat_grid"], valid_inp,
                                         valid_vox, pnet_p, offr_p)
        _REFINE_ORACLE.update({"in": start, "out": (pos, ev)})
    return _REFINE_ORACLE["out"]


def step_result(dd, loss, feat, mods, keys):
    res = {"loss." + k: loss[k].detach() for k in loss}
    res.update({k: dd[k].detach() for k in keys})
    if feat is not None and feat.grad is not None:
        res["full_rgb_feat"] = feat.grad
    for i, m in enumerate(mods):
        res.update({"m%d.%s" % (i, k): q.grad for k, q in m.named_parameters() if q.grad is not None})
    return res


# ------------------------------------------------------------------------------------------------------------------
# Entries: device inputs + call(live) -> results + check(results)
# ------------------------------------------------------------------------------------------------------------------
class Entry:
    """One entry point on one scene.

    inputs      {name: host tensor}: everything the entry reads from device memory that the caller supplies (the
                harness uploads them; `call` finds the device copies under the same names in `live`)
    modules     nn.Modules on the device whose parameters the entry reads
    call        call(live) -> tensor / dict / list of device tensors. Launches only.
    check       check(results): the reference and the bound of the entry's existing test
    zero        names of integer / mask inputs whose decoy is all zero: zero is a valid value of each (noted at the
                builder). Every other integer input's decoy is the input itself, every float input's is NaN.
    loose       {result key: fn(got, base)}: the results the documents name as not bit-reproducible, each with the
                run-to-run bound of its existing test; every other result is compared bit for bit
    reads_back  None, or the call site of the host read that makes the caller wait for its stream inside the entry
    side        None, or a function returning the second stream the entry owns (the "slow side" mode)
    finish      None, or finish(cloned results) -> results, applied once the stream is synchronised (capacity buffers
                cut to the counts the device wrote)
    """

    def __init__(self, inputs, call, check, modules=(), zero=(), loose=None, reads_back=None, side=None, finish=None):
        self.inputs, self.call, self.check, self.modules = dict(inputs), call, check, tuple(modules)
        self.zero, self.loose, self.reads_back, self.side = frozenset(zero), dict(loose or {}), reads_back, side
        self.finish = finish
        assert self.zero <= set(self.inputs)


def _feat_grid_loose(a, b):
    """feat_grid's gradient where every RoI box clamps at the border: float atomics; the bound of
    test_workspace_gpu.py::test_lidf_query_train."""
    assert (a - b).abs().max().item() <= 16 * 2.0 ** -24 * b.abs().max().item()


def _held_by_reference(a, b):
    """lidf_rows_backward_f32's d vox_feat (float atomics, lidf_hip.h): the reference bound of check() holds it."""


# -- geometry and samplers -----------------------------------------------------------------------------------------
def entry_exclusive_scan(dev, n=32769):
    """lidf_exclusive_scan_i32 at the first three-launch length. Decoy zero: the values are summands, not indices."""
    from implicit_depth_amd import _lib
    L = _lib.lib()

    def call(live):
        out = torch.full((n + 1,), -7, dtype=torch.int32, device=dev)
        wsb = L.lidf_exclusive_scan_workspace_bytes(n)
        ws = _lib.workspace(wsb, dev)
        _lib.check(L.lidf_exclusive_scan_i32(_lib.ptr(live["x"]), n, _lib.ptr(out), _lib.ptr(ws), wsb,
                                             _lib.current_stream(dev)))
        return out

    def check(got):
        ref = torch.zeros(n + 1, dtype=torch.int64)
        ref[1:] = torch.cumsum(scan_values(n).long(), 0)
        assert (got.cpu().long() == ref).all()

    return Entry({"x": scan_values(n)}, call, check, zero=("x",))


def entry_get_occ_vox_bound(dev, n=20000, B=3):
    """get_occ_vox_bound. lidf_vox_mark_kernel drops a NaN point (its cell test fails) and range-checks the frame
    index, so NaN points and frame 0 for every point are valid inputs."""
    from implicit_depth_amd.query import get_occ_vox_bound
    from test_voxelize_gpu import check as check_vox
    xyz, bid = voxel_points(n, B)

    def call(live):
        return get_occ_vox_bound(live["xyz"], live["bid"], batch=B)

    return Entry({"xyz": xyz, "bid": bid.int()}, call, lambda got: check_vox(got, voxel_ref(n, B)), zero=("bid",),
                 reads_back="query.get_occ_vox_bound: counts.tolist() (V, Nv)")


def _check_pairs(got, d, vb, rb, vbid):
    m_ref, t_ref = orc.ray_aabb(d, vb, rb, vbid)
    pr_ref, pv_ref, pt_ref, off_ref = orc.pairs_from_dense(m_ref, t_ref)
    off, pr, pv, pt = got
    assert (off.cpu().long() == off_ref).all() and (pr.cpu().long() == pr_ref).all()
    assert (pv.cpu().long() == pv_ref).all() and (pt.cpu() == pt_ref).all()


def entry_ray_aabb_voxel_list(dev, R=257, V=300):
    """compute_ray_aabb, voxel by voxel. Frame indices are compared, never used as indices: decoy zero."""
    from implicit_depth_amd.query import compute_ray_aabb
    from test_boxes_gpu import scene
    d, vb, rb, vbid = scene(R, V, R + V)

    def call(live):
        return compute_ray_aabb(live["ray_dir"], live["voxel_bound"], live["ray_bid"], live["voxel_bid"])

    return Entry({"ray_dir": torch.from_numpy(d), "voxel_bound": torch.from_numpy(vb), "ray_bid": torch.from_numpy(rb),
                  "voxel_bid": torch.from_numpy(vbid)}, call, lambda got: _check_pairs(got, d, vb, rb, vbid),
                 zero=("ray_bid", "voxel_bid"), reads_back="query.compute_ray_aabb: pair_off[-1].item() (P)")


def entry_ray_aabb_grid_walk(dev, R=700, B=2, fill=0.3):
    """compute_ray_aabb, the regular-grid walk. lidf_grid_build_kernel range-checks frame and cell of every voxel,
    the walk range-checks the ray's frame and loops over the grid's own extents: frame 0 and cell (0, 0, 0) for
    everything are valid inputs. The count and the fill pass are separated by the host read of P, so both see the
    same inputs on any stream."""
    from implicit_depth_amd.query import compute_ray_aabb
    from test_boxes_gpu import grid_scene
    d, vb, rb, vbid, coord = grid_scene(R, B, 9, fill, seed=R + B)
    assert vb.shape[0] <= 600

    def call(live):
        return compute_ray_aabb(live["ray_dir"], live["voxel_bound"], live["ray_bid"], live["voxel_bid"],
                                voxel_coord=live["voxel_coord"], grid_dims=(9, 9, 9), batch=B)

    return Entry({"ray_dir": d, "voxel_bound": vb, "ray_bid": rb, "voxel_bid": vbid, "voxel_coord": coord.int()}, call,
                 lambda got: _check_pairs(got, d.numpy(), vb.numpy(), rb.numpy(), vbid.numpy()),
                 zero=("ray_bid", "voxel_bid", "voxel_coord"),
                 reads_back="query.compute_ray_aabb: pair_off[-1].item() (P)")


def entry_pcl_aabb(dev, N=900, V=70):
    """pcl_aabb.forward / last_voxel (tests/test_boxes_gpu.py::test_pcl_aabb's scene and reference). Frame indices
    are compared, never used as indices: decoy zero. A NaN coordinate fails no comparison of the inclusive test."""
    from implicit_depth_amd.extensions import pcl_aabb
    from test_boxes_gpu import scene
    d, vb, rb, vbid = scene(N, V, 7 * N + V)
    pts = np.random.default_rng(5).uniform(-1.1, 1.1, size=(N, 3)).astype(np.float32)
    k = min(N, V)
    pts[:k] = vb[:k, :3]  # on a corner: inclusive bounds, several voxels may contain it

    def call(live):
        t = [live[k] for k in ("pts", "voxel_bound", "pcl_bid", "voxel_bid")]
        return {"mask": pcl_aabb.forward(*t), "last": pcl_aabb.last_voxel(*t)}

    def check(got):
        ref = orc.pcl_aabb(pts, vb, rb, vbid)
        assert (got["mask"].cpu().numpy() == ref).all()
        exp = np.where(ref.any(0), V - 1 - np.argmax(ref[::-1], axis=0), -1)
        assert (got["last"].cpu().numpy() == exp).all()

    return Entry({"pts": torch.from_numpy(pts), "voxel_bound": torch.from_numpy(vb), "pcl_bid": torch.from_numpy(rb),
                  "voxel_bid": torch.from_numpy(vbid)}, call, check, zero=("pcl_bid", "voxel_bid"))


def entry_get_miss_ray(dev, shape=(2, 16, 24)):
    from implicit_depth_amd.query import get_miss_ray
    from test_miss_ray_gpu import _check
    B, h, w = shape
    mask = torch.from_numpy((np.random.default_rng(h * w).random(shape) < 0.4).astype(np.uint8))
    fx, fy, cx, cy = [t.cpu() for t in intr(B, h, w, "cpu")]

    def call(live):
        return get_miss_ray(live["mask"], live["fx"], live["fy"], live["cx"], live["cy"])

    def check(got):
        ref = orc.get_miss_ray(mask, fx, fy, cx, cy)
        _check(got, {k: v.numpy() for k, v in ref.items() if torch.is_tensor(v)}, ref["total_miss_sample_num"])

    return Entry({"mask": mask, "fx": fx, "fy": fy, "cx": cx, "cy": cy}, call, check, zero=("mask",),
                 reads_back="query._compact_mask: cnt.item() (R)")


def entry_sample_valid_points(dev, n=40):
    """query.sample_valid_launch (the sampler without its optional host check). An all-zero mask is the documented
    check=False case, and (0, 0) is a valid (seed, counter)."""
    import sampler_ref as sr
    from implicit_depth_amd import query as Q
    from test_sample_valid_gpu import SEED
    mask_np = mask_2x16x24()
    bs, h, w = mask_np.shape

    def call(live):
        out = {"bid": torch.full((bs * n,), -7, dtype=torch.int32, device=dev),
               "flat": torch.full((bs * n,), -7, dtype=torch.int32, device=dev),
               "idx": torch.full((bs * n, 2), -7, dtype=torch.int64, device=dev),
               "cnt": torch.full((bs,), -7, dtype=torch.int32, device=dev)}
        Q.sample_valid_launch(live["mask"], n, live["state"], out["bid"], out["flat"], out["idx"], out["cnt"],
                              Q.sample_valid_workspace(bs, h, w, dev))
        out["state"] = live["state"]
        return out

    def check(got):
        want, want_cnt = sr.sample_valid_points(mask_np, n, SEED, 5)
        assert (got["cnt"].cpu().numpy() == want_cnt).all() and (got["idx"].cpu().numpy() == want).all()
        assert (got["bid"].cpu().numpy() == want[:, 0]).all() and (got["flat"].cpu().numpy() == want[:, 1]).all()
        sr.check_sample(mask_np, n, got["idx"].cpu().numpy())
        assert got["state"].cpu().tolist() == Q.sampler_state(SEED, "cpu", 6).tolist()

    return Entry({"mask": torch.from_numpy(mask_np), "state": Q.sampler_state(SEED, "cpu", 5)}, call, check,
                 zero=("mask", "state"))


def entry_sample_miss_window(dev, n=60):
    """query.sample_miss_window with the caller's state counter staged like an input."""
    import miss_window_ref as mw
    from implicit_depth_amd import query as Q
    from test_miss_window_gpu import _check
    mask_np = mask_2x16x24(seed=7)
    bs, h, w = mask_np.shape
    fx, fy, cx, cy = [t.cpu() for t in intr(bs, h, w, "cpu")]

    def call(live):
        out = Q.sample_miss_window(live["mask"], live["fx"], live["fy"], live["cx"], live["cy"], n, state=live["state"])
        return dict(out, state=live["state"])

    def check(got):
        got = dict(got)
        assert got.pop("state").cpu().tolist() == Q.sampler_state(3, "cpu", 2).tolist()
        _check(got, mask_np, torch.from_numpy(mask_np).to(dev), intr(bs, h, w, dev), n,
               mw.select(mask_np, n, seed=3, counter=1))

    return Entry({"mask": torch.from_numpy(mask_np), "fx": fx, "fy": fy, "cx": cx, "cy": cy,
                  "state": Q.sampler_state(3, "cpu", 1)}, call, check, zero=("mask", "state"),
                 reads_back="query.sample_miss_window: buf.pop('n_rays').tolist() (R_out, T)")


# -- inference -----------------------------------------------------------------------------------------------------
def entry_embed(dev, multires=8):
    """get_embedder's forward (tests/test_parity_gpu.py's embedding test: its points, reference and bound)."""
    from implicit_depth_amd import get_embedder
    g = torch.Generator().manual_seed(1)
    x = (torch.rand(1000, 3, generator=g) - 0.5) * 4.6
    x[0] = 0.0
    x[1] = torch.tensor([2.3, -2.3, 1e-7])
    fn, dim = get_embedder(multires)

    def call(live):
        with torch.no_grad():
            return fn(live["x"])

    def check(got):
        ref = orc.embed(x, multires)
        assert dim == ref.shape[1] == got.shape[1]
        assert (got.cpu() - ref).abs().max().item() <= 1e-6

    return Entry({"x": x}, call, check)


def entry_embed_backward(dev, multires=8):
    """The embedder under autograd (tests/test_train_gpu.py::test_embed_gradient: its points, reference and bound)."""
    from implicit_depth_amd import get_embedder
    fn, dim = get_embedder(multires)
    g = torch.Generator().manual_seed(3)
    x = (torch.rand(500, 3, generator=g) - 0.5) * 4.0
    wgt = torch.randn(500, dim, generator=g)

    def call(live):
        xd = live["x"].clone().requires_grad_(True)
        e = fn(xd)
        (e * live["wgt"]).sum().backward()
        return {"e": e.detach(), "grad": xd.grad}

    def check(got):
        xr = x.clone().double().requires_grad_(True)
        outs = [xr] + [f(xr * 2.0 ** o) for o in range(multires) for f in (torch.sin, torch.cos)]
        (torch.cat(outs, -1) * wgt.double()).sum().backward()
        assert got["e"].shape == (500, dim)
        scale = max(1.0, xr.grad.abs().max().item())
        assert (got["grad"].cpu().double() - xr.grad).abs().max().item() <= 2e-5 * scale

    return Entry({"x": x, "wgt": wgt}, call, check)


def entry_decoders_300_rows(dev, precision):
    from implicit_depth_amd import decoders_forward
    d = 385
    pp = orc.randomize_biases(orc.init_decoder("IMNET", d, 1, 5.0), 2)
    po = orc.randomize_biases(orc.init_decoder("IEF", d, 3, 5.0), 4)
    mp, mo = make_module("IMNET", pp, d, dev), make_module("IEF", po, d, dev)
    x = torch.randn(300, d, generator=torch.Generator().manual_seed(5))

    def call(live):
        with torch.no_grad():
            return decoders_forward(live["x"], mp, mo, precision=precision)

    def check(got):
        assert (got[0].cpu() - orc.imnet_forward(pp, x)).abs().max().item() <= TOL
        assert (got[1].cpu() - orc.ief_forward(po, x, 2)).abs().max().item() <= TOL

    return Entry({"x": x}, call, check, modules=(mp, mo))


def entry_decoder_chain(dev, gf, n=2049):
    """lidf_decoder_chain_f32 as test_decoder_chain_matches_the_layers holds it: the layer-by-layer path's own
    distance from float64 is the yardstick."""
    import copy
    import os
    from implicit_depth_amd import IEF, generic
    inp = 385
    torch.manual_seed(gf + inp)
    mod = IEF("cpu", inp, 1, gf, n_iter=2)
    for p in mod.parameters():
        p.data.mul_(6.0)
    ref_mod = copy.deepcopy(mod).double()
    ref_mod.init_offset = ref_mod.init_offset.double()
    mod = mod.to(dev).eval()
    mod.device, mod.init_offset = dev, mod.init_offset.to(dev)
    assert generic.chain_ok(mod)
    x = torch.randn(n, inp, generator=torch.Generator().manual_seed(n))

    def call(live):
        with torch.no_grad():
            return generic.decoder_forward(mod, live["x"])

    def check(got):
        with torch.no_grad():
            ref = ref_mod.forward_composite(x.double())
            old = os.environ.get("LIDF_CHAIN16")
            os.environ["LIDF_CHAIN16"] = "0"
            try:
                layers = generic.decoder_forward(mod, x.to(dev))
            finally:
                if old is None:
                    del os.environ["LIDF_CHAIN16"]
                else:
                    os.environ["LIDF_CHAIN16"] = old
        e_chain = float((got.double().cpu() - ref).abs().max())
        e_layers = float((layers.double().cpu() - ref).abs().max())
        assert e_chain <= max(1e-5, 1.5 * e_layers), (e_chain, e_layers)
        assert float((got - layers).abs().max()) <= 4e-5

    return Entry({"x": x}, call, check, modules=(mod,))


_SCENE_KEYS = ("ray_dir", "ray_pix", "ray_bid", "ray_flat", "pair_off", "pair_ray", "pair_vox", "pair_t", "feat_grid",
               "vox_feat", "vox_center")


def _scene_inputs(scene, keys=_SCENE_KEYS):
    return {k: scene[k] for k in keys if k in scene}


def entry_lidf_query(dev, precision="f32"):
    """lidf_query on the ragged 2 x 13 x 17 x 6 scene (index arrays keep their values as decoys: pair_ray, pair_vox,
    pair_off, ray_pix and ray_flat are indices)."""
    from implicit_depth_amd.query import lidf_query
    scene, ref = query_scene()
    D = scene["D"]
    prob, off = make_module("IMNET", scene["prob_p"], D, dev), make_module("IEF", scene["off_p"], D, dev)

    def call(live):
        depth = torch.zeros((scene["B"], scene["h"], scene["w"]), device=dev)
        with torch.no_grad():
            out = lidf_query(live["ray_dir"], live["ray_pix"], live["ray_bid"], live["pair_off"], live["pair_ray"],
                             live["pair_vox"], live["pair_t"], live["feat_grid"], live["vox_feat"], prob, off,
                             ray_flat=live["ray_flat"], depth=depth, precision=precision, want_rayfeat=True)
        out["depth"] = depth
        return {k: out[k] for k in QUERY_KEYS}

    return Entry(_scene_inputs(scene, _SCENE_KEYS[:-1]), call, lambda got: check_query(scene, ref, got),
                 modules=(prob, off))


def entry_lidf_query_shim(dev):
    """The same query through the pybind extension (csrc/lidf_torch_ext.cpp: its own getCurrentHIPStream), as
    tests/test_torch_ext_gpu.py calls it. decoder_weights() hands the parameters' own storage over, so the late
    weights arrive in it."""
    import os
    import pytest
    from implicit_depth_amd import torch_ext
    if not os.path.exists(torch_ext.EXT_PATH):     # (build() goes on without the shim when the host compiler fails)
        pytest.skip("the pybind shim was not built")
    m = torch_ext.ext()
    scene, ref = query_scene()
    D = scene["D"]
    prob, off = make_module("IMNET", scene["prob_p"], D, dev), make_module("IEF", scene["off_p"], D, dev)
    keys = ("pred_offset", "pred_prob_end", "pair_pred_pos", "pred_prob_end_softmax", "max_pair_id", "pred_pos")

    def call(live):
        pw, ow = torch_ext.decoder_weights(prob), torch_ext.decoder_weights(off)
        assert ({t.data_ptr() for t in pw + ow}
                == {p.data_ptr() for p in list(prob.parameters()) + list(off.parameters())})
        depth = torch.zeros((scene["B"], scene["h"], scene["w"]), device=dev)
        out = m.forward_query(live["ray_dir"], live["ray_pix"], live["ray_bid"], live["ray_flat"], live["pair_off"],
                              live["pair_ray"], live["pair_vox"], live["pair_t"], live["feat_grid"], live["vox_feat"],
                              None, pw, ow, 2, 0.001, False, 8, 4, 8, False, 0.0, 1.0, 0.25, depth, 0)
        res = dict(zip(keys, out))
        res["depth"] = depth
        return res

    inputs = _scene_inputs(scene, _SCENE_KEYS[:-1])
    for k in ("ray_pix", "ray_bid", "ray_flat"):
        inputs[k] = inputs[k].long()
    return Entry(inputs, call, lambda got: check_query(scene, ref, got), modules=(prob, off))


def entry_lidf_query_generic_gf32(dev):
    from implicit_depth_amd import IEF, IMNet, generic
    from implicit_depth_amd.query import lidf_query
    scene, ref = query_scene_gf32()
    D = scene["D"]
    prob, off = IMNet(D, 1, 32), IEF(dev, D, 1, 32, n_iter=2)
    prob.load_state_dict(scene["prob_p"]), off.load_state_dict(scene["off_p"])
    prob, off = prob.to(dev).eval(), off.to(dev).eval()
    assert generic.chain_ok(prob) and generic.chain_ok(off)

    def call(live):
        depth = torch.zeros((scene["B"], scene["h"], scene["w"]), device=dev)
        with torch.no_grad():
            out = lidf_query(live["ray_dir"], live["ray_pix"], live["ray_bid"], live["pair_off"], live["pair_ray"],
                             live["pair_vox"], live["pair_t"], live["feat_grid"], live["vox_feat"], prob, off,
                             ray_flat=live["ray_flat"], depth=depth)
        out["depth"] = depth
        return {k: out[k] for k in QUERY_KEYS if k in out}

    return Entry(_scene_inputs(scene, _SCENE_KEYS[:-1]), call, lambda got: check_query(scene, ref, got),
                 modules=(prob, off))


def entry_pointnet_inference(dev, n, v):
    p, inp, vox, ref = pointnet_case(n, v)
    m = make_pointnet(p, dev)

    def call(live):
        with torch.no_grad():
            return m(live["inp"], live["vox"], n_vox=v)

    def check(got):
        assert got.shape == ref.shape and (got.cpu() - ref).abs().max().item() <= 2e-5

    return Entry({"inp": inp, "vox": vox}, call, check, modules=(m,))


def entry_lidf_refine(dev, cell_table):
    """lidf_refine, two iterations, from the product's own stage 1 (computed once on the default stream, then an
    input like any other). A NaN position is a documented input of both end-voxel kernels (lidf_refine.hip: such a
    ray walks the voxel list); every index array keeps its values."""
    from implicit_depth_amd.query import lidf_query, lidf_refine
    from implicit_depth_amd.synthetic import GRID_RES, GRID_XMIN, PART_SIZE
    from util import to_dev
    scene, vb, vbid, rgb, valid_inp, valid_vox, pnet_p, offr_p = refine_case()
    s = to_dev(scene, dev)
    D = scene["D"]
    prob, off = make_module("IMNET", scene["prob_p"], D, dev), make_module("IEF", scene["off_p"], D, dev)
    pnet, offr = make_pointnet(pnet_p, dev), make_module("IEF", offr_p, 334, dev)
    with torch.no_grad():
        s1 = lidf_query(s["ray_dir"], s["ray_pix"], s["ray_bid"], s["pair_off"], s["pair_ray"], s["pair_vox"],
                        s["pair_t"], s["feat_grid"], s["vox_feat"], prob, off)
    torch.cuda.synchronize(dev)
    pos1, mid1 = s1["pred_pos"].cpu(), s1["max_pair_id"].cpu()
    inputs = {k: scene[k] for k in ("ray_dir", "ray_pix", "ray_bid", "ray_flat", "pair_vox", "feat_grid")}
    inputs.update(pred_pos=pos1, max_pair_id=mid1, voxel_bound=vb, voxel_bid=vbid, rgb=rgb, valid_inp=valid_inp,
                  valid_vox=valid_vox)
    if cell_table:
        ci = torch.arange(GRID_RES)
        inputs["voxel_coord"] = torch.stack(torch.meshgrid(ci, ci, ci, indexing="ij"), -1).reshape(-1, 3).repeat(
            2, 1).int().contiguous()

    def call(live):
        grid = {"xmin": torch.tensor(GRID_XMIN), "grid_dims": (GRID_RES,) * 3, "part_size": PART_SIZE,
                "voxel_coord": live["voxel_coord"]} if cell_table else None
        with torch.no_grad():
            return lidf_refine(live["ray_dir"], live["ray_pix"], live["ray_bid"], live["ray_flat"], live["pred_pos"],
                               live["max_pair_id"], live["pair_vox"], live["voxel_bound"], live["voxel_bid"],
                               live["rgb"], live["feat_grid"], live["valid_inp"], live["valid_vox"], pnet, offr,
                               forward_times=2, grid=grid)

    def check(got):
        pos, ev = refine_oracle(pos1, mid1)
        assert (got[0].cpu() - pos).abs().max().item() <= TOL
        assert (got[1].cpu().long() == ev).all()

    return Entry(inputs, call, check, modules=(pnet, offr))


def entry_depth_metrics(dev, h=37, w=53):
    """depth_metrics at the source resolution (test_metrics_gpu's maps and bound). The zeroed workspace is kept per
    (device, stream): a fresh stream meets a fresh one."""
    from implicit_depth_amd import query as Q
    from test_metrics_gpu import _maps
    pred, gt, seg = _maps(h, w, seed=h + w)

    def call(live):
        out = Q.depth_metrics(live["pred"], live["gt"], live["seg"], None)
        return {k: out[k] for k in Q.METRIC_NAMES + ("count",)}

    def check(got):
        ref = orc.depth_metrics(pred, gt, seg, None)
        assert float(got["count"]) == float(ref["count"])
        for k in Q.METRIC_NAMES:
            r, v = float(ref[k]), float(got[k])
            assert abs(v - r) <= 2e-6 * max(1.0, abs(r)), (k, v, r)

    return Entry({"pred": pred, "gt": gt, "seg": seg}, call, check, zero=("seg",))


# -- training ------------------------------------------------------------------------------------------------------
def _zero_grads(*mods):
    for m in mods:
        for q in m.parameters():
            q.grad = None


def entry_decoder_training_320_rows(dev, n=320):
    """Forward with kept activations + backward of one IEF (tests/test_f64_gpu.py::test_decoder_module_backward at
    320 rows)."""
    from test_f64_gpu import _masked_weights
    d = 385
    p = orc.randomize_biases(orc.init_decoder("IEF", d, 31, 5.0), 32)
    m = make_module("IEF", p, d, dev).train()
    gen = torch.Generator().manual_seed(n)
    x = torch.randn(n, d, generator=gen)
    w = _masked_weights(p, x.to(dev), "IEF", n, gen, dev).cpu()

    def call(live):
        _zero_grads(m)
        xg = live["x"].clone().requires_grad_(True)
        y = m(xg)
        (y.reshape(-1) * live["w"]).sum().backward()
        out = {k: q.grad for k, q in m.named_parameters()}
        out.update(input=xg.grad, y=y.detach())
        return out

    def check(got):
        xd, wd = x.to(dev), w.to(dev)
        _, g64 = oracle_grads(p, xd, "IEF", wd, torch.float64)
        _, g32 = oracle_grads(p, xd, "IEF", wd, torch.float32)
        for k in g64:
            assert_f64_close("IEF n=%d d%s" % (n, k), got[k], g64[k], g32[k], k=k_for(k))

    return Entry({"x": x, "w": w}, call, check, modules=(m,))


def entry_decoder_pair_node_320_rows(dev, n=320):
    """decoders_forward_train (tests/test_f64_gpu.py::test_decoder_pair_node_backward at 320 rows)."""
    from implicit_depth_amd import decoders_forward_train
    from test_f64_gpu import _check_decoder_out, _masked_weights
    d = 385
    pp = orc.randomize_biases(orc.init_decoder("IMNET", d, 21, 5.0), 22)
    po = orc.randomize_biases(orc.init_decoder("IEF", d, 23, 5.0), 24)
    prob, off = make_module("IMNET", pp, d, dev).train(), make_module("IEF", po, d, dev).train()
    gen = torch.Generator().manual_seed(n + d)
    x = torch.randn(n, d, generator=gen)
    wp = _masked_weights(pp, x.to(dev), "IMNET", n, gen, dev).cpu()
    wo = _masked_weights(po, x.to(dev), "IEF", n, gen, dev).cpu()

    def call(live):
        _zero_grads(prob, off)
        xg = live["x"].clone().requires_grad_(True)
        yp, yo = decoders_forward_train(xg, prob, off)
        ((yp.reshape(-1) * live["wp"]).sum() + (yo.reshape(-1) * live["wo"]).sum()).backward()
        out = {"prob." + k: q.grad for k, q in prob.named_parameters()}
        out.update({"off." + k: q.grad for k, q in off.named_parameters()})
        out.update(input=xg.grad, yp=yp.detach(), yo=yo.detach())
        return out

    def check(got):
        xd, wpd, wod = x.to(dev), wp.to(dev), wo.to(dev)
        refs = {}
        for dt in (torch.float64, torch.float32):
            yp_r, gp = oracle_grads(pp, xd, "IMNET", wpd, dt)
            yo_r, go = oracle_grads(po, xd, "IEF", wod, dt)
            g = {"prob." + k: v for k, v in gp.items() if k != "input"}
            g.update({"off." + k: v for k, v in go.items() if k != "input"})
            g["input"] = gp["input"] + go["input"]
            refs[dt] = (yp_r, yo_r, g)
        _check_decoder_out("pair prob", got["yp"], refs[torch.float64][0], refs[torch.float32][0], False)
        _check_decoder_out("pair off", got["yo"], refs[torch.float64][1], refs[torch.float32][1], False)
        for k in refs[torch.float64][2]:
            assert_f64_close("pair d%s" % k, got[k], refs[torch.float64][2][k], refs[torch.float32][2][k], k=k_for(k))

    return Entry({"x": x, "wp": wp, "wo": wo}, call, check, modules=(prob, off))


def entry_lidf_query_train(dev, factorised, offsets):
    """lidf_query_train forward + backward on the ragged 2 x 12 x 16 x 8 scene. The factorised path owns the training
    side stream (query._train_side_stream): lidf_pe_rows_f32 in the forward, offset_dec's backward."""
    from implicit_depth_amd import query as Q
    sel = offsets == "selected"
    scene, w, ref, gref = query_train_case(sel)
    D = scene["D"]
    kw = dict(offset_range=(-0.2, 0.2), part_size=0.25, pos_rel=True, factorised=factorised, offsets=offsets)
    prob = make_module("IMNET", scene["prob_p"], D, dev).train()
    off = make_module("IEF", scene["off_p"], D, dev).train()
    inputs = _scene_inputs(scene)
    del inputs["ray_flat"]
    inputs.update({"w_" + k: v for k, v in w.items()})

    def call(live):
        _zero_grads(prob, off)
        fgd = live["feat_grid"].clone().requires_grad_(True)
        vfd = live["vox_feat"].clone().requires_grad_(True)
        out = Q.lidf_query_train(live["ray_dir"], live["ray_pix"], live["ray_bid"], live["pair_off"], live["pair_ray"],
                                 live["pair_vox"], live["pair_t"], fgd, vfd, prob, off, vox_center=live["vox_center"],
                                 **kw)
        query_loss(out, {k: live["w_" + k] for k in w}, sel).backward()
        res = {k: out[k].detach() for k in ("pred_offset", "pred_prob_end", "pair_pred_pos", "pred_pos", "max_pair_id")}
        res.update({"feat_grid": fgd.grad, "vox_feat": vfd.grad})
        res.update({"prob." + k: v.grad for k, v in prob.named_parameters()})
        res.update({"off." + k: v.grad for k, v in off.named_parameters()})
        return res

    def check(got):
        mid = got["max_pair_id"].cpu()
        live_rows = mid[mid < scene["P"]]
        for k in ("pred_prob_end", "pred_pos"):
            assert (got[k].cpu() - ref[k]).abs().max().item() <= TOL, k
        for k in ("pred_offset", "pair_pred_pos"):
            rows = live_rows if sel else slice(None)
            assert (got[k].cpu()[rows] - ref[k][rows]).abs().max().item() <= TOL, k
        for k, g in gref.items():
            close_rel(got[k].cpu(), g, k, 5e-4, 1e-2)

    loose = {"feat_grid": _feat_grid_loose}
    if not factorised:
        loose["vox_feat"] = _held_by_reference
    return Entry(inputs, call, check, modules=(prob, off), loose=loose,
                 side=(lambda: Q._train_side_stream(dev)) if factorised else None)


def entry_pointnet_training(dev, n, v):
    """tests/test_train_gpu.py::test_pointnet_gradients' reference and bounds."""
    p, inp, vox, wgt, ref, grads = pointnet_train_case(n, v)
    m = make_pointnet(p, dev).train()

    def call(live):
        _zero_grads(m)
        xd = live["inp"].clone().requires_grad_(True)
        out = m(xd, live["vox"], n_vox=v)
        (out * live["wgt"]).sum().backward()
        res = {k: q.grad for k, q in m.named_parameters()}
        res.update(inp=xd.grad, out=out.detach())
        return res

    def check(got):
        assert (got["out"].cpu() - ref).abs().max().item() <= 2e-5
        for k, g in grads.items():
            close_rel(got[k].cpu(), g, k, 5e-4, 1e-2)

    return Entry({"inp": inp, "vox": vox, "wgt": wgt}, call, check, modules=(m,))


def entry_topk_mean_five_jobs(dev):
    """lidf_topk_mean_f32, five jobs in one call (tests/test_hard_neg_gpu.py::test_five_jobs_in_one_call). NaN values
    are a tested input of the select kernel (pattern 'special'), and so is a device count of zero."""
    from implicit_depth_amd import _lib
    from test_hard_neg_gpu import _check, _pattern
    L = _lib.lib()
    ns = [1, 257, 4097, 10000, 65]
    pats = ["uniform", "five_values", "last_digit", "uniform", "signed_zeros"]
    ratio = 0.3
    vals = [_pattern(p, n) for p, n in zip(pats, ns)]
    vals[3][np.random.default_rng(5).random(ns[3]) < 0.8] = -np.inf
    count3 = int(np.isfinite(vals[3]).sum())
    inputs = {"v%d" % i: torch.from_numpy(v) for i, v in enumerate(vals)}
    inputs["count3"] = torch.tensor([count3], dtype=torch.int32)

    def call(live):
        dw = [torch.full((n,), 5.0, device=dev) for n in ns]
        means = torch.full((5,), 123.0, device=dev)
        jobs = (_lib.LidfTopkJob * 5)()
        for i in range(5):
            jobs[i] = _lib.LidfTopkJob(live["v%d" % i].data_ptr(), ns[i], live["count3"].data_ptr() if i == 3 else None,
                                       means[i:].data_ptr(), dw[i].data_ptr())
        wsb = L.lidf_topk_mean_workspace_bytes(5, max(ns))
        ws = _lib.workspace(wsb, dev)
        with torch.cuda.device(dev):
            _lib.check(L.lidf_topk_mean_f32(jobs, 5, ratio, _lib.ptr(ws), wsb, _lib.current_stream(dev)))
        return {"means": means, "weights": dw}

    def check(got):
        for i in range(5):
            _check(got["means"][i], got["weights"][i], vals[i], ratio, count3 if i == 3 else None, what="job %d" % i)

    return Entry(inputs, call, check, zero=("count3",))


def entry_eval_loss(dev, stage):
    """The evaluation-flavour loss of one stage on the ragged 3 x 20 x 27 case (tests/test_eval_loss_gpu.py)."""
    import eval_loss_ref as el
    from test_eval_loss_gpu import _check, _product_dd, _run
    d = el.random_case(3, 20, 27, 0.6, seed=5)
    opt = dict(smooth_w=0.5)
    dd0 = _product_dd(d, "cpu")
    keys = [k for k, v in dd0.items() if torch.is_tensor(v)]

    def call(live):
        dd = dict(dd0)
        dd.update({k: live[k] for k in keys})
        return _run(dd, stage, "valid", **opt)

    return Entry({k: dd0[k] for k in keys}, call, lambda got: _check("3x20x27", got, d, stage, None, **opt),
                 zero=("corrupt_mask",))


# -- the whole frame -----------------------------------------------------------------------------------------------
def entry_frame_runner(dev, side_stream, graph):
    """pipeline.FrameRunner on the (2, 48, 64) batch of test_frame_equals_stepwise_path, one runner for every run of
    the case (its workspace, buffers and packed weight streams persist, as in a trainer's evaluation loop). The
    valid mask (depth_corrupt under mask_type 'all') is zero as a decoy — a frame without valid points is the
    reference's early exit, which the library runs on empty lists; the frame's voxel build drops NaN points like
    lidf_vox_mark_kernel, its pair list is cut at max_pairs, and stage 2 takes NaN positions (lidf_refine.hip).
    side_stream=True owns FrameRunner.side[0] (created by the warm-up frame)."""
    from implicit_depth_amd import pipeline as pl
    from implicit_depth_amd.synthetic import synthetic_batch
    from test_frame_gpu import SAME, SAME_INT, _compare, _dev, _models, _stepwise
    B, h, w = 2, 48, 64
    models = _models(dev)
    opt = pl.LidfOptions(valid_stride=None, refine_use_all_pix=False)
    batch, feat = synthetic_batch(B, h, w, seed=78, hole_frac=1.9)
    keys = ("rgb", "xyz_corrupt", "depth_corrupt", "fx", "fy", "cx", "cy")
    runner = pl.FrameRunner(B, h, w, dev, models[0], models[1], models[2], opt, models[3], models[4],
                            side_stream=side_stream)
    if graph:
        with torch.no_grad():
            runner.load(_dev(batch, dev), feat.to(dev))
            runner.capture()
        torch.cuda.synchronize(dev)

    def call(live):
        with torch.no_grad():
            runner.run({k: live[k] for k in keys}, live["feat"])
        return dict(runner.buf)

    def finish(res):          # FrameRunner.result() on the cloned buffers: cut to the counts the device wrote
        real, runner.buf = runner.buf, res
        try:
            ok, dd = runner.result()
        finally:
            runner.buf = real
        assert ok, dd["counts"]
        return {k: dd[k] for k in SAME + SAME_INT + ("counts",)}

    def check(got):
        ok, step = _stepwise(_dev(batch, dev), feat.to(dev), models, opt)
        torch.cuda.synchronize(dev)
        assert ok
        _compare(got, step)

    inputs = {k: batch[k] for k in keys}
    inputs["feat"] = feat
    return Entry(inputs, call, check, modules=models, zero=("depth_corrupt",), finish=finish,
                 side=(lambda: runner.side[0]) if side_stream else None)


# -- stage 2 and the whole training steps --------------------------------------------------------------------------
def refine_train_scene(dev):
    """tests/test_train_gpu.py::test_refine_train_fused_step_vs_composed's scene (cell table on): host tensors, plus
    the occupied voxels of its points as get_occ_vox_bound builds them on `dev` (occ, vb, vbid)."""
    from implicit_depth_amd.query import get_occ_vox_bound
    g = torch.Generator().manual_seed(17)
    B, h, w, R, P = 2, 20, 24, 700, 900
    pts = torch.rand(600, 3, generator=g) * torch.tensor([1.6, 1.6, 1.6]) + torch.tensor([-0.8, -0.8, 0.2])
    pb = torch.randint(0, B, (600,), generator=g).int()
    occ = get_occ_vox_bound(pts.to(dev), pb.to(dev), B, res=8)
    vb, vbid = occ["voxel_bound"], occ["occ_vox_bid"].int().contiguous()
    V = vb.shape[0]
    bid = torch.randint(0, B, (R,), generator=g)
    ctr = ((vb[:, :3] + vb[:, 3:]) / 2).cpu()
    own = [torch.nonzero(vbid.cpu() == b)[:, 0] for b in range(B)]
    pick = torch.stack([own[int(b)][torch.randint(0, own[int(b)].numel(), (1,), generator=g)][0] for b in bid])
    pos0 = ctr[pick] + (torch.rand(R, 3, generator=g) - 0.5) * 0.3
    ray_dir = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=1)
    flat = torch.randint(0, h * w, (R,), generator=g)
    ray_pix = torch.stack((flat % w, flat // w), 1).int()
    pair_vox = torch.randint(0, V, (P,), generator=g).int()
    mid = torch.randint(0, P + 1, (R,), generator=g)
    rgb, feat = torch.randn(B, 3, h, w, generator=g), torch.randn(B, 32, h, w, generator=g)
    valid_inp = torch.randn(500, 6, generator=g) * 0.2
    valid_vox = torch.randint(0, V, (500,), generator=g).int()
    wgt = torch.randn(R, 3, generator=g)
    pnet_p = orc.init_pointnet(5, 1.5)
    dec_p = orc.randomize_biases(orc.init_decoder("IEF", 334, 77, 5.0), 78)
    return dict(B=B, h=h, w=w, R=R, P=P, occ=occ, vb=vb, vbid=vbid, V=V, bid=bid, pos0=pos0, ray_dir=ray_dir, flat=flat,
                ray_pix=ray_pix, pair_vox=pair_vox, mid=mid, rgb=rgb, feat=feat, valid_inp=valid_inp,
                valid_vox=valid_vox, wgt=wgt, pnet_p=pnet_p, dec_p=dec_p)


def entry_lidf_refine_train(dev):
    """lidf_refine_train, forward and backward, three iterations with the cell table, against the step composed from
    the modules' own autograd functions (test_workspace_gpu.py::test_lidf_refine_train's bounds). NaN positions are a
    documented input of the end-voxel kernels; every index array and the grid keep their values."""
    from implicit_depth_amd.query import _lidf_refine_train_composed, lidf_refine_train
    sc = refine_train_scene(dev)
    torch.cuda.synchronize(dev)
    occ = sc["occ"]
    xmin = occ["xmin"].cpu()          # (a host tensor: the grid's origin is read on the host, query._refine_cells)
    pnet, dec = make_pointnet(sc["pnet_p"], dev).train(), make_module("IEF", sc["dec_p"], 334, dev).train()
    inputs = {"ray_dir": sc["ray_dir"], "ray_pix": sc["ray_pix"], "bid": sc["bid"].int(), "flat": sc["flat"].int(),
              "pos0": sc["pos0"], "mid": sc["mid"], "pair_vox": sc["pair_vox"], "vb": sc["vb"].cpu(),
              "vbid": sc["vbid"].cpu(), "rgb": sc["rgb"], "feat": sc["feat"], "valid_inp": sc["valid_inp"],
              "valid_vox": sc["valid_vox"], "wgt": sc["wgt"], "voxel_coord": occ["voxel_coord"].cpu()}

    def step(fn, live, **kw):
        _zero_grads(pnet, dec)
        pp = live["pos0"].clone().requires_grad_(True)
        fg = live["feat"].clone().requires_grad_(True)
        got, ev = fn(live["ray_dir"], live["ray_pix"], live["bid"], live["flat"], pp, live["mid"], live["pair_vox"],
                     live["vb"], live["vbid"], live["rgb"], fg, live["valid_inp"], live["valid_vox"], pnet, dec,
                     forward_times=3, pos_rel=True, pnet_pos_rel=False, perturb_noise=0.03, **kw)
        (got * live["wgt"]).sum().backward()
        res = {"pos": got.detach(), "ev": ev, "pred_pos": pp.grad, "feat_grid": fg.grad}
        res.update({"pnet." + k: q.grad for k, q in pnet.named_parameters()})
        res.update({"dec." + k: q.grad for k, q in dec.named_parameters()})
        return res

    def call(live):
        return step(lidf_refine_train, live, grid=dict(occ, xmin=xmin, voxel_coord=live["voxel_coord"]))

    def check(got):
        live = {k: v.to(dev) for k, v in inputs.items()}
        ref = {k: v.clone() for k, v in step(_lidf_refine_train_composed, live).items()}
        torch.cuda.synchronize(dev)
        assert torch.equal(got["ev"], ref["ev"])
        assert (got["pos"] - ref["pos"]).abs().max().item() <= TOL
        for k, gr in ref.items():
            if k not in ("pos", "ev"):
                err = (got[k] - gr).abs().max().item()
                assert err <= 1e-3 * max(gr.abs().max().item(), 1e-3), (k, err, gr.abs().max().item())

    def feat_loose(a, b):     # border taps are float atomics: the existing test's two-run bound
        assert (a - b).abs().max().item() <= 1e-5 * max(b.abs().max().item(), 1e-3)

    return Entry(inputs, call, check, modules=(pnet, dec), loose={"feat_grid": feat_loose})


class _Grads:
    """Stands in for a module in the existing tests' checks: named_parameters() over cloned gradients."""

    def __init__(self, grads):
        self.grads = grads

    def named_parameters(self):
        import types
        return [(k, types.SimpleNamespace(grad=g)) for k, g in self.grads.items()]


_BATCH_MASKS = ("depth_corrupt", "corrupt_mask", "valid_mask")
_STEP_READS = ("pipeline._train_geometry: the size reads of query._compact_mask (cnt.item()), get_occ_vox_bound "
               "(counts.tolist()) and compute_ray_aabb (pair_off[-1].item())")


def entry_stage1_training_step(dev, name="e0"):
    """pipeline.lidf_forward_train + backward on the g9 fixture (test_train_step_gpu.py::
    test_whole_step_against_the_reference). The step's first launch is the mark pass of the valid mask, followed by
    a size read: a zero mask ends the step at the reference's first early exit, and every later launch follows a
    host wait on the caller's stream."""
    import train_loss_ref as tl
    from implicit_depth_amd import LidfLossOptions, LidfOptions, lidf_forward_train
    from test_train_step_gpu import _close, _g9_modules, _zero_bias_bound
    g, gp = tl.g9_files()
    d, ref = tl.g9_case(g, name)
    epoch, opt = tl.g9_opt(name)
    batch, feat = tl.g9_batch(g)
    mods = _g9_modules(g, dev)
    keys = [k for k, v in batch.items() if torch.is_tensor(v)]
    inputs = {k: batch[k] for k in keys}
    inputs["full_rgb_feat"] = feat
    names = ("pnet_model", "prob_dec", "offset_dec")

    def call(live):
        _zero_grads(*mods)
        b = dict(batch)
        b.update({k: live[k] for k in keys})
        fg = live["full_rgb_feat"].clone().requires_grad_(True)
        np.random.seed(int(g["np_seed"]))   # (sample_miss_rays draws the window as the reference does)
        ok, dd, loss = lidf_forward_train(b, fg, *mods, opt=LidfOptions(miss_sample_num=int(g["miss_sample_num"])),
                                          loss_opt=LidfLossOptions(**opt), epoch=epoch)
        assert ok
        loss["loss_net"].backward()
        res = {"loss": {k: v.detach() for k, v in loss.items()}, "full_rgb_feat": fg.grad,
               "dd": {k: dd[k].detach() for k in ("pred_pos", "pred_prob_end", "miss_bid", "miss_flat_img_id",
                                                  "pair_ray")}}
        res.update({n: {k: q.grad for k, q in m.named_parameters()} for n, m in zip(names, mods)})
        return res

    def check(got):
        dd, loss = got["dd"], got["loss"]
        assert torch.equal(dd["miss_bid"].cpu(), d["miss_bid"]) and torch.equal(dd["miss_flat_img_id"].cpu(), d["miss_flat"])
        assert dd["pair_ray"].shape[0] == d["pair_ray"].shape[0]
        bad = []
        for i, k in enumerate(tl.LOSS_KEYS):
            _close(loss[k].cpu(), ref["loss"][i], (name, k), bad)
        _close(got["full_rgb_feat"].cpu(), ref["g_full_rgb_feat"], (name, "full_rgb_feat"), bad)
        stride = int(g["param_stride"])
        for mod in names:
            for k, grad in got[mod].items():
                want = torch.from_numpy(gp["%s_g_%s.%s" % (name, mod, k)])
                have = grad.cpu().reshape(-1)
                have = have[::stride] if have.numel() > 4096 else have
                if (mod, k) == ("prob_dec", "linear_4.bias"):
                    assert abs(float(have)) <= _zero_bias_bound(d["pair_ray"].shape[0])
                    continue
                _close(have, want, (name, mod, k), bad)
        assert not bad, bad

    return Entry(inputs, call, check, modules=mods, zero=_BATCH_MASKS, loose={"full_rgb_feat": _feat_grid_loose},
                 reads_back=_STEP_READS)


def entry_refine_training_step(dev, name="plain"):
    """pipeline.train_refine_step + backward on the g10 fixture (test_refine_train_step_gpu.py::
    test_whole_step_against_the_reference); decoys as for the stage-1 step."""
    import refine_loss_ref as rl
    from implicit_depth_amd import LidfLossOptions, LidfOptions, train_refine_step
    from test_refine_train_step_gpu import _check_step, _g10_modules
    g, gp = rl.g10_files()
    d, ref = rl.g10_case(g, name)
    batch, feat = rl.g10_batch(g)
    opt = LidfOptions(miss_sample_num=int(g["miss_sample_num"]), maxpool_label_epo=0)
    loss_opt = LidfLossOptions(prob_w=0.0, **rl.G10_CASES[name])   # (train_refine.yaml: one loss section, prob_w 0)
    mods, mods_r = _g10_modules(g, dev)
    keys = [k for k, v in batch.items() if torch.is_tensor(v)]
    inputs = {k: batch[k] for k in keys}
    inputs["full_rgb_feat"] = feat

    def call(live):
        _zero_grads(*mods, *mods_r)
        b = dict(batch)
        b.update({k: live[k] for k in keys})
        np.random.seed(ref["np_seed"])
        ok, dd, loss1, loss = train_refine_step(b, live["full_rgb_feat"], *mods, *mods_r, opt=opt, loss_opt=loss_opt,
                                                epoch=int(g["epoch"]))
        assert ok
        loss["loss_net"].backward()
        return {"loss": {k: v.detach() for k, v in loss.items()}, "loss1": {k: v.detach() for k, v in loss1.items()},
                "dd": {k: (dd[k].detach() if torch.is_tensor(dd[k]) else dd[k])
                       for k in ("pred_pos", "pred_pos_refine", "end_voxel_id", "miss_bid", "miss_flat_img_id",
                                 "pair_ray", "refine_perturb_noise")},
                "grads": [{k: q.grad for k, q in m.named_parameters()} for m in mods_r]}

    def check(got):
        assert (got["dd"]["pred_pos"].cpu() - d["pred_pos"]).abs().max().item() <= TOL
        _check_step(g, gp, name, got["dd"], got["loss"], [_Grads(gr) for gr in got["grads"]], ref, d)

    return Entry(inputs, call, check, modules=tuple(mods) + tuple(mods_r), zero=_BATCH_MASKS, reads_back=_STEP_READS)


def entry_stage1_loss_device_select(dev, name="e0_hn"):
    """compute_gt + lidf_loss forward + backward with hard-negative mining on the device
    (test_hard_neg_gpu.py::test_lidf_loss_device_route_on_the_fixture's reference and bounds)."""
    import train_loss_ref as tl
    from implicit_depth_amd import LidfLossOptions, lidf_loss
    from implicit_depth_amd.losses import compute_gt
    from test_hard_neg_gpu import _stage1_dd
    g, _ = tl.g9_files()
    d, ref = tl.g9_case(g, name)
    epoch, opt = tl.g9_opt(name)
    dd0, order = _stage1_dd(d, "cpu")
    keys = [k for k, v in dd0.items() if torch.is_tensor(v)]

    def call(live):
        dd = dict(dd0)
        dd.update({k: live[k] for k in keys})
        for k in ("pred_pos", "pred_prob_end"):
            dd[k] = live[k].clone().requires_grad_(True)
        compute_gt(dd)
        out = lidf_loss(dd, LidfLossOptions(hard_neg_select="device", **opt), "train", epoch)
        out["loss_net"].backward()
        res = {k: v.detach() for k, v in out.items()}
        res.update(g_pred_pos=dd["pred_pos"].grad, g_logit=dd["pred_prob_end"].grad)
        return res

    def check(got):
        loss64, gp64, gl64 = tl.loss_and_grads(d, torch.float64, epoch, **opt)
        inv = torch.empty_like(order)
        inv[order] = torch.arange(inv.shape[0])
        for i, k in enumerate(tl.LOSS_KEYS):
            assert_f64_close("g9 %s %s" % (name, k), got[k].cpu().reshape(1), loss64[i].reshape(1),
                             ref["loss"][i].reshape(1))
        assert_f64_close("g9 g_pred_pos", got["g_pred_pos"].cpu(), gp64, ref["g_pred_pos"])
        assert_f64_close("g9 g_pred_prob_end", got["g_logit"].cpu()[inv], gl64, ref["g_pred_prob_end"])

    return Entry({k: dd0[k].detach() for k in keys}, call, check)


def entry_refine_loss_device_select(dev):
    """refine_loss forward + backward with hard-negative mining on the device
    (test_hard_neg_gpu.py::test_refine_loss_device_route_on_the_fixture's reference and bounds)."""
    import refine_loss_ref as rl
    from implicit_depth_amd import LidfLossOptions, refine_loss
    from test_hard_neg_gpu import _refine_dd
    g, _ = rl.g10_files()
    d, ref = rl.g10_case(g, "hn")
    epoch, opt = int(g["epoch"]), rl.G10_CASES["hn"]
    dd0 = _refine_dd(d, "cpu")
    keys = [k for k, v in dd0.items() if torch.is_tensor(v)]

    def call(live):
        dd = dict(dd0)
        dd.update({k: live[k] for k in keys})
        dd["pred_pos_refine"] = live["pred_pos_refine"].clone().requires_grad_(True)
        out = refine_loss(dd, LidfLossOptions(hard_neg_select="device", **opt), "train", epoch)
        out["loss_net"].backward()
        res = {k: v.detach() for k, v in out.items()}
        res["g_pred_pos_refine"] = dd["pred_pos_refine"].grad
        return res

    def check(got):
        loss64, gp64 = rl.loss_and_grad(d, torch.float64, epoch, 1.0, **opt)
        for i, k in enumerate(rl.REFINE_LOSS_KEYS):
            assert_f64_close("g10 hn %s" % k, got[k].cpu().reshape(1), loss64[i].reshape(1), ref["loss"][i].reshape(1))
        assert_f64_close("g10 hn g_pred_pos_refine", got["g_pred_pos_refine"].cpu(), gp64, ref["g_pred_pos_refine"])

    return Entry({k: dd0[k].detach() for k in keys}, call, check)
