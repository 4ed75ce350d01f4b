"""Stage 2 against float64 references (util.assert_f64_close, as tests/test_f64_gpu.py does for stage 1): PointNet2Stage
under autograd (lidf_pointnet_train.hip: forward chains, backward phases A and B, lidf_pnet_dw4_kernel, the chunked
per-voxel sums), the refine inference call and the refine training step, fused (lidf_refine_train, one node) and
composed. The float32 oracle's own error against float64 on the same inputs is the unit; the HIP result may be
F64_K = 4 times less accurate (bias gradients K_BIAS = 6), elementwise and normwise.

The inputs are conditioned (tests/pointnet_ref.py): points at a ReLU kink or at a near-tie of a pooling, and rays
at a decoder kink or at a voxel face, are dropped until the float64 evaluation flags none, so that rounding
decides no route and the unit is rounding error alone (tests/test_pointnet_ref.py checks that on the CPU). Exact
ties are checked on their own against torch_scatter's rule, the lowest row."""
import functools
import gc

import pytest
import torch

import pointnet_ref as ref
from util import assert_f64_close, f64, k_for, make_module, make_pointnet, orc, tf32_off

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _full_precision_references():
    with tf32_off():
        yield
    gc.collect()
    torch.cuda.empty_cache()


def _check_all(tag, got, r64, r32):
    """assert_f64_close on every tensor of r64 (every ratio is printed), then one assertion naming all that fail."""
    failed, report = [], []
    for k in r64:
        try:
            assert_f64_close("%s %s" % (tag, k), got[k], r64[k], r32[k], k=k_for(k), report=report)
        except AssertionError as e:
            failed.append(str(e))
    print("%s: worst ratio elementwise %.2f / normwise %.2f" % (tag, max(r["ratio_max"] for r in report),
                                                                  max(r["ratio_nrm"] for r in report)))
    assert not failed, "\n".join(failed)


# ---------------------------------------------------------------------------------------------------------------
# PointNet2Stage under autograd
# ---------------------------------------------------------------------------------------------------------------
def _pointnet_product(p, x, vx, V, w, cuda):
    m = make_pointnet(p, cuda).train()
    xd = x.to(cuda).requires_grad_(True)
    out = m(xd, vx.to(cuda), n_vox=V)
    (out * w.to(cuda)).sum().backward()
    got = {k: q.grad for k, q in m.named_parameters()}
    got["inp"], got["out"] = xd.grad, out.detach()
    return got


def _pointnet_refs(fn, p, x, vx, V, w, cuda):
    refs = []
    for dt in (torch.float64, torch.float32):
        out, g = ref.pointnet_grads(fn, p, x, vx, V, w, dt, device=cuda)
        g["out"] = out
        refs.append(g)
    return refs


# left_in: the dropped points stay in the arrays with vox = -1, together with a random 20 % of the rows
@pytest.mark.parametrize("n,V,left_in", [(n, V, False) for n, V in ref.SHAPES] + [(257, 9, True), (20000, 5000, True)])
def test_pointnet_train(cuda, n, V, left_in):
    """make_pointnet(...).train() under autograd at the shapes of pointnet_ref.SHAPES: the output and the gradient of
    every parameter and of the input against orc.pointnet2stage in float64 / float32 on the GPU."""
    c = ref.pointnet_case(n, V, 0.2 if left_in else 0.0)
    keep = c["keep"]
    x_ref, v_ref = c["inp"][keep], c["vox"][keep]
    print("(%d, %d): %d of %d points in, %d output entries masked" % (n, V, int(keep.sum()), n, c["masked"]))
    if left_in:
        got = _pointnet_product(c["p"], c["inp"], torch.where(keep, c["vox"], torch.full_like(c["vox"], -1)), V,
                                c["w"], cuda)
        assert not got["inp"][~keep.to(cuda)].any()           # a row left out has no gradient at all
        got["inp"] = got["inp"][keep.to(cuda)]
    else:
        got = _pointnet_product(c["p"], x_ref, v_ref, V, c["w"], cuda)
    r64, r32 = _pointnet_refs(orc.pointnet2stage, c["p"], x_ref, v_ref, V, c["w"], cuda)
    _check_all("pointnet (%d, %d)%s" % (n, V, " left in" if left_in else ""), got, r64, r32)


@functools.lru_cache(maxsize=None)
def _tied_case():
    """About 600 points in 7 voxels, every row of a conditioned set of 200 present two to four times: the copies are
    laid out in rounds (copy r of every row that has one, in row order), so no two copies are adjacent; 15 % of the
    copies are left out (vox = -1), of a row that loses all of them the last one is put back."""
    V = 7
    g = torch.Generator().manual_seed(5)
    p = orc.init_pointnet(7, 1.5)
    base, bv = torch.randn(200, 6, generator=g), torch.randint(0, V, (200,), generator=g)
    w = torch.randn(V, 128, generator=g)
    keep, out_mask, _ = ref.condition_pointnet(f64(p), base, bv, V)
    base, bv = base[keep], bv[keep]
    copies = 2 + torch.arange(base.shape[0]) % 3
    src = torch.cat([torch.nonzero(copies > r)[:, 0] for r in range(4)])
    vox = bv[src].clone()
    vox[torch.rand(src.numel(), generator=g) < 0.15] = -1
    for b in range(base.shape[0]):
        mine = torch.nonzero(src == b)[:, 0]
        if bool((vox[mine] < 0).all()):
            vox[mine[-1]] = bv[b]
    return p, base[src].contiguous(), vox, src, torch.where(out_mask, torch.zeros_like(w), w), V


def test_pointnet_train_exact_ties(cuda):
    """Exactly tied maxima: the whole gradient of a pooled entry goes to the lowest row that holds it
    (torch_scatter's rule; pointnet_ref.pointnet2stage_argrouted), every other copy's input gradient is exactly 0."""
    p, x, vox, src, w, V = _tied_case()
    got = _pointnet_product(p, x, vox, V, w, cuda)
    inside = vox >= 0
    lowest = torch.zeros(x.shape[0], dtype=torch.bool)
    for b in torch.unique(src).tolist():
        lowest[torch.nonzero((src == b) & inside)[0, 0]] = True
    gi = got["inp"].cpu()
    assert gi[lowest].any() and not gi[~lowest].any()
    got["inp"] = got["inp"][inside.to(cuda)]
    r64, r32 = _pointnet_refs(ref.pointnet2stage_argrouted, p, x[inside], vox[inside], V, w, cuda)
    assert not r64["inp"].cpu()[~lowest[inside]].any()
    _check_all("pointnet ties", got, r64, r32)


# ---------------------------------------------------------------------------------------------------------------
# the refine step
# ---------------------------------------------------------------------------------------------------------------
REFINE_KEYS = ("ray_dir", "ray_pix", "ray_bid", "ray_flat", "pred_pos", "max_pair_id", "pair_vox", "voxel_bound",
               "voxel_bid", "rgb_img", "feat_grid", "valid_inp", "valid_vox")


def _upstream(case):
    return torch.randn(case["pred_pos"].shape, generator=torch.Generator().manual_seed(3))


@functools.lru_cache(maxsize=None)
def _refine_refs(forward_times, pos_rel, pnet_pos_rel):
    """Float64 and float32 autograd through the orc.refine_step chain on the CPU (it goes through numpy), once per
    configuration: [(pos, end voxels, gradients)] for float64, float32."""
    case = ref.conditioned_refine_case(pos_rel, pnet_pos_rel)[0]
    return [ref.refine_grads(case, dt, forward_times, _upstream(case), pos_rel=pos_rel, pnet_pos_rel=pnet_pos_rel)
            for dt in (torch.float64, torch.float32)]


def _modules(case, cuda):
    return make_pointnet(case["pnet_p"], cuda), make_module("IEF", case["off_p"], 334, cuda)


@pytest.mark.parametrize("forward_times", [1, 2])
def test_refine_inference(cuda, forward_times):
    """lidf_refine (f32) from the perturbed start: positions against the float64 / float32 chain, equal end voxels."""
    from implicit_depth_amd.query import lidf_refine
    case = ref.conditioned_refine_case()[0]
    (p64, e64, _), (p32, e32, _) = _refine_refs(forward_times, False, True)
    assert torch.equal(e64, e32)
    t = {k: case[k].to(cuda) for k in REFINE_KEYS}
    t["pred_pos"] = (case["pred_pos"] + case["noise"] * case["ray_dir"]).contiguous().to(cuda)
    pnet, dec = _modules(case, cuda)
    with torch.no_grad():
        pos, ev = lidf_refine(*[t[k] for k in REFINE_KEYS], pnet, dec, forward_times=forward_times)
    assert torch.equal(ev.cpu().long(), e64)
    assert_f64_close("refine inference x%d pos" % forward_times, pos, p64, p32)


# forward_times = 1: every embedding argument is an exact input; 2: iteration 1's rounding enters iteration 2's
# 2^7-octave embedding, the float32 oracle itself is 1-2e-5 off float64 and the unit grows with it; grid: the end
# voxels through the cell table (the fused step only); relative positions for the decoder, absolute for the PointNet
@pytest.mark.parametrize("path,forward_times,pos_rel,pnet_pos_rel,use_grid", [
    ("fused", 1, False, True, False), ("composed", 1, False, True, False),
    ("fused", 2, False, True, False), ("composed", 2, False, True, False),
    ("fused", 2, False, True, True),
    ("fused", 2, True, False, False), ("composed", 2, True, False, False)])
def test_refine_train(cuda, path, forward_times, pos_rel, pnet_pos_rel, use_grid):
    """lidf_refine_train / _lidf_refine_train_composed on the conditioned scene (pointnet_ref.refine_case): positions,
    end voxels (equal) and the gradient of every PointNet2Stage and IEF parameter, of the incoming pred_pos and of
    feat_grid against float64 / float32 autograd through orc.refine_step."""
    from implicit_depth_amd.query import _lidf_refine_train_composed, lidf_refine_train
    case, keep_ray, keep_valid, _ = ref.conditioned_refine_case(pos_rel, pnet_pos_rel)
    print("refine scene: %d of %d rays, %d of %d valid points in" % (int(keep_ray.sum()), keep_ray.numel(),
                                                                     int(keep_valid.sum()), keep_valid.numel()))
    (p64, e64, g64), (p32, e32, g32) = _refine_refs(forward_times, pos_rel, pnet_pos_rel)
    assert torch.equal(e64, e32)
    t = {k: case[k].to(cuda) for k in REFINE_KEYS}
    t["pred_pos"].requires_grad_(True)
    t["feat_grid"].requires_grad_(True)
    pnet, dec = _modules(case, cuda)
    pnet.train(), dec.train()
    kw = dict(forward_times=forward_times, pos_rel=pos_rel, pnet_pos_rel=pnet_pos_rel, perturb_noise=case["noise"])
    if use_grid:
        kw["grid"] = dict(case["grid"], voxel_coord=case["grid"]["voxel_coord"].to(cuda))
    fn = lidf_refine_train if path == "fused" else _lidf_refine_train_composed
    pos, ev = fn(*[t[k] for k in REFINE_KEYS], pnet, dec, **kw)
    assert torch.equal(ev.cpu().long(), e64)
    (pos * _upstream(case).to(cuda)).sum().backward()
    got = {"pnet." + k: q.grad for k, q in pnet.named_parameters()}
    got.update({"dec." + k: q.grad for k, q in dec.named_parameters()})
    got.update({"pred_pos": t["pred_pos"].grad, "feat_grid": t["feat_grid"].grad, "pos": pos.detach()})
    tag = "refine %s x%d%s%s" % (path, forward_times, " pos_rel" if pos_rel else "", " grid" if use_grid else "")
    _check_all(tag, got, dict(g64, pos=p64), dict(g32, pos=p32))
