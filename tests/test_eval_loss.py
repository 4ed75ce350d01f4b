"""CPU: the evaluation flavour ('valid' / 'test') of the two losses. tests/golden/g12_valid_loss.npz — the reference's
own LIDF.forward / RefineNet.forward — pins the tests' restatement (eval_loss_ref.py) and the product's torch-op
composites in float32; the composites follow the restatement in float64; their training flavour is unchanged; the
C-ABI argument errors of the two new entry points (checked before any HIP call)."""
import ctypes as C

import pytest
import torch

import eval_loss_ref as el
import train_loss_ref as tl
from util import ROOT  # noqa: F401  (puts the repository on sys.path)

# as tests/test_train_loss.py: the same float32 formulas, sums of a few hundred terms associated differently
F32_ROUNDING = 2e-5


def _near(got, ref, what):
    got, ref = got.double(), ref.double()
    if torch.isnan(ref).any():
        assert torch.equal(torch.isnan(got), torch.isnan(ref)), what
        return
    err = (got - ref).abs().max().item()
    assert err <= F32_ROUNDING * max(ref.abs().max().item(), 1e-30), (what, err, got, ref)


def _opt(g, name):
    pos_w, prob_w, surf_w, smooth_w, _ = (float(v) for v in g[name + "_loss_opt"])
    return dict(pos_w=pos_w, prob_w=prob_w, surf_norm_w=surf_w, smooth_w=smooth_w, **el.G12_CASES[name][1])


def _composite_dd(d, dt):
    dd = {k: d[k] for k in ("bs", "h", "w", "pair_ray", "pcl_label", "corrupt_mask")}
    for k in ("xyz_flat", "xyz_corrupt_flat", "gt_pos", "pred_pos", "pred_prob_end", "pred_pos_refine"):
        dd[k] = d[k].to(dt)
    dd["miss_bid"], dd["miss_flat_img_id"] = d["miss_bid"], d["miss_flat"]
    return dd


@pytest.mark.parametrize("stage", (1, 2))
@pytest.mark.parametrize("name", sorted(el.G12_CASES))
def test_restatement_and_composite_reproduce_the_reference(name, stage):
    from implicit_depth_amd import LidfLossOptions, lidf_loss_composite, refine_loss_composite
    g = el.g12_file()
    d, ref = el.g12_case(g, name)
    exp_type, opt = el.G12_CASES[name][0], _opt(g, name)
    want = ref["loss"] if stage == 1 else ref["loss_refine"]
    keys = el.EVAL_LOSS_KEYS if stage == 1 else el.REFINE_EVAL_LOSS_KEYS
    assert want.shape[0] == len(keys) == (17 if stage == 1 else 15)
    out = el.eval_loss_ref(d, torch.float32, stage, 0, **opt)
    assert int(out["count"]) == int(g[name + "_n_stat"]) > 0
    n = float(out["count"])
    comp = (lidf_loss_composite if stage == 1 else refine_loss_composite)(
        _composite_dd(d, torch.float32), LidfLossOptions(**opt), exp_type, 0)
    assert tuple(comp) == keys and not any(v.requires_grad for v in comp.values())
    for i, k in enumerate(keys):
        print(name, stage, k, float(out[k]), float(comp[k]), float(want[i]))
        if k in ("a1", "a2", "a3"):   # counts: exact (the generator keeps every threshold away from the limits)
            assert round(float(out[k]) * n) == round(float(want[i]) * n) == round(float(comp[k]) * n), (name, k)
        else:
            _near(out[k], want[i], (name, stage, k))
            _near(comp[k], want[i], (name, stage, k, "composite"))
    # the composite in float64 follows the restatement in float64
    out64 = el.eval_loss_ref(d, torch.float64, stage, 0, **opt)
    comp64 = (lidf_loss_composite if stage == 1 else refine_loss_composite)(
        _composite_dd(d, torch.float64), LidfLossOptions(**opt), exp_type, 0)
    for k in keys:
        assert comp64[k].dtype == torch.float64
        assert abs(float(comp64[k]) - float(out64[k])) <= 1e-11 * max(abs(float(out64[k])), 1e-3), (name, stage, k)


def test_the_base_cloud_matters_in_the_fixture():
    """Case b has queried pixels beside non-queried ones at which xyz_corrupt != xyz: the training flavour's base
    cloud gives other surface-normal and smoothness terms."""
    g = el.g12_file()
    d, ref = el.g12_case(g, "b")
    wrong = el.eval_loss_ref(dict(d, xyz_corrupt_flat=d["xyz_flat"]), torch.float32, 1, 0, **_opt(g, "b"))
    for k, i in (("surf_norm_loss", 2), ("smooth_loss", 3)):
        assert abs(float(wrong[k]) - float(ref["loss"][i])) > 1e-3 * abs(float(ref["loss"][i])), k


def test_training_flavour_of_the_composites_is_unchanged():
    from implicit_depth_amd import LidfLossOptions, lidf_loss_composite
    g, _ = tl.g9_files()
    for name in sorted(tl.G9_CASES):
        d, ref = tl.g9_case(g, name)
        epoch, opt = tl.g9_opt(name)
        dd = {k: d[k] for k in ("bs", "h", "w", "xyz_flat", "pair_ray", "gt_pos", "pcl_label", "pred_pos",
                                "pred_prob_end")}
        dd["miss_bid"], dd["miss_flat_img_id"] = d["miss_bid"], d["miss_flat"]
        # xyz_corrupt_flat present and different: the training flavour must not read it
        dd["xyz_corrupt_flat"] = torch.zeros_like(d["xyz_flat"])
        out = lidf_loss_composite(dd, LidfLossOptions(**opt), "train", epoch)
        assert tuple(out) == tl.LOSS_KEYS
        want = tl.loss_ref(d, epoch, **opt)
        for k in tl.LOSS_KEYS:
            _near(out[k].detach(), want[k].detach(), (name, k))


def test_eval_flavour_needs_its_base_cloud_and_a_known_exp_type():
    from implicit_depth_amd import lidf_loss, lidf_loss_composite, refine_loss, refine_loss_composite
    g = el.g12_file()
    d, _ = el.g12_case(g, "b")
    dd = _composite_dd(d, torch.float32)
    for fn in (lidf_loss, refine_loss):   # (with the base cloud present the fused calls get as far as the device check)
        with pytest.raises(RuntimeError, match="CUDA"):
            fn(dd, None, "valid")
    del dd["xyz_corrupt_flat"]
    for fn in (lidf_loss, refine_loss, lidf_loss_composite, refine_loss_composite):
        with pytest.raises(NotImplementedError, match="xyz_corrupt_flat"):
            fn(dd, None, "valid")
        with pytest.raises(ValueError, match="exp_type"):
            fn(dd, None, "eval")


def test_eval_abi_argument_errors_without_gpu():
    """Status codes of the new entry points for malformed calls (checked before any HIP call)."""
    from implicit_depth_amd import _lib
    L = _lib.lib()
    A = _lib.LidfEvalLossArgs
    for fn in (L.lidf_stage1_eval_loss_f32, L.lidf_refine_eval_loss_f32):
        assert fn.argtypes == [C.POINTER(A), C.c_void_p] and fn.restype == C.c_int
        assert fn(None, None) == -1
        a = A()
        assert fn(C.byref(a), None) == 0             # no ray: nothing to do
        a.n_rays = 5
        assert fn(C.byref(a), None) == -1            # NULL inputs
        a.n_rays = -1
        assert fn(C.byref(a), None) == -1
        a.n_rays, a.batch, a.height, a.width = 1, 1 << 16, 1 << 16, 1 << 16
        assert fn(C.byref(a), None) == -2            # more pixels than an int32 index reaches
    # complete pointers (never dereferenced on the host), then one defect at a time
    buf = (C.c_char * 64)()
    p = C.addressof(buf)

    def args():
        a = A()
        a.n_rays, a.n_pairs, a.batch, a.height, a.width = 3, 0, 2, 4, 4
        for k in ("xyz_base", "ray_bid", "ray_flat", "pair_off", "pix2ray", "gt_pos", "gt_max_pair_id", "n_label",
                  "pred_pos", "loss", "workspace"):
            setattr(a, k, p)
        a.workspace_bytes = 1 << 20
        return a
    a = args()
    a.loss = None
    assert L.lidf_stage1_eval_loss_f32(C.byref(a), None) == -1
    a = args()
    a.workspace_bytes = 8
    assert L.lidf_stage1_eval_loss_f32(C.byref(a), None) == -3 and L.lidf_refine_eval_loss_f32(C.byref(a), None) == -3
    a = args()
    a.workspace = p + 4                               # misaligned
    assert L.lidf_refine_eval_loss_f32(C.byref(a), None) == -1
    a = args()
    a.surf_norm_dist = p                              # the three per-ray vectors of the normals: all or none
    assert L.lidf_refine_eval_loss_f32(C.byref(a), None) == -1
    a = args()
    a.resize_metrics = 1                              # the resized-frame statistics are the bs == 1 branch
    assert L.lidf_stage1_eval_loss_f32(C.byref(a), None) == -1
    a.batch = 1                                       # ... and read xyz_gt
    assert L.lidf_stage1_eval_loss_f32(C.byref(a), None) == -1
    a.xyz_gt, a.seg_dtype = p, 7
    assert L.lidf_stage1_eval_loss_f32(C.byref(a), None) == -1
    a = args()
    a.n_pairs = 4                                     # pairs without labels / logits (stage 2 reads neither)
    assert L.lidf_stage1_eval_loss_f32(C.byref(a), None) == -1
    # hard-negative mining after the forward: the unreduced vectors must exist
    a = args()
    for fn in (L.lidf_stage1_eval_hard_neg_f32, L.lidf_refine_eval_hard_neg_f32):
        assert fn(None, 0.1, None, 0, None) == -1
        assert fn(C.byref(a), 0.1, p, 1 << 20, None) == -1
    # sizes: 18 double partial sums per block of 256 rays; the bs == 1 branch adds the statistics' workspace, its
    # outputs and two depth images
    for fn in (L.lidf_stage1_eval_loss_workspace_bytes, L.lidf_refine_eval_loss_workspace_bytes):
        assert fn(0, 0) == 0 and fn(600, 0) == 3 * 18 * 8
        assert fn(600, 384) == 3 * 18 * 8 + L.lidf_depth_metrics_workspace_bytes() + 64 + 2 * 384 * 4
