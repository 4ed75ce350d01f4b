"""CPU: the stage-1 training loss. tests/golden/g9_train_step.npz — the reference's own
LIDF.forward(batch, 'train', epoch) — pins the tests' restatement (train_loss_ref.py) and the product's torch-op
composite (losses.lidf_loss_composite) in float32; the fused entry points refuse CPU tensors."""
import pytest
import torch

import train_loss_ref as tl
from util import ROOT  # noqa: F401  (puts the repository on sys.path)

# Both sides evaluate the same float32 formulas; what differs is the association of sums of at most a few hundred
# terms (per-ray softmax sums, means over 42 rays / 38 labels, the 3-term dot products of the normals). Each such
# sum carries a relative error of at most n 2^-24 on its largest partial sum: 2e-5 of the largest magnitude of the
# compared tensor leaves a factor of a few over n = 64 .. 126, and is 10x below the 2e-4 of the training tests.
F32_ROUNDING = 2e-5


def _near(got, ref, what):
    scale = ref.abs().max().item()
    err = (got - ref).abs().max().item()
    assert err <= F32_ROUNDING * max(scale, 1e-30), (what, err, scale)


@pytest.mark.parametrize("name", sorted(tl.G9_CASES))
def test_restatement_reproduces_the_reference(name):
    g, _ = tl.g9_files()
    d, ref = tl.g9_case(g, name)
    epoch, opt = tl.g9_opt(name)
    gt_pos, label, max_id = tl.compute_gt_ref(d["xyz_flat"], d["miss_bid"], d["miss_flat"], d["voxel_bound"],
                                              d["pair_ray"], d["pair_vox"])
    assert torch.equal(gt_pos, d["gt_pos"])
    assert torch.equal(label, d["pcl_label"]) and label.dtype == torch.int64
    if epoch < 6:   # (the label-selected pair; at epoch 6 the reference stores the arg-max of the logits)
        assert torch.equal(max_id, d["max_pair_id"])
    n_lab = torch.bincount(d["pair_ray"], weights=label.double(), minlength=gt_pos.shape[0])
    n_pair = torch.bincount(d["pair_ray"], minlength=gt_pos.shape[0])
    assert int(n_lab.max()) == 2 and bool(((n_pair > 0) & (n_lab == 0)).any()) and bool((n_pair == 0).any())
    loss, gp, gl = tl.loss_and_grads(d, torch.float32, epoch, **opt)
    for i, k in enumerate(tl.LOSS_KEYS):
        print(name, k, float(loss[i]), float(ref["loss"][i]))
        _near(loss[i], ref["loss"][i], (name, k))
    _near(gp, ref["g_pred_pos"], (name, "g_pred_pos"))
    _near(gl, ref["g_pred_prob_end"], (name, "g_pred_prob_end"))


def _composite_dd(d):
    dd = {k: d[k] for k in ("bs", "h", "w", "xyz_flat", "pair_ray", "gt_pos", "pcl_label")}
    dd["miss_bid"], dd["miss_flat_img_id"] = d["miss_bid"], d["miss_flat"]
    dd["pred_pos"] = d["pred_pos"].clone().requires_grad_(True)
    dd["pred_prob_end"] = d["pred_prob_end"].clone().requires_grad_(True)
    return dd


@pytest.mark.parametrize("name", sorted(tl.G9_CASES))
def test_composite_reproduces_the_reference(name):
    from implicit_depth_amd import LidfLossOptions, lidf_loss_composite
    g, _ = tl.g9_files()
    d, ref = tl.g9_case(g, name)
    epoch, opt = tl.g9_opt(name)
    dd = _composite_dd(d)
    out = lidf_loss_composite(dd, LidfLossOptions(**opt), "train", epoch)
    assert tuple(out) == tl.LOSS_KEYS
    out["loss_net"].backward()
    for i, k in enumerate(tl.LOSS_KEYS):
        _near(out[k].detach(), ref["loss"][i], (name, k))
    _near(dd["pred_pos"].grad, ref["g_pred_pos"], (name, "g_pred_pos"))
    _near(dd["pred_prob_end"].grad, ref["g_pred_prob_end"], (name, "g_pred_prob_end"))


def test_composite_in_float64_follows_the_restatement():
    from implicit_depth_amd import LidfLossOptions, lidf_loss_composite
    g, _ = tl.g9_files()
    d, _ = tl.g9_case(g, "e6")
    loss, gp, gl = tl.loss_and_grads(d, torch.float64, 6, smooth_w=0.3)
    dd = _composite_dd(d)
    dd["pred_pos"] = d["pred_pos"].double().requires_grad_(True)
    dd["pred_prob_end"] = d["pred_prob_end"].double().requires_grad_(True)
    out = lidf_loss_composite(dd, LidfLossOptions(smooth_w=0.3), "train", 6)
    out["loss_net"].backward()
    assert out["loss_net"].dtype == torch.float64
    got = torch.stack([out[k].detach() for k in tl.LOSS_KEYS])
    assert (got - loss).abs().max().item() <= 1e-12 * loss.abs().max().item()
    assert (dd["pred_pos"].grad - gp).abs().max().item() <= 1e-12 * gp.abs().max().item()
    assert (dd["pred_prob_end"].grad - gl).abs().max().item() <= 1e-12 * max(gl.abs().max().item(), 1.0)


def test_no_labelled_pair_gives_nan_prob_loss_in_the_definitions():
    """torch.mean of an empty tensor (models/pipeline.py:486): NaN prob_loss and loss_net, finite other terms, and
    gradients that the empty mean does not reach."""
    from implicit_depth_amd import lidf_loss_composite
    g, _ = tl.g9_files()
    d, _ = tl.g9_case(g, "e0")
    d["pcl_label"] = torch.zeros_like(d["pcl_label"])
    loss, gp, gl = tl.loss_and_grads(d, torch.float32, 0)
    out = lidf_loss_composite(_composite_dd(d), None, "train", 0)
    for v in (dict(zip(tl.LOSS_KEYS, loss)), out):
        assert torch.isnan(v["prob_loss"]) and torch.isnan(v["loss_net"])
        assert all(torch.isfinite(v[k]) for k in ("pos_loss", "surf_norm_loss", "smooth_loss", "err", "angle_err"))
    assert torch.isfinite(gp).all() and bool((gl == 0).all())


def test_fused_entry_points_refuse_cpu_tensors():
    from implicit_depth_amd import IEF, IMNet, PointNet2Stage, lidf_forward_train, lidf_loss
    from implicit_depth_amd.losses import compute_gt
    g, _ = tl.g9_files()
    batch, feat = tl.g9_batch(g)
    with pytest.raises(RuntimeError, match="CUDA"):
        lidf_forward_train(batch, feat, PointNet2Stage(6, 128, 32), IMNet(385, 1), IEF("cpu", 385, 1, n_iter=2))
    d, _ = tl.g9_case(g, "e0")
    dd = _composite_dd(d)
    with pytest.raises(RuntimeError, match="CUDA"):
        lidf_loss(dd)
    dd.update({"ray_bid": d["miss_bid"].int(), "ray_flat": d["miss_flat"].int(),
               "pair_off": torch.zeros(d["miss_bid"].shape[0] + 1, dtype=torch.int32),
               "pair_vox": d["pair_vox"].int(), "voxel_bound": d["voxel_bound"]})
    with pytest.raises(RuntimeError, match="CUDA"):
        compute_gt(dd)
    with pytest.raises(NotImplementedError):
        lidf_loss(dd, exp_type="test")


def test_loss_abi_argument_errors_without_gpu():
    """Status codes of the new entry points for malformed calls (checked before any HIP call)."""
    import ctypes as C
    from implicit_depth_amd import _lib
    L = _lib.lib()
    a = _lib.LidfLossArgs()
    assert L.lidf_stage1_loss_f32(None, None) == -1 and L.lidf_stage1_loss_backward_f32(None, None) == -1
    assert L.lidf_stage1_loss_f32(C.byref(a), None) == 0          # no ray: nothing to do
    a.n_rays = 5
    assert L.lidf_stage1_loss_f32(C.byref(a), None) == -1         # NULL inputs
    a.n_rays = -1
    assert L.lidf_stage1_loss_backward_f32(C.byref(a), None) == -1
    assert L.lidf_stage1_loss_workspace_bytes(0) == 0
    assert L.lidf_stage1_loss_workspace_bytes(20000) >= (20000 // 256) * 9 * 8
    null = C.c_void_p(None)
    assert L.lidf_pair_labels_f32(null, 1, 4, 4, null, null, 3, null, null, 0, null, 0, null, null, null, null, null,
                                  null, null) == -1               # no n_label
