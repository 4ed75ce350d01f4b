"""Tests only: the training part of RefineNet.compute_loss (models/pipeline.py:760-840) restated in torch ops on
image-sized tensors, in the dtype of the inputs (float32 or float64). The fixture tests/golden/g10_refine_train.npz
(the reference's own stage-2 iteration) pins this restatement in float32; its float64 evaluation is then the yardstick
of the HIP loss at other shapes (util.assert_f64_close)."""
import math
import os

import torch
import torch.nn.functional as F

from train_loss_ref import image_normals

REFINE_LOSS_KEYS = ("pos_loss", "surf_norm_loss", "smooth_loss", "loss_net", "err", "angle_err")
LOSS_DEFAULTS = dict(hard_neg=False, hard_neg_ratio=None, pos_w=100.0, surf_norm_w=10.0, surf_norm_epo=0, smooth_w=0,
                     smooth_epo=0)


def refine_loss_ref(d, epoch=0, **opt):
    """d: bs, h, w, xyz_flat [bs,h*w,3], miss_bid, miss_flat [R], gt_pos [R,3], pred_pos_refine [R,3] (may require
    grad). Returns loss_dict_refine (0-dim tensors with their graphs)."""
    o = dict(LOSS_DEFAULTS, **opt)
    bs, h, w = d["bs"], d["h"], d["w"]
    pred = d["pred_pos_refine"]
    dt = pred.dtype
    gt_pos = d["gt_pos"].to(dt)
    bid, flat = d["miss_bid"], d["miss_flat"]

    def reduce(v):
        if not o["hard_neg"]:
            return torch.mean(v)
        return torch.mean(torch.topk(v, int(v.shape[0] * o["hard_neg_ratio"]))[0])
    pos_loss = torch.mean((pred - gt_pos).abs()) if not o["hard_neg"] else reduce(torch.mean((pred - gt_pos).abs(), -1))

    def frame_with(pos):   # the train flavour (:775-777): the ground-truth frame with the sampled pixels replaced
        img = d["xyz_flat"].to(dt).clone()
        img[bid, flat] = pos
        return img.reshape(bs, h, w, 3).permute(0, 3, 1, 2)

    def at_rays(img):   # [b,c,h,w] -> [R,c]
        return img.permute(0, 2, 3, 1).reshape(bs, h * w, -1)[bid, flat]
    n_gt, _, _ = image_normals(frame_with(gt_pos))
    n_pred, dx, dy = image_normals(frame_with(pred))
    cos = F.cosine_similarity(at_rays(n_pred), at_rays(n_gt), dim=-1)
    surf = reduce((1 - cos) / 2.0)
    angle_err = torch.mean(torch.acos(torch.clamp(cos, min=-1, max=1))) / math.pi * 180.0
    smooth = reduce(at_rays((dx * dx).sum(1, keepdim=True))[:, 0]) + reduce(at_rays((dy * dy).sum(1, keepdim=True))[:, 0])
    net = o["pos_w"] * pos_loss
    if o["surf_norm_w"] > 0 and epoch >= o["surf_norm_epo"]:
        net = net + o["surf_norm_w"] * surf
    if o["smooth_w"] > 0 and epoch >= o["smooth_epo"]:
        net = net + o["smooth_w"] * smooth
    with torch.no_grad():
        keep = (gt_pos.abs().sum(-1) != 0).to(dt)
        l2 = ((pred - gt_pos) ** 2).sum(-1).sqrt()
        err = (l2 * keep).sum() / keep.sum() if keep.sum() > 0 else torch.zeros((), dtype=dt)
    return {"pos_loss": pos_loss, "surf_norm_loss": surf, "smooth_loss": smooth, "loss_net": net, "err": err,
            "angle_err": angle_err}


def loss_and_grad(d, dt, epoch=0, upstream=1.0, **opt):
    """refine_loss_ref at dtype dt on a fresh leaf of pred_pos_refine: ([6] losses, g_pred_pos_refine) for the
    upstream gradient `upstream` of loss_net."""
    c = dict(d)
    c["xyz_flat"], c["gt_pos"] = d["xyz_flat"].to(dt), d["gt_pos"].to(dt)
    c["pred_pos_refine"] = d["pred_pos_refine"].detach().to(dt, copy=True).requires_grad_(True)
    out = refine_loss_ref(c, epoch, **opt)
    (out["loss_net"] * upstream).backward()
    vec = torch.stack([out[k].detach().reshape(()) for k in REFINE_LOSS_KEYS])
    g = c["pred_pos_refine"].grad
    return vec, g if g is not None else torch.zeros_like(c["pred_pos_refine"])


# ----------------------------------------------------------------------------------------------
# Random cases
# ----------------------------------------------------------------------------------------------
def random_case(R, bs=2, h=12, w=20, seed=0, full_frame=False, zero_gt=False):
    """A restatement dict on bs frames of h x w: a smooth surface plus noise, R sampled pixels that always include the
    last pixel of frame 0 and the first pixel of frame 1 (R >= 2), in an order in which a ray's left or upper
    neighbour lies far away in the ray list (a random permutation); full_frame: every pixel of frame 0."""
    gen = torch.Generator().manual_seed(seed)
    ys, xs = torch.meshgrid(torch.arange(h).float(), torch.arange(w).float(), indexing="ij")
    z = 1.0 + 0.01 * xs + 0.02 * ys
    xyz = torch.stack(((xs - w / 2) * z / 20.0, (ys - h / 2) * z / 20.0, z), -1).reshape(1, h * w, 3).repeat(bs, 1, 1)
    xyz = (xyz + 0.003 * torch.randn(xyz.shape, generator=gen)).contiguous()
    n_pix = bs * h * w
    if full_frame:
        lin = torch.arange(h * w)
    elif R == 1:
        lin = torch.tensor([h * w - 1])
    else:
        rest = torch.randperm(n_pix, generator=gen)
        rest = rest[(rest != h * w - 1) & (rest != h * w)][:R - 2]
        lin = torch.cat((torch.tensor([h * w - 1, h * w]), rest))
    lin = lin[torch.randperm(lin.shape[0], generator=gen)]
    R = lin.shape[0]
    bid, flat = lin // (h * w), lin % (h * w)
    gt = torch.zeros(R, 3) if zero_gt else xyz[bid, flat].clone()
    if zero_gt:
        xyz[bid, flat] = 0.0
    pred = xyz[bid, flat] + 0.02 * torch.randn(R, 3, generator=gen) + (0.05 if zero_gt else 0.0)
    return {"bs": bs, "h": h, "w": w, "xyz_flat": xyz, "miss_bid": bid, "miss_flat": flat, "gt_pos": gt,
            "pred_pos_refine": pred}


# (name, R, case options, epoch, loss options, upstream gradient): the smallest shapes at which the kernels can go
# wrong — one lane, a partial block, two blocks, three partial sums; every pixel of a frame; all gt_pos zero; the four
# on / off combinations of the two epoch gates; an upstream gradient other than 1
RANDOM_CASES = [
    ("one_ray", 1, {}, 0, dict(smooth_w=0.5), 1.0),
    ("partial_block", 255, {}, 0, dict(smooth_w=0.5), 1.0),
    ("two_blocks", 257, {}, 0, dict(smooth_w=0.5), 1.0),
    # (600 rays need more than the 480 pixels of two 12 x 20 frames: this case has three)
    ("three_partials_upstream", 600, dict(bs=3), 0, dict(smooth_w=0.5), 0.37),
    ("full_frame", 240, dict(full_frame=True), 0, dict(smooth_w=0.5), 1.0),
    ("zero_gt", 257, dict(zero_gt=True), 0, dict(smooth_w=0.5), 1.0),
    ("gates_off_off", 257, {}, 1, dict(surf_norm_epo=2, smooth_w=0.5, smooth_epo=2), 1.0),
    ("gates_on_off", 257, {}, 1, dict(surf_norm_epo=1, smooth_w=0.5, smooth_epo=2), 1.0),
    ("gates_off_on", 257, {}, 1, dict(surf_norm_epo=2, smooth_w=0.5, smooth_epo=1), 1.0),
    ("gates_on_on", 257, {}, 1, dict(surf_norm_epo=1, smooth_w=0.5, smooth_epo=1), 1.0),
]


# ----------------------------------------------------------------------------------------------
# tests/golden/g10_refine_train.npz (tests/golden/make_golden_refine_train.py)
# ----------------------------------------------------------------------------------------------
G10_CASES = {"plain": {}, "hn": dict(hard_neg=True, hard_neg_ratio=0.1, pos_w=20.0, surf_norm_w=2.0),
             "smooth": dict(smooth_w=1.0), "noperturb": {}}
G10_MODULES = ("pnet_model", "offset_dec")


def g10_files():
    import numpy as np
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    return (np.load(os.path.join(here, "g10_refine_train.npz")),
            np.load(os.path.join(here, "g10_refine_train_params.npz")))


def g10_batch(g):
    """The reference's dataset-item keys of the fixture's batch, and full_rgb_feat."""
    batch = {k: torch.from_numpy(g["batch_" + k]) for k in ("rgb", "xyz", "xyz_corrupt", "depth_corrupt",
                                                             "corrupt_mask", "valid_mask")}
    intr = torch.from_numpy(g["intr"])
    batch.update({"fx": intr[:, 0].clone(), "fy": intr[:, 1].clone(), "cx": intr[:, 2].clone(),
                  "cy": intr[:, 3].clone(), "item_path": ["a", "b"]})
    return batch, torch.from_numpy(g["full_rgb_feat"])


def g10_case(g, name):
    """One case as refine_loss_ref's input dict (plus stage 1's outputs, pairs in the reference's voxel-major
    order), and the stored results."""
    t = lambda k: torch.from_numpy(g["%s_%s" % (name, k)])  # noqa: E731
    bs, _, h, w = g["batch_xyz"].shape
    d = {"bs": bs, "h": h, "w": w,
         "xyz_flat": torch.from_numpy(g["batch_xyz"]).permute(0, 2, 3, 1).reshape(bs, h * w, 3).contiguous(),
         "miss_bid": t("miss_bid"), "miss_flat": t("miss_flat_img_id"), "pair_ray": t("miss_ray_intersect_idx"),
         "pair_vox": t("occ_vox_intersect_idx"), "voxel_bound": t("voxel_bound"), "gt_pos": t("gt_pos"),
         "max_pair_id": t("max_pair_id"), "pred_pos": t("pred_pos"), "pred_pos_refine": t("pred_pos_refine")}
    noise = float(g[name + "_noise"])
    ref = {"loss": t("loss"), "loss_stage1": t("loss_stage1"), "g_pred_pos_refine": t("g_pred_pos_refine"),
           "end_voxel_id": t("end_voxel_id"), "noise": None if math.isnan(noise) else noise,
           "np_seed": int(g[name + "_np_seed"])}
    return d, ref
