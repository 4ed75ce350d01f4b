"""Tests only: LIDF.compute_gt and the training part of LIDF.compute_loss (models/pipeline.py:298-336, 468-566)
restated in torch ops on image-sized tensors, in the dtype of the inputs (float32 or float64). The fixture
tests/golden/g9_train_step.npz (the reference's own run) pins this restatement in float32; its float64 evaluation is
then the yardstick of the HIP loss at other shapes (util.assert_f64_close).

Pairs may come in any order (`pair_ray`, `pair_vox` [P]); ties of the per-ray arg-max go to the lowest position in
that order, as torch_scatter's scatter_max."""
import math

import torch
import torch.nn.functional as F

LOSS_KEYS = ("pos_loss", "prob_loss", "surf_norm_loss", "smooth_loss", "loss_net", "acc", "err", "angle_err")
LOSS_DEFAULTS = dict(hard_neg=False, hard_neg_ratio=None, pos_w=100.0, prob_w=0.5, surf_norm_w=10.0, surf_norm_epo=0,
                     smooth_w=0, smooth_epo=0)


def segment_argmax(src, index, n):
    """[n] long: per segment the lowest position of its largest value; src.shape[0] for an empty segment."""
    P = src.shape[0]
    top = torch.full((n,), float("-inf"), dtype=src.dtype).scatter_reduce(0, index, src, reduce="amax")
    at = torch.arange(P)
    cand = torch.where(src == top[index], at, torch.full_like(at, P))
    return torch.full((n,), P, dtype=torch.long).scatter_reduce(0, index, cand, reduce="amin")


def compute_gt_ref(xyz_flat, miss_bid, miss_flat, voxel_bound, pair_ray, pair_vox):
    """gt_pos [R,3], pcl_label [P] int64, max_pair_id [R] int64 (P for a ray without pairs)."""
    gt_pos = xyz_flat[miss_bid, miss_flat]
    g, vb = gt_pos[pair_ray], voxel_bound[pair_vox]
    outside = torch.zeros(pair_ray.shape[0], dtype=torch.bool)
    for k in range(3):   # inclusive bounds; a NaN coordinate fails no comparison
        outside |= (g[:, k] < vb[:, k]) | (g[:, k] > vb[:, 3 + k])
    label = (~outside).long()
    return gt_pos, label, segment_argmax(label.to(xyz_flat.dtype), pair_ray, miss_bid.shape[0])


def image_normals(img):
    """img [b,3,h,w] -> (unit normals, dx, dy): forward differences to the right / downwards, zero in the last
    column / row, cross product, division by (norm + 1e-8)."""
    dx, dy = torch.zeros_like(img), torch.zeros_like(img)
    dx[:, :, :, :-1] = img[:, :, :, 1:] - img[:, :, :, :-1]
    dy[:, :, :-1, :] = img[:, :, 1:, :] - img[:, :, :-1, :]
    n = torch.cross(dx, dy, dim=1)
    return n / (torch.norm(n, dim=1, keepdim=True) + 1e-8), dx, dy


def loss_ref(d, epoch=0, **opt):
    """d: bs, h, w, xyz_flat [bs,h*w,3], miss_bid, miss_flat [R], pair_ray [P], gt_pos [R,3], pcl_label [P],
    pred_pos [R,3], pred_prob_end [P,1] (the last two may require grad). Returns loss_dict (0-dim tensors with
    their graphs)."""
    o = dict(LOSS_DEFAULTS, **opt)
    bs, h, w = d["bs"], d["h"], d["w"]
    pred_pos, logit = d["pred_pos"], d["pred_prob_end"].reshape(-1)
    dt = pred_pos.dtype
    gt_pos, label, ray = d["gt_pos"].to(dt), d["pcl_label"], d["pair_ray"]
    bid, flat = d["miss_bid"], d["miss_flat"]
    R, P = pred_pos.shape[0], logit.shape[0]

    def reduce(v):
        if not o["hard_neg"]:
            return torch.mean(v)
        return torch.mean(torch.topk(v, int(v.shape[0] * o["hard_neg_ratio"]))[0])
    pos_loss = torch.mean((pred_pos - gt_pos).abs()) if not o["hard_neg"] else \
        reduce(torch.mean((pred_pos - gt_pos).abs(), -1))
    top = torch.full((R,), float("-inf"), dtype=dt).scatter_reduce(0, ray, logit.detach(), reduce="amax")
    z = logit - top[ray]
    log_sm = z - torch.log(torch.zeros(R, dtype=dt).index_add(0, ray, z.exp()))[ray]
    prob_loss = reduce(-log_sm[label.nonzero().reshape(-1)])

    def frame_with(pos):
        img = d["xyz_flat"].to(dt).clone()
        img[bid, flat] = pos
        return img.reshape(bs, h, w, 3).permute(0, 3, 1, 2)

    def at_rays(img):   # [b,c,h,w] -> [R,c]
        return img.permute(0, 2, 3, 1).reshape(bs, h * w, -1)[bid, flat]
    n_gt, _, _ = image_normals(frame_with(gt_pos))
    n_pred, dx, dy = image_normals(frame_with(pred_pos))
    cos = F.cosine_similarity(at_rays(n_pred), at_rays(n_gt), dim=-1)
    surf = reduce((1 - cos) / 2.0)
    angle_err = torch.mean(torch.acos(torch.clamp(cos, min=-1, max=1))) / math.pi * 180.0
    smooth = reduce(at_rays((dx * dx).sum(1, keepdim=True))[:, 0]) + reduce(at_rays((dy * dy).sum(1, keepdim=True))[:, 0])
    net = o["pos_w"] * pos_loss + o["prob_w"] * prob_loss
    if o["surf_norm_w"] > 0 and epoch >= o["surf_norm_epo"]:
        net = net + o["surf_norm_w"] * surf
    if o["smooth_w"] > 0 and epoch >= o["smooth_epo"]:
        net = net + o["smooth_w"] * smooth
    with torch.no_grad():
        pred_label = segment_argmax(log_sm.exp(), ray, R)
        gt_label = segment_argmax(label.to(dt), ray, R)
        acc = (pred_label == gt_label).to(dt).sum() / R
        keep = (gt_pos.abs().sum(-1) != 0).to(dt)
        l2 = ((pred_pos - gt_pos) ** 2).sum(-1).sqrt()
        err = (l2 * keep).sum() / keep.sum() if keep.sum() > 0 else torch.zeros((), dtype=dt)
    return {"pos_loss": pos_loss, "prob_loss": prob_loss, "surf_norm_loss": surf, "smooth_loss": smooth,
            "loss_net": net, "acc": acc, "err": err, "angle_err": angle_err}


def loss_and_grads(d, dt, epoch=0, **opt):
    """loss_ref at dtype dt on fresh leaves of pred_pos / pred_prob_end: ([8] losses, g_pred_pos, g_pred_prob_end)."""
    c = dict(d)
    c["xyz_flat"], c["gt_pos"] = d["xyz_flat"].to(dt), d["gt_pos"].to(dt)
    c["pred_pos"] = d["pred_pos"].detach().to(dt, copy=True).requires_grad_(True)
    c["pred_prob_end"] = d["pred_prob_end"].detach().to(dt, copy=True).requires_grad_(True)
    out = loss_ref(c, epoch, **opt)
    out["loss_net"].backward()
    vec = torch.stack([out[k].detach().reshape(()) for k in LOSS_KEYS])
    gp = c["pred_pos"].grad if c["pred_pos"].grad is not None else torch.zeros_like(c["pred_pos"])
    gl = c["pred_prob_end"].grad if c["pred_prob_end"].grad is not None else torch.zeros_like(c["pred_prob_end"])
    return vec, gp, gl


# ----------------------------------------------------------------------------------------------
# tests/golden/g9_train_step.npz (tests/golden/make_golden_train.py)
# ----------------------------------------------------------------------------------------------
G9_CASES = {"e0": (0, False), "e0_hn": (0, True), "e6": (6, False), "e6_hn": (6, True)}
G9_MODULES = ("prob_dec", "offset_dec", "pnet_model")


def g9_files():
    import os
    import numpy as np
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    return np.load(os.path.join(here, "g9_train_step.npz")), np.load(os.path.join(here, "g9_train_step_params.npz"))


def g9_opt(name):
    epoch, hard_neg = G9_CASES[name]
    return epoch, dict(hard_neg=hard_neg, hard_neg_ratio=0.1 if hard_neg else None)


def g9_batch(g):
    """The reference's dataset-item keys of the fixture's batch, and full_rgb_feat."""
    batch = {k: torch.from_numpy(g["batch_" + k]) for k in ("rgb", "xyz", "xyz_corrupt", "depth_corrupt",
                                                             "corrupt_mask", "valid_mask")}
    intr = torch.from_numpy(g["intr"])
    batch.update({"fx": intr[:, 0].clone(), "fy": intr[:, 1].clone(), "cx": intr[:, 2].clone(),
                  "cy": intr[:, 3].clone(), "item_path": ["a", "b"]})
    return batch, torch.from_numpy(g["full_rgb_feat"])


def g9_case(g, name):
    """One case as loss_ref's input dict, pairs in the reference's voxel-major order, plus the stored results."""
    t = lambda k: torch.from_numpy(g["%s_%s" % (name, k)])  # noqa: E731
    bs, _, h, w = g["batch_xyz"].shape
    d = {"bs": bs, "h": h, "w": w,
         "xyz_flat": torch.from_numpy(g["batch_xyz"]).permute(0, 2, 3, 1).reshape(bs, h * w, 3).contiguous(),
         "miss_bid": t("miss_bid"), "miss_flat": t("miss_flat_img_id"), "pair_ray": t("miss_ray_intersect_idx"),
         "pair_vox": t("occ_vox_intersect_idx"), "voxel_bound": t("voxel_bound"), "gt_pos": t("gt_pos"),
         "pcl_label": t("pcl_label"), "max_pair_id": t("max_pair_id"), "pred_pos": t("pred_pos"),
         "pred_prob_end": t("pred_prob_end")}
    ref = {"loss": t("loss"), "g_pred_pos": t("g_pred_pos"), "g_pred_prob_end": t("g_pred_prob_end"),
           "g_full_rgb_feat": t("g_full_rgb_feat")}
    return d, ref
