"""Tests only: the exp_type != 'train' flavour of LIDF.compute_loss and RefineNet.compute_loss
(models/pipeline.py:468-650, 760-919) restated in torch ops on image-sized tensors, in the dtype of the inputs
(float32 or float64). The fixture tests/golden/g12_valid_loss.npz (the reference's own LIDF.forward / RefineNet.forward
for 'valid' and 'test') pins this restatement in float32; its float64 evaluation is then the yardstick of the HIP loss
at other shapes (util.assert_f64_close).

It is train_loss_ref.loss_ref / refine_loss_ref.refine_loss_ref with xyz_corrupt_flat as the frame the queried pixels
are replaced in (:497, :779) — the ground truth still comes from gt_pos —, followed by the nine statistics of :571-618.
"""
import os

import numpy as np
import torch

from refine_loss_ref import REFINE_LOSS_KEYS, refine_loss_ref
from train_loss_ref import LOSS_KEYS, loss_ref
from util import orc

METRIC_KEYS = ("a1", "a2", "a3", "rmse", "rmse_log", "log10", "abs_rel", "mae", "sq_rel")
EVAL_LOSS_KEYS = LOSS_KEYS + METRIC_KEYS
REFINE_EVAL_LOSS_KEYS = REFINE_LOSS_KEYS + METRIC_KEYS
EVAL_SIZE = (144, 256)   # cv2.resize(..., (256, 144)), :582


def selection(d, pred_pos):
    """(gt, pred, mask) of the statistics in the dtype of pred_pos: the rays' depths and their nonzero-ground-truth
    mask (bs != 1), or the resized depth images and gt > 0 & corrupt_mask (bs == 1)."""
    dt = pred_pos.dtype
    bs, h, w = d["bs"], d["h"], d["w"]
    gt_pos = d["gt_pos"].to(dt)
    if bs != 1:
        return gt_pos[:, 2], pred_pos[:, 2], gt_pos.abs().sum(-1) != 0
    sy = torch.tensor(orc.resize_nearest_index(h, EVAL_SIZE[0]))
    sx = torch.tensor(orc.resize_nearest_index(w, EVAL_SIZE[1]))
    gt = d["xyz_flat"].to(dt).reshape(bs, h, w, 3)[0, :, :, 2][sy][:, sx].clone()
    gt[torch.isnan(gt)] = 0
    gt[torch.isinf(gt)] = 0
    seg = d["corrupt_mask"].reshape(bs, h, w)[0].to(torch.uint8)[sy][:, sx]
    frame = d["xyz_corrupt_flat"].to(dt).clone()
    frame[d["miss_bid"], d["miss_flat"]] = pred_pos
    pred = frame.reshape(bs, h, w, 3)[0, :, :, 2][sy][:, sx]
    return gt, pred, (gt > 0) & (seg != 0)


def statistics(gt, pred):
    """The nine statistics of the selected elements (:605-618), in their dtype; safe_log10 is the natural logarithm
    there (:607)."""
    dt = gt.dtype
    safe_log = lambda v: torch.log(torch.clamp(v, 1e-6, 1e6))  # noqa: E731
    thresh = torch.max(gt / pred, pred / gt)
    return {"a1": (thresh < 1.05).to(dt).mean(), "a2": (thresh < 1.10).to(dt).mean(),
            "a3": (thresh < 1.25).to(dt).mean(), "rmse": ((gt - pred) ** 2).mean().sqrt(),
            "rmse_log": ((safe_log(gt) - safe_log(pred)) ** 2).mean().sqrt(),
            "log10": (safe_log(gt) - safe_log(pred)).abs().mean(), "abs_rel": ((gt - pred).abs() / gt).mean(),
            "mae": (gt - pred).abs().mean(), "sq_rel": ((gt - pred) ** 2 / gt).mean()}


def _to(d, dt):
    c = dict(d)
    for k in ("xyz_flat", "xyz_corrupt_flat", "gt_pos", "pred_pos", "pred_prob_end", "pred_pos_refine"):
        if k in c:
            c[k] = c[k].detach().to(dt)
    return c


def eval_loss_ref(d, dt, stage=1, epoch=0, **opt):
    """The 17 (stage 2: 15) entries of loss_dict at dtype dt as a dict of 0-dim tensors, plus "count": the number of
    elements the statistics are taken over. d: train_loss_ref.loss_ref's dict (stage 2: pred_pos_refine) plus
    xyz_corrupt_flat [bs,h*w,3] and, for bs == 1, corrupt_mask."""
    c = _to(d, dt)
    base = dict(c, xyz_flat=c["xyz_corrupt_flat"])
    with torch.no_grad():
        out = loss_ref(base, epoch, **opt) if stage == 1 else refine_loss_ref(base, epoch, **opt)
        pred = c["pred_pos"] if stage == 1 else c["pred_pos_refine"]
        gt, p, mask = selection(c, pred)
        out.update(statistics(gt[mask], p[mask]))
        out["count"] = mask.sum()
    return out


def vector(out, stage=1):
    return torch.stack([out[k].reshape(()) for k in (EVAL_LOSS_KEYS if stage == 1 else REFINE_EVAL_LOSS_KEYS)])


# ----------------------------------------------------------------------------------------------
# Random cases (stage 2's inputs plus, for stage 1, a pair list): the shapes of the GPU tests
# ----------------------------------------------------------------------------------------------
def random_case(bs, h, w, hole=0.6, seed=0, pairs=True, zero_gt=False):
    """A frame batch with a hole fraction of about `hole`: the queried pixels are the holes (in torch.nonzero's
    order, as get_miss_ray gives them); xyz_corrupt is xyz with the holes zeroed and a small offset elsewhere, so
    that a build reading xyz_flat as the base cloud fails; about one ground-truth point in eight is the zero point;
    every ray has 0-3 pairs with random logits and labels."""
    gen = torch.Generator().manual_seed(seed)
    ys, xs = torch.meshgrid(torch.arange(h).float(), torch.arange(w).float(), indexing="ij")
    z = 1.0 + 0.01 * xs + 0.02 * ys
    xyz = torch.stack(((xs - w / 2) * z / 20.0, (ys - h / 2) * z / 20.0, z), -1).reshape(1, h * w, 3).repeat(bs, 1, 1)
    xyz = (xyz + 0.003 * torch.randn(xyz.shape, generator=gen)).contiguous()
    mask = torch.rand((bs, h * w), generator=gen) < hole
    mask[0, h * w - 1] = True
    mask[0, h * w - 2] = False
    dead = (torch.rand((bs, h * w), generator=gen) < 0.125) & mask
    if zero_gt:
        dead = mask.clone()
    xyz[dead] = 0.0
    nz = mask.nonzero()
    bid, flat = nz[:, 0].contiguous(), nz[:, 1].contiguous()
    R = bid.shape[0]
    corrupt = (xyz + 0.004).clone()
    corrupt[mask] = 0.0
    gt = xyz[bid, flat].clone()
    pred = (xyz[bid, flat] + 0.02 * torch.randn((R, 3), generator=gen)).contiguous()
    pred[gt.abs().sum(-1) == 0] += 1.0
    d = {"bs": bs, "h": h, "w": w, "xyz_flat": xyz, "xyz_corrupt_flat": corrupt.contiguous(),
         "corrupt_mask": mask.reshape(bs, h, w).float(), "miss_bid": bid, "miss_flat": flat, "gt_pos": gt,
         "pred_pos": pred, "pred_pos_refine": (pred + 0.005 * torch.randn((R, 3), generator=gen)).contiguous()}
    if pairs:
        n = torch.randint(0, 4, (R,), generator=gen)
        n[0] = 0
        ray = torch.repeat_interleave(torch.arange(R), n)
        P = ray.shape[0]
        d["pair_ray"] = ray
        d["pair_off"] = torch.cat((torch.zeros(1, dtype=torch.long), n.cumsum(0))).to(torch.int32)
        d["pred_prob_end"] = torch.randn((P, 1), generator=gen)
        d["pcl_label"] = (torch.rand((P,), generator=gen) < 0.4).long()
    return d


# ----------------------------------------------------------------------------------------------
# tests/golden/g12_valid_loss.npz (tests/golden/make_golden_valid.py)
# ----------------------------------------------------------------------------------------------
G12_CASES = {"a": ("valid", {}), "b": ("valid", {}), "c": ("valid", dict(hard_neg=True, hard_neg_ratio=0.1)),
             "d": ("test", {})}


def g12_file():
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    return np.load(os.path.join(here, "g12_valid_loss.npz"))


def g12_case(g, name):
    """One case as eval_loss_ref's input dict (pairs in the reference's voxel-major order) and the reference's two
    loss_dicts as vectors."""
    t = lambda k: torch.from_numpy(g["%s_%s" % (name, k)])  # noqa: E731
    xyz, corrupt = t("xyz"), t("xyz_corrupt")
    bs, _, h, w = xyz.shape
    flat = lambda v: v.permute(0, 2, 3, 1).reshape(bs, h * w, 3).contiguous()  # noqa: E731
    d = {"bs": bs, "h": h, "w": w, "xyz_flat": flat(xyz), "xyz_corrupt_flat": flat(corrupt),
         "corrupt_mask": t("corrupt_mask").reshape(bs, h, w), "miss_bid": t("miss_bid"),
         "miss_flat": t("miss_flat_img_id"), "pair_ray": t("miss_ray_intersect_idx"),
         "pair_vox": t("occ_vox_intersect_idx"), "voxel_bound": t("voxel_bound"), "gt_pos": t("gt_pos"),
         "pcl_label": t("pcl_label"), "pred_pos": t("pred_pos"), "pred_prob_end": t("pred_prob_end"),
         "pred_pos_refine": t("pred_pos_refine")}
    return d, {"loss": t("loss"), "loss_refine": t("loss_refine")}
