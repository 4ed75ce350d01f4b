"""losses.py — ground-truth labels and the losses of stage 1 and stage 2, training and evaluation flavour.

Reference counterparts (paths relative to /root/reference/src):
  compute_gt           <- LIDF.compute_gt                       models/pipeline.py:298-336
  lidf_loss            <- LIDF.compute_loss                     models/pipeline.py:468-650: exp_type 'train' (:468-566,
                       differentiable) and 'valid' / 'test' (the evaluation flavour: xyz_corrupt_flat as the base
                       cloud of the normals, the nine ClearGrasp statistics, no backward)
  lidf_loss_composite  the same loss in plain torch ops (any dtype, any device): the A/B partner of
                       lidf_loss and the route for CPU callers
  refine_loss          <- RefineNet.compute_loss                models/pipeline.py:760-919, the same three flavours
  refine_loss_composite  the same in plain torch ops
  LidfLossOptions      <- the loss.* keys of experiments/implicit_depth/default_config.yaml:97-107
  per_frame=True       of the four losses: every frame of a batch gets the loss_dict test() reports at bs == 1
                       (lidf_stage1_eval_loss_frames_f32 / lidf_refine_eval_loss_frames_f32), as [bs] tensors
  frame_slice          the bs == 1 data_dict of one frame of a batch: what a per-frame row means

compute_gt and lidf_loss run in liblidf_hip.so (csrc/lidf_loss.hip): one launch for the labels, two for the
loss, one for its backward; no ray x voxel mask and no image-sized normal map is built, and nothing here
reads a size or a value back to the host (hard-negative mining by torch.topk, the default route, reads the label
count: its k depends on it; LidfLossOptions.hard_neg_select = "device" takes the top-k means in csrc/lidf_select.hip
and reads nothing). topk_mean is that select for a caller's own loss term.
Pairs are RAY-MAJOR as everywhere in this package: pcl_label / gt_max_pair_id index that list
(query.to_reference_order gives the reference's voxel-major order).
"""
import ctypes as C

import torch
import torch.nn.functional as F

from . import _lib
from .query import _as_i32, _f32, _i32

LOSS_KEYS = ("pos_loss", "prob_loss", "surf_norm_loss", "smooth_loss", "loss_net", "acc", "err", "angle_err")
REFINE_LOSS_KEYS = ("pos_loss", "surf_norm_loss", "smooth_loss", "loss_net", "err", "angle_err")
# what exp_type 'valid' / 'test' appends (models/pipeline.py:639-649, 906-917)
EVAL_METRIC_KEYS = ("a1", "a2", "a3", "rmse", "rmse_log", "log10", "abs_rel", "mae", "sq_rel")
EVAL_LOSS_KEYS = LOSS_KEYS + EVAL_METRIC_KEYS
REFINE_EVAL_LOSS_KEYS = REFINE_LOSS_KEYS + EVAL_METRIC_KEYS
EXP_TYPES = ("train", "valid", "test")


class LidfLossOptions:
    """loss.* of default_config.yaml:97-107 (train_refine_hardneg.yaml: hard_neg True, hard_neg_ratio 0.1).
    The defaults are stage 1's (train_lidf.yaml). Stage 2 reads the same keys (prob_w and prob_loss_type are not
    used there) and ships other values: train_refine.yaml pos_w 100 / surf_norm_w 10, train_refine_hardneg.yaml
    pos_w 20 / surf_norm_w 2 with hard_neg True and hard_neg_ratio 0.1.
    hard_neg_select (no reference counterpart) is the route of hard-negative mining in lidf_loss / refine_loss:
    "torch" (the default) is torch.topk per term, "device" is the radix select of csrc/lidf_select.hip — one launch
    sequence for every term, no label count read back, and ties at the k-th value go to the lowest indices where
    torch.topk leaves the choice open. The composites ignore it."""

    def __init__(self, **kw):
        self.hard_neg = False
        self.hard_neg_ratio = None
        self.hard_neg_select = "torch"
        self.pos_loss_type = "single"
        self.pos_w = 100.0
        self.prob_loss_type = "ray"
        self.prob_w = 0.5
        self.surf_norm_w = 10.0
        self.surf_norm_epo = 0
        self.smooth_w = 0
        self.smooth_epo = 0
        for k, v in kw.items():
            if not hasattr(self, k):
                raise TypeError("unknown option %s" % k)
            setattr(self, k, v)


def _check_types(opt, prob=True):
    if opt.pos_loss_type != "single":
        raise NotImplementedError("pos_loss_type %s" % opt.pos_loss_type)
    if prob and opt.prob_loss_type != "ray":
        raise NotImplementedError("prob_loss_type %s" % opt.prob_loss_type)
    if opt.hard_neg and opt.hard_neg_ratio is None:
        raise ValueError("hard_neg needs hard_neg_ratio")
    if opt.hard_neg_select not in ("torch", "device"):
        raise ValueError("hard_neg_select must be 'torch' or 'device', not %r" % (opt.hard_neg_select,))


def _terms_on(opt, epoch):
    """Whether the surface-normal / smoothness terms enter loss_net (models/pipeline.py:543-546)."""
    return (opt.surf_norm_w > 0 and epoch >= opt.surf_norm_epo, opt.smooth_w > 0 and epoch >= opt.smooth_epo)


def _ray_index(dd):
    """(ray_bid, ray_flat) int32 of the sampled rays, from the int32 forms or the reference's int64 keys."""
    bid = dd["ray_bid"] if "ray_bid" in dd else dd["miss_bid"]
    flat = dd["ray_flat"] if "ray_flat" in dd else dd["miss_flat_img_id"]
    return _as_i32(bid, "ray_bid").contiguous(), _as_i32(flat, "ray_flat").contiguous()


def compute_gt(dd):
    """LIDF.compute_gt (models/pipeline.py:298-336) on lidf_forward_train's data_dict (xyz_flat, the sampled rays,
    the ray-major pair list, voxel_bound). Adds gt_pos [R,3], pcl_label [P] int64 (the reference's dtype),
    pcl_label_float [P], gt_max_pair_id [R] int64 — the label-selected pair of every ray, scatter_max's choice of
    :445: what lidf_query_train takes as max_pair_id while epoch < maxpool_label_epo — and n_label, the number of
    labelled pairs as a 0-dim device tensor; pix2ray [bs*h*w] int32 (the ray of a sampled pixel, -1 elsewhere) is
    kept for lidf_loss. valid_*_in_intersect (:312-335) are read nowhere in the reference and are not built."""
    xyz = dd["xyz_flat"]
    ray_bid, ray_flat = _ray_index(dd)
    pair_off, pair_vox, vb = dd["pair_off"], dd["pair_vox"], dd["voxel_bound"]
    _lib.require_cuda(xyz, ray_bid, ray_flat, pair_off, pair_vox, vb,
                      names=["xyz_flat", "ray_bid", "ray_flat", "pair_off", "pair_vox", "voxel_bound"])
    _f32(xyz, "xyz_flat"), _f32(vb, "voxel_bound"), _i32(pair_off, "pair_off"), _i32(pair_vox, "pair_vox")
    bs, h, w = dd["bs"], dd["h"], dd["w"]
    R, P, V = ray_bid.shape[0], pair_vox.shape[0], vb.shape[0]
    if tuple(xyz.shape) != (bs, h * w, 3) or pair_off.shape[0] != R + 1 or tuple(vb.shape) != (V, 6):
        raise RuntimeError("xyz_flat / pair_off / voxel_bound must be [bs,h*w,3] / [R+1] / [V,6]")
    dev = xyz.device
    f32 = dict(dtype=torch.float32, device=dev)
    i64 = dict(dtype=torch.int64, device=dev)
    out = {
        "gt_pos": torch.empty((R, 3), **f32), "pcl_label": torch.empty((P,), **i64),
        "pcl_label_float": torch.empty((P,), **f32), "gt_max_pair_id": torch.empty((R,), **i64),
        "pix2ray": torch.empty((bs * h * w,), dtype=torch.int32, device=dev),
    }
    n_label = torch.empty((1,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().lidf_pair_labels_f32(
            _lib.ptr(xyz), bs, h, w, _lib.ptr(ray_bid), _lib.ptr(ray_flat), R, _lib.ptr(pair_off),
            _lib.ptr(pair_vox), P, _lib.ptr(vb), V, _lib.ptr(out["gt_pos"]), _lib.ptr(out["pcl_label"]),
            _lib.ptr(out["pcl_label_float"]), _lib.ptr(out["gt_max_pair_id"]), _lib.ptr(n_label),
            _lib.ptr(out["pix2ray"]), _lib.current_stream(dev)))
    out["n_label"] = n_label[0]
    dd.update(out)
    return dd


def _loss_args(t, cfg):
    """LidfLossArgs over the tensors `t` (a dict; absent / None entries stay NULL)."""
    a = _lib.LidfLossArgs()
    a.n_rays, a.n_pairs = t["gt_pos"].shape[0], t["pcl_label"].shape[0]
    a.batch, a.height, a.width = cfg["bs"], cfg["h"], cfg["w"]
    a.pos_w, a.prob_w = float(cfg["pos_w"]), float(cfg["prob_w"])
    a.surf_norm_w, a.smooth_w = float(cfg["surf_norm_w"]), float(cfg["smooth_w"])
    a.surf_norm_on, a.smooth_on = int(cfg["surf_on"]), int(cfg["smooth_on"])
    for k, v in t.items():
        if v is not None:
            setattr(a, k, v.data_ptr())
    return a


def _topk_weights(v, k):
    """(mean of the k largest entries of v, weights 1/k at them and 0 elsewhere): torch.topk as in
    models/pipeline.py:475-490, 514-539."""
    top, idx = torch.topk(v, k)
    w = torch.zeros_like(v)
    if k > 0:
        w[idx] = 1.0 / k
    return torch.mean(top), w


def _stage1_topk(fwd, loss, n_label, R, cfg):
    """Hard-negative mining of stage 1 by torch.topk (models/pipeline.py:475-490, 514-539): the means over the top-k
    elements of the unreduced terms. Returns (loss with its first five entries replaced, the five weight vectors a
    backward takes)."""
    ratio = cfg["hard_neg_ratio"]
    kr = int(R * ratio)
    kl = int(int(n_label.item()) * ratio)   # (the one size read: k of the labelled pairs)
    pos, w_pos = _topk_weights(fwd["pos_unreduced"], kr)
    prob, w_prob = _topk_weights(fwd["prob_unreduced"], kl)
    surf, w_surf = _topk_weights(fwd["surf_norm_dist"], kr)
    sdx, w_dx = _topk_weights(fwd["dx_dist"], kr)
    sdy, w_dy = _topk_weights(fwd["dy_dist"], kr)
    smooth = sdx + sdy
    net = cfg["pos_w"] * pos + cfg["prob_w"] * prob
    if cfg["surf_on"]:
        net = net + cfg["surf_norm_w"] * surf
    if cfg["smooth_on"]:
        net = net + cfg["smooth_w"] * smooth
    return torch.cat((torch.stack((pos, prob, surf, smooth, net)), loss[5:])), (w_pos, w_prob, w_surf, w_dx, w_dy)


def _refine_topk(fwd, loss, R, cfg):
    """Hard-negative mining of stage 2 by torch.topk (models/pipeline.py:767-770, 799-801, 818-821): k = int(R *
    ratio) is known on the host, so nothing is read back. Returns (loss with its first four entries replaced, the
    four weight vectors)."""
    k = int(R * cfg["hard_neg_ratio"])
    pos, w_pos = _topk_weights(fwd["pos_unreduced"], k)
    surf, w_surf = _topk_weights(fwd["surf_norm_dist"], k)
    sdx, w_dx = _topk_weights(fwd["dx_dist"], k)
    sdy, w_dy = _topk_weights(fwd["dy_dist"], k)
    smooth = sdx + sdy
    net = cfg["pos_w"] * pos
    if cfg["surf_on"]:
        net = net + cfg["surf_norm_w"] * surf
    if cfg["smooth_on"]:
        net = net + cfg["smooth_w"] * smooth
    return torch.cat((torch.stack((pos, surf, smooth, net)), loss[4:])), (w_pos, w_surf, w_dx, w_dy)


def _ratio(ratio):
    ratio = float(ratio)
    if not 0.0 <= ratio <= 1.0:
        raise ValueError("ratio must lie in [0, 1], not %r" % ratio)
    return ratio


def topk_mean(values, ratio, count=None):
    """(mean of the k largest entries of `values`, weights [n]: float32(1 / k) at them and 0 elsewhere) by the radix
    select of csrc/lidf_select.hip (lidf_topk_mean_f32). values: a float32 CUDA tensor, read flattened; k =
    int(count * ratio) with count = n, or a 0-dim / [1] int32 device tensor that stays on the device (nothing is read
    back; the call can be captured in a graph). torch.topk's order (NaN greatest, -0.0 == +0.0); ties at the k-th
    value go to the lowest indices; k == 0 gives a NaN mean and zero weights. Not differentiable: the weights are
    what a backward multiplies with."""
    ratio = _ratio(ratio)
    _lib.require_cuda(values, count, names=["values", "count"])
    _f32(values, "values")
    v = values.detach().reshape(-1)
    if count is not None:
        if count.dtype != torch.int32 or count.numel() != 1 or count.device != v.device:
            raise RuntimeError("count must be one int32 on the device of values")
        count = count.reshape(1)
    dev, n = v.device, v.shape[0]
    mean = torch.empty((), dtype=torch.float32, device=dev)
    w = torch.empty((n,), dtype=torch.float32, device=dev)
    L = _lib.lib()
    wsb = L.lidf_topk_mean_workspace_bytes(1, n)
    ws = _lib.workspace(wsb, dev)
    job = _lib.LidfTopkJob(v.data_ptr() if n else None, n, None if count is None else count.data_ptr(),
                           mean.data_ptr(), w.data_ptr() if n else None)
    with torch.cuda.device(dev):
        _lib.check(L.lidf_topk_mean_f32(C.byref(job), 1, ratio, _lib.ptr(ws), wsb, _lib.current_stream(dev)))
    return mean, w


class _Stage1LossFn(torch.autograd.Function):
    """compute_loss of the training step as one autograd node over pred_pos and pred_prob_end
    (lidf_stage1_loss_f32 / lidf_stage1_loss_backward_f32). Outputs: loss_net (differentiable) and the [8] vector
    of loss_dict (detached: the other seven entries are metrics)."""

    @staticmethod
    def forward(ctx, pred_pos, pred_prob, cfg, maps, xyz, ray_bid, ray_flat, pair_off, pix2ray, gt_pos, pcl_label,
                gt_max_pair_id, n_label):
        dev = xyz.device
        pp = pred_pos.detach().contiguous()
        lg = pred_prob.detach().reshape(-1).contiguous()
        R, P = gt_pos.shape[0], pcl_label.shape[0]
        f32 = dict(dtype=torch.float32, device=dev)
        L = _lib.lib()
        wsb = L.lidf_stage1_loss_workspace_bytes(R)
        n_label = n_label.reshape(1)
        t = {"xyz": xyz, "ray_bid": ray_bid, "ray_flat": ray_flat, "pair_off": pair_off, "pix2ray": pix2ray,
             "gt_pos": gt_pos, "pcl_label": pcl_label, "gt_max_pair_id": gt_max_pair_id, "n_label": n_label,
             "pred_pos": pp, "pred_prob": lg}
        fwd = {"loss": torch.empty((8,), **f32), "pos_unreduced": torch.empty((R,), **f32),
               "surf_norm_dist": torch.empty((R,), **f32), "dx_dist": torch.empty((R,), **f32),
               "dy_dist": torch.empty((R,), **f32), "prob_unreduced": torch.empty((P,), **f32),
               "ray_lse": torch.empty((R, 2), **f32), "workspace": _lib.workspace(wsb, dev)}
        if maps is not None:
            fwd["gt_surf_norm_img"], fwd["pred_surf_norm_img"] = maps
        a = _loss_args(dict(t, **fwd), cfg)
        a.workspace_bytes = wsb
        with torch.cuda.device(dev):
            _lib.check(L.lidf_stage1_loss_f32(C.byref(a), _lib.current_stream(dev)))
        loss = fwd["loss"]
        weights = (None,) * 5
        if cfg["hard_neg"] and cfg["hard_neg_select"] == "device":
            # the same means by the radix select of lidf_select.hip: one launch sequence for the five terms, k of the
            # labelled pairs taken from n_label on the device, loss[0..4] rewritten in place
            weights = tuple(torch.empty((n,), **f32) for n in (R, P, R, R, R))
            hsb = L.lidf_topk_mean_workspace_bytes(5, max(R, P))
            hws = _lib.workspace(hsb, dev)
            with torch.cuda.device(dev):
                _lib.check(L.lidf_stage1_hard_neg_f32(C.byref(a), _ratio(cfg["hard_neg_ratio"]),
                                                      *(_lib.ptr(w) for w in weights), _lib.ptr(hws), hsb,
                                                      _lib.current_stream(dev)))
        elif cfg["hard_neg"]:
            # the top-k means by torch.topk; the backward takes them as per-element weights
            loss, weights = _stage1_topk(fwd, loss, n_label, R, cfg)
        ctx.cfg = cfg
        ctx.shapes = (tuple(pred_pos.shape), tuple(pred_prob.shape))
        ctx.has_w = cfg["hard_neg"]
        saved = [t[k] for k in ("xyz", "ray_bid", "ray_flat", "pair_off", "pix2ray", "gt_pos", "pcl_label",
                                "gt_max_pair_id", "n_label", "pred_pos", "pred_prob")] + [fwd["ray_lse"]]
        ctx.save_for_backward(*saved, *(weights if ctx.has_w else ()))
        net = loss[4].clone()
        ctx.mark_non_differentiable(loss)
        return net, loss

    @staticmethod
    def backward(ctx, g_net, _g_loss):
        s = ctx.saved_tensors
        names = ("xyz", "ray_bid", "ray_flat", "pair_off", "pix2ray", "gt_pos", "pcl_label", "gt_max_pair_id",
                 "n_label", "pred_pos", "pred_prob", "ray_lse")
        t = dict(zip(names, s[:12]))
        if ctx.has_w:
            t.update(zip(("w_pos", "w_prob", "w_surf", "w_dx", "w_dy"), s[12:]))
        dev = t["xyz"].device
        R, P = t["gt_pos"].shape[0], t["pcl_label"].shape[0]
        t["g_loss_net"] = g_net.detach().reshape(1).contiguous().float()
        t["g_pred_pos"] = torch.empty((R, 3), dtype=torch.float32, device=dev)
        t["g_logit"] = torch.empty((P,), dtype=torch.float32, device=dev)
        a = _loss_args(t, ctx.cfg)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().lidf_stage1_loss_backward_f32(C.byref(a), _lib.current_stream(dev)))
        return (t["g_pred_pos"].reshape(ctx.shapes[0]), t["g_logit"].reshape(ctx.shapes[1])) + (None,) * 11


def _cfg(dd, opt, epoch):
    surf_on, smooth_on = _terms_on(opt, epoch)
    return {"bs": dd["bs"], "h": dd["h"], "w": dd["w"], "pos_w": float(opt.pos_w), "prob_w": float(opt.prob_w),
            "surf_norm_w": float(opt.surf_norm_w), "smooth_w": float(opt.smooth_w), "surf_on": surf_on,
            "smooth_on": smooth_on, "hard_neg": bool(opt.hard_neg),
            "hard_neg_ratio": opt.hard_neg_ratio, "hard_neg_select": opt.hard_neg_select}


_PER_FRAME_TRAIN = ("%s: per_frame is the evaluation flavour's ('valid' / 'test': the loss_dict the reference's test() "
                    "reports per frame at bs == 1); the training loss is one mean over the batch's rays and carries "
                    "a backward — there is no per-frame training loss")
_PER_FRAME_HARD_NEG = ("%s: per_frame with loss.hard_neg — there is no per-frame hard-negative select (the top-k of "
                       "every term would be taken per frame); evaluate such frames one by one: "
                       "losses.frame_slice(dd, b) and the bs == 1 call")


def _refuse_per_frame(who, opt, exp_type):
    if exp_type == "train":
        raise NotImplementedError(_PER_FRAME_TRAIN % who)
    if opt.hard_neg:
        raise NotImplementedError(_PER_FRAME_HARD_NEG % who)


def _nan_rows(keys, bs, dtype, device):
    """The per-frame dict of a batch without a ray: no frame has a loss_dict (models/pipeline.py:686)."""
    return {k: torch.full((bs,), float("nan"), dtype=dtype, device=device) for k in keys}


def _frame_ends(bid, b):
    """Device tensor [2]: first ray of frame b and of frame b + 1 in the grouped (non-decreasing) ray_bid."""
    return torch.searchsorted(bid.contiguous(), torch.tensor([b, b + 1], dtype=bid.dtype, device=bid.device))


_SLICE_FRAME_KEYS = ("xyz_flat", "xyz_corrupt_flat", "pred_depth", "pred_depth_refine")
_SLICE_RAY_KEYS = ("ray_flat", "miss_flat_img_id", "gt_pos", "pred_pos", "pred_pos_refine")
_SLICE_PAIR_KEYS = ("pcl_label", "pcl_label_float", "pred_prob_end", "pair_vox", "pair_t")


def _n_pairs(dd):
    """P of a data_dict, from any of its [P] lists."""
    for k in ("pcl_label", "pair_vox", "pred_prob_end", "pair_ray"):
        if k in dd:
            return dd[k].shape[0]
    raise KeyError("frame_slice: gt_max_pair_id without a pair list")


def frame_slice(dd, b):
    """The bs == 1 data_dict of frame b of a batch dict (lidf_forward's / FrameRunner.result()'s with the entries
    loss_dict adds, compute_gt's entries where present), on any device: what lidf_loss / refine_loss / the composites /
    pipeline.eval_metrics read, cut to the frame —
      the frame's rows of xyz_flat / xyz_corrupt_flat / corrupt_mask / pred_depth / pred_depth_refine;
      its rays (ray_flat, gt_pos, pred_pos, pred_pos_refine) with ray_bid 0;
      its pairs (pcl_label, pred_prob_end, pair_vox, pair_t; pair_ray in the slice's ray numbers) with pair_off and
      gt_max_pair_id re-based (a ray without pairs gets the slice's own P); voxel_bound stays whole (pair_vox indexes it);
      pix2ray of the frame re-based to the slice's ray numbers; n_label, its own count of labelled pairs.
    The rays must be grouped by frame (ray_bid non-decreasing, as every list of this package is). The two range ends
    (and with pair_off the two pair ends) are read on the host in one copy. Row b of a per_frame=True loss is, bit for
    bit, the bs == 1 loss of this dict; with loss.hard_neg it is the only route to a frame's numbers."""
    bs, h, w = dd["bs"], dd["h"], dd["w"]
    if not 0 <= b < bs:
        raise IndexError("frame_slice: frame %d of a batch of %d" % (b, bs))
    bid_key = "ray_bid" if "ray_bid" in dd else "miss_bid"
    bid = dd[bid_key]
    ends = _frame_ends(bid, b)
    off = dd.get("pair_off")
    if off is not None:
        s, e, p0, p1 = torch.cat((ends.long(), off[ends].long())).tolist()
    else:
        s, e = ends.tolist()
    out = {"bs": 1, "h": h, "w": w}
    for k in _SLICE_FRAME_KEYS:
        if k in dd:
            out[k] = dd[k][b:b + 1]
    if "corrupt_mask" in dd:
        out["corrupt_mask"] = dd["corrupt_mask"].reshape(bs, h, w)[b:b + 1]
    for k in ("ray_bid", "miss_bid"):
        if k in dd:
            out[k] = torch.zeros_like(dd[k][s:e])
    for k in _SLICE_RAY_KEYS:
        if k in dd:
            out[k] = dd[k][s:e]
    P = None
    if off is not None:
        P = p1 - p0
        out["pair_off"] = off[s:e + 1] - p0
        for k in _SLICE_PAIR_KEYS:
            if k in dd:
                out[k] = dd[k][p0:p1]
        if "pair_ray" in dd:
            out["pair_ray"] = dd["pair_ray"][p0:p1] - s
    elif "pair_ray" in dd:   # (pairs in any order, the reference's voxel-major one included: a mask, not a range)
        ray = dd["pair_ray"]
        keep = (ray >= s) & (ray < e)
        out["pair_ray"] = ray[keep] - s
        P = int(out["pair_ray"].shape[0])
        for k in _SLICE_PAIR_KEYS:
            if k in dd:
                out[k] = dd[k][keep]
    if "voxel_bound" in dd:
        out["voxel_bound"] = dd["voxel_bound"]
    if "gt_max_pair_id" in dd and off is not None:
        gm = dd["gt_max_pair_id"][s:e]
        out["gt_max_pair_id"] = torch.where(gm >= _n_pairs(dd), torch.full_like(gm, P), gm - p0)
    if "pcl_label" in out and ("n_label" in dd or "gt_max_pair_id" in out):
        out["n_label"] = (out["pcl_label"] != 0).sum().to(torch.int32)
    if "pix2ray" in dd:
        t = dd["pix2ray"][b * h * w:(b + 1) * h * w]
        out["pix2ray"] = torch.where(t >= 0, t - s, t)
    return out


def _per_frame_composite(fn, keys, who, dd, opt, exp_type, epoch, pred_key):
    """per_frame=True of a composite: fn on frame_slice(dd, b) for every frame, stacked to [bs] tensors in the dtype
    and on the device of dd[pred_key]; a frame without a ray gives NaN entries."""
    _refuse_per_frame(who, opt, exp_type)
    pred = dd[pred_key]
    nan = torch.full((), float("nan"), dtype=pred.dtype, device=pred.device)
    rows = []
    for b in range(dd["bs"]):
        fd = frame_slice(dd, b)
        rows.append(fn(fd, opt, exp_type, epoch) if fd[pred_key].shape[0] else {k: nan for k in keys})
    return {k: torch.stack([r[k].reshape(()) for r in rows]) for k in keys}


def _eval_loss(dd, opt, epoch, pairs, t, per_frame=False):
    """The evaluation flavour (exp_type 'valid' / 'test', models/pipeline.py:468-650, 760-919) of either stage over
    the checked tensors `t` (LidfEvalLossArgs' names): lidf_stage1_eval_loss_f32 / lidf_refine_eval_loss_f32, two
    launches (bs == 1, the resized-frame statistics: a memset and four). Forward only: every entry is detached, no
    autograd node is made, and the unreduced [R] / [P] terms are allocated under hard_neg alone. Nothing is read
    back, except the label count of stage 1 under hard_neg with hard_neg_select "torch".
    per_frame: lidf_stage1_eval_loss_frames_f32 / lidf_refine_eval_loss_frames_f32 — the resized-frame branch for
    every frame of the batch (a memset and four launches), [bs] tensors; at bs == 1 the plain call, reshaped."""
    from .query import _seg_mask_arg
    who = "lidf_loss" if pairs else "refine_loss"
    bs, h, w = dd["bs"], dd["h"], dd["w"]
    if per_frame and bs == 1:
        return {k: v.reshape(1) for k, v in _eval_loss(dd, opt, epoch, pairs, t).items()}
    base, xyz = dd["xyz_corrupt_flat"], dd["xyz_flat"]
    _lib.require_cuda(base, names=["xyz_corrupt_flat"])
    _f32(base, "xyz_corrupt_flat")
    if tuple(base.shape) != (bs, h * w, 3) or base.device != xyz.device:
        raise RuntimeError("%s: xyz_corrupt_flat must be [bs,h*w,3] on the device of xyz_flat" % who)
    dev = xyz.device
    R, P = t["gt_pos"].shape[0], (t["pcl_label"].shape[0] if pairs else 0)
    cfg = _cfg(dd, opt, epoch)
    resize = bs == 1 or per_frame   # (the reference's branch, models/pipeline.py:572, 844)
    t = dict(t, xyz_base=base)
    seg_dtype = 0
    if resize:
        if "corrupt_mask" not in dd:
            raise RuntimeError("%s: at bs == 1 the statistics are masked by dd['corrupt_mask'] "
                               "(models/pipeline.py:587-590), which dd lacks" % who)
        mask = dd["corrupt_mask"]
        if mask.numel() != bs * h * w:
            raise RuntimeError("%s: corrupt_mask must hold bs*h*w elements" % who)
        t["xyz_gt"] = xyz
        t["seg_mask"], seg_dtype = _seg_mask_arg(mask.reshape(bs, h, w))
    f32 = dict(dtype=torch.float32, device=dev)
    keys = EVAL_LOSS_KEYS if pairs else REFINE_EVAL_LOSS_KEYS
    if per_frame:
        L = _lib.lib()
        size_fn, loss_fn = (
            (L.lidf_stage1_eval_loss_frames_workspace_bytes, L.lidf_stage1_eval_loss_frames_f32) if pairs else
            (L.lidf_refine_eval_loss_frames_workspace_bytes, L.lidf_refine_eval_loss_frames_f32))
        loss = torch.empty((bs, len(keys)), **f32)
        wsb = size_fn(bs, h, w)
        ws = _lib.workspace(wsb, dev)
        a = _lib.LidfEvalLossArgs()
        a.n_rays, a.n_pairs = R, P
        a.batch, a.height, a.width, a.resize_metrics, a.seg_dtype = bs, h, w, 1, seg_dtype
        a.pos_w, a.prob_w = cfg["pos_w"], cfg["prob_w"]
        a.surf_norm_w, a.smooth_w = cfg["surf_norm_w"], cfg["smooth_w"]
        a.surf_norm_on, a.smooth_on = int(cfg["surf_on"]), int(cfg["smooth_on"])
        for k, v in t.items():
            if v is not None and k != "n_label":   # (every frame counts its own labelled pairs)
                setattr(a, k, v.data_ptr())
        a.loss, a.workspace, a.workspace_bytes = loss.data_ptr(), ws.data_ptr(), wsb
        with torch.no_grad(), torch.cuda.device(dev):
            _lib.check(loss_fn(C.byref(a), _lib.current_stream(dev)))
        return {k: loss[:, i] for i, k in enumerate(keys)}
    out = {"loss": torch.empty((len(keys),), **f32)}
    if cfg["hard_neg"]:
        out.update({k: torch.empty((R,), **f32) for k in ("pos_unreduced", "surf_norm_dist", "dx_dist", "dy_dist")})
        if pairs:
            out["prob_unreduced"] = torch.empty((P,), **f32)
    L = _lib.lib()
    size_fn, loss_fn, hard_fn = (
        (L.lidf_stage1_eval_loss_workspace_bytes, L.lidf_stage1_eval_loss_f32, L.lidf_stage1_eval_hard_neg_f32)
        if pairs else
        (L.lidf_refine_eval_loss_workspace_bytes, L.lidf_refine_eval_loss_f32, L.lidf_refine_eval_hard_neg_f32))
    wsb = size_fn(R, h * w if resize else 0)
    ws = _lib.workspace(wsb, dev)
    a = _lib.LidfEvalLossArgs()
    a.n_rays, a.n_pairs = R, P
    a.batch, a.height, a.width, a.resize_metrics, a.seg_dtype = bs, h, w, int(resize), seg_dtype
    a.pos_w, a.prob_w = cfg["pos_w"], cfg["prob_w"]
    a.surf_norm_w, a.smooth_w = cfg["surf_norm_w"], cfg["smooth_w"]
    a.surf_norm_on, a.smooth_on = int(cfg["surf_on"]), int(cfg["smooth_on"])
    for k, v in dict(t, **out).items():
        if v is not None:
            setattr(a, k, v.data_ptr())
    a.workspace, a.workspace_bytes = ws.data_ptr(), wsb
    with torch.no_grad(), torch.cuda.device(dev):
        _lib.check(loss_fn(C.byref(a), _lib.current_stream(dev)))
        loss = out["loss"]
        if cfg["hard_neg"] and cfg["hard_neg_select"] == "device":
            hsb = L.lidf_topk_mean_workspace_bytes(5 if pairs else 4, max(R, P))
            hws = _lib.workspace(hsb, dev)
            _lib.check(hard_fn(C.byref(a), _ratio(cfg["hard_neg_ratio"]), _lib.ptr(hws), hsb,
                               _lib.current_stream(dev)))
        elif cfg["hard_neg"]:
            loss = _stage1_topk(out, loss, t["n_label"], R, cfg)[0] if pairs else _refine_topk(out, loss, R, cfg)[0]
    return {k: loss[i] for i, k in enumerate(EVAL_LOSS_KEYS if pairs else REFINE_EVAL_LOSS_KEYS)}


def lidf_loss(dd, loss_opt=None, exp_type="train", epoch=0, normal_maps=False, per_frame=False):
    """LIDF.compute_loss for exp_type == 'train' (models/pipeline.py:468-566) on lidf_forward_train's data_dict
    (compute_gt's entries + pred_pos [R,3] and pred_prob_end [P,1] of lidf_query_train): the reference's loss_dict
    — pos_loss, prob_loss, surf_norm_loss, smooth_loss, loss_net, acc, err, angle_err — as 0-dim device tensors.
    loss_net carries the graph (one autograd node whose inputs are pred_pos and pred_prob_end); the other seven
    are detached. Nothing is read back to the host, except the label count under hard_neg with the default
    hard_neg_select "torch" (torch.topk per term; its k of the labelled pairs is a host number). With "device" the
    five top-k means come from csrc/lidf_select.hip, which reads n_label on the device: nothing is read back.
    normal_maps=True adds gt_surf_norm_img / pred_surf_norm_img [bs,3,h,w] to dd (visualisation only).

    exp_type 'valid' / 'test' (:468-650) is the evaluation flavour, what a trainer's validate() / test() reads: the
    same dict followed by a1, a2, a3, rmse, rmse_log, log10, abs_rel, mae, sq_rel (EVAL_LOSS_KEYS), every entry —
    loss_net included — detached, no autograd node. The surface-normal and smoothness terms are taken on
    dd['xyz_corrupt_flat'] with the queried pixels replaced (:497); the nine statistics over the rays with a nonzero
    gt_pos when dd['bs'] != 1, over the 144 x 256 resize of the frame masked by gt > 0 and dd['corrupt_mask'] when
    dd['bs'] == 1 (bit-equal to pipeline.eval_metrics on the same depth image). A dict without xyz_corrupt_flat (the
    training step's own) has no evaluation flavour: NotImplementedError. hard_neg applies as in training, by
    either hard_neg_select route; without it no [R] / [P] term buffer is allocated.

    per_frame=True ('valid' / 'test' only): the same keys in the same order, each a detached float32 [bs] device
    tensor — entry b is what this call returns for frame b alone at bs == 1 (frame_slice(dd, b)), bit for bit: the
    loss_dict the reference's test() reports per frame, the nine statistics over that frame's 144 x 256 resize. One
    call (lidf_stage1_eval_loss_frames_f32: a memset and four launches), no host read; the rays must be grouped by
    frame. A frame without a ray has no loss_dict in the reference: its entries are NaN (a batch without any ray:
    all NaN, no error). 'train' and loss.hard_neg raise NotImplementedError; bs == 1 is the plain call as [1]."""
    opt = loss_opt or LidfLossOptions()
    _base_cloud(dd, exp_type, "lidf_loss")
    _check_types(opt)
    if per_frame:
        _refuse_per_frame("lidf_loss", opt, exp_type)
    pred_pos, pred_prob = dd["pred_pos"], dd["pred_prob_end"]
    _lib.require_cuda(pred_pos, pred_prob, dd["xyz_flat"], names=["pred_pos", "pred_prob_end", "xyz_flat"])
    _f32(pred_pos, "pred_pos"), _f32(pred_prob, "pred_prob_end")
    if "pix2ray" not in dd or "gt_pos" not in dd:
        compute_gt(dd)
    ray_bid, ray_flat = _ray_index(dd)
    R, P = dd["gt_pos"].shape[0], dd["pcl_label"].shape[0]
    if tuple(pred_pos.shape) != (R, 3) or pred_prob.numel() != P:
        raise RuntimeError("pred_pos / pred_prob_end must be [R,3] / [P,1]")
    # compute_gt's entries may come from an earlier call on a reused dict: the kernels index with them unchecked
    xyz, pair_off, pix2ray = dd["xyz_flat"], dd["pair_off"], dd["pix2ray"]
    gt = [dd[k] for k in ("gt_pos", "pcl_label", "gt_max_pair_id", "n_label")]
    _lib.require_cuda(pair_off, pix2ray, ray_bid, ray_flat, *gt,
                      names=["pair_off", "pix2ray", "ray_bid", "ray_flat", "gt_pos", "pcl_label", "gt_max_pair_id",
                             "n_label"])
    _f32(xyz, "xyz_flat"), _i32(pair_off, "pair_off"), _i32(pix2ray, "pix2ray"), _f32(gt[0], "gt_pos")
    n_pix = dd["bs"] * dd["h"] * dd["w"]
    if (tuple(xyz.shape) != (dd["bs"], dd["h"] * dd["w"], 3) or tuple(pair_off.shape) != (R + 1,)
            or tuple(pix2ray.shape) != (n_pix,) or ray_bid.shape[0] != R or ray_flat.shape[0] != R
            or tuple(gt[0].shape) != (R, 3) or tuple(gt[2].shape) != (R,)
            or gt[1].dtype != torch.int64 or gt[2].dtype != torch.int64 or gt[3].dtype != torch.int32
            or gt[3].numel() != 1):
        raise RuntimeError("lidf_loss: xyz_flat / pair_off / pix2ray / ray index / compute_gt's entries do not "
                           "belong to one frame batch and ray set: [bs,h*w,3] / [R+1] int32 / [bs*h*w] int32 / [R] "
                           "/ gt_pos [R,3], pcl_label [P] and gt_max_pair_id [R] int64, n_label int32 — run "
                           "compute_gt(dd) again")
    if R == 0 and per_frame:
        return _nan_rows(EVAL_LOSS_KEYS, dd["bs"], torch.float32, xyz.device)
    if R == 0:
        raise RuntimeError("lidf_loss: no ray (the reference returns before compute_loss, models/pipeline.py:686)")
    if exp_type != "train":
        if normal_maps:
            raise NotImplementedError("lidf_loss: normal_maps is the training flavour's")
        t = {"ray_bid": ray_bid, "ray_flat": ray_flat, "pair_off": pair_off, "pix2ray": pix2ray, "gt_pos": gt[0],
             "pcl_label": gt[1], "gt_max_pair_id": gt[2], "n_label": gt[3].reshape(1),
             "pred_pos": pred_pos.detach().contiguous(), "pred_prob": pred_prob.detach().reshape(-1).contiguous()}
        return _eval_loss(dd, opt, epoch, True, t, per_frame)
    maps = None
    if normal_maps:
        shape = (dd["bs"], 3, dd["h"], dd["w"])
        maps = tuple(torch.empty(shape, dtype=torch.float32, device=pred_pos.device) for _ in range(2))
        dd["gt_surf_norm_img"], dd["pred_surf_norm_img"] = maps
    net, loss = _Stage1LossFn.apply(
        pred_pos, pred_prob, _cfg(dd, opt, epoch), maps, dd["xyz_flat"].contiguous(), ray_bid, ray_flat,
        dd["pair_off"], dd["pix2ray"], dd["gt_pos"], dd["pcl_label"], dd["gt_max_pair_id"], dd["n_label"])
    out = {k: loss[i] for i, k in enumerate(LOSS_KEYS)}
    out["loss_net"] = net
    return out


# ------------------------------------------------------------------------------------------------
# The same loss in plain torch ops
# ------------------------------------------------------------------------------------------------
def _first_argmax(src, index, n, fill):
    """Per segment the lowest position of the largest value (scatter_max's index); `fill` for an empty segment
    and for a segment in which no value compares equal to the maximum (NaN)."""
    top = torch.full((n,), float("-inf"), dtype=src.dtype, device=src.device)
    top = top.scatter_reduce(0, index, src, reduce="amax", include_self=True)
    at = torch.arange(src.shape[0], device=src.device)
    cand = torch.where((src == top[index]) & (src > float("-inf")), at, torch.full_like(at, fill))
    return torch.full((n,), fill, dtype=torch.long, device=src.device).scatter_reduce(
        0, index, cand, reduce="amin", include_self=True)


def _neighbour_normals(xyz, table, pos, lin, x, y, h, w):
    """Normals of the frame `xyz` [N,3] (sampled pixels replaced by `pos`) at the sampled pixels `lin`:
    (unit normal, dx, dy) with dx = right - self, dy = below - self, constant 0 in the last column / row."""
    n_pix = xyz.shape[0]

    def point(q):
        t = table[q]
        return torch.where((t >= 0).unsqueeze(-1), pos[t.clamp(min=0)], xyz[q])
    zero = torch.zeros((), dtype=pos.dtype, device=pos.device)
    dx = torch.where((x < w - 1).unsqueeze(-1), point((lin + 1).clamp(max=n_pix - 1)) - pos, zero)
    dy = torch.where((y < h - 1).unsqueeze(-1), point((lin + w).clamp(max=n_pix - 1)) - pos, zero)
    n = torch.linalg.cross(dx, dy, dim=-1)
    return n / (torch.linalg.vector_norm(n, dim=-1, keepdim=True) + 1e-8), dx, dy


def _resize_nearest_index(src, dst, device):
    """Source index of every destination index of cv2.resize(..., interpolation=INTER_NEAREST):
    min(floor(index * (1 / (dst / src))), src - 1), the factor in double (lidf_depth_metrics_kernel's rule)."""
    at = torch.arange(dst, dtype=torch.float64, device=device) * (1.0 / (dst / src))
    return torch.floor(at).long().clamp(max=src - 1)


def _composite_statistics(dd, pred_pos, gt_pos, eval_size=(144, 256)):
    """The nine statistics of exp_type 'valid' / 'test' (models/pipeline.py:571-618) in torch ops, in the dtype of
    pred_pos: {a1 .. sq_rel}. The selection is a boolean mask (a size read on a GPU)."""
    dt, dev = pred_pos.dtype, pred_pos.device
    bs, h, w = dd["bs"], dd["h"], dd["w"]
    with torch.no_grad():
        if bs != 1:
            keep = torch.sum(gt_pos.abs(), -1) != 0
            pred, gt = pred_pos[:, 2][keep], gt_pos[:, 2][keep]
        else:
            bid = (dd["ray_bid"] if "ray_bid" in dd else dd["miss_bid"]).long()
            flat = (dd["ray_flat"] if "ray_flat" in dd else dd["miss_flat_img_id"]).long()
            sy, sx = _resize_nearest_index(h, eval_size[0], dev), _resize_nearest_index(w, eval_size[1], dev)
            gt = dd["xyz_flat"].to(dt).reshape(bs, h, w, 3)[0, :, :, 2][sy][:, sx]
            gt = torch.where(torch.isfinite(gt), gt, torch.zeros_like(gt))
            seg = dd["corrupt_mask"].reshape(h, w)
            # (the reference's astype(np.uint8), :588: truncation toward zero, modulo 256)
            seg = (seg.long() & 255) != 0 if seg.is_floating_point() else seg != 0
            mask = (gt > 0) & seg[sy][:, sx]
            frame = dd["xyz_corrupt_flat"].to(dt).clone()
            frame[bid, flat] = pred_pos.detach()
            pred = frame.reshape(bs, h, w, 3)[0, :, :, 2][sy][:, sx]
            gt, pred = gt[mask], pred[mask]
        safe_log = lambda v: torch.log(torch.clamp(v, 1e-6, 1e6))  # noqa: E731  (safe_log10 is this too, :607)
        thresh = torch.max(gt / pred, pred / gt)
        d = gt - pred
        ld = safe_log(gt) - safe_log(pred)
        return {"a1": (thresh < 1.05).to(dt).mean(), "a2": (thresh < 1.10).to(dt).mean(),
                "a3": (thresh < 1.25).to(dt).mean(), "rmse": (d ** 2).mean().sqrt(),
                "rmse_log": (ld ** 2).mean().sqrt(), "log10": ld.abs().mean(), "abs_rel": (d.abs() / gt).mean(),
                "mae": d.abs().mean(), "sq_rel": (d ** 2 / gt).mean()}


def _base_cloud(dd, exp_type, who):
    """The key of the cloud the queried pixels are replaced in for the normals: xyz_flat for 'train',
    xyz_corrupt_flat for 'valid' / 'test' (models/pipeline.py:493-498, 775-780). A dict that holds the training
    step's entries alone has no evaluation flavour: NotImplementedError, before any tensor is looked at."""
    if exp_type not in EXP_TYPES:
        raise ValueError("exp_type must be one of %s, not %r" % (EXP_TYPES, exp_type))
    if exp_type == "train":
        return "xyz_flat"
    if "xyz_corrupt_flat" not in dd:
        raise NotImplementedError(
            "%s: exp_type %r takes its surface normals and smoothness on dd['xyz_corrupt_flat'] "
            "(models/pipeline.py:497, 779), which this dict lacks — with xyz_flat alone only 'train' is defined; "
            "the nine statistics on their own are pipeline.eval_metrics" % (who, exp_type))
    return "xyz_corrupt_flat"


def _composite_terms(dd, pred_pos, gt_pos, opt, base="xyz_flat"):
    """What the two composites share: (reduce, pos_loss, surf_norm_loss, smooth_loss, angle_err, err) of `pred_pos`
    against `gt_pos` at the sampled pixels of dd; dd[base] is the cloud the sampled pixels are replaced in."""
    dt, dev = pred_pos.dtype, pred_pos.device
    bs, h, w = dd["bs"], dd["h"], dd["w"]
    bid = (dd["ray_bid"] if "ray_bid" in dd else dd["miss_bid"]).long()
    flat = (dd["ray_flat"] if "ray_flat" in dd else dd["miss_flat_img_id"]).long()
    R = pred_pos.shape[0]
    topk_mean = lambda v: torch.mean(torch.topk(v, int(v.shape[0] * opt.hard_neg_ratio))[0])  # noqa: E731
    reduce = topk_mean if opt.hard_neg else torch.mean
    pos_loss = reduce(torch.mean((pred_pos - gt_pos).abs(), -1)) if opt.hard_neg else \
        torch.mean((pred_pos - gt_pos).abs())
    # surface normals and smoothness at the sampled pixels
    xyz = dd[base].reshape(-1, 3).to(dt)
    lin = bid * (h * w) + flat
    table = torch.full((bs * h * w,), -1, dtype=torch.long, device=dev)
    table[lin] = torch.arange(R, device=dev)
    x, y = flat % w, flat // w
    n_gt, _, _ = _neighbour_normals(xyz, table, gt_pos, lin, x, y, h, w)
    n_pred, dx, dy = _neighbour_normals(xyz, table, pred_pos, lin, x, y, h, w)
    cos = F.cosine_similarity(n_pred, n_gt, dim=-1)
    surf_norm_loss = reduce((1 - cos) / 2.0)
    angle_err = torch.mean(torch.acos(torch.clamp(cos, min=-1, max=1))) / torch.pi * 180.0
    smooth_loss = reduce(torch.sum(dx * dx, -1)) + reduce(torch.sum(dy * dy, -1))
    with torch.no_grad():
        nonzero = (torch.sum(gt_pos.abs(), -1) != 0).to(dt)
        l2 = torch.sqrt(torch.sum((pred_pos - gt_pos) ** 2, -1))
        n = torch.sum(nonzero)
        err = torch.where(n == 0, torch.zeros_like(n), torch.sum(l2 * nonzero) / n.clamp(min=1))
    return reduce, pos_loss, surf_norm_loss, smooth_loss, angle_err, err


def lidf_loss_composite(dd, loss_opt=None, exp_type="train", epoch=0, per_frame=False):
    """lidf_loss written in differentiable torch ops, in the dtype of pred_pos, on any device: per-ray
    log-softmax by scatter reductions, the normals by gathering each sampled pixel's right and lower neighbour.
    Needs gt_pos and pcl_label in dd (compute_gt's, or a caller's own); every entry of the returned loss_dict
    carries its graph. It takes many small launches where lidf_loss takes three.
    exp_type 'valid' / 'test': the evaluation flavour (dd['xyz_corrupt_flat'] as the base cloud; the nine statistics
    appended, and dd['corrupt_mask'] read, as lidf_loss describes); its entries are detached.
    per_frame=True ('valid' / 'test', no hard_neg): this function on frame_slice(dd, b) for every frame, as [bs]
    tensors; a frame without a ray gives NaN entries."""
    opt = loss_opt or LidfLossOptions()
    base = _base_cloud(dd, exp_type, "lidf_loss_composite")
    _check_types(opt)
    if per_frame:
        return _per_frame_composite(lidf_loss_composite, EVAL_LOSS_KEYS, "lidf_loss_composite", dd, opt, exp_type,
                                    epoch, "pred_pos")
    pred_pos, logit = dd["pred_pos"], dd["pred_prob_end"].reshape(-1)
    dt, dev = pred_pos.dtype, pred_pos.device
    gt_pos, label = dd["gt_pos"].to(dt), dd["pcl_label"].long()
    ray = dd["pair_ray"].long()
    R, P = pred_pos.shape[0], logit.shape[0]
    reduce, pos_loss, surf_norm_loss, smooth_loss, angle_err, err = _composite_terms(dd, pred_pos, gt_pos, opt, base)
    # ray termination: -log_softmax over each ray's pairs at the labelled pairs
    top = torch.full((R,), float("-inf"), dtype=dt, device=dev).scatter_reduce(
        0, ray, logit.detach(), reduce="amax", include_self=True)
    z = logit - top[ray]
    lse = torch.log(torch.zeros((R,), dtype=dt, device=dev).index_add(0, ray, torch.exp(z)))
    log_sm = z - lse[ray]
    prob_loss = reduce(-log_sm[torch.nonzero(label, as_tuple=False).reshape(-1)])
    loss_net = opt.pos_w * pos_loss + opt.prob_w * prob_loss
    surf_on, smooth_on = _terms_on(opt, epoch)
    if surf_on:
        loss_net = loss_net + opt.surf_norm_w * surf_norm_loss
    if smooth_on:
        loss_net = loss_net + opt.smooth_w * smooth_loss
    with torch.no_grad():
        sm = torch.exp(log_sm)
        pred_label = _first_argmax(sm, ray, R, P)
        gt_label = _first_argmax(label.to(dt), ray, R, P)
        acc = torch.sum(torch.eq(pred_label, gt_label).to(dt)) / R
    out = {"pos_loss": pos_loss, "prob_loss": prob_loss, "surf_norm_loss": surf_norm_loss,
           "smooth_loss": smooth_loss, "loss_net": loss_net, "acc": acc, "err": err, "angle_err": angle_err}
    if exp_type != "train":
        out = {k: v.detach() for k, v in out.items()}
        out.update(_composite_statistics(dd, pred_pos.detach(), gt_pos))
    return out


# ------------------------------------------------------------------------------------------------
# Stage 2: the loss of the refinement network
# ------------------------------------------------------------------------------------------------
_REFINE_IN = ("xyz", "ray_bid", "ray_flat", "pix2ray", "gt_pos", "pred_pos_refine")


def _refine_loss_args(t, cfg):
    """LidfRefineLossArgs over the tensors `t` (a dict; absent / None entries stay NULL)."""
    a = _lib.LidfRefineLossArgs()
    a.n_rays = t["gt_pos"].shape[0]
    a.batch, a.height, a.width = cfg["bs"], cfg["h"], cfg["w"]
    a.pos_w, a.surf_norm_w, a.smooth_w = float(cfg["pos_w"]), float(cfg["surf_norm_w"]), float(cfg["smooth_w"])
    a.surf_norm_on, a.smooth_on = int(cfg["surf_on"]), int(cfg["smooth_on"])
    for k, v in t.items():
        if v is not None:
            setattr(a, k, v.data_ptr())
    return a


class _RefineLossFn(torch.autograd.Function):
    """RefineNet.compute_loss of the training step as one autograd node over pred_pos_refine
    (lidf_refine_loss_f32 / lidf_refine_loss_backward_f32). Outputs: loss_net (differentiable) and the [6] vector
    of loss_dict (detached)."""

    @staticmethod
    def forward(ctx, pred_pos, cfg, img, xyz, ray_bid, ray_flat, pix2ray, gt_pos):
        dev = xyz.device
        pp = pred_pos.detach().contiguous()
        R = gt_pos.shape[0]
        f32 = dict(dtype=torch.float32, device=dev)
        L = _lib.lib()
        wsb = L.lidf_refine_loss_workspace_bytes(R)
        t = dict(zip(_REFINE_IN, (xyz, ray_bid, ray_flat, pix2ray, gt_pos, pp)))
        fwd = {"loss": torch.empty((6,), **f32), "pos_unreduced": torch.empty((R,), **f32),
               "surf_norm_dist": torch.empty((R,), **f32), "dx_dist": torch.empty((R,), **f32),
               "dy_dist": torch.empty((R,), **f32), "workspace": _lib.workspace(wsb, dev),
               "pred_surf_norm_img": img}
        a = _refine_loss_args(dict(t, **fwd), cfg)
        a.workspace_bytes = wsb
        with torch.cuda.device(dev):
            _lib.check(L.lidf_refine_loss_f32(C.byref(a), _lib.current_stream(dev)))
        loss = fwd["loss"]
        weights = ()
        if cfg["hard_neg"] and cfg["hard_neg_select"] == "device":
            # the same means by the radix select of lidf_select.hip, loss[0..3] rewritten in place
            weights = tuple(torch.empty((R,), **f32) for _ in range(4))
            hsb = L.lidf_topk_mean_workspace_bytes(4, R)
            hws = _lib.workspace(hsb, dev)
            with torch.cuda.device(dev):
                _lib.check(L.lidf_refine_hard_neg_f32(C.byref(a), _ratio(cfg["hard_neg_ratio"]),
                                                      *(_lib.ptr(w) for w in weights), _lib.ptr(hws), hsb,
                                                      _lib.current_stream(dev)))
        elif cfg["hard_neg"]:
            loss, weights = _refine_topk(fwd, loss, R, cfg)
        ctx.cfg = cfg
        ctx.shape = tuple(pred_pos.shape)
        ctx.save_for_backward(*t.values(), *weights)
        net = loss[3].clone()
        ctx.mark_non_differentiable(loss)
        return net, loss

    @staticmethod
    def backward(ctx, g_net, _g_loss):
        s = ctx.saved_tensors
        t = dict(zip(_REFINE_IN, s[:6]))
        t.update(zip(("w_pos", "w_surf", "w_dx", "w_dy"), s[6:]))
        dev = t["xyz"].device
        t["g_loss_net"] = g_net.detach().reshape(1).contiguous().float()
        t["g_pred_pos"] = torch.empty((t["gt_pos"].shape[0], 3), dtype=torch.float32, device=dev)
        a = _refine_loss_args(t, ctx.cfg)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().lidf_refine_loss_backward_f32(C.byref(a), _lib.current_stream(dev)))
        return (t["g_pred_pos"].reshape(ctx.shape),) + (None,) * 7


def refine_loss(dd, loss_opt=None, exp_type="train", epoch=0, normal_maps=False, per_frame=False):
    """RefineNet.compute_loss for exp_type == 'train' (models/pipeline.py:760-840) on the data_dict of the stage-2
    training step (pred_pos_refine [R,3], xyz_flat, the sampled rays): the reference's loss_dict — pos_loss,
    surf_norm_loss, smooth_loss, loss_net, err, angle_err — as 0-dim device tensors. loss_net carries the graph (one
    autograd node over pred_pos_refine: lidf_refine_loss_f32 and its backward, three launches in all); the other
    five are detached. gt_pos and pix2ray are compute_gt's: it runs here when dd lacks them (it needs the pair list
    then; the loss itself reads none — a ray without pairs is an ordinary ray). Nothing is read back to the host,
    hard_neg included: its k = int(R * hard_neg_ratio) is known there. hard_neg_select "torch" (the default) takes
    the four top-k means by torch.topk, "device" by csrc/lidf_select.hip in one launch sequence (ties at the k-th
    value: the lowest indices).
    loss_opt: LidfLossOptions; its defaults are train_refine.yaml's pos_w 100 / surf_norm_w 10, and
    train_refine_hardneg.yaml is LidfLossOptions(hard_neg=True, hard_neg_ratio=0.1, pos_w=20.0, surf_norm_w=2.0).
    normal_maps=True adds pred_surf_norm_img_refine [bs,3,h,w] to dd (:894, visualisation only).
    exp_type 'valid' / 'test' (:760-919): the evaluation flavour as in lidf_loss — REFINE_EVAL_LOSS_KEYS, detached,
    dd['xyz_corrupt_flat'] as the base cloud, the nine statistics by dd['bs'] == 1 or not.
    per_frame=True: as lidf_loss's — [bs] tensors, entry b the bs == 1 call on frame_slice(dd, b) bit for bit
    (lidf_refine_eval_loss_frames_f32), NaN for a frame without a ray; 'train' and hard_neg are refused."""
    opt = loss_opt or LidfLossOptions()
    _base_cloud(dd, exp_type, "refine_loss")
    _check_types(opt, prob=False)
    if per_frame:
        _refuse_per_frame("refine_loss", opt, exp_type)
    pred = dd["pred_pos_refine"]
    _lib.require_cuda(pred, dd["xyz_flat"], names=["pred_pos_refine", "xyz_flat"])
    _f32(pred, "pred_pos_refine")
    if "pix2ray" not in dd or "gt_pos" not in dd:
        compute_gt(dd)
    ray_bid, ray_flat = _ray_index(dd)
    # compute_gt's entries may come from an earlier call on a reused dict: the kernels index with them unchecked
    xyz, pix2ray, gt_pos = dd["xyz_flat"], dd["pix2ray"], dd["gt_pos"]
    _lib.require_cuda(pix2ray, ray_bid, ray_flat, gt_pos, names=["pix2ray", "ray_bid", "ray_flat", "gt_pos"])
    _f32(xyz, "xyz_flat"), _i32(pix2ray, "pix2ray"), _f32(gt_pos, "gt_pos")
    bs, h, w = dd["bs"], dd["h"], dd["w"]
    R = gt_pos.shape[0]
    if (tuple(pred.shape) != (R, 3) or tuple(gt_pos.shape) != (R, 3) or tuple(xyz.shape) != (bs, h * w, 3)
            or tuple(pix2ray.shape) != (bs * h * w,) or tuple(ray_bid.shape) != (R,)
            or tuple(ray_flat.shape) != (R,)):
        raise RuntimeError("refine_loss: pred_pos_refine / gt_pos / xyz_flat / pix2ray / ray index do not belong to "
                           "one frame batch and ray set: [R,3] / [R,3] / [bs,h*w,3] / [bs*h*w] int32 / [R] — run "
                           "compute_gt(dd) again")
    if R == 0 and per_frame:
        return _nan_rows(REFINE_EVAL_LOSS_KEYS, bs, torch.float32, xyz.device)
    if R == 0:
        raise RuntimeError("refine_loss: no ray (the reference returns before stage 2, models/pipeline.py:686)")
    if exp_type != "train":
        if normal_maps:
            raise NotImplementedError("refine_loss: normal_maps is the training flavour's")
        t = {"ray_bid": ray_bid, "ray_flat": ray_flat, "pix2ray": pix2ray, "gt_pos": gt_pos,
             "pred_pos": pred.detach().contiguous()}
        return _eval_loss(dd, opt, epoch, False, t, per_frame)
    img = None
    if normal_maps:
        img = torch.empty((bs, 3, h, w), dtype=torch.float32, device=pred.device)
        dd["pred_surf_norm_img_refine"] = img
    cfg = _cfg(dd, opt, epoch)
    net, loss = _RefineLossFn.apply(pred, cfg, img, xyz.contiguous(), ray_bid, ray_flat, pix2ray.contiguous(),
                                    gt_pos.contiguous())
    out = {k: loss[i] for i, k in enumerate(REFINE_LOSS_KEYS)}
    out["loss_net"] = net
    return out


def refine_loss_composite(dd, loss_opt=None, exp_type="train", epoch=0, per_frame=False):
    """refine_loss written in differentiable torch ops, in the dtype of pred_pos_refine, on any device (the A/B
    partner of refine_loss and the route for CPU callers). Needs gt_pos in dd; every entry of the returned loss_dict
    carries its graph. exp_type 'valid' / 'test': the evaluation flavour, as lidf_loss_composite's; per_frame=True
    as there."""
    opt = loss_opt or LidfLossOptions()
    base = _base_cloud(dd, exp_type, "refine_loss_composite")
    _check_types(opt, prob=False)
    if per_frame:
        return _per_frame_composite(refine_loss_composite, REFINE_EVAL_LOSS_KEYS, "refine_loss_composite", dd, opt,
                                    exp_type, epoch, "pred_pos_refine")
    pred = dd["pred_pos_refine"]
    gt_pos = dd["gt_pos"].to(pred.dtype)
    _, pos_loss, surf_norm_loss, smooth_loss, angle_err, err = _composite_terms(dd, pred, gt_pos, opt, base)
    loss_net = opt.pos_w * pos_loss
    surf_on, smooth_on = _terms_on(opt, epoch)
    if surf_on:
        loss_net = loss_net + opt.surf_norm_w * surf_norm_loss
    if smooth_on:
        loss_net = loss_net + opt.smooth_w * smooth_loss
    out = {"pos_loss": pos_loss, "surf_norm_loss": surf_norm_loss, "smooth_loss": smooth_loss,
           "loss_net": loss_net, "err": err, "angle_err": angle_err}
    if exp_type != "train":
        out = {k: v.detach() for k, v in out.items()}
        out.update(_composite_statistics(dd, pred.detach(), gt_pos))
    return out
