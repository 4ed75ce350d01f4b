"""train_step_time.py — times of the stage-1 training step's ground truth + loss on one MI355X.

    python scripts/train_step_time.py [--frames 8] [--reps 30] [--out FILE.json]

In one process, on the 8 x 240 x 320 synthetic batch with the shipped window of 20,000 rays per frame:
  fused      losses.compute_gt + losses.lidf_loss, forward and backward (csrc/lidf_loss.hip)
  composite  the route the reference takes, on the same tensors: dense extensions.pcl_aabb.forward mask [V, R],
             gather of the pairs' labels, scatter-max selection, losses.lidf_loss_composite forward and backward
The two variants alternate inside the timed loop (device events around each, after a warm-up of both), so that
clock state and other tenants of the machine hit both alike. Then the whole pipeline.lidf_forward_train step
(forward + backward) is timed the same way. Launch counts come from torch's profiler on one extra step of each
(kernel and memset records), taken after the timed loops. The stage-2 leg ("stage2" in the result) does the same for
losses.refine_loss against losses.refine_loss_composite on the pred_pos_refine of one pipeline.train_refine_step, and
for that whole step (frozen stage 1 + RefineNet forward + backward). Prints one JSON line; --out writes it to a file
too.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--hole-frac", type=float, default=1.9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_step_time.py needs a GPU: a CPU run gives no time")
    from implicit_depth_amd import (LidfLossOptions, LidfOptions, lidf_forward_train, lidf_loss, lidf_loss_composite)
    from implicit_depth_amd.extensions import pcl_aabb
    from implicit_depth_amd.losses import compute_gt
    from implicit_depth_amd.synthetic import init_decoder_params, synthetic_batch
    from util import make_module, make_pointnet, orc
    dev = torch.device("cuda:0")
    B, h, w = args.frames, 240, 320
    batch, feat = synthetic_batch(B, h, w, seed=3, hole_frac=args.hole_frac)
    batch = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in batch.items()}
    feat = feat.to(dev).requires_grad_(True)
    pnet = make_pointnet(orc.init_pointnet(3, 1.5), dev).train()
    prob = make_module("IMNET", init_decoder_params("IMNET", 385, 7, 5.0), 385, dev).train()
    off = make_module("IEF", init_decoder_params("IEF", 385, 8, 5.0), 385, dev).train()
    mods = (pnet, prob, off)
    opt, lopt = LidfOptions(), LidfLossOptions()

    def whole_step():
        for m in mods:
            for p in m.parameters():
                p.grad = None
        feat.grad = None
        np.random.seed(77)
        ok, dd, loss = lidf_forward_train(batch, feat, *mods, opt=opt, loss_opt=lopt, epoch=0)
        assert ok
        loss["loss_net"].backward()
        return dd, loss

    dd, loss = whole_step()
    R, P, V = dd["total_miss_sample_num"], dd["pair_ray"].shape[0], dd["voxel_bound"].shape[0]
    base = {k: dd[k] for k in ("bs", "h", "w", "xyz_flat", "ray_bid", "ray_flat", "miss_bid", "miss_flat_img_id",
                               "pair_off", "pair_ray", "pair_vox", "voxel_bound", "voxel_bid")}
    pred_pos, logit = dd["pred_pos"].detach().clone(), dd["pred_prob_end"].detach().clone()

    def fused():
        d = dict(base)
        d["pred_pos"], d["pred_prob_end"] = pred_pos.requires_grad_(True), logit.requires_grad_(True)
        pred_pos.grad = logit.grad = None
        compute_gt(d)
        out = lidf_loss(d, lopt, "train", 0)
        out["loss_net"].backward()
        return out, pred_pos.grad, logit.grad

    def composite():
        d = dict(base)
        d["pred_pos"], d["pred_prob_end"] = pred_pos.requires_grad_(True), logit.requires_grad_(True)
        pred_pos.grad = logit.grad = None
        # LIDF.compute_gt as the reference runs it: the dense [V, R] mask, then the pairs' entries
        gt_pos = d["xyz_flat"][d["miss_bid"], d["miss_flat_img_id"]]
        mask = pcl_aabb.forward(gt_pos.contiguous(), d["voxel_bound"], d["ray_bid"], d["voxel_bid"]).long()
        label = mask[d["pair_vox"].long(), d["pair_ray"].long()]
        d["gt_pos"], d["pcl_label"] = gt_pos, label
        from implicit_depth_amd.losses import _first_argmax
        d["gt_max_pair_id"] = _first_argmax(label.float(), d["pair_ray"].long(), R, P)
        out = lidf_loss_composite(d, lopt, "train", 0)
        out["loss_net"].backward()
        return out, pred_pos.grad, logit.grad

    # same results first (faster and different is not faster)
    of, gpf, glf = fused()
    gpf, glf = gpf.clone(), glf.clone()
    oc, gpc, glc = composite()
    same = {k: [float(of[k]), float(oc[k])] for k in of}
    grad_diff = [float((gpf - gpc).abs().max() / gpc.abs().max()), float((glf - glc).abs().max() / glc.abs().max())]

    def timed(fns, reps):
        for fn in fns:
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ms = [[] for _ in fns]
        for _ in range(reps):
            for i, fn in enumerate(fns):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                ms[i].append(a.elapsed_time(b))
        return [{"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "p90_ms": float(np.percentile(v, 90)),
                 "reps": reps} for v in ms]

    t_fused, t_comp = timed((fused, composite), args.reps)
    (t_step,) = timed((whole_step,), max(args.reps // 3, 5))

    def launches(fn):
        try:
            from torch.profiler import ProfilerActivity, profile
            fn()
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                fn()
                torch.cuda.synchronize()
            ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
            return len(ev)
        except Exception as e:   # the count is a by-product: a profiler problem must not lose the times
            return "not measured (%s)" % type(e).__name__

    # ---- stage 2: RefineNet's loss fused against the composite, and the whole stage-2 step
    from implicit_depth_amd import refine_loss, refine_loss_composite, train_refine_step
    pnet_r = make_pointnet(orc.init_pointnet(4, 1.5), dev).train()
    off_r = make_module("IEF", init_decoder_params("IEF", 334, 9, 5.0), 334, dev).train()
    ropt, rlopt = LidfOptions(maxpool_label_epo=0), LidfLossOptions(prob_w=0.0)   # train_refine.yaml

    def refine_step():
        for m in (pnet_r, off_r):
            for p in m.parameters():
                p.grad = None
        np.random.seed(77)
        ok, d2, _, l2 = train_refine_step(batch, feat, *mods, pnet_r, off_r, opt=ropt, loss_opt=rlopt, epoch=0)
        assert ok
        l2["loss_net"].backward()
        return d2, l2

    dd2, _ = refine_step()
    base2 = {k: dd2[k] for k in ("bs", "h", "w", "xyz_flat", "ray_bid", "ray_flat", "miss_bid", "miss_flat_img_id",
                                 "gt_pos", "pix2ray")}
    pos_r = dd2["pred_pos_refine"].detach().clone()

    def stage2(fn):
        def run():
            d = dict(base2)
            d["pred_pos_refine"] = pos_r.requires_grad_(True)
            pos_r.grad = None
            out = fn(d, rlopt, "train", 0)
            out["loss_net"].backward()
            return out, pos_r.grad
        return run
    fused2, composite2 = stage2(refine_loss), stage2(refine_loss_composite)
    of2, g2f = fused2()
    g2f = g2f.clone()
    oc2, g2c = composite2()
    same2 = {k: [float(of2[k]), float(oc2[k])] for k in of2}
    t_fused2, t_comp2 = timed((fused2, composite2), args.reps)
    (t_step2,) = timed((refine_step,), max(args.reps // 3, 5))
    res2 = {
        "what": "stage-2 training step: RefineNet's loss, fused (lidf_loss.hip) vs composite (torch ops)",
        "rays": dd2["total_miss_sample_num"], "fused_loss_fwd_bwd": t_fused2, "composite_loss_fwd_bwd": t_comp2,
        "whole_step_fwd_bwd": t_step2, "speedup_median": t_comp2["median_ms"] / t_fused2["median_ms"],
        "launches": {"fused": launches(fused2), "composite": launches(composite2), "whole_step": launches(refine_step)},
        "loss_dict_fused_vs_composite": same2,
        "grad_rel_diff_pred_pos_refine": float((g2f - g2c).abs().max() / g2c.abs().max()),
    }

    res = {
        "what": "stage-1 training step: ground truth + loss, fused (lidf_loss.hip) vs composite (dense pcl_aabb + torch ops)",
        "device": torch.cuda.get_device_name(0), "clock": "device events around each call, variants alternating",
        "frames": B, "h": h, "w": w, "rays": R, "pairs": P, "voxels": V, "labels": int(dd["n_label"]),
        "fused_gt_loss_fwd_bwd": t_fused, "composite_gt_loss_fwd_bwd": t_comp, "whole_step_fwd_bwd": t_step,
        "speedup_median": t_comp["median_ms"] / t_fused["median_ms"],
        "launches": {"fused": launches(fused), "composite": launches(composite), "whole_step": launches(whole_step)},
        "loss_dict_fused_vs_composite": same, "grad_rel_diff_pred_pos_logit": grad_diff,
        "stage2": res2,
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
