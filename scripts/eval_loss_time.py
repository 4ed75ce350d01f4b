"""eval_loss_time.py — time of the evaluation-flavour losses ('valid') on the device, by HIP events.

Writes profiles/eval_loss_time.json: for both stages, ms per call of losses.lidf_loss / refine_loss (the HIP kernels)
and of their float32 torch-op twins losses.lidf_loss_composite / refine_loss_composite (the route a user has without
the kernels), at 1 x 240 x 320 with every pixel queried (the shipped validation shape, the bs == 1 branch) and at
8 x 240 x 320 with a mask of about 30 % of the pixels (the ray branch). Launches per call of the HIP route are those of
its launch sequence, not measured here. Warm-up calls first, then the median of REPS timed groups.

    python scripts/eval_loss_time.py [--reps 20] [--inner 10]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_case(bs, h, w, frac, dev, seed=0):
    """A data_dict for the four loss functions: a smooth surface, the queried pixels in torch.nonzero's order, three
    pairs per ray, compute_gt's entries built directly."""
    gen = torch.Generator().manual_seed(seed)
    ys, xs = torch.meshgrid(torch.arange(h).float(), torch.arange(w).float(), indexing="ij")
    z = 1.0 + 0.001 * xs + 0.002 * ys
    xyz = torch.stack(((xs - w / 2) * z / 200.0, (ys - h / 2) * z / 200.0, z), -1).reshape(1, h * w, 3).repeat(bs, 1, 1)
    xyz = (xyz + 0.003 * torch.randn(xyz.shape, generator=gen)).contiguous()
    mask = torch.rand((bs, h * w), generator=gen) < frac if frac < 1 else torch.ones((bs, h * w), dtype=torch.bool)
    nz = mask.nonzero()
    bid, flat = nz[:, 0].contiguous(), nz[:, 1].contiguous()
    R = bid.shape[0]
    corrupt = xyz.clone()
    corrupt[mask] = 0.0
    P = 3 * R
    table = torch.full((bs * h * w,), -1, dtype=torch.int32)
    table[bid * (h * w) + flat] = torch.arange(R, dtype=torch.int32)
    label = torch.zeros(P, dtype=torch.int64)
    label[1::3] = 1
    pred = xyz[bid, flat] + 0.02 * torch.randn((R, 3), generator=gen)
    dd = {"bs": bs, "h": h, "w": w, "xyz_flat": xyz, "xyz_corrupt_flat": corrupt, "corrupt_mask": mask.reshape(bs, h, w).float(),
          "ray_bid": bid.int(), "ray_flat": flat.int(), "gt_pos": xyz[bid, flat].contiguous(), "pix2ray": table,
          "pair_off": (3 * torch.arange(R + 1)).int(), "pair_ray": torch.arange(R).repeat_interleave(3),
          "pcl_label": label, "gt_max_pair_id": 3 * torch.arange(R) + 1,
          "n_label": torch.tensor([R], dtype=torch.int32), "pred_pos": pred.contiguous(),
          "pred_pos_refine": (pred + 0.005).contiguous(), "pred_prob_end": torch.randn((P, 1), generator=gen)}
    dd = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in dd.items()}
    dd["n_label"] = dd["n_label"][0]
    return dd, R


def time_ms(fn, reps, inner):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / inner)
    times.sort()
    return {"median_ms": times[len(times) // 2], "min_ms": times[0], "max_ms": times[-1]}


def main():
    from implicit_depth_amd import lidf_loss, lidf_loss_composite, refine_loss, refine_loss_composite
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "inner": a.inner, "exp_type": "valid",
           "baseline": "losses.*_composite, float32 torch ops on the device", "cases": []}
    for name, bs, frac in (("1x240x320_all", 1, 1.0), ("8x240x320_pred", 8, 0.3)):
        dd, R = make_case(bs, 240, 320, frac, dev)
        row = {"case": name, "rays": R, "pairs": 3 * R}
        for stage, hip, comp in ((1, lidf_loss, lidf_loss_composite), (2, refine_loss, refine_loss_composite)):
            row["stage%d_hip" % stage] = time_ms(lambda: hip(dd, None, "valid", 0), a.reps, a.inner)
            row["stage%d_torch_ops" % stage] = time_ms(lambda: comp(dd, None, "valid", 0), a.reps, max(a.inner // 5, 1))
        out["cases"].append(row)
        print(json.dumps(row))
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "eval_loss_time.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
