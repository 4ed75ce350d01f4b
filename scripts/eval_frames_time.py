"""eval_frames_time.py — time of the per-frame evaluation losses and depth statistics of a batch, by HIP events.

Writes profiles/eval_frames_time.json: at 16 x 240 x 320 with every pixel queried and with about 12,000 rays per
frame, ms per call of
  leg 1  the per-frame call: lidf_loss / refine_loss(per_frame=True) and query.depth_metrics_frames alone;
  leg 2  what a caller did for the statistics before: 16 x query.depth_metrics on the frames;
  leg 3  what a caller did for the losses before: 16 x (losses.frame_slice + the bs == 1 call).
The method is scripts/eval_loss_time.py's: warm-up calls, then the median of REPS timed groups of INNER calls, one
session. The events bracket the host work of a leg as well (frame_slice reads two range ends per frame). Launches per
call are those of the launch sequences, not measured here.

    python scripts/eval_frames_time.py [--reps 20] [--inner 10] [--out profiles/eval_frames_time.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from eval_loss_time import make_case, time_ms  # noqa: E402  (scripts/ is the script's own directory)

LAUNCHES = {
    "per_frame_loss": "1 memset + 4 launches for the whole batch",
    "per_frame_statistics": "1 launch for the whole batch",
    "loop_statistics": "16 x 1 launch",
    "loop_loss": "16 x (1 memset + 4 launches) + 16 x frame_slice (torch ops and one host read each)",
}


def main():
    from implicit_depth_amd import frame_slice, lidf_loss, refine_loss
    from implicit_depth_amd import query as Q
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_frames_time.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, h, w = 16, 240, 320
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "inner": a.inner, "exp_type": "test",
           "launches": LAUNCHES, "cases": []}
    for name, frac in (("16x240x320_all", 1.0), ("16x240x320_12k_rays", 12000.0 / (h * w))):
        dd, R = make_case(B, h, w, frac, dev)
        depth = dd["xyz_corrupt_flat"][:, :, 2].reshape(-1).clone()
        depth[dd["ray_bid"].long() * (h * w) + dd["ray_flat"].long()] = dd["pred_pos"][:, 2]
        pred = depth.reshape(B, h, w)
        gt = dd["xyz_flat"][:, :, 2].reshape(B, h, w).contiguous()
        seg = dd["corrupt_mask"]
        row = {"case": name, "rays": R, "pairs": 3 * R}

        def loop(fn):
            for b in range(B):
                fn(frame_slice(dd, b), None, "test", 0)

        def loop_statistics():
            for b in range(B):
                Q.depth_metrics(pred[b], gt[b], seg[b])

        for stage, fn in ((1, lidf_loss), (2, refine_loss)):
            row["stage%d_per_frame" % stage] = time_ms(lambda: fn(dd, None, "test", 0, per_frame=True), a.reps, a.inner)
            row["stage%d_loop_of_one_frame_calls" % stage] = time_ms(lambda: loop(fn), a.reps, max(a.inner // 5, 1))
        row["statistics_per_frame"] = time_ms(lambda: Q.depth_metrics_frames(pred, gt, seg), a.reps, a.inner)
        row["statistics_loop_of_one_frame_calls"] = time_ms(loop_statistics, a.reps, a.inner)
        out["cases"].append(row)
        print(json.dumps(row))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
