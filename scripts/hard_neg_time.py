"""hard_neg_time.py — what hard-negative mining costs in the two loss nodes on one MI355X, by route.

    python scripts/hard_neg_time.py [--reps 200] [--warmup 50] [--head TEXT] [--out profiles/hard_neg_time.json]

The driver (no GPU of its own) starts one child process per leg, each under its own time limit, and stops at the
first leg that fails: nothing further is started on a device a leg may have faulted.
  time      loss forward + backward of refine_loss and of lidf_loss at 8 x 20,000 rays (the 8 x 240 x 320 synthetic
            training geometry of implicit_depth_amd/synthetic.py, its pairs and labels), each with hard_neg off, with
            LidfLossOptions.hard_neg_select = "torch" (torch.topk per term) and with "device" (csrc/lidf_select.hip).
            Device events around each call, the three variants alternating inside the timed loop, after a warm-up of
            each. The yardstick of the device route is the torch route of the same session.
  launches  the same six calls once each under a kernel trace (torch.profiler's device activities) in a process of
            their own: kernels and memory operations enqueued by one forward + backward.
Prints one JSON line; --out writes it to a file too. --head records the source revision when the tree that runs is
not a git checkout.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LEG_LIMIT_S = {"time": 400, "launches": 240}
B, H, W = 8, 240, 320
VARIANTS = (("hard_neg_off", dict()),
            ("torch", dict(hard_neg=True, hard_neg_ratio=0.1, hard_neg_select="torch")),
            ("device", dict(hard_neg=True, hard_neg_ratio=0.1, hard_neg_select="device")))


def stats(v):
    import numpy as np
    return {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "p90_ms": float(np.percentile(v, 90)),
            "reps": len(v)}


def timed(fns, reps, warmup):
    """Device events around each call, the variants alternating."""
    import torch
    for fn in fns:
        for _ in range(warmup):
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
    return [stats(v) for v in ms]


def build_calls():
    """{stage: {variant: fn}} — fn runs one loss forward + backward on fixed inputs — and the shapes."""
    import numpy as np
    import torch
    from implicit_depth_amd import LidfLossOptions, LidfOptions, lidf_forward_train, lidf_loss, refine_loss
    from implicit_depth_amd.synthetic import init_decoder_params, synthetic_batch
    from util import make_module, make_pointnet, orc
    dev = torch.device("cuda:0")
    batch, feat = synthetic_batch(B, H, W, seed=3, hole_frac=1.9)
    batch = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in batch.items()}
    pnet = make_pointnet(orc.init_pointnet(3, 1.5), dev).train()
    prob = make_module("IMNET", init_decoder_params("IMNET", 385, 7, 5.0), 385, dev).train()
    off = make_module("IEF", init_decoder_params("IEF", 385, 8, 5.0), 385, dev).train()
    np.random.seed(77)
    ok, dd, _ = lidf_forward_train(batch, feat.to(dev).requires_grad_(True), pnet, prob, off, opt=LidfOptions(),
                                   loss_opt=LidfLossOptions(smooth_w=0.5), epoch=0)
    assert ok
    R, P = dd["gt_pos"].shape[0], dd["pcl_label"].shape[0]
    assert R == B * 20000
    base = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in dd.items()}
    gen = torch.Generator().manual_seed(11)
    refined = (base["pred_pos"] + 0.01 * torch.randn(R, 3, generator=gen).to(dev)).contiguous()
    calls = {"refine_loss": {}, "lidf_loss": {}}
    for name, kw in VARIANTS:
        opt2 = LidfLossOptions(pos_w=20.0, surf_norm_w=2.0, smooth_w=0.5, **kw)   # train_refine_hardneg.yaml's weights
        opt1 = LidfLossOptions(smooth_w=0.5, **kw)

        def stage2(opt=opt2):
            d = dict(base)
            d["pred_pos_refine"] = refined.clone().requires_grad_(True)
            refine_loss(d, opt)["loss_net"].backward()
            return d["pred_pos_refine"].grad

        def stage1(opt=opt1):
            d = dict(base)
            d["pred_pos"] = base["pred_pos"].clone().requires_grad_(True)
            d["pred_prob_end"] = base["pred_prob_end"].clone().requires_grad_(True)
            lidf_loss(d, opt)["loss_net"].backward()
            return d["pred_pos"].grad

        calls["refine_loss"][name], calls["lidf_loss"][name] = stage2, stage1
    shapes = {"frames": [B, H, W], "rays": R, "pairs": P, "labelled_pairs": int(dd["n_label"]),
              "hard_neg_ratio": 0.1, "k_rays": int(R * 0.1), "k_pairs": int(int(dd["n_label"]) * 0.1)}
    return calls, shapes


def leg_time(reps, warmup):
    import torch
    calls, shapes = build_calls()
    out = {"shapes": shapes}
    for stage, fns in calls.items():
        # the two routes select the same elements unless values tie at the k-th place: the gradients agree to the
        # means' rounding wherever both are finite
        g_t, g_d = fns["torch"](), fns["device"]()
        diff = float((g_t - g_d).abs().max())
        t = timed(list(fns.values()), reps, warmup)
        row = dict(zip(fns, t))
        row["gradient_max_abs_difference_torch_vs_device"] = diff
        row["device_over_torch_median"] = row["device"]["median_ms"] / row["torch"]["median_ms"]
        row["mining_cost_ms"] = {k: row[k]["median_ms"] - row["hard_neg_off"]["median_ms"] for k in ("torch", "device")}
        row["device_no_slower"] = row["device"]["median_ms"] <= row["torch"]["median_ms"]
        out[stage] = row
    torch.cuda.synchronize()
    return out


def leg_launches(reps, warmup):
    import torch
    from torch.profiler import ProfilerActivity, profile
    calls, _ = build_calls()
    out = {}
    for stage, fns in calls.items():
        out[stage] = {}
        for name, fn in fns.items():
            fn()
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                fn()
                torch.cuda.synchronize()
            ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
            mem = [e for e in ev if e.name.lower().startswith(("memset", "memcpy"))]
            out[stage][name] = {"kernels": len(ev) - len(mem), "memory_ops": len(mem),
                                "select_kernels": len([e for e in ev if "lidf_select" in e.name])}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--head", default=None)
    ap.add_argument("--leg", default=None, choices=sorted(LEG_LIMIT_S))
    args = ap.parse_args()
    if args.leg:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("hard_neg_time.py needs a GPU: a CPU run gives no time")
        res = {"time": leg_time, "launches": leg_launches}[args.leg](args.reps, args.warmup)
        res["device"] = torch.cuda.get_device_name(0)
        print("LEG_RESULT " + json.dumps(res))
        return
    head = args.head
    if head is None:
        try:
            head = subprocess.run(["git", "-C", ROOT, "describe", "--always", "--dirty"], stdout=subprocess.PIPE,
                                  stderr=subprocess.DEVNULL, text=True, check=True).stdout.strip()
        except (OSError, subprocess.CalledProcessError):
            head = "unknown (not a git checkout)"
    res = {"what": "hard-negative mining in refine_loss / lidf_loss: off, torch.topk per term, the device select "
                   "(lidf_select.hip); loss forward + backward",
           "clock": "device events around each call, %d repetitions after %d, variants alternating, one session"
                    % (args.reps, args.warmup),
           "launch_counts": "torch.profiler device activities of one forward + backward, in a process of its own",
           "git_head": head}
    for leg in ("time", "launches"):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg, "--reps", str(args.reps),
                                "--warmup", str(args.warmup)],
                               stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=LEG_LIMIT_S[leg])
        except subprocess.TimeoutExpired:
            res[leg] = "not measured: the leg ran into its limit of %d s" % LEG_LIMIT_S[leg]
            break
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("LEG_RESULT ")]
        if p.returncode != 0 or not lines:
            res[leg] = "not measured: exit status %d: %s" % (p.returncode, p.stderr.strip()[-400:])
            break
        res[leg] = json.loads(lines[-1][len("LEG_RESULT "):])
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
