"""sampler_time.py — times of the device-side valid-point sampler (lidf_sample_valid_points) on one MI355X.

    python scripts/sampler_time.py [--reps 50] [--out profiles/sampler_time.json]

The driver (no GPU of its own) starts one child process per leg, each under its own time limit, and stops at the
first leg that fails: nothing further is started on a device a leg may have faulted.
  sampler  1 x 240 x 320 and 8 x 240 x 320 masks of density ~0.7, n = 10000:
           device   query.sample_valid_launch into preallocated buffers (three launches + the counter's add)
           torch    the reference's per-image loop (utils/point_utils.py:79-125) restated with the same torch / numpy
                    calls on the same masks — what a caller of the shipped configs runs today
           The two alternate inside the timed loop, device events around each call, after a warm-up of both.
  frame    FrameRunner on the 1 x 240 x 320 synthetic frame, stage 1 + 2 as a captured graph: valid_sample_num = 10000
           against the valid_stride frame (bench.py's stand-in), alternating replays; launches per frame from
           torch's profiler.
Prints one JSON line; --out writes it to a file too.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LEG_LIMIT_S = {"sampler": 240, "frame": 240}


def stats(v):
    import numpy as np
    return {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "p90_ms": float(np.percentile(v, 90)),
            "reps": len(v)}


def timed(fns, reps, warmup=5):
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


def torch_reference_loop(mask, n):
    """The reference's sampler as callers run it today, restated: block-ordered nonzero, unique_consecutive, then
    per image tensor-valued size comparisons (host reads) and np.random.choice / torch.randint / torch.randperm."""
    import numpy as np
    import torch
    bs, h, w = mask.shape
    dev = mask.device
    blocks = mask.reshape(bs, h // 8, 8, w // 8, 8).permute(0, 1, 3, 2, 4).contiguous()
    nz = torch.nonzero(blocks)
    _, per_image = torch.unique_consecutive(nz[:, 0], return_counts=True)
    ends = torch.cumsum(per_image, 0)
    start = torch.zeros((), dtype=torch.long, device=dev)
    picks = []
    for i in range(ends.shape[0]):
        end = ends[i]
        cnt = end - start
        if cnt < n:
            own = torch.arange(int(start), int(end), device=dev)
            pool = own.repeat(int(np.ceil(float(n) / float(cnt)) - 1))
            extra = np.random.choice(pool.shape[0], int(n - cnt), replace=False)
            picks.append(torch.cat((own, pool[torch.from_numpy(extra).to(dev)])))
        else:
            step = cnt // n
            inum = int(cnt // step)
            off = torch.randint(0, int(step), (inum,)).to(dev)
            sel = start + off + step * torch.arange(inum, device=dev)
            picks.append(sel[torch.randperm(inum)[:n].to(dev)])
        start = end
    p = nz[torch.cat(picks)]
    flat = (p[:, 1] * 8 + p[:, 3]) * w + p[:, 2] * 8 + p[:, 4]
    return torch.stack((p[:, 0], flat), -1)


def leg_sampler(reps):
    import numpy as np
    import torch
    import sampler_ref as sr
    from implicit_depth_amd import query as Q
    dev = torch.device("cuda:0")
    n, out = 10000, {}
    for bs in (1, 8):
        rng = np.random.default_rng(bs)
        mask_np = (rng.random((bs, 240, 320)) < 0.7).astype(np.float32)
        mask = torch.from_numpy(mask_np).to(dev)
        state = Q.sampler_state(7, dev)
        bid = torch.empty((bs * n,), dtype=torch.int32, device=dev)
        flat, cnt = torch.empty_like(bid), torch.empty((bs,), dtype=torch.int32, device=dev)
        ws = Q.sample_valid_workspace(bs, 240, 320, dev)

        def device():
            Q.sample_valid_launch(mask, n, state, bid, flat, None, cnt, ws)

        def reference():
            return torch_reference_loop(mask, n)

        device()
        got = torch.stack((bid, flat), 1).cpu().numpy()
        sr.check_sample(mask_np, n, got)                       # both are valid samples of the same masks
        sr.check_sample(mask_np, n, reference().cpu().numpy())
        t_dev, t_ref = timed((device, reference), reps)
        # the library call alone: 20 calls back to back between one pair of events (no counter add, no Python gap)
        L = Q._lib.lib()
        args = (Q._lib.ptr(mask), 0, bs, 240, 320, n, Q._lib.ptr(state), Q._lib.ptr(bid), Q._lib.ptr(flat), None,
                Q._lib.ptr(cnt), Q._lib.ptr(ws), ws.numel(), Q._lib.current_stream(dev))

        def burst():
            for _ in range(20):
                L.lidf_sample_valid_points(*args)

        (t_burst,) = timed((burst,), max(reps // 5, 5))
        out["%dx240x320" % bs] = {
            "valid_per_image": [int(v) for v in mask_np.reshape(bs, -1).sum(1)], "sample_num": n,
            "device_call": t_dev, "torch_reference_loop": t_ref,
            "library_call_alone_ms": {k: (v / 20 if k != "reps" else v) for k, v in t_burst.items()},
            "speedup_median": t_ref["median_ms"] / t_dev["median_ms"],
            "device_faster": t_dev["median_ms"] < t_ref["median_ms"],
        }
    return out


def leg_frame(reps):
    import torch
    from implicit_depth_amd import pipeline as pl
    from implicit_depth_amd.synthetic import init_decoder_params, synthetic_batch
    from util import make_module, make_pointnet, orc
    dev = torch.device("cuda:0")
    B, h, w, n = 1, 240, 320, 10000
    batch, feat = synthetic_batch(B, h, w, seed=77)
    batch = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in batch.items()}
    feat = feat.to(dev)
    models = (make_pointnet(orc.init_pointnet(3, 1.5), dev),
              make_module("IMNET", init_decoder_params("IMNET", 385, 7, 5.0), 385, dev),
              make_module("IEF", init_decoder_params("IEF", 385, 8, 5.0), 385, dev))
    refine = dict(pnet_model_refine=make_pointnet(orc.init_pointnet(4, 1.5), dev),
                  offset_dec_refine=make_module("IEF", init_decoder_params("IEF", 334, 9, 5.0), 334, dev))
    n_valid = int((batch["depth_corrupt"] != 0).sum().item())
    stride = max(1, n_valid // (n * B))
    runners = {"valid_stride": pl.FrameRunner(B, h, w, dev, *models, pl.LidfOptions(valid_stride=stride), **refine),
               "valid_sample_num": pl.FrameRunner(B, h, w, dev, *models, pl.LidfOptions(valid_sample_num=n),
                                                  sampler_state=pl.Q.sampler_state(7, dev), **refine)}
    counts = {}
    with torch.no_grad():
        for k, r in runners.items():
            r.load(batch, feat)
            r.capture()
            r.run()
            ok, dd = r.result()
            assert ok
            counts[k] = {c: dd["counts"][c] for c in ("NVS", "V", "R", "P")}
    fns = [lambda r=r: r.run() for r in runners.values()]
    with torch.no_grad():
        t = timed(fns, reps)

    def launches(fn):
        try:
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                fn()
                torch.cuda.synchronize()
            return len([e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA])
        except Exception as e:   # the count is a by-product: a profiler problem must not lose the times
            return "not measured (%s)" % type(e).__name__

    with torch.no_grad():
        ln = [launches(fn) for fn in fns]
    out = {"frame": "%dx%dx%d, stage 1 + 2, captured graph, f32" % (B, h, w), "valid_pixels": n_valid, "stride": stride}
    for (k, _), tk, lk in zip(runners.items(), t, ln):
        out[k] = {"per_frame": tk, "launches": lk, "counts": counts[k]}
    out["sampled_minus_stride_median_ms"] = t[1]["median_ms"] - t[0]["median_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default=None, choices=sorted(LEG_LIMIT_S))
    args = ap.parse_args()
    if args.leg:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("sampler_time.py needs a GPU: a CPU run gives no time")
        res = {"sampler": leg_sampler, "frame": leg_frame}[args.leg](args.reps)
        res["device"] = torch.cuda.get_device_name(0)
        print("LEG_RESULT " + json.dumps(res))
        return
    res = {"what": "device-side valid-point sampler (lidf_sample.hip): ballot, scan and sampling launches",
           "clock": "device events around each call, variants alternating, one session"}
    for leg in ("sampler", "frame"):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg, "--reps", str(args.reps)],
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
