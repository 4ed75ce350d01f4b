"""miss_window_time.py — times of the device-side miss-ray window (lidf_miss_ray_window_f32) on one MI355X.

    python scripts/miss_window_time.py [--reps 50] [--out profiles/miss_window_time.json]

The driver (no GPU of its own) starts one child process per leg, each under its own time limit, and stops at the
first leg that fails: nothing further is started on a device a leg may have faulted.
  window  8 x 240 x 320 corrupt masks of density ~0.35 (every image holds more than 20,000 corrupt pixels: the shipped
          situation) and 1 x 240 x 320 of density ~0.2 (nothing is sampled), n = 20000:
          device  query.sample_miss_window                     (three launches, the counter's add, one read)
          numpy   query.get_miss_ray + query.sample_miss_rays  (today's route: two reads, np.random.choice per image)
          Both routes block on a read, so the host's wall time from the call to the returned dict is recorded next to
          the device events around the call. The two alternate inside the timed loop after a warm-up of both.
          Launches per call from torch's profiler.
  step    pipeline.lidf_forward_train, forward + backward, on the 8-frame synthetic batch of scripts/train_step_time.py:
          miss_sample = 'device' against 'numpy', alternating, the median over the groups.
Prints one JSON line; --out writes it to a file too.
"""
import argparse
import datetime
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LEG_LIMIT_S = {"window": 240, "step": 400}


def stats(v):
    import numpy as np
    return {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "p90_ms": float(np.percentile(v, 90)),
            "reps": len(v)}


def timed(fns, reps, warmup=5):
    """Per call: device events around it and the host's wall clock from the call to its return (every variant ends
    on a blocking read or is followed by a synchronize), the variants alternating."""
    import torch
    for fn in fns:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ev, wall = [[] for _ in fns], [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record()
            fn()
            b.record()
            b.synchronize()
            wall[i].append((time.perf_counter() - t0) * 1e3)
            ev[i].append(a.elapsed_time(b))
    return [{"device_events": stats(e), "host_wall": stats(w)} for e, w in zip(ev, wall)]


def launches(fn):
    import torch
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return len([e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA])
    except Exception as e:   # the count is a by-product: a profiler problem must not lose the times
        return "not measured (%s)" % type(e).__name__


def leg_window(reps):
    import numpy as np
    import torch
    import miss_window_ref as mw
    from implicit_depth_amd import query as Q
    dev = torch.device("cuda:0")
    n, out = 20000, {}
    for bs, density in ((8, 0.35), (1, 0.2)):
        rng = np.random.default_rng(bs)
        mask_np = (rng.random((bs, 240, 320)) < density).astype(np.float32)
        mask = torch.from_numpy(mask_np).to(dev)
        one = torch.ones((bs,), device=dev)
        intr = (one * 300.0, one * 305.0, one * 159.5, one * 119.5)
        state = Q.sampler_state(7, dev)

        def device():
            return Q.sample_miss_window(mask, *intr, n, state=state)

        def numpy_route():
            return Q.sample_miss_rays(Q.get_miss_ray(mask, *intr), bs, n)

        # both are windows of the same mask first (faster and different is not faster)
        counter = int(state[1].item())
        got = device()
        want = mw.select(mask_np, n, seed=7, counter=counter)
        assert got["miss_window"].cpu().numpy().tolist() == want["window"].tolist()
        assert (got["miss_flat_img_id"].cpu().numpy() == want["miss_flat_img_id"]).all()
        ref = numpy_route()
        mw.check_window(mask_np, n, {k: ref[k].cpu().numpy() for k in ("miss_bid", "miss_flat_img_id")})
        t_dev, t_np = timed((device, numpy_route), reps)
        out["%dx240x320" % bs] = {
            "corrupt_per_image": [int(v) for v in mask_np.reshape(bs, -1).sum(1)], "miss_sample_num": n,
            "sampling": bool(bs * n < mask_np.sum()), "rays_out": int(want["n_rays"][0]),
            "device": dict(t_dev, launches=launches(device)), "numpy": dict(t_np, launches=launches(numpy_route)),
            "host_wall_speedup_median": t_np["host_wall"]["median_ms"] / t_dev["host_wall"]["median_ms"],
            "device_faster_host_wall": t_dev["host_wall"]["median_ms"] < t_np["host_wall"]["median_ms"],
            "device_faster_device_events": t_dev["device_events"]["median_ms"] < t_np["device_events"]["median_ms"],
        }
    return out


def leg_step(reps):
    import numpy as np
    import torch
    from implicit_depth_amd import LidfLossOptions, LidfOptions, lidf_forward_train
    from implicit_depth_amd import query as Q
    from implicit_depth_amd.synthetic import init_decoder_params, synthetic_batch
    from util import make_module, make_pointnet, orc
    dev = torch.device("cuda:0")
    B, h, w = 8, 240, 320
    batch, feat = synthetic_batch(B, h, w, seed=3, hole_frac=1.9)
    corrupt = [int(v) for v in batch["corrupt_mask"].reshape(B, -1).sum(1)]
    batch = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in batch.items()}
    feat = feat.to(dev).requires_grad_(True)
    mods = (make_pointnet(orc.init_pointnet(3, 1.5), dev).train(),
            make_module("IMNET", init_decoder_params("IMNET", 385, 7, 5.0), 385, dev).train(),
            make_module("IEF", init_decoder_params("IEF", 385, 8, 5.0), 385, dev).train())
    lopt = LidfLossOptions()
    opts = {"device": LidfOptions(miss_sample="device", sampler_state=Q.sampler_state(7, dev)),
            "numpy": LidfOptions()}
    sizes = {}

    def step(route):
        for m in mods:
            for p in m.parameters():
                p.grad = None
        feat.grad = None
        np.random.seed(77)
        ok, dd, loss = lidf_forward_train(batch, feat, *mods, opt=opts[route], loss_opt=lopt, epoch=0)
        assert ok
        loss["loss_net"].backward()
        torch.cuda.synchronize()
        sizes[route] = {"R": dd["total_miss_sample_num"], "P": int(dd["pair_ray"].shape[0])}

    fns = [lambda r=r: step(r) for r in opts]
    t = timed(fns, max(reps, 20), warmup=3)
    out = {"batch": "%dx%dx%d synthetic, hole_frac 1.9, miss_sample_num 20000" % (B, h, w), "corrupt_per_image": corrupt,
           "what": "lidf_forward_train forward + backward, ending on a synchronize"}
    for (route, _), tk, fn in zip(opts.items(), t, fns):
        out[route] = dict(tk, launches=launches(fn), **sizes[route])
    out["device_minus_numpy_host_wall_median_ms"] = t[0]["host_wall"]["median_ms"] - t[1]["host_wall"]["median_ms"]
    out["device_faster_host_wall"] = t[0]["host_wall"]["median_ms"] < t[1]["host_wall"]["median_ms"]
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
            raise SystemExit("miss_window_time.py needs a GPU: a CPU run gives no time")
        res = {"window": leg_window, "step": leg_step}[args.leg](args.reps)
        res["gpu"] = torch.cuda.get_device_name(0)   # ('device' is a route's name in both legs)
        print("LEG_RESULT " + json.dumps(res))
        return
    res = {"what": "device-side miss-ray window (lidf_sample.hip): block count, window and fill launches",
           "clock": "host wall clock from call to return and device events around each call, variants alternating, "
                    "one session",
           "date": datetime.date.today().isoformat()}
    for leg in ("window", "step"):
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
