"""roi_backward_time.py — what the bit-reproducible RoIAlign adjoint (roi_backward="ordered") costs.

    python scripts/roi_backward_time.py [--reps 30] [--warmup 5] [--head TEXT] [--out profiles/roi_backward_time.json]

The driver (no GPU of its own) starts one child process under a time limit. The child measures, in one session with
device events around each call and the routes alternating inside the timed loop:
  adjoint   d full_rgb_feat from d rayfeat at 8 x 240 x 320 with the 160,000 window rays of the synthetic training
            geometry (implicit_depth_amd/synthetic.py, 20,000 per image), and at 1 x 240 x 320 with every pixel a ray:
              default    lidf_ray_features_backward_f32 with its whole workspace (float atomics at the border),
              ordered    lidf_ray_features_backward_ordered_f32,
              baseline   lidf_roi_align_backward_f32 on the same inputs (32 channels, 2 bins): the reproducible
                         adjoint a caller could assemble before the ordered route existed.
            The ordered route must not be slower than the baseline (median, no margin): the script records the
            verdict and exits with status 1 when it is. Its time against the default route is reported, not bounded.
  step      pipeline.lidf_forward_train forward + backward on the 8-frame synthetic batch with both settings.
Prints one JSON line; --out writes it to a file too. --head records the source revision when the tree that runs is
not a git checkout. A development aid: bench.py does not run it.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LIMIT_S = 420
B, H, W = 8, 240, 320


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


def adjoint_calls(dev, ray_pix, ray_bid, nb, bbox, lv, seed):
    """{column: fn} on one ray set, every call writing a d_feat_grid of its own, and those outputs."""
    import torch
    from implicit_depth_amd import _lib
    L = _lib.lib()
    R = ray_pix.shape[0]
    gen = torch.Generator(device=dev).manual_seed(seed)
    g = torch.randn(R, 128 + 3 + 6 * lv, generator=gen, device=dev)
    g_roi = g[:, :128].contiguous()
    out = {k: torch.empty(nb, 32, H, W, device=dev) for k in ("default", "ordered", "baseline")}
    wsb = L.lidf_ray_features_backward_ordered_workspace_bytes(nb, H, W)
    wsb_base = L.lidf_roi_align_backward_workspace_bytes(nb, H, W)
    ws, ws_base = _lib.workspace(wsb, dev), _lib.workspace(wsb_base, dev)

    def feat_entry(fn, dst):
        _lib.check(fn(_lib.ptr(g), _lib.ptr(ray_pix), _lib.ptr(ray_bid), R, nb, H, W, bbox, lv, _lib.ptr(dst),
                      _lib.ptr(ws), wsb, _lib.current_stream(dev)))

    def baseline():
        _lib.check(L.lidf_roi_align_backward_f32(
            _lib.ptr(g_roi), 128, _lib.ptr(ray_pix), _lib.ptr(ray_bid), R, nb, 32, H, W, bbox, 2,
            _lib.ptr(out["baseline"]), _lib.ptr(ws_base), wsb_base, _lib.current_stream(dev)))

    return {"default": lambda: feat_entry(L.lidf_ray_features_backward_f32, out["default"]),
            "ordered": lambda: feat_entry(L.lidf_ray_features_backward_ordered_f32, out["ordered"]),
            "baseline": baseline}, out


def measure(reps, warmup):
    import numpy as np
    import torch
    from implicit_depth_amd import LidfOptions, lidf_forward_train, pipeline
    from implicit_depth_amd.synthetic import init_decoder_params, synthetic_batch
    from util import make_module, make_pointnet, orc
    dev = torch.device("cuda:0")
    batch, feat = synthetic_batch(B, H, W, seed=3, hole_frac=1.9)
    batch = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in batch.items()}
    feat = feat.to(dev)
    np.random.seed(77)
    opt = LidfOptions()
    ok, dd = pipeline._train_geometry(batch, feat, opt, None)
    assert ok and dd["miss_ray_dir"].shape[0] == B * 20000
    half = opt.roi_inp_bbox // 2
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.int32), torch.arange(W, dtype=torch.int32), indexing="ij")
    sets = {"8x240x320_window_rays": (dd["ray_pix"].to(torch.int32).contiguous(),
                                      dd["ray_bid"].to(torch.int32).contiguous(), B),
            "1x240x320_every_pixel": (torch.stack((xs.reshape(-1), ys.reshape(-1)), 1).contiguous().to(dev),
                                      torch.zeros(H * W, dtype=torch.int32, device=dev), 1)}
    res = {"adjoint": {}}
    verdict = True
    for name, (pix, bid, nb) in sets.items():
        calls, out = adjoint_calls(dev, pix, bid, nb, opt.roi_inp_bbox, opt.multires_views, 5)
        row = dict(zip(calls, timed(list(calls.values()), reps, warmup)))
        x, y = pix[:, 0], pix[:, 1]
        clamped = int(((x < half) | (x > W - 1 - half) | (y < half) | (y > H - 1 - half)).sum())
        row["rays"], row["rays_with_a_clamped_box"] = int(pix.shape[0]), clamped
        scale = float(out["baseline"].abs().max())
        row["max_abs_difference_ordered_vs_baseline"] = float((out["ordered"] - out["baseline"]).abs().max())
        row["max_abs_difference_default_vs_baseline"] = float((out["default"] - out["baseline"]).abs().max())
        row["max_abs_gradient"] = scale
        first = out["ordered"].clone()
        calls["ordered"]()
        row["ordered_second_run_bit_identical"] = bool(torch.equal(first, out["ordered"]))
        row["ordered_over_default_median"] = row["ordered"]["median_ms"] / row["default"]["median_ms"]
        row["ordered_over_baseline_median"] = row["ordered"]["median_ms"] / row["baseline"]["median_ms"]
        row["ordered_not_slower_than_baseline"] = row["ordered"]["median_ms"] <= row["baseline"]["median_ms"]
        verdict = verdict and row["ordered_not_slower_than_baseline"]
        res["adjoint"][name] = row
    res["ordered_not_slower_than_baseline"] = verdict
    # the whole stage-1 step, both settings
    mods = (make_pointnet(orc.init_pointnet(3, 1.5), dev).train(),
            make_module("IMNET", init_decoder_params("IMNET", 385, 7, 5.0), 385, dev).train(),
            make_module("IEF", init_decoder_params("IEF", 385, 8, 5.0), 385, dev).train())

    def step(route):
        for m in mods:
            for q in m.parameters():
                q.grad = None
        f = feat.clone().requires_grad_()
        np.random.seed(77)
        ok, _, loss = lidf_forward_train(batch, f, *mods, opt=LidfOptions(roi_backward=route), epoch=0)
        assert ok
        loss["loss_net"].backward()
        return f.grad

    steps = {"atomic": lambda: step("atomic"), "ordered": lambda: step("ordered")}
    row = dict(zip(steps, timed(list(steps.values()), max(reps // 3, 5), min(warmup, 3))))
    row["ordered_over_atomic_median"] = row["ordered"]["median_ms"] / row["atomic"]["median_ms"]
    row["ordered_second_run_bit_identical"] = bool(torch.equal(step("ordered"), step("ordered")))
    res["lidf_forward_train_forward_backward_8_frames"] = row
    torch.cuda.synchronize()
    res["device"] = torch.cuda.get_device_name(0)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--head", default=None)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("roi_backward_time.py needs a GPU: a CPU run gives no time")
        print("LEG_RESULT " + json.dumps(measure(args.reps, args.warmup)))
        return
    head = args.head
    if head is None:
        try:
            head = subprocess.run(["git", "-C", ROOT, "describe", "--always", "--dirty"], stdout=subprocess.PIPE,
                                  stderr=subprocess.DEVNULL, text=True, check=True).stdout.strip()
        except (OSError, subprocess.CalledProcessError):
            head = "unknown (not a git checkout)"
    res = {"what": "RoIAlign's adjoint to full_rgb_feat at the shipped widths: the default route "
                   "(lidf_ray_features_backward_f32, float atomics at the border), the ordered route "
                   "(lidf_ray_features_backward_ordered_f32) and the baseline lidf_roi_align_backward_f32 (the "
                   "reproducible adjoint before the ordered route); lidf_forward_train forward + backward with "
                   "roi_backward 'atomic' and 'ordered'",
           "clock": "device events around each call, %d repetitions after %d, routes alternating, one session"
                    % (args.reps, args.warmup),
           "git_head": head}
    status = 0
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps),
                            "--warmup", str(args.warmup)],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=LIMIT_S)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("LEG_RESULT ")]
        if p.returncode != 0 or not lines:
            res["result"], status = "not measured: exit status %d: %s" % (p.returncode, p.stderr.strip()[-400:]), 2
        else:
            res["result"] = json.loads(lines[-1][len("LEG_RESULT "):])
            status = 0 if res["result"]["ordered_not_slower_than_baseline"] else 1
    except subprocess.TimeoutExpired:
        res["result"], status = "not measured: the run reached its limit of %d s" % LIMIT_S, 2
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    sys.exit(status)


if __name__ == "__main__":
    main()
