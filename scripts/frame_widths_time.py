"""frame_widths_time.py — the evaluation frame in one call at decoder widths 32 / 64 / 128 on one MI355X.

    python scripts/frame_widths_time.py [--frames 2000] [--warmup 300] [--out profiles/frame_widths_time.json]

One process, the geometry-derived 1 x 240 x 320 frame and the options of `bench.py --workload e2e` (shipped PointNets,
valid_stride for 10,000 valid points, 2 refine iterations). Rows:
  shipped 64/64/64      pipeline.FrameRunner -> lidf_frame_f32 (the anchor), eager and graph replay
  chain 64/64/64        the same decoders through lidf_frame_widths_f32 (FrameRunner(chain_route=True))
  32/32/32, 128/128/128 FrameRunner -> lidf_frame_widths_f32, eager and graph replay
  stepwise at the three widths: pipeline.lidf_forward + refine_forward (four host size reads per frame)
Per row: milliseconds per frame (wall clock over --frames back-to-back frames after --warmup, one synchronise at each
end), launches per frame (kernel and memset records of torch's profiler over one extra frame, as
scripts/train_step_time.py counts them) and the bytes of the runner's workspaces. Prints one JSON line; --out writes
it to a file too.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("frame_widths_time.py needs a GPU: a CPU run gives no time")
    from implicit_depth_amd import IEF, IMNet, PointNet2Stage, pipeline as pl
    from implicit_depth_amd.synthetic import init_decoder_params, synthetic_batch
    dev = torch.device("cuda:0")
    B, h, w = 1, 240, 320
    batch, feat = synthetic_batch(B, h, w, seed=77)
    batch = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in batch.items()}
    feat = feat.to(dev)
    torch.manual_seed(3)
    pnet = PointNet2Stage(6, 128, 32).to(dev).eval()
    pnet_r = PointNet2Stage(6, 128, 32).to(dev).eval()
    n_valid = int((batch["depth_corrupt"] != 0).sum().item())
    opt = pl.LidfOptions(valid_stride=max(1, n_valid // (10000 * B)))

    def decoders(gf):
        prob = IMNet(385, 1, gf).to(dev).eval()
        off = IEF(dev, 385, 1, gf, n_iter=2).to(dev).eval()
        offr = IEF(dev, 334, 1, gf, n_iter=2).to(dev).eval()
        if gf == 64:   # bench.py's parameters
            prob.load_state_dict(init_decoder_params("IMNET", 385, 7, 5.0))
            off.load_state_dict(init_decoder_params("IEF", 385, 8, 5.0))
            offr.load_state_dict(init_decoder_params("IEF", 334, 9, 5.0))
        else:          # the reference's initialisation x 5, as those
            for m in (prob, off, offr):
                for p in m.parameters():
                    p.data.mul_(5.0)
        return prob, off, offr

    def timed(step):
        with torch.no_grad():
            for _ in range(args.warmup):
                step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.frames):
                step()
            torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.frames

    def launches(step):
        try:
            from torch.profiler import ProfilerActivity, profile
            with torch.no_grad():
                step()
                torch.cuda.synchronize()
                with profile(activities=[ProfilerActivity.CUDA]) as prof:
                    step()
                    torch.cuda.synchronize()
            return len([e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA])
        except Exception as e:   # the count is a by-product: a profiler problem must not lose the times
            return "not measured (%s)" % type(e).__name__

    rows = []
    for gf, chain in ((64, False), (64, True), (32, False), (128, False)):
        prob, off, offr = decoders(gf)
        sizes = None
        for mode in ("eager", "graph"):
            runner = pl.FrameRunner(B, h, w, dev, pnet, prob, off, opt, pnet_r, offr, chain_route=chain,
                                    side_stream=False)
            with torch.no_grad():
                runner.load(batch, feat)
                if mode == "graph":
                    runner.capture()
            step = lambda r=runner: r.run(batch, feat)   # noqa: E731
            ms = timed(step)
            ok, dd = runner.result()
            assert ok
            sizes = {"R": dd["counts"]["R"], "P": dd["counts"]["P"], "V": dd["counts"]["V"]}
            ws = runner.ws.numel() + (runner.ws_widths.numel() if runner.widths else 0)
            rows.append({"route": "lidf_frame_widths_f32" if runner.widths else "lidf_frame_f32", "gf": [gf] * 3,
                         "mode": mode, "ms_per_frame": round(ms, 4),
                         "launches_per_frame": launches(step) if mode == "eager" else "one graph replay",
                         "workspace_bytes": ws, "max_pairs": runner.max_pairs,
                         "pe_slab": int(runner.wd.pe_slab_pairs) if runner.widths else None, "counts": sizes})
            del runner
        if not chain:
            def stepwise():
                ok, dd = pl.lidf_forward(batch, feat, pnet, prob, off, opt)
                assert ok
                pl.refine_forward(dd, pnet_r, offr, opt)
            rows.append({"route": "lidf_forward + refine_forward", "gf": [gf] * 3, "mode": "stepwise",
                         "ms_per_frame": round(timed(stepwise), 4), "launches_per_frame": launches(stepwise),
                         "workspace_bytes": None, "counts": sizes})
    res = {"what": "evaluation frame in one call at decoder widths 32 / 64 / 128 against the stepwise path",
           "device": torch.cuda.get_device_name(0), "frame": [B, h, w], "frames": args.frames, "warmup": args.warmup,
           "clock": "wall clock over back-to-back frames, one synchronise at each end; no metrics kernel", "rows": rows}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
