"""chain_split_time.py — precision "f16x3" against "f32" at decoders of gf_dim 32 / 64 / 128 on one MI355X.

    python scripts/chain_split_time.py [--groups 5] [--reps 4] [--warmup 2] [--only a,b,c] [--out profiles/chain_split_time.json]

One process, one session; both precisions of a configuration are timed in alternating groups, so the f32 route of the
same session is the yardstick. Per precision: `groups` groups of `reps` back-to-back calls between two device events,
after `warmup` untimed calls; the figure is the median of the groups' means, the spread (max - min) / median of the
groups. Measurements:
  (a) the chain launch alone (generic.decoder_chain: lidf_decoder_chain_f32 / lidf_decoder_chain_split_f32, packed
      once, the later calls prepacked) on 4,915,200 rows x 102 columns with the query's two gathered tables, for the
      IMNet (one pass) and the IEF (two passes) of every width
  (b) lidf_query at the headline shape 240 x 320 rays x 64 candidates (bench.py's scene). gf_dim 32 / 128: lidf_query
      itself; gf_dim 64: generic.query, the 64-wide chain (lidf_query routes the shipped configuration to its
      fixed-width kernels, which this script does not time)
  (c) pipeline.lidf_forward + refine_forward, stepwise, on the 1 x 240 x 320 frame of `bench.py --workload e2e`
      (shipped PointNets, 2 refine iterations); gf_dim 64 runs the shipped fixed-width kernels here in both precisions
Prints one JSON line; --out writes it to a file too."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PRECISIONS = ("f32", "f16x3")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=5)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="a,b,c")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("chain_split_time.py needs a GPU: a CPU run gives no time")
    from implicit_depth_amd import IEF, IMNet, PointNet2Stage, generic, pipeline as pl
    from implicit_depth_amd.query import lidf_query
    from implicit_depth_amd.synthetic import init_decoder_params, synthetic_batch, synthetic_scene
    dev = torch.device("cuda:0")
    only = set(args.only.split(","))

    def module(kind, d, gf, seed):
        m = IEF(dev, d, 1, gf, n_iter=2) if kind == "IEF" else IMNet(d, 1, gf)
        m.load_state_dict(init_decoder_params(kind, d, seed, 5.0, gf=gf))
        return m.to(dev).eval()

    def timed(steps):
        """steps: {precision: callable}. Alternating groups; {precision: (median ms per call, spread)}."""
        ms = {p: [] for p in steps}
        with torch.no_grad():
            for p, step in steps.items():
                for _ in range(args.warmup):
                    step()
            torch.cuda.synchronize()
            for _ in range(args.groups):
                for p, step in steps.items():
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(args.reps):
                        step()
                    b.record()
                    b.synchronize()
                    ms[p].append(a.elapsed_time(b) / args.reps)
        return {p: (statistics.median(v), (max(v) - min(v)) / statistics.median(v)) for p, v in ms.items()}

    def row(what, gf, points, t, **extra):
        r = {"measurement": what, "gf": gf, "points": points}
        for p, (m, spread) in t.items():
            r[p] = {"ms": round(m, 4), "mpoints_per_s": round(points / m / 1e3, 2), "spread": round(spread, 4)}
        r["f16x3_over_f32"] = round(t["f32"][0] / t["f16x3"][0], 3)
        r.update(extra)
        print(json.dumps(r), flush=True)
        return r

    rows = []
    scene = synthetic_scene(1, 240, 320, 64, seed=1235)
    s = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in scene.items()}
    P, D, E2 = scene["P"], scene["D"], 102
    qargs = (s["ray_dir"], s["ray_pix"].int(), s["ray_bid"].int(), s["pair_off"], s["pair_ray"], s["pair_vox"], s["pair_t"],
             s["feat_grid"], s["vox_feat"])

    if "a" in only:
        # the operand and tables of the query's chain launch: embedding rows [P, 102] with 16 floats of slack behind
        # them, a per-voxel table with the bias and a per-ray table, gathered by the scene's own index arrays
        g = torch.Generator(device=dev).manual_seed(1)
        pe = torch.zeros((P * E2 + 16,), dtype=torch.float32, device=dev)
        pe = pe[:P * E2].uniform_(-1.0, 1.0, generator=g).view(P, E2)      # (sin / cos values and positions: |x| <= 1)
        for gf in (32, 64, 128):
            for kind in ("IMNET", "IEF"):
                mod = module(kind, D, gf, 7 if kind == "IMNET" else 8)
                voxpart = torch.randn(scene["V"], 4 * gf, generator=g, device=dev)
                raypart = torch.randn(scene["R"], 4 * gf, generator=g, device=dev)
                out = torch.empty((P, 1), dtype=torch.float32, device=dev)
                packs = {p: {} for p in PRECISIONS}
                steps = {p: (lambda p=p: generic.decoder_chain(
                    mod, pe, E2, w1_col0=256, voxpart=voxpart, vox_idx=s["pair_vox"], raypart=raypart,
                    ray_idx=s["pair_ray"], out=out, padded=True, packed=packs[p], precision=p)) for p in PRECISIONS}
                rows.append(row("a: chain launch alone", gf, P, timed(steps), kind=kind,
                                passes=2 if kind == "IEF" else 1, columns=E2))
        del pe

    if "b" in only:
        for gf in (32, 64, 128):
            prob, off = module("IMNET", D, gf, 7), module("IEF", D, gf, 8)
            if gf == 64:
                steps = {p: (lambda p=p: generic.query(*qargs, prob, off, 8, 4, 8, 2, (0.0, 1.0), 0.25, None, False,
                                                       None, None, False, precision=p)) for p in PRECISIONS}
                route = "generic.query (the 64-wide chain)"
            else:
                steps = {p: (lambda p=p: lidf_query(*qargs, prob, off, precision=p)) for p in PRECISIONS}
                route = "lidf_query"
            rows.append(row("b: query, 240 x 320 x 64", gf, P, timed(steps), route=route))

    if "c" in only:
        B, h, w = 1, 240, 320
        batch, feat = synthetic_batch(B, h, w, seed=77)
        batch = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in batch.items()}
        feat = feat.to(dev)
        torch.manual_seed(3)
        pnet = PointNet2Stage(6, 128, 32).to(dev).eval()
        pnet_r = PointNet2Stage(6, 128, 32).to(dev).eval()
        n_valid = int((batch["depth_corrupt"] != 0).sum().item())
        opt = pl.LidfOptions(valid_stride=max(1, n_valid // (10000 * B)))
        for gf in (32, 64, 128):
            prob, off, offr = module("IMNET", 385, gf, 7), module("IEF", 385, gf, 8), module("IEF", 334, gf, 9)
            pairs = {}

            def frame(p):
                ok, dd = pl.lidf_forward(batch, feat, pnet, prob, off, opt, precision=p)
                assert ok
                pl.refine_forward(dd, pnet_r, offr, opt, precision=p)
                pairs["P"] = int(dd["pair_ray"].shape[0])
            steps = {p: (lambda p=p: frame(p)) for p in PRECISIONS}
            t = timed(steps)
            rows.append(row("c: lidf_forward + refine_forward, stepwise", gf, pairs["P"], t,
                            route="fixed-width kernels (shipped configuration)" if gf == 64 else "any-width chain"))

    res = {"what": "precision f16x3 against f32 at decoders of gf_dim 32 / 64 / 128: the split-f16 decoder chain",
           "device": torch.cuda.get_device_name(0), "groups": args.groups, "reps": args.reps, "warmup": args.warmup,
           "clock": "device events around `reps` back-to-back calls; median of `groups` alternating groups; spread = "
                    "(max - min) / median of the groups", "rows": rows}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
