"""selected_split_time.py — precision "f16x3" together with offsets "selected" against each option alone, on one MI355X.

    python scripts/selected_split_time.py [--only query,frame] [--out profiles/selected_split_time.json]
    python scripts/selected_split_time.py --leg f16x3/all --shape headline      # one leg, one JSON line (library A/Bs)
    python scripts/selected_split_time.py --leg f16x3/selected --shape list     # the one-pair-per-ray list, R = 76,800
    python scripts/selected_split_time.py --merge-ab lines.jsonl --out ...      # fold A/B lines into the profile

One process, one session per invocation. Device events around `reps` back-to-back calls make one group; the legs'
groups alternate; `reps` is sized per leg from two warm calls so that a leg's groups cover at least `--window`
seconds in total. The figure is the median of the groups' means, the spread (max - min) / median of the groups.
Every leg is run twice ("x/y" and "x/y again", not adjacent in the rotation): the difference between the two
medians of identical legs is the session's repeat spread.

  query  lidf_query, four legs {f32, f16x3} x {all, selected}: the headline shape 240 x 320 rays x 64 candidates
         (bench.py's scene) and the ragged pair list of the `bench.py --workload e2e` frame (about 3.6 pairs per ray);
         Mpoints/s = P / call time
  frame  pipeline.FrameRunner on that 1 x 240 x 320 frame, the same four legs, eager and replayed from a graph: ms
         per frame
  --leg  one leg alone: for A/Bs of two builds of the library in one session (LIDF_HIP_LIB selects the build;
         scripts/selected_split_ab.sh is the driver that alternates the processes, wraps them in rocprofv3
         --kernel-trace and writes the lines --merge-ab folds in; its header says how the two other builds are
         made). --shape list is the scene with ONE candidate per ray: P = R = 76,800, so the
         selected list is every pair — the launch the list form of lidf_points_h_kernel exists for. Under
         `rocprofv3 --kernel-trace` this invocation gives that launch's own duration (--trace-db reads it back)."""
import argparse
import json
import os
import sqlite3
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = ("f32/all", "f32/selected", "f16x3/all", "f16x3/selected")


def timed(steps, groups, window):
    """steps: {leg: callable}. {leg: {"ms", "spread", "reps", "groups"}} + the repeat spread of identical legs."""
    order = list(steps) + [k + " again" for k in steps]
    fn = {k: steps[k.replace(" again", "")] for k in order}
    reps, ms = {}, {k: [] for k in order}
    with torch.no_grad():
        for k in steps:
            fn[k]()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn[k]()
            fn[k]()
            b.record()
            b.synchronize()
            one = a.elapsed_time(b) / 2
            reps[k] = reps[k + " again"] = max(2, int(window * 1e3 / groups / max(one, 1e-3)) + 1)
        for _ in range(groups):
            for k in order:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(reps[k]):
                    fn[k]()
                b.record()
                b.synchronize()
                ms[k].append(a.elapsed_time(b) / reps[k])
    out = {}
    for k in steps:
        m, m2 = statistics.median(ms[k]), statistics.median(ms[k + " again"])
        out[k] = {"ms": round(m, 5), "ms_again": round(m2, 5), "repeat_spread": round(abs(m - m2) / m, 4),
                  "spread": round((max(ms[k]) - min(ms[k])) / m, 4), "reps": reps[k], "groups": groups}
    return out


def models(dev):
    from implicit_depth_amd import IEF, IMNet, PointNet2Stage
    from implicit_depth_amd.synthetic import init_decoder_params
    torch.manual_seed(3)
    pnet, pnet_r = PointNet2Stage(6, 128, 32).to(dev).eval(), PointNet2Stage(6, 128, 32).to(dev).eval()
    prob = IMNet(385, 1, 64).to(dev).eval()
    prob.load_state_dict(init_decoder_params("IMNET", 385, 7, 5.0))
    off = IEF(dev, 385, 1, 64, n_iter=2).to(dev).eval()
    off.load_state_dict(init_decoder_params("IEF", 385, 8, 5.0))
    offr = IEF(dev, 334, 1, 64, n_iter=2).to(dev).eval()
    offr.load_state_dict(init_decoder_params("IEF", 334, 9, 5.0))
    return pnet, prob, off, pnet_r, offr


def bench_frame(dev):
    """The batch, feature map and options of `bench.py --workload e2e` (one 240 x 320 frame)."""
    from implicit_depth_amd import pipeline as pl
    from implicit_depth_amd.synthetic import synthetic_batch
    batch, feat = synthetic_batch(1, 240, 320, seed=77)
    batch = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in batch.items()}
    n_valid = int((batch["depth_corrupt"] != 0).sum().item())
    return batch, feat.to(dev), pl.LidfOptions(valid_stride=max(1, n_valid // 10000))


def query_shapes(dev, which):
    """{name: (positional arguments of lidf_query in front of the decoders, R, P)}"""
    from implicit_depth_amd import pipeline as pl
    from implicit_depth_amd.synthetic import synthetic_scene
    out = {}
    for name, n in (("headline", 64), ("list", 1)):
        if name in which:
            sc = synthetic_scene(1, 240, 320, n, seed=1235)
            s = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in sc.items()}
            out[name] = ((s["ray_dir"], s["ray_pix"].int(), s["ray_bid"].int(), s["pair_off"], s["pair_ray"],
                          s["pair_vox"], s["pair_t"], s["feat_grid"], s["vox_feat"]), sc["R"], sc["P"])
    if "bench frame" in which:
        batch, feat, opt = bench_frame(dev)
        m = models(dev)
        with torch.no_grad():
            ok, dd = pl.lidf_forward(batch, feat, m[0], m[1], m[2], opt)
        assert ok
        out["bench frame"] = ((dd["miss_ray_dir"], dd["ray_pix"].int(), dd["ray_bid"].int(), dd["pair_off"], dd["pair_ray"],
                               dd["pair_vox"], dd["pair_t"], feat, dd["occ_voxel_feat"]),
                              int(dd["miss_ray_dir"].shape[0]), int(dd["pair_ray"].shape[0]))
    return out


def query_step(qargs, prob, off, leg, ws):
    from implicit_depth_amd.query import lidf_query
    precision, offsets = leg.split("/")

    def step():
        ws["w"] = lidf_query(*qargs, prob, off, precision=precision, offsets=offsets, want_softmax=True,
                             workspace=ws.get("w"))["workspace"]
    return step


def trace_db(path):
    """Per-kernel durations of lidf_points_h_kernel launches in a rocprofv3 --kernel-trace database, in launch order:
    the launches alternate prob_dec over the pairs / offset_dec over the list, whatever instantiation runs them."""
    cur = sqlite3.connect(path).cursor()
    try:
        rows = list(cur.execute("select name, duration from kernels where name like '%lidf_points_h_kernel%' order by start"))
    except sqlite3.OperationalError:
        rows = list(cur.execute("select name, duration from kernels where name like '%lidf_points_h_kernel%'"))
    res = {}
    for which, sel in (("prob launch", rows[0::2]), ("list launch", rows[1::2])):
        d = [r[1] / 1e3 for r in sel][2:]           # (the first calls carry the code object's load)
        res[which] = {"kernel": sel[0][0][:48] if sel else None, "launches": len(d),
                      "median_us": round(statistics.median(d), 2) if d else None,
                      "spread": round((max(d) - min(d)) / statistics.median(d), 4) if d else None}
    return res


def launches_per_frame(path):
    """Kernel launches between the last two launches of the frame's head kernel (one per frame) in a rocprofv3
    --kernel-trace database of `--frame-leg`."""
    cur = sqlite3.connect(path).cursor()
    names = [r[0] for r in cur.execute("select name from kernels order by start")]
    idx = [i for i, n in enumerate(names) if "frame_head" in n]
    return {"frames_seen": len(idx), "launches_per_frame": idx[-1] - idx[-2] if len(idx) >= 2 else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=5)
    ap.add_argument("--window", type=float, default=1.0, help="seconds of timed calls per leg, in total")
    ap.add_argument("--only", default="query,frame")
    ap.add_argument("--leg", default=None)
    ap.add_argument("--shape", default="headline", choices=["headline", "list", "bench frame"])
    ap.add_argument("--tag", default="tree")
    ap.add_argument("--trace-db", default=None)
    ap.add_argument("--frame-leg", default=None, help="run 4 eager one-stream frames of this leg (for a kernel trace)")
    ap.add_argument("--frames-db", default=None, help="count the launches per frame in the trace of --frame-leg")
    ap.add_argument("--merge-ab", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    if args.trace_db:
        print(json.dumps({"tag": args.tag, "trace": trace_db(args.trace_db)}))
        return
    if args.frames_db:
        print(json.dumps({"tag": args.tag, "frame_launches": launches_per_frame(args.frames_db)}))
        return
    if args.merge_ab:
        path = args.out or os.path.join(ROOT, "profiles", "selected_split_time.json")
        res = json.load(open(path)) if os.path.exists(path) else {}
        res["library_ab"] = [json.loads(l) for l in open(args.merge_ab) if l.strip().startswith("{")]
        with open(path, "w") as f:
            f.write(json.dumps(res) + "\n")
        return
    if not torch.cuda.is_available():
        raise SystemExit("selected_split_time.py needs a GPU: a CPU run gives no time")
    from implicit_depth_amd import pipeline as pl
    dev = torch.device("cuda:0")
    pnet, prob, off, pnet_r, offr = models(dev)

    if args.frame_leg:
        batch, feat, opt = bench_frame(dev)
        precision, offsets = args.frame_leg.split("/")
        r = pl.FrameRunner(1, 240, 320, dev, pnet, prob, off, opt, pnet_r, offr, precision=precision, offsets=offsets,
                           side_stream=False)
        with torch.no_grad():
            for _ in range(4):
                r.run(batch, feat)
        torch.cuda.synchronize()
        return
    if args.leg:
        (qargs, R, P), = query_shapes(dev, (args.shape,)).values()
        t = timed({args.leg: query_step(qargs, prob, off, args.leg, {})}, args.groups, args.window)[args.leg]
        print(json.dumps({"tag": args.tag, "lib": "the build LIDF_HIP_LIB names (see tag)" if os.environ.get("LIDF_HIP_LIB") else "this tree", "leg": args.leg,
                          "shape": args.shape, "R": R, "P": P, **t, "mpoints_per_s": round(P / t["ms"] / 1e3, 2)}))
        return

    only = set(args.only.split(","))
    res = {"what": "precision f16x3 with offsets selected against each option alone (shipped widths)",
           "device": torch.cuda.get_device_name(0),
           "clock": "device events around `reps` back-to-back calls; median of `groups` alternating groups; spread = (max - "
                    "min) / median of a leg's groups; repeat_spread = |median - median of the same leg run again| / median",
           "query": [], "frame": []}
    if "query" in only:
        for name, (qargs, R, P) in query_shapes(dev, ("headline", "bench frame")).items():
            t = timed({leg: query_step(qargs, prob, off, leg, {}) for leg in LEGS}, args.groups, args.window)
            for leg in LEGS:
                t[leg]["mpoints_per_s"] = round(P / t[leg]["ms"] / 1e3, 2)
            row = {"shape": name, "R": R, "P": P, "pairs_per_ray": round(P / R, 2), "legs": t,
                   "both_beats_each_alone": t["f16x3/selected"]["ms"] < min(t["f16x3/all"]["ms"], t["f32/selected"]["ms"])}
            print(json.dumps(row), flush=True)
            res["query"].append(row)
    if "frame" in only:
        batch, feat, opt = bench_frame(dev)
        for graph in (False, True):
            steps, runners = {}, {}
            for leg in LEGS:
                precision, offsets = leg.split("/")
                r = pl.FrameRunner(1, 240, 320, dev, pnet, prob, off, opt, pnet_r, offr, precision=precision,
                                   offsets=offsets)
                with torch.no_grad():
                    r.load(batch, feat)
                    if graph:
                        r.capture()
                    r.run()
                runners[leg] = r
                steps[leg] = r.run
            t = timed(steps, args.groups, args.window)
            counts = {leg: runners[leg].result()[1]["counts"] for leg in LEGS}
            row = {"mode": "replayed" if graph else "eager", "R": counts[LEGS[0]]["R"], "P": counts[LEGS[0]]["P"],
                   "legs": t,
                   "both_beats_each_alone": t["f16x3/selected"]["ms"] < min(t["f16x3/all"]["ms"], t["f32/selected"]["ms"])}
            print(json.dumps(row), flush=True)
            res["frame"].append(row)
            del runners, steps
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        old = json.load(open(args.out)) if os.path.exists(args.out) else {}
        for k in ("library_ab",):
            if k in old:
                res[k] = old[k]
        with open(args.out, "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
