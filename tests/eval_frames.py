"""Tests only: batches for the per-frame evaluation losses (per_frame=True) built FROM bs == 1 restatement dicts
(eval_loss_ref.random_case / g12_case), so that the yardstick of row b is frame b's own dict through code that exists
without the feature — the bs == 1 call, the float64 restatement, the reference's fixture — and never something the
code under test produced.

  concat_frames([d0, d1, ...])   one batch dict in the restatement's format: miss_bid = b, pair_ray offset by the rays
                                 before it
  without_rays(d)                the same frame with empty ray and pair lists (the reference's early exit)
  cut_frames(d)                  the frames of a bs > 1 restatement dict as bs == 1 dicts (as test_eval_loss_gpu.sized
                                 cuts frame 0)
  batch_a / batch_b              the two batches of the tests, with their loss options
"""
import torch

import eval_loss_ref as el

_FRAME = ("xyz_flat", "xyz_corrupt_flat")
_RAY = ("miss_flat", "gt_pos", "pred_pos", "pred_pos_refine")
_PAIR = ("pred_prob_end", "pcl_label")


def concat_frames(ds):
    h, w = ds[0]["h"], ds[0]["w"]
    assert all(d["bs"] == 1 and d["h"] == h and d["w"] == w for d in ds)
    out = {"bs": len(ds), "h": h, "w": w}
    for k in _FRAME:
        out[k] = torch.cat([d[k] for d in ds]).contiguous()
    out["corrupt_mask"] = torch.cat([d["corrupt_mask"].reshape(1, h, w).float() for d in ds]).contiguous()
    out["miss_bid"] = torch.cat([torch.full_like(d["miss_bid"], b) for b, d in enumerate(ds)])
    for k in _RAY + _PAIR:
        out[k] = torch.cat([d[k] for d in ds]).contiguous()
    first, rays = 0, []
    for d in ds:
        rays.append(d["pair_ray"] + first)
        first += d["miss_bid"].shape[0]
    out["pair_ray"] = torch.cat(rays)
    return out


def without_rays(d):
    c = dict(d)
    for k in ("miss_bid", "miss_flat") + _RAY[1:] + _PAIR + ("pair_ray",):
        c[k] = d[k][:0].clone()
    if "pair_off" in d:
        c["pair_off"] = d["pair_off"][:1].clone()
    return c


def cut_frames(d):
    """The frames of a batch in (frame, pixel) ray order as bs == 1 dicts."""
    out, first = [], 0
    for b in range(d["bs"]):
        n = int((d["miss_bid"] == b).sum())
        pk = (d["pair_ray"] >= first) & (d["pair_ray"] < first + n)
        c = {"bs": 1, "h": d["h"], "w": d["w"], "pair_ray": d["pair_ray"][pk] - first,
             "miss_bid": torch.zeros(n, dtype=d["miss_bid"].dtype)}
        for k in _FRAME + ("corrupt_mask",):
            c[k] = d[k][b:b + 1].contiguous()
        for k in _RAY:
            c[k] = d[k][first:first + n].contiguous()
        for k in _PAIR:
            c[k] = d[k][pk].contiguous()
        out.append(c)
        first += n
    return out


def g12_opt(g, name):
    pos_w, prob_w, surf_w, smooth_w, _ = (float(v) for v in g[name + "_loss_opt"])
    return dict(pos_w=pos_w, prob_w=prob_w, surf_norm_w=surf_w, smooth_w=smooth_w, **el.G12_CASES[name][1])


def batch_a():
    """5 x 16 x 24: one block (232 rays) | the reference's own 'test' run, every pixel a ray (384 = h * w, the bound the
    launch is sized from: 256 + 128) | no ray | all ground truth the zero point (244 rays, no valid pixel) | no
    labelled pair (227 rays). Returns (frames, loss options of g12 'd', the fixture's two vectors of frame 1)."""
    g = el.g12_file()
    d1, ref = el.g12_case(g, "d")
    d4 = el.random_case(1, 16, 24, 0.6, seed=22)
    d4["pcl_label"] = torch.zeros_like(d4["pcl_label"])
    frames = [el.random_case(1, 16, 24, 0.6, seed=23), d1, without_rays(el.random_case(1, 16, 24, 0.6, seed=24)),
              el.random_case(1, 16, 24, 0.6, seed=21, zero_gt=True), d4]
    assert [f["miss_bid"].shape[0] for f in frames] == [232, 384, 0, 244, 227]
    return frames, g12_opt(g, "d"), ref


def batch_b():
    """3 x 20 x 27 with 305 / 330 / 338 rays: two blocks per frame with a ragged second one, and frame boundaries at
    rays 305 and 635 — inside a global block of 256."""
    frames = cut_frames(el.random_case(3, 20, 27, 0.6, seed=5))
    assert [f["miss_bid"].shape[0] for f in frames] == [305, 330, 338]
    return frames, dict(smooth_w=0.5)
