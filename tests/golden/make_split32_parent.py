"""The split-f16 decoders on 32 x 32 tiles (precision="f16x3": the fused per-point query and the decoder on
materialised rows) as the build BEFORE the fold of their two kernel files into csrc/lidf_split32.h computed them.
tests/test_split32_parent_gpu.py compares bit patterns: the kernels have no atomics on their outputs, the fold keeps
the order of every accumulation and the stream format, so outputs and packed streams are the same bits.

Run once on an MI355X with that parent build:  python tests/golden/make_split32_parent.py
It writes tests/golden/split32_parent.npz — outputs of this project's own kernels only. The test imports this file
for the cases and their inputs; every input comes from numpy's PCG64 at SEED, weights ~ N(0, 1 / fan-in) with
non-zero biases (make_chain16_parent.decoder_params). Every case is run twice here and nothing is written if the two
runs differ. A row's result depends on the row alone in the rows kernel and on its 32-point wave-tile in the fused one,
never on the workgroup that ran it, so no case depends on the compute-unit count.

Rows kernel (decoders.decoders_forward), cases (n, D, nets, offset decoder, strided):
  rows n: 1 (one live lane, the rest clamped), 33 (second wavefront of a tile), 129 (second tile), 32,901 = 128 x 257
    + 5 (with one workgroup per compute unit a workgroup walks a second tile through the running feed; SHA-256 plus the
    first and last 64 values);
  width D: 385 (25 k-steps, no multiple of the burst of 4), 334 (stage 2), 15 (the bias column is the last of the only
    k-step), 16 (the bias column opens a second k-step), 30 (the scalar tail branch of load_x);
  nets: prob only, offset only, both; offset net: an IEF with n_iter 2, an IMNet with sigmoid;
  input stride: ld_inp == D, ld_inp > D (columns 7.. of rows 404 floats apart: unaligned vector loads).
Kept of that product, 28 cases:
  A  every D x n in (1, 33, 129), both nets, IEF, contiguous (15): the width paths at every row edge;
  B  n = 32,901 at D 385 (both, IEF), D 334 (offset only, IEF: the stage-2 launch), D 30 (both, IMNet, strided) (3):
     the second tile of a workgroup needs many rows, not many forms;
  C  n = 129, D 385: prob only / offset only IEF / offset only IMNet / both with the IMNet (4): the sequencer's net
     and pass counts (1 or 2 nets, 1 or 2 passes per net) — they do not interact with the width;
  D  n = 33, strided, every D (5), and n = 129, D 334, offset only, strided (1): the stride only changes load_x.
Fused kernel (query.lidf_query), cases (pair list, pos_rel, multires, offset decoder, offsets):
  pair lists: one ray with one pair; one ray with 33 pairs; 40 rays of one pair each (a wave-tile of 32 rays: every
    extra rank-1 round); rays of 3 to 5 pairs (tiles straddling more than two rays, todo != 0); 647 = 128 x 5 + 7
    pairs on 64-pair rays (a whole grab, a partial grab, the prefetch past the end).
Kept, 24 cases: every list at (pos_rel False, multires 8, IEF) x offsets all / selected (10: FORM_ALL, and FORM_PART
  with FORM_LIST); the two many-tile lists with pos_rel True / multires 5 / an IMNet, one at a time, x all / selected
  (12: none of the three touches the ray rounds or the grabs, so they ride on two lists); the 40-ray list with an IMNet
  selected and with multires 5 (2).
Stage 2 (query.lidf_refine): 33 rays, two iterations, an IEF: pred_pos and end_voxel_id.
Stream bytes, for an IEF and an IMNet offset decoder at multires 5 and 8: SHA-256 of lidf_query_pack_f32's blob at
  f16x3 and of the workspace of a lidf_decoders_split_f32 call (the stream and aux at its head), both zeroed first."""
import ctypes as C
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from make_chain16_parent import decoder_params, digest  # noqa: E402

SEED = 20261022
N_LARGE = 128 * 257 + 5
LDX, COL0 = 404, 7
DS = (385, 334, 15, 16, 30)
FIXTURE = os.path.join(HERE, "split32_parent.npz")
QUERY_KEYS = ("pred_offset", "pred_prob_end", "pair_pred_pos", "pred_prob_end_softmax", "max_pair_id", "pred_pos")


def _rng(*key):
    return np.random.Generator(np.random.PCG64([SEED] + [int(k) for k in key]))


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


# ---- rows kernel
def rows_cases():
    """(n, D, nets, off_kind, strided); nets: "prob" | "off" | "both"."""
    a = [(n, d, "both", "IEF", False) for d in DS for n in (1, 33, 129)]
    b = [(N_LARGE, 385, "both", "IEF", False), (N_LARGE, 334, "off", "IEF", False),
         (N_LARGE, 30, "both", "IMNET", True)]
    c = [(129, 385, "prob", "IEF", False), (129, 385, "off", "IEF", False), (129, 385, "off", "IMNET", False),
         (129, 385, "both", "IMNET", False)]
    d = [(33, dd, "both", "IEF", True) for dd in DS] + [(129, 334, "off", "IEF", True)]
    return a + b + c + d


def rows_inputs(dev):
    """The pool every case's rows are cut from, and per width a prob IMNet, an IEF (n_iter 2) and an IMNet with
    sigmoid as offset decoders."""
    from util import make_module
    rng = _rng(1)
    inp = {"x": _t(rng.standard_normal((N_LARGE, LDX), dtype=np.float32)).to(dev)}
    for d in DS:
        inp[d, "prob"] = make_module("IMNET", decoder_params(rng, "IMNET", d, 64), d, dev)
        inp[d, "IEF"] = make_module("IEF", decoder_params(rng, "IEF", d, 64), d, dev, n_iter=2)
        inp[d, "IMNET"] = make_module("IMNET", decoder_params(rng, "IMNET", d, 64), d, dev, use_sigmoid=True)
    return inp


def run_rows_case(inp, case):
    """[k, n] on the host: the outputs of the case's nets, prob first."""
    from implicit_depth_amd.decoders import decoders_forward
    n, d, nets, off_kind, strided = case
    x = inp["x"][:n, COL0:COL0 + d] if strided else inp["x"][:n, :d].contiguous()
    if strided and n > 1:
        assert x.stride(0) == LDX
    with torch.no_grad():
        outs = decoders_forward(x, inp[d, "prob"] if nets != "off" else None,
                                inp[d, off_kind] if nets != "prob" else None, precision="f16x3")
    return np.stack([o.reshape(-1).cpu().numpy() for o in outs if o is not None])


# ---- fused kernel
IMG_H, IMG_W = 8, 16
PAIR_LISTS = ("one", "ray33", "rays40", "rays3to5", "p647")


def pair_counts(name):
    if name == "one":
        return np.array([1])
    if name == "ray33":
        return np.array([33])
    if name == "rays40":
        return np.ones(40, dtype=np.int64)
    if name == "rays3to5":
        return _rng(2).integers(3, 6, 60)
    return np.array([64] * 10 + [7])


def query_cases():
    """(pair list, pos_rel, multires, off_kind, offsets)."""
    out = [(pl, False, 8, "IEF", o) for pl in PAIR_LISTS for o in ("all", "selected")]
    for pl in ("rays3to5", "p647"):
        for var in ((True, 8, "IEF"), (False, 5, "IEF"), (False, 8, "IMNET")):
            out += [(pl,) + var + (o,) for o in ("all", "selected")]
    return out + [("rays40", False, 8, "IMNET", "selected"), ("rays40", False, 5, "IEF", "all")]


def query_scene(name, dev):
    """The first R pixels of an 8 x 16 image as rays, pair_counts(name) segments per ray inside the 9 x 9 x 9 grid of
    implicit_depth_amd.synthetic (its geometry; features from PCG64)."""
    from implicit_depth_amd import synthetic as syn
    cnt = pair_counts(name)
    R = len(cnt)
    rng = _rng(3, PAIR_LISTS.index(name))
    ray_dir, ray_pix, _ = syn.pixel_rays(1, IMG_H, IMG_W)
    ray_dir, ray_pix = ray_dir[:R].contiguous(), ray_pix[:R].contiguous()
    pair_ray = np.repeat(np.arange(R), cnt)
    k = np.concatenate([np.arange(c) for c in cnt]).astype(np.float32)
    delta = (np.float32(1.75) / cnt.astype(np.float32))[pair_ray]
    t_enter = np.float32(0.25) + k * delta
    pair_t = _t(np.stack((t_enter, t_enter + delta), -1).astype(np.float32))
    mid = ray_dir[_t(pair_ray)] * pair_t.mean(1, keepdim=True)
    cell = torch.floor((mid - torch.tensor(syn.GRID_XMIN)) / syn.PART_SIZE).long().clamp(0, syn.GRID_RES - 1)
    vox = (cell[:, 0] * syn.GRID_RES + cell[:, 1]) * syn.GRID_RES + cell[:, 2]
    ci = torch.arange(syn.GRID_RES, dtype=torch.float32)
    cxyz = torch.stack(torch.meshgrid(ci, ci, ci, indexing="ij"), -1).reshape(-1, 3)
    s = {
        "ray_dir": ray_dir, "ray_pix": ray_pix, "ray_bid": torch.zeros(R, dtype=torch.int32),
        "ray_flat": torch.arange(R, dtype=torch.int32),
        "pair_off": _t(np.concatenate(([0], np.cumsum(cnt))).astype(np.int32)),
        "pair_ray": _t(pair_ray.astype(np.int32)), "pair_vox": vox.int(), "pair_t": pair_t,
        "feat_grid": _t(rng.standard_normal((1, 32, IMG_H, IMG_W), dtype=np.float32)),
        "vox_feat": _t(np.maximum(rng.standard_normal((syn.GRID_RES ** 3, 128), dtype=np.float32), 0)),
        "vox_center": (torch.tensor(syn.GRID_XMIN) + (cxyz + 0.5) * syn.PART_SIZE).contiguous(),
    }
    return {key: v.to(dev) for key, v in s.items()}


def query_D(multires):
    return 256 + 2 * (3 + 6 * multires) + 27


def query_inputs(dev):
    """The five scenes and per multires a prob IMNet, an IEF (n_iter 2) and an IMNet as offset decoders."""
    from util import make_module
    rng = _rng(4)
    inp = {pl: query_scene(pl, dev) for pl in PAIR_LISTS}
    for L in (8, 5):
        d = query_D(L)
        inp[L, "prob"] = make_module("IMNET", decoder_params(rng, "IMNET", d, 64), d, dev)
        inp[L, "IEF"] = make_module("IEF", decoder_params(rng, "IEF", d, 64), d, dev, n_iter=2)
        inp[L, "IMNET"] = make_module("IMNET", decoder_params(rng, "IMNET", d, 64), d, dev)
    return inp


def run_query_case(inp, case):
    """The QUERY_KEYS outputs on the host (offsets="selected": the unwritten rows are NaN)."""
    from implicit_depth_amd.query import lidf_query
    pl, pos_rel, multires, off_kind, offsets = case
    s = inp[pl]
    with torch.no_grad():
        got = lidf_query(s["ray_dir"], s["ray_pix"], s["ray_bid"], s["pair_off"], s["pair_ray"], s["pair_vox"],
                         s["pair_t"], s["feat_grid"], s["vox_feat"], inp[multires, "prob"], inp[multires, off_kind],
                         ray_flat=s["ray_flat"], multires=multires, vox_center=s["vox_center"], pos_rel=pos_rel,
                         precision="f16x3", offsets=offsets)
    return [got[key].cpu().numpy() for key in QUERY_KEYS]


# ---- stage 2
def run_refine_case(dev):
    """pred_pos [33, 3] and end_voxel_id [33] of two refine iterations at f16x3, on the host."""
    from implicit_depth_amd.query import lidf_refine
    from implicit_depth_amd.synthetic import synthetic_scene
    from util import closed_form_pointnet, make_module, make_pointnet
    rng = _rng(5)
    h, w = 3, 11
    scene = synthetic_scene(1, h, w, 6, seed=31)   # every ray crosses 6 voxels
    R, V = scene["R"], scene["V"]
    t = _t(rng.uniform(0.3, 1.9, (R, 1)).astype(np.float32))
    pred_pos = scene["ray_dir"] * t
    max_pair_id = scene["pair_off"][:-1].long() + _t(rng.integers(0, 6, R))
    vb = torch.cat((scene["vox_center"] - 0.125, scene["vox_center"] + 0.125), 1)
    vbid = torch.zeros(V, dtype=torch.int32)
    rgb = _t(rng.standard_normal((1, 3, h, w), dtype=np.float32))
    valid_inp = _t(rng.standard_normal((300, 6), dtype=np.float32) * np.float32(0.2))
    valid_vox = _t(rng.integers(0, V, 300).astype(np.int32))
    off = make_module("IEF", decoder_params(rng, "IEF", 334, 64), 334, dev, n_iter=2)
    pnet = make_pointnet(closed_form_pointnet(41), dev)
    with torch.no_grad():
        pos, ev = lidf_refine(scene["ray_dir"].to(dev), scene["ray_pix"].to(dev), scene["ray_bid"].to(dev),
                              scene["ray_flat"].to(dev), pred_pos.to(dev), max_pair_id.to(dev),
                              scene["pair_vox"].to(dev), vb.to(dev), vbid.to(dev), rgb.to(dev),
                              scene["feat_grid"].to(dev), valid_inp.to(dev), valid_vox.to(dev), pnet, off,
                              forward_times=2, precision="f16x3")
    return pos.cpu().numpy(), ev.cpu().numpy()


# ---- stream bytes
def stream_cases():
    return [(L, kind) for L in (5, 8) for kind in ("IEF", "IMNET")]


def run_stream_case(inp, case):
    """(SHA-256 of the fused query's packed blob at f16x3, SHA-256 of the decoders' workspace after a one-row split
    call: the rows stream and aux at its head). Both buffers are zeroed first, so what the packers leave alone counts
    too. inp: query_inputs."""
    from implicit_depth_amd import _lib
    from implicit_depth_amd.decoders import _decoder_struct
    from implicit_depth_amd.query import PRECISIONS
    L, kind = case
    prob, off = inp[L, "prob"], inp[L, kind]
    dev = next(prob.parameters()).device
    lib, keep = _lib.lib(), []
    dp, do = _decoder_struct(prob, keep), _decoder_struct(off, keep)
    d = query_D(L)
    blob = torch.zeros(lib.lidf_query_pack_bytes(), dtype=torch.uint8, device=dev)
    wsb = lib.lidf_decoders_workspace_bytes(1, d)
    ws = torch.zeros(wsb, dtype=torch.uint8, device=dev)
    x = torch.zeros((1, d), dtype=torch.float32, device=dev)
    out = torch.empty((2, 1), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.lidf_query_pack_f32(C.byref(dp), C.byref(do), L, 4, PRECISIONS["f16x3"], _lib.ptr(blob),
                                           blob.numel(), _lib.current_stream(dev)))
        _lib.check(lib.lidf_decoders_split_f32(_lib.ptr(x), 1, d, d, C.byref(dp), C.byref(do), _lib.ptr(out[0]),
                                               _lib.ptr(out[1]), _lib.ptr(ws), wsb, _lib.current_stream(dev)))
    return digest(blob.cpu().numpy()), digest(ws.cpu().numpy())


def _twice(fn, *args):
    """fn's arrays, after a second run gave the same bytes."""
    a, b = fn(*args), fn(*args)
    for u, v in zip(a, b):
        if u.dtype != v.dtype or u.shape != v.shape or u.tobytes() != v.tobytes():
            raise SystemExit("two runs differ, nothing written: %r" % (args[-1:],))
    return a


def main():
    dev = torch.device("cuda:0")
    data = {}
    inp = rows_inputs(dev)
    for i, case in enumerate(rows_cases()):
        out = _twice(run_rows_case, inp, case)
        out = np.stack(out)
        assert np.isfinite(out).all(), case
        if case[0] == N_LARGE:
            data["rows_sha_%d" % i] = digest(out)
            data["rows_head_%d" % i], data["rows_tail_%d" % i] = out[:, :64], out[:, -64:]
        else:
            data["rows_%d" % i] = out
    del inp
    inp = query_inputs(dev)
    for i, case in enumerate(query_cases()):
        for key, v in zip(QUERY_KEYS, _twice(run_query_case, inp, case)):
            if case[-1] == "all" or key not in ("pred_offset", "pair_pred_pos"):
                assert np.isfinite(v).all(), (case, key)
            data["query_%d_%s" % (i, key)] = v
    for i, case in enumerate(stream_cases()):
        data["stream_fused_%d" % i], data["stream_rows_%d" % i] = _twice(run_stream_case, inp, case)
    data["refine_pos"], data["refine_ev"] = _twice(run_refine_case, dev)
    assert np.isfinite(data["refine_pos"]).all()
    np.savez_compressed(FIXTURE, **data)
    print("wrote %s: %d rows cases, %d query cases, %d stream cases, 1 refine case, %d bytes"
          % (FIXTURE, len(rows_cases()), len(query_cases()), len(stream_cases()), os.path.getsize(FIXTURE)))


if __name__ == "__main__":
    main()
