"""The chained 16-row decoders' outputs as the build BEFORE the fold of their three kernel files computed them
(tests/test_chain16_parent_gpu.py compares with torch.equal: the kernels have no atomics and the fold keeps the order
of every accumulation, so the outputs are the same bits).

Run once on an MI355X (256 compute units) with that parent build:  python tests/golden/make_chain16_parent.py
It writes tests/golden/chain16_parent.npz — outputs of this project's own kernels only. The test imports this file
for the cases and their inputs; every input comes from numpy's PCG64 at SEED (the stage-2 scenes' geometry from
implicit_depth_amd.synthetic, which is seeded too).

Any-width entries (lidf_decoder_chain_f32 / lidf_decoder_chain_split_f32 through generic.decoder_chain), the full
product of
  gf 32 / 64 / 128;  an IMNet with sigmoid / an IEF with n_iter 3;  both precisions;
  rows 1 (one sub-tile), 17 (a masked partial sub-tile), 33 (a pair and an odd one), 81,961 = 16 (1024 x 5 + 3) - 7
    (on 256 compute units 5 or 6 sub-tiles per SIMD: every wavefront walks pairs and an odd sub-tile, uneven slots);
  k 51 (column masking), 128 (an eighth k-group: the late request of the f32 kernel, the partner group of the split
    one), 130 (an odd number of groups in the split form);
  tables: voxpart[vox_idx] + raypart rows | raypart[ray_idx] | raypart rows | none.
Stage 2 (query.lidf_refine): 1 / 17 / 33 / 2,000 rays; multires 10 (four k-groups, all prefetched) and 16 (seven, three
requested late); an IEF with two iterations and an IMNet.
Small outputs are stored whole; the 81,961-row ones as SHA-256 of their bytes plus the first and last 64 values."""
import hashlib
import itertools
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

SEED = 20261021
CUS = 256                      # the slot split of the large case is a function of the compute-unit count
N_LARGE = 81961
NS = (1, 17, 33, N_LARGE)
KS = (51, 128, 130)
GFS = (32, 64, 128)
KINDS = ("IMNET", "IEF")
PRECISIONS = ("f32", "f16x3")
TABLES = ("both", "ray_idx", "ray_rows", "none")
INP_DIM, W1_COL0, LDX = 136, 3, 144   # k operand columns multiply W1[:, 3 : 3 + k]; rows of X are 144 floats apart
N_VOX, N_RAYROWS = 37, 53
FIXTURE = os.path.join(HERE, "chain16_parent.npz")


def chain_cases():
    """(gf, kind, precision, k, table, n) in the order of the fixture's rows."""
    return list(itertools.product(GFS, KINDS, PRECISIONS, KS, TABLES, NS))


def decoder_params(rng, kind, inp_dim, gf):
    """A state dict with activations of order 1 in every layer (weights ~ N(0, 1 / fan-in)), non-zero biases."""
    def normal(shape, std):
        return torch.from_numpy((rng.standard_normal(shape, dtype=np.float32) * np.float32(std)))
    p = {}
    if kind == "IEF":
        p["offset_enc.weight"] = normal((16, 1), 0.5)
        p["offset_enc.bias"] = normal((16,), 0.1)
    d1 = inp_dim + (16 if kind == "IEF" else 0)
    for i, (din, dout) in enumerate(((d1, 4 * gf), (4 * gf, 2 * gf), (2 * gf, gf), (gf, 1)), 1):
        p["linear_%d.weight" % i] = normal((dout, din), din ** -0.5)
        p["linear_%d.bias" % i] = normal((dout,), 0.05)
    return p


def chain_inputs(dev):
    """The shared inputs of every any-width case, made once: X [N_LARGE, LDX] (columns at or beyond k are NOT zero:
    the kernels mask them), a pool the tables are cut from, the index arrays, one module per (gf, kind)."""
    from util import make_module
    rng = np.random.Generator(np.random.PCG64(SEED))
    inp = {
        "x": torch.from_numpy(rng.standard_normal((N_LARGE, LDX), dtype=np.float32)).to(dev),
        "pool": torch.from_numpy(rng.standard_normal(N_LARGE * 512, dtype=np.float32) * np.float32(0.5)).to(dev),
        "vox_idx": torch.from_numpy(rng.integers(0, N_VOX, N_LARGE).astype(np.int32)).to(dev),
        "ray_idx": torch.from_numpy(rng.integers(0, N_RAYROWS, N_LARGE).astype(np.int32)).to(dev),
    }
    for gf in GFS:
        for kind in KINDS:
            p = decoder_params(rng, kind, INP_DIM, gf)
            inp[gf, kind] = make_module(kind, p, INP_DIM, dev, n_iter=3, use_sigmoid=kind == "IMNET", gf=gf)
    return inp


def run_chain_case(inp, case):
    """One launch (padded=True: X is readable up to column 16 ceil(k / 16) <= LDX of every row). Returns [n] on the
    host."""
    from implicit_depth_amd import generic
    gf, kind, precision, k, table, n = case
    pool = inp["pool"]
    row = 4 * gf
    kw = {}
    if table == "both":   # the stage-2 form: a gathered per-voxel row plus the row's own
        kw = dict(voxpart=pool[-N_VOX * row:].view(N_VOX, row), vox_idx=inp["vox_idx"][:n],
                  raypart=pool[:n * row].view(n, row))
    elif table == "ray_idx":
        kw = dict(raypart=pool[:N_RAYROWS * row].view(N_RAYROWS, row), ray_idx=inp["ray_idx"][:n])
    elif table == "ray_rows":
        kw = dict(raypart=pool[:n * row].view(n, row))
    with torch.no_grad():
        out = generic.decoder_chain(inp[gf, kind], inp["x"][:n], k, w1_col0=W1_COL0, padded=True,
                                    precision=precision, **kw)
    return out.reshape(-1).cpu().numpy()


def digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


# ---- stage 2
REFINE_SCENES = ((1, 1), (1, 17), (3, 11), (40, 50))   # h x w of one frame: 1, 17, 33 and 2,000 rays
REFINE_MULTIRES = (10, 16)
REFINE_KINDS = ("IEF", "IMNET")


def refine_cases():
    return list(itertools.product(REFINE_SCENES, REFINE_MULTIRES, REFINE_KINDS))


def run_refine_case(dev, case):
    """pred_pos [R, 3] and end_voxel_id [R] of two refine iterations, on the host."""
    from implicit_depth_amd.query import lidf_refine
    from implicit_depth_amd.synthetic import synthetic_scene
    from util import closed_form_pointnet, make_module, make_pointnet
    (h, w), multires, kind = case
    rng = np.random.Generator(np.random.PCG64([SEED, h, w, multires, len(kind)]))
    scene = synthetic_scene(1, h, w, 6, seed=31)   # every ray crosses 6 voxels
    R, V = scene["R"], scene["V"]
    t = torch.from_numpy(rng.uniform(0.3, 1.9, (R, 1)).astype(np.float32))
    pred_pos = scene["ray_dir"] * t
    max_pair_id = scene["pair_off"][:-1].long() + torch.from_numpy(rng.integers(0, 6, R))
    vb = torch.cat((scene["vox_center"] - 0.125, scene["vox_center"] + 0.125), 1)
    vbid = torch.zeros(V, dtype=torch.int32)
    rgb = torch.from_numpy(rng.standard_normal((1, 3, h, w), dtype=np.float32))
    valid_inp = torch.from_numpy(rng.standard_normal((300, 6), dtype=np.float32) * np.float32(0.2))
    valid_vox = torch.from_numpy(rng.integers(0, V, 300).astype(np.int32))
    D = 256 + 3 + 6 * multires + 27
    off = make_module(kind, decoder_params(rng, kind, D, 64), D, dev, n_iter=2)
    pnet = make_pointnet(closed_form_pointnet(41), dev)
    with torch.no_grad():
        pos, ev = lidf_refine(scene["ray_dir"].to(dev), scene["ray_pix"].to(dev), scene["ray_bid"].to(dev),
                              scene["ray_flat"].to(dev), pred_pos.to(dev), max_pair_id.to(dev),
                              scene["pair_vox"].to(dev), vb.to(dev), vbid.to(dev), rgb.to(dev),
                              scene["feat_grid"].to(dev), valid_inp.to(dev), valid_vox.to(dev), pnet, off,
                              forward_times=2, multires=multires)
    return pos.cpu().numpy(), ev.cpu().numpy()


def main():
    dev = torch.device("cuda:0")
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    assert cus == CUS, "the fixture is defined on %d compute units, this device has %d" % (CUS, cus)
    inp = chain_inputs(dev)
    small = {n: [] for n in NS if n != N_LARGE}
    sha, head, tail = [], [], []
    for case in chain_cases():
        out = run_chain_case(inp, case)
        assert np.isfinite(out).all(), case
        if case[-1] == N_LARGE:
            sha.append(digest(out)); head.append(out[:64]); tail.append(out[-64:])
        else:
            small[case[-1]].append(out)
    data = {"chain_%d" % n: np.stack(v) for n, v in small.items()}
    data.update(chain_sha=np.stack(sha), chain_head=np.stack(head), chain_tail=np.stack(tail))
    for i, case in enumerate(refine_cases()):
        pos, ev = run_refine_case(dev, case)
        assert np.isfinite(pos).all(), case
        data["refine_pos_%d" % i], data["refine_ev_%d" % i] = pos, ev
    np.savez_compressed(FIXTURE, **data)
    print("wrote %s: %d chain cases, %d refine cases, %d bytes" % (FIXTURE, len(chain_cases()), len(refine_cases()),
                                                                  os.path.getsize(FIXTURE)))


if __name__ == "__main__":
    main()
