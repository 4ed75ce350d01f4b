"""CPU: the valid-point sampler's semantics (include/lidf_hip.h, lidf_sample_valid_points) as tests/sampler_ref.py
states them — the structural checker is validated on the REFERENCE's own outputs (tests/golden/g11_sample_valid.npz,
utils/point_utils.py sample_valid_points) before it judges the numpy twin of the kernel; the twin's deterministic
parts equal the reference's; its draws are uniform (chi-square of per-rank inclusion counts, fixed seeds); and the C
ABI refuses malformed calls without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sampler_ref as sr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CHI_CALLS = 2000


def g11():
    return np.load(os.path.join(HERE, "golden", "g11_sample_valid.npz"))


def g11_cases(g=None):
    """[(mask uint8 [bs,h,w], n, reference idx int64 [bs*n,2])] of the golden file."""
    g = g11() if g is None else g
    out = []
    for k in range(int(g["n_cases"])):
        shape = tuple(int(v) for v in g["shape_%d" % k])
        mask = np.unpackbits(g["mask_%d" % k])[:int(np.prod(shape))].reshape(shape)
        n = int(g["n_%d" % k])
        ref = np.stack((np.repeat(np.arange(shape[0]), n), g["ref_%d" % k].astype(np.int64)), 1)
        out.append((mask, n, ref))
    return out


def test_golden_covers_the_cases():
    """dense with step > 1, step 1 with inum > n, cnt == n, sparse, both kinds in one batch, the shipped shape."""
    kinds = set()
    for mask, n, _ in g11_cases():
        per = []
        for m in mask:
            cnt = int(m.sum())
            per.append("sparse" if cnt < n else "equal" if cnt == n else "step1" if cnt // n == 1 else "dense")
        kinds.update(per)
        if len(set(per)) > 1 and "sparse" in per:
            kinds.add("mixed")
        if mask.shape == (3, 240, 320) and n == 10000:
            kinds.add("shipped")
    assert kinds >= {"sparse", "equal", "step1", "dense", "mixed", "shipped"}, kinds
    assert bool(g11()["empty_raises"])   # the reference dies (AssertionError) on an all-zero image


def test_checker_accepts_the_reference():
    for mask, n, ref in g11_cases():
        sr.check_sample(mask, n, ref)


def test_checker_rejects_wrong_samples():
    mask, n, ref = g11_cases()[0]          # dense, step 8
    bad = ref.copy()
    bad[1, 1] = bad[0, 1]                  # the same interval twice
    with pytest.raises(AssertionError):
        sr.check_sample(mask, n, bad)
    bad = ref.copy()
    bad[0, 1] = int(np.flatnonzero(mask[0].reshape(-1) == 0)[0])   # not a valid pixel
    with pytest.raises(AssertionError):
        sr.check_sample(mask, n, bad)
    mask, n, ref = g11_cases()[3]          # sparse, 4 valid pixels
    bad = ref.copy()
    bad[[0, 1]] = bad[[1, 0]]              # head out of block order
    with pytest.raises(AssertionError):
        sr.check_sample(mask, n, bad)
    bad = ref.copy()
    bad[4:, 1] = bad[0, 1]                 # more copies of one point than the pool holds
    with pytest.raises(AssertionError):
        sr.check_sample(mask, n, bad)


def test_checker_accepts_the_twin():
    for mask, n, _ in g11_cases():
        idx, cnt = sr.sample_valid_points(mask, n, seed=1234, counter=7)
        assert (cnt == mask.reshape(mask.shape[0], -1).sum(1)).all()
        sr.check_sample(mask, n, idx)
    rng = np.random.default_rng(5)
    for k in range(40):
        h, w = 8 * int(rng.integers(1, 5)), 8 * int(rng.integers(1, 5))
        mask = (rng.random((2, h, w)) < rng.uniform(0.05, 1.0)).astype(np.uint8)
        mask[:, 0, 0] = 1
        n = int(rng.integers(1, 2 * h * w))
        sr.check_sample(mask, n, sr.sample_valid_points(mask, n, seed=k, counter=3 * k)[0])


def test_twin_matches_the_deterministic_parts_of_the_reference():
    seen = set()
    for mask, n, ref in g11_cases():
        idx, _ = sr.sample_valid_points(mask, n, seed=99, counter=0)
        for b in range(mask.shape[0]):
            cnt = int(mask[b].sum())
            r, t = ref[b * n:(b + 1) * n, 1], idx[b * n:(b + 1) * n, 1]
            # block order itself: the reference's flat ids, sorted by block-order rank, are a subsequence of ours
            order = sr.block_order(mask[b])
            pos = np.full(mask[b].size, -1)
            pos[order] = np.arange(cnt)
            assert (pos[r] >= 0).all()
            if cnt < n:
                assert (t[:cnt] == r[:cnt]).all() and (t[:cnt] == order).all()
                seen.add("sparse")
            if cnt == n:
                assert (np.sort(t) == np.sort(r)).all()
                seen.add("equal")
    assert seen == {"sparse", "equal"}


def test_same_state_same_sample_and_the_counter_matters():
    mask, n, _ = g11_cases()[0]
    mask = np.stack((mask[0], mask[0]))     # two identical images
    a, _ = sr.sample_valid_points(mask, n, seed=5, counter=11)
    b, _ = sr.sample_valid_points(mask, n, seed=5, counter=11)
    c, _ = sr.sample_valid_points(mask, n, seed=5, counter=12)
    d, _ = sr.sample_valid_points(mask, n, seed=6, counter=11)
    assert (a == b).all() and (a != c).any() and (a != d).any()
    assert (a[:n, 1] != a[n:, 1]).any()     # the image index is part of the Philox counter


@pytest.mark.parametrize("name", ["dense", "sparse"])
def test_uniformity_of_the_twin(name):
    """Pearson's chi-square of the per-rank inclusion counts over 2000 calls with consecutive counters must stay
    below mean + 6 standard deviations of the chi-square distribution (dof + 6 sqrt(2 dof)): 500.1 for the dense
    set-up (cnt 344, n 40: step 8, inum 43, 344 live ranks), 100.3 for the sparse one (cnt 45, n 100; the
    statistic is over the n - cnt drawn slots, the first cnt being fixed). The reference's own sampler, recorded
    in g11 with the same statistic, must be inside the bound too. Twin: 319.6 dense, 19.8 sparse."""
    g = g11()
    mask, n = g["chi_%s_mask" % name], int(g["chi_%s_n" % name])
    cnt = int(mask.sum())
    assert (cnt, n) == {"dense": (344, 40), "sparse": (45, 100)}[name]
    stat, dof, dead = sr.chi_square(mask[0], n, lambda k: sr.sample_valid_points(mask, n, 20261018, k)[0][:, 1],
                                    CHI_CALLS)
    bound = sr.chi_bound(dof)
    print("chi-square %s: twin %.1f, reference %.1f, dof %d, bound %.1f" % (name, stat, float(g["chi_" + name]), dof,
                                                                             bound))
    assert dof == int(g["chi_%s_dof" % name]) == {"dense": 343, "sparse": 44}[name]
    assert abs(bound - {"dense": 500.1, "sparse": 100.3}[name]) < 0.05
    assert float(g["chi_" + name]) <= bound and int(g["chi_%s_dead" % name]) == 0
    assert dead == 0          # ranks >= inum*step are never drawn
    assert stat <= bound


def test_dead_ranks_are_never_drawn():
    """cnt 350, n 40: step 8, inum 43 — ranks 344 .. 349 stay out, in every call."""
    rng = np.random.default_rng(3)
    m = np.zeros(16 * 24, dtype=np.uint8)
    m[rng.choice(m.shape[0], 350, replace=False)] = 1
    mask = m.reshape(1, 16, 24)
    stat, dof, dead = sr.chi_square(mask[0], 40, lambda k: sr.sample_valid_points(mask, 40, 1, k)[0][:, 1], 200)
    assert dof == 343 and dead == 0


# ---- the C ABI and the Python surface, without a GPU ----------------------------------------------------------
def test_header_and_signatures():
    from implicit_depth_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "lidf_hip.h")).read()
    assert re.search(r"#define LIDF_ABI_VERSION 14\b", hdr) and _lib.ABI == 14
    assert "lidf_sample_valid_points(const void* mask, int mask_dtype, int batch, int height, int width," in hdr
    assert "size_t lidf_sample_valid_workspace_bytes(int batch, int height, int width);" in hdr
    res, args = _lib.SIGNATURES["lidf_sample_valid_points"]
    P, I = C.c_void_p, C.c_int
    assert res is C.c_int and args == [P, I, I, I, I, I, P, P, P, P, P, P, C.c_size_t, P]
    assert _lib.SIGNATURES["lidf_sample_valid_workspace_bytes"] == (C.c_size_t, [I, I, I])


def test_malformed_calls_are_refused_before_any_hip_call():
    from implicit_depth_amd import _lib
    L = _lib.lib()
    assert L.lidf_version() == 14
    BAD = -1
    ws_bytes = L.lidf_sample_valid_workspace_bytes(2, 16, 24)
    assert ws_bytes >= 2 * 6 * 8 + 2 * 7 * 4
    # host buffers stand in for device memory: none of these calls may reach a kernel launch
    buf = (C.c_char * 65536)()
    p = C.cast(buf, C.c_void_p)

    def call(mask=p, dtype=0, bs=2, h=16, w=24, n=10, rng=p, bid=p, flat=p, idx=None, cnt=p, ws=p, wsb=ws_bytes):
        return L.lidf_sample_valid_points(mask, dtype, bs, h, w, n, rng, bid, flat, idx, cnt, ws, wsb, None)

    assert call(h=12) == BAD and call(w=20) == BAD and call(h=0) == BAD
    assert call(n=0) == BAD and call(n=-3) == BAD
    assert call(bs=0) == BAD and call(bs=-1) == BAD
    assert call(dtype=4) == BAD and call(dtype=-1) == BAD
    for name in ("mask", "rng", "bid", "flat", "cnt", "ws"):
        assert call(**{name: None}) == BAD, name
    assert call(wsb=ws_bytes - 1) == BAD and call(wsb=0) == BAD


def test_stale_library_message(tmp_path, monkeypatch):
    """An ABI-14 library from before the sampler answers the right version and lacks the symbols: lib() says so."""
    import subprocess
    from implicit_depth_amd import _lib
    src = tmp_path / "old.c"
    src.write_text("int lidf_version(void) { return 14; }\n")
    so = tmp_path / "libold.so"
    subprocess.run(["gcc", "-shared", "-fPIC", "-o", str(so), str(src)], check=True)
    monkeypatch.setattr(_lib, "LIB_PATH", str(so))
    monkeypatch.setattr(_lib, "_lib", None)
    with pytest.raises(RuntimeError, match="rebuild the library"):
        _lib.lib()


def test_options():
    from implicit_depth_amd.pipeline import LidfOptions
    with pytest.raises(ValueError):
        LidfOptions(valid_sample_num=100, valid_stride=2)
    with pytest.raises(ValueError):
        LidfOptions(valid_sample_num=0)
    assert LidfOptions().sample_num() == 0 and LidfOptions(valid_sample_num=-1).sample_num() == 0
    assert LidfOptions(valid_sample_num=-1, valid_stride=3).sample_num() == 0
    assert LidfOptions(valid_sample_num=10000).sample_num() == 10000
    assert LidfOptions(valid_sample_num=10000, valid_stride=1).sample_num() == 10000
    opt = LidfOptions(valid_sample_num=5)
    opt.valid_stride = 2                     # set after construction: caught where the option is read
    with pytest.raises(ValueError):
        opt.sample_num()


def test_python_surface_refuses_before_the_device():
    import torch
    from implicit_depth_amd import query as Q
    with pytest.raises(ValueError):
        Q.sample_valid_points(torch.ones(1, 8, 8), 4, block_x=4)
    with pytest.raises(ValueError):
        Q.sample_valid_points(torch.ones(1, 8, 8), 4, block_y=16)
    with pytest.raises(ValueError):
        Q.sample_valid_points(torch.ones(1, 12, 8), 4)
    with pytest.raises(RuntimeError, match="CUDA"):
        Q.sample_valid_points(torch.ones(1, 8, 8), 4)
