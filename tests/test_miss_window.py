"""CPU: the miss-ray window's semantics (include/lidf_hip.h, lidf_miss_ray_window_f32) as tests/miss_window_ref.py
states them — the structural checker is validated on the REFERENCE's own window (tests/golden/g6_miss_ray.npz 't_*',
LIDF.get_miss_ray in the train flavour) before it judges the numpy twin of the kernels; the twin selects what the
oracle's restatement selects for the same starts; both branches of `sampling` and their edges; the twin's starts are
uniform (chi-square, one fixed seed); and the C ABI and the Python surface refuse malformed calls without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import miss_window_ref as mw
from util import orc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
G6_STARTS = [29, 1, 0]
CHI_SEED, CHI_CALLS = 20261019, 20000


def g6():
    g = np.load(os.path.join(HERE, "golden", "g6_miss_ray.npz"))
    return g, g["t_mask"], int(g["t_miss_sample_num"])


def test_checker_accepts_the_reference():
    g, mask, n = g6()
    assert mask.shape == (3, 12, 16) and n == 20 and mw.nonzero(mask).sum(1).tolist() == [96, 90, 15]
    ref = {"miss_bid": g["t_miss_bid"], "miss_flat_img_id": g["t_miss_flat_img_id"]}
    assert mw.check_window(mask, n, ref) == G6_STARTS
    ref["window"] = [[96, 29, 20, 0], [90, 1, 20, 20], [15, 0, 15, 40]]
    ref["n_rays"] = [55, 201]
    assert mw.check_window(mask, n, ref) == G6_STARTS


def test_checker_rejects_wrong_windows():
    g, mask, n = g6()
    bid, flat = g["t_miss_bid"], g["t_miss_flat_img_id"]
    mw.check_window(mask, n, {"miss_bid": bid, "miss_flat_img_id": flat})
    for drop in (0, 7, 19, 20, 54):                        # one row dropped
        keep = np.arange(bid.shape[0]) != drop
        with pytest.raises(AssertionError):
            mw.check_window(mask, n, {"miss_bid": bid[keep], "miss_flat_img_id": flat[keep]})
    for a, b in ((3, 4), (0, 19), (19, 20), (45, 50)):     # two rows swapped (inside an image and across two)
        perm = np.arange(bid.shape[0])
        perm[[a, b]] = perm[[b, a]]
        with pytest.raises(AssertionError):
            mw.check_window(mask, n, {"miss_bid": bid[perm], "miss_flat_img_id": flat[perm]})
    # a start beyond cnt - n: image 0 from rank 77 on holds 19 pixels only
    order = np.flatnonzero(mw.nonzero(mask)[0])
    late = {"miss_bid": np.concatenate((np.zeros(19, dtype=np.int64), bid[20:])),
            "miss_flat_img_id": np.concatenate((order[77:], flat[20:]))}
    with pytest.raises(AssertionError):
        mw.check_window(mask, n, late)
    with pytest.raises(AssertionError):                    # ... and a window tensor that claims one
        mw.check_window(mask, n, {"miss_bid": bid, "miss_flat_img_id": flat,
                                  "window": [[96, 77, 20, 0], [90, 1, 20, 20], [15, 0, 15, 40]]})
    with pytest.raises(AssertionError):                    # a pixel the mask does not hold
        bad = flat.copy()
        bad[0] = int(np.flatnonzero(~mw.nonzero(mask)[0])[0])
        mw.check_window(mask, n, {"miss_bid": bid, "miss_flat_img_id": bad})


def test_twin_against_the_oracle(monkeypatch):
    import torch
    g, mask, n = g6()
    tw = mw.select(mask, n, starts=G6_STARTS)
    assert tw["window"].tolist() == [[96, 29, 20, 0], [90, 1, 20, 20], [15, 0, 15, 40]] and tw["n_rays"].tolist() == [55, 201]
    mw.check_window(mask, n, tw)
    miss_idx = torch.nonzero(torch.from_numpy(mask).reshape(3, -1), as_tuple=False)
    drawn = list(G6_STARTS)

    def choice(start_range):   # np.random.choice(start_range) of the reference, answering the recorded starts
        s = drawn.pop(0)
        assert 0 <= s < start_range
        return s

    monkeypatch.setattr(orc.np.random, "choice", choice)
    rows = orc.sample_miss_window(miss_idx, 3, n)
    assert (rows.numpy() == tw["rows"]).all()
    assert (miss_idx[rows, 0].numpy() == tw["miss_bid"]).all() and (miss_idx[rows, 1].numpy() == tw["miss_flat_img_id"]).all()
    for k in ("miss_bid", "miss_flat_img_id", "miss_img_ind"):   # and the reference's own run
        assert (tw[k] == g["t_" + k]).all(), k
    # every other start of image 0, the reference's restatement again
    for s0 in (0, 76):
        tw = mw.select(mask, n, starts=[s0, 70, 5])
        drawn[:] = [s0, 70]
        assert (orc.sample_miss_window(miss_idx, 3, n).numpy() == tw["rows"]).all()
        assert tw["window"][:, 1].tolist() == [s0, 70, 0]
    assert (orc.sample_miss_window(miss_idx, 3, -1).numpy() == np.arange(201)).all()


def _counts_mask(counts, hw=(5, 9), seed=0):
    rng = np.random.default_rng(seed)
    mask = np.zeros((len(counts), hw[0] * hw[1]), dtype=np.float32)
    for b, c in enumerate(counts):
        mask[b, rng.choice(mask.shape[1], c, replace=False)] = 1.0 + b
    return mask.reshape(len(counts), *hw)


def test_both_branches_and_their_edges():
    n = 20
    mask = _counts_mask([30, 30, 0])                       # T = 60 = bs * n: nothing is sampled
    for kw in (dict(seed=3, counter=0), dict(starts=[5, 5, 5])):
        tw = mw.select(mask, n, **kw)
        assert tw["window"].tolist() == [[30, 0, 30, 0], [30, 0, 30, 30], [0, 0, 0, 60]] and tw["n_rays"].tolist() == [60, 60]
        assert (tw["rows"] == np.arange(60)).all()
        mw.check_window(mask, n, tw)
    mask.reshape(3, -1)[2, 11] = 1.0                       # one more pixel: T = 61 > 60, images 0 and 1 are windowed
    tw = mw.select(mask, n, seed=3, counter=0)
    w = tw["window"]
    assert w[:, 0].tolist() == [30, 30, 1] and w[:, 2].tolist() == [20, 20, 1] and w[:, 3].tolist() == [0, 20, 40]
    assert 0 <= w[0, 1] <= 10 and 0 <= w[1, 1] <= 10 and w[2, 1] == 0 and tw["n_rays"].tolist() == [41, 61]
    assert w[0, 1] == mw.draw_start(30, n, 0, 3, 0) and w[1, 1] == mw.draw_start(30, n, 1, 3, 0)
    mw.check_window(mask, n, tw)
    tw = mw.select(mask, n, starts=[-4, 99, 7])            # starts are clamped, and ignored where nothing is drawn
    assert tw["window"][:, 1].tolist() == [0, 10, 0]
    mw.check_window(mask, n, tw)
    mask = _counts_mask([20, 45, 21])                      # cnt == n keeps the whole image; cnt == n + 1: a range of 2
    seen = set()
    for c in range(64):
        tw = mw.select(mask, n, seed=9, counter=c)
        w = tw["window"]
        assert w[0].tolist() == [20, 0, 20, 0] and w[2, 2] == 20 and w[2, 1] in (0, 1) and 0 <= w[1, 1] <= 25
        mw.check_window(mask, n, tw)
        seen.add(int(w[2, 1]))
    assert seen == {0, 1}
    # NaN is non-zero, -0.0 is zero; integer and bool masks
    m = np.zeros((1, 2, 4), dtype=np.float32)
    m[0, 0, 1], m[0, 1, 2], m[0, 1, 3] = np.nan, -0.0, 1e-30
    assert mw.select(m, 1, starts=[1])["miss_flat_img_id"].tolist() == [7]
    assert mw.select(m, 2, starts=[0])["miss_flat_img_id"].tolist() == [1, 7]
    for dt in (np.uint8, np.bool_, np.int32, np.int64):
        assert mw.select((m != 0).astype(dt), 1, starts=[0])["miss_flat_img_id"].tolist() == [1]


def test_state_and_domain():
    """The same state gives the same window; seed, counter and image all enter; the window's counter domain is not
    one of the valid sampler's."""
    import sampler_ref as sr
    assert mw.DOMAIN == 0x80000002 and mw.DOMAIN not in (sr.KEY_WORD, sr.KEY_WORD + 1)
    big = 76800 - 20000 + 1
    a = [mw.draw_start(76800, 20000, b, 5, 11) for b in range(8)]
    assert a == [mw.draw_start(76800, 20000, b, 5, 11) for b in range(8)] and len(set(a)) == 8
    assert all(0 <= s < big for s in a)
    assert a != [mw.draw_start(76800, 20000, b, 5, 12) for b in range(8)]
    assert a != [mw.draw_start(76800, 20000, b, 6, 11) for b in range(8)]
    many = mw.draw_start(76800, 20000, 3, 5, np.arange(9, 14, dtype=np.uint64))
    assert many.tolist() == [mw.draw_start(76800, 20000, 3, 5, c) for c in range(9, 14)]
    assert mw.draw_start(96, 20, 0, -1, -1) == mw.draw_start(96, 20, 0, 2 ** 64 - 1, 2 ** 64 - 1)


def test_uniformity_of_the_twin():
    """g6 image 0 (cnt 96, n 20: 77 possible starts), 20,000 consecutive counters of one seed: Pearson's chi-square of
    the start counts against the uniform expectation stays below the 1 - 1e-6 quantile of chi-square with 76 degrees
    of freedom. The seed is fixed, so the outcome is too."""
    from scipy.stats import chi2
    _, mask, n = g6()
    cnt = int(mw.nonzero(mask)[0].sum())
    rng = cnt - n + 1
    assert rng == 77
    s = mw.draw_start(cnt, n, 0, CHI_SEED, np.arange(CHI_CALLS, dtype=np.uint64))
    counts = np.bincount(s, minlength=rng)
    assert counts.shape[0] == rng and counts.min() > 0
    exp = CHI_CALLS / rng
    stat = float(((counts - exp) ** 2 / exp).sum())
    bound = float(chi2.ppf(1 - 1e-6, rng - 1))
    print("chi-square of the starts: %.1f, bound %.1f (dof %d)" % (stat, bound, rng - 1))
    assert stat <= bound


# ---- the C ABI and the Python surface, without a GPU ----------------------------------------------------------
def test_header_and_signatures():
    from implicit_depth_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "lidf_hip.h")).read()
    assert re.search(r"#define LIDF_ABI_VERSION 14\b", hdr) and _lib.ABI == 14
    assert "size_t lidf_miss_window_workspace_bytes(int batch, int64_t n_pixels);" in hdr
    assert "int lidf_miss_ray_window_f32(const void* mask, int mask_dtype, const float* intr, int batch, int height, int width," in hdr
    for words in ("Philox4x32-10", "0x80000000 + 2", "(cnt_b, s_b, len_b, dst_b)", "(R_out, T)", "batch * n < T",
                  "clamp(starts[b], 0, cnt_b - n)", "rows >= R_out", "lidf_miss_window_workspace_bytes / lidf_miss_ray_window_f32"):
        assert words in hdr, words
    P, I = C.c_void_p, C.c_int
    res, args = _lib.SIGNATURES["lidf_miss_ray_window_f32"]
    assert res is C.c_int and args == [P, I, P, I, I, I, I] + [P] * 12 + [C.c_size_t, P]
    assert _lib.SIGNATURES["lidf_miss_window_workspace_bytes"] == (C.c_size_t, [I, C.c_int64])


def test_malformed_calls_are_refused_before_any_hip_call():
    from implicit_depth_amd import _lib
    L = _lib.lib()
    assert L.lidf_version() == 14
    BAD, UNSUPPORTED, WORKSPACE = -1, -2, -3
    ws_bytes = L.lidf_miss_window_workspace_bytes(3, 3 * 12 * 16)
    assert ws_bytes >= 2 * 4 * 1 + 4 * 4 and L.lidf_miss_window_workspace_bytes(0, 10) == 0
    assert L.lidf_miss_window_workspace_bytes(8, 8 * 240 * 320) >= 2 * 4 * 600 + 4 * 9
    # host buffers stand in for device memory: none of these calls may reach a kernel launch
    buf = (C.c_char * 65536)()
    p = C.cast(buf, C.c_void_p)

    def call(mask=p, dtype=0, intr=p, bs=3, h=12, w=16, n=20, rng=p, starts=None, bid=p, flat=p, pix=p, rdir=p, b64=p,
             f64=p, p64=p, window=p, n_rays=p, ws=p, wsb=ws_bytes):
        return L.lidf_miss_ray_window_f32(mask, dtype, intr, bs, h, w, n, rng, starts, bid, flat, pix, rdir, b64, f64,
                                          p64, window, n_rays, ws, wsb, None)

    assert call(bs=0) == BAD and call(bs=-1) == BAD
    assert call(n=0) == BAD and call(n=-1) == BAD and call(n=-20000) == BAD
    assert call(h=0) == BAD and call(h=-12) == BAD and call(w=0) == BAD and call(w=-1) == BAD
    assert call(dtype=4) == BAD and call(dtype=-1) == BAD
    for name in ("mask", "window", "n_rays", "ws"):
        assert call(**{name: None}) == BAD, name
    assert call(rng=None, starts=None) == BAD
    assert call(intr=None) == BAD                                    # ray_dir without intr
    assert call(wsb=ws_bytes - 1) == WORKSPACE and call(wsb=0) == WORKSPACE
    assert call(bs=3, n=2 ** 30) == UNSUPPORTED                       # bs * n beyond int32
    assert call(bs=1, h=65536, w=32768) == UNSUPPORTED                # more pixels than lidf_miss_ray_count takes


def test_options():
    from implicit_depth_amd.pipeline import LidfOptions
    assert LidfOptions().miss_sample == "numpy" and LidfOptions().miss_starts is None
    assert LidfOptions(miss_sample="device").miss_route() == "device"
    assert LidfOptions(miss_sample="numpy").miss_route() == "numpy"
    for bad in ("Device", "gpu", None, 1, ""):
        with pytest.raises(ValueError):
            LidfOptions(miss_sample=bad)
    opt = LidfOptions()
    opt.miss_sample = "hip"                  # set after construction: caught where the option is read
    with pytest.raises(ValueError):
        opt.miss_route()


def test_python_surface_refuses_before_the_device():
    import torch
    from implicit_depth_amd import query as Q
    one = torch.ones(1)
    with pytest.raises(RuntimeError, match="CUDA"):
        Q.sample_miss_window(torch.ones(1, 8, 8), one, one, one, one, 4)
    with pytest.raises(RuntimeError, match="CUDA"):
        Q.sample_miss_window(torch.ones(1, 8, 8), one, one, one, one, 4, state=torch.zeros(2, dtype=torch.int64))
    for state in (torch.zeros(2, dtype=torch.int32), torch.zeros(3, dtype=torch.int64), torch.zeros(2, 1, dtype=torch.int64)):
        with pytest.raises(RuntimeError, match="state must be"):
            Q.sample_miss_window(torch.ones(1, 8, 8), one, one, one, one, 4, state=state)
    with pytest.raises(RuntimeError, match="starts must be"):
        Q.sample_miss_window(torch.ones(1, 8, 8), one, one, one, one, 4, starts=torch.zeros(1, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="starts must be"):
        Q.sample_miss_window(torch.ones(2, 8, 8), one, one, one, one, 4, starts=torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError):
        Q.sample_miss_window(torch.ones(1, 8, 8), one, one, one, one, 0)
    with pytest.raises(RuntimeError, match="dtype"):
        Q.sample_miss_window(torch.ones(1, 8, 8).half(), one, one, one, one, 4)
    with pytest.raises(RuntimeError, match="CUDA"):   # -1 is plain get_miss_ray
        Q.sample_miss_window(torch.ones(1, 8, 8), one, one, one, one, -1)
