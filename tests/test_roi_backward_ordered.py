"""CPU: the ordered RoIAlign adjoint (roi_backward="ordered", lidf_ray_features_backward_ordered_f32).

The numpy float32 twin of its summation order (roi_backward_ref.py) is held to float64 — autograd of the oracle's
RoIAlign in torch ops (roi_ref.py), with the float32 torch-op adjoint's own error as the unit (util.assert_f64_close,
F64_K) — and must refuse three wrong adjoints. The entry's argument and workspace errors precede the first HIP call,
so they run here through ctypes; the option is checked where it is set."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import roi_backward_ref as rb
from util import F64_K, ROOT, assert_f64_close

BAD, UNSUP, WS = -1, -2, -3
FAKE = 0x10000   # an aligned address no check dereferences

# (B, H, W, roi_inp_bbox): boxes clamped on both sides, the smallest image with an interior, partial last tiles,
# an odd half, the narrowest box
SHAPES = [(1, 5, 7, 8), (2, 9, 9, 8), (1, 18, 35, 8), (2, 12, 16, 6), (2, 12, 16, 2)]


def _case(B, H, W, seed):
    pix, bid = rb.pixel_rays(B, H, W)
    g = np.random.default_rng(seed).standard_normal((pix.shape[0], 128 + 27)).astype(np.float32)
    return g, pix, bid


_REFS = {}


def _refs(shape):
    """(g, pix, bid, float64 adjoint, float32 torch-op adjoint) of a shape, computed once."""
    if shape not in _REFS:
        B, H, W, bbox = shape
        g, pix, bid = _case(B, H, W, 11)
        _REFS[shape] = (g, pix, bid, rb.torch_adjoint(g, pix, bid, B, H, W, bbox, torch.float64),
                        rb.torch_adjoint(g, pix, bid, B, H, W, bbox, torch.float32))
    return _REFS[shape]


@pytest.mark.parametrize("shape", SHAPES)
def test_twin_against_float64(shape):
    B, H, W, bbox = shape
    g, pix, bid, r64, r32 = _refs(shape)
    got = rb.roi_backward_ordered(g, pix, bid, B, H, W, bbox)
    assert got.dtype == np.float32 and got.shape == (B, 32, H, W)
    assert_f64_close("ordered twin %s" % (shape,), torch.from_numpy(got), r64, r32, k=F64_K)


def test_twin_sparse_and_shared_pixels_against_float64():
    """Rays of one frame only, and pixels named by two and three rays (the twin adds them in ray order)."""
    B, H, W, bbox = 2, 12, 16, 8
    idx = np.array([0, 15, 15, 100, 100, 100, 191, 37, 5 * 16 + 8])
    pix = np.stack((idx % W, idx // W), 1).astype(np.int32)
    bid = np.ones(len(idx), dtype=np.int32)
    g = np.random.default_rng(12).standard_normal((len(idx), 155)).astype(np.float32)
    got = rb.roi_backward_ordered(g, pix, bid, B, H, W, bbox)
    assert not got[0].any()
    assert_f64_close("ordered twin, shared pixels", torch.from_numpy(got),
                     rb.torch_adjoint(g, pix, bid, B, H, W, bbox, torch.float64),
                     rb.torch_adjoint(g, pix, bid, B, H, W, bbox, torch.float32), k=F64_K)


@pytest.mark.parametrize("mutate", ["drop_clamped", "swap_bins", "unclamped_count"])
@pytest.mark.parametrize("shape", [(1, 5, 7, 8), (1, 18, 35, 8), (2, 12, 16, 6)])
def test_twin_refuses_wrong_adjoint(shape, mutate):
    """An adjoint that drops the clamped boxes, swaps two bins, or divides by the unclamped box's sample count."""
    B, H, W, bbox = shape
    g, pix, bid, r64, r32 = _refs(shape)
    wrong = rb.roi_backward_ordered(g, pix, bid, B, H, W, bbox, mutate=mutate)
    with pytest.raises(AssertionError):
        assert_f64_close("%s %s" % (mutate, shape), torch.from_numpy(wrong), r64, r32, k=F64_K)


def test_twin_is_its_own_rerun():
    g, pix, bid = _case(1, 18, 35, 13)
    a = rb.roi_backward_ordered(g, pix, bid, 1, 18, 35, 8)
    b = rb.roi_backward_ordered(g.copy(), pix.copy(), bid.copy(), 1, 18, 35, 8)
    assert np.array_equal(a, b)


# ---- the C entry, without a GPU -------------------------------------------------------------------------------------
def _call(L, d_rayfeat=FAKE, pix=FAKE, bid=FAKE, n=10, B=2, H=24, W=32, bbox=8, lv=4, d_feat=FAKE, ws=FAKE,
          wsb=None):
    if wsb is None:
        wsb = L.lidf_ray_features_backward_ordered_workspace_bytes(B, H, W)
    return L.lidf_ray_features_backward_ordered_f32(d_rayfeat, pix, bid, n, B, H, W, bbox, lv, d_feat, ws, wsb, None)


def test_ordered_workspace_bytes():
    from implicit_depth_amd import _lib
    L = _lib.lib()
    f = L.lidf_ray_features_backward_ordered_workspace_bytes
    assert f(2, 24, 32) == 2 * 129 * 24 * 32 * 4          # the parked image and the rays-per-pixel table
    assert f(8, 240, 320) == 8 * 129 * 240 * 320 * 4
    assert f(0, 24, 32) == 0 and f(2, -1, 32) == 0 and f(2, 24, 0) == 0


def test_ordered_argument_errors_without_gpu():
    from implicit_depth_amd import _lib
    L = _lib.lib()
    assert _call(L, n=-1) == BAD
    for kw in (dict(B=0), dict(H=0), dict(W=-3), dict(d_feat=None), dict(lv=-1), dict(lv=17)):
        assert _call(L, **kw) == BAD, kw
    assert _call(L, n=0, d_feat=None) == BAD              # the output is written on an empty ray set too
    for kw in (dict(d_rayfeat=None), dict(pix=None), dict(bid=None)):
        assert _call(L, **kw) == BAD, kw
    # half = roi_inp_bbox / 2 outside 1 .. 16, and sizes beyond the launch grid
    for kw in (dict(bbox=0), dict(bbox=1), dict(bbox=34), dict(bbox=-8), dict(B=2048), dict(B=4, H=16384, W=16384)):
        assert _call(L, **kw) == UNSUP, kw


def test_ordered_workspace_error_without_gpu():
    """A short or missing workspace is an error: the ordered route has no fallback to float atomics."""
    from implicit_depth_amd import _lib
    L = _lib.lib()
    need = L.lidf_ray_features_backward_ordered_workspace_bytes(2, 24, 32)
    assert _call(L, wsb=need - 1) == WS
    assert _call(L, wsb=2 * 128 * 24 * 32 * 4) == WS      # the size at which the default route still parks
    assert _call(L, wsb=0) == WS
    assert _call(L, ws=None) == WS
    assert _call(L, bbox=6, wsb=need - 1) == WS and _call(L, bbox=33 - 1, wsb=need - 1) == WS


def test_header_declares_both_entries():
    with open(os.path.join(ROOT, "include", "lidf_hip.h")) as f:
        text = f.read()
    assert re.search(r"size_t\s+lidf_ray_features_backward_ordered_workspace_bytes\(int32_t batch, int32_t height, "
                     r"int32_t width\);", text)
    m = re.search(r"int\s+lidf_ray_features_backward_ordered_f32\(([^;]*)\);", text)
    d = re.search(r"int\s+lidf_ray_features_backward_f32\(([^;]*)\);", text)
    assert m and d
    norm = lambda s: re.sub(r"\s+", " ", s).strip()
    assert norm(m.group(1)) == norm(d.group(1))           # the argument list of lidf_ray_features_backward_f32
    from implicit_depth_amd import _lib
    assert (_lib.SIGNATURES["lidf_ray_features_backward_ordered_f32"]
            == _lib.SIGNATURES["lidf_ray_features_backward_f32"])
    L = _lib.lib()
    assert L.lidf_ray_features_backward_ordered_f32.argtypes == L.lidf_ray_features_backward_f32.argtypes
    assert L.lidf_ray_features_backward_ordered_workspace_bytes.restype is C.c_size_t


# ---- the option -----------------------------------------------------------------------------------------------------
def test_options_roi_backward():
    from implicit_depth_amd.pipeline import LidfOptions
    assert LidfOptions().roi_backward == "atomic"
    assert LidfOptions(roi_backward="ordered").roi_route() == "ordered"
    for bad in ("x", "", None, "Ordered", True):
        with pytest.raises(ValueError):
            LidfOptions(roi_backward=bad)
    opt = LidfOptions()
    opt.roi_backward = "x"                                 # set after construction: caught where it is read
    with pytest.raises(ValueError):
        opt.roi_route()


def test_query_entry_points_refuse_unknown_roi_backward():
    """Checked before any tensor is looked at."""
    from implicit_depth_amd import query as Q
    with pytest.raises(ValueError):
        Q.lidf_query_train(*([None] * 11), roi_backward="x")
    with pytest.raises(ValueError):
        Q.lidf_refine_train(*([None] * 15), roi_backward="sorted")
