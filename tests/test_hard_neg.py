"""CPU: hard-negative mining on the device (csrc/lidf_select.hip) — the numpy twin the GPU tests hold the kernels to
(tests/hard_neg_ref.py), the option, the exported symbols and the C ABI's argument checks, which run before any HIP
call."""
import ctypes as C

import numpy as np
import pytest
import torch

import hard_neg_ref as hn

BAD, UNSUP, WS = -1, -2, -3


@pytest.mark.parametrize("n,ratio", [(10, 0.1), (257, 0.1), (257, 1.0), (1000, 0.37), (4097, 0.1)])
def test_twin_agrees_with_torch_topk_without_ties(n, ratio):
    v = torch.randn(n, generator=torch.Generator().manual_seed(n)).float()
    assert torch.unique(v).numel() == n
    r = hn.topk_mean_ref(v.numpy(), ratio)
    top, idx = torch.topk(v, int(n * ratio))
    assert r["k"] == top.numel()
    assert np.array_equal(r["sel"], np.sort(idx.numpy()))
    assert np.array_equal(np.sort(v.numpy()[r["sel"]])[::-1], top.numpy())
    assert abs(r["mean64"] - float(top.double().mean())) <= 1e-12 * r["scale"]
    w = torch.zeros(n)
    w[idx] = 1.0 / top.numel()
    assert np.array_equal(r["weights"], w.numpy())


def test_twin_order_and_ties():
    nan, inf = float("nan"), float("inf")
    v = np.array([1.0, nan, -inf, inf, -nan, 0.0, -0.0, 1e-45, -1e-45, -3.0, 1.0], dtype=np.float32)
    key = hn.order_key(v)
    assert key[1] == key[4] == 0xffffffff and key[5] == key[6]                # NaNs equal, +-0 equal
    assert key[1] > key[3] > key[0] == key[10] > key[7] > key[5] > key[8] > key[9] > key[2]
    # NaN first (torch.topk's order), then +inf; equal values: the lowest index
    assert list(hn.topk_mean_ref(v, 2 / 11 + 1e-9)["sel"]) == [1, 4]
    assert list(hn.topk_mean_ref(v, 4 / 11 + 1e-9)["sel"]) == [0, 1, 3, 4]
    assert list(hn.topk_mean_ref(v, 7 / 11 + 1e-9)["sel"]) == [0, 1, 3, 4, 5, 7, 10]   # +0.0 at 5 before -0.0 at 6
    top = torch.topk(torch.from_numpy(v), 3)[0]
    assert torch.isnan(top[:2]).all() and top[2] == inf
    z = hn.topk_mean_ref(np.zeros(20, dtype=np.float32), 0.25)
    assert list(z["sel"]) == [0, 1, 2, 3, 4] and z["mean64"] == 0.0
    e = hn.topk_mean_ref(np.ones(9, dtype=np.float32), 0.1)
    assert e["k"] == 0 and np.isnan(e["mean64"]) and not e["weights"].any()


def test_k_is_a_double_product():
    assert hn.k_of(100, 0.29) == 28 and hn.k_of(100, 0.57) == 56
    assert int(np.float32(100) * np.float32(0.29)) == 29 and int(np.float32(100) * np.float32(0.57)) == 57
    assert hn.topk_mean_ref(np.arange(100, dtype=np.float32), 0.29)["k"] == 28
    assert hn.topk_mean_ref(np.arange(100, dtype=np.float32), 0.5, count=7)["k"] == 3


def test_option_values():
    from implicit_depth_amd import LidfLossOptions
    from implicit_depth_amd.losses import _check_types
    assert LidfLossOptions().hard_neg_select == "torch"
    _check_types(LidfLossOptions(hard_neg_select="device"))
    _check_types(LidfLossOptions(hard_neg=True, hard_neg_ratio=0.1, hard_neg_select="device"), prob=False)
    for bad in ("x", "", None, "Device"):
        with pytest.raises(ValueError, match="hard_neg_select"):
            _check_types(LidfLossOptions(hard_neg_select=bad))


def test_symbols_are_exported_with_signatures():
    import implicit_depth_amd
    from implicit_depth_amd import _lib
    L = _lib.lib()
    for name in ("lidf_topk_mean_workspace_bytes", "lidf_topk_mean_f32", "lidf_stage1_hard_neg_f32",
                 "lidf_refine_hard_neg_f32"):
        assert name in _lib.SIGNATURES and hasattr(L, name), name
        assert getattr(L, name).argtypes == _lib.SIGNATURES[name][1]
    assert _lib.SIGNATURES["lidf_topk_mean_f32"][1][2] is C.c_double      # the ratio travels as a double
    assert [f for f, _ in _lib.LidfTopkJob._fields_] == ["values", "n", "count", "mean", "weights"]
    assert L.lidf_version() == _lib.ABI == 14
    assert callable(implicit_depth_amd.topk_mean) and "topk_mean" in implicit_depth_amd.__all__


def test_topk_mean_refuses_cpu_tensors_and_bad_ratios():
    from implicit_depth_amd import topk_mean
    with pytest.raises(RuntimeError, match="CUDA"):
        topk_mean(torch.zeros(8), 0.1)
    for ratio in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="ratio"):
            topk_mean(torch.zeros(8), ratio)


def _job(values=0x10000, n=100, count=None, mean=0x20000, weights=0x30000):
    from implicit_depth_amd import _lib
    return _lib.LidfTopkJob(values, n, count, mean, weights)


def test_c_abi_argument_errors_without_gpu():
    """Every refusal below comes back before a HIP call or a dereference: the pointers are made-up numbers."""
    from implicit_depth_amd import _lib
    L = _lib.lib()
    ws, need = C.c_void_p(0x100000), L.lidf_topk_mean_workspace_bytes(1, 100)
    call = lambda job, n_jobs=1, ratio=0.1, w=ws, b=need: L.lidf_topk_mean_f32(  # noqa: E731
        None if job is None else C.byref(job), n_jobs, ratio, w, b, None)
    assert call(None) == BAD
    assert call(_job(), n_jobs=0) == BAD and call(_job(), n_jobs=9) == BAD and call(_job(), n_jobs=-1) == BAD
    assert call(_job(values=None)) == BAD
    assert call(_job(mean=None)) == BAD
    assert call(_job(n=-1)) == BAD
    for ratio in (-1e-9, 1.0 + 1e-9, float("nan"), float("inf")):
        assert call(_job(), ratio=ratio) == BAD
    assert call(_job(values=0x10002)) == BAD and call(_job(weights=0x30001)) == BAD
    assert call(_job(n=2 ** 31)) == UNSUP
    # the workspace: missing, or a byte short
    assert call(_job(), w=None) == WS
    assert call(_job(), b=need - 1) == WS
    assert call(_job(), b=0) == WS
    jobs = (_lib.LidfTopkJob * 2)(_job(n=100), _job(n=50000))
    need2 = L.lidf_topk_mean_workspace_bytes(2, 50000)
    assert L.lidf_topk_mean_f32(jobs, 2, 0.1, ws, need2 - 1, None) == WS
    assert L.lidf_topk_mean_f32(jobs, 2, 0.1, ws, need, None) == WS      # sized for the smaller job
    jobs[1].mean = None
    assert L.lidf_topk_mean_f32(jobs, 2, 0.1, ws, need2, None) == BAD    # a later job's NULL mean
    # the stage wrappers
    nul = (None,) * 4
    assert L.lidf_stage1_hard_neg_f32(None, 0.1, None, *nul, ws, need, None) == BAD
    assert L.lidf_refine_hard_neg_f32(None, 0.1, *nul, ws, need, None) == BAD
    a = _lib.LidfRefineLossArgs()
    a.n_rays = -1
    assert L.lidf_refine_hard_neg_f32(C.byref(a), 0.1, *nul, ws, need, None) == BAD
    a.n_rays = 0
    assert L.lidf_refine_hard_neg_f32(C.byref(a), 0.1, *nul, ws, need, None) == 0     # no ray: nothing to do
    # a forward's struct without its outputs, a ratio out of range, a workspace too small
    a.n_rays, a.batch, a.height, a.width = 100, 1, 10, 10
    for f in ("xyz", "ray_bid", "ray_flat", "pix2ray", "gt_pos", "pred_pos_refine"):
        setattr(a, f, 0x40000)
    assert L.lidf_refine_hard_neg_f32(C.byref(a), 0.1, *nul, ws, need, None) == BAD
    for f in ("loss", "pos_unreduced", "surf_norm_dist", "dx_dist", "dy_dist"):
        setattr(a, f, 0x50000)
    assert L.lidf_refine_hard_neg_f32(C.byref(a), 1.5, *nul, ws, 1 << 20, None) == BAD
    assert L.lidf_refine_hard_neg_f32(C.byref(a), 0.1, *nul, ws, 64, None) == WS
    s = _lib.LidfLossArgs()
    s.n_rays = -1
    assert L.lidf_stage1_hard_neg_f32(C.byref(s), 0.1, None, *nul, ws, need, None) == BAD


def test_workspace_size_is_monotone():
    from implicit_depth_amd import _lib
    L = _lib.lib()
    size = L.lidf_topk_mean_workspace_bytes
    ns = [0, 1, 9, 4093, 4094, 4096, 4097, 160000, 1000003, 2 ** 31 - 2]
    for jobs in range(1, 9):
        got = [size(jobs, n) for n in ns]
        assert all(a <= b for a, b in zip(got, got[1:])), got
        assert got[0] > 0        # n_max == 0 still runs the kernel that writes the NaN means and their state
    for n in ns:
        got = [size(jobs, n) for jobs in range(1, 9)]
        assert all(a < b for a, b in zip(got, got[1:])), got
    # what is refused has no size
    assert size(0, 100) == 0 and size(9, 100) == 0 and size(1, -1) == 0
    # 16 bytes per slab of 4096 values and job (a double and two counters), beside the fixed histograms
    assert size(1, 1000003) - size(1, 0) < 16 * (1000003 // 4096 + 2) + 3 * 256
