"""CPU: the stage-2 training loss. tests/golden/g10_refine_train.npz — the reference's own stage-2 iteration — pins the
tests' restatement (refine_loss_ref.py) in float32; the product's torch-op composite (losses.refine_loss_composite) is
held against the restatement in float64; ABI 14's entry points, struct layout and argument checks."""
import ctypes as C
import os
import re

import pytest
import torch

import refine_loss_ref as rl
from util import ROOT

# As tests/test_train_loss.py: both sides evaluate the same float32 formulas and differ in the association of sums of
# at most 126 terms (means over 42 rays x 3 coordinates, 3-term dot products of the normals).
F32_ROUNDING = 2e-5


def _near(got, ref, what):
    scale = ref.abs().max().item()
    err = (got - ref).abs().max().item()
    print(what, "err %.3g scale %.3g" % (err, scale))
    assert err <= F32_ROUNDING * max(scale, 1e-30), (what, err, scale)


@pytest.mark.parametrize("name", sorted(rl.G10_CASES))
def test_restatement_reproduces_the_reference(name):
    g, _ = rl.g10_files()
    d, ref = rl.g10_case(g, name)
    assert torch.equal(d["xyz_flat"][d["miss_bid"], d["miss_flat"]], d["gt_pos"])
    assert (ref["noise"] is None) == (name == "noperturb")
    assert bool((torch.bincount(d["pair_ray"], minlength=d["gt_pos"].shape[0]) == 0).any())   # a ray without pairs
    loss, gp = rl.loss_and_grad(d, torch.float32, int(g["epoch"]), **rl.G10_CASES[name])
    for i, k in enumerate(rl.REFINE_LOSS_KEYS):
        _near(loss[i], ref["loss"][i], (name, k))
    _near(gp, ref["g_pred_pos_refine"], (name, "g_pred_pos_refine"))


def _composite_dd(d, dt, dev="cpu"):
    dd = {"bs": d["bs"], "h": d["h"], "w": d["w"], "xyz_flat": d["xyz_flat"].to(dev), "gt_pos": d["gt_pos"].to(dev),
          "miss_bid": d["miss_bid"].to(dev), "miss_flat_img_id": d["miss_flat"].to(dev)}
    dd["pred_pos_refine"] = d["pred_pos_refine"].to(dev, dt, copy=True).requires_grad_(True)
    return dd


@pytest.mark.parametrize("case", rl.RANDOM_CASES, ids=[c[0] for c in rl.RANDOM_CASES])
def test_composite_in_float64_follows_the_restatement(case):
    from implicit_depth_amd import LidfLossOptions, refine_loss_composite
    name, R, kw, epoch, opt, up = case
    d = rl.random_case(R, **kw)
    loss, gp = rl.loss_and_grad(d, torch.float64, epoch, up, **opt)
    dd = _composite_dd(d, torch.float64)
    out = refine_loss_composite(dd, LidfLossOptions(**opt), "train", epoch)
    assert tuple(out) == rl.REFINE_LOSS_KEYS and out["loss_net"].dtype == torch.float64
    (out["loss_net"] * up).backward()
    got = torch.stack([out[k].detach() for k in rl.REFINE_LOSS_KEYS])
    assert (got - loss).abs().max().item() <= 1e-12 * loss.abs().max().item()
    assert (dd["pred_pos_refine"].grad - gp).abs().max().item() <= 1e-12 * gp.abs().max().item()
    if kw.get("zero_gt"):
        assert float(got[4]) == 0.0   # err: no ray whose gt_pos is not the zero point


@pytest.mark.parametrize("name", sorted(rl.G10_CASES))
def test_composite_on_the_fixture(name):
    from implicit_depth_amd import LidfLossOptions, refine_loss_composite
    g, _ = rl.g10_files()
    d, ref = rl.g10_case(g, name)
    opt = rl.G10_CASES[name]
    loss, gp = rl.loss_and_grad(d, torch.float64, 0, **opt)
    dd = _composite_dd(d, torch.float64)
    out = refine_loss_composite(dd, LidfLossOptions(**opt), "train", 0)
    out["loss_net"].backward()
    got = torch.stack([out[k].detach() for k in rl.REFINE_LOSS_KEYS])
    assert (got - loss).abs().max().item() <= 1e-12 * loss.abs().max().item()
    assert (dd["pred_pos_refine"].grad - gp).abs().max().item() <= 1e-12 * gp.abs().max().item()
    dd = _composite_dd(d, torch.float32)   # and in float32 it reproduces the reference's numbers
    out = refine_loss_composite(dd, LidfLossOptions(**opt), "train", 0)
    out["loss_net"].backward()
    for i, k in enumerate(rl.REFINE_LOSS_KEYS):
        _near(out[k].detach(), ref["loss"][i], (name, k))
    _near(dd["pred_pos_refine"].grad, ref["g_pred_pos_refine"], (name, "g_pred_pos_refine"))


def test_hard_neg_with_k_zero_gives_nan_means():
    """R < 10 at ratio 0.1: k = 0, torch.mean of an empty tensor (models/pipeline.py:768-770) — NaN losses and a
    gradient that the empty means do not reach, in the restatement and in the composite alike."""
    from implicit_depth_amd import LidfLossOptions, refine_loss_composite
    d = rl.random_case(7)
    opt = dict(hard_neg=True, hard_neg_ratio=0.1, smooth_w=0.5)
    loss, gp = rl.loss_and_grad(d, torch.float32, 0, **opt)
    dd = _composite_dd(d, torch.float32)
    out = refine_loss_composite(dd, LidfLossOptions(**opt))
    out["loss_net"].backward()
    for v in (dict(zip(rl.REFINE_LOSS_KEYS, loss)), out):
        assert all(torch.isnan(v[k]) for k in ("pos_loss", "surf_norm_loss", "smooth_loss", "loss_net"))
        assert torch.isfinite(v["err"]) and torch.isfinite(v["angle_err"])
    assert bool((gp == 0).all()) and bool((dd["pred_pos_refine"].grad == 0).all())


def test_refusals_without_gpu():
    from implicit_depth_amd import (IEF, PointNet2Stage, refine_forward_train, refine_loss, refine_loss_composite,
                                    train_refine_step)
    import train_loss_ref as tl
    g, _ = rl.g10_files()
    d, _ = rl.g10_case(g, "plain")
    dd = _composite_dd(d, torch.float32)
    with pytest.raises(RuntimeError, match="CUDA"):
        refine_loss(dd)
    for fn in (refine_loss, refine_loss_composite):
        with pytest.raises(NotImplementedError, match="train"):
            fn(dd, exp_type="valid")
    with pytest.raises(NotImplementedError, match="eval_metrics"):
        refine_loss(dd, exp_type="valid")
    batch, feat = rl.g10_batch(g)
    from implicit_depth_amd import IMNet
    with pytest.raises(RuntimeError, match="CUDA"):
        train_refine_step(batch, feat, PointNet2Stage(6, 128, 32), IMNet(385, 1), IEF("cpu", 385, 1, n_iter=2),
                          PointNet2Stage(6, 128, 32), IEF("cpu", 334, 1, n_iter=2))
    assert callable(refine_forward_train) and tl.LOSS_KEYS[1] == "prob_loss"


def test_refusal_texts_name_the_stage2_training_step():
    from implicit_depth_amd import IEF, PointNet2Stage, pipeline as pl
    from implicit_depth_amd.query import lidf_refine
    z = torch.zeros(1)
    offr, pn = IEF(torch.device("cpu"), 334, 1, n_iter=2), PointNet2Stage(6, 128, 32)
    with pytest.raises(RuntimeError, match="inference path.*pipeline.refine_forward_train") as e:
        lidf_refine(z, z, z, z, z, z, z, z, z, z, z, z, z, pn, offr)
    assert "has no backward" not in str(e.value)
    with pytest.raises(RuntimeError, match="inference path.*pipeline.refine_forward_train"):
        pl.refine_forward({}, pn, offr)


def test_options_of_stage2():
    from implicit_depth_amd import LidfLossOptions, LidfOptions
    o = LidfOptions()
    assert o.refine_perturb is True and o.refine_perturb_prob == 0.8
    assert LidfOptions(refine_perturb=False).refine_perturb is False
    doc = LidfLossOptions.__doc__
    assert "train_refine.yaml" in doc and "train_refine_hardneg.yaml" in doc and "20" in doc


def test_abi_14_and_the_new_entries(tmp_path):
    """The ABI number, the ctypes signatures, the struct layout against gcc's view of the header, and the status
    codes of malformed calls (checked before any HIP call)."""
    import subprocess
    from implicit_depth_amd import _lib
    src = open(os.path.join(ROOT, "include", "lidf_hip.h")).read()
    assert int(re.search(r"#define\s+LIDF_ABI_VERSION\s+(\d+)", src).group(1)) == 14
    L = _lib.lib()
    assert L.lidf_version() == _lib.ABI == 14
    A = _lib.LidfRefineLossArgs
    assert _lib.SIGNATURES["lidf_refine_loss_workspace_bytes"] == (C.c_size_t, [C.c_int64])
    for fn in ("lidf_refine_loss_f32", "lidf_refine_loss_backward_f32"):
        assert _lib.SIGNATURES[fn] == (C.c_int, [C.POINTER(A), C.c_void_p])
        assert getattr(L, fn).argtypes == [C.POINTER(A), C.c_void_p] and getattr(L, fn).restype == C.c_int
    assert L.lidf_refine_loss_workspace_bytes.restype == C.c_size_t
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "lidf_hip.h"', 'int main(void){',
             'printf("size %zu\\n", sizeof(LidfRefineLossArgs));']
    for f, _ in A._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(LidfRefineLossArgs, %s));' % (f, f))
    lines.append("return 0;}")
    (tmp_path / "probe.c").write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "probe.c"), "-o", str(exe)], check=True)
    seen = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True,
                                                    text=True).stdout.strip().splitlines())
    assert int(seen.pop("size")) == C.sizeof(A)
    assert set(seen) == {f for f, _ in A._fields_} and len(seen) == 29
    for f, _ in A._fields_:
        assert int(seen[f]) == getattr(A, f).offset, f
    # status codes
    a = A()
    assert L.lidf_refine_loss_f32(None, None) == -1 and L.lidf_refine_loss_backward_f32(None, None) == -1
    assert L.lidf_refine_loss_f32(C.byref(a), None) == 0           # no ray: nothing to do
    assert L.lidf_refine_loss_backward_f32(C.byref(a), None) == 0
    a.n_rays = 5
    assert L.lidf_refine_loss_f32(C.byref(a), None) == -1          # NULL inputs
    assert L.lidf_refine_loss_backward_f32(C.byref(a), None) == -1
    a.n_rays = -1
    assert L.lidf_refine_loss_f32(C.byref(a), None) == -1
    a.n_rays, a.batch, a.height, a.width = 1, 1 << 16, 1 << 16, 1 << 16
    assert L.lidf_refine_loss_f32(C.byref(a), None) == -2          # more pixels than an int32 index reaches
    assert L.lidf_refine_loss_workspace_bytes(0) == 0
    assert L.lidf_refine_loss_workspace_bytes(600) == 3 * 9 * 8     # three partial sums of nine doubles
    assert b"workspace" in L.lidf_strerror(-3)
