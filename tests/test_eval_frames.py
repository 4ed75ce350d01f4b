"""CPU: the per-frame evaluation losses without a GPU. frame_slice gives back the frames a batch was joined from; the
torch-op composites with per_frame=True follow the float64 restatement frame by frame (NaN positions included, a frame
without a ray all NaN); 'train' and hard_neg are refused with the reason; the binding names the new entries and asks
for a rebuild when the library lacks them; the C-ABI argument errors (checked before any HIP call)."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

import eval_frames as ef
import eval_loss_ref as el
from test_eval_loss_gpu import _product_dd
from util import ROOT

NEW = ("lidf_depth_metrics_frames_workspace_bytes", "lidf_depth_metrics_frames_f32",
       "lidf_stage1_eval_loss_frames_workspace_bytes", "lidf_refine_eval_loss_frames_workspace_bytes",
       "lidf_stage1_eval_loss_frames_f32", "lidf_refine_eval_loss_frames_f32")


def _batches():
    fa, opt_a, _ = ef.batch_a()
    fb, opt_b = ef.batch_b()
    return (("A", fa, opt_a), ("B", fb, opt_b))


def test_the_special_frames_of_batch_a_are_what_they_claim():
    frames, opt, ref = ef.batch_a()
    # the float64 restatement reproduces the fixture's vectors of the reference's own run with g12 d's options
    for stage, want in ((1, ref["loss"]), (2, ref["loss_refine"])):
        got = el.vector(el.eval_loss_ref(frames[1], torch.float64, stage, 0, **opt), stage)
        assert ((got - want.double()).abs() <= 2e-7 * want.double().abs()).all(), (stage, got, want)
    for stage in (1, 2):
        keys = el.EVAL_LOSS_KEYS if stage == 1 else el.REFINE_EVAL_LOSS_KEYS
        zero = el.eval_loss_ref(frames[3], torch.float64, stage, 0, **opt)
        assert int(zero["count"]) == 0 and float(zero["err"]) == 0.0
        assert {k for k in keys if torch.isnan(zero[k])} == set(el.METRIC_KEYS)
        unl = el.eval_loss_ref(frames[4], torch.float64, stage, 0, **opt)
        assert {k for k in keys if torch.isnan(unl[k])} == ({"prob_loss", "loss_net"} if stage == 1 else set())


def test_frame_slice_gives_back_the_frames_a_batch_was_joined_from():
    from implicit_depth_amd import frame_slice
    for name, frames, _ in _batches():
        dd = _product_dd(ef.concat_frames(frames), "cpu")
        for b, d in enumerate(frames):
            want, got = _product_dd(d, "cpu"), frame_slice(dd, b)
            for k, v in want.items():
                if not torch.is_tensor(v):
                    assert got[k] == v, (name, b, k)
                elif k == "corrupt_mask":
                    assert torch.equal(got[k], v.reshape(1, d["h"], d["w"]).float()), (name, b, k)
                else:
                    assert got[k].dtype == v.dtype and got[k].shape == v.shape and torch.equal(got[k], v), (name, b, k)
    with pytest.raises(IndexError):
        frame_slice(dd, 3)


def _composite_dd(d, dt):
    dd = {k: d[k] for k in ("bs", "h", "w", "pair_ray", "pcl_label", "corrupt_mask")}
    for k in ("xyz_flat", "xyz_corrupt_flat", "gt_pos", "pred_pos", "pred_prob_end", "pred_pos_refine"):
        dd[k] = d[k].to(dt)
    dd["miss_bid"], dd["miss_flat_img_id"] = d["miss_bid"], d["miss_flat"]
    return dd


@pytest.mark.parametrize("stage", (1, 2))
def test_composites_per_frame_follow_the_float64_restatement(stage):
    from implicit_depth_amd import LidfLossOptions, lidf_loss_composite, refine_loss_composite
    fn = lidf_loss_composite if stage == 1 else refine_loss_composite
    keys = el.EVAL_LOSS_KEYS if stage == 1 else el.REFINE_EVAL_LOSS_KEYS
    for name, frames, opt in _batches():
        # (the pairs of a joined batch lie frame by frame, inside a frame in the reference's voxel-major order)
        out = fn(_composite_dd(ef.concat_frames(frames), torch.float64), LidfLossOptions(**opt), "test", 0,
                 per_frame=True)
        assert tuple(out) == keys
        for k in keys:
            assert out[k].shape == (len(frames),) and out[k].dtype == torch.float64 and not out[k].requires_grad
        for b, d in enumerate(frames):
            if d["miss_bid"].shape[0] == 0:
                assert all(torch.isnan(out[k][b]) for k in keys), (name, b)
                continue
            want = el.eval_loss_ref(d, torch.float64, stage, 0, **opt)
            for k in keys:
                if torch.isnan(want[k]):
                    assert torch.isnan(out[k][b]), (name, b, k)
                else:   # (test_eval_loss.py's bound for the composite against the restatement in float64)
                    assert abs(float(out[k][b]) - float(want[k])) <= 1e-11 * max(abs(float(want[k])), 1e-3), (name, b, k)
    assert torch.isnan(torch.stack([out[k] for k in keys])).sum() == 0   # (batch B has no NaN)


def test_per_frame_refuses_the_training_flavour_and_hard_neg():
    from implicit_depth_amd import (LidfLossOptions, lidf_loss, lidf_loss_composite, refine_loss,
                                    refine_loss_composite)
    from implicit_depth_amd import pipeline as pl
    frames, opt = ef.batch_b()
    dd = _composite_dd(ef.concat_frames(frames), torch.float32)
    hard = LidfLossOptions(hard_neg=True, hard_neg_ratio=0.1)
    for fn in (lidf_loss, refine_loss, lidf_loss_composite, refine_loss_composite):
        with pytest.raises(NotImplementedError, match="no per-frame training loss"):
            fn(dd, None, "train", 0, per_frame=True)
        with pytest.raises(NotImplementedError, match="hard-negative.*frame_slice"):
            fn(dd, hard, "valid", 0, per_frame=True)
    with pytest.raises(NotImplementedError, match="frame_slice"):
        pl.eval_loss(dd, hard, "test", per_frame=True)
    # (without the flag the fused calls get as far as the device check, as before)
    with pytest.raises(RuntimeError, match="CUDA"):
        lidf_loss(dd, hard, "valid", 0)


def test_header_keeps_abi_14_and_declares_the_entries():
    from implicit_depth_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "lidf_hip.h")).read()
    assert re.search(r"#define LIDF_ABI_VERSION 14\b", hdr) and _lib.ABI == 14
    for name in NEW:
        assert re.search(r"\b(size_t|int) %s\(" % name, hdr), name
        assert name in _lib.SIGNATURES
    assert "grouped by frame" in hdr and "unspecified" in hdr and "BIT FOR BIT" in hdr
    S = _lib.SIGNATURES
    assert S["lidf_stage1_eval_loss_frames_f32"] == S["lidf_refine_eval_loss_frames_f32"] == \
        S["lidf_stage1_eval_loss_f32"]
    # the one-frame call's arguments with the batch after seg_dtype
    one, many = S["lidf_depth_metrics_f32"], S["lidf_depth_metrics_frames_f32"]
    assert many[0] == one[0] and len(many[1]) == len(one[1]) + 1


def test_stale_library_message(tmp_path, monkeypatch):
    """An ABI-14 library from before these entries answers the right version, has every other symbol and lacks
    these: lib() names a missing one and asks for a rebuild."""
    from implicit_depth_amd import _lib
    src = tmp_path / "old.c"
    body = ["int lidf_version(void) { return 14; }"]
    body += ["int %s(void) { return 0; }" % n for n in _lib.SIGNATURES if n not in NEW and n != "lidf_version"]
    src.write_text("\n".join(body) + "\n")
    so = tmp_path / "libold.so"
    subprocess.run(["gcc", "-shared", "-fPIC", "-o", str(so), str(src)], check=True)
    monkeypatch.setattr(_lib, "LIB_PATH", str(so))
    monkeypatch.setattr(_lib, "_lib", None)
    with pytest.raises(RuntimeError, match="lacks lidf_(depth_metrics|stage1_eval_loss|refine_eval_loss)_frames.*"
                                           "rebuild the library"):
        _lib.lib()


def test_frames_abi_sizes_and_argument_errors_without_gpu():
    from implicit_depth_amd import _lib
    L = _lib.lib()
    one = L.lidf_depth_metrics_workspace_bytes()
    assert L.lidf_depth_metrics_frames_workspace_bytes(0) == 0 and L.lidf_depth_metrics_frames_workspace_bytes(5) == 5 * one
    # 18 double partial sums (stage 1: 19, the frame's label count) per block of 256 pixels of every frame, the
    # per-frame statistics workspaces, their outputs [B, 10] padded to 64 bytes, two depth images per frame
    for fn, ns in ((L.lidf_stage1_eval_loss_frames_workspace_bytes, 19), (L.lidf_refine_eval_loss_frames_workspace_bytes, 18)):
        assert fn(0, 16, 24) == 0 and fn(3, 0, 24) == 0
        assert fn(5, 16, 24) == 5 * 2 * ns * 8 + 5 * one + 256 + 2 * 5 * 384 * 4
        assert fn(3, 20, 27) == 3 * 3 * ns * 8 + 3 * one + 128 + 2 * 3 * 540 * 4
    buf = (C.c_char * 64)()
    p = C.addressof(buf)
    dm = L.lidf_depth_metrics_frames_f32
    assert dm(None, None, None, 0, 0, 4, 4, 4, 4, None, None, 0, None) == 0           # no frame: nothing to do
    assert dm(p, p, None, 0, -1, 4, 4, 4, 4, p, p, 1 << 20, None) == -1
    assert dm(p, p, None, 0, 2, 0, 4, 4, 4, p, p, 1 << 20, None) == -1
    assert dm(None, p, None, 0, 2, 4, 4, 4, 4, p, p, 1 << 20, None) == -1
    assert dm(p, p, None, 1, 2, 4, 4, 4, 4, p, p, 1 << 20, None) == -1                 # a mask type without a mask
    assert dm(p, p, None, 0, 70000, 4, 4, 4, 4, p, p, 1 << 30, None) == -2
    assert dm(p, p, None, 0, 2, 4, 4, 4, 4, p, p, 2 * one - 1, None) == -3
    assert dm(p, p, None, 0, 2, 4, 4, 4, 4, p, p + 4, 1 << 20, None) == -1             # misaligned

    def args():
        a = _lib.LidfEvalLossArgs()
        a.n_rays, a.n_pairs, a.batch, a.height, a.width = 3, 0, 2, 4, 4
        for k in ("xyz_base", "xyz_gt", "ray_bid", "ray_flat", "pair_off", "pix2ray", "gt_pos", "gt_max_pair_id",
                  "pred_pos", "loss", "workspace"):
            setattr(a, k, p)
        a.workspace_bytes = 1 << 20
        return a
    for fn in (L.lidf_stage1_eval_loss_frames_f32, L.lidf_refine_eval_loss_frames_f32):
        assert fn(None, None) == -1
        assert fn(C.byref(_lib.LidfEvalLossArgs()), None) == 0                          # no frame
        a = args()
        a.xyz_gt = None                                                                 # required: every frame is resized
        assert fn(C.byref(a), None) == -1
        a = args()
        a.seg_dtype = 2                                                                 # a mask type without a mask
        assert fn(C.byref(a), None) == -1
        for k in ("pos_unreduced", "surf_norm_dist", "dx_dist", "dy_dist", "prob_unreduced"):
            a = args()
            setattr(a, k, p)                                                            # no per-frame hard-negative select
            assert fn(C.byref(a), None) == -1, k
        a = args()
        a.loss = None
        assert fn(C.byref(a), None) == -1
        a = args()
        a.workspace_bytes = 64
        assert fn(C.byref(a), None) == -3
        a = args()
        a.workspace = p + 4
        assert fn(C.byref(a), None) == -1
        a = args()
        a.batch = 70000
        assert fn(C.byref(a), None) == -2
    a = args()
    a.pair_off = None                                                                   # stage 2 reads no pair list
    assert L.lidf_stage1_eval_loss_frames_f32(C.byref(a), None) == -1
    a = args()
    assert a.n_label is None                                                            # not read: may stay NULL
    a.n_pairs = 4                                                                       # pairs without labels / logits
    assert L.lidf_stage1_eval_loss_frames_f32(C.byref(a), None) == -1
