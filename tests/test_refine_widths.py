"""Stage-2 training at other widths, the parts that need no GPU: the conditioned reference scenes of
tests/refine_widths_ref.py, the two per-ray entries' declarations, bindings and argument checks (every refusal comes
before the first HIP call), and lidf_refine_train's new parameters."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

import refine_widths_ref as rw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("cfg", rw.CONFIGS + [rw.SHIPPED], ids=rw.cfg_id)
def test_conditioned_scenes_keep_their_caps(cfg):
    """Conditioning drops at most 15 % of the rays and 5 % of the valid points (asserted by conditioned()), and the
    float64 and float32 chains end in the same voxels, in both iterations."""
    for pos_rel, pnet_pos_rel in rw.SETTINGS:
        case, keep_ray, keep_valid, _ = rw.conditioned(cfg, pos_rel, pnet_pos_rel)
        assert int(keep_ray.sum()) >= (1 - rw.RAY_CAP) * keep_ray.numel()
        assert int(keep_valid.sum()) >= (1 - rw.VALID_CAP) * keep_valid.numel()
        with torch.no_grad():
            _, e64 = rw.chain(case, torch.float64, 2, pos_rel, pnet_pos_rel)
            _, e32 = rw.chain(case, torch.float32, 2, pos_rel, pnet_pos_rel)
        assert all(torch.equal(a, b) for a, b in zip(e64, e32))


def test_entries_are_declared_and_bound():
    from implicit_depth_amd import _lib
    with open(os.path.join(ROOT, "include", "lidf_hip.h")) as f:
        header = f.read()
    assert re.search(r"#define LIDF_ABI_VERSION 14\b", header)
    L = _lib.lib()
    for name in ("lidf_refine_step_workspace_bytes", "lidf_refine_step_forward_f32", "lidf_refine_step_backward_f32"):
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SIGNATURES and getattr(L, name) is not None


def test_refine_step_entries_check_arguments_without_gpu():
    from implicit_depth_amd import _lib
    L = _lib.lib()
    BAD, UNSUPPORTED, WORKSPACE = -1, -2, -3
    null = C.c_void_p(None)
    some = C.c_void_p(4096)     # a non-NULL, 16-byte aligned address that is never dereferenced by a refused call
    res, xmin = (C.c_int32 * 3)(9, 9, 9), (C.c_float * 3)(-1.125, -1.125, -0.125)

    def fwd(pos=some, mid=some, pv=some, P=7, vb=some, vbid=some, V=5, rbid=some, rflat=some, rgb=some, B=2, h=4, w=6,
            R=3, Nv=10, L_=8, coord=null, gres=null, gxmin=null, part=0.25, ev=some, pn=some, pnv=some, pe=some,
            ld=51, ws=null, wsb=0):
        return L.lidf_refine_step_forward_f32(pos, mid, pv, P, vb, vbid, V, rbid, rflat, rgb, B, h, w, R, Nv, 1, 0, L_,
                                              coord, gres, gxmin, part, 0, ev, pn, pnv, pe, ld, ws, wsb, null)

    for kw in (dict(R=-1), dict(P=-1), dict(V=-1), dict(Nv=-1), dict(L_=-1), dict(L_=17), dict(V=0), dict(B=0),
               dict(h=0), dict(w=-3), dict(ld=50), dict(pos=null), dict(mid=null), dict(pv=null), dict(vb=null),
               dict(vbid=null), dict(rbid=null), dict(rflat=null), dict(rgb=null), dict(ev=null), dict(pn=null),
               dict(pnv=null), dict(pe=null), dict(pe=C.c_void_p(4098)), dict(pos=C.c_void_p(4097)),
               dict(coord=some), dict(coord=some, gres=res), dict(coord=some, gres=res, gxmin=xmin, part=0.0),
               dict(coord=some, gres=(C.c_int32 * 3)(9, 0, 9), gxmin=xmin)):
        assert fwd(**kw) == BAD, kw
    assert fwd(R=0, pos=null, pe=null, V=0) == 0                        # no ray: nothing to launch
    assert fwd(L_=0, ld=2) == BAD and fwd(R=0x15555555, Nv=1) == UNSUPPORTED
    grid = dict(coord=some, gres=res, gxmin=xmin)
    assert fwd(**grid) == WORKSPACE and fwd(ws=some, wsb=4 * 2 * 729 - 1, **grid) == WORKSPACE
    assert fwd(gres=(C.c_int32 * 3)(2048, 2048, 2048), coord=some, gxmin=xmin, ws=some, wsb=1 << 40) == UNSUPPORTED
    assert L.lidf_refine_step_workspace_bytes(2, res) == 4 * 2 * 729
    assert L.lidf_refine_step_workspace_bytes(0, res) == 0 and L.lidf_refine_step_workspace_bytes(2, null) == 0
    assert L.lidf_refine_step_workspace_bytes(2, (C.c_int32 * 3)(9, -1, 9)) == 0

    def bwd(g=some, d=some, d_off=some, pos=some, ev=some, vb=some, rel=1, d_pe=some, L_=8, rows=some, d_pos=some, R=3):
        return L.lidf_refine_step_backward_f32(g, d, -0.2, 0.2, d_off, pos, ev, vb, rel, d_pe, L_, rows, d_pos, R, null)

    for kw in (dict(R=-1), dict(L_=-1), dict(L_=17), dict(g=null), dict(d=null), dict(pos=null), dict(ev=null),
               dict(vb=null)):
        assert bwd(**kw) == BAD, kw
    assert bwd(R=0, g=null) == 0 and bwd(d_off=null, d_pos=null, g=null) == 0     # no ray / no output: no launch
    assert bwd(R=0x15555556) == UNSUPPORTED


def test_lidf_refine_train_has_the_new_parameters():
    from implicit_depth_amd import generic
    from implicit_depth_amd.query import lidf_refine_train
    p = inspect.signature(lidf_refine_train).parameters
    assert p["roi_out_bbox"].default == 2 and p["factorised"].default is None
    g = inspect.signature(generic.refine_train).parameters
    assert set(p) - {"factorised"} == set(g)          # the same arguments as the any-width route behind it
