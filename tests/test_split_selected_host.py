"""CPU, through ctypes: lidf_query_f32 takes precision f16x3 together with offsets_selected (the refusal stood in front
of every HIP call, so its absence shows without a GPU), still refuses more than 8 octaves at f16x3, and the mode costs
no workspace: the list launch's tile counter lives in the 256-byte counter slot the query workspace already had."""
import ctypes as C

OK, BAD, UNSUP = 0, -1, -2
FAKE = 0x10000   # a 16-byte aligned address no check dereferences


def _fake_decoder(_lib, ief):
    d = _lib.LidfDecoder()
    for field, _ in d._fields_[:10 if ief else 8]:
        setattr(d, field, FAKE)
    d.is_ief, d.n_iter = (1, 2) if ief else (0, 1)
    return d


def _query_args(_lib, keep, multires=8, precision=1, selected=1):
    q = _lib.LidfQueryArgs()
    prob, off = _fake_decoder(_lib, False), _fake_decoder(_lib, True)
    keep += [prob, off]
    q.prob, q.off = C.pointer(prob), C.pointer(off)
    q.multires, q.multires_views, q.roi_inp_bbox = multires, 4, 8
    q.n_rays = q.n_pairs = q.n_vox = 0
    q.precision, q.offsets_selected = precision, selected
    return q


def test_query_takes_f16x3_with_selected_offsets():
    from implicit_depth_amd import _lib
    L = _lib.lib()
    keep = []
    # no rays: LIDF_OK from the early exit behind the model checks, before any HIP call
    assert L.lidf_query_f32(C.byref(_query_args(_lib, keep)), None) == OK
    for precision, selected in ((0, 0), (0, 1), (1, 0)):            # (the three combinations that existed)
        assert L.lidf_query_f32(C.byref(_query_args(_lib, keep, precision=precision, selected=selected)), None) == OK
    # the split-f16 kernel is built for up to 8 octaves, in this mode as in the other
    assert L.lidf_query_f32(C.byref(_query_args(_lib, keep, multires=9)), None) == UNSUP
    assert L.lidf_query_f32(C.byref(_query_args(_lib, keep, multires=9, selected=0)), None) == UNSUP
    assert L.lidf_query_f32(C.byref(_query_args(_lib, keep, multires=9, precision=0)), None) == OK
    assert L.lidf_query_f32(C.byref(_query_args(_lib, keep, precision=2)), None) == BAD


def test_workspace_sizes_are_the_parents():
    """The literals are what the library of the commit before this mode answered (built from that commit's sources,
    the two functions called through ctypes with exactly these arguments): R = 1,961 rays and V = 729 voxels without a
    box-sum image, the headline R = 76,800 with the 1 x 32 x 240 x 320 image; the 1 x 24 x 32 and the 2 x 240 x 320
    frame on the 9^3 grid at 32 pairs per pixel and two refine iterations."""
    from implicit_depth_amd import _lib
    L = _lib.lib()
    assert L.lidf_query_workspace_bytes(1961, 729, 0) == 8877568
    assert L.lidf_query_workspace_bytes(76800, 729, 32 * 240 * 320) == 242633984
    res = (C.c_int32 * 3)(9, 9, 9)
    assert L.lidf_frame_workspace_bytes(1, 24, 32, res, 32 * 24 * 32, 0, 2) == 11230464
    assert L.lidf_frame_workspace_bytes(2, 240, 320, res, 32 * 2 * 240 * 320, 0, 2) == 940102144


def test_abi_version_stays_14():
    """No new symbol and no struct change: the header and the binding still say 14."""
    import os
    import re
    from util import ROOT
    from implicit_depth_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "lidf_hip.h")).read()
    assert re.search(r"#define LIDF_ABI_VERSION 14\b", hdr) and _lib.ABI == 14
