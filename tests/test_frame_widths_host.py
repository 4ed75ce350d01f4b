"""CPU: the argument checks of lidf_frame_widths_f32 (the frame with decoders of gf_dim 32 / 64 / 128) and of
lidf_decoder_chain_f32's table alignment — every one of them precedes the first HIP call, so they run without a GPU —
and the ctypes mirror of LidfFrameWidths against gcc's view of include/lidf_hip.h."""
import ctypes as C
import os
import subprocess

from util import ROOT

BAD, UNSUP, WS = -1, -2, -3
FAKE = 0x10000   # a 16-byte aligned address no check dereferences


def _fake_decoder(_lib, ief):
    d = _lib.LidfDecoder()
    for field, _ in d._fields_[:10 if ief else 8]:
        setattr(d, field, FAKE)
    d.is_ief, d.n_iter = (1, 2) if ief else (0, 1)
    return d


def _frame_args(_lib, keep):
    """A LidfFrameArgs that passes every check in front of the any-width ones: sizes of a 1 x 24 x 32 frame, every
    device pointer the fake address."""
    L = _lib.lib()
    a = _lib.LidfFrameArgs()
    for field, typ in a._fields_:
        if typ is C.c_void_p and field not in ("miss_mask", "aux_stream", "ev_fork", "ev_join", "valid_idx_bid",
                                               "valid_idx_flat", "packed_query", "packed_refine"):
            setattr(a, field, FAKE)
    a.batch, a.height, a.width = 1, 24, 32
    a.res = (C.c_int32 * 3)(9, 9, 9)
    a.part_size, a.valid_stride, a.max_pairs = 0.25, 1, 32 * 24 * 32
    a.multires, a.multires_views, a.roi_inp_bbox = 8, 4, 8
    a.refine_times, a.pack_mode = 2, 1
    prob, off, offr = _fake_decoder(_lib, False), _fake_decoder(_lib, True), _fake_decoder(_lib, True)
    pn, pnr = _lib.LidfPointNet(), _lib.LidfPointNet()
    keep += [prob, off, offr, pn, pnr]
    a.prob, a.off, a.off_refine = C.pointer(prob), C.pointer(off), C.pointer(offr)
    a.pnet, a.pnet_refine = C.pointer(pn), C.pointer(pnr)
    a.workspace_bytes = L.lidf_frame_workspace_bytes(1, 24, 32, a.res, a.max_pairs, 0, 2)
    a.pack_blob_bytes = L.lidf_frame_pack_bytes()
    return a


def _widths(_lib, a, gfs=(32, 128, 64), slab=0):
    L = _lib.lib()
    wd = _lib.LidfFrameWidths()
    wd.prob_gf, wd.off_gf, wd.refine_gf = gfs
    wd.pe_slab_pairs = slab
    wd.workspace = wd.pack_blob = wd.pack_guard = FAKE
    wd.workspace_bytes = L.lidf_frame_widths_workspace_bytes(1, 24, 32, a.res, a.max_pairs, a.refine_times,
                                                             a.multires, a.multires_views, C.byref(wd))
    wd.pack_blob_bytes = L.lidf_frame_widths_pack_bytes(a.multires, a.multires_views, C.byref(wd))
    return wd


def test_frame_widths_argument_errors_without_gpu():
    from implicit_depth_amd import _lib
    L = _lib.lib()
    keep = []
    a = _frame_args(_lib, keep)
    assert L.lidf_frame_widths_f32(C.byref(a), None, None) == BAD
    assert L.lidf_frame_widths_f32(None, C.byref(_widths(_lib, a)), None) == BAD
    assert L.lidf_frame_widths_f32(C.byref(a), C.byref(_widths(_lib, a, (48, 32, 32))), None) == UNSUP
    assert L.lidf_frame_widths_f32(C.byref(a), C.byref(_widths(_lib, a, (32, 32, 16))), None) == UNSUP
    wd = _widths(_lib, a)
    assert wd.workspace_bytes > 0 and wd.pack_blob_bytes > 0
    for field in ("workspace_bytes", "pack_blob_bytes"):          # each buffer of LidfFrameWidths one byte short
        wd = _widths(_lib, a)
        setattr(wd, field, getattr(wd, field) - 1)
        assert L.lidf_frame_widths_f32(C.byref(a), C.byref(wd), None) == WS, field
    for field in ("workspace_bytes", "pack_blob_bytes"):          # ... and each of LidfFrameArgs
        b = _frame_args(_lib, keep)
        setattr(b, field, getattr(b, field) - 1)
        assert L.lidf_frame_widths_f32(C.byref(b), C.byref(_widths(_lib, b)), None) == WS, field
    wd = _widths(_lib, a)
    wd.pack_guard = None
    assert L.lidf_frame_widths_f32(C.byref(a), C.byref(wd), None) == WS
    # what is built for the shipped widths alone
    for field, value in (("precision", 1), ("offsets_selected", 1), ("aux_stream", FAKE)):
        b = _frame_args(_lib, keep)
        setattr(b, field, value)
        assert L.lidf_frame_widths_f32(C.byref(b), C.byref(_widths(_lib, b)), None) == UNSUP, field
    # the size functions refuse what the entry refuses
    res = (C.c_int32 * 3)(9, 9, 9)
    bad = _widths(_lib, a)
    bad.prob_gf = 48
    assert L.lidf_frame_widths_workspace_bytes(1, 24, 32, res, 1000, 2, 8, 4, C.byref(bad)) == 0
    assert L.lidf_frame_widths_pack_bytes(8, 4, C.byref(bad)) == 0
    assert L.lidf_frame_widths_workspace_bytes(1, 24, 32, res, 1000, 2, 8, 4, None) == 0
    assert L.lidf_frame_widths_pack_guard_bytes() >= 3 * L.lidf_pack_guard_bytes()
    # a larger slab of embedding rows is a larger workspace, bounded by max_pairs
    small, large = _widths(_lib, a, slab=1000), _widths(_lib, a, slab=2000)
    assert abs(large.workspace_bytes - small.workspace_bytes - 1000 * 2 * 51 * 4) < 256   # (256-byte slots)
    assert _widths(_lib, a, slab=10 ** 9).workspace_bytes == _widths(_lib, a, slab=a.max_pairs).workspace_bytes


def test_decoder_chain_refuses_misaligned_tables_without_gpu():
    """lidf_decoder_chain_f32 loads voxpart / raypart rows as aligned 16-byte pieces."""
    from implicit_depth_amd import _lib
    L = _lib.lib()
    d = _fake_decoder(_lib, True)
    wsb = L.lidf_decoder_chain_workspace_bytes(32, 102)

    def call(voxpart, raypart):
        return L.lidf_decoder_chain_f32(C.byref(d), 32, 385, FAKE, 102, 102, 256, 10, voxpart, FAKE, raypart, FAKE,
                                        FAKE, 0, FAKE, wsb, None)
    assert call(FAKE + 4, FAKE) == BAD
    assert call(FAKE, FAKE + 8) == BAD
    assert call(FAKE + 4, None) == BAD
    # (an aligned call is not made here: with a device present it would launch on the fake addresses)


def test_frame_widths_struct_matches_header(tmp_path):
    """The ctypes mirror of LidfFrameWidths against the C compiler's view of include/lidf_hip.h."""
    from implicit_depth_amd import _lib
    cls = _lib.LidfFrameWidths
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "lidf_hip.h"', 'int main(void){',
             'printf("size %zu\\n", sizeof(LidfFrameWidths));', 'printf("abi %d\\n", LIDF_ABI_VERSION);',
             'printf("slab %d\\n", LIDF_FRAME_PE_SLAB);']
    for f, _ in cls._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(LidfFrameWidths, %s));' % (f, f))
    lines.append("return 0;}")
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    seen = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True,
                                                    text=True).stdout.strip().splitlines())
    assert int(seen["size"]) == C.sizeof(cls)
    for f, _ in cls._fields_:
        assert int(seen[f]) == getattr(cls, f).offset, f
    assert int(seen["abi"]) == _lib.ABI == 14
    from implicit_depth_amd import generic
    assert int(seen["slab"]) == generic.QUERY_SLAB
