"""The two any-width training adjoints' argument checks (no GPU: every refusal comes before the first HIP call)."""
import ctypes as C


def test_train_width_entries_check_arguments_without_gpu():
    from implicit_depth_amd import _lib
    L = _lib.lib()
    BAD = -1
    null = C.c_void_p(None)
    some = C.c_void_p(4096)     # a non-NULL, 16-byte aligned address that is never dereferenced by a refused call

    def roi(d_out=some, ld=12, pix=some, bid=some, n=5, B=1, Cn=3, h=8, w=8, inp=8, outb=2, d_feat=some, ws=some,
            wsb=1 << 20):
        return L.lidf_roi_align_backward_f32(d_out, ld, pix, bid, n, B, Cn, h, w, inp, outb, d_feat, ws, wsb, null)

    for kw in (dict(d_out=null), dict(pix=null), dict(bid=null), dict(d_feat=null), dict(n=-1), dict(B=-1),
               dict(Cn=-2), dict(h=-8), dict(w=-8), dict(inp=-1), dict(outb=0), dict(outb=-3), dict(ld=11)):
        assert roi(**kw) == BAD, kw
    assert roi(ws=null) == -3 and roi(wsb=16) == -3          # LIDF_ERR_WORKSPACE
    # an empty gradient: nothing has to be written
    assert roi(B=0) == 0 and roi(Cn=0) == 0 and roi(h=0, n=0, d_feat=null) == 0
    assert L.lidf_roi_align_backward_workspace_bytes(1, 8, 8) >= 3 * 64 * 4
    assert L.lidf_roi_align_backward_workspace_bytes(8, 240, 320) >= 3 * 8 * 240 * 320 * 4
    assert L.lidf_roi_align_backward_workspace_bytes(0, 8, 8) == 0

    def g2(dz=some, n=10, ncols=8, seg=some, n_seg=3, d2=some, idx=some, nv=4, d1=some, ws=null, wsb=0):
        return L.lidf_gather2_backward_f32(dz, n, ncols, seg, n_seg, d2, idx, nv, d1, ws, wsb, null)

    for kw in (dict(dz=null), dict(seg=null), dict(idx=null), dict(n=-1), dict(n_seg=-1), dict(nv=-1), dict(ncols=0),
               dict(ncols=-4), dict(ncols=6), dict(ncols=255), dict(dz=C.c_void_p(4100))):
        assert g2(**kw) == BAD, kw
    # no destination row in either table: nothing has to be written
    assert g2(n_seg=0, nv=0) == 0 and g2(d2=null, d1=null) == 0 and g2(n=0, dz=null, n_seg=0, nv=0) == 0
    assert L.lidf_gather2_backward_workspace_bytes(5000, 1458, 128) > 1458 * 128 * 4
    assert L.lidf_gather2_backward_workspace_bytes(1, 1, 4) > 0
    assert L.lidf_gather2_backward_workspace_bytes(5000, 1458, 6) == 0       # not a multiple of 4
    assert L.lidf_gather2_backward_workspace_bytes(5000, 16385, 128) == 0    # above the sorted form's bound
