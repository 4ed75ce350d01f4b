"""The split-f16 decoder chain's entry points as the binding sees them, without a GPU: the ABI number stays, the two
symbols are declared and bound, a stale library is named, and the size function refuses other widths."""
import ctypes as C
import os
import re
import subprocess

import pytest

from util import ROOT

NEW = ("lidf_decoder_chain_split_workspace_bytes", "lidf_decoder_chain_split_f32")


def test_header_keeps_abi_14_and_declares_the_entries():
    from implicit_depth_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "lidf_hip.h")).read()
    assert re.search(r"#define LIDF_ABI_VERSION 14\b", hdr) and _lib.ABI == 14
    assert "size_t lidf_decoder_chain_split_workspace_bytes(int32_t gf_dim, int32_t k);" in hdr
    assert re.search(r"\bint lidf_decoder_chain_split_f32\(const LidfDecoder\* dec, int32_t gf_dim, int32_t inp_dim,", hdr)
    # the accuracy contract is stated where the entry is declared
    block = hdr[hdr.index("split-f16 precision"):hdr.index("int lidf_decoder_chain_split_f32(")]
    assert "2^-22" in block and "65504" in block and "stays f32" in block


def test_signatures_mirror_the_f32_entry():
    from implicit_depth_amd import _lib
    for name in NEW:
        assert name in _lib.SIGNATURES
    assert _lib.SIGNATURES[NEW[0]] == _lib.SIGNATURES["lidf_decoder_chain_workspace_bytes"]
    assert _lib.SIGNATURES[NEW[1]] == _lib.SIGNATURES["lidf_decoder_chain_f32"]


def test_stale_library_message(tmp_path, monkeypatch):
    """An ABI-14 library from before this entry answers the right version, has every other symbol and lacks these:
    lib() names the missing one and asks for a rebuild."""
    from implicit_depth_amd import _lib
    src = tmp_path / "old.c"
    body = ["int lidf_version(void) { return 14; }"]
    body += ["int %s(void) { return 0; }" % n for n in _lib.SIGNATURES if n not in NEW and n != "lidf_version"]
    src.write_text("\n".join(body) + "\n")
    so = tmp_path / "libold.so"
    subprocess.run(["gcc", "-shared", "-fPIC", "-o", str(so), str(src)], check=True)
    monkeypatch.setattr(_lib, "LIB_PATH", str(so))
    monkeypatch.setattr(_lib, "_lib", None)
    with pytest.raises(RuntimeError, match="lacks lidf_decoder_chain_split.*rebuild the library"):
        _lib.lib()


def test_workspace_bytes_and_refusals_before_any_hip_call():
    from implicit_depth_amd import _lib
    L = _lib.lib()
    assert L.lidf_version() == 14
    for gf in (0, 16, 48, 96, 256):
        assert L.lidf_decoder_chain_split_workspace_bytes(gf, 102) == 0
    assert L.lidf_decoder_chain_split_workspace_bytes(64, 0) == 0
    for gf in (32, 64, 128):
        G, kp = gf // 16, ((102 + 15) // 16 + 1) // 2
        raw = (2 * G + 3) // 4 + 8 * G * G + G + (G + 3) // 4 + 2 * G * G
        nb = L.lidf_decoder_chain_split_workspace_bytes(gf, 102)
        # 4 bytes per weight as in the f32 stream: layer 1 in pairs of 16-column groups (two 1 KiB quads per pair and
        # output tile), the pass section padded to at most 16 quads, then w4 | b4
        assert (kp * 8 * G + raw) * 1024 + (gf + 1) * 4 <= nb <= (kp * 8 * G + raw + 16) * 1024 + 4096
    # host buffers stand in for device memory: none of these calls may reach a kernel launch
    buf = (C.c_char * 4096)()
    p = C.cast(buf, C.c_void_p)
    dec = _lib.LidfDecoder()
    for f, _ in dec._fields_:
        if f in ("w1", "b1", "w2", "b2", "w3", "b3", "w4", "b4"):
            setattr(dec, f, p)
    # (the same error codes as the f32 entry: taken from it)
    BAD = -1
    UNSUPPORTED = L.lidf_decoder_chain_f32(C.byref(dec), 48, 20, p, 20, 20, 0, 4, p, None, None, None, p, 0, p, 4096, None)
    WORKSPACE = L.lidf_decoder_chain_f32(C.byref(dec), 32, 20, p, 20, 20, 0, 4, p, None, None, None, p, 0, p, 16, None)

    def call(gf=32, inp=20, ldx=20, k=20, c0=0, n=4, vox=p, vidx=None, ray=None, ridx=None, out=p, ws=p, wsb=16):
        return L.lidf_decoder_chain_split_f32(C.byref(dec), gf, inp, p, ldx, k, c0, n, vox, vidx, ray, ridx, out, 0,
                                              ws, wsb, None)
    assert call(gf=48) == UNSUPPORTED != 0 and call(gf=256) == UNSUPPORTED
    assert call(k=0) == BAD and call(ldx=19) == BAD and call(c0=1) == BAD and call(n=-1) == BAD
    assert call(vox=C.c_void_p(p.value + 4)) == BAD                      # the tables are read as aligned 16-byte pieces
    assert call(vox=None, vidx=p) == BAD and call(ridx=p) == BAD
    assert call(out=None) == BAD
    assert call() == WORKSPACE != 0 and call(ws=None) == WORKSPACE       # too small a workspace: refused, not launched
    assert call(n=0) == 0
