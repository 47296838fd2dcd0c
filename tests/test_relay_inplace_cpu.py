"""The in-place relay step without a device: qf_parse_frame_headers_dev and
qf_recode_frames_dev are exported, declared and bound, RecodeFramesShape is the
header's qf_recode_frames_shape, a NULL context fails before any device work,
and the Python mirrors check every buffer before the library sees a pointer.
CPU only."""
import ctypes
import re

import pytest

from quicfuscate_amd import _lib as L

SYMBOLS = ("qf_parse_frame_headers_dev", "qf_recode_frames_dev")


@pytest.mark.parametrize("name", SYMBOLS)
def test_relay_inplace_symbols_are_exported(name):
    lib = L._lib()
    assert name in L.header_symbols()
    assert hasattr(lib, name)
    assert name in L._SIGS


def test_recode_frames_shape_matches_the_header():
    txt = re.sub(r"/\*.*?\*/", " ", L.HEADER.read_text(), flags=re.S)
    m = re.search(r"typedef struct qf_recode_frames_shape\s*\{(.*?)\}\s*qf_recode_frames_shape\s*;", txt, flags=re.S)
    assert m, "qf_recode_frames_shape is not declared in qf_fec.h"
    ctype = {"uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64}
    fields = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ty, names = decl.split(None, 1)
        fields += [(n.strip(), ctype[ty]) for n in names.split(",")]
    assert [f[0] for f in fields] == ["k", "L", "max_rows", "m", "flags", "reserved", "src_gen_stride",
                                      "out_row_stride", "out_gen_stride"]
    assert list(L.RecodeFramesShape._fields_) == fields
    # six u32 then three u64: no padding
    assert ctypes.sizeof(L.RecodeFramesShape) == 6 * 4 + 3 * 8 == 48
    assert L.RecodeFramesShape.src_gen_stride.offset == 24


def test_signatures_have_the_header_argument_counts():
    txt = re.sub(r"/\*.*?\*/", " ", L.HEADER.read_text(), flags=re.S)
    for name in SYMBOLS:
        m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", txt, flags=re.S)
        assert m, name
        assert len(L._SIGS[name][1]) == len(m.group(1).split(",")), name


def test_null_context_fails_before_any_device_work():
    lib = L._lib()
    assert lib.qf_parse_frame_headers_dev(None, 4, 16, 1, 4, None, 32, None, None, None, None, None, None, None,
                                          None, None, None) == L.QF_EINVAL
    sh = L.RecodeFramesShape(4, 16, 4, 2, 0, 0, 128, 16, 32)
    assert lib.qf_recode_frames_dev(None, ctypes.byref(sh), 1, None, None, None, None, None, None, None, 0, None,
                                    None, None, None) == L.QF_EINVAL


def test_mirror_rejects_undersized_recode_frames_buffers():
    import torch

    from quicfuscate_amd import fec

    k, n, m, Lb, G = 16, 5, 3, 100, 3
    fs, ors = 144, 112
    src = torch.zeros(G * n * fs, dtype=torch.uint8)
    off = torch.zeros(G * n, dtype=torch.int32)
    ln = torch.zeros(G * n, dtype=torch.int32)
    idx = torch.zeros(G * n, dtype=torch.int16)
    co = torch.zeros(G * n * k, dtype=torch.uint8)
    out = torch.zeros(G * m * ors, dtype=torch.uint8)
    oc = torch.zeros(G * m * k, dtype=torch.uint8)
    st = torch.zeros(G, dtype=torch.int32)
    kw = dict(max_rows=n, src_gen_stride=n * fs, out_row_stride=ors, out_gen_stride=m * ors, G=G)

    def call(src=src, off=off, ln=ln, idx=idx, co=co, out=out, oc=oc, st=st, **extra):
        fec.recode_frames(src, off, ln, idx, co, out, oc, st, k, m, Lb, **kw, **extra)

    with pytest.raises(ValueError, match="src"):
        call(src=src[:-1])
    with pytest.raises(ValueError, match="row_off"):
        call(off=off[:-1])
    with pytest.raises(ValueError, match="row_len"):
        call(ln=ln[:-1])
    with pytest.raises(ValueError, match="row_index"):
        call(idx=idx[:-1])
    with pytest.raises(ValueError, match="row_coeffs"):
        call(co=co[:-1])
    # the last output row needs only L of its stride
    with pytest.raises(ValueError, match="out:"):
        call(out=out[: (G * m - 1) * ors + Lb - 1])
    with pytest.raises(ValueError, match="out_coeffs"):
        call(oc=oc[:-1])
    with pytest.raises(ValueError, match="status"):
        call(st=st[:-1])
    with pytest.raises(ValueError, match="out_len"):
        call(out_len=torch.zeros(G * m - 1, dtype=torch.int32))
    with pytest.raises(ValueError, match="n_rows"):
        call(n_rows=torch.zeros(G - 1, dtype=torch.int32))
    with pytest.raises(ValueError, match="mix"):
        call(mix=torch.zeros(G * m * n - 1, dtype=torch.uint8))


def test_mirror_rejects_undersized_parse_frame_headers_buffers():
    import torch

    from quicfuscate_amd import fec

    k, n, Lb, G = 16, 5, 100, 3
    fs = 144
    frames = torch.zeros(G * n * fs, dtype=torch.uint8)
    flen = torch.zeros(G * n, dtype=torch.int32)
    ids = torch.zeros(G * n, dtype=torch.int64)
    idx = torch.zeros(G * n, dtype=torch.int16)
    nr = torch.zeros(G, dtype=torch.int32)
    st = torch.zeros(G * n, dtype=torch.int32)
    co = torch.zeros(G * n * k, dtype=torch.uint8)
    rl = torch.zeros(G * n, dtype=torch.int32)
    ro = torch.zeros(G * n, dtype=torch.int32)
    kw = dict(max_rows=n, frame_stride=fs, G=G)

    def call(frames=frames, flen=flen, ids=ids, idx=idx, nr=nr, st=st, co=co, rl=rl, ro=ro, **extra):
        fec.parse_frame_headers(frames, flen, ids, idx, nr, st, co, rl, ro, k, Lb, **kw, **extra)

    with pytest.raises(ValueError, match="frames"):
        call(frames=frames[:-1])
    with pytest.raises(ValueError, match="frame_len"):
        call(flen=flen[:-1])
    with pytest.raises(ValueError, match="ids"):
        call(ids=ids[:-1])
    with pytest.raises(ValueError, match="row_index"):
        call(idx=idx[:-1])
    with pytest.raises(ValueError, match="n_rows"):
        call(nr=nr[:-1])
    with pytest.raises(ValueError, match="frame_status"):
        call(st=st[:-1])
    with pytest.raises(ValueError, match="row_coeffs"):
        call(co=co[:-1])
    with pytest.raises(ValueError, match="row_len"):
        call(rl=rl[:-1])
    with pytest.raises(ValueError, match="row_off"):
        call(ro=ro[:-1])
    with pytest.raises(ValueError, match="n_frames"):
        call(n_frames=torch.zeros(G - 1, dtype=torch.int32))
    with pytest.raises(ValueError, match="frame_off"):
        call(frame_off=torch.zeros(G * n - 1, dtype=torch.int32))
