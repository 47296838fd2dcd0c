"""Device framing of coded rows without a device: the three symbols are
exported, FrameRowsShape is the header's qf_frame_rows_shape, the payload
offset helper follows its formula, a NULL context fails before any device
work, and the Python mirrors check every buffer before the library sees a
pointer.  CPU only."""
import ctypes
import re

import pytest

from quicfuscate_amd import _lib as L

SYMBOLS = ("qf_frame_payload_offset", "qf_frame_rows_dev", "qf_parse_frames_coded_dev")


@pytest.mark.parametrize("name", SYMBOLS)
def test_wire_coded_symbols_are_exported(name):
    lib = L._lib()
    assert name in L.header_symbols()
    assert hasattr(lib, name)
    assert name in L._SIGS


def test_frame_rows_shape_matches_the_header():
    txt = re.sub(r"/\*.*?\*/", " ", L.HEADER.read_text(), flags=re.S)
    m = re.search(r"typedef struct qf_frame_rows_shape\s*\{(.*?)\}\s*qf_frame_rows_shape\s*;", txt, flags=re.S)
    assert m, "qf_frame_rows_shape is not declared in qf_fec.h"
    ctype = {"uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64}
    fields = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ty, names = decl.split(None, 1)
        fields += [(n.strip(), ctype[ty]) for n in names.split(",")]
    assert [f[0] for f in fields] == ["k", "r", "L", "max_rows", "flags", "reserved", "row_stride",
                                      "rows_gen_stride", "frame_stride"]
    assert list(L.FrameRowsShape._fields_) == fields
    # six u32 then three u64: no padding
    assert ctypes.sizeof(L.FrameRowsShape) == 6 * 4 + 3 * 8 == 48
    assert L.FrameRowsShape.row_stride.offset == 24
    flag = re.search(r"#define\s+QF_FRAME_IN_PLACE\s+(\w+)", txt)
    assert flag and int(flag.group(1).rstrip("uU"), 0) == L.QF_FRAME_IN_PLACE


def test_frame_payload_offset_formula():
    from quicfuscate_amd import fec

    lib = L._lib()
    for k in range(1, 257):
        want = (3 + k + 15) // 16 * 16
        assert lib.qf_frame_payload_offset(k) == want, k
        assert fec.frame_payload_offset(k) == want
        assert want % 16 == 0 and 3 + k <= want < 3 + k + 16
    assert lib.qf_frame_payload_offset(0) == 0
    assert lib.qf_frame_payload_offset(257) == 0
    assert fec.frame_payload_offset(0) == 0 and fec.frame_payload_offset(257) == 0


def test_null_context_fails_before_any_device_work():
    lib = L._lib()
    sh = L.FrameRowsShape(4, 0, 16, 4, 0, 0, 16, 64, 32)
    assert lib.qf_frame_rows_dev(None, ctypes.byref(sh), 1, None, None, None, None, None, None, None,
                                 None) == L.QF_EINVAL
    assert lib.qf_parse_frames_coded_dev(None, 4, 16, 1, 4, None, 32, None, None, None, None, None, 16, 64, None,
                                         None, None, None, None) == L.QF_EINVAL


def test_mirror_rejects_undersized_frame_rows_buffers():
    import torch

    from quicfuscate_amd import fec

    k, n, Lb, G = 16, 5, 100, 3
    rs, P = 112, 32
    fs = P + 112
    rows = torch.zeros(G * n * rs, dtype=torch.uint8)
    frames = torch.zeros(G * n * fs, dtype=torch.uint8)
    flen = torch.zeros(G * n, dtype=torch.int32)
    kw = dict(max_rows=n, row_stride=rs, rows_gen_stride=n * rs, frame_stride=fs, G=G)

    def call(rows=rows, frames=frames, flen=flen, **extra):
        fec.frame_rows(rows, frames, flen, k, Lb, **kw, **extra)

    # the last row needs only L of its stride, the last slot only P + L
    with pytest.raises(ValueError, match="rows"):
        call(rows=rows[: (G * n - 1) * rs + Lb - 1])
    with pytest.raises(ValueError, match="frames"):
        call(frames=frames[: (G * n - 1) * fs + P + Lb - 1])
    with pytest.raises(ValueError, match="frame_len"):
        call(flen=flen[:-1])
    with pytest.raises(ValueError, match="frame_off"):
        call(frame_off=torch.zeros(G * n - 1, dtype=torch.int32))
    with pytest.raises(ValueError, match="row_index"):
        call(row_index=torch.zeros(G * n - 1, dtype=torch.int16))
    with pytest.raises(ValueError, match="n_rows"):
        call(n_rows=torch.zeros(G - 1, dtype=torch.int32))
    with pytest.raises(ValueError, match="row_coeffs"):
        call(row_coeffs=torch.zeros(G * n * k - 1, dtype=torch.uint8))
    with pytest.raises(ValueError, match="row_len"):
        call(row_len=torch.zeros(G * n - 1, dtype=torch.int32))
    # in place the rows are not read: only the frame buffer is checked
    with pytest.raises(ValueError, match="frames"):
        call(rows=None, in_place=True, frames=frames[:-fs])


def test_mirror_rejects_undersized_parse_frames_coded_buffers():
    import torch

    from quicfuscate_amd import fec

    k, n, Lb, G = 16, 5, 100, 3
    rs, fs = 112, 144
    frames = torch.zeros(G * n * fs, dtype=torch.uint8)
    flen = torch.zeros(G * n, dtype=torch.int32)
    ids = torch.zeros(G * n, dtype=torch.int64)
    rows = torch.zeros(G * n * rs, dtype=torch.uint8)
    idx = torch.zeros(G * n, dtype=torch.int16)
    nr = torch.zeros(G, dtype=torch.int32)
    st = torch.zeros(G * n, dtype=torch.int32)
    co = torch.zeros(G * n * k, dtype=torch.uint8)
    kw = dict(max_rows=n, frame_stride=fs, row_stride=rs, rows_gen_stride=n * rs, G=G)

    def call(frames=frames, flen=flen, ids=ids, rows=rows, idx=idx, nr=nr, st=st, co=co, **extra):
        fec.parse_frames_coded(frames, flen, ids, rows, idx, nr, st, co, k, Lb, **kw, **extra)

    with pytest.raises(ValueError, match="frames"):
        call(frames=frames[:-1])
    with pytest.raises(ValueError, match="frame_len"):
        call(flen=flen[:-1])
    with pytest.raises(ValueError, match="ids"):
        call(ids=ids[:-1])
    with pytest.raises(ValueError, match="rows"):
        call(rows=rows[: (G * n - 1) * rs + Lb - 1])
    with pytest.raises(ValueError, match="row_index"):
        call(idx=idx[:-1])
    with pytest.raises(ValueError, match="n_rows"):
        call(nr=nr[:-1])
    with pytest.raises(ValueError, match="frame_status"):
        call(st=st[:-1])
    with pytest.raises(ValueError, match="row_coeffs"):
        call(co=co[:-1])
    with pytest.raises(ValueError, match="n_frames"):
        call(n_frames=torch.zeros(G - 1, dtype=torch.int32))
    with pytest.raises(ValueError, match="frame_off"):
        call(frame_off=torch.zeros(G * n - 1, dtype=torch.int32))
    with pytest.raises(ValueError, match="row_len"):
        call(row_len=torch.zeros(G * n - 1, dtype=torch.int32))
