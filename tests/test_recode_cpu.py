"""qf_recode_batch without a device: the symbol is exported, the Python mirror
checks every buffer before the library sees a pointer, and RecodeShape is the
header's qf_recode_shape.  CPU only."""
import ctypes
import re

import pytest

from quicfuscate_amd import _lib as L


def test_recode_symbol_is_exported():
    lib = L._lib()
    assert "qf_recode_batch" in L.header_symbols()
    assert hasattr(lib, "qf_recode_batch")
    assert "qf_recode_batch" in L._SIGS


def test_recode_shape_matches_the_header():
    txt = re.sub(r"/\*.*?\*/", " ", L.HEADER.read_text(), flags=re.S)
    m = re.search(r"typedef struct qf_recode_shape\s*\{(.*?)\}\s*qf_recode_shape\s*;", txt, flags=re.S)
    assert m, "qf_recode_shape is not declared in qf_fec.h"
    ctype = {"uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64}
    fields = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ty, names = decl.split(None, 1)
        fields += [(n.strip(), ctype[ty]) for n in names.split(",")]
    assert [f[0] for f in fields] == ["k", "r", "L", "max_rows", "m", "flags", "row_stride", "rows_gen_stride",
                                      "out_row_stride", "out_gen_stride"]
    assert list(L.RecodeShape._fields_) == fields
    # six u32 then four u64: no padding
    assert ctypes.sizeof(L.RecodeShape) == 6 * 4 + 4 * 8
    assert L.RecodeShape.row_stride.offset == 24


def test_recode_bad_shapes_fail_before_any_device_work():
    """Call-level errors need no context state: a NULL context or shape is
    QF_EINVAL (the shape checks themselves run on the GPU suite)."""
    lib = L._lib()
    sh = L.RecodeShape(4, 0, 16, 4, 2, 0, 16, 64, 16, 32)
    assert lib.qf_recode_batch(None, ctypes.byref(sh), 1, None, None, None, None, None, 0, None, None,
                               None) == L.QF_EINVAL


def test_mirror_rejects_undersized_recode_buffers():
    import torch

    from quicfuscate_amd import fec

    k, n, m, Lb, G = 16, 12, 5, 100, 3
    rs = 112
    rows = torch.zeros(G * n * rs, dtype=torch.uint8)
    idx = torch.zeros(G * n, dtype=torch.int16)
    out = torch.zeros(G * m * rs, dtype=torch.uint8)
    oc = torch.zeros(G * m * k, dtype=torch.uint8)
    st = torch.zeros(G, dtype=torch.int32)
    kw = dict(max_rows=n, row_stride=rs, rows_gen_stride=n * rs, out_row_stride=rs, out_gen_stride=m * rs, G=G)

    def call(rows=rows, idx=idx, out=out, oc=oc, st=st, **extra):
        fec.recode_batch(rows, idx, out, oc, st, k, m, Lb, **kw, **extra)

    # the last row needs only L of its stride
    need_rows = (G - 1) * n * rs + (n - 1) * rs + Lb
    with pytest.raises(ValueError, match="rows"):
        call(rows=rows[: need_rows - 1])
    with pytest.raises(ValueError, match="row_index"):
        call(idx=idx[:-1])
    with pytest.raises(ValueError, match="out:"):
        call(out=out[: (G - 1) * m * rs + (m - 1) * rs + Lb - 1])
    with pytest.raises(ValueError, match="out_coeffs"):
        call(oc=oc[:-1])
    with pytest.raises(ValueError, match="status"):
        call(st=st[:-1])
    with pytest.raises(ValueError, match="n_rows"):
        call(n_rows=torch.zeros(G - 1, dtype=torch.int32))
    with pytest.raises(ValueError, match="row_coeffs"):
        call(row_coeffs=torch.zeros(G * n * k - 1, dtype=torch.uint8))
    with pytest.raises(ValueError, match="mix"):
        call(mix=torch.zeros(G * m * n - 1, dtype=torch.uint8))
