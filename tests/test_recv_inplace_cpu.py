"""The in-place receive step without a device: qf_decode_frames_dev is
exported, declared and bound, DecodeFramesShape is the header's
qf_decode_frames_shape, a NULL context or shape fails before any device work,
the Python mirror checks every buffer before the library sees a pointer, and
the reference the device tests compare with (tests/recv_ref.py) agrees with
tests/rank_ref.py and the oracle's decode on the planted arrival orders.
CPU only."""
import ctypes
import re

import numpy as np
import pytest

from quicfuscate_amd import _lib as L
from tests import rank_ref, recv_ref

NAME = "qf_decode_frames_dev"


def test_decode_frames_symbol_is_exported():
    lib = L._lib()
    assert NAME in L.header_symbols()
    assert hasattr(lib, NAME)
    assert NAME in L._SIGS


def test_decode_frames_shape_matches_the_header():
    txt = re.sub(r"/\*.*?\*/", " ", L.HEADER.read_text(), flags=re.S)
    m = re.search(r"typedef struct qf_decode_frames_shape\s*\{(.*?)\}\s*qf_decode_frames_shape\s*;", txt, flags=re.S)
    assert m, "qf_decode_frames_shape is not declared in qf_fec.h"
    ctype = {"uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64}
    fields = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ty, names = decl.split(None, 1)
        fields += [(n.strip(), ctype[ty]) for n in names.split(",")]
    assert [f[0] for f in fields] == ["k", "r", "L", "max_rows", "flags", "reserved", "src_gen_stride",
                                      "rec_row_stride", "rec_gen_stride"]
    assert list(L.DecodeFramesShape._fields_) == fields
    # six u32 then three u64: no padding
    assert ctypes.sizeof(L.DecodeFramesShape) == 6 * 4 + 3 * 8 == 48
    offs = [getattr(L.DecodeFramesShape, f[0]).offset for f in fields]
    assert offs == [0, 4, 8, 12, 16, 20, 24, 32, 40]


def test_signature_has_the_header_argument_count():
    txt = re.sub(r"/\*.*?\*/", " ", L.HEADER.read_text(), flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\((.*?)\)\s*;", txt, flags=re.S)
    assert m
    assert len(L._SIGS[NAME][1]) == len(m.group(1).split(",")) == 16


def test_null_context_or_shape_fails_before_any_device_work():
    lib = L._lib()
    sh = L.DecodeFramesShape(4, 4, 16, 4, 0, 0, 128, 16, 64)
    nulls = [None] * 13
    assert lib.qf_decode_frames_dev(None, ctypes.byref(sh), 1, *nulls) == L.QF_EINVAL
    # any non-NULL context pointer: the shape is checked before the context is touched
    fake = ctypes.create_string_buffer(64)
    assert lib.qf_decode_frames_dev(ctypes.cast(fake, ctypes.c_void_p), None, 1, *nulls) == L.QF_EINVAL


def test_mirror_rejects_undersized_decode_frames_buffers():
    import torch

    from quicfuscate_amd import fec

    k, r, n, Lb, G = 16, 6, 20, 100, 3
    fs, rrs = 144, 112
    src = torch.zeros(G * n * fs, dtype=torch.uint8)
    off = torch.zeros(G * n, dtype=torch.int32)
    ln = torch.zeros(G * n, dtype=torch.int32)
    idx = torch.zeros(G * n, dtype=torch.int16)
    co = torch.zeros(G * n * k, dtype=torch.uint8)
    rec = torch.zeros(G * r * rrs, dtype=torch.uint8)
    ri = torch.zeros(G * r, dtype=torch.int16)
    nrec = torch.zeros(G, dtype=torch.int32)
    st = torch.zeros(G, dtype=torch.int32)
    kw = dict(max_rows=n, src_gen_stride=n * fs, rec_row_stride=rrs, rec_gen_stride=r * rrs, G=G)

    def call(src=src, off=off, ln=ln, idx=idx, co=co, rec=rec, ri=ri, nrec=nrec, st=st, **extra):
        fec.decode_frames(src, off, ln, idx, co, rec, ri, nrec, st, k, r, Lb, **kw, **extra)

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
    # the last recovered row needs only L of its stride
    with pytest.raises(ValueError, match="rec:"):
        call(rec=rec[: (G * r - 1) * rrs + Lb - 1])
    with pytest.raises(ValueError, match="rec_index"):
        call(ri=ri[:-1])
    with pytest.raises(ValueError, match="n_rec"):
        call(nrec=nrec[:-1])
    with pytest.raises(ValueError, match="status"):
        call(st=st[:-1])
    with pytest.raises(ValueError, match="n_rows"):
        call(n_rows=torch.zeros(G - 1, dtype=torch.int32))
    with pytest.raises(ValueError, match="rank"):
        call(rank=torch.zeros(G - 1, dtype=torch.int32))
    with pytest.raises(ValueError, match="innovative"):
        call(innovative=torch.zeros(G * n - 1, dtype=torch.uint8))
    with pytest.raises(ValueError, match="src_slot"):
        call(src_slot=torch.zeros(G * k - 1, dtype=torch.int16))


def test_reference_on_the_planted_arrival_orders(oracle):
    """recv_ref.decode_ref (zero-padded rows, innovative filter, decode,
    src_slot) against rank_ref and the oracle's decode over the compacted rows."""
    k, Lb = 16, 100
    names, src, idx, co, V, rows = recv_ref.plant(oracle, np.random.default_rng(77), k, Lb)
    assert len(names) >= 6
    short = 0
    for g, name in enumerate(names):
        lens = [recv_ref.trimmed_len(rows[g, s]) if s % 3 else Lb for s in range(24)]
        short += sum(1 for x in lens if x < Lb)
        pay = [rows[g, s, : lens[s]].tobytes() for s in range(24)]
        ref = recv_ref.decode_ref(oracle, k, k, Lb, idx[g], co[g], pay)
        flags, rank = rank_ref.innovative(V[g])
        assert ref["status"] == recv_ref.OK and ref["rank"] == rank == k, name
        assert np.array_equal(ref["flags"], flags), name
        keep = np.flatnonzero(flags)
        have = {int(idx[g, s]): int(s) for s in keep if idx[g, s] < k}
        assert ref["erased"] == [i for i in range(k) if i not in have], name
        assert np.array_equal(ref["rec"], src[g][ref["erased"]]), name
        for i in range(k):
            assert ref["src_slot"][i] == have.get(i, recv_ref.NONE16), (name, i)
            if i in have:
                # the accepted systematic row is the source, at its own length
                assert pay[have[i]] == src[g, i, : lens[have[i]]].tobytes()
                assert not src[g, i, lens[have[i]]:].any()
        st, dec, _ = oracle.decode(k, idx[g][keep], rows[g][keep], co[g][keep])
        assert st == 0 and np.array_equal(dec, src[g]), name
    assert short > 20, "no frame carries fewer than L bytes"
    by = dict(zip(names, range(len(names))))
    g = by["duplicated systematic index"]
    pay = [rows[g, s].tobytes() for s in range(24)]
    assert recv_ref.decode_ref(oracle, k, k, Lb, idx[g], co[g], pay)["src_slot"][6] == 2     # slot 11 repeats it
    g = by["e2 + e7, then systematic 2, then systematic 7"]
    ref = recv_ref.decode_ref(oracle, k, k, Lb, idx[g], co[g], [rows[g, s].tobytes() for s in range(24)])
    assert ref["src_slot"][2] == 1 and ref["src_slot"][7] == recv_ref.NONE16 and 7 in ref["erased"]


def test_reference_statuses(oracle):
    k, Lb = 4, 8
    rng = np.random.default_rng(4)
    co = rng.integers(1, 256, (6, k), dtype=np.uint8)
    pay = [bytes(Lb)] * 6
    # rank short of k
    assert recv_ref.decode_ref(oracle, k, k, Lb, [0, 1, 0, 1], co[:4], pay[:4])["status"] == recv_ref.ENOTREADY
    assert recv_ref.decode_ref(oracle, k, k, Lb, [], co[:0], [])["status"] == recv_ref.ENOTREADY
    # a coded index with index - k >= 256
    assert recv_ref.decode_ref(oracle, k, k, Lb, [0, 1, 2, k + 256], co[:4], pay[:4])["status"] == recv_ref.EINVAL
    # more erased sources than min(k, r)
    ref = recv_ref.decode_ref(oracle, k, 1, Lb, [k, k + 1, 0, 1], co[:4], pay[:4])
    assert ref["status"] == recv_ref.EINVAL and ref["rank"] == k
