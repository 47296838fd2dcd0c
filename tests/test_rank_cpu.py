"""The innovative-row rule without a device: the new symbols are exported,
RankShape is the header's qf_rank_shape, qf_gf256_rank equals the numpy
reference (tests/rank_ref.py), and the Python mirrors check every buffer before
the library sees a pointer.  CPU only."""
import ctypes
import re

import numpy as np
import pytest

from quicfuscate_amd import _lib as L
from tests import rank_ref

NEW_SYMBOLS = ["qf_gf256_rank", "qf_rank_batch", "qf_decode_innovative_batch", "qf_decoder_set_innovative",
               "qf_decoder_rank"]


@pytest.mark.parametrize("name", NEW_SYMBOLS)
def test_rank_symbols_are_exported(name):
    lib = L._lib()
    assert name in L.header_symbols()
    assert hasattr(lib, name)
    assert name in L._SIGS


def test_rank_shape_matches_the_header():
    txt = re.sub(r"/\*.*?\*/", " ", L.HEADER.read_text(), flags=re.S)
    m = re.search(r"typedef struct qf_rank_shape\s*\{(.*?)\}\s*qf_rank_shape\s*;", txt, flags=re.S)
    assert m, "qf_rank_shape is not declared in qf_fec.h"
    fields = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ty, names = decl.split(None, 1)
        assert ty == "uint32_t"
        fields += [(n.strip(), ctypes.c_uint32) for n in names.split(",")]
    assert [f[0] for f in fields] == ["k", "r", "max_rows", "flags"]
    assert list(L.RankShape._fields_) == fields
    assert ctypes.sizeof(L.RankShape) == 16


def planted_cases(rng, k=16):
    """name -> (n x k) vectors: the arrival orders the device tests plant
    (tests/test_gpu_rank.py builds its generations from the same function)."""
    def unit(i):
        v = np.zeros(k, np.uint8)
        v[i] = 1
        return v

    def rnd(n):
        return rng.integers(1, 256, (n, k), dtype=np.uint8)

    from tests import oracle_py

    def comb(a, va, b, vb):
        return (oracle_py.encode(np.stack([va, vb]), 1, np.array([[a, b]], np.uint8))[0]).astype(np.uint8)

    cases = {}
    V = rnd(24)
    V[9] = comb(0x53, V[1], 0xCA, V[3])
    cases["combination of slots 1 and 3"] = V
    V = rnd(24)
    V[4] = 0
    cases["zero vector"] = V
    V = rnd(24)
    V[2], V[11] = unit(6), unit(6)
    cases["duplicated systematic index"] = V
    V = rnd(24)
    V[0] = unit(2) ^ unit(7)
    V[1], V[2] = unit(2), unit(7)
    cases["e2 + e7, then systematic 2, then systematic 7"] = V
    V = rnd(24)
    V[0, :5] = 0
    V[1] = unit(5)
    cases["coded row with its first nonzero at column 5, then systematic 5"] = V
    V = rnd(24)
    # rank 16 reached at slot 19: slots 5, 8, 12, 17 repeat or combine earlier ones
    V[5] = V[0]
    V[8] = comb(2, V[1], 3, V[7])
    V[12] = 0
    V[17] = comb(9, V[16], 1, V[2])
    cases["rank k at slot 19, four rows behind it"] = V
    return cases


def _lib_rank(V):
    V = np.ascontiguousarray(V, np.uint8)
    n, k = V.shape
    flags = np.full(n + 8, 0x77, np.uint8)
    rank = ctypes.c_uint32(12345)
    s = L._lib().qf_gf256_rank(k, n, V.ctypes.data, flags.ctypes.data, ctypes.byref(rank))
    assert s == L.QF_OK
    assert (flags[n:] == 0x77).all()
    return flags[:n], int(rank.value)


def test_gf256_rank_equals_the_reference_on_random_matrices(oracle):
    rng = np.random.default_rng(2024)
    ks = [1, 5, 16, 64, 100, 255]
    count = dependent = 0
    while count < 200:
        k = ks[count % len(ks)]
        n = [1, k - 1, k, k + 9][(count // len(ks)) % 4]
        count += 1
        if n == 0:
            n = 1
        # entries from {0, 0, 1, random}: dependencies occur
        pick = rng.integers(0, 4, (n, k))
        V = np.where(pick < 2, 0, np.where(pick == 2, 1, rng.integers(0, 256, (n, k)))).astype(np.uint8)
        want_flags, want_rank = rank_ref.innovative(V)
        flags, rank = _lib_rank(V)
        assert rank == want_rank and np.array_equal(flags, want_flags), (k, n, count)
        dependent += int(want_rank < min(n, k))
    assert dependent >= 10, "the random matrices held no dependent rows"


def test_gf256_rank_equals_the_reference_on_the_planted_cases(oracle):
    for name, V in planted_cases(np.random.default_rng(77)).items():
        want_flags, want_rank = rank_ref.innovative(V)
        flags, rank = _lib_rank(V)
        assert rank == want_rank and np.array_equal(flags, want_flags), name
    cases = planted_cases(np.random.default_rng(77))
    f, r = rank_ref.innovative(cases["e2 + e7, then systematic 2, then systematic 7"])
    assert list(f[:3]) == [1, 1, 0]
    f, r = rank_ref.innovative(cases["coded row with its first nonzero at column 5, then systematic 5"])
    assert list(f[:2]) == [1, 1]
    f, r = rank_ref.innovative(cases["rank k at slot 19, four rows behind it"])
    assert r == 16 and f[19] == 1 and not f[20:].any() and f[:20].sum() == 16


def test_gf256_rank_without_flags_and_bad_arguments():
    lib = L._lib()
    V = np.eye(4, dtype=np.uint8)
    rank = ctypes.c_uint32(0)
    assert lib.qf_gf256_rank(4, 4, V.ctypes.data, None, ctypes.byref(rank)) == L.QF_OK and rank.value == 4
    assert lib.qf_gf256_rank(4, 0, None, None, ctypes.byref(rank)) == L.QF_OK and rank.value == 0
    assert lib.qf_gf256_rank(0, 4, V.ctypes.data, None, ctypes.byref(rank)) == L.QF_EINVAL
    assert lib.qf_gf256_rank(4, 4, None, None, ctypes.byref(rank)) == L.QF_EINVAL
    assert lib.qf_gf256_rank(4, 4, V.ctypes.data, None, None) == L.QF_EINVAL


def test_mirror_gf_rank(oracle):
    from quicfuscate_amd import fec

    V = planted_cases(np.random.default_rng(5))["duplicated systematic index"]
    want_flags, want_rank = rank_ref.innovative(V)
    rank, flags = fec.gf_rank(V, 16)
    assert rank == want_rank and flags == want_flags.tolist()
    assert fec.gf_rank(V.tobytes(), 16) == (rank, flags)
    with pytest.raises(ValueError):
        fec.gf_rank(b"\1\2\3", 2)


def test_rank_calls_with_null_context_or_shape():
    """Call-level errors need no context state (the shape checks themselves run
    on the GPU suite)."""
    lib = L._lib()
    rs = L.RankShape(4, 0, 4, 0)
    ds = L.DecodeShape(4, 2, 16, 4, 16, 64, 16, 32)
    assert lib.qf_rank_batch(None, ctypes.byref(rs), 1, None, None, None, None, None, None) == L.QF_EINVAL
    assert lib.qf_decode_innovative_batch(None, ctypes.byref(ds), 1, None, None, None, None, None, None, None, None,
                                          None, None) == L.QF_EINVAL
    assert lib.qf_decoder_set_innovative(None, 1) == L.QF_EINVAL
    assert lib.qf_decoder_rank(None) == L.QF_EINVAL


def test_mirrors_reject_undersized_buffers():
    import torch

    from quicfuscate_amd import fec

    k, r, n, Lb, G = 16, 8, 20, 100, 3
    rs = 112
    em = min(k, r)
    rows = torch.zeros(G * n * rs, dtype=torch.uint8)
    idx = torch.zeros(G * n, dtype=torch.int16)
    rec = torch.zeros(G * em * rs, dtype=torch.uint8)
    ri = torch.zeros(G * em, dtype=torch.int16)
    nrec = torch.zeros(G, dtype=torch.int32)
    st = torch.zeros(G, dtype=torch.int32)
    rank = torch.zeros(G, dtype=torch.int32)

    def call_rank(idx=idx, rank=rank, st=st, **extra):
        fec.rank_batch(idx, rank, st, k, r=r, max_rows=n, G=G, **extra)

    with pytest.raises(ValueError, match="row_index"):
        call_rank(idx=idx[:-1])
    with pytest.raises(ValueError, match="rank"):
        call_rank(rank=rank[:-1])
    with pytest.raises(ValueError, match="status"):
        call_rank(st=st[:-1])
    with pytest.raises(ValueError, match="n_rows"):
        call_rank(n_rows=torch.zeros(G - 1, dtype=torch.int32))
    with pytest.raises(ValueError, match="row_coeffs"):
        call_rank(row_coeffs=torch.zeros(G * n * k - 1, dtype=torch.uint8))
    with pytest.raises(ValueError, match="innovative"):
        call_rank(innovative=torch.zeros(G * n - 1, dtype=torch.uint8))

    kw = dict(max_rows=n, row_stride=rs, rows_gen_stride=n * rs, rec_row_stride=rs, rec_gen_stride=em * rs, G=G)

    def call_dec(rows=rows, idx=idx, rec=rec, ri=ri, nrec=nrec, st=st, **extra):
        fec.decode_innovative_batch(rows, idx, rec, ri, nrec, st, k, r, Lb, **kw, **extra)

    need_rows = (G - 1) * n * rs + (n - 1) * rs + Lb
    with pytest.raises(ValueError, match="rows"):
        call_dec(rows=rows[: need_rows - 1])
    with pytest.raises(ValueError, match="row_index"):
        call_dec(idx=idx[:-1])
    with pytest.raises(ValueError, match="rec:"):
        call_dec(rec=rec[: (G - 1) * em * rs + (em - 1) * rs + Lb - 1])
    with pytest.raises(ValueError, match="rec_index"):
        call_dec(ri=ri[:-1])
    with pytest.raises(ValueError, match="n_rec"):
        call_dec(nrec=nrec[:-1])
    with pytest.raises(ValueError, match="status"):
        call_dec(st=st[:-1])
    with pytest.raises(ValueError, match="row_coeffs"):
        call_dec(row_coeffs=torch.zeros(G * n * k - 1, dtype=torch.uint8))
    with pytest.raises(ValueError, match="rank"):
        call_dec(rank=rank[:-1])
    with pytest.raises(ValueError, match="innovative"):
        call_dec(innovative=torch.zeros(G * n - 1, dtype=torch.uint8))
