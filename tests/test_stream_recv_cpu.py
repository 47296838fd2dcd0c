"""The streaming receive step without a device: qf_rank_state_bytes,
qf_rank_update_batch and qf_store_append_dev are exported, declared and bound,
StoreShape is the header's qf_store_shape, the state size keeps its promises, a
NULL context or shape and every bad shape field fail before any device work,
the Python mirrors check every buffer, and the seeded traffic of
tests/test_gpu_stream_recv.py holds, on the reference side, the cases those
tests are about.  CPU only."""
import ctypes
import re

import numpy as np
import pytest

from quicfuscate_amd import _lib as L
from tests import rank_ref, store_ref

NAMES = ("qf_rank_state_bytes", "qf_rank_update_batch", "qf_store_append_dev")
E = L.QF_EINVAL


@pytest.mark.parametrize("name", NAMES)
def test_symbols_are_exported(name):
    lib = L._lib()
    assert name in L.header_symbols()
    assert hasattr(lib, name)
    assert name in L._SIGS


def test_store_shape_matches_the_header():
    txt = re.sub(r"/\*.*?\*/", " ", L.HEADER.read_text(), flags=re.S)
    m = re.search(r"typedef struct qf_store_shape\s*\{(.*?)\}\s*qf_store_shape\s*;", txt, flags=re.S)
    assert m, "qf_store_shape is not declared in qf_fec.h"
    ctype = {"uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64}
    fields = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ty, names = decl.split(None, 1)
        fields += [(n.strip(), ctype[ty]) for n in names.split(",")]
    assert [f[0] for f in fields] == ["k", "L", "max_rows", "cap", "flags", "reserved", "src_gen_stride",
                                      "store_row_stride", "store_gen_stride"]
    assert list(L.StoreShape._fields_) == fields
    assert ctypes.sizeof(L.StoreShape) == 6 * 4 + 3 * 8 == 48


@pytest.mark.parametrize("name,count", [("qf_rank_update_batch", 10), ("qf_store_append_dev", 17)])
def test_signatures_have_the_header_argument_count(name, count):
    txt = re.sub(r"/\*.*?\*/", " ", L.HEADER.read_text(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", txt, flags=re.S)
    assert m
    assert len(L._SIGS[name][1]) == len(m.group(1).split(",")) == count


def test_rank_state_bytes():
    from quicfuscate_amd import fec

    assert fec.rank_state_bytes(0) == 0 and fec.rank_state_bytes(257) == 0 and fec.rank_state_bytes(1 << 20) == 0
    prev = 0
    for k in range(1, 257):
        b = fec.rank_state_bytes(k)
        assert b > 0 and b % 16 == 0, k
        assert b >= prev, k
        prev = b
        # what k_rank_filter holds in LDS without its exp / log tables, plus a 16-byte header
        kc, kp = (k + 15) // 16 * 16, (k + 7) // 8 * 8 + 4
        lds = 768 + 10 * kc + k * kp
        assert b <= lds - 768 + 16, (k, b, lds)
        # at least the basis itself: k rows of k bytes
        assert b >= k * k, k
    # smaller than that bound, not just within it: pivrow, first, lfac, stage and later are not stored
    assert fec.rank_state_bytes(64) <= 64 * 64 + 64 + 48


def _fake_ctx():
    buf = ctypes.create_string_buffer(64)
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def test_rank_update_null_context_shape_and_bad_fields():
    lib = L._lib()
    keep, ctx = _fake_ctx()
    nulls = [None] * 7
    sh = L.RankShape(8, 0, 4, 0)
    assert lib.qf_rank_update_batch(None, ctypes.byref(sh), 1, *nulls) == E
    assert lib.qf_rank_update_batch(ctx, None, 1, *nulls) == E
    # the shape is checked before the context is touched
    for bad in (L.RankShape(0, 0, 4, 0), L.RankShape(257, 0, 4, 0), L.RankShape(8, 0, 0, 0),
                L.RankShape(8, 0, 4097, 0), L.RankShape(8, 0, 4, 1)):
        assert lib.qf_rank_update_batch(ctx, ctypes.byref(bad), 1, *nulls) == E
    rng_ = L.RankShape(200, 57, 4, 0)                       # Cauchy rows of (k, r) with k + r > 256
    assert lib.qf_rank_update_batch(ctx, ctypes.byref(rng_), 1, *nulls) == L.QF_ERANGE
    assert lib.qf_rank_update_batch(ctx, ctypes.byref(sh), 0, *nulls) == L.QF_OK      # G == 0
    # required pointers (row_index, state, rank, status), and the state's alignment
    b = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(b) + 15) // 16 * 16
    args = dict(idx=p, n=None, co=None, state=p + 256, fl=None, rk=p + 2048, st=p + 2304)
    order = ("idx", "n", "co", "state", "fl", "rk", "st")
    for nm in ("idx", "state", "rk", "st"):
        a = [None if o == nm else args[o] for o in order]
        assert lib.qf_rank_update_batch(ctx, ctypes.byref(sh), 1, *a) == E, nm
    a = [args[o] + (8 if o == "state" else 0) if args[o] else None for o in order]
    assert lib.qf_rank_update_batch(ctx, ctypes.byref(sh), 1, *a) == E
    del keep


def test_store_append_null_context_shape_and_bad_fields():
    lib = L._lib()
    keep, ctx = _fake_ctx()
    nulls = [None] * 14

    def status(k=8, Lb=100, mr=6, cap=8, flags=0, reserved=0, sgs=6 * 128, rs=112, gs=8 * 112, G=1, handle=ctx,
               shape=True):
        sh = L.StoreShape(k, Lb, mr, cap, flags, reserved, sgs, rs, gs)
        return lib.qf_store_append_dev(handle, ctypes.byref(sh) if shape else None, G, *nulls)

    assert status(G=0) == L.QF_OK                            # a good shape: nothing else is looked at
    assert status() == E                                     # ... and with G = 1 the NULL pointers are
    assert status(handle=None, G=0) == E and status(shape=False, G=0) == E
    assert status(k=0, G=0) == E and status(k=257, G=0) == E and status(k=256, G=0) == L.QF_OK
    assert status(Lb=0, G=0) == E
    assert status(mr=0, G=0) == E and status(mr=1025, G=0) == E and status(mr=1024, G=0) == L.QF_OK
    assert status(cap=0, G=0) == E and status(cap=1025, G=0) == E
    assert status(cap=1024, gs=1024 * 112, G=0) == L.QF_OK
    assert status(flags=1, G=0) == E and status(reserved=1, G=0) == E
    assert status(sgs=6 * 128 + 8, G=0) == E
    assert status(rs=104, G=0) == E                          # not a multiple of 16
    assert status(rs=96, G=0) == E                           # below round_up(L, 16)
    assert status(Lb=112, G=0) == L.QF_OK and status(Lb=113, G=0) == E
    assert status(gs=8 * 112 + 8, G=0) == E and status(gs=8 * 112 - 16, G=0) == E
    assert status(gs=8 * 112 + 16, G=0) == L.QF_OK
    # cap * store_row_stride above 2^32: the offsets are u32
    big = 1 << 23
    assert status(cap=512, rs=big, gs=512 * big, G=0) == L.QF_OK
    assert status(cap=512, rs=big + 16, gs=512 * (big + 16), G=0) == E
    del keep


def test_mirrors_reject_undersized_buffers():
    import torch

    from quicfuscate_amd import fec

    k, mr, cap, Lb, G = 8, 6, 8, 100, 3
    sb = fec.rank_state_bytes(k)
    u8 = lambda n: torch.zeros(n, dtype=torch.uint8)          # noqa: E731
    i32 = lambda n: torch.zeros(n, dtype=torch.int32)         # noqa: E731
    i16 = lambda n: torch.zeros(n, dtype=torch.int16)         # noqa: E731
    idx, state, rank, st = i16(G * mr), u8(G * sb), i32(G), i32(G)

    def upd(idx=idx, state=state, rank=rank, st=st, **extra):
        fec.rank_update_batch(idx, state, rank, st, k, max_rows=mr, G=G, **extra)

    for what, kw in (("row_index", dict(idx=idx[:-1])), ("state", dict(state=state[:-1])), ("rank", dict(rank=rank[:-1])),
                     ("status", dict(st=st[:-1])), ("n_rows", dict(n_rows=i32(G - 1))),
                     ("row_coeffs", dict(row_coeffs=u8(G * mr * k - 1))), ("innovative", dict(innovative=u8(G * mr - 1)))):
        with pytest.raises(ValueError, match=what):
            upd(**kw)
    rs, fs = 112, 128
    b = dict(src=u8(G * mr * fs), ro=i32(G * mr), rl=i32(G * mr), idx=idx, co=u8(G * mr * k), store=u8(G * cap * rs),
             so=i32(G * cap), sl=i32(G * cap), si=i16(G * cap), sc=u8(G * cap * k), sn=i32(G), st=st)
    names = dict(src="src", ro="row_off", rl="row_len", idx="row_index", co="row_coeffs", store="store:", so="store_off",
                 sl="store_len", si="store_index", sc="store_coeffs", sn="store_n", st="status")

    def app(**kw):
        a = {**b, **{key: v for key, v in kw.items() if key in b}}
        extra = {key: v for key, v in kw.items() if key not in b}
        fec.store_append(a["src"], a["ro"], a["rl"], a["idx"], a["co"], a["store"], a["so"], a["sl"], a["si"], a["sc"],
                         a["sn"], a["st"], k, Lb, max_rows=mr, cap=cap, src_gen_stride=mr * fs, store_row_stride=rs,
                         store_gen_stride=cap * rs, G=G, **extra)

    for key, what in names.items():
        with pytest.raises(ValueError, match=what):
            app(**{key: b[key][:-1]})
    with pytest.raises(ValueError, match="n_rows"):
        app(n_rows=i32(G - 1))
    with pytest.raises(ValueError, match="take"):
        app(take=u8(G * mr - 1))


def test_store_reference_appends_and_refuses():
    k, Lb, mr, cap, G = 4, 20, 4, 3, 4
    sgs = mr * 48
    src = np.arange(G * sgs, dtype=np.uint32).astype(np.uint8).reshape(G, sgs)
    off = np.tile(np.arange(mr, dtype=np.uint32) * 48, (G, 1))
    ln = np.tile(np.array([20, 0, 17, 1], np.uint32), (G, 1))
    idx = np.tile(np.array([0, k, 2, k], np.uint16), (G, 1))
    co = np.arange(G * mr * k, dtype=np.uint32).astype(np.uint8).reshape(G, mr, k)
    take = np.array([[1, 0, 1, 1], [1, 1, 1, 1], [1, 0, 0, 0], [0, 0, 0, 0]], np.uint8)
    ln[2, 0] = 21                                            # longer than L, and taken
    s = store_ref.Store(G, k, Lb, cap)
    st = s.append(src, sgs, off, ln, idx, co, None, take)
    assert st.tolist() == [store_ref.OK, store_ref.ETOOSMALL, store_ref.EINVAL, store_ref.OK]
    assert s.n.tolist() == [3, 0, 0, 0]
    assert (s.bytes[1:] == store_ref.FILL).all()
    rs = s.row_stride
    assert s.off[0].tolist() == [0, rs, 2 * rs] and s.len[0].tolist() == [20, 17, 1] and s.index[0].tolist() == [0, 2, k]
    assert np.array_equal(s.bytes[0, :20], src[0, :20]) and not s.bytes[0, 20:32].any()
    assert (s.bytes[0, 32:rs] == store_ref.FILL).all()
    assert np.array_equal(s.bytes[0, rs: rs + 17], src[0, 96: 113]) and not s.bytes[0, rs + 17: rs + 32].any()
    assert s.bytes[0, 2 * rs] == src[0, 144] and not s.bytes[0, 2 * rs + 1: 2 * rs + 16].any()
    assert np.array_equal(s.coeffs[0], co[0, [0, 2, 3]])
    # a second append goes behind the first; the count stops it at cap
    st = s.append(src, sgs, off, ln, idx, co, np.array([1, 1, 1, 5], np.uint32), None)
    assert st.tolist() == [store_ref.ETOOSMALL, store_ref.OK, store_ref.EINVAL, store_ref.EINVAL]
    assert s.n.tolist() == [3, 1, 0, 0]


def test_seeded_traffic_holds_the_cases_the_device_tests_are_about(oracle):
    for k in store_ref.STREAM_K:
        case = store_ref.stream_case(k)
        for g in range(case["G"]):
            # the reference agrees with the library's host rule
            from quicfuscate_amd import fec
            V = store_ref.vectors_of(k, case["idx"][g], case["co"][g])
            rk, fl = fec.gf_rank(V, k)
            assert rk == case["rank"][g] and fl == case["flags"][g].tolist(), (k, g)
        for j, split in enumerate(case["splits"]):
            late_dependent = spanned_unit = full_early = 0
            idle = 0
            for g in range(case["G"]):
                idx, co, flags, pl = case["idx"][g], case["co"][g], case["flags"][g], case["plant"][g]
                counts = split[g]
                assert sum(counts) == len(idx) and len(counts) == store_ref.STREAM_CALLS
                idle += sum(1 for c in counts if c == 0)
                call_of = np.repeat(np.arange(len(counts)), counts)
                first_call = int(call_of[0])
                late_dependent += sum(1 for s in range(len(idx)) if idx[s] >= k and not flags[s] and co[s].any()
                                      and call_of[s] > first_call)
                # source b as a systematic row: not received before, spanned by the
                # earlier rows (the pair e_a + x e_b and source a among them) in any
                # elimination order, with room left in the span, in a later call
                sb = pl["sys_b"]
                V = store_ref.vectors_of(k, idx, co)
                before = rank_ref.innovative(V[:sb])[1]
                with_b = rank_ref.innovative(np.vstack([V[:sb], V[sb: sb + 1]]))[1]
                if (idx[sb] == pl["b"] and not flags[sb] and pl["b"] not in idx[:sb].tolist() and before < k
                        and with_b == before and call_of[sb] > call_of[pl["pair"]]):
                    spanned_unit += 1
                k_at = int(np.flatnonzero(np.cumsum(flags) == k)[0]) if case["rank"][g] == k else None
                if k_at is not None and call_of[k_at] < call_of[-1]:
                    full_early += 1
            assert late_dependent and spanned_unit and full_early, (k, j, late_dependent, spanned_unit, full_early)
            assert idle, (k, j, "no generation is idle in any call")
