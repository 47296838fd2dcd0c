"""The flat-poll ingest without a device: qf_parse_poll_headers_dev,
qf_rank_update_sel_batch and qf_store_append_sel_dev are exported, declared and
bound with the header's argument counts, a NULL context, shape or list and
every bad field fail before any device work, the Python mirrors check every
buffer, tests/poll_ref.py groups a hand-written poll as the header states, and
the seeded polls of tests/test_gpu_poll_ingest.py hold the cases those tests
are about.  CPU only."""
import ctypes
import re

import numpy as np
import pytest

from quicfuscate_amd import _lib as L
from tests import poll_ref as PR
from tests import rank_ref

NAMES = (("qf_parse_poll_headers_dev", 24), ("qf_rank_update_sel_batch", 11), ("qf_store_append_sel_dev", 17))
E = L.QF_EINVAL


@pytest.mark.parametrize("name,count", NAMES)
def test_symbols_are_exported_with_the_header_argument_count(name, count):
    lib = L._lib()
    assert name in L.header_symbols()
    assert hasattr(lib, name)
    assert name in L._SIGS
    txt = re.sub(r"/\*.*?\*/", " ", L.HEADER.read_text(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", txt, flags=re.S)
    assert m
    assert len(L._SIGS[name][1]) == len(m.group(1).split(",")) == count


def _fake_ctx():
    buf = ctypes.create_string_buffer(64)
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def _mem():
    b = ctypes.create_string_buffer(8192)
    return b, (ctypes.addressof(b) + 15) // 16 * 16


def test_parse_poll_null_context_and_bad_fields():
    lib = L._lib()
    keep, ctx = _fake_ctx()
    mem, p = _mem()
    ptr_names = ("frames", "flen", "foff", "ids", "gen", "nfr", "sel", "n_sel", "n_match", "idx", "n_rows", "co", "rl",
                 "ro", "est", "fst")

    def status(handle=ctx, k=8, Lb=40, mr=6, fs=64, N=10, G_src=23, n_max=8, **ptrs):
        a = {n: p + 256 * i for i, n in enumerate(ptr_names)}
        a.update(ptrs)
        return lib.qf_parse_poll_headers_dev(handle, k, Lb, mr, a["frames"], fs, N, a["flen"], a["foff"], a["ids"],
                                             a["gen"], a["nfr"], G_src, n_max, a["sel"], a["n_sel"], a["n_match"],
                                             a["idx"], a["n_rows"], a["co"], a["rl"], a["ro"], a["est"], a["fst"])

    # every check comes before the context is touched (a fake context would crash otherwise)
    assert status(handle=None) == E
    assert status(k=0) == E and status(k=257) == E
    assert status(Lb=0) == E
    assert status(mr=0) == E and status(mr=1025) == E
    assert status(G_src=0) == E and status(G_src=(1 << 24) + 1) == E
    assert status(n_max=0) == E
    assert status(fs=72) == E                                   # not a multiple of 16
    assert status(fs=1 << 20, N=(1 << 12) + 1) == E             # N_max * frame_stride above 2^32
    assert status(frames=p + 8) == E                            # not 16-byte aligned
    for nm in ptr_names:
        if nm not in ("foff", "nfr", "n_match"):
            assert status(**{nm: None}) == E, nm
    del keep, mem


def test_rank_update_sel_null_context_shape_list_and_bad_fields():
    lib = L._lib()
    keep, ctx = _fake_ctx()
    mem, p = _mem()
    sh = L.RankShape(8, 0, 4, 0)
    good = L.GenSel(p, None, 4, 9)
    order = ("idx", "n", "co", "state", "fl", "rsel", "rk", "st")
    args = dict(idx=p + 256, n=None, co=None, state=p + 512, fl=None, rsel=None, rk=None, st=p + 4096)

    def status(handle=ctx, shape=sh, sel=good, **over):
        a = {**args, **over}
        return lib.qf_rank_update_sel_batch(handle, ctypes.byref(shape) if shape else None,
                                            ctypes.byref(sel) if sel else None, *[a[o] for o in order])

    assert status(handle=None) == E and status(shape=None) == E and status(sel=None) == E
    assert status(sel=L.GenSel(None, None, 4, 9)) == E
    assert status(sel=L.GenSel(p, None, 0, 9)) == E
    assert status(sel=L.GenSel(p, None, 4, 0)) == E
    for bad in (L.RankShape(0, 0, 4, 0), L.RankShape(257, 0, 4, 0), L.RankShape(8, 0, 0, 0), L.RankShape(8, 0, 4097, 0),
                L.RankShape(8, 0, 4, 1)):
        assert status(shape=bad) == E
    assert status(shape=L.RankShape(200, 57, 4, 0)) == L.QF_ERANGE
    for nm in ("idx", "state", "st"):
        assert status(**{nm: None}) == E, nm
    assert status(state=p + 512 + 8) == E
    del keep, mem


def test_store_append_sel_null_context_shape_list_and_bad_fields():
    lib = L._lib()
    keep, ctx = _fake_ctx()
    mem, p = _mem()
    good = L.GenSel(p, None, 4, 9)
    nulls = [None] * 14

    def status(k=8, Lb=100, mr=6, cap=8, flags=0, reserved=0, sgs=6 * 128, rs=112, gs=8 * 112, handle=ctx, shape=True,
               sel=good):
        sh = L.StoreShape(k, Lb, mr, cap, flags, reserved, sgs, rs, gs)
        return lib.qf_store_append_sel_dev(handle, ctypes.byref(sh) if shape else None,
                                           ctypes.byref(sel) if sel else None, *nulls)

    assert status() == E                                        # a good shape and list: the NULL pointers
    assert status(handle=None) == E and status(shape=False) == E and status(sel=None) == E
    assert status(sel=L.GenSel(None, None, 4, 9)) == E
    assert status(sel=L.GenSel(p, None, 0, 9)) == E and status(sel=L.GenSel(p, None, 4, 0)) == E
    # the shape rules are those of the dense call: each one alone fails
    b = [p + 256 * i for i in range(1, 15)]
    b[4] = None                                                 # n_rows
    b[6] = None                                                 # take

    def full(**kw):
        sh = L.StoreShape(*[kw.get(n, d) for n, d in (("k", 8), ("Lb", 100), ("mr", 6), ("cap", 8), ("flags", 0),
                                                        ("reserved", 0), ("sgs", 6 * 128), ("rs", 112), ("gs", 8 * 112))])
        return lib.qf_store_append_sel_dev(ctx, ctypes.byref(sh), ctypes.byref(good), *kw.get("ptrs", b))

    for kw in (dict(k=0), dict(k=257), dict(Lb=0), dict(mr=0), dict(mr=1025), dict(cap=0), dict(cap=1025), dict(flags=1),
               dict(reserved=1), dict(sgs=6 * 128 + 8), dict(rs=104), dict(rs=96), dict(gs=8 * 112 + 8),
               dict(gs=8 * 112 - 16), dict(cap=512, rs=(1 << 23) + 16, gs=512 * ((1 << 23) + 16))):
        assert full(**kw) == E, kw
    for i in range(14):
        if i not in (4, 6):
            assert full(ptrs=[None if j == i else x for j, x in enumerate(b)]) == E, i
    assert full(ptrs=[b[0] + 8] + b[1:]) == E                   # src not 16-byte aligned
    del keep, mem


def test_mirrors_reject_undersized_buffers():
    import torch

    from quicfuscate_amd import fec

    k, mr, cap, Lb, N, G_src, n_max, fs = 8, 6, 8, 40, 10, 5, 3, 64
    sb = fec.rank_state_bytes(k)
    u8 = lambda n: torch.zeros(n, dtype=torch.uint8)            # noqa: E731
    i32 = lambda n: torch.zeros(n, dtype=torch.int32)           # noqa: E731
    i16 = lambda n: torch.zeros(n, dtype=torch.int16)           # noqa: E731
    i64 = lambda n: torch.zeros(n, dtype=torch.int64)           # noqa: E731
    b = dict(frames=u8(N * fs), frame_len=i32(N), ids=i64(N), frame_gen=i32(N), sel=i32(n_max), n_sel=i32(1),
             row_index=i16(n_max * mr), n_rows=i32(n_max), row_coeffs=u8(n_max * mr * k), row_len=i32(n_max * mr),
             row_off=i32(n_max * mr), entry_status=i32(n_max), frame_status=i32(N))

    def parse(**kw):
        a = {**b, **{key: v for key, v in kw.items() if key in b}}
        extra = {key: v for key, v in kw.items() if key not in b}
        fec.parse_poll_headers(*[a[n] for n in b], k, Lb, max_rows=mr, frame_stride=fs, N_max=N, G_src=G_src, n_max=n_max,
                               **extra)

    for key in b:
        with pytest.raises(ValueError, match=key):
            parse(**{key: b[key][:-1]})
    for key, t in (("n_frames", i32(0)), ("frame_off", i32(N - 1)), ("n_match", i32(0))):
        with pytest.raises(ValueError, match=key):
            parse(**{key: t})

    sel, n_sel, idx, state, st = b["sel"], b["n_sel"], b["row_index"], u8(G_src * sb), i32(n_max)

    def upd(sel=sel, n_sel=n_sel, idx=idx, state=state, st=st, **extra):
        fec.rank_update_sel_batch(sel, n_sel, idx, state, st, k, max_rows=mr, n_max=n_max, G_src=G_src, **extra)

    for what, kw in (("sel", dict(sel=sel[:-1])), ("n_sel", dict(n_sel=i32(0))), ("row_index", dict(idx=idx[:-1])),
                     ("state", dict(state=state[:-1])), ("status", dict(st=st[:-1])), ("n_rows", dict(n_rows=i32(n_max - 1))),
                     ("row_coeffs", dict(row_coeffs=u8(n_max * mr * k - 1))),
                     ("innovative", dict(innovative=u8(n_max * mr - 1))), ("rank_sel", dict(rank_sel=i32(n_max - 1))),
                     ("rank", dict(rank=i32(G_src - 1)))):
        with pytest.raises(ValueError, match=what):
            upd(**kw)

    rs = 48
    s = dict(sel=sel, n_sel=n_sel, src=u8(N * fs), row_off=b["row_off"], row_len=b["row_len"], row_index=idx,
             row_coeffs=b["row_coeffs"], store=u8(G_src * cap * rs), store_off=i32(G_src * cap),
             store_len=i32(G_src * cap), store_index=i16(G_src * cap), store_coeffs=u8(G_src * cap * k),
             store_n=i32(G_src), status=st)

    def app(**kw):
        a = {**s, **{key: v for key, v in kw.items() if key in s}}
        extra = {key: v for key, v in kw.items() if key not in s}
        fec.store_append_sel(*[a[n] for n in s], k, Lb, max_rows=mr, cap=cap, src_bytes=N * fs, store_row_stride=rs,
                             store_gen_stride=cap * rs, n_max=n_max, G_src=G_src, **extra)

    for key in s:
        with pytest.raises(ValueError, match="store:" if key == "store" else key):
            app(**{key: s[key][:-1]})
    with pytest.raises(ValueError, match="n_rows"):
        app(n_rows=i32(n_max - 1))
    with pytest.raises(ValueError, match="take"):
        app(take=u8(n_max * mr - 1))


def test_reference_groups_a_hand_written_poll():
    k, Lb, mr, G_src = 4, 20, 2, 6
    p = PR.Poll(k, Lb, 9)
    pay = np.arange(5, dtype=np.uint8)
    v = np.array([1, 2, 3, 4], np.uint8)
    # arrival order: gen 4, 1, 4, 6 (bad tag), 1, 2, 1 (third of gen 1: overflow), 0xFFFFFFFF, 4 past n_frames
    p.put_sys(0, 4, 7, pay)            # id 7 % 4 = 3
    p.put_coded(1, 1, 0, v, pay)
    p.put_coded(2, 4, 0, v, pay[:0])
    p.put_sys(3, 6, 1, pay)
    p.put_sys(4, 1, 1, pay)
    p.put_coded(5, 2, 0, v, pay, cl=k + 1)   # QF_ERANGE: entry 2 is listed with no row
    p.put_sys(6, 1, 2, pay)
    p.put_sys(7, 0xFFFFFFFF, 1, pay)
    p.put_sys(8, 4, 1, pay)
    r = PR.ingest(p, 8, G_src, 4, mr)
    assert r.N == 8 and r.sel[:3].tolist() == [1, 2, 4] and r.n_sel == r.n_match == 3 and r.sel[3] == PR.FILL32
    assert r.entries == [[], [5], [0, 2]]
    assert r.entry_status.tolist() == [PR.ETOOSMALL, PR.OK, PR.OK, PR.OK]
    assert r.n_rows.tolist() == [0, 0, 2, 0]
    assert r.frame_status[:8].tolist() == [PR.OK, PR.ENOTREADY, PR.OK, PR.EINVAL, PR.ENOTREADY, PR.ERANGE, PR.ENOTREADY,
                                           PR.EINVAL]
    assert r.frame_status.view(np.uint32)[8] == PR.FILL32                       # at or above N: not written
    P = p.P
    assert r.row_off[2].tolist() == [0 * p.fs + P, 2 * p.fs + P] and r.row_len[2].tolist() == [5, 0]
    assert r.row_index[2].tolist() == [3, k]
    assert r.row_coeffs[2].tolist() == [[0, 0, 0, 1], [1, 2, 3, 4]]
    assert (r.row_off[:2] == PR.FILL32).all() and (r.row_coeffs[3] == PR.FILL).all()
    # a full list: generation 4 is touched but not listed, its frames can come again
    r = PR.ingest(p, None, G_src, 2, mr)
    assert r.sel.tolist() == [1, 2] and r.n_sel == 2 and r.n_match == 3
    assert [r.frame_status[f] for f in (0, 2, 8)] == [PR.ENOTREADY] * 3
    # the overflow rule does not depend on order: a third frame makes the entry QF_ETOOSMALL wherever it arrives
    r = PR.ingest(p, 6, G_src, 4, mr)
    assert r.entries[0] == [1, 4] and r.entry_status[0] == PR.OK and r.n_rows[0] == 2
    # the host sort of the same poll
    r = PR.ingest(p, 8, G_src, 4, mr)
    fr, fl, fo, ids, nfr = PR.dense_poll(p, r.entries, 4, mr)
    assert nfr.tolist() == [0, 1, 2, 0] and np.array_equal(fr[2, 1], p.frames[2]) and ids[2, 0] == 7
    assert (fr[0] == PR.FILL).all()


@pytest.mark.parametrize("k,mr", PR.SHAPES)
def test_seeded_polls_hold_the_cases_the_device_tests_are_about(k, mr):
    G_src, N = PR.G_POLL, PR.N_POLL
    for seed in (1, 2, 3):
        p = PR.make_poll(k, mr, seed)
        r = PR.ingest(p, None, G_src, G_src, mr)
        touched = r.sel[: r.n_sel].tolist()
        assert r.n_sel == r.n_match and all(g not in touched for g in PR.UNTOUCHED)
        per = {g: [f for f in range(N) if p.gen[f] == g] for g in touched}
        # interleaved: some generation's frames are not a contiguous run of the poll
        assert any(m[-1] - m[0] + 1 > len(m) for m in per.values())
        # slot claims cross waves and 256-thread blocks
        assert any(m[0] < 64 and m[-1] >= 256 for m in per.values())
        assert len(per[PR.GEN_EXACT]) == mr and len(per[PR.GEN_OVER]) == mr + 1
        je, jo = touched.index(PR.GEN_EXACT), touched.index(PR.GEN_OVER)
        assert r.entry_status[je] == PR.OK and r.entries[je] == per[PR.GEN_EXACT]
        assert r.entry_status[jo] == PR.ETOOSMALL and r.n_rows[jo] == 0
        assert all(r.frame_status[f] == PR.ENOTREADY for f in per[PR.GEN_OVER])
        if mr == 70:
            assert k == 64 and r.n_rows[je] > 64, "the in-entry sort does not cross a wave"
        tags = set(int(t) for t in p.gen)
        assert G_src in tags and 0xFFFFFFFF in tags
        assert all(r.frame_status[f] == PR.EINVAL for f in range(N) if p.gen[f] >= G_src)
        # one frame of each invalid per-frame status, parsed (their generations are listed and not overflowed)
        for kind in PR.BAD_KINDS:
            f = p.kind.index(kind)
            assert p.kind.count(kind) == 1 and r.frame_status[f] == PR.BAD_STATUS[kind], (kind, r.frame_status[f])
        # the special generation: v, e_c, v again, e_c again, the zero vector, v + e_c -> flags 1 1 0 0 0 0
        jc = touched.index(PR.GEN_CASES)
        assert r.n_rows[jc] == 6
        co, idx = r.row_coeffs[jc, :6], r.row_index[jc, :6]
        assert idx.tolist() == [k, 2 % k, k, 2 % k, k, k] and not co[4].any()
        assert np.array_equal(co[0], co[2]) and np.array_equal(co[1], co[3])
        fl, rk = rank_ref.innovative(co.copy())
        assert fl.tolist() == [1, 1, 0, 0, 0, 0] and rk == 2
        # ... and in any other order of the same rows the flags differ
        fl2, _ = rank_ref.innovative(co[::-1].copy())
        assert fl2.tolist() != fl.tolist()
        # ragged row lengths, with the boundary ones
        lens = set(int(x) for j in range(r.n_sel) for x in r.row_len[j, : r.n_rows[j]])
        assert {0, 1, 15, 16, 17, PR.L_POLL} <= lens
        # a list shorter than the touched set
        n_max = 8
        assert r.n_match > n_max
        short = PR.ingest(p, None, G_src, n_max, mr)
        assert short.n_sel == n_max and short.n_match == r.n_match and short.sel.tolist() == touched[:n_max]
        assert any(short.frame_status[f] == PR.ENOTREADY and r.frame_status[f] == PR.OK for f in range(N))
    # the counts the device tests pass: 0, above N_max, NULL
    p = PR.make_poll(k, mr, 1)
    assert PR.ingest(p, 0, G_src, G_src, mr).n_sel == 0
    assert PR.ingest(p, N + 7, G_src, G_src, mr).N == N == PR.ingest(p, None, G_src, G_src, mr).N
