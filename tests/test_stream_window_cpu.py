"""The generation window without a device: qf_gen_window_dev and
qf_gen_window_sel_dev are exported, declared and bound with the header's
argument counts, the two new statuses have texts, a NULL context and every bad
field fail before any device work, the Python mirrors check every buffer,
tests/window_ref.py gives what the header states on a hand-written poll, the
seeded polls of tests/test_gpu_stream_window.py hold the cases those tests are
about, and the seeded stream of the loop test stays within its conditions under
the model alone.  CPU only."""
import ctypes
import re

import numpy as np
import pytest

from quicfuscate_amd import _lib as L
from tests import window_ref as WR

NAMES = (("qf_gen_window_dev", 13), ("qf_gen_window_sel_dev", 5))
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


def test_constants_and_status_texts():
    lib = L._lib()
    txt = L.HEADER.read_text()
    assert re.search(r"#define\s+QF_ESTALE\s+\(-8\)", txt) and re.search(r"#define\s+QF_ECLOSED\s+\(-9\)", txt)
    assert re.search(r"#define\s+QF_GEN_NONE\s+0xFFFFFFFFu", txt) and re.search(r"#define\s+QF_WINDOW_CLOSE\s+1u", txt)
    assert re.search(r"#define\s+QF_ABI_VERSION\s+1\b", txt) and lib.qf_abi_version() == 1
    assert (L.QF_ESTALE, L.QF_ECLOSED, L.QF_GEN_NONE, L.QF_WINDOW_CLOSE) == (-8, -9, 0xFFFFFFFF, 1)
    assert (WR.ESTALE, WR.ECLOSED, WR.GEN_NONE) == (L.QF_ESTALE, L.QF_ECLOSED, L.QF_GEN_NONE)
    stale, closed, unknown = (lib.qf_strerror(s).decode() for s in (-8, -9, -100))
    assert stale and closed and stale != closed and unknown not in (stale, closed)
    assert len({lib.qf_strerror(s) for s in range(-9, 1)}) == 10


def _fake_ctx():
    buf = ctypes.create_string_buffer(64)
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def _mem():
    b = ctypes.create_string_buffer(8192)
    return b, (ctypes.addressof(b) + 15) // 16 * 16


def test_window_null_context_and_bad_fields():
    lib = L._lib()
    keep, ctx = _fake_ctx()
    mem, p = _mem()
    ptr_names = ("ids", "nfr", "win", "gen", "fst", "esel", "nev", "eid")

    def status(handle=ctx, G_src=23, N=10, flags=0, nem=10, **ptrs):
        a = {n: p + 512 * i for i, n in enumerate(ptr_names)}
        a.update(ptrs)
        return lib.qf_gen_window_dev(handle, G_src, N, a["ids"], a["nfr"], a["win"], flags, a["gen"], a["fst"], nem,
                                     a["esel"], a["nev"], a["eid"])

    # every check comes before the context is touched (a fake context would crash otherwise)
    assert status(handle=None) == E
    assert status(G_src=0) == E and status(G_src=(1 << 24) + 1) == E
    assert status(flags=1) == E and status(flags=1 << 31) == E
    assert status(nem=9) == E                                   # below min(N_max, G_src) = N_max
    assert status(N=40, nem=22) == E                            # ... = G_src
    assert status(N=0, nem=0, win=None) == E
    for nm in ("win", "esel", "nev", "ids", "gen", "fst"):
        assert status(**{nm: None}) == E, nm
    for nm in ("win", "esel", "nev"):                           # required with N_max == 0 as well
        assert status(N=0, nem=0, ids=None, gen=None, fst=None, **{nm: None}) == E, nm
    assert status(win=p + 1024 + 4) == E                        # not 8-byte aligned
    del keep, mem


def test_window_sel_null_context_list_and_bad_fields():
    lib = L._lib()
    keep, ctx = _fake_ctx()
    mem, p = _mem()
    good = L.GenSel(p, None, 4, 9)

    def status(handle=ctx, sel=good, win=p + 512, flags=L.QF_WINDOW_CLOSE, ids=p + 1024):
        return lib.qf_gen_window_sel_dev(handle, ctypes.byref(sel) if sel else None, win, flags, ids)

    assert status(handle=None) == E and status(sel=None) == E and status(win=None) == E
    assert status(sel=L.GenSel(None, None, 4, 9)) == E
    assert status(sel=L.GenSel(p, None, 0, 9)) == E and status(sel=L.GenSel(p, None, 4, 0)) == E
    assert status(flags=2) == E and status(flags=3) == E
    assert status(flags=0, ids=None) == E                       # neither the flag nor ids
    del keep, mem


def test_mirrors_reject_undersized_buffers():
    import torch

    from quicfuscate_amd import fec

    N, G_src, nem, n_max = 10, 5, 5, 3
    i32 = lambda n: torch.zeros(n, dtype=torch.int32)           # noqa: E731
    i64 = lambda n: torch.zeros(n, dtype=torch.int64)           # noqa: E731
    b = dict(frame_id=i64(N), win=i64(G_src), frame_gen=i32(N), frame_status=i32(N), evict_sel=i32(nem), n_evict=i32(1))

    def win(**kw):
        a = {**b, **{key: v for key, v in kw.items() if key in b}}
        extra = {key: v for key, v in kw.items() if key not in b}
        fec.gen_window(*[a[n] for n in b], G_src=G_src, N_max=N, n_evict_max=nem, **extra)

    for key in b:
        with pytest.raises(ValueError, match=key):
            win(**{key: b[key][:-1]})
    for key, t in (("n_frames", i32(0)), ("evict_id", i64(nem - 1))):
        with pytest.raises(ValueError, match=key):
            win(**{key: t})

    sel, n_sel, w, ids = i32(n_max), i32(1), i64(G_src), i64(n_max)
    for what, kw in (("sel", dict(sel=sel[:-1])), ("n_sel", dict(n_sel=i32(0))), ("win", dict(win=w[:-1])),
                     ("ids", dict(ids=ids[:-1]))):
        a = dict(sel=sel, n_sel=n_sel, win=w, ids=ids)
        a.update(kw)
        with pytest.raises(ValueError, match=what):
            fec.gen_window_sel(a["sel"], a["n_sel"], a["win"], n_max=n_max, G_src=G_src, ids=a["ids"], close=True)


def test_model_on_a_hand_written_poll():
    G = 5
    C = WR.CLOSED
    # slot 0 empty, 1 open with 6, 2 closed with 7, 3 open with 13, 4 closed with 9
    win = np.array([0, 6 + 1, (7 + 1) | C, 13 + 1, (9 + 1) | C], np.uint64)
    #      f: 0   1  2  3   4  5  6   7           8        9        10
    ids = [10, 5, 11, 6, 12, 7, 8, 13, WR.ID_LIMIT, 14, 14 + 2 * G]
    ids = np.array(ids + [19], np.uint64)                   # frame 11 lies past n_frames
    r = WR.window(win, ids, 11, G, 5)
    assert r.N == 11
    # slot 0: 10 beats 5 whatever the order; slot 1: 11 displaces the open 6; slot 2: 12 displaces the closed 7;
    # slot 3: 8 is older than 13, which stays; slot 4: 24 beats 14 and displaces the closed 9
    assert r.win.tolist() == [10 + 1, 11 + 1, 12 + 1, 13 + 1, 24 + 1]
    assert r.n_evict == 1 and r.evict_sel[0] == 1 and r.evict_id[0] == 6
    assert (r.evict_sel[1:] == WR.FILL32).all() and (r.evict_id[1:] == WR.FILL64).all()
    assert r.frame_status[:11].tolist() == [WR.OK, WR.ESTALE, WR.OK, WR.ESTALE, WR.OK, WR.ESTALE, WR.ESTALE, WR.OK,
                                            WR.EINVAL, WR.ESTALE, WR.OK]
    N = WR.GEN_NONE
    assert r.frame_gen[:11].tolist() == [0, N, 1, N, 2, N, N, 3, N, N, 4]
    assert r.frame_gen[11] == WR.FILL32 and r.frame_status.view(np.uint32)[11] == WR.FILL32
    # the same poll again: nothing is displaced, every newest frame is current
    r2 = WR.window(r.win, ids, 11, G, 5)
    assert np.array_equal(r2.win, r.win) and r2.n_evict == 0
    assert np.array_equal(r2.frame_status, r.frame_status) and np.array_equal(r2.frame_gen, r.frame_gen)
    # closing slots 1 and 4 (4 listed twice), an invalid entry, an empty slot, an unused entry
    w0 = np.array([0, 11 + 1, (12 + 1) | C, 13 + 1, 24 + 1], np.uint64)
    after, out = WR.window_sel(w0, [4, 1, 7, 0, 4, 3], 5, 6, G, True)
    assert out.tolist() == [24, 11, WR.NO_ID, WR.NO_ID, 24, WR.NO_ID]
    assert after.tolist() == [0, (11 + 1) | C, (12 + 1) | C, 13 + 1, (24 + 1) | C]
    same, out2 = WR.window_sel(w0, [4, 1, 7, 0, 4, 3], None, 6, G, False)
    assert np.array_equal(same, w0) and out2.tolist() == [24, 11, WR.NO_ID, WR.NO_ID, 24, 13]
    # a frame of a closed generation, and a full count
    r3 = WR.window(after, np.array([11, 24, 13, 1], np.uint64), None, G, 4)
    assert r3.frame_status.tolist() == [WR.ECLOSED, WR.ECLOSED, WR.OK, WR.ESTALE] and np.array_equal(r3.win, after)
    assert r3.frame_gen.tolist() == [N, N, 3, N] and r3.n_evict == 0
    # every id shares the slot of G_src = 1
    r4 = WR.window(np.zeros(1, np.uint64), np.array([3, 9, 4], np.uint64), None, 1, 1)
    assert r4.win.tolist() == [10] and r4.frame_gen.tolist() == [N, 0, N] and r4.n_evict == 0


def test_the_case_poll_holds_every_case_by_name():
    win, ids, named = WR.make_case(1)
    G = WR.G_CASE
    assert len(ids) == WR.N_CASE and len(win) == G
    r = WR.window(win, ids, None, G, G)
    st, tag = r.frame_status, r.frame_gen

    def all_are(name, status, slot):
        assert named[name], name
        for f in named[name]:
            assert st[f] == status and tag[f] == (slot if status == WR.OK else WR.GEN_NONE), (name, f, st[f], tag[f])

    assert all(int(ids[f]) < G for f in named["small"]) and all(G <= int(ids[f]) < 2 * G for f in named["small_ring"])
    all_are("small", WR.OK, WR.S_SMALL)
    all_are("small_ring", WR.OK, WR.S_SMALL_RING)
    assert all(int(ids[f]) >> 32 and int(ids[f]) & 0xFFFFFFFF for f in named["base"])       # both words
    all_are("base", WR.OK, WR.S_BASE)
    # two and three ids of one slot, the oldest arriving last
    all_are("two_old", WR.ESTALE, 0)
    all_are("two_new", WR.OK, WR.S_TWO)
    assert max(named["two_old"]) > max(named["two_new"])
    for nm in ("three_old", "three_mid"):
        all_are(nm, WR.ESTALE, 0)
    all_are("three_new", WR.OK, WR.S_THREE)
    assert max(named["three_old"]) > max(named["three_mid"] + named["three_new"])
    # displacing an open entry lists the slot, displacing a closed one does not
    all_are("evicts", WR.OK, WR.S_EVICT)
    all_are("over_closed", WR.OK, WR.S_OVER_CLOSED)
    ev = r.evict_sel[: r.n_evict].tolist()
    assert WR.S_EVICT in ev and WR.S_EVICT_TWICE in ev and WR.S_OVER_CLOSED not in ev and ev == sorted(ev)
    assert int(r.evict_id[ev.index(WR.S_EVICT)]) == WR.case_id(WR.S_EVICT, 0)
    assert int(r.evict_id[ev.index(WR.S_EVICT_TWICE)]) == WR.case_id(WR.S_EVICT_TWICE, 0)
    all_are("twice_mid", WR.ESTALE, 0)
    all_are("twice_new", WR.OK, WR.S_EVICT_TWICE)
    assert WR.held(r.win[WR.S_OVER_CLOSED]) == WR.case_id(WR.S_OVER_CLOSED, 1) and not int(r.win[WR.S_OVER_CLOSED]) >> 63
    assert (r.evict_sel[r.n_evict:] == WR.FILL32).all() and r.n_evict < G
    # a frame of a closed generation, a stale frame beside a current one, an unchanged entry
    all_are("closed", WR.ECLOSED, 0)
    all_are("stale", WR.ESTALE, 0)
    all_are("current", WR.OK, WR.S_STALE)
    all_are("same", WR.OK, WR.S_SAME)
    for s in (WR.S_CLOSED, WR.S_STALE, WR.S_SAME):
        assert r.win[s] == win[s]
    # 2^62 - 1 is valid, 2^62 and 2^64 - 1 are not and touch no slot
    (f,) = named["max_id"]
    assert int(ids[f]) == (1 << 62) - 1 and st[f] == WR.OK and tag[f] == WR.S_MAXID and int(r.win[WR.S_MAXID]) == 1 << 62
    assert sorted(int(ids[f]) for f in named["invalid"]) == [1 << 62, (1 << 64) - 1]
    all_are("invalid", WR.EINVAL, 0)
    assert (1 << 62) % G == WR.S_INVALID_ONLY and r.win[WR.S_INVALID_ONLY] == win[WR.S_INVALID_ONLY] != 0
    # slots no frame maps to: empty, open and closed
    untouched = [s for s in range(G) if s not in r.touched]
    assert {WR.S_EMPTY_IDLE, WR.S_OPEN_IDLE, WR.S_CLOSED_IDLE, WR.S_INVALID_ONLY} <= set(untouched)
    assert win[WR.S_EMPTY_IDLE] == 0 and 0 < int(win[WR.S_OPEN_IDLE]) < WR.CLOSED <= int(win[WR.S_CLOSED_IDLE])
    assert all(r.win[s] == win[s] for s in untouched)
    # the prepared window holds all three kinds, and every status turns up
    assert {0, 1, 2} == {0 if w == 0 else 2 if int(w) >> 63 else 1 for w in win}
    assert {WR.OK, WR.EINVAL, WR.ESTALE, WR.ECLOSED} == set(int(x) for x in st)
    # the counts the device tests pass
    assert WR.window(win, ids, 0, G, G).n_evict == 0 and WR.window(win, ids, 0, G, G).touched == []
    assert WR.window(win, ids, WR.N_CASE + 7, G, G).N == WR.N_CASE
    half = WR.window(win, ids, 150, G, G)
    assert half.N == 150 and (half.frame_gen[150:] == WR.FILL32).all() and not np.array_equal(half.win, r.win)


def test_the_random_polls_hold_their_shapes():
    win, ids = WR.random_case(1, 200, 3)
    r = WR.window(win, ids, None, 1, 1)
    assert len(set(int(x) for x in ids)) > 3 and r.touched == [0] and (r.frame_status == WR.ESTALE).any()
    G, N = 70001, 4096
    win, ids = WR.random_case(G, N, 5)
    r = WR.window(win, ids, None, G, N)
    per_block = 2048                                            # generations of one select block
    assert G % per_block and G // per_block >= 8
    ev = r.evict_sel[: r.n_evict]
    assert len(set(int(s) // per_block for s in ev)) >= 8 and int(ev.max()) >= G // per_block * per_block
    assert 100 < r.n_evict < N and {WR.OK, WR.ESTALE, WR.ECLOSED} <= set(int(x) for x in r.frame_status)


def test_the_seeded_stream_stays_within_its_conditions():
    records, stats = WR.simulate(WR.SEED_LOOP)
    assert WR.GENS_LOOP > 3 * WR.G_LOOP
    assert stats["completions"] >= 20 and stats["evictions_with_rows"] >= 5, stats
    assert stats["stale"] >= 1 and stats["closed"] >= 1 and stats["full_lists"] >= 1, stats
    assert len(stats["delivered"]) == stats["completions"]
    assert all(WR.BASE_LOOP <= x < WR.BASE_LOOP + WR.GENS_LOOP for x in stats["delivered"])
    # completions spread over the ring more than once, and over several polls
    assert max(stats["delivered"]) - min(stats["delivered"]) > 2 * WR.G_LOOP
    assert len(set(stats["delivered"].values())) > 5
    for rec in records:
        assert rec.n <= WR.N_LOOP and len(rec.completed) <= WR.LIST_LOOP
        per_id = {}
        for g, _ in rec.take:
            per_id[g] = per_id.get(g, 0) + 1
        assert max(per_id.values()) <= WR.MR_LOOP
    # every frame of the stream ends as ingested or dropped, none is lost in the ring
    ended = sum(st != WR.ENOTREADY for rec in records for st in rec.status)
    assert ended == len(WR.make_stream(WR.SEED_LOOP))
