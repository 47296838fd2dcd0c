"""The generation window on the MI355X: qf_gen_window_dev and
qf_gen_window_sel_dev byte for byte against tests/window_ref.py, the hand-off
of the tags to qf_parse_poll_headers_dev, and the whole receive loop over a
stream whose generation ids run more than three times round the slot ring:
window -> the two resets over the evict list -> ingest -> listed update ->
listed append -> select -> listed decode -> close -> the two resets.

Every output starts as 0xCC with guard bytes behind it, the bytes a call must
not write are checked to still be 0xCC, and the sources are checked to be
unchanged.  The polls and the stream are tests/window_ref.py's;
tests/test_stream_window_cpu.py asserts that they hold the cases these tests
are about."""
import numpy as np
import pytest

from tests import poll_ref as PR
from tests import test_gpu_poll_ingest as T
from tests import test_gpu_recv_inplace as I
from tests import window_ref as WR

pytestmark = pytest.mark.gpu

FILL, GUARD, NONE16 = T.FILL, T.GUARD, T.NONE16
_r16, _dev, _filled, _host, _body = T._r16, T._dev, T._filled, T._host, T._body


def _guarded(a):
    """A host array on the device with 0xCC guard bytes behind it."""
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return _dev(np.concatenate([raw, np.full(GUARD, FILL, np.uint8)]))


def _count(n):
    return None if n in (None, "null") else _dev(np.array([n], np.uint32))


def run_window(qf, win, ids, n_frames, G_src, nem, t_win=None, with_ids=True):
    """qf_gen_window_dev over a window (host array, or a guarded device buffer
    that is updated in place) -> the device buffers, host views of every output."""
    N = len(ids)
    t_win = _guarded(win) if t_win is None else t_win
    t_ids = _dev(np.asarray(ids, np.uint64))
    d = dict(win=t_win, gen=_filled(4 * N + GUARD), fst=_filled(4 * N + GUARD), esel=_filled(4 * nem + GUARD),
             nev=_filled(4 + GUARD), eid=_filled(8 * nem + GUARD) if with_ids else None)
    qf.gen_window(t_ids, t_win, d["gen"], d["fst"], d["esel"], d["nev"], G_src=G_src, N_max=N, n_evict_max=nem,
                  n_frames=_count(n_frames), evict_id=d["eid"])
    qf.default_context().sync()
    assert np.array_equal(_host(t_ids, np.uint64), np.asarray(ids, np.uint64)), "the ids were written"
    return d, window_views(d, N, G_src, nem)


def window_views(d, N, G_src, nem):
    return dict(win=_body(d["win"], 8 * G_src, np.uint64), gen=_body(d["gen"], 4 * N, np.uint32),
                fst=_body(d["fst"], 4 * N, np.int32), esel=_body(d["esel"], 4 * nem, np.uint32),
                nev=int(_body(d["nev"], 4, np.uint32)[0]),
                eid=_body(d["eid"], 8 * nem, np.uint64) if d["eid"] is not None else None)


def check_window(h, ref):
    """Every byte against the model: the window (untouched entries unchanged), the tags and statuses (0xCC at
    and above N), the evict list (0xCC at and above n_evict)."""
    assert h["nev"] == ref.n_evict
    for key, want in (("win", ref.win), ("gen", ref.frame_gen), ("fst", ref.frame_status), ("esel", ref.evict_sel),
                      ("eid", ref.evict_id)):
        if h[key] is None:
            continue
        bad = np.argwhere(h[key] != want)
        assert bad.size == 0, f"{key} differs from the model at {bad[:4].tolist()}"


# ---------------------------------------------------------------------------
# qf_gen_window_dev against the model
# ---------------------------------------------------------------------------
def test_cases_against_the_model(qf, gpu_ctx):
    win, ids, named = WR.make_case(1)
    G = WR.G_CASE
    ref = WR.window(win, ids, None, G, G)
    assert 0 < ref.n_evict < G and len(ref.touched) < G
    d, h = run_window(qf, win, ids, "null", G, G)
    check_window(h, ref)
    # a larger list and no evict_id: the same list, nothing behind it
    d, h = run_window(qf, win, ids, "null", G, G + 9, with_ids=False)
    check_window(h, WR.window(win, ids, None, G, G + 9))


@pytest.mark.parametrize("n_frames", [0, WR.N_CASE + 7, 150, "null"])
def test_frame_counts(qf, gpu_ctx, n_frames):
    win, ids, _ = WR.make_case(1)
    G = WR.G_CASE
    ref = WR.window(win, ids, None if n_frames == "null" else n_frames, G, G)
    assert ref.N == {0: 0, WR.N_CASE + 7: WR.N_CASE, 150: 150, "null": WR.N_CASE}[n_frames]
    d, h = run_window(qf, win, ids, n_frames, G, G)
    check_window(h, ref)
    if n_frames == 0:
        assert h["nev"] == 0 and np.array_equal(h["win"], win) and (h["gen"] == WR.FILL32).all()


def test_no_frame_slots(qf, gpu_ctx):
    """N_max == 0: *n_evict_dev = 0 and nothing else, with no per-frame pointer."""
    win, _, _ = WR.make_case(1)
    G = WR.G_CASE
    t_win, esel, nev = _guarded(win), _filled(GUARD), _filled(4 + GUARD)
    qf.gen_window(None, t_win, None, None, esel, nev, G_src=G, N_max=0, n_evict_max=0)
    qf.default_context().sync()
    assert int(_body(nev, 4, np.uint32)[0]) == 0 and np.array_equal(_body(t_win, 8 * G, np.uint64), win)
    assert (_host(esel) == FILL).all()


@pytest.mark.parametrize("G_src,N,seed", [(1, 200, 3), (70001, 4096, 5)], ids=["one_slot", "many_select_blocks"])
def test_slot_count_shapes(qf, gpu_ctx, G_src, N, seed):
    win, ids = WR.random_case(G_src, N, seed)
    nem = min(N, G_src)
    d, h = run_window(qf, win, ids, "null", G_src, nem)
    check_window(h, WR.window(win, ids, None, G_src, nem))


@pytest.mark.parametrize("case", ["cases", "many_select_blocks"])
def test_two_runs_give_identical_bytes(qf, gpu_ctx, case):
    if case == "cases":
        (win, ids, _), G = WR.make_case(1), WR.G_CASE
    else:
        G = 70001
        win, ids = WR.random_case(G, 4096, 5)
    nem = min(len(ids), G)
    _, a = run_window(qf, win, ids, "null", G, nem)
    _, b = run_window(qf, win, ids, "null", G, nem)
    assert a["nev"] == b["nev"] > 0
    for key in ("win", "gen", "fst", "esel", "eid"):
        assert np.array_equal(a[key], b[key]), f"{key} differs between two runs"


# ---------------------------------------------------------------------------
# qf_gen_window_sel_dev
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("close", [True, False], ids=["close", "read"])
@pytest.mark.parametrize("variant", ["below", "clamped", "null"])
def test_ids_of_a_list_and_closing_it(qf, gpu_ctx, variant, close):
    win, ids, _ = WR.make_case(1)
    G = WR.G_CASE
    win = WR.window(win, ids, None, G, G).win
    open_slots = [s for s in range(G) if win[s] and not int(win[s]) >> 63]
    closed_slots = [s for s in range(G) if int(win[s]) >> 63]
    assert len(open_slots) >= 3 and closed_slots and win[WR.S_EMPTY_IDLE] == 0
    # a duplicate, an entry >= G_src, an empty slot, a slot that is closed already, and entries past the count
    sel = np.array([open_slots[1], G + 2, open_slots[0], WR.S_EMPTY_IDLE, open_slots[1], closed_slots[0], 0xFFFFFFFF,
                    open_slots[2], open_slots[0]], np.uint32)
    n_max = len(sel)
    n_sel = dict(below=n_max - 2, clamped=n_max + 5, null=None)[variant]
    want_win, want_ids = WR.window_sel(win, sel, n_sel, n_max, G, close)
    if variant == "below":
        assert want_ids[-1] == WR.NO_ID and want_win[open_slots[2]] == win[open_slots[2]]      # unused entries
    else:
        assert want_ids[-2] == WR.held(win[open_slots[2]])
    t_win, t_sel, t_ids = _guarded(win), _dev(sel), _filled(8 * n_max + GUARD)
    qf.gen_window_sel(t_sel, _count(n_sel), t_win, n_max=n_max, G_src=G, ids=t_ids, close=close)
    qf.default_context().sync()
    assert np.array_equal(_host(t_sel, np.uint32), sel), "the list was written"
    assert np.array_equal(_body(t_ids, 8 * n_max, np.uint64), want_ids)
    got = _body(t_win, 8 * G, np.uint64)
    assert np.array_equal(got, want_win)
    assert np.array_equal(got, win) != close
    if close:
        # closing without ids gives the same window
        t_win2 = _guarded(win)
        qf.gen_window_sel(t_sel, _count(n_sel), t_win2, n_max=n_max, G_src=G, close=True)
        qf.default_context().sync()
        assert np.array_equal(_body(t_win2, 8 * G, np.uint64), want_win)


# ---------------------------------------------------------------------------
# the tags as the ingest's
# ---------------------------------------------------------------------------
def _plain_poll(k, Lb, ids, tags):
    """One systematic frame per id, tagged as given."""
    rng = np.random.default_rng(77)
    p = PR.Poll(k, Lb, len(ids))
    for f in range(len(ids)):
        p.put_sys(f, 0, int(rng.integers(0, 1 << 30)), rng.integers(0, 256, int(rng.integers(0, Lb + 1)), dtype=np.uint8))
    p.gen[:] = tags
    return p


def test_hand_off_to_the_ingest(qf, gpu_ctx):
    win, ids, _ = WR.make_case(1)
    G, k, Lb, mr = WR.G_CASE, 5, 40, 70
    ref = WR.window(win, ids, None, G, G)
    d, h = run_window(qf, win, ids, "null", G, G)
    check_window(h, ref)
    p = _plain_poll(k, Lb, ids, ref.frame_gen)
    fp = T.FlatPoll(p)
    fp.gen = d["gen"][: 4 * len(ids)]                  # the window's own output, on the device
    _, hi = T.run_ingest(qf, fp, G, G, mr)
    T.check_against_reference(hi, PR.ingest(p, None, G, G, mr))
    ok = ref.frame_status == WR.OK
    assert ok.any() and not ok.all()
    assert (hi["fst"][~ok] == T.EINVAL).all(), "a dropped frame was not refused by the ingest"
    assert (hi["fst"][ok] == T.OK).all()
    assert hi["sel"][: hi["n_sel"]].tolist() == sorted(set(int(s) for s in ref.frame_gen[ok])) and hi["n_match"] == hi["n_sel"]


# ---------------------------------------------------------------------------
# the whole loop past the ring
# ---------------------------------------------------------------------------
class LoopReceiver:
    """The receiver of the loop test: T.Receiver plus seen, the window and the buffers of the window call."""

    def __init__(self, qf, oracle):
        import torch

        k, r, Lb, G = WR.K_LOOP, WR.R_LOOP, WR.L_LOOP, WR.G_LOOP
        self.qf, self.k, self.r, self.L, self.G, self.N, self.mr, self.n_list = qf, k, r, Lb, G, WR.N_LOOP, WR.MR_LOOP, WR.LIST_LOOP
        rng = np.random.default_rng(2024)
        self.src = rng.integers(0, 256, (WR.GENS_LOOP, k, Lb), dtype=np.uint8)
        self.C = oracle.cauchy(k, r)
        self.rep = np.stack([oracle.encode(self.src[g], r, self.C) for g in range(WR.GENS_LOOP)])
        self.rc = T.Receiver(qf, G, k, Lb, k, 0)
        self.seen = torch.zeros(G, dtype=torch.int32, device="cuda")
        self.win = _guarded(np.zeros(G, np.uint64))
        self.fs = PR.payload_offset(k) + _r16(Lb)

    def window_step(self, rec):
        """The window and the two resets over the evict list -> the window call's buffers and host views."""
        qf, G, k, rc = self.qf, self.G, self.k, self.rc
        d, h = run_window(qf, None, rec.ids, rec.n, G, G, t_win=self.win)
        qf.stream_reset(d["esel"], d["nev"], k, n_max=G, G_src=G, state=rc.state, store_n=rc.n, seen=self.seen)
        qf.stream_reset(d["esel"], d["nev"], k, n_max=G, G_src=G, seen=rc.rank)
        return d, h

    def poll_of(self, rec):
        k = self.k
        p = PR.Poll(k, self.L, self.N, self.fs)
        for f, (g, s) in enumerate(rec.take):
            if s < k:
                p.put_sys(f, 0, k * (g + 1) + s, self.src[g, s])
            else:
                p.put_coded(f, 0, 5000 + s, self.C[s - k], self.rep[g, s - k])
        p.gen[:] = rec.w.frame_gen
        return p

    def finish_step(self, t_ids):
        """Select, listed decode, a snapshot of the store, close, the two resets -> buffers."""
        qf, G, k, r, rc, n_list = self.qf, self.G, self.k, self.r, self.rc, self.n_list
        em = min(k, r)
        self.rec_rs = _r16(self.L) + 16
        self.rec_gs = em * self.rec_rs
        t_sel, t_nsel = _filled(4 * n_list + GUARD), _filled(4 + GUARD)
        qf.gen_select(rc.rank, t_sel, t_nsel, G=G, min_rank=k, n_max=n_list, seen=self.seen, mark=True)
        t = I._outputs(n_list, k, em, k, self.rec_gs)
        qf.decode_frames_sel(t_sel, t_nsel, rc.bytes, rc.off, rc.len, rc.index, rc.coeffs, t["rec"], t["ri"], t["nrec"],
                             t["st"], k, r, self.L, n_max=n_list, G_src=G, max_rows=k, src_gen_stride=rc.gs,
                             rec_row_stride=self.rec_rs, rec_gen_stride=self.rec_gs, n_rows=rc.n, src_slot=t["slot"])
        snap = rc.snapshot()
        qf.gen_window_sel(t_sel, t_nsel, self.win, n_max=n_list, G_src=G, ids=t_ids, close=True)
        qf.stream_reset(t_sel, t_nsel, k, n_max=n_list, G_src=G, state=rc.state, store_n=rc.n, seen=self.seen)
        qf.stream_reset(t_sel, t_nsel, k, n_max=n_list, G_src=G, seen=rc.rank)
        qf.default_context().sync()
        return t_sel, t_nsel, t, snap


def test_the_loop_past_the_ring(qf, oracle, gpu_ctx):
    records, stats = WR.simulate(WR.SEED_LOOP)
    lr = LoopReceiver(qf, oracle)
    k, Lb, G, N, mr, n_list, rc = lr.k, lr.L, lr.G, lr.N, lr.mr, lr.n_list, lr.rc
    em = min(k, lr.r)
    delivered, evicted_with_rows, stale, closed, full = {}, 0, 0, 0, 0
    for polls, rec in enumerate(records, 1):
        # 1-2: the window and the two resets over the evict list
        d, h = lr.window_step(rec)
        qf.default_context().sync()
        check_window(h, rec.w)
        if rec.w.n_evict:
            snap = rc.snapshot()
            seen = _host(lr.seen, np.uint32)
            for s in rec.w.evicted:
                assert not snap["state"][s].any() and snap["n"][s] == 0 and snap["rank"][s] == 0 and seen[s] == 0, (polls, s)
        evicted_with_rows += len(rec.evicted_with_rows)
        # 3: the ingest with the window's tags
        p = lr.poll_of(rec)
        fp = T.FlatPoll(p, rec.n)
        fp.gen = d["gen"][: 4 * N]
        di, hi = T.run_ingest(qf, fp, G, n_list, mr)
        T.check_against_reference(hi, PR.ingest(p, rec.n, G, n_list, mr))
        status = [int(h["fst"][f]) if h["fst"][f] != WR.OK else int(hi["fst"][f]) for f in range(rec.n)]
        assert status == rec.status, polls
        assert all(hi["fst"][f] == T.EINVAL for f in range(rec.n) if h["fst"][f] != WR.OK)
        stale += status.count(WR.ESTALE)
        closed += status.count(WR.ECLOSED)
        full += hi["n_match"] > hi["n_sel"]
        # 4-5: the listed update and append
        fl, _, st, ast = rc.listed_poll(di["sel"], di["n_sel"], n_list, di, mr, fp.frames, N * lr.fs, rank_sel=False)
        assert (st == T.OK).all() and (ast == T.OK).all()
        # 6-9: select, decode, close, the two resets
        t_ids = _filled(8 * n_list + GUARD)
        t_sel, t_nsel, t, snap = lr.finish_step(t_ids)
        assert snap["rank"].tolist() == rec.rank, polls
        n_done = int(_body(t_nsel, 4, np.uint32)[0])
        finished = _body(t_sel, 4 * n_list, np.uint32)[:n_done].tolist()
        labels = _body(t_ids, 8 * n_list, np.uint64)
        assert finished == rec.completed and labels[:n_done].tolist() == rec.labels and (labels[n_done:] == WR.NO_ID).all()
        out = I._collect(t, n_list, k, em, k, Lb, lr.rec_rs, lr.rec_gs, ("slot",))
        after = rc.snapshot()
        for j, s in enumerate(finished):
            label = int(labels[j])
            g = label - WR.BASE_LOOP
            assert label not in delivered and 0 <= g < WR.GENS_LOOP and label % G == s, (polls, j, label)
            assert snap["n"][s] == k and out["st"][j] == T.OK, (polls, j, s)
            rix = out["ri"][j, : out["nrec"][j]].tolist()
            rows = np.zeros((k, Lb), np.uint8)
            for i in range(k):
                c = int(out["slot"][j, i])
                if c == NONE16:
                    rows[i] = out["rec"][j, rix.index(i)]
                else:
                    assert snap["index"][s, c] == i
                    ln, off = int(snap["len"][s, c]), int(snap["off"][s, c])
                    rows[i, :ln] = snap["bytes"][s, off: off + ln]
            assert np.array_equal(rows, lr.src[g]), f"generation {label} was not recovered"
            delivered[label] = polls
            assert not after["state"][s].any() and after["n"][s] == 0 and after["rank"][s] == 0, s
        assert np.array_equal(_body(lr.win, 8 * G, np.uint64), rec.win_after), polls
        assert not _host(lr.seen, np.uint32)[finished].any()
    assert delivered == stats["delivered"]
    assert len(delivered) >= 20 and evicted_with_rows >= 5 and stale >= 1 and closed >= 1 and full >= 1
    assert (evicted_with_rows, stale, closed, full) == (stats["evictions_with_rows"], stats["stale"], stats["closed"],
                                                        stats["full_lists"])


def test_profile_names(qf, oracle, gpu_ctx):
    records, _ = WR.simulate(WR.SEED_LOOP)
    lr = LoopReceiver(qf, oracle)
    rec = records[0]
    t_ids = _filled(8 * lr.n_list + GUARD)
    gpu_ctx.sync()
    gpu_ctx.profile(True)
    d, h = lr.window_step(rec)
    p = lr.poll_of(rec)
    fp = T.FlatPoll(p, rec.n)
    fp.gen = d["gen"][: 4 * lr.N]
    di, hi = T.run_ingest(qf, fp, lr.G, lr.n_list, lr.mr)
    lr.rc.listed_poll(di["sel"], di["n_sel"], lr.n_list, di, lr.mr, fp.frames, lr.N * lr.fs, rank_sel=False)
    lr.finish_step(t_ids)
    times = gpu_ctx.kernel_times()
    gpu_ctx.profile(False)
    for name in ("k_window_max", "k_window_apply", "k_window_tag", "k_window_sel"):
        assert name in times and times[name][0] == 1, (name, times)
    assert {"k_gen_select", "k_poll_count", "k_poll_place", "k_poll_headers", "k_rank_update_sel", "k_store_prepare_sel",
            "k_store_rows_sel", "k_stream_reset"} <= set(times), times
    assert times["k_gen_select"][0] == 3 and times["k_stream_reset"][0] == 4, times
