"""The streaming receive step on the MI355X: qf_rank_update_batch against
tests/rank_ref.py, qf_gf256_rank and one qf_rank_batch over the whole arrival
sequence, however the sequence is split over calls; qf_store_append_dev against
tests/store_ref.py; and polls of parse headers -> update -> append, decoded
and recoded from the store, against the one-shot calls over all frames.

Every output buffer starts as 0xCC and the bytes a call must not write are
checked to still be 0xCC; source slots are 0xCC outside the frames, so a read
past row_len shows up in the zeroed tail of a stored row.  The traffic is
tests/store_ref.py's; tests/test_stream_recv_cpu.py asserts that it holds the
cases these tests are about."""
import numpy as np
import pytest

from tests import rank_ref, recv_ref, store_ref
from tests import test_gpu_rank as K
from tests import test_gpu_recv_inplace as I
from tests import test_gpu_relay_inplace as R
from tests import test_gpu_wire_coded as W

pytestmark = pytest.mark.gpu

FILL, FILL16, FILL32, NONE16 = 0xCC, 0xCCCC, 0xCCCCCCCC, 0xFFFF
OK, EINVAL, ENOTREADY, ETOOSMALL = 0, -1, -3, -7

_r16, _P, _dev, _filled, _host = W._r16, W._P, W._dev, W._filled, W._host


# ---------------------------------------------------------------------------
# rank state
# ---------------------------------------------------------------------------
class States:
    """G rank states of generation size k on the device, zeroed, with 64 bytes
    of 0xCC behind them (room: bytes per generation, default the state size)."""

    def __init__(self, qf, G, k, room=None):
        import torch

        self.qf, self.G, self.k = qf, G, k
        self.sb = qf.rank_state_bytes(k) if room is None else room
        self.t = torch.zeros(G * self.sb + 64, dtype=torch.uint8, device="cuda")
        self.t[G * self.sb:] = FILL

    def bytes(self):
        h = _host(self.t)
        assert (h[self.G * self.sb:] == FILL).all(), "bytes behind the last state were written"
        return h[: self.G * self.sb].reshape(self.G, self.sb).copy()

    def update(self, idx, co=None, r=0, mr=None, pass_n=True, k=None):
        """One qf_rank_update_batch: idx[g] the indices of generation g's slots
        in this call, co[g] their vectors (n_g, k) or None -> flags (list of
        (n_g,) arrays), rank (G,), status (G,).  Flags at and after n_g must be
        0, everything behind the outputs 0xCC."""
        G, k = self.G, self.k if k is None else k
        n = np.array([len(x) for x in idx], np.uint32)
        mr = max(1, int(n.max())) if mr is None else mr
        a_idx = np.full((G, mr), FILL16, np.uint16)
        a_co = np.full((G, mr, k), FILL, np.uint8)
        for g in range(G):
            a_idx[g, : n[g]] = idx[g]
            if co is not None and n[g]:
                a_co[g, : n[g]] = co[g]
        t_fl, t_rk, t_st = _filled(G * mr + 64), _filled(4 * G + 16), _filled(4 * G + 16)
        self.qf.rank_update_batch(_dev(a_idx), self.t, t_rk, t_st, k, r=r, max_rows=mr, G=G,
                                  n_rows=_dev(n) if pass_n else None, row_coeffs=_dev(a_co) if co is not None else None,
                                  innovative=t_fl)
        self.qf.default_context().sync()
        fl, rk, st = _host(t_fl), _host(t_rk, np.uint32), _host(t_st, np.int32)
        assert (fl[G * mr:] == FILL).all() and (rk[G:] == FILL32).all() and (st[G:].view(np.uint32) == FILL32).all()
        fl = fl[: G * mr].reshape(G, mr)
        for g in range(G):
            assert not fl[g, n[g]:].any(), f"flags behind the {n[g]} slots of generation {g} are not zero"
        return [fl[g, : n[g]].copy() for g in range(G)], rk[:G].copy(), st[:G].copy()


def feed(st, idx, co, counts, r=0, mr=None):
    """The sequences idx[g] / co[g] in calls of counts[g][t] slots -> the
    concatenated flags per generation, the last ranks; every status QF_OK and
    every call's rank the number of flags so far."""
    G = st.G
    pos = [0] * G
    flags = [[] for _ in range(G)]
    rk = np.zeros(G, np.uint32)
    for t in range(len(counts[0])):
        sl = [slice(pos[g], pos[g] + counts[g][t]) for g in range(G)]
        fl, rk, status = st.update([idx[g][sl[g]] for g in range(G)], None if co is None else [co[g][sl[g]] for g in range(G)],
                                   r=r, mr=mr)
        assert (status == OK).all(), (t, status)
        for g in range(G):
            flags[g].append(fl[g])
            pos[g] += counts[g][t]
            assert rk[g] == sum(int(f.sum()) for f in flags[g]), (t, g)
    assert all(pos[g] == len(idx[g]) for g in range(G))
    return [np.concatenate(f) for f in flags], rk


def one_shot(qf, k, idx, co, r=0):
    """qf_rank_batch over the whole sequences."""
    G, mr = len(idx), max(len(x) for x in idx)
    a_idx = np.full((G, mr), FILL16, np.uint16)
    a_co = np.full((G, mr, k), FILL, np.uint8)
    n = np.array([len(x) for x in idx], np.uint32)
    for g in range(G):
        a_idx[g, : n[g]] = idx[g]
        if co is not None:
            a_co[g, : n[g]] = co[g]
    t_fl, t_rk, t_st = _filled(G * mr), _filled(4 * G), _filled(4 * G)
    qf.rank_batch(_dev(a_idx), t_rk, t_st, k, r=r, max_rows=mr, G=G, n_rows=_dev(n),
                  row_coeffs=_dev(a_co) if co is not None else None, innovative=t_fl)
    qf.default_context().sync()
    assert (_host(t_st, np.int32) == OK).all()
    fl = _host(t_fl).reshape(G, mr)
    return [fl[g, : n[g]].copy() for g in range(G)], _host(t_rk, np.uint32).copy()


def check_all_splits(qf, k, idx, co, ref_flags, ref_rank, splits, r=0):
    G = len(idx)
    n = [len(x) for x in idx]
    dev_flags, dev_rank = one_shot(qf, k, idx, co, r)
    ways = [("one call", [[n[g]] for g in range(G)]),
            ("one slot per call", [[1] * n[g] + [0] * (max(n) - n[g]) for g in range(G)])]
    ways += [(f"split {j}", s) for j, s in enumerate(splits)]
    for name, counts in ways:
        flags, rank = feed(States(qf, G, k), idx, co, counts, r=r)
        for g in range(G):
            assert np.array_equal(flags[g], ref_flags[g]), (name, g, flags[g].tolist(), ref_flags[g].tolist())
            assert np.array_equal(flags[g], dev_flags[g]), (name, g)
            assert rank[g] == ref_rank[g] == dev_rank[g], (name, g, rank[g], ref_rank[g], dev_rank[g])


@pytest.mark.parametrize("k", store_ref.STREAM_K)
def test_split_invariance(qf, oracle, gpu_ctx, k):
    case = store_ref.stream_case(k)
    for g in range(case["G"]):
        rk, fl = qf.gf_rank(store_ref.vectors_of(k, case["idx"][g], case["co"][g]), k)
        assert rk == case["rank"][g] and fl == case["flags"][g].tolist(), g
    assert any(rk == k for rk in case["rank"])
    check_all_splits(qf, k, case["idx"], case["co"], case["flags"], case["rank"], case["splits"])


def test_split_invariance_cauchy_rows_without_vectors(qf, oracle, gpu_ctx):
    k, r, G = 8, 6, 3
    rng = np.random.default_rng(86)
    idx = [store_ref.cauchy_arrival(rng, k, r) for _ in range(G)]
    C = oracle.cauchy(k, r)
    refs = [rank_ref.innovative(rank_ref.vectors(k, r, x.astype(np.int64), None, C)) for x in idx]
    assert all(rk == k for _, rk in refs) and all(not f.all() for f, _ in refs)
    assert any(0 < f[:k].sum() < k for f, _ in refs)
    splits = [store_ref.cuts(np.random.default_rng(860 + j), [len(x) for x in idx], store_ref.STREAM_CALLS) for j in range(3)]
    check_all_splits(qf, k, idx, None, [f for f, _ in refs], [rk for _, rk in refs], splits, r=r)
    # a state may see calls with and without vectors: the Cauchy rows given explicitly half of the time
    st = States(qf, G, k)
    flags = [[] for _ in range(G)]
    for t, lo in enumerate(range(0, 16, 4)):
        part = [x[lo: lo + 4] for x in idx]
        co = [np.stack([C[i - k] if i >= k else np.eye(k, dtype=np.uint8)[i] for i in p]) for p in part] if t % 2 else None
        fl, rk, status = st.update(part, co, r=r, mr=4 + t)
        assert (status == OK).all()
        for g in range(G):
            flags[g].append(fl[g])
    for g in range(G):
        assert np.array_equal(np.concatenate(flags[g]), refs[g][0]) and rk[g] == k, g


def test_chunk_loop_resumes_from_restored_state(qf, oracle, gpu_ctx):
    """max_rows = 70 in the second call: its first 64 slots leave the rank
    short of k (34 of them repeat the first call's and their own rows), so the
    walk's second chunk starts from the restored span plus the first chunk's."""
    k = 64
    case = store_ref.stream_case(k)
    G = case["G"]
    order = np.concatenate([np.arange(0, 40), np.arange(0, 34), np.arange(40, 46)])
    idx = [case["idx"][g][order] for g in range(G)]
    co = [case["co"][g][order] for g in range(G)]
    refs = [rank_ref.innovative(store_ref.vectors_of(k, idx[g], co[g])) for g in range(G)]
    assert all(f[10 + 64:].any() and not f[40:74].any() for f, _ in refs), "the second chunk brings nothing new"
    flags, rank = feed(States(qf, G, k), idx, co, [[10, 70]] * G, mr=70)
    dev_flags, dev_rank = one_shot(qf, k, idx, co)
    for g in range(G):
        assert np.array_equal(flags[g], refs[g][0]) and rank[g] == refs[g][1] < k, g
        assert np.array_equal(flags[g], dev_flags[g]) and rank[g] == dev_rank[g], g


def test_classic_mistakes_across_a_call_boundary(qf, oracle, gpu_ctx):
    k = 8
    pair = np.zeros(k, np.uint8)
    pair[2], pair[7] = 1, 1
    late = np.zeros(k, np.uint8)
    late[5:] = [0x53, 0x07, 0xE1]                              # first nonzero: column 5
    unit = lambda i: np.eye(k, dtype=np.uint8)[i]             # noqa: E731
    st = States(qf, 2, k)
    calls = [([k], pair[None], [k], late[None], [1, 1]),      # coded e2 + e7          | coded, pivot 5 at best
             ([2], unit(2)[None], [5], unit(5)[None], [1, 1]),   # systematic 2: new   | systematic 5: new
             ([7], unit(7)[None], [k], late[None], [0, 0])]      # systematic 7: spanned | the same coded row again
    for t, (i0, c0, i1, c1, want) in enumerate(calls):
        fl, rk, status = st.update([np.array(i0, np.uint16), np.array(i1, np.uint16)], [c0, c1])
        assert (status == OK).all()
        assert [int(fl[0][0]), int(fl[1][0])] == want, (t, fl)
        assert rk.tolist() == [min(t + 1, 2)] * 2, (t, rk)
    # the same three rows per generation in one call of qf_rank_batch
    fl, rk = one_shot(qf, k, [np.array([k, 2, 7], np.uint16), np.array([k, 5, k], np.uint16)],
                      [np.stack([pair, unit(2), unit(7)]), np.stack([late, unit(5), late])])
    assert fl[0].tolist() == [1, 1, 0] and fl[1].tolist() == [1, 1, 0] and rk.tolist() == [2, 2]


def test_state_handling(qf, oracle, gpu_ctx):
    k = 8
    case = store_ref.stream_case(k)
    G, idx, co = case["G"], case["idx"], case["co"]
    st = States(qf, G, k)
    assert not st.bytes().any()
    # an empty call on empty states: nothing written, rank 0
    fl, rk, status = st.update([x[:0] for x in idx], [c[:0] for c in co], mr=3)
    assert (status == OK).all() and not rk.any() and not st.bytes().any()
    fl, rk, status = st.update([x[:5] for x in idx], [c[:5] for c in co])
    want = [int(case["flags"][g][:5].sum()) for g in range(G)]
    assert (status == OK).all() and rk.tolist() == want and all(0 < w < k for w in want)
    snap = st.bytes()
    assert all(snap[g].any() for g in range(G))
    # n = 0: the state bytes stay, the rank is reported
    fl, rk, status = st.update([x[:0] for x in idx], [c[:0] for c in co], mr=2)
    assert (status == OK).all() and rk.tolist() == want and np.array_equal(st.bytes(), snap)
    # NULL n_rows means max_rows slots each
    st2 = States(qf, G, k)
    fl2, rk2, _ = st2.update([x[:5] for x in idx], [c[:5] for c in co], pass_n=False)
    assert rk2.tolist() == want and np.array_equal(st2.bytes(), snap)
    # a slot that breaks its "needs" (index - k >= 256) in generation 1: its slots are
    # ignored as a whole, the state stays, the prior rank is reported; the others go on
    bad = [x[5:9].copy() for x in idx]
    bad[1][2] = k + 256
    fl, rk, status = st.update(bad, [c[5:9] for c in co])
    assert status.tolist() == [OK, EINVAL, OK][:G] and rk[1] == want[1] and not fl[1].any()
    now = st.bytes()
    assert np.array_equal(now[1], snap[1])
    for g in (0, 2):
        assert np.array_equal(fl[g], case["flags"][g][5:9]) and rk[g] == int(case["flags"][g][:9].sum()), g
    # generation 1 again without the bad slot, then the rest: the reference's flags throughout
    fl, rk, status = st.update([x[9:9] if g != 1 else x[5:9] for g, x in enumerate(idx)],
                               [c[9:9] if g != 1 else c[5:9] for g, c in enumerate(co)])
    assert (status == OK).all() and np.array_equal(fl[1], case["flags"][1][5:9])
    fl, rk, status = st.update([x[9:] for x in idx], [c[9:] for c in co])
    for g in range(G):
        assert np.array_equal(fl[g], case["flags"][g][9:]) and rk[g] == case["rank"][g] == k, g
    # the rank has reached k: every later flag is 0, the rank stays, and so does the state
    full = st.bytes()
    fl, rk, status = st.update([x[:6] for x in idx], [c[:6] for c in co])
    assert (status == OK).all() and (rk == k).all() and not any(f.any() for f in fl)
    assert np.array_equal(st.bytes(), full)
    # zeroing one generation's state resets that generation only
    st.t[st.sb: 2 * st.sb] = 0
    fl, rk, status = st.update([x[:6] for x in idx], [c[:6] for c in co])
    assert (status == OK).all() and rk[0] == k and rk[2] == k and not fl[0].any() and not fl[2].any()
    assert np.array_equal(fl[1], case["flags"][1][:6]) and rk[1] == int(case["flags"][1][:6].sum())
    after = st.bytes()
    assert np.array_equal(after[0], full[0]) and np.array_equal(after[2], full[2])


def test_invalid_states(qf, oracle, gpu_ctx):
    k = 8
    case = store_ref.stream_case(k)
    idx, co = case["idx"][0], case["co"][0]
    # a state written at k = 8 and passed with k = 12
    st = States(qf, 1, k, room=qf.rank_state_bytes(12))
    fl, rk, status = st.update([idx[:6]], [co[:6]])
    assert status[0] == OK and rk[0] > 0
    snap = st.bytes()
    co12 = np.zeros((3, 12), np.uint8)
    co12[:, :3] = np.eye(3, dtype=np.uint8)
    fl, rk, status = st.update([np.array([0, 1, 2], np.uint16)], [co12], k=12)
    assert status[0] == EINVAL and rk[0] == 0 and not fl[0].any()
    assert np.array_equal(st.bytes(), snap)
    # ... and with no slot in the call: the header alone decides
    fl, rk, status = st.update([idx[:0]], [co12[:0]], k=12, mr=2)
    assert status[0] == EINVAL and rk[0] == 0 and np.array_equal(st.bytes(), snap)
    # a state of 0xCC bytes beside a good one
    st = States(qf, 2, k)
    st.t[st.sb: 2 * st.sb] = FILL
    fl, rk, status = st.update([idx[:6], idx[:6]], [co[:6], co[:6]])
    assert status.tolist() == [OK, EINVAL] and rk[1] == 0 and not fl[1].any()
    assert np.array_equal(fl[0], case["flags"][0][:6])
    assert (st.bytes()[1] == FILL).all()
    # a good header over pivot columns at or above k: refused by the range check
    st = States(qf, 1, k)
    two = np.array([[3, 0, 9, 0, 0, 7, 0, 1], [0, 5, 0, 0, 2, 0, 8, 0]], np.uint8)
    fl, rk, status = st.update([np.array([k, k], np.uint16)], [two])
    assert status[0] == OK and rk[0] == 2
    st.t[48: 48 + 16] = 0xF0
    snap = st.bytes()
    fl, rk, status = st.update([idx[:4]], [co[:4]])
    assert status[0] == EINVAL and rk[0] == 0 and not fl[0].any() and np.array_equal(st.bytes(), snap)


# ---------------------------------------------------------------------------
# row store
# ---------------------------------------------------------------------------
class DevStore:
    """The device side of store_ref.Store: the same arrays, 0xCC, plus 64 bytes
    of 0xCC behind each."""

    def __init__(self, qf, ref):
        import torch

        self.qf, self.ref = qf, ref
        G, cap, k = ref.G, ref.cap, ref.k
        self.bytes = _filled(G * ref.gen_stride + 64)
        self.off, self.len = _filled(4 * G * cap + 64), _filled(4 * G * cap + 64)
        self.index, self.coeffs = _filled(2 * G * cap + 64), _filled(G * cap * k + 64)
        self.n = torch.zeros(G, dtype=torch.int32, device="cuda")

    def append(self, src, sgs, ro, rl, idx, co, n=None, take=None, mr=None):
        """Device tensors in; -> status (G,).  mr: input slots per generation."""
        ref = self.ref
        t_st = _filled(4 * ref.G + 16)
        self.qf.store_append(src, ro, rl, idx, co, self.bytes, self.off, self.len, self.index, self.coeffs, self.n, t_st,
                             ref.k, ref.L, max_rows=mr, cap=ref.cap, src_gen_stride=sgs, store_row_stride=ref.row_stride,
                             store_gen_stride=ref.gen_stride, G=ref.G, n_rows=n, take=take)
        self.qf.default_context().sync()
        st = _host(t_st, np.int32)
        assert (st[ref.G:].view(np.uint32) == FILL32).all()
        return st[: ref.G].copy()

    def check(self):
        """Every byte of every store array is the reference's."""
        ref = self.ref
        G, cap, k = ref.G, ref.cap, ref.k
        for name, t, dt, want in (("bytes", self.bytes, np.uint8, ref.bytes), ("off", self.off, np.uint32, ref.off),
                                  ("len", self.len, np.uint32, ref.len), ("index", self.index, np.uint16, ref.index),
                                  ("coeffs", self.coeffs, np.uint8, ref.coeffs)):
            h = _host(t)
            body = want.size * want.itemsize
            assert (h[body:] == FILL).all(), f"bytes behind store {name} were written"
            got = h[:body].view(dt).reshape(want.shape)
            bad = np.argwhere(got != want)
            assert bad.size == 0, f"store {name} differs at {bad[:4].tolist()}"
        assert np.array_equal(_host(self.n, np.uint32), ref.n), (_host(self.n, np.uint32), ref.n)


def rows_in_slots(rng, k, Lb, idx_calls, lens):
    """One call's rows as qf_parse_frame_headers_dev leaves them: generation g
    has the slots idx_calls[g]; row s lies at byte P of slot s of a region of
    mr slots of P + round_up(L, 16) bytes, 0xCC outside its bytes -> region
    (G, mr * fs), row_off, row_len (G, mr), mr, fs."""
    G = len(idx_calls)
    mr = max(1, max(len(x) for x in idx_calls))
    P = _P(k)
    fs = P + _r16(Lb)
    region = np.full((G, mr, fs), FILL, np.uint8)
    ro = np.full((G, mr), FILL32, np.uint32)
    rl = np.full((G, mr), FILL32, np.uint32)
    c = 0
    for g in range(G):
        for s in range(len(idx_calls[g])):
            ln = lens[(c // 2) % len(lens)] if c % 2 else int(rng.integers(0, Lb + 1))
            c += 1
            region[g, s, P: P + ln] = rng.integers(0, 256, ln, dtype=np.uint8)
            ro[g, s], rl[g, s] = s * fs + P, ln
    return region.reshape(G, mr * fs), ro, rl, mr, fs


@pytest.mark.parametrize("use_flags", [False, True], ids=["take_null", "take_flags"])
@pytest.mark.parametrize("k,Lb", [(8, 100), (64, 1200)])
def test_append_against_the_reference(qf, oracle, gpu_ctx, k, Lb, use_flags):
    case = store_ref.stream_case(k)
    G, idx, co = case["G"], case["idx"], case["co"]
    n_all = [len(x) for x in idx]
    rng = np.random.default_rng(k * 31 + Lb + use_flags)
    counts = store_ref.cuts(rng, n_all, 3)
    cap = k if use_flags else max(n_all)
    ref = store_ref.Store(G, k, Lb, cap, gen_gap=48)
    dev = DevStore(qf, ref)
    st = States(qf, G, k)
    lens = [0, 1, 15, 16, 17, Lb]
    seen_lens = set()
    pos = [0] * G
    for t in range(3):
        part = [idx[g][pos[g]: pos[g] + counts[g][t]] for g in range(G)]
        cpart = [co[g][pos[g]: pos[g] + counts[g][t]] for g in range(G)]
        region, ro, rl, mr, fs = rows_in_slots(rng, k, Lb, part, lens)
        seen_lens |= set(rl[rl != FILL32].tolist())
        a_idx = np.full((G, mr), FILL16, np.uint16)
        a_co = np.full((G, mr, k), FILL, np.uint8)
        n = np.array([len(p) for p in part], np.uint32)
        for g in range(G):
            a_idx[g, : n[g]] = np.minimum(part[g], k)
            a_co[g, : n[g]] = cpart[g]
        take, t_take = None, None
        if use_flags:
            fl, rk, status = st.update(part, cpart, mr=mr)
            take = np.full((G, mr), FILL, np.uint8)               # (bytes behind n are not looked at)
            for g in range(G):
                take[g, : n[g]] = fl[g]
                assert np.array_equal(fl[g], case["flags"][g][pos[g]: pos[g] + counts[g][t]]), (t, g)
            t_take = _dev(take)
        want = ref.append(region, mr * fs, ro, rl, a_idx, a_co, n, take)
        t_src = _dev(region)
        got = dev.append(t_src, mr * fs, _dev(ro), _dev(rl), _dev(a_idx), _dev(a_co), _dev(n), t_take, mr=mr)
        assert np.array_equal(got, want) and (got == OK).all(), (t, got, want)
        assert np.array_equal(_host(t_src), region.reshape(-1)), "the source was written"
        dev.check()
        for g in range(G):
            pos[g] += counts[g][t]
    if use_flags:
        assert ref.n.tolist() == case["rank"]
    else:
        assert ref.n.tolist() == n_all
    assert {0, 1, 15, 16, 17, Lb} <= seen_lens
    if not use_flags:
        assert {0, 1, 15, 16, 17, Lb} <= set(ref.len[ref.len != FILL32].tolist())


def test_append_refusals_leave_the_generation_untouched(qf, oracle, gpu_ctx):
    k, Lb, mr, cap, G = 8, 100, 6, 3, 5
    rng = np.random.default_rng(5100)
    P = _P(k)
    fs = P + _r16(Lb)
    sgs = mr * fs
    ref = store_ref.Store(G, k, Lb, cap)
    dev = DevStore(qf, ref)

    def call(take, n=None, edit=None):
        region = np.full((G, mr, fs), FILL, np.uint8)
        ro = np.tile((np.arange(mr, dtype=np.uint32) * fs + P), (G, 1))
        rl = rng.integers(0, Lb + 1, (G, mr)).astype(np.uint32)
        for g in range(G):
            for s in range(mr):
                region[g, s, P: P + rl[g, s]] = rng.integers(0, 256, int(rl[g, s]), dtype=np.uint8)
        if edit:
            edit(ro, rl)
        idx = rng.integers(0, k + 1, (G, mr)).astype(np.uint16)
        co = rng.integers(0, 256, (G, mr, k), dtype=np.uint8)
        region = region.reshape(G, sgs)
        nn = None if n is None else np.array(n, np.uint32)
        want = ref.append(region, sgs, ro, rl, idx, co, nn, take)
        got = dev.append(_dev(region), sgs, _dev(ro), _dev(rl), _dev(idx), _dev(co), None if nn is None else _dev(nn),
                         _dev(take), mr=mr)
        assert np.array_equal(got, want), (got, want)
        dev.check()
        return got

    def bad_rows(ro, rl):
        rl[2, 1] = Lb + 1                  # taken, longer than L
        ro[3, 4] += 8                      # taken, not at a multiple of 16
        ro[4, 5], rl[4, 5] = sgs - 16, 17  # taken, ends behind the generation's region
        rl[0, 2] = Lb + 1                  # not taken: nobody looks
        ro[0, 3] += 8

    take = np.zeros((G, mr), np.uint8)
    take[0, [0, 5]] = 1
    take[1, [0, 1, 2, 4]] = 1              # four rows into three slots
    take[2, [1, 3]] = 1
    take[3, [4]] = 1
    take[4, [0, 5]] = 1
    got = call(take, edit=bad_rows)
    assert got.tolist() == [OK, ETOOSMALL, EINVAL, EINVAL, EINVAL] and ref.n.tolist() == [2, 0, 0, 0, 0]
    # the refused generations take rows afterwards; generation 0 fills up
    take = np.zeros((G, mr), np.uint8)
    take[:, 1] = 1
    take[1, 3] = 1
    got = call(take)
    assert (got == OK).all() and ref.n.tolist() == [3, 2, 1, 1, 1]
    # full: one more row is refused, none is fine; a count above max_rows is QF_EINVAL
    take = np.zeros((G, mr), np.uint8)
    take[0, 0] = 1
    take[2, :] = 1
    take[3, 2] = 1
    got = call(take, n=[mr, mr, mr + 1, 3, 0])
    assert got.tolist() == [ETOOSMALL, OK, EINVAL, OK, OK] and ref.n.tolist() == [3, 2, 1, 2, 1]


# ---------------------------------------------------------------------------
# polls end to end
# ---------------------------------------------------------------------------
def shape_a_gens(oracle, rng, k, Lb, G, r):
    """DESIGN 3.10's shape (a) scaled to k (at k = 64: 51 systematic rows and
    26 coded ones, at least 13 sources erased and at most 26, when the rank is
    reached before the last systematic rows), plus repeats of systematic rows and
    combinations of earlier rows, shuffled; the last generation stops two rows
    short of k.  -> K.Gens (a coded row has index k)."""
    e = max(2, 13 * k // 64)
    few = max(1, k // 16)
    mr = (k - e) + 2 * e + 2 * few
    idx = np.full((G, mr), k, np.uint16)
    co = np.zeros((G, mr, k), np.uint8)
    for g in range(G):
        have = [int(x) for x in rng.permutation(k)[: k - e]]
        kinds = [("sys", i) for i in have] + [("sys", have[int(rng.integers(0, len(have)))]) for _ in range(few)]
        kinds += [("rnd", None)] * (2 * e) + [("dep", None)] * few
        for s, j in enumerate(rng.permutation(mr)):
            kind, i = kinds[int(j)]
            if kind == "sys":
                idx[g, s] = i
                co[g, s, i] = 1
            elif kind == "rnd" or s < 2:
                co[g, s] = rng.integers(0, 256, k)
            else:
                p, q = (int(x) for x in rng.choice(s, 2, replace=False))
                co[g, s] = store_ref._scale(oracle, co[g, p], 0x35) ^ store_ref._scale(oracle, co[g, q], 0xB2)
    n = np.full(G, mr, np.uint32)
    n[G - 1] = k - 2
    return K.Gens(oracle, k, r, Lb, recv_ref.tailed_sources(rng, G, k, Lb), idx, n, co)


def poll_of(oracle, rx, lo, hi):
    """The frames [lo[g], hi[g]) of every generation as one poll's buffer."""
    G = rx.G
    mr = max(1, max(hi[g] - lo[g] for g in range(G)))
    p = R.Received(oracle, None, rx.k, rx.L, mr, rx.fs, [[] for _ in range(G)], [rx.L])
    for g in range(G):
        c = hi[g] - lo[g]
        p.frames[g, :c], p.flen[g, :c] = rx.frames[g, lo[g]: hi[g]], rx.flen[g, lo[g]: hi[g]]
        p.foff[g, :c], p.ids[g, :c] = rx.foff[g, lo[g]: hi[g]], rx.ids[g, lo[g]: hi[g]]
        p.nfr[g] = c
    return p


def run_polls(qf, oracle, rx, gs, counts, cap):
    """parse headers -> update -> append per poll -> the store (reference and
    device side) and the last ranks."""
    G, k, Lb = gs.G, gs.k, gs.L
    ref = store_ref.Store(G, k, Lb, cap)
    dev = DevStore(qf, ref)
    st = States(qf, G, k)
    pos = [0] * G
    rk = None
    for t in range(len(counts[0])):
        hi = [pos[g] + counts[g][t] for g in range(G)]
        p = poll_of(oracle, rx, pos, hi)
        h = R.run_headers(qf, p)
        n = _host(h["n"], np.uint32)[:G]
        assert n.tolist() == [counts[g][t] for g in range(G)]
        t_fl, t_rk, t_st = _filled(G * p.mr + 64), _filled(4 * G + 16), _filled(4 * G + 16)
        qf.rank_update_batch(h["idx"], st.t, t_rk, t_st, k, max_rows=p.mr, G=G, n_rows=h["n"], row_coeffs=h["co"],
                             innovative=t_fl)
        status = dev.append(h["frames"], p.mr * p.fs, h["ro"], h["rl"], h["idx"], h["co"], h["n"], t_fl, mr=p.mr)
        assert (status == OK).all() and (_host(t_st, np.int32)[:G] == OK).all()
        fl = _host(t_fl)[: G * p.mr].reshape(G, p.mr)
        rk = _host(t_rk, np.uint32)[:G].copy()
        for g in range(G):
            assert np.array_equal(fl[g, : n[g]], gs.flags[g][pos[g]: hi[g]]), (t, g)
        # the reference append over the parser's outputs
        take = fl.copy()
        ref.append(p.frames.reshape(G, -1), p.mr * p.fs, _host(h["ro"], np.uint32)[: G * p.mr].reshape(G, p.mr),
                   _host(h["rl"], np.uint32)[: G * p.mr].reshape(G, p.mr),
                   _host(h["idx"], np.uint16)[: G * p.mr].reshape(G, p.mr),
                   _host(h["co"])[: G * p.mr * k].reshape(G, p.mr, k), n, take)
        dev.check()
        pos = hi
    assert pos == [int(x) for x in gs.n]
    return ref, dev, rk


@pytest.mark.parametrize("k,Lb,G,r", [(8, 100, 5, 4), (64, 1200, 3, 32)])
def test_polls_then_decode_from_the_store(qf, oracle, gpu_ctx, k, Lb, G, r):
    rng = np.random.default_rng(k * 1000 + Lb)
    gs = shape_a_gens(oracle, rng, k, Lb, G, r)
    assert all(gs.rank[g] == k for g in range(G - 1)) and gs.rank[G - 1] < k
    assert all(not gs.flags[g][: gs.n[g]].all() for g in range(G - 1)), "no dependent row"
    rx, lens = I.frame_gens(oracle, gs)
    counts = store_ref.cuts(np.random.default_rng(k + 4), [int(x) for x in gs.n], 4)
    ref, dev, rk = run_polls(qf, oracle, rx, gs, counts, cap=k)
    assert rk.tolist() == gs.rank and ref.n.tolist() == gs.rank
    # one shot over all frames in arrival order
    one = I.run_inplace(qf, rx, R.run_headers(qf, rx), r)
    # ... and over the store
    em = min(k, r)
    rec_rs = _r16(Lb) + 16
    rec_gs = em * rec_rs
    t = I._outputs(G, k, em, k, rec_gs)
    qf.decode_frames(dev.bytes, dev.off, dev.len, dev.index, dev.coeffs, t["rec"], t["ri"], t["nrec"], t["st"], k, r, Lb,
                     max_rows=k, src_gen_stride=ref.gen_stride, rec_row_stride=rec_rs, rec_gen_stride=rec_gs, G=G,
                     n_rows=dev.n, rank=t["rank"], innovative=t["flags"], src_slot=t["slot"])
    qf.default_context().sync()
    dev.check()                                                # the store was not written
    out = I._collect(t, G, k, em, k, Lb, rec_rs, rec_gs, ("rank", "flags", "slot"))
    for key in ("rec", "ri", "nrec", "st", "rank"):
        assert np.array_equal(out[key], one[key]), f"{key} differs from the one-shot decode"
    assert out["st"].tolist() == [OK] * (G - 1) + [ENOTREADY]
    for g in range(G):
        # the store holds innovative rows only: its own filter takes them all
        assert out["flags"][g, : ref.n[g]].all() and not out["flags"][g, ref.n[g]:].any(), g
    # every source packet is the original
    for g in range(G - 1):
        rix = out["ri"][g, : out["nrec"][g]].tolist()
        assert 0 < len(rix) <= em
        for i in range(k):
            c = int(out["slot"][g, i])
            pkt = np.zeros(Lb, np.uint8)
            if c == NONE16:
                pkt[:] = out["rec"][g, rix.index(i)]
            else:
                assert ref.index[g, c] == i
                pkt[: ref.len[g, c]] = ref.bytes[g, ref.off[g, c]: ref.off[g, c] + ref.len[g, c]]
            assert np.array_equal(pkt, gs.src[g, i]), (g, i)


def test_polls_then_recode_from_the_store(qf, oracle, gpu_ctx):
    k, Lb, G, m = 8, 100, 3, 5
    rng = np.random.default_rng(8100)
    gs = shape_a_gens(oracle, rng, k, Lb, G, 4)
    rx, lens = I.frame_gens(oracle, gs)
    counts = store_ref.cuts(np.random.default_rng(12), [int(x) for x in gs.n], 4)
    ref, dev, rk = run_polls(qf, oracle, rx, gs, counts, cap=k)
    # the one-shot buffer: the innovative frames only, in the same order
    keep = [np.flatnonzero(gs.flags[g][: gs.n[g]]) for g in range(G)]
    mr2 = max(len(x) for x in keep)
    inn = R.Received(oracle, None, k, Lb, mr2, rx.fs, [[] for _ in range(G)], [Lb])
    for g in range(G):
        c = len(keep[g])
        inn.frames[g, :c], inn.flen[g, :c] = rx.frames[g, keep[g]], rx.flen[g, keep[g]]
        inn.foff[g, :c], inn.ids[g, :c] = rx.foff[g, keep[g]], rx.ids[g, keep[g]]
        inn.nfr[g] = c
    h = R.run_headers(qf, inn)
    assert _host(h["n"], np.uint32)[:G].tolist() == gs.rank
    M = rng.integers(0, 256, (G, m, k), dtype=np.uint8)
    ors = _r16(Lb) + 16

    def recode(src, ro, rl, idx, co, n, mr, sgs):
        mix = np.zeros((G, m, mr), np.uint8)
        mix[:, :, : min(mr, k)] = M[:, :, : min(mr, k)]
        t_out, t_oc, t_ol, t_st = _filled(G * m * ors + 64), _filled(G * m * k + 64), _filled(4 * G * m + 16), _filled(4 * G + 16)
        qf.recode_frames(src, ro, rl, idx, co, t_out, t_oc, t_st, k, m, Lb, max_rows=mr, src_gen_stride=sgs,
                         out_row_stride=ors, out_gen_stride=m * ors, G=G, n_rows=n, mix=_dev(mix), out_len=t_ol)
        qf.default_context().sync()
        return _host(t_out).copy(), _host(t_oc).copy(), _host(t_ol).copy(), _host(t_st, np.int32).copy()

    a = recode(dev.bytes, dev.off, dev.len, dev.index, dev.coeffs, dev.n, k, ref.gen_stride)
    b = recode(h["frames"], h["ro"], h["rl"], h["idx"], h["co"], h["n"], mr2, mr2 * rx.fs)
    for name, x, y in zip(("out", "out_coeffs", "out_len", "status"), a, b):
        assert np.array_equal(x, y), f"{name} differs from the recode over the innovative frames"
    assert (a[3][:G] == OK).all() and a[0][: Lb].any()
    dev.check()


def test_profile_names(qf, oracle, gpu_ctx):
    k, Lb, G = 8, 100, 2
    rng = np.random.default_rng(3)
    region, ro, rl, mr, fs = rows_in_slots(rng, k, Lb, [np.arange(3), np.arange(2)], [Lb])
    ref = store_ref.Store(G, k, Lb, k)
    dev = DevStore(qf, ref)
    st = States(qf, G, k)
    idx = np.tile(np.arange(mr, dtype=np.uint16), (G, 1))
    co = np.tile(np.eye(k, dtype=np.uint8)[:mr], (G, 1, 1))
    gpu_ctx.sync()
    gpu_ctx.profile(True)
    st.update([idx[0, :3], idx[1, :2]], [co[0, :3], co[1, :2]])
    dev.append(_dev(region), mr * fs, _dev(ro), _dev(rl), _dev(idx), _dev(co), _dev(np.array([3, 2], np.uint32)), None, mr=mr)
    times = gpu_ctx.kernel_times()
    gpu_ctx.profile(False)
    assert sorted(times) == ["k_rank_update", "k_store_prepare", "k_store_rows"], times
    assert all(v[0] == 1 for v in times.values()), times
