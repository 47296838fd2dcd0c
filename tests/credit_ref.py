"""Reference of qf_rank_report_sel_dev and qf_credit_update_dev -- TEST
INFRASTRUCTURE ONLY.

Both calls restated in plain numpy from the rules written in include/qf_fec.h
above them (the ids need all 64 bits, so that arithmetic is done on Python
ints).  Nothing here touches the library under test.

ReportCall:   the inputs of one qf_rank_report_sel_dev call and model(), which
              returns every output buffer whole, as the call leaves it when it
              starts from `before` (default: every byte 0xCC).
CreditCall:   the same for qf_credit_update_dev (the state and the credit are
              both read and written).
report_cases, credit_cases, credit_sequences: the named calls of the device
              test and of the host-emulation test.
lossy_loop:   emit_ref.loop_model with a drop mask on the second hop, the
              receiver's two report lists every poll, the relay's credit update
              and empty polls until nothing is left to send."""
from __future__ import annotations

import functools

import numpy as np

from tests import emit_ref as E

OK, EINVAL, ENOTREADY, ESTALE = 0, -1, -3, -8
FILL = 0xCC
FILL32 = 0xCCCCCCCC
U64MAX = (1 << 64) - 1
ID_LIMIT = 1 << 62
CLOSED = 1 << 63
REPORT = np.dtype([("id", "<u8"), ("rank", "<u4"), ("reserved", "<u4")])
STATE = np.dtype([("owner", "<u8"), ("peer", "<u4"), ("reserved", "<u4")])
assert REPORT.itemsize == 16 and STATE.itemsize == 16


def held(entry: int) -> int:
    """id + 1 of a window entry, 0 for an empty one."""
    return int(entry) & ~CLOSED


def ceil_rho(x: int, num: int, den: int) -> int:
    return -(-x * num // den)


def records(rows) -> np.ndarray:
    """[(id, rank, reserved), ...] -> an array of reports."""
    a = np.zeros(len(rows), REPORT)
    for i, (x, r, z) in enumerate(rows):
        a[i] = (x, r, z)
    return a


def poisoned(n: int, dt) -> np.ndarray:
    return np.full(n * np.dtype(dt).itemsize, FILL, np.uint8).view(dt)


# ---------------------------------------------------------------------------
# qf_rank_report_sel_dev
# ---------------------------------------------------------------------------
class ReportCall:
    def __init__(self, k, sel, win, rank, N_max, n_sel=None, append=False):
        self.k, self.N_max, self.n_sel, self.append = k, N_max, n_sel, append
        self.sel = np.asarray(sel, np.uint32)
        self.win = np.asarray(win, np.uint64)
        self.rank = np.asarray(rank, np.uint32)
        self.n_max, self.G_src = len(self.sel), len(self.win)

    def blank(self, n_reports: int = FILL32) -> dict:
        return dict(reports=poisoned(self.N_max, REPORT), n_reports=np.array([n_reports], np.uint32),
                    n_left=np.full(1, FILL32, np.uint32))

    def model(self, before: dict | None = None) -> dict:
        o = {key: v.copy() for key, v in (before or self.blank()).items()}
        n = self.n_max if self.n_sel is None else min(int(self.n_sel), self.n_max)
        base = min(int(o["n_reports"][0]), self.N_max) if self.append else 0
        for j in range(n):
            if base + j >= self.N_max:
                break
            s = int(self.sel[j])
            rec = (U64MAX, 0, 0)
            if s < self.G_src and int(self.win[s]) != 0:
                w = int(self.win[s])
                rec = (held(w) - 1, self.k if w & CLOSED else min(int(self.rank[s]), self.k), 0)
            o["reports"][base + j] = rec
        o["n_reports"][0] = min(base + n, self.N_max)
        o["n_left"][0] = base + n - min(base + n, self.N_max)
        return o


def random_window(rng, G: int, base: int | None = None):
    """-> win (G,) u64 with empty, open and closed entries, each slot's id in cycle 1 of the ring."""
    base = ((1 << 40) // G + 1) * G if base is None else base
    kind = rng.integers(0, 3, G)
    kind[: min(3, G)] = [1, 0, 2][: min(3, G)]                # every kind where there is room
    win = np.zeros(G, np.uint64)
    for s in range(G):
        x = base + G + s + 1
        win[s] = 0 if kind[s] == 0 else x if kind[s] == 1 else x | CLOSED
    return win, base


def make_report(k, n_max, G, N_max, seed, **kw) -> ReportCall:
    """A shuffled list over a random window with a duplicate, an entry >= G_src, ranks 0 .. k + 2."""
    rng = np.random.default_rng(seed)
    win, _ = random_window(rng, G)
    rank = rng.integers(0, k + 3, G).astype(np.uint32)
    rank[0] = k + 2
    sel = rng.integers(0, G, n_max).astype(np.uint32)
    head = [0, 1 % G, 2 % G, G + 3, 0, 0xFFFFFFFF][: n_max]
    sel[: len(head)] = head
    return ReportCall(k, rng.permutation(sel), win, rank, N_max, **kw)


def report_cases() -> dict:
    """name -> (call, the buffers it starts from, n_left given)."""
    c = {}
    for n_max in (1, 64, 65):
        x = make_report(4, n_max, 23, n_max + 2, 100 + n_max)
        c[f"n_max{n_max}"] = (x, x.blank(), True)
    x = make_report(256, 65, 130, 100, 110, n_sel=0)
    c["n_sel_0"] = (x, x.blank(), True)
    x = make_report(64, 65, 130, 100, 111, n_sel=30)
    c["n_sel_mid"] = (x, x.blank(), False)
    x = make_report(1, 65, 7, 100, 112, n_sel=1000)
    c["n_sel_above_n_max"] = (x, x.blank(), True)
    x = make_report(4, 20, 23, 12, 113)
    c["overflow"] = (x, x.blank(5), True)                  # without append a stale length is ignored
    for name, base in dict(base0=0, base_mid=7, base_fits=10, base_full=30, base_above=1000).items():
        x = make_report(4, 20, 23, 30, 120, append=True)
        c[f"append_{name}"] = (x, x.blank(base), name != "base_mid")
    return c


# ---------------------------------------------------------------------------
# qf_credit_update_dev
# ---------------------------------------------------------------------------
class CreditCall:
    def __init__(self, k, num, den, cap, win, rank, sent, reports=None, n_reports=None, N_max=None, status=True):
        self.k, self.num, self.den, self.cap = k, num, den, cap
        self.win = np.asarray(win, np.uint64)
        self.rank = np.asarray(rank, np.uint32)
        self.sent = np.asarray(sent, np.uint32)
        self.G = len(self.win)
        self.reports = None if reports is None else np.asarray(reports, REPORT)
        self.N_max = (0 if reports is None else len(self.reports)) if N_max is None else N_max
        self.n_reports, self.status = n_reports, status

    def blank(self, state=None, credit=None) -> dict:
        """The buffers a first call starts from: a zeroed state, everything else 0xCC."""
        return dict(state=np.zeros(self.G, STATE) if state is None else np.asarray(state, STATE).copy(),
                    credit=np.full(self.G, FILL32, np.uint32) if credit is None else np.asarray(credit, np.uint32).copy(),
                    status=np.full(self.N_max, FILL32, np.uint32).view(np.int32))

    def statuses(self):
        """-> status per looked-at report, fresh: slot -> the largest QF_OK rank."""
        N = self.N_max if self.n_reports is None else min(int(self.n_reports), self.N_max)
        st, fresh = [], {}
        for f in range(N):
            x, r, z = (int(v) for v in self.reports[f])
            if x >= ID_LIMIT or r > self.k or z != 0:
                st.append(EINVAL)
                continue
            s = x % self.G
            h = held(self.win[s])
            if h > x + 1:
                st.append(ESTALE)
            elif h < x + 1:
                st.append(ENOTREADY)
            else:
                st.append(OK)
                fresh[s] = max(fresh.get(s, 0), r)
        return st, fresh

    def model(self, before: dict | None = None) -> dict:
        o = {key: v.copy() for key, v in (before or self.blank()).items()}
        st, fresh = self.statuses()
        if self.status:
            o["status"][: len(st)] = st
        k, num, den = self.k, self.num, self.den
        for s in range(self.G):
            h = held(self.win[s])
            if h == 0:
                o["state"][s], o["credit"][s] = (0, 0, 0), 0
                continue
            mine = int(o["state"][s]["owner"]) == h
            p = int(o["state"][s]["peer"]) if mine else 0
            prev = int(o["credit"][s]) if mine else 0
            r, sent = min(int(self.rank[s]), k), int(self.sent[s])
            peer = max(p, fresh.get(s, 0))
            if peer >= k:
                credit = sent
            else:
                c = max(prev, ceil_rho(r, num, den))
                if s in fresh:
                    c = max(c, sent + ceil_rho(max(0, r - peer), num, den))
                credit = min(c, self.cap)
            o["state"][s], o["credit"][s] = (h, peer, 0), credit
        return o


def make_credit(G, k, num, den, cap, N_max, seed, *, n_reports=None, n_reports_null=False, status=True):
    """-> (call, the buffers it starts from).  A random window; ranks 0 .. k + 2;
    states that belong to the slot's generation, to another one, or to none
    (the previous credit of the last two is 0xCC); reports for the held id, an
    older and a newer one, with every kind of invalid record among them."""
    rng = np.random.default_rng(seed)
    win, base = random_window(rng, G)
    rank = rng.integers(0, k + 3, G).astype(np.uint32)
    sent = rng.integers(0, cap + 1, G).astype(np.uint32)
    state = np.zeros(G, STATE)
    credit = np.full(G, FILL32, np.uint32)
    for s in range(G):
        kind, h = int(rng.integers(0, 3)), held(win[s])
        if kind == 1 and h:
            state[s] = (h, int(rng.integers(0, k + 1)), 0)
            credit[s] = int(rng.integers(0, cap + 1))
        elif kind == 2:
            state[s] = (base + s + 1, int(rng.integers(0, k + 1)), 0)   # the generation of the cycle before
    rep = None
    if N_max:
        rows = []
        for f in range(N_max):
            s = int(rng.integers(0, G))
            x = base + int(rng.integers(0, 3)) * G + s               # older, held (or empty), newer
            if rng.random() < 0.6:
                x = base + G + s
            r, z = int(rng.integers(0, k + 1)), 0
            u = rng.random()
            if u < 0.05:
                r = k + 1 + int(rng.integers(0, 3))
            elif u < 0.10:
                z = 1 + int(rng.integers(0, 9))
            elif u < 0.15:
                x = (ID_LIMIT, U64MAX, ID_LIMIT + s)[int(rng.integers(0, 3))]
            elif u < 0.30:
                r = k
            rows.append((x, r, z))
        rep = records(rows)
    n = None if n_reports_null or not N_max else (N_max if n_reports is None else n_reports)
    c = CreditCall(k, num, den, cap, win, rank, sent, rep, n, N_max, status)
    return c, c.blank(state, credit)


def credit_cases() -> dict:
    """name -> (call, the buffers it starts from)."""
    c = {}
    for i, G in enumerate((1, 63, 64, 65, 130)):
        c[f"G{G}"] = make_credit(G, 4, 3, 2, 16, 64, 200 + i)
    for i, (k, num, den, cap) in enumerate(((1, 1, 1, 4), (4, 5, 4, 16), (64, 3, 2, 128), (256, 5, 4, 1024),
                                            (64, 65535, 1, 100), (256, 65535, 65535, 1 << 20))):
        c[f"k{k}_rho{num}_{den}"] = make_credit(65, k, num, den, cap, 65, 210 + i)
    for i, N in enumerate((0, 1, 64, 65, 130)):
        c[f"N{N}"] = make_credit(63, 4, 3, 2, 16, N, 220 + i)
    c["n_reports_above_N_max"] = make_credit(23, 4, 3, 2, 16, 40, 230, n_reports=1000)
    c["n_reports_mid"] = make_credit(23, 4, 3, 2, 16, 40, 231, n_reports=17)
    c["n_reports_0"] = make_credit(23, 4, 3, 2, 16, 40, 232, n_reports=0)
    c["n_reports_null"] = make_credit(23, 4, 3, 2, 16, 40, 233, n_reports_null=True)
    c["no_status"] = make_credit(23, 4, 3, 2, 16, 40, 234, status=False)
    # one slot's reports in different waves with different ranks: the maximum wins
    G, k = 5, 64
    base = (1 << 40) // G * G
    win = np.array([0, base + 1 + 1, 0, 0, 0], np.uint64)
    ranks = [int(x) for x in np.random.default_rng(240).integers(0, 40, 130)]
    ranks[3], ranks[70], ranks[129] = 41, 57, 50
    x = CreditCall(k, 1, 1, 256, win, [0, 60, 0, 0, 0], [0, 9, 0, 0, 0], records([(base + 1, r, 0) for r in ranks]))
    c["one_slot_many_waves"] = (x, x.blank())
    # the id edges: 2^62 - 1 is a generation, 2^62 and UINT64_MAX are not
    G = 7
    s = (ID_LIMIT - 1) % G
    win = np.zeros(G, np.uint64)
    win[s] = ID_LIMIT
    win[(s + 1) % G] = 5 * G + (s + 1) % G + 1
    x = CreditCall(4, 1, 1, 16, win, np.full(G, 3), np.full(G, 1),
                   records([(ID_LIMIT - 1, 2, 0), (ID_LIMIT, 2, 0), (U64MAX, 0, 0), (U64MAX, 2, 0)]))
    c["id_edges"] = (x, x.blank())
    return c


def credit_sequences() -> dict:
    """name -> [calls]: each call starts from what the one before left."""
    q = {}
    G, k = 4, 4
    base = (1 << 40) + 8
    open_ = lambda cyc: np.array([base + cyc * G + s + 1 for s in range(G)], np.uint64)   # noqa: E731
    rep = lambda *rows: records(list(rows))                                                    # noqa: E731
    # a slot whose window entry changed between two calls: the state restarts, the old credit is ignored
    w1 = open_(0)
    w2 = w1.copy()
    w2[1] = base + G + 1 + 1
    q["restart"] = [CreditCall(k, 3, 2, 16, w1, [4, 4, 2, 0], [0, 0, 0, 0], rep((base + 1, 3, 0))),
                    CreditCall(k, 3, 2, 16, w2, [4, 1, 2, 0], [6, 0, 3, 0])]
    # the same report twice in one call, once more in the next, and then the peer is satisfied
    again = rep((base + 2, 1, 0), (base + 2, 1, 0))
    q["repeat"] = [CreditCall(k, 1, 1, 16, w1, [0, 0, 3, 0], [0, 0, 3, 0], again),
                   CreditCall(k, 1, 1, 16, w1, [0, 0, 3, 0], [0, 0, 5, 0], again[:1]),
                   CreditCall(k, 1, 1, 16, w1, [0, 0, 3, 0], [0, 0, 7, 0]),
                   CreditCall(k, 1, 1, 16, w1, [0, 0, 4, 0], [0, 0, 7, 0], rep((base + 2, 4, 0))),
                   CreditCall(k, 1, 1, 16, w1, [0, 0, 4, 0], [0, 0, 7, 0], rep((base + 2, 2, 0)))]
    # closed at the sender, then emptied by hand: credit 0 and a state that forgets
    w3 = w1.copy()
    w3[0] = int(w3[0]) | CLOSED
    w4 = w3.copy()
    w4[0] = 0
    q["closed_then_empty"] = [CreditCall(k, 3, 2, 16, w3, [2, 0, 0, 0], [1, 0, 0, 0], rep((base, 1, 0))),
                              CreditCall(k, 3, 2, 16, w4, [2, 0, 0, 0], [1, 0, 0, 0], rep((base, 1, 0)))]
    # the cap holds against a ratio of 65535
    q["cap"] = [CreditCall(k, 65535, 1, 9, w1, [1, 2, 300, 0], [0, 0, 8, 0], rep((base + 2, 0, 0))),
                CreditCall(k, 65535, 1, 7, w1, [1, 2, 300, 0], [0, 0, 8, 0])]
    return q


def run_sequence(calls):
    """-> the outputs of each call under the model."""
    outs, state, credit = [], None, None
    for c in calls:
        o = c.model(c.blank(state, credit))
        state, credit = o["state"], o["credit"]
        outs.append(o)
    return outs


# ---------------------------------------------------------------------------
# the lossy loop: emit_ref's source -> relay -> receiver with drops on the second hop
# ---------------------------------------------------------------------------
CAP_LOOP = 4 * E.K_LOOP
N_REPORTS = 2 * E.G_LOOP          # the report buffer: the completed list, then the deadline list
MAX_POLLS = len(E.SCHED) + 16
# The recode's seed of poll p.  fill_splitmix adds the word index to the seed, so the seeds of two polls
# are further apart than the G * M * k / 8 words a poll draws: with consecutive seeds the rows a generation
# sends in its second poll repeat the mix of rows it sent in its first, and add no rank at the receiver.
SEED_STRIDE = 16
assert SEED_STRIDE * 8 >= E.G_LOOP * E.M_RELAY * E.K_LOOP


def poll_seed(p: int, seed: int = E.SEED_LOOP) -> int:
    return seed + SEED_STRIDE * p


def dropped2(g: int, n: int) -> bool:
    """The drop mask of the second hop: frame n of wire generation g, counted over all frames the relay emits for g."""
    return (g + 2 * n) % 5 == 0


def receiver_reports(win, rank, done):
    """The receiver's two calls after the closing reset -> (first call, its outputs, second call, its outputs)."""
    G, k = E.G_LOOP, E.K_LOOP
    sel = np.full(G, FILL32, np.uint32)
    sel[: len(done)] = done
    a = ReportCall(k, sel, win, rank, N_REPORTS, n_sel=len(done))
    oa = a.model()
    listed = [s for s in range(G) if rank[s] >= 1]
    sel = np.full(G, FILL32, np.uint32)
    sel[: len(listed)] = listed
    b = ReportCall(k, sel, win, rank, N_REPORTS, n_sel=len(listed), append=True)
    return a, oa, b, b.model(oa)


def lossy_loop(oracle, num: int, den: int, reports: bool, seed: int = E.SEED_LOOP):
    """-> spec, the per-poll records, the statistics the tests assert on."""
    from tests import partial_ref as P
    from tests import window_ref as WR

    spec = E.LoopSpec()
    k, G, M = E.K_LOOP, E.G_LOOP, E.M_RELAY
    relay, rx = E.Node(), E.Node()
    state, credit = np.zeros(G, STATE), np.full(G, FILL32, np.uint32)
    back = dict(reports=poisoned(N_REPORTS, REPORT), n_reports=np.zeros(1, np.uint32))   # what the receiver sent last
    polls, emitted, delivered, satisfied, after_k = [], {}, {}, {}, {}
    max_sent = 0
    for p in range(MAX_POLLS):
        gens = E.SCHED[p] if p < len(E.SCHED) else []
        rec = dict(gens=gens)
        a, b = spec.source_calls(gens)
        q1 = b.model(a.model())
        q1["frame_len"][spec.drop_list(gens)] = 0
        rec["q1"] = q1
        relay.ingest(q1, E.N_SRC)
        # the relay: reports of the last poll and ranks to credit, select over sent, recode, ids, emit
        rank = relay.rank()
        cc = CreditCall(k, num, den, CAP_LOOP, relay.win, rank, relay.sent.copy(),
                        back["reports"] if reports else None, int(back["n_reports"][0]) if reports else None,
                        N_REPORTS if reports else 0)
        co = cc.model(cc.blank(state, credit))
        state, credit = co["state"], co["credit"]
        for f, st in enumerate(cc.statuses()[0]):
            if st == OK and int(cc.reports[f]["rank"]) == k:
                satisfied.setdefault(int(cc.reports[f]["id"]) - E.BASE_LOOP, p)
        listed = [s for s in range(G) if credit[s] >= 1 and credit[s] > relay.sent[s]]
        sel = np.full(G, FILL32, np.uint32)
        sel[: len(listed)] = listed
        mix = oracle.fill_splitmix(G * M * k, poll_seed(p, seed)).reshape(G, M, k)
        rows = np.full((G, M, spec.rs), E.FILL, np.uint8)
        vec = np.zeros((G, M, k), np.uint8)
        rl = np.zeros((G, M), np.uint32)
        st = np.full(G, ENOTREADY, np.int32)
        for j, s in enumerate(listed):
            n = len(relay.vec[s])
            vec[j] = P.encode_rows(mix[j, :, :n], np.stack(relay.vec[s]))
            rows[j, :, :E.L_LOOP] = P.encode_rows(mix[j, :, :n], np.stack(relay.pay[s]))
            rl[j], st[j] = E.L_LOOP, OK
        _, ids = WR.window_sel(relay.win, sel, len(listed), G, G, False)
        c = spec.relay_call(sel, len(listed), rows.reshape(-1), vec, rl, st, ids, credit.copy(), relay.sent.copy())
        q2 = c.model()
        relay.sent = q2["sent"].copy()         # (a later eviction zeroes the node's entry, not the record's)
        max_sent = max(max_sent, int(relay.sent.max()))
        # the second hop's drops, by each generation's running frame count
        drops = []
        for f in range(int(q2["n_frames"][0])):
            g = int(q2["frame_id"][f]) - E.BASE_LOOP
            if dropped2(g, emitted.get(g, 0)):
                drops.append(f)
            emitted[g] = emitted.get(g, 0) + 1
            if g in satisfied:
                after_k[g] = after_k.get(g, 0) + 1
        wire = {key: v.copy() for key, v in q2.items()}
        wire["frame_len"][drops] = 0
        rec.update(credit_call=cc, credit_out=co, call=c, q2=q2, drops=drops,
                   listed=[(s, WR.held(relay.win[s]) - E.BASE_LOOP) for s in listed])
        # the receiver: ingest, the complete generations leave and close, then the two report lists
        rx.ingest(wire, E.N_RELAY)
        done = [s for s in range(G) if len(rx.vec[s]) == k]
        for s in done:
            g = WR.held(rx.win[s]) - E.BASE_LOOP
            assert g not in delivered
            got = np.stack(rx.pay[s])
            assert np.array_equal(got, P.encode_rows(np.stack(rx.vec[s]), spec.src[g])), "a row is not its vector x the sources"
            delivered[g] = p
            rx.reset(s)
        rx.win, _ = WR.window_sel(rx.win, done, len(done), G, G, True)
        ra, oa, rb, ob = receiver_reports(rx.win, rx.rank(), done)
        rec.update(done=done, report_calls=(ra, rb), report_out=(oa, ob))
        pending = reports and int(ob["n_reports"][0]) > 0
        back = ob
        polls.append(rec)
        if p >= len(E.SCHED) - 1 and not listed and not pending:
            break
    else:
        raise AssertionError("the loop does not come to rest")
    return spec, polls, dict(emitted=emitted, delivered=delivered, max_sent=max_sent, satisfied=satisfied,
                             after_k=after_k, frames=sum(emitted.values()))


@functools.lru_cache(maxsize=None)
def _loop_cached(num, den, reports):
    from tests import oracle_py

    return lossy_loop(oracle_py, num, den, reports)
