"""Reference of qf_emit_frames_sel_dev -- TEST INFRASTRUCTURE ONLY.

The call restated in plain numpy from the rules written in include/qf_fec.h
above it: per entry the status and the frames it wants, the queue positions by
an exclusive prefix, the emitted prefix, and per frame the bytes of
Packet::to_raw in the payload-aligned slot layout.  Nothing here touches the
library under test.

Call:        the inputs of one call as numpy arrays (None where the C pointer
             is NULL) and model(), which returns every output buffer whole, as
             the call leaves it when it starts from `before` (default: every
             byte 0xCC).
make_call:   a call over random rows, poisoned outside their lengths.
cases():     the named calls of the device test and of the host-emulation test.
LoopSpec, Node, loop_model: source -> relay -> receiver under the models
             (window_ref, poll_ref, rank_ref; the recode as oracle.fill_splitmix
             mix x vectors), with the calls and the drop mask that the device
             test runs with real calls."""
from __future__ import annotations

import numpy as np

OK, EINVAL, ENOTREADY, ERANK = 0, -1, -3, -4
FILL = 0xCC
NONE32 = 0xFFFFFFFF
U64MAX = (1 << 64) - 1


def r16(x: int) -> int:
    return (x + 15) // 16 * 16


def payload_offset(k: int) -> int:
    return r16(3 + k)


def frame_bytes(k: int, idx: int, vec, payload) -> bytes:
    """Packet::to_raw of one row: systematic (idx < k) or coded with vec."""
    if idx < k:
        return b"\x01" + bytes(payload)
    return bytes([0, k >> 8, k & 0xFF]) + bytes(vec) + bytes(payload)


class Call:
    def __init__(self, k, L, max_rows, n_max, G_src, N_max, row_stride, rows_gen_stride, frame_stride, sel, rows, ids,
                 n_sel=None, row_index=None, n_rows=None, row_coeffs=None, row_len=None, in_status=None, rank=None,
                 sent=None, append=False):
        self.k, self.L, self.max_rows, self.n_max, self.G_src, self.N_max = k, L, max_rows, n_max, G_src, N_max
        self.row_stride, self.rows_gen_stride, self.frame_stride = row_stride, rows_gen_stride, frame_stride
        self.sel = np.asarray(sel, np.uint32)
        self.n_sel = n_sel
        self.rows = np.asarray(rows, np.uint8)
        self.ids = np.asarray(ids, np.uint64)
        self.row_index = None if row_index is None else np.asarray(row_index, np.uint16).reshape(n_max, max_rows)
        self.n_rows = None if n_rows is None else np.asarray(n_rows, np.uint32)
        self.row_coeffs = None if row_coeffs is None else np.asarray(row_coeffs, np.uint8).reshape(n_max, max_rows, k)
        self.row_len = None if row_len is None else np.asarray(row_len, np.uint32).reshape(n_max, max_rows)
        self.in_status = None if in_status is None else np.asarray(in_status, np.int32)
        self.rank = None if rank is None else np.asarray(rank, np.uint32)
        self.sent = None if sent is None else np.asarray(sent, np.uint32)
        self.append = append

    @property
    def P(self):
        return payload_offset(self.k)

    def blank(self, n_frames: int = 0xCCCCCCCC) -> dict:
        """Every output buffer as the tests hand it over: 0xCC everywhere."""
        N, n = self.N_max, self.n_max
        b = dict(frames=np.full(N * self.frame_stride, FILL, np.uint8),
                 frame_len=np.full(N, 0xCCCCCCCC, np.uint32), frame_off=np.full(N, 0xCCCCCCCC, np.uint32),
                 frame_id=np.full(N, 0xCCCCCCCCCCCCCCCC, np.uint64), frame_pkt=np.full(N, 0xCCCCCCCCCCCCCCCC, np.uint64),
                 n_frames=np.array([n_frames], np.uint32), n_left=np.full(1, 0xCCCCCCCC, np.uint32),
                 entry_first=np.full(n, 0xCCCCCCCC, np.uint32), entry_count=np.full(n, 0xCCCCCCCC, np.uint32),
                 entry_status=np.full(n, -858993460, np.int32))
        if self.sent is not None:
            b["sent"] = self.sent.copy()
        return b

    def entries(self):
        """-> (status so far, wanted frames) per entry."""
        n = self.n_max if self.n_sel is None else min(int(self.n_sel), self.n_max)
        st = np.full(self.n_max, ENOTREADY, np.int32)
        want = np.zeros(self.n_max, np.int64)
        for j in range(n):
            g = int(self.sel[j])
            if g >= self.G_src or int(self.ids[j]) >= 1 << 62:
                st[j] = EINVAL
                continue
            nj = self.max_rows if self.n_rows is None else min(int(self.n_rows[j]), self.max_rows)
            bad = False
            if self.row_len is not None and (self.row_len[j, :nj] > self.L).any():
                bad = True
            if self.row_index is not None and self.row_coeffs is None and (self.row_index[j, :nj] >= self.k).any():
                bad = True
            if bad:
                st[j] = EINVAL
                continue
            if self.in_status is not None and int(self.in_status[j]) != OK:
                st[j] = int(self.in_status[j])
                continue
            st[j] = OK
            c = nj
            if self.rank is not None:
                rk, sn = int(self.rank[g]), int(self.sent[g])
                c = min(nj, rk - sn) if rk > sn else 0
            want[j] = c
        return st, want

    def model(self, before: dict | None = None) -> dict:
        o = {key: v.copy() for key, v in (before or self.blank()).items()}
        k, P, fs = self.k, self.P, self.frame_stride
        st, want = self.entries()
        base = min(int(o["n_frames"][0]), self.N_max) if self.append else 0
        at = 0
        emitted = 0
        frames = o["frames"].reshape(self.N_max, fs)
        for j in range(self.n_max):
            first, count = NONE32, 0
            c = int(want[j])
            if st[j] == OK:
                if base + at + c <= self.N_max:
                    count = c
                    if c:
                        first = base + at
                else:
                    st[j] = ENOTREADY
            o["entry_first"][j], o["entry_count"][j] = first, count
            for s in range(count):
                q = base + at + s
                rlen = self.L if self.row_len is None else int(self.row_len[j, s])
                idx = k if self.row_index is None else min(int(self.row_index[j, s]), k)
                r0 = j * self.rows_gen_stride + s * self.row_stride
                raw = frame_bytes(k, idx, None if idx < k else self.row_coeffs[j, s], self.rows[r0: r0 + rlen])
                foff = P - (len(raw) - rlen)
                frames[q, foff: foff + len(raw)] = np.frombuffer(raw, np.uint8)
                o["frame_len"][q], o["frame_off"][q] = len(raw), foff
                o["frame_id"][q] = self.ids[j]
                o["frame_pkt"][q] = idx if idx < k else 0
            if count and self.sent is not None:
                o["sent"][int(self.sel[j])] += count
            emitted += count
            at += c
        o["entry_status"][:] = st
        o["n_frames"][0] = base + emitted
        o["n_left"][0] = min(at - emitted, NONE32)
        return o


def rows_bytes(n_max, max_rows, row_stride, rows_gen_stride, L):
    """rows_dev to the end of its last row's last 16-byte unit."""
    return (n_max - 1) * rows_gen_stride + (max_rows - 1) * row_stride + r16(L)


def make_call(k, L, max_rows, n_max, *, N_max=None, G_src=None, seed=1, all_coded=False, lens="L", n_rows=None,
              frame_extra=0, row_extra=0, budget=None, vectors=True, **kw) -> Call:
    """A call over random rows.  lens: "L", "zero", "ragged" (0..L, both ends
    present) or None (row_len NULL).  Rows mix systematic and coded ones unless
    all_coded (row_index NULL).  budget: None or (rank, sent) per generation."""
    rng = np.random.default_rng(seed)
    G_src = G_src or n_max + 3
    rs = r16(L) + row_extra
    gs = max_rows * rs + row_extra
    fs = payload_offset(k) + r16(L) + frame_extra if frame_extra else r16(payload_offset(k) + L)
    N_max = N_max if N_max is not None else n_max * max_rows
    if lens is None or lens == "L":
        rl = np.full((n_max, max_rows), L, np.uint32)
    elif lens == "zero":
        rl = np.zeros((n_max, max_rows), np.uint32)
    else:
        rl = rng.integers(0, L + 1, (n_max, max_rows)).astype(np.uint32)
        rl.reshape(-1)[:2] = (0, L)
    buf = np.full((n_max, gs), FILL, np.uint8)
    data = rng.integers(0, 256, (n_max, max_rows, L), np.uint8)
    for s in range(max_rows):
        inside = np.arange(L)[None, :] < rl[:, s, None]
        buf[:, s * rs: s * rs + L] = np.where(inside, data[:, s], FILL)
    rows = buf.reshape(-1)[: rows_bytes(n_max, max_rows, rs, gs, L)].copy()
    coeffs = rng.integers(0, 256, (n_max, max_rows, k), np.uint8) if vectors else None
    if all_coded:
        ri = None
    else:
        ri = np.where(rng.random((n_max, max_rows)) < 0.5, rng.integers(0, k, (n_max, max_rows)), k).astype(np.uint16)
        if not vectors:
            ri = rng.integers(0, k, (n_max, max_rows)).astype(np.uint16)
    sel = rng.permutation(G_src)[:n_max].astype(np.uint32) if G_src >= n_max else rng.integers(0, G_src, n_max)
    ids = rng.integers(0, 1 << 40, n_max).astype(np.uint64)
    rank = sent = None
    if budget is not None:
        rank, sent = (np.asarray(x, np.uint32) for x in budget)
    return Call(k, L, max_rows, n_max, G_src, N_max, rs, gs, fs, sel, rows, ids, row_index=ri, n_rows=n_rows,
                row_coeffs=coeffs, row_len=None if lens is None else rl, rank=rank, sent=sent, **kw)


# ---------------------------------------------------------------------------
# the named cases (small: the host emulation runs them under a sanitizer)
# ---------------------------------------------------------------------------
SHAPE_K = (1, 13, 14, 64, 253, 255)
SHAPE_L = (1, 15, 16, 17, 48)


def cases() -> dict:
    c = {}
    for i, k in enumerate(SHAPE_K):
        c[f"k{k}"] = make_call(k, 17, 5, 3, seed=10 + i, lens="ragged", n_rows=[5, 0, 9])
        c[f"k{k}_coded"] = make_call(k, 48, 1, 4, seed=20 + i, all_coded=True, lens=None, frame_extra=32)
    for i, L in enumerate(SHAPE_L):
        c[f"L{L}"] = make_call(14, L, 5, 3, seed=30 + i, lens="ragged", row_extra=16)
        c[f"L{L}_full"] = make_call(64, L, 1, 3, seed=40 + i, lens="L")
    c["len_zero"] = make_call(13, 16, 5, 2, seed=50, lens="zero")
    c["systematic_no_vectors"] = make_call(4, 16, 5, 3, seed=51, vectors=False)
    # lists
    x = make_call(4, 16, 5, 9, G_src=6, seed=60, lens="ragged", n_sel=7)
    x.sel[:] = [0, 6, 1, 2, 3, 4, 5, 0, 99]              # entry 1 invalid; 7, 8 unused
    x.ids[2], x.ids[3] = U64MAX, 1 << 62
    x.in_status = np.array([OK, OK, OK, OK, ERANK, OK, OK, OK, OK], np.int32)
    x.row_len[5, 2] = 17                                 # a row longer than L
    c["list"] = x
    x = make_call(4, 16, 5, 3, seed=61, vectors=False)
    x.row_index[1, 3] = 4                                # a coded row without vectors
    x.n_rows = np.array([5, 4, 5], np.uint32)
    c["list_coded_without_vectors"] = x
    x = make_call(4, 16, 5, 3, seed=62, vectors=False)
    x.row_index[1, 3] = 4
    x.n_rows = np.array([5, 3, 5], np.uint32)            # ... behind its entry's rows: not looked at
    c["list_coded_row_unused"] = x
    c["n_sel_above_n_max"] = make_call(4, 16, 5, 3, seed=63, n_sel=1000)
    # queue
    c["exact_fit"] = make_call(4, 16, 5, 4, seed=70, n_rows=[5, 2, 0, 3], N_max=10)
    c["cutoff"] = make_call(4, 16, 5, 6, seed=71, n_rows=[5, 2, 4, 0, 1, 5], N_max=8)
    c["cutoff_first"] = make_call(4, 16, 5, 2, seed=72, N_max=4)
    c["stale_n_frames"] = make_call(4, 16, 5, 2, seed=73)
    # budget: rank - sent of 0 and below n_j, and sent above rank (no wrap: nothing is wanted)
    x = make_call(4, 16, 5, 5, G_src=5, seed=80, budget=([3, 4, 2, 0, 1], [3, 1, 0, 0, 5]))
    x.sel[:] = [0, 1, 2, 3, 4]
    c["budget"] = x
    # ... and above n_j: the entry's n_j rows bound the count, and the rows behind them are not looked at
    x = make_call(4, 16, 5, 4, G_src=4, seed=82, lens="ragged", n_rows=[2, 5, 1, 0],
                  budget=([9, 2, 3, 1], [5, 0, 0, 0]))
    x.sel[:] = [0, 1, 2, 3]
    for j, n in enumerate(x.n_rows):
        x.row_len[j, n:] = 0xFFFF                       # longer than L: QF_EINVAL if it were read
    c["budget_above_rows"] = x
    x = make_call(4, 16, 5, 4, G_src=4, seed=81, budget=([4, 4, 4, 4], [0, 1, 2, 3]), N_max=6)
    x.sel[:] = [3, 2, 1, 0]
    c["budget_overflow"] = x
    return c


APPEND_BASES = {"base0": 0, "base_mid": 3, "base_full": 12, "base_above": 1000}


def append_case(name: str):
    """-> (call, the output buffers it starts from)."""
    c = make_call(13, 17, 5, 3, seed=90, lens="ragged", n_rows=[4, 1, 5], N_max=12, append=True)
    return c, c.blank(APPEND_BASES[name])


def scale_cases(per_block: int = 64, grid_frames: int = 0) -> dict:
    """Tiny rows, many entries: three scan blocks plus one entry, and (device
    test only: grid_frames > 0) more frames than one round of the copy's grid."""
    c = {}
    n = 3 * per_block + 1
    rng = np.random.default_rng(5)
    c["scan_blocks"] = make_call(4, 16, 2, n, seed=95, n_rows=rng.integers(0, 3, n).astype(np.uint32), N_max=n - 40)
    if grid_frames:
        n = grid_frames // 4 + 3
        c["grid_rounds"] = make_call(4, 16, 4, n, seed=96, lens=None, all_coded=True)
    return c


# ---------------------------------------------------------------------------
# the loop: source -> relay -> receiver, k = 4, L = 48, 4 slots, 12 wire generations
# ---------------------------------------------------------------------------
K_LOOP, L_LOOP, G_LOOP, GENS_LOOP = 4, 48, 4, 12
R_SRC, M_RELAY, NS_LOOP, N_SRC, N_RELAY, MR_LOOP = 2, 4, 2, 12, 6, 8
BASE_LOOP = (1 << 40) + 2
SEED_LOOP = 0x51ED
# the wire generations the source sends in each poll: a poll with two makes the relay's queue overflow
SCHED = ([0], [1, 2], [], [3], [4, 5], [], [6], [7, 8], [], [9], [10, 11], [], [])


def dropped(g: int, f: int) -> bool:
    """The fixed drop mask of the first hop: frame f (source i, or k + repair t) of generation g."""
    return (3 * g + 2 * f) % 7 == 0 or (g + f) % 6 == 5


class LoopSpec:
    def __init__(self):
        from tests import partial_ref as P

        rng = np.random.default_rng(77)
        self.src = rng.integers(1, 256, (GENS_LOOP, K_LOOP, L_LOOP), dtype=np.uint8)
        self.rep_vec = rng.integers(1, 256, (GENS_LOOP, R_SRC, K_LOOP), dtype=np.uint8)
        self.rep = np.stack([P.encode_rows(self.rep_vec[g], self.src[g]) for g in range(GENS_LOOP)])
        self.rs = r16(L_LOOP)
        self.fs = payload_offset(K_LOOP) + self.rs

    def source_calls(self, gens):
        """The source's two calls for a poll: its packets as systematic rows, then the repairs appended."""
        k, rs, n = K_LOOP, self.rs, len(gens)
        ids = np.full(NS_LOOP, U64MAX, np.uint64)
        ids[:n] = [BASE_LOOP + g for g in gens]
        rows = np.full((NS_LOOP, k, rs), FILL, np.uint8)
        reps = np.full((NS_LOOP, R_SRC, rs), FILL, np.uint8)
        vec = np.full((NS_LOOP, R_SRC, k), FILL, np.uint8)
        for j, g in enumerate(gens):
            rows[j, :, :L_LOOP], reps[j, :, :L_LOOP], vec[j] = self.src[g], self.rep[g], self.rep_vec[g]
        a = Call(k, L_LOOP, k, NS_LOOP, NS_LOOP, N_SRC, rs, k * rs, self.fs, np.arange(NS_LOOP), rows.reshape(-1), ids,
                 n_sel=n, row_index=np.tile(np.arange(k, dtype=np.uint16), NS_LOOP))
        b = Call(k, L_LOOP, R_SRC, NS_LOOP, NS_LOOP, N_SRC, rs, R_SRC * rs, self.fs, np.arange(NS_LOOP),
                 reps.reshape(-1), ids, n_sel=n, row_coeffs=vec, append=True)
        return a, b

    def drop_list(self, gens):
        """The queue positions of the source's frames that the first hop drops."""
        k, n = K_LOOP, len(gens)
        out = [j * k + i for j, g in enumerate(gens) for i in range(k) if dropped(g, i)]
        return out + [n * k + j * R_SRC + t for j, g in enumerate(gens) for t in range(R_SRC) if dropped(g, k + t)]

    def relay_call(self, sel, n_sel, rows, coeffs, row_len, status, ids, rank, sent) -> Call:
        """The relay's call over a listed recode's outputs."""
        return Call(K_LOOP, L_LOOP, M_RELAY, G_LOOP, G_LOOP, N_RELAY, self.rs, M_RELAY * self.rs, self.fs, sel, rows, ids,
                    n_sel=n_sel, row_coeffs=coeffs, row_len=row_len, in_status=status, rank=rank, sent=sent)


class Node:
    """A relay or receiver under the models: the window and, per slot, the innovative rows."""

    def __init__(self):
        self.win = np.zeros(G_LOOP, np.uint64)
        self.vec = [[] for _ in range(G_LOOP)]
        self.pay = [[] for _ in range(G_LOOP)]
        self.sent = np.zeros(G_LOOP, np.uint32)

    def rank(self):
        return np.array([len(v) for v in self.vec], np.uint32)

    def reset(self, s):
        self.vec[s], self.pay[s], self.sent[s] = [], [], 0

    def ingest(self, q, N):
        """A flat poll (an emit call's outputs, unmodified but for dropped lengths) through the window and
        ingest models into the stores."""
        from tests import poll_ref as PR
        from tests import rank_ref
        from tests import window_ref as WR

        n = int(q["n_frames"][0])
        w = WR.window(self.win, q["frame_id"], n, G_LOOP, G_LOOP)
        self.win = w.win
        for s in w.evicted:
            self.reset(s)
        p = PR.Poll(K_LOOP, L_LOOP, N, len(q["frames"]) // N)
        p.frames = q["frames"].reshape(N, -1)
        p.flen, p.foff, p.ids, p.gen = q["frame_len"], q["frame_off"], q["frame_pkt"], w.frame_gen
        ing = PR.ingest(p, n, G_LOOP, G_LOOP, MR_LOOP)
        assert (ing.entry_status[: ing.n_sel] == OK).all()
        for j in range(ing.n_sel):
            s = int(ing.sel[j])
            for c in range(int(ing.n_rows[j])):
                vec = ing.row_coeffs[j, c].copy()
                if rank_ref.innovative(np.stack(self.vec[s] + [vec]))[1] > len(self.vec[s]):
                    row = np.zeros(L_LOOP, np.uint8)
                    o, ln = int(ing.row_off[j, c]), int(ing.row_len[j, c])
                    row[:ln] = q["frames"][o: o + ln]
                    self.vec[s].append(vec)
                    self.pay[s].append(row)
        return w


def loop_model(oracle):
    """The loop under the models alone -> the per-poll records and the statistics the tests assert on."""
    from tests import partial_ref as P
    from tests import window_ref as WR

    spec = LoopSpec()
    k, G, M = K_LOOP, G_LOOP, M_RELAY
    relay, rx = Node(), Node()
    polls = []
    emitted = {}                 # wire generation -> frames the relay emitted
    final_rank = {}              # wire generation -> the relay's last rank
    delivered = {}               # wire generation -> poll in which the receiver completed it
    for p, gens in enumerate(SCHED):
        rec = dict(gens=gens)
        # the source: two calls, then the first hop's drops
        a, b = spec.source_calls(gens)
        q1 = b.model(a.model())
        q1["frame_len"][spec.drop_list(gens)] = 0
        rec["q1"] = q1
        relay.ingest(q1, N_SRC)
        # the relay: select over sent, the listed recode, the ids, the emit
        rank = relay.rank()
        listed = [s for s in range(G) if rank[s] > relay.sent[s]]
        sel = np.full(G, 0xCCCCCCCC, np.uint32)
        sel[: len(listed)] = listed
        mix = oracle.fill_splitmix(G * M * k, SEED_LOOP + p).reshape(G, M, k)
        rows = np.full((G, M, spec.rs), FILL, np.uint8)
        co = np.zeros((G, M, k), np.uint8)
        rl = np.zeros((G, M), np.uint32)
        st = np.full(G, ENOTREADY, np.int32)
        for j, s in enumerate(listed):
            n = len(relay.vec[s])
            co[j] = P.encode_rows(mix[j, :, :n], np.stack(relay.vec[s]))
            rows[j, :, :L_LOOP] = P.encode_rows(mix[j, :, :n], np.stack(relay.pay[s]))
            rl[j], st[j] = L_LOOP, OK
        _, ids = WR.window_sel(relay.win, sel, len(listed), G, G, False)
        c = spec.relay_call(sel, len(listed), rows.reshape(-1), co, rl, st, ids, rank, relay.sent.copy())
        q2 = c.model()
        relay.sent = q2["sent"]
        rec.update(call=c, q2=q2, listed=[(s, WR.held(relay.win[s]) - BASE_LOOP) for s in listed])
        for j, (s, g) in enumerate(rec["listed"]):
            emitted[g] = emitted.get(g, 0) + int(q2["entry_count"][j])
            final_rank[g] = int(rank[s])
        # the receiver: no drops on the second hop (the budget leaves no redundancy to lose)
        rx.ingest(q2, N_RELAY)
        done = [s for s in range(G) if len(rx.vec[s]) == k]
        for s in done:
            g = WR.held(rx.win[s]) - BASE_LOOP
            assert g not in delivered
            got = np.stack(rx.pay[s])
            assert np.array_equal(got, P.encode_rows(np.stack(rx.vec[s]), spec.src[g])), "a row is not its vector x the sources"
            delivered[g] = p
            rx.reset(s)
        rx.win, _ = WR.window_sel(rx.win, done, len(done), G, G, True)
        rec["done"] = done
        polls.append(rec)
    return spec, polls, dict(emitted=emitted, final_rank=final_rank, delivered=delivered)
