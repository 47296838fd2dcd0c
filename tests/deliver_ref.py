"""Reference of the delivery step -- TEST INFRASTRUCTURE ONLY.

deliver:     every output of qf_deliver_frames_dev / qf_deliver_frames_sel_dev
             over arrays laid out as the calls take them.  The outputs start as
             the buffers the caller passes in (0xCC in the tests), so the bytes
             a call must not write are part of the result.
loop_model:  a stream of wire generations through the streaming receive loop of
             INTEGRATION.md under the models alone (window_ref, partial_ref and
             this module): the window, deliver step 1b over the evict list, the
             ingest, deliver step 7a over the completed list, the resets, and
             two deadline flushes in mid-stream.  G_src = 4, k = 4, L = 48.

Plain numpy; the ids and state words need all 64 bits, so that arithmetic is
done on Python ints."""
from __future__ import annotations

import functools

import numpy as np

from tests import partial_ref as P
from tests import rank_ref
from tests import window_ref as WR

OK, EINVAL, ENOTREADY = 0, -1, -3
NONE16 = 0xFFFF
WORDS = 5
UNKNOWN, STORED, RECOVERED, EARLIER = 0, 1, 2, 3
ID_LIMIT = 1 << 62
FILL = 0xCC


def r16(x: int) -> int:
    return (x + 15) // 16 * 16


class Shape:
    """qf_deliver_shape."""

    def __init__(self, k, e_max, L, max_rows, src_gs, rec_rs, rec_gs, out_rs, out_gs):
        self.k, self.e_max, self.L, self.max_rows = k, e_max, L, max_rows
        self.src_gs, self.rec_rs, self.rec_gs, self.out_rs, self.out_gs = src_gs, rec_rs, rec_gs, out_rs, out_gs


def poisoned(sh: Shape, G: int, guard: int = 0) -> dict:
    """The six output buffers of a call over G entries, every byte 0xCC."""
    k = sh.k
    return dict(out=np.full(G * sh.out_gs + guard, FILL, np.uint8), out_len=np.full(G * k + guard // 4, 0xCCCCCCCC, np.uint32),
                out_state=np.full(G * k + guard, FILL, np.uint8), n_out=np.full(G + guard // 4, 0xCCCCCCCC, np.uint32),
                n_known=np.full(G + guard // 4, 0xCCCCCCCC, np.uint32),
                status=np.full(G + guard // 4, 0xCCCCCCCC, np.uint32).view(np.int32))


def deliver(sh: Shape, G: int, src, row_off, row_len, rec, rec_index, n_rec, dec_status, src_slot, ids=None,
            delivered=None, sel=None, n_sel=None, G_src=None, into=None) -> dict:
    """-> out, out_len, out_state, n_out, n_known, status (copies of `into`,
    poisoned() when None, with the call's writes), delivered (the state
    afterwards, None without one), packets: per entry the (source, bytes) pairs
    that left, and reads: per entry the (which, offset, length) payload ranges
    the call may read.
    src: flat u8 of the source generations; row_off / row_len (G_src,
    max_rows); rec flat u8 or None; rec_index (G, e_max); n_rec, dec_status
    (G,); src_slot (G, k); ids (G,) u64 or None; delivered (G_src, 5) u64 or
    None.  sel: a list of G entries (the listed form), n_sel a count or None."""
    k, L, mr, em = sh.k, sh.L, sh.max_rows, sh.e_max
    o = {key: v.copy() for key, v in (poisoned(sh, G) if into is None else into).items()}
    state = None if delivered is None else np.array(delivered, np.uint64).reshape(-1, WORDS).copy()
    rec_index = np.asarray(rec_index, np.uint16).reshape(G, em) if em else np.zeros((G, 0), np.uint16)
    src_slot = np.asarray(src_slot, np.uint16).reshape(G, k)
    row_off = np.asarray(row_off, np.uint32).reshape(-1, mr)
    row_len = np.asarray(row_len, np.uint32).reshape(-1, mr)
    n_used = G
    if sel is not None and n_sel is not None:
        n_used = min(int(n_sel), G)
    packets, reads = [], []
    for j in range(G):
        packets.append([])
        reads.append([])

        def nothing(status):
            o["out_len"][j * k: (j + 1) * k] = 0
            o["out_state"][j * k: (j + 1) * k] = 0
            o["n_out"][j], o["n_known"][j], o["status"][j] = 0, 0, status

        gs = j
        if sel is not None:
            if j >= n_used:
                nothing(ENOTREADY)
                continue
            gs = int(sel[j])
            if gs >= G_src:
                nothing(EINVAL)
                continue
        if int(dec_status[j]) not in (OK, ENOTREADY):
            nothing(ENOTREADY)
            continue
        tagged = state is not None and ids is not None
        tag = 0
        if tagged:
            x = int(ids[j])
            if x >= ID_LIMIT:
                nothing(EINVAL)
                continue
            tag = x + 1
        nr = int(n_rec[j])
        if nr > em:
            nothing(EINVAL)
            continue
        slots = [int(s) for s in src_slot[j]]
        D = [int(i) for i in rec_index[j, :nr]]
        bad = any(s != NONE16 and s >= mr for s in slots) or any(i >= k for i in D)
        if not bad:
            S = [i for i in range(k) if slots[i] != NONE16]
            named = S + D
            bad = len(set(named)) != len(named)
            for i in S:
                off, ln = int(row_off[gs, slots[i]]), int(row_len[gs, slots[i]])
                bad = bad or ln > L or off % 16 != 0 or off + ln > sh.src_gs
        if bad:
            nothing(EINVAL)
            continue
        old = [0] * 4
        if state is not None and (not tagged or int(state[gs, 0]) == tag):
            old = [int(w) for w in state[gs, 1:]]
        marked = {i for i in range(k) if old[i // 64] >> (i % 64) & 1}
        known = set(S) | set(D)
        new = sorted(known - marked)
        for i in range(k):
            at = j * k + i
            if i in new:
                if slots[i] != NONE16:
                    off, ln = int(row_off[gs, slots[i]]), int(row_len[gs, slots[i]])
                    data = np.asarray(src[gs * sh.src_gs + off: gs * sh.src_gs + off + ln], np.uint8)
                    reads[j].append(("src", gs * sh.src_gs + off, ln))
                    o["out_state"][at] = STORED
                else:
                    m = D.index(i)
                    ln = L
                    data = np.asarray(rec[j * sh.rec_gs + m * sh.rec_rs: j * sh.rec_gs + m * sh.rec_rs + L], np.uint8)
                    reads[j].append(("rec", j * sh.rec_gs + m * sh.rec_rs, ln))
                    o["out_state"][at] = RECOVERED
                base = j * sh.out_gs + i * sh.out_rs
                o["out"][base: base + r16(ln)] = 0
                o["out"][base: base + ln] = data
                o["out_len"][at] = ln
                packets[j].append((i, data.tobytes()))
            else:
                o["out_len"][at] = 0
                o["out_state"][at] = EARLIER if i in marked else UNKNOWN
        o["n_out"][j], o["n_known"][j], o["status"][j] = len(new), len(known | marked), OK
        if state is not None and new:
            for i in new:
                old[i // 64] |= 1 << (i % 64)
            state[gs, 1:] = old
            if tagged:
                state[gs, 0] = tag
    o["delivered"], o["packets"], o["reads"] = state, packets, reads
    return o


# ---------------------------------------------------------------------------
# a decode's outputs from the model of the decode
# ---------------------------------------------------------------------------
def decode_outputs(sh: Shape, refs, fill: bool = True) -> dict:
    """partial_ref results (one per entry) as the arrays the decode calls leave:
    rec (flat, 0xCC where nothing is written), rec_index, n_rec, dec_status,
    src_slot."""
    G, k, em = len(refs), sh.k, sh.e_max
    rec = np.full(G * sh.rec_gs, FILL if fill else 0, np.uint8)
    ri = np.full((G, em), 0xCCCC if fill else 0, np.uint16)
    nrec, st = np.zeros(G, np.uint32), np.zeros(G, np.int32)
    slot = np.full((G, k), NONE16, np.uint16)
    for g, ref in enumerate(refs):
        for m, i in enumerate(ref["D"]):
            rec[g * sh.rec_gs + m * sh.rec_rs: g * sh.rec_gs + m * sh.rec_rs + sh.L] = ref["rec"][m]
            ri[g, m] = i
        nrec[g], st[g] = len(ref["D"]), ref["status"]
        slot[g] = ref["src_slot"]
    return dict(rec=rec, rec_index=ri, n_rec=nrec, dec_status=st, src_slot=slot)


class Call:
    """The inputs of one call as host arrays, and the model over them."""

    def __init__(self, sh: Shape, G: int, src, row_off, row_len, dec: dict, ids=None, delivered=None, sel=None,
                 n_sel=None, G_src=None):
        self.sh, self.G, self.src, self.row_off, self.row_len, self.dec = sh, G, src, row_off, row_len, dec
        self.ids, self.delivered, self.sel, self.n_sel, self.G_src = ids, delivered, sel, n_sel, G_src

    def model(self, into=None, delivered="own") -> dict:
        d = self.dec
        return deliver(self.sh, self.G, self.src, self.row_off, self.row_len, d["rec"], d["rec_index"], d["n_rec"],
                       d["dec_status"], d["src_slot"], ids=self.ids,
                       delivered=self.delivered if isinstance(delivered, str) else delivered, sel=self.sel,
                       n_sel=self.n_sel, G_src=self.G_src, into=into)


def synth(rng, sh: Shape, specs, G_src=None) -> Call:
    """A dense call (or the source side of a listed one) from a description per
    generation: dict(stored={source: (slot, length)}, D=[recovered sources in
    rec order], status=OK).  Rows of random nonzero bytes, row s of a
    generation at offset (max_rows - 1 - s) * row stride (the arrival order is
    not the address order) when the region holds max_rows rows, else packed in
    slot order of use; 0xCC everywhere else."""
    G, k, mr, em, L = len(specs), sh.k, sh.max_rows, sh.e_max, sh.L
    rs = r16(L)
    src = np.full(G * sh.src_gs, FILL, np.uint8)
    off = np.full((G, mr), 0xCCCCCCCC, np.uint32)
    ln = np.full((G, mr), 0xCCCCCCCC, np.uint32)
    rec = np.full(G * sh.rec_gs, FILL, np.uint8)
    ri = np.full((G, em), 0xCCCC, np.uint16)
    nrec, st = np.zeros(G, np.uint32), np.zeros(G, np.int32)
    slot = np.full((G, k), NONE16, np.uint16)
    dense = mr * rs <= sh.src_gs
    for g, spec in enumerate(specs):
        for t, (i, (s, n)) in enumerate(sorted(spec.get("stored", {}).items())):
            o = (mr - 1 - s) * rs if dense else t * rs
            assert o + r16(n) <= sh.src_gs
            off[g, s], ln[g, s], slot[g, i] = o, n, s
            src[g * sh.src_gs + o: g * sh.src_gs + o + n] = rng.integers(1, 256, n, dtype=np.uint8)
        for m, i in enumerate(spec.get("D", [])):
            ri[g, m] = i
            rec[g * sh.rec_gs + m * sh.rec_rs: g * sh.rec_gs + m * sh.rec_rs + L] = rng.integers(1, 256, L, dtype=np.uint8)
        nrec[g], st[g] = len(spec.get("D", [])), spec.get("status", OK)
    return Call(sh, G, src, off, ln, dict(rec=rec, rec_index=ri, n_rec=nrec, dec_status=st, src_slot=slot), G_src=G_src)


INCONSISTENT = ("slot", "n_rec", "rec_index", "twice", "both", "len", "align", "past")


def inconsistent_call(what: str) -> Call:
    """Three generations that each store sources 0 and 4 (slots 1 and 2) and
    recover 1 and 3, k = 5, with generation 1 made inconsistent; a zeroed state
    and the ids 5, 6, 7."""
    sh = simple_shape(5, 3, 20, 6)
    good = dict(stored={0: (1, 20), 4: (2, 3)}, D=[1, 3])
    c = synth(np.random.default_rng(3), sh, [good, good, good])
    d = c.dec
    if what == "slot":
        d["src_slot"][1, 2] = sh.max_rows
    elif what == "n_rec":
        d["n_rec"][1] = sh.e_max + 1
    elif what == "rec_index":
        d["rec_index"][1, 1] = sh.k
    elif what == "twice":
        d["rec_index"][1, 1] = 1
    elif what == "both":
        d["rec_index"][1, 0] = 4
    elif what == "len":
        c.row_len[1, 2] = sh.L + 1
    elif what == "align":
        c.row_off[1, 1] += 8
    elif what == "past":
        c.row_off[1, 2], c.row_len[1, 2] = sh.src_gs - 16, 17
    else:
        assert what == "none"
    c.delivered = np.zeros((3, WORDS), np.uint64)
    c.ids = np.array([5, 6, 7], np.uint64)
    return c


def simple_shape(k, e_max, L, max_rows, rows_held=None, out_pad=0) -> Shape:
    """Strides with a gap behind every row and generation; rows_held: the rows
    a source region has room for (None: max_rows)."""
    rs = r16(L)
    held = max_rows if rows_held is None else rows_held
    return Shape(k, e_max, L, max_rows, held * rs + 32, rs + 16, e_max * (rs + 16) + 48, rs + out_pad,
                 k * (rs + out_pad) + 32)


def random_specs(rng, sh: Shape, G: int, lens=None):
    """Per generation a random split of the sources into stored, recovered (at
    most e_max) and unknown, slots a random choice of max_rows, lengths from
    `lens` (None: 0, 1, 16, L and random ones)."""
    k, L = sh.k, sh.L
    specs = []
    for g in range(G):
        order = rng.permutation(k)
        n_d = int(rng.integers(0, min(sh.e_max, k) + 1))
        n_s = int(rng.integers(0, min(k - n_d, sh.max_rows) + 1))
        D = sorted(int(i) for i in order[:n_d])
        S = [int(i) for i in order[n_d: n_d + n_s]]
        slots = rng.choice(sh.max_rows, n_s, replace=False)
        pool = lens if lens is not None else [0, 1, min(16, L), L, int(rng.integers(0, L + 1))]
        stored = {i: (int(s), int(pool[int(rng.integers(0, len(pool)))])) for i, s in zip(S, slots)}
        specs.append(dict(stored=stored, D=D, status=OK if n_d + n_s == k else ENOTREADY))
    return specs


# ---------------------------------------------------------------------------
# the shapes of the device test and of the host emulation: synthetic decode outputs
# ---------------------------------------------------------------------------
def _with_state(rng, c, marked=True):
    """A state and ids for a dense call: every other generation starts with
    random sources of its wire generation marked, one with another generation's tag."""
    k, G = c.sh.k, c.G
    c.ids = (np.uint64(1 << 40) + rng.integers(0, 1 << 20, G).astype(np.uint64)).astype(np.uint64)
    st = np.zeros((G, WORDS), np.uint64)
    for g in range(G):
        if marked and g % 2 == 0:
            bits = [int(b) for b in rng.integers(0, 2, k)]
            st[g, 0] = int(c.ids[g]) + 1 if g % 4 == 0 or G < 3 else int(c.ids[g]) + 5
            for i, b in enumerate(bits):
                if b:
                    st[g, 1 + i // 64] |= np.uint64(1 << (i % 64))
    c.delivered = st
    return c


def shape_cases():
    """name -> Call.  k at the mask-word and lanes-per-source edges, L at the
    unit edges with row lengths 0, 1, 16 and L mixed, a wide out_row_stride,
    slots above 255, e_max 0 without rec, n_rec 0 and e_max."""
    cases = {}
    for k in (1, 3, 64, 65, 128, 129, 256):
        rng = np.random.default_rng(k)
        em = min(k, 6)
        sh = simple_shape(k, em, 33, k + 3)
        specs = random_specs(rng, sh, 3)
        specs.append(dict(stored={i: (k + 2 - i, 33 if i % 3 else i % 34) for i in range(k)}))      # every source stored
        rest = [i for i in range(k) if i >= em]
        specs.append(dict(stored={i: (i, 16) for i in rest}, D=list(range(em))[::-1]))              # n_rec = e_max
        specs.append(dict(stored={i: (i, 1) for i in range(0, k, 2)}, D=[], status=ENOTREADY))        # n_rec = 0
        cases[f"k{k}"] = _with_state(rng, synth(rng, sh, specs))
    for L in (1, 15, 16, 17, 33, 1200):
        rng = np.random.default_rng(1000 + L)
        sh = simple_shape(5, 2, L, 6)
        pool = sorted({0, 1, min(16, L), L})
        cases[f"L{L}"] = _with_state(rng, synth(rng, sh, random_specs(rng, sh, 6, lens=pool)), marked=False)
    rng = np.random.default_rng(7)
    sh = simple_shape(7, 3, 40, 9, out_pad=32)
    cases["wide_out_rows"] = synth(rng, sh, random_specs(rng, sh, 5))
    sh = simple_shape(4, 1, 20, 1024, rows_held=4)
    cases["slots_above_255"] = _with_state(rng, synth(rng, sh, [dict(stored={0: (1000, 20), 1: (255, 3), 2: (256, 0)}, D=[3]),
                                                                 dict(stored={3: (1023, 17)}, status=ENOTREADY)]),
                                           marked=False)
    sh = simple_shape(6, 0, 24, 8)
    c = synth(rng, sh, [dict(stored={i: (7 - i, 24 - i) for i in range(6)}), dict(stored={2: (0, 5)}, status=ENOTREADY)])
    c.dec["rec"] = None
    c.dec["rec_index"] = None
    cases["e_max_0"] = c
    return cases


# ---------------------------------------------------------------------------
# the loop: G_src = 4, k = 4, L = 48
# ---------------------------------------------------------------------------
K_LOOP, R_LOOP, L_LOOP, G_LOOP, GENS_LOOP, N_LOOP, MR_LOOP = 4, 4, 48, 4, 30, 24, 8
BASE_LOOP = (1 << 40) + 1
FLUSH_AFTER = (5, 6, 13, 14, 21, 22)      # deadline flushes behind these polls


def loop_stream(rng):
    """Per wire generation the frames that survive, (source index or k + j,
    vector): the systematic frames and R_LOOP sparse repairs.  Loss by
    generation: none, a quarter, a half and three quarters of the frames in
    turn, so that generations complete at once, complete late, and never."""
    k = K_LOOP
    gens = []
    for g in range(GENS_LOOP):
        frames = [(i, P.unit(k, i)) for i in range(k)]
        frames += [(k + j, P.over(rng, k, rng.choice(k, 2 + j % 2, replace=False).tolist())) for j in range(R_LOOP)]
        loss = (0.0, 0.3, 0.55, 0.75)[(g // 2) % 4] if g % 7 != 3 else 0.0
        fr = [f for f in frames if rng.random() >= loss]
        gens.append([fr[i] for i in rng.permutation(len(fr))])
    return gens


class Slot:
    """The model of one slot's row store: the innovative rows in arrival order."""

    def __init__(self):
        self.idx, self.vec, self.pay = [], [], []

    def add(self, i, v, row):
        vec = P.unit(K_LOOP, i) if i < K_LOOP else v
        if rank_ref.innovative(np.stack(self.vec + [vec]))[1] > len(self.vec):
            self.idx.append(i)
            self.vec.append(vec)
            self.pay.append(row)

    def ref(self):
        co = np.stack(self.vec) if self.vec else np.zeros((0, K_LOOP), np.uint8)
        return P.partial_ref(K_LOOP, R_LOOP, L_LOOP, np.array(self.idx, np.int64), co, [p.tobytes() for p in self.pay])


class Step:
    """One deliver call of the loop under the model: the listed slots, the wire
    generations they hold, the decode's references, the state before the call
    and the model's result."""


class LoopPoll:
    """One poll of the loop under the model alone."""


def loop_shape() -> Shape:
    k, Lb = K_LOOP, L_LOOP
    rs = r16(Lb)
    return Shape(k, min(k, R_LOOP), Lb, k, k * rs + 32, rs + 16, min(k, R_LOOP) * (rs + 16), rs, k * rs)


def _store_arrays(sh: Shape, slots):
    """The stores of all slots as qf_store_append_dev leaves them: row c at c * store_row_stride."""
    G, rs = len(slots), r16(sh.L)
    src = np.full(G * sh.src_gs, FILL, np.uint8)
    off = np.full((G, sh.max_rows), 0xCCCCCCCC, np.uint32)
    ln = np.full((G, sh.max_rows), 0xCCCCCCCC, np.uint32)
    for s, slot in enumerate(slots):
        for c, row in enumerate(slot.pay):
            off[s, c], ln[s, c] = c * rs, len(row)
            src[s * sh.src_gs + c * rs: s * sh.src_gs + c * rs + len(row)] = row
    return src, off, ln


@functools.lru_cache(maxsize=None)
def loop_model():
    """-> src (GENS, k, L), stream, polls, stats.  Generation g's surviving
    frames go out in polls g, g + 1 and g + 2; it is displaced by generation g +
    G_LOOP.  Each poll holds the deliver steps it runs (q.evict 1b, q.done 7a,
    q.flush a deadline flush behind the poll, or None)."""
    k, G, N = K_LOOP, G_LOOP, N_LOOP
    sh = loop_shape()
    rng = np.random.default_rng(31)
    stream = loop_stream(rng)
    src = rng.integers(1, 256, (GENS_LOOP, k, L_LOOP), dtype=np.uint8)
    win =np.zeros(G, np.uint64)
    slots = [Slot() for _ in range(G)]
    holds = [None] * G
    state = np.zeros((G, WORDS), np.uint64)
    left = {}                 # (wire generation, source) -> the bytes that left
    determined = {}           # wire generation -> the sources some decode reported
    flushed = set()
    stats = dict(flushed_then_completed=0, flushed_then_displaced=0, slot_reused=0, earlier=0, completed=0, displaced=0)

    def step(listed, id_of):
        """deliver over the listed (slot, generation) pairs; id_of: the ids the device call is given."""
        st = Step()
        st.listed = listed
        st.refs = [slots[s].ref() for s, _ in listed]
        nothing = P.partial_ref(k, R_LOOP, L_LOOP, [], np.zeros((0, k), np.uint8), [])
        st.dec = decode_outputs(sh, st.refs + [nothing] * (G - len(listed)))
        st.ids = np.full(G, WR.NO_ID, np.uint64)
        st.ids[: len(listed)] = [id_of(g) for _, g in listed]
        st.sel = [s for s, _ in listed]
        st.before = state.copy()
        store = _store_arrays(sh, slots)
        st.res = deliver(sh, G, *store, st.dec["rec"], st.dec["rec_index"], st.dec["n_rec"], st.dec["dec_status"],
                         st.dec["src_slot"], ids=st.ids, delivered=state, sel=st.sel + [0] * (G - len(listed)),
                         n_sel=len(listed), G_src=G)
        state[:] = st.res["delivered"]
        for j, (s, g) in enumerate(listed):
            ref = st.refs[j]
            assert st.res["status"][j] == OK and ref["status"] in (OK, ENOTREADY)
            tag = int(st.before[s, 0])
            stats["slot_reused"] += tag not in (0, BASE_LOOP + g + 1)
            stats["earlier"] += int((st.res["out_state"][j * k: (j + 1) * k] == EARLIER).sum())
            determined.setdefault(g, set()).update(i for i in range(k) if ref["src_slot"][i] != NONE16)
            determined[g].update(ref["D"])
            for i, data in st.res["packets"][j]:
                assert (g, i) not in left, f"source {i} of generation {g} left twice"
                left[(g, i)] = data
        return st

    polls = []
    for poll in range(GENS_LOOP + 2):
        q = LoopPoll()
        take = []
        for g in range(max(0, poll - 2), min(poll + 1, GENS_LOOP)):
            fr = stream[g]
            third = -(-len(fr) // 3)
            take += [(g, f) for f in fr[(poll - g) * third: (poll - g + 1) * third]]
        q.take = [take[i] for i in rng.permutation(len(take))]
        assert len(q.take) <= N
        q.ids = np.full(N, BASE_LOOP, np.uint64)
        q.ids[: len(q.take)] = [BASE_LOOP + g for g, _ in q.take]
        q.w = WR.window(win, q.ids, len(q.take), G, G)
        win = q.w.win
        # 1b: what the displaced generations hold leaves before their slots are reset
        assert [holds[s] for s in q.w.evicted] == [int(x) - BASE_LOOP for x in q.w.evict_id[: q.w.n_evict]]
        q.evict = step([(s, holds[s]) for s in q.w.evicted], lambda g: BASE_LOOP + g)
        for s in q.w.evicted:
            stats["displaced"] += 1
            stats["flushed_then_displaced"] += holds[s] in flushed
            slots[s], holds[s] = Slot(), None
        q.rows = []
        for f, (g, (i, v)) in enumerate(q.take):
            row = P.encode_rows(v[None, :], src[g])[0]
            q.rows.append(row)
            if q.w.frame_status[f] == WR.OK:
                s = int(q.w.frame_gen[f])
                assert holds[s] in (None, g)
                holds[s] = g
                slots[s].add(i, v, row)
        # 7a: the completed generations, with the ids their slots hold
        done = [(s, holds[s]) for s in range(G) if len(slots[s].idx) == k]
        q.done = step(done, lambda g: BASE_LOOP + g)
        for s, g in done:
            stats["completed"] += 1
            stats["flushed_then_completed"] += g in flushed
            slots[s], holds[s] = Slot(), None
        win, _ = WR.window_sel(win, [s for s, _ in done], len(done), G, G, True)
        q.win_after = win
        # a deadline flush: every slot that holds a row, nothing is reset
        q.flush = None
        if poll in FLUSH_AFTER:
            listed = [(s, holds[s]) for s in range(G) if slots[s].idx]
            q.flush = step(listed, lambda g: BASE_LOOP + g)
            flushed.update(g for _, g in listed)
        polls.append(q)
    # the end of the stream: a last flush over what is left
    last = LoopPoll()
    last.flush = step([(s, holds[s]) for s in range(G) if slots[s].idx], lambda g: BASE_LOOP + g)
    stats["left"], stats["determined"] = left, determined
    return src, stream, polls, last, stats


def check_exactly_once(src, left, determined):
    """Every (wire generation, source) some decode determined has left, once
    (step() asserts that), with the source's bytes; nothing else has."""
    want = {(g, i) for g, known in determined.items() for i in known}
    assert set(left) == want, (sorted(set(left) - want)[:4], sorted(want - set(left))[:4])
    for (g, i), data in left.items():
        row = np.zeros(src.shape[2], np.uint8)
        row[: len(data)] = np.frombuffer(data, np.uint8)
        assert np.array_equal(row, src[g, i]), (g, i)


def check_loop_stats(stats):
    """The stream holds what the loop tests are about."""
    assert stats["flushed_then_completed"] >= 1 and stats["flushed_then_displaced"] >= 1, stats
    assert stats["slot_reused"] >= 1 and stats["earlier"] >= 4, stats
    assert stats["completed"] >= 6 and stats["displaced"] >= 6, stats
