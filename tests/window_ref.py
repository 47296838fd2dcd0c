"""Reference of the generation window -- TEST INFRASTRUCTURE ONLY.

The window maps the unbounded generation ids of the wire onto the G_src slots
of a streaming receiver (qf_gen_window_dev, qf_gen_window_sel_dev): entry 0 is
an empty slot, otherwise bits 0..62 hold id + 1 and bit 63 the closed flag; the
slot of id x is x % G_src.  This module holds, in plain Python over numpy
arrays (the ids need all 64 bits, so the arithmetic is done on Python ints):

window:       every output of qf_gen_window_dev, 0xCC where the call writes
              nothing, and the window afterwards.
window_sel:   qf_gen_window_sel_dev: the ids of a list and the window
              afterwards (closed or only read).
make_case:    the seeded poll and prepared window of the case test, with the
              frames and slots of each case by name.
random_case:  a random window and poll for any G_src.
make_stream / simulate:  the seeded stream of the loop test and the whole loop
              under these rules alone, poll by poll."""
from __future__ import annotations

import functools

import numpy as np

from tests import poll_ref as PR

FILL32, FILL64 = 0xCCCCCCCC, 0xCCCCCCCCCCCCCCCC
OK, EINVAL, ENOTREADY, ESTALE, ECLOSED = 0, -1, -3, -8, -9
CLOSED = 1 << 63
ID_LIMIT = 1 << 62
GEN_NONE = 0xFFFFFFFF
NO_ID = (1 << 64) - 1


def held(entry: int):
    """The id an entry holds, None for an empty one."""
    entry = int(entry)
    return None if entry == 0 else (entry & ~CLOSED) - 1


class Windowed:
    """The outputs of qf_gen_window_dev."""

    def __init__(self, win, ids, n_frames, G_src: int, n_evict_max: int):
        N_max = len(ids)
        N = N_max if n_frames is None else min(int(n_frames), N_max)
        assert n_evict_max >= min(N_max, G_src)
        self.N = N
        self.before = np.array(win, np.uint64)
        self.win = self.before.copy()
        self.frame_gen = np.full(N_max, FILL32, np.uint32)
        self.frame_status = np.full(N_max, FILL32, np.uint32).view(np.int32)
        self.evict_sel = np.full(n_evict_max, FILL32, np.uint32)
        self.evict_id = np.full(n_evict_max, FILL64, np.uint64)
        newest = {}
        for f in range(N):
            x = int(ids[f])
            if x < ID_LIMIT:
                s = x % G_src
                newest[s] = max(newest.get(s, -1), x)
        self.touched = sorted(newest)
        evicted = []
        for s in self.touched:
            w = int(self.before[s])
            if w == 0 or newest[s] > held(w):
                self.win[s] = newest[s] + 1
                if w != 0 and not w & CLOSED:
                    evicted.append((s, held(w)))
        self.n_evict = len(evicted)
        for j, (s, x) in enumerate(evicted):
            self.evict_sel[j], self.evict_id[j] = s, x
        self.evicted = [s for s, _ in evicted]
        for f in range(N):
            x = int(ids[f])
            tag, st = GEN_NONE, EINVAL
            if x < ID_LIMIT:
                s = x % G_src
                w = int(self.win[s])
                if x < held(w):
                    st = ESTALE
                elif w & CLOSED:
                    st = ECLOSED
                else:
                    assert x == held(w)
                    tag, st = s, OK
            self.frame_gen[f], self.frame_status[f] = tag, st


def window(win, ids, n_frames, G_src: int, n_evict_max: int) -> Windowed:
    return Windowed(win, ids, n_frames, G_src, n_evict_max)


def window_sel(win, sel, n_sel, n_max: int, G_src: int, close: bool):
    """-> the window afterwards, ids (n_max,): every entry of ids is written."""
    out = np.array(win, np.uint64)
    n = n_max if n_sel is None else min(int(n_sel), n_max)
    ids = np.full(n_max, NO_ID, np.uint64)
    for j in range(n):
        g = int(sel[j])
        if g < G_src and int(win[g]) != 0:
            ids[j] = held(win[g])
            if close:
                out[g] = int(win[g]) | CLOSED
    return out, ids


# ---------------------------------------------------------------------------
# the case poll: G_src = 23, N_max = 300, one slot per case
# ---------------------------------------------------------------------------
G_CASE, N_CASE = 23, 300
BASE_CASE = ((1 << 40) // G_CASE + 1) * G_CASE            # a multiple of G_src above 2^40: both words are used
S_EMPTY_IDLE, S_OPEN_IDLE, S_CLOSED_IDLE = 0, 9, 22        # no frame maps to them
S_SMALL, S_SMALL_RING, S_BASE, S_TWO, S_THREE = 1, 2, 3, 4, 5
S_EVICT, S_OVER_CLOSED, S_CLOSED, S_STALE, S_SAME = 6, 7, 8, 10, 11
S_MAXID, S_INVALID_ONLY, S_EVICT_TWICE = 12, 13, 14        # (2^62 - 1) % 23 = 12, 2^62 % 23 = 13
S_RANDOM = tuple(range(15, 22))


def case_id(slot: int, cycle: int) -> int:
    return BASE_CASE + cycle * G_CASE + slot


@functools.lru_cache(maxsize=None)
def make_case(seed: int = 1):
    """-> win (23,) u64, ids (300,) u64, named: {case: frame numbers}."""
    rng = np.random.default_rng(4200 + seed)
    G = G_CASE
    win = [0] * G
    win[S_OPEN_IDLE] = case_id(S_OPEN_IDLE, 1) + 1
    win[S_CLOSED_IDLE] = (case_id(S_CLOSED_IDLE, 2) + 1) | CLOSED
    win[S_EVICT] = case_id(S_EVICT, 0) + 1
    win[S_OVER_CLOSED] = (case_id(S_OVER_CLOSED, 0) + 1) | CLOSED
    win[S_CLOSED] = (case_id(S_CLOSED, 1) + 1) | CLOSED
    win[S_STALE] = case_id(S_STALE, 1) + 1
    win[S_SAME] = case_id(S_SAME, 0) + 1
    win[S_INVALID_ONLY] = case_id(S_INVALID_ONLY, 0) + 1
    win[S_EVICT_TWICE] = case_id(S_EVICT_TWICE, 0) + 1
    frames = []                                            # (id, case name)
    frames += [(S_SMALL, "small")] * 3                     # an id < G_src
    frames += [(S_SMALL_RING + G, "small_ring")] * 2       # an id >= G_src, no base
    frames += [(case_id(S_BASE, 0), "base")] * 4
    frames += [(case_id(S_TWO, 0), "two_old")] * 3 + [(case_id(S_TWO, 1), "two_new")] * 3
    frames += [(case_id(S_THREE, 0), "three_old")] * 2 + [(case_id(S_THREE, 1), "three_mid")] * 2
    frames += [(case_id(S_THREE, 2), "three_new")] * 2
    frames += [(case_id(S_EVICT, 1), "evicts")] * 3
    frames += [(case_id(S_OVER_CLOSED, 1), "over_closed")] * 2
    frames += [(case_id(S_CLOSED, 1), "closed")] * 3
    frames += [(case_id(S_STALE, 0), "stale")] * 2 + [(case_id(S_STALE, 1), "current")] * 2
    frames += [(case_id(S_SAME, 0), "same")] * 3
    frames += [(ID_LIMIT - 1, "max_id"), (ID_LIMIT, "invalid"), (NO_ID, "invalid")]
    frames += [(case_id(S_EVICT_TWICE, 1), "twice_mid")] * 2 + [(case_id(S_EVICT_TWICE, 2), "twice_new")] * 2
    for s in S_RANDOM:                                     # random states against random cycles
        c0 = int(rng.integers(0, 4))
        win[s] = (0, case_id(s, c0) + 1, (case_id(s, c0) + 1) | CLOSED)[int(rng.integers(0, 3))]
    while len(frames) < N_CASE:
        s = int(rng.choice(S_RANDOM))
        frames.append((case_id(s, int(rng.integers(0, 6))), "random"))
    order = [int(i) for i in rng.permutation(N_CASE)]
    frames = [frames[i] for i in order]
    # the oldest id of a slot with several ids arrives last
    for old, others in (("two_old", ("two_new",)), ("three_old", ("three_mid", "three_new"))):
        last = max(f for f, (_, nm) in enumerate(frames) if nm in others + (old,))
        first_old = next(f for f, (_, nm) in enumerate(frames) if nm == old)
        frames[last], frames[first_old] = frames[first_old], frames[last]
    ids = np.array([x for x, _ in frames], np.uint64)
    named = {}
    for f, (_, nm) in enumerate(frames):
        named.setdefault(nm, []).append(f)
    return np.array(win, np.uint64), ids, named


@functools.lru_cache(maxsize=None)
def random_case(G_src: int, N: int, seed: int):
    """A random window of G_src slots (empty / open / closed) and N random ids around it."""
    rng = np.random.default_rng(seed * 7919 + G_src)
    base = ((1 << 40) // G_src + 1) * G_src
    state = rng.integers(0, 3, G_src)
    cyc = rng.integers(0, 4, G_src).astype(np.uint64)
    entry = np.uint64(base + 1) + cyc * np.uint64(G_src) + np.arange(G_src, dtype=np.uint64)
    win = np.where(state == 0, np.uint64(0), np.where(state == 2, entry | np.uint64(CLOSED), entry)).astype(np.uint64)
    slots = rng.integers(0, G_src, N).astype(np.uint64)
    ids = np.uint64(base) + rng.integers(0, 6, N).astype(np.uint64) * np.uint64(G_src) + slots
    return win, ids.astype(np.uint64)


# ---------------------------------------------------------------------------
# the loop past the ring
# ---------------------------------------------------------------------------
K_LOOP, R_LOOP, L_LOOP, G_LOOP, GENS_LOOP = 8, 4, 100, 11, 40
N_LOOP, MR_LOOP, LIST_LOOP = 24, 3, 6
BASE_LOOP = (1 << 40) + 3
SEED_LOOP = 0


def make_stream(seed: int = SEED_LOOP):
    """The arrival order of the stream: (generation g, frame s), s < k a
    systematic frame, s >= k the Cauchy repair s - k.  Per-frame loss 0.15, 0.6
    for every fifth generation; the order jittered by about one generation."""
    rng = np.random.default_rng(9100 + seed)
    n = K_LOOP + R_LOOP
    arrivals = []
    for g in range(GENS_LOOP):
        loss = 0.6 if g % 5 == 2 else 0.15
        for s in range(n):
            if rng.random() >= loss:
                arrivals.append((g * n + s + float(rng.uniform(-n, n)), g, s))
    arrivals.sort()
    return [(g, s) for _, g, s in arrivals]


class PollRecord:
    """One poll of the loop under the model: what the device must produce."""


@functools.lru_cache(maxsize=None)
def simulate(seed: int = SEED_LOOP):
    """The whole loop over make_stream(seed) -> records (one PollRecord per
    poll), stats.  Any k distinct frames of a generation are independent
    (systematic rows and Cauchy repairs), so a slot's rank is the number of
    distinct frames it ingested, k at the most."""
    k, G, N_max, mr, n_list = K_LOOP, G_LOOP, N_LOOP, MR_LOOP, LIST_LOOP
    queue = make_stream(seed)
    win = np.zeros(G, np.uint64)
    have = [set() for _ in range(G)]
    seen = [0] * G
    delivered = {}
    stats = dict(completions=0, evictions=0, evictions_with_rows=0, stale=0, closed=0, full_lists=0, polls=0)
    records = []
    while queue:
        stats["polls"] += 1
        assert stats["polls"] < 400
        # the poll ring: at most N_max frames and at most max_rows of an id per poll, the rest waits in order
        take, wait, count, blocked = [], [], {}, set()
        for g, s in queue:
            if len(take) < N_max and count.get(g, 0) < mr and g not in blocked:
                take.append((g, s))
                count[g] = count.get(g, 0) + 1
            else:
                wait.append((g, s))
                blocked.add(g)
        rec = PollRecord()
        rec.take, rec.n = take, len(take)
        rec.ids = np.full(N_max, FILL64, np.uint64)
        rec.ids[: rec.n] = [BASE_LOOP + g for g, _ in take]
        rec.w = window(win, rec.ids, rec.n, G, G)
        win = rec.w.win.copy()
        rec.evicted_with_rows = [s for s in rec.w.evicted if have[s]]
        for s in rec.w.evicted:
            have[s], seen[s] = set(), 0
        stats["evictions"] += rec.w.n_evict
        stats["evictions_with_rows"] += len(rec.evicted_with_rows)
        sel, n_match, entries, est, tag_status = PR.group(rec.w.frame_gen, rec.n, G, n_list, mr)
        assert (est == OK).all()
        rec.sel, rec.n_match = sel, n_match
        stats["full_lists"] += n_match > len(sel)
        rec.status = []
        for f in range(rec.n):
            st = int(rec.w.frame_status[f])
            if st == OK and tag_status[f] is not None:
                st = tag_status[f]
            assert st in (OK, ENOTREADY, ESTALE, ECLOSED)
            rec.status.append(st)
            stats["stale"] += st == ESTALE
            stats["closed"] += st == ECLOSED
            if st == OK:
                have[int(rec.w.frame_gen[f])].add(take[f])
        rank = [min(k, len(h)) for h in have]
        rec.rank = rank
        rec.completed = [s for s in range(G) if rank[s] >= k and rank[s] > seen[s]][:n_list]
        rec.labels = [held(win[s]) for s in rec.completed]
        for s, x in zip(rec.completed, rec.labels):
            assert x not in delivered, "a generation is delivered twice"
            delivered[x] = stats["polls"]
            win[s] = int(win[s]) | CLOSED
            have[s], seen[s] = set(), 0
        stats["completions"] += len(rec.completed)
        rec.win_after = win.copy()
        records.append(rec)
        queue = [take[f] for f in range(rec.n) if rec.status[f] == ENOTREADY] + wait
    stats["delivered"] = delivered
    return records, stats
