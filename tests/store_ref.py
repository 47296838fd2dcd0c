"""Reference of the streaming receive step -- TEST INFRASTRUCTURE ONLY.

Store: what qf_store_append_dev must leave in a row store, in plain numpy.
Every array starts as 0xCC, so comparing whole arrays with the device's also
checks the bytes an append must not write.  Per generation: n_rows above
max_rows or a taken row with row_len > L, row_off % 16 != 0 or row_off +
row_len > src_gen_stride is QF_EINVAL; otherwise more taken rows than free
slots is QF_ETOOSMALL; a generation that fails appends nothing.  The taken
rows go behind the old count in arrival order, round_up(row_len, 16) bytes
each with the bytes after row_len zero.

arrival / cauchy_arrival / cuts: the seeded traffic of the streaming tests, one
arrival sequence of vectors per generation and its split over calls;
tests/test_stream_recv_cpu.py asserts on the reference side that the seeds in
use contain the cases the device tests are about."""
from __future__ import annotations

import functools

import numpy as np

from tests import rank_ref

OK, EINVAL, ETOOSMALL = 0, -1, -7
FILL = 0xCC


def r16(x: int) -> int:
    return (x + 15) // 16 * 16


class Store:
    def __init__(self, G: int, k: int, L: int, cap: int, row_stride: int | None = None, gen_gap: int = 0):
        self.G, self.k, self.L, self.cap = G, k, L, cap
        self.row_stride = r16(L) + 16 if row_stride is None else row_stride
        self.gen_stride = cap * self.row_stride + gen_gap
        self.bytes = np.full((G, self.gen_stride), FILL, np.uint8)
        self.off = np.full((G, cap), 0xCCCCCCCC, np.uint32)
        self.len = np.full((G, cap), 0xCCCCCCCC, np.uint32)
        self.index = np.full((G, cap), 0xCCCC, np.uint16)
        self.coeffs = np.full((G, cap, k), FILL, np.uint8)
        self.n = np.zeros(G, np.uint32)

    def append(self, src, src_gen_stride, row_off, row_len, row_index, row_coeffs, n_rows=None, take=None):
        """src (G, >= src_gen_stride) bytes; row_off / row_len / row_index (G, mr);
        row_coeffs (G, mr, k); n_rows (G,) or None; take (G, mr) or None -> status (G,)."""
        G, mr = row_off.shape
        status = np.zeros(G, np.int32)
        for g in range(G):
            n = mr if n_rows is None else int(n_rows[g])
            if n > mr:
                status[g] = EINVAL
                continue
            taken = [s for s in range(n) if take is None or take[g, s]]
            bad = any(int(row_len[g, s]) > self.L or int(row_off[g, s]) % 16 or
                      int(row_off[g, s]) + int(row_len[g, s]) > src_gen_stride for s in taken)
            if bad:
                status[g] = EINVAL
                continue
            c0 = int(self.n[g])
            if c0 + len(taken) > self.cap:
                status[g] = ETOOSMALL
                continue
            for j, s in enumerate(taken):
                c = c0 + j
                o, ln = int(row_off[g, s]), int(row_len[g, s])
                at = c * self.row_stride
                self.bytes[g, at: at + r16(ln)] = 0
                self.bytes[g, at: at + ln] = src[g, o: o + ln]
                self.off[g, c], self.len[g, c], self.index[g, c] = at, ln, row_index[g, s]
                self.coeffs[g, c] = row_coeffs[g, s]
            self.n[g] = c0 + len(taken)
        return status


# ---------------------------------------------------------------------------
# seeded traffic
# ---------------------------------------------------------------------------
def _scale(oracle, v, c):
    e, lg = oracle.tables()
    e, lg = e.astype(np.int64), lg.astype(np.int64)
    if not c:
        return np.zeros_like(v)
    out = e[lg[v] + int(lg[c])].astype(np.uint8)
    out[v == 0] = 0
    return out


def arrival(oracle, rng, k: int):
    """One generation's arrival sequence of 5 k // 4 + 6 slots with explicit
    vectors -> idx (n,) u16 (a coded row has index k), coeffs (n, k), and the
    planted slots dict(pair, sys_a, sys_b): the coded row e_a + x e_b in slot
    0 or 1, source a as a systematic row about a third in, source b about half
    way (spanned by then, so not innovative).  Around them, shuffled:
    systematic rows of half the sources, repeats of some, random coded rows,
    combinations of two earlier rows and one zero vector."""
    n = 5 * k // 4 + 6
    few = max(1, k // 16)
    perm = [int(x) for x in rng.permutation(k)]
    a, b = perm[0], perm[1]
    sys_rest = perm[2: max(2, k // 2)]
    kinds = [("sys", i) for i in sys_rest]
    pool = sys_rest + [a]
    kinds += [("sys", pool[int(rng.integers(0, len(pool)))]) for _ in range(few)]
    kinds += [("dep", None)] * few + [("zero", None)]
    kinds += [("rnd", None)] * (n - 3 - len(kinds))
    order = [kinds[int(i)] for i in rng.permutation(len(kinds))]
    at_pair = int(rng.integers(0, 2))
    at_a, at_b = max(at_pair + 1, n // 3), max(at_pair + 2, n // 2)
    order.insert(at_pair, ("pair", None))
    order.insert(at_a, ("sys", a))
    order.insert(at_b, ("sys", b))
    assert len(order) == n
    idx = np.full(n, k, np.uint16)
    co = np.zeros((n, k), np.uint8)
    for s, (kind, i) in enumerate(order):
        if kind == "sys":
            idx[s] = i
            co[s, i] = 1
        elif kind == "pair":
            co[s, a], co[s, b] = 1, int(rng.integers(2, 256))
        elif kind == "rnd" or (kind == "dep" and s < 2):
            co[s] = rng.integers(0, 256, k)
        elif kind == "dep":
            p, q = (int(x) for x in rng.choice(s, 2, replace=False))
            co[s] = _scale(oracle, co[p], int(rng.integers(1, 256))) ^ _scale(oracle, co[q], int(rng.integers(1, 256)))
    return idx, co, dict(pair=at_pair, sys_a=at_a, sys_b=at_b, a=a, b=b)


def cauchy_arrival(rng, k: int, r: int):
    """Systematic rows and Cauchy rows k + j (j < r) without vectors, with
    repeats of both kinds: 5 k // 4 + 6 slots -> idx (n,) u16."""
    n = 5 * k // 4 + 6
    some = [int(x) for x in rng.permutation(k)[: k - 3]] + [k + j for j in range(r)]
    extra = [some[int(rng.integers(0, len(some)))] for _ in range(n - len(some))]
    out = some + extra
    return np.array([out[int(i)] for i in rng.permutation(n)], np.uint16)


def cuts(rng, n_slots, calls: int):
    """Per generation the slot counts of `calls` consecutive calls (they sum to
    the generation's n); about a third of the calls bring a generation nothing.
    The first generation gets its first quarter in the first call (an
    arrival() sequence has its planted pair there and the spanned systematic
    row half way) and its last two rows in the last call (behind the point
    where such a sequence reaches rank k)."""
    out = []
    for gi, n in enumerate(n_slots):
        head, tail, mid = (n // 4, 2, calls - 2) if gi == 0 else (0, 0, calls)
        w = rng.random(mid) * (rng.random(mid) > 0.35)
        if not w.any():
            w[int(rng.integers(0, mid))] = 1.0
        edges = np.floor(np.cumsum(w) / w.sum() * (n - head - tail) + 1e-9).astype(np.int64)
        edges[-1] = n - head - tail
        counts = np.diff(np.concatenate([[0], edges])).tolist()
        out.append(([head] + counts + [tail]) if gi == 0 else counts)
    return out


def vectors_of(k, idx, co):
    return rank_ref.vectors(k, 0, np.minimum(idx.astype(np.int64), k), co, None)


STREAM_K = (4, 8, 64, 65, 130, 256)      # every columns-per-lane count of the filter, and LDS above 64 KB
STREAM_SEED = {4: 40, 8: 80, 64: 640, 65: 650, 130: 1300, 256: 2560}
STREAM_CALLS = 5


@functools.lru_cache(maxsize=None)
def stream_case(k: int) -> dict:
    """The split-invariance traffic of generation size k: G arrival sequences
    (idx, coeffs, planted slots), the reference flags and ranks of each, and
    three seeded splits over STREAM_CALLS calls.  Computed once per process."""
    from tests import oracle_py

    G = 3 if k <= 65 else 2                # (the numpy elimination takes a second per generation at k = 256)
    rng = np.random.default_rng(STREAM_SEED[k])
    gens = [arrival(oracle_py, rng, k) for _ in range(G)]
    refs = [rank_ref.innovative(vectors_of(k, idx, co)) for idx, co, _ in gens]
    n = [len(g[0]) for g in gens]
    splits = [cuts(np.random.default_rng(1000 * STREAM_SEED[k] + j), n, STREAM_CALLS) for j in range(3)]
    return dict(k=k, G=G, idx=[g[0] for g in gens], co=[g[1] for g in gens], plant=[g[2] for g in gens],
                flags=[r[0] for r in refs], rank=[r[1] for r in refs], splits=splits)
