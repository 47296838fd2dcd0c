"""Reference of the streaming steps over a list -- TEST INFRASTRUCTURE ONLY.

select: the match rule of qf_gen_select_dev in plain numpy: generation g
matches iff rank[g] >= min_rank and (seen is None or rank[g] > seen[g]); the
first n_max matches in ascending order are the list; with mark the listed
generations' seen becomes their rank, the overflow stays unmarked.

gathered: "the dense batch a list stands for".  Entry j < n = min(n_sel, n_max)
with sel[j] < G_src gets the metadata of source generation sel[j] and a copy
of its region; an entry >= G_src is set aside (returned in `invalid`, n_rows 0
in the batch); entries n .. n_max - 1 have n_rows 0.  Regions and metadata of
entries that stand for nothing are 0xCC, so a call over the batch that looks
at them shows up.

listed_store: a row store (tests/store_ref.Store) of G_src generations filled
through Store.append with innovative rows only: generation 0 complete with a
ragged last row, generation 1 two rows short of k, the others complete, rows
of full length in every third generation (the payload pass's full path)."""
from __future__ import annotations

import functools

import numpy as np

from tests import store_ref

FILL = store_ref.FILL
UNUSED = 0xFFFFFFFF


def select(rank, seen, min_rank: int, n_max: int, mark: bool):
    """-> sel (list, ascending, <= n_max long), n_match, seen afterwards (None without seen)."""
    rank = np.asarray(rank, np.uint32)
    m = rank >= min_rank
    if seen is not None:
        m &= rank > np.asarray(seen, np.uint32)
    hits = np.flatnonzero(m)
    sel = hits[:n_max]
    after = None if seen is None else np.asarray(seen, np.uint32).copy()
    if mark:
        assert seen is not None
        after[sel] = rank[sel]
    return [int(g) for g in sel], int(hits.size), after


def used(sel, n_sel, n_max: int) -> int:
    return n_max if n_sel is None else min(int(n_sel), n_max)


def gathered(st: store_ref.Store, sel, n_sel, n_max: int):
    """-> Store-like batch of n_max generations (bytes, off, len, index, coeffs, n) and the invalid entries."""
    b = store_ref.Store(n_max, st.k, st.L, st.cap, row_stride=st.row_stride, gen_gap=st.gen_stride - st.cap * st.row_stride)
    invalid = []
    for j in range(used(sel, n_sel, n_max)):
        g = int(sel[j])
        if g >= st.G:
            invalid.append(j)
            continue
        b.bytes[j], b.off[j], b.len[j], b.index[j], b.coeffs[j], b.n[j] = (st.bytes[g], st.off[g], st.len[g],
                                                                           st.index[g], st.coeffs[g], st.n[g])
    return b, invalid


@functools.lru_cache(maxsize=None)
def listed_store(k: int, r: int, cap: int, L: int, G_src: int, seed: int):
    """-> Store, want_rank (G_src,): the rank each generation was built to have."""
    rng = np.random.default_rng(seed)
    st = store_ref.Store(G_src, k, L, cap)
    mr = k
    fs = store_ref.r16(L)
    want = np.full(G_src, k, np.uint32)
    want[1 % G_src] = max(k - 2, 0) if G_src > 1 else k
    region = np.full((G_src, mr * fs), FILL, np.uint8)
    ro = np.tile(np.arange(mr, dtype=np.uint32) * fs, (G_src, 1))
    rl = np.zeros((G_src, mr), np.uint32)
    idx = np.full((G_src, mr), k, np.uint16)
    co = np.zeros((G_src, mr, k), np.uint8)
    n = np.zeros(G_src, np.uint32)
    for g in range(G_src):
        e = int(rng.integers(1, min(k, r) + 1))             # erased sources: within the decode's capacity
        have = [int(x) for x in rng.permutation(k)[: k - e]]
        kinds = have + [k] * e
        order = [kinds[int(i)] for i in rng.permutation(k)][: int(want[g])]
        for s, i in enumerate(order):
            idx[g, s] = i
            if i < k:
                co[g, s, i] = 1
            else:
                co[g, s] = rng.integers(1, 256, k)
            rl[g, s] = L if g % 3 == 2 else int(rng.integers(max(1, L - 20), L + 1))
        if g == 0:
            rl[g, len(order) - 1] = L - 7 if L > 23 else L - 1   # a ragged last row: not a multiple of 16
        for s in range(len(order)):
            region[g, s * fs: s * fs + rl[g, s]] = rng.integers(0, 256, int(rl[g, s]), dtype=np.uint8)
        n[g] = len(order)
    status = st.append(region, mr * fs, ro, rl, idx, co, n)
    assert (status == store_ref.OK).all() and np.array_equal(st.n, want)
    return st, want


def special_list(rng, G_src: int, n_max: int):
    """A shuffled list of n_max entries with a duplicate (of generation 0, the
    ragged one), generation 1 (rank < k) and an entry >= G_src; the rest random."""
    base = [0, 1 % G_src, 0, G_src + 3]
    assert n_max >= len(base)
    base += [int(x) for x in rng.integers(0, G_src, n_max - len(base))]
    return [base[int(i)] for i in rng.permutation(n_max)]
