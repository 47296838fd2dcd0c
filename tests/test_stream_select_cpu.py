"""tests/select_ref.py holds the cases tests/test_gpu_stream_select.py is about
(CPU only): more matches than n_max, a generation that completes exactly in
the poll beside one that was complete before, QF_SELECT_MARK leaving the
overflow unmarked for the next call, and lists with a duplicate, a descending
pair, an invalid entry and a count below n_max."""
import numpy as np

from tests import rank_ref, select_ref, store_ref

# (k, r, cap, L, G_src, n_max, seed) of the listed decode; the first two also serve the listed recode
SHAPES = [(4, 4, 6, 40, 37, 9, 4406), (64, 16, 64, 1200, 12, 5, 6416), (200, 8, 200, 1040, 3, 4, 2008)]
SELECT_G = (1, 63, 64, 65, 1025, 70001)


def select_inputs(G: int):
    """rank / seen of the select tests at k = 8: a third complete, half of those seen before."""
    rng = np.random.default_rng(G)
    k = 8
    rank = rng.integers(0, k, G).astype(np.uint32)
    rank[rng.random(G) < 0.4] = k
    rank[G - 1] = k                                   # the ragged final block has a match in its last lane
    seen = np.where(rng.random(G) < 0.5, rank, rng.integers(0, k, G)).astype(np.uint32)
    seen = np.minimum(seen, rank)
    return k, rank, seen


def test_select_rule_and_overflow():
    for G in SELECT_G:
        k, rank, seen = select_inputs(G)
        full, n_all, _ = select_ref.select(rank, None, k, G, False)
        assert n_all == int((rank == k).sum()) >= 1 and full == sorted(full)
        fresh, n_fresh, _ = select_ref.select(rank, seen, k, G, False)
        assert set(fresh) <= set(full)
        if G >= 63:
            # one completes exactly now, one was complete (and seen) before
            assert 0 < n_fresh < n_all
            assert any(rank[g] == k and seen[g] == k for g in range(G))
            assert any(rank[g] == k and seen[g] < k for g in range(G))
            # overflow: n_max below the match count; MARK leaves the rest for the next call
            n_max = n_fresh // 2
            assert 0 < n_max < n_fresh
            a, na, seen1 = select_ref.select(rank, seen, k, n_max, True)
            assert a == fresh[:n_max] and na == n_fresh
            assert all(seen1[g] == k for g in a) and all(seen1[g] == seen[g] for g in fresh[n_max:])
            b, nb, seen2 = select_ref.select(rank, seen1, k, G, True)
            assert b == fresh[n_max:] and nb == n_fresh - n_max
            c, nc, _ = select_ref.select(rank, seen2, k, G, True)
            assert c == [] and nc == 0
    # the relay's use: min_rank = 1, listed whenever the rank grew
    rank = np.array([0, 3, 3, 5], np.uint32)
    seen = np.array([0, 3, 1, 0], np.uint32)
    assert select_ref.select(rank, seen, 1, 4, False)[0] == [2, 3]
    # 70,001 generations cross the block-count scan with a ragged final block
    assert 70001 % 2048 not in (0, 2047) and 70001 // 2048 >= 2


def test_lists_and_the_batch_they_stand_for():
    for k, r, cap, L, G_src, n_max, seed in SHAPES[:2]:
        st, want = select_ref.listed_store(k, r, cap, L, G_src, seed)
        # generation 0 complete with a ragged last row, generation 1 short of k, full-length rows somewhere
        for g in (0, 1, 2):
            co = st.coeffs[g, : st.n[g]]
            idx = st.index[g, : st.n[g]]
            fl, rk = rank_ref.innovative(store_ref.vectors_of(k, idx, co))
            assert rk == st.n[g] == want[g] and fl.all(), g
        assert st.n[0] == k and st.n[1] == k - 2 and st.len[0, k - 1] % 16 != 0
        assert (st.len[2, :k] == L).all()
        sel = select_ref.special_list(np.random.default_rng(seed + 1), G_src, n_max)
        assert len(sel) == n_max and sel.count(0) >= 2 and 1 in sel and any(g >= G_src for g in sel)
        assert any(a > b for a, b in zip(sel, sel[1:])), "no descending pair"
        for n_sel in (n_max - 1, n_max + 5, None, 0):
            n = select_ref.used(sel, n_sel, n_max)
            assert n == {n_max - 1: n_max - 1, n_max + 5: n_max, None: n_max, 0: 0}[n_sel]
            cut = sel[:n] + [select_ref.UNUSED] * (n_max - n)
            b, invalid = select_ref.gathered(st, cut, n_sel, n_max)
            assert invalid == [j for j in range(n) if sel[j] >= G_src]
            for j in range(n_max):
                if j < n and sel[j] < G_src:
                    g = sel[j]
                    assert b.n[j] == st.n[g] and np.array_equal(b.bytes[j], st.bytes[g])
                    assert np.array_equal(b.coeffs[j], st.coeffs[g]) and np.array_equal(b.off[j], st.off[g])
                else:
                    assert b.n[j] == 0 and (b.bytes[j] == select_ref.FILL).all()
    # the third shape is small enough to state directly: four entries over three generations
    k, r, cap, L, G_src, n_max, seed = SHAPES[2]
    assert n_max > G_src and (L + 15) // 16 == 65
    assert (SHAPES[0][3] + 15) // 16 == 3
