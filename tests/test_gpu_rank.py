"""qf_rank_batch and qf_decode_innovative_batch on the MI355X, bit for bit.

The reference is tests/rank_ref.py (numpy elimination in arrival order); the
expected decode is the sources the rows were built from, and oracle.decode over
the compacted (innovative) rows.  Every generation's payloads are consistent
with its vectors (rows = V x sources), and the payload of every slot the
reference calls non-innovative is overwritten with 0xEE: a kernel that accepts
such a slot cannot return the sources."""
import numpy as np
import pytest

from tests import rank_ref
from tests.test_rank_cpu import planted_cases

pytestmark = pytest.mark.gpu

SENT = 0xA5
OK, EINVAL, ERANGE, ENOTREADY, ERANK = 0, -1, -2, -3, -4


def _r16(x):
    return (x + 15) // 16 * 16


class Gens:
    """G generations of received rows: src (G, k, L), idx (G, mr), n (G,),
    coeffs (G, mr, k) or None (Cauchy rows of (k, r)), rows (G, mr, L)."""

    def __init__(self, oracle, k, r, L, src, idx, n, coeffs, fill=True):
        self.k, self.r, self.L = k, r, L
        self.src = src
        self.idx = np.ascontiguousarray(idx, np.uint16)
        self.G, self.mr = self.idx.shape
        self.n = np.full(self.G, self.mr, np.uint32) if n is None else np.asarray(n, np.uint32)
        self.coeffs = coeffs
        C = oracle.cauchy(k, r) if (coeffs is None and r) else None
        lim = 256 if coeffs is not None else r
        self.rows = np.zeros((self.G, self.mr, L), np.uint8)
        self.valid, self.flags, self.rank, self.V = [], [], [], []
        for g in range(self.G):
            n_g = min(int(self.n[g]), self.mr)
            ix = self.idx[g, :n_g].astype(np.int64)
            ok = bool(((ix < k) | (ix - k < lim)).all())
            self.valid.append(ok)
            f = np.zeros(self.mr, np.uint8)
            rank = 0
            V = None
            if ok:
                V = rank_ref.vectors(k, r, ix, None if coeffs is None else coeffs[g], C)
                if n_g:
                    fl, rank = rank_ref.innovative(V)
                    f[:n_g] = fl
                    self.rows[g, :n_g] = oracle.encode(src[g], n_g, np.ascontiguousarray(V))
            if fill:
                self.rows[g][f == 0] = 0xEE
            self.V.append(V)
            self.flags.append(f)
            self.rank.append(rank)

    def expected(self, g):
        """(status, erased sources ascending) of the innovative decode."""
        k = self.k
        if not self.valid[g]:
            return EINVAL, []
        if self.rank[g] < k:
            return ENOTREADY, []
        have = {int(self.idx[g, s]) for s in np.flatnonzero(self.flags[g]) if self.idx[g, s] < k}
        erased = [i for i in range(k) if i not in have]
        if len(erased) > min(k, self.r, 128):
            return EINVAL, []
        return OK, erased


def _dev(a, dt=None):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).cuda()


def run_rank(qf, gs, pass_n=True, want_flags=True):
    """-> flags (G, mr) or None, rank (G,), status (G,); sentinels checked."""
    import torch

    G, mr = gs.G, gs.mr
    t_idx = _dev(gs.idx.view(np.int16))
    t_n = _dev(gs.n.view(np.int32)) if pass_n else None
    t_co = _dev(gs.coeffs) if gs.coeffs is not None else None
    t_fl = torch.full((G * mr + 64,), SENT, dtype=torch.uint8, device="cuda") if want_flags else None
    t_rk = torch.full((G + 4,), 777, dtype=torch.int32, device="cuda")
    t_st = torch.full((G + 4,), 77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    qf.rank_batch(t_idx, t_rk, t_st, gs.k, r=gs.r, max_rows=mr, G=G, n_rows=t_n, row_coeffs=t_co, innovative=t_fl)
    qf.default_context().sync()
    rk, st = t_rk.cpu().numpy(), t_st.cpu().numpy()
    assert (rk[G:] == 777).all() and (st[G:] == 77).all()
    fl = None
    if want_flags:
        fl = t_fl.cpu().numpy()
        assert (fl[G * mr:] == SENT).all()
        fl = fl[: G * mr].reshape(G, mr)
    return fl, rk[:G], st[:G]


def run_decode(qf, gs, innovative=True, pass_n=True, want_rank=True, want_flags=True, gap=0):
    """-> dict(rec (G, em, L), ri (G, em), nrec, st, rank, flags).  Bytes the
    call must not write are sentinel-checked here."""
    import torch

    k, r, L, G, mr = gs.k, gs.r, gs.L, gs.G, gs.mr
    em = min(k, r)
    rs = _r16(L) + 16
    rows = np.full((G, mr, rs), 0x3C, np.uint8)     # bytes past L of a row must not reach the output
    rows[:, :, :L] = gs.rows
    rec_rs = _r16(L) + 16
    rec_gs = em * rec_rs + gap
    t_rows = _dev(rows)
    t_idx = _dev(gs.idx.view(np.int16))
    t_n = _dev(gs.n.view(np.int32)) if pass_n else None
    t_co = _dev(gs.coeffs) if gs.coeffs is not None else None
    t_rec = torch.full((G * rec_gs + 64,), SENT, dtype=torch.uint8, device="cuda")
    t_ri = torch.full((G * em + 8,), 0x5A5A, dtype=torch.int16, device="cuda")
    t_nrec = torch.full((G + 4,), 555, dtype=torch.int32, device="cuda")
    t_st = torch.full((G + 4,), 77, dtype=torch.int32, device="cuda")
    t_rk = torch.full((G + 4,), 777, dtype=torch.int32, device="cuda") if (innovative and want_rank) else None
    t_fl = torch.full((G * mr + 64,), SENT, dtype=torch.uint8, device="cuda") if (innovative and want_flags) else None
    kw = dict(max_rows=mr, row_stride=rs, rows_gen_stride=mr * rs, rec_row_stride=rec_rs, rec_gen_stride=rec_gs,
              G=G, n_rows=t_n, row_coeffs=t_co)
    torch.cuda.synchronize()
    if innovative:
        qf.decode_innovative_batch(t_rows, t_idx, t_rec, t_ri, t_nrec, t_st, k, r, L, rank=t_rk, innovative=t_fl,
                                   **kw)
    else:
        qf.decode_batch(t_rows, t_idx, t_rec, t_ri, t_nrec, t_st, k, r, L, **kw)
    qf.default_context().sync()
    rec, ri = t_rec.cpu().numpy(), t_ri.cpu().numpy().view(np.uint16)
    nrec, st = t_nrec.cpu().numpy(), t_st.cpu().numpy()
    assert (rec[G * rec_gs:] == SENT).all() and (ri[G * em:] == 0x5A5A).all()
    assert (nrec[G:] == 555).all() and (st[G:] == 77).all()
    rg = rec[: G * rec_gs].reshape(G, rec_gs)
    assert (rg[:, em * rec_rs:] == SENT).all(), "bytes after a generation's last recovered row were written"
    rrow = rg[:, : em * rec_rs].reshape(G, em, rec_rs)
    assert (rrow[:, :, L:] == SENT).all(), "bytes between L and rec_row_stride were written"
    out = dict(rec=rrow[:, :, :L].copy(), ri=ri[: G * em].reshape(G, em).copy(), nrec=nrec[:G].copy(),
               st=st[:G].copy(), rank=None, flags=None)
    if t_rk is not None:
        rk = t_rk.cpu().numpy()
        assert (rk[G:] == 777).all()
        out["rank"] = rk[:G].copy()
    if t_fl is not None:
        fl = t_fl.cpu().numpy()
        assert (fl[G * mr:] == SENT).all()
        out["flags"] = fl[: G * mr].reshape(G, mr).copy()
    return out


def check_rank(gs, got):
    fl, rk, st = got
    for g in range(gs.G):
        assert st[g] == (OK if gs.valid[g] else EINVAL), (g, st[g])
        assert rk[g] == gs.rank[g], (g, rk[g], gs.rank[g])
        if fl is not None:
            assert np.array_equal(fl[g], gs.flags[g]), (g, fl[g].tolist(), gs.flags[g].tolist())


def check_decode(oracle, gs, out):
    for g in range(gs.G):
        est, erased = gs.expected(g)
        assert out["st"][g] == est, (g, out["st"][g], est)
        assert out["st"][g] != ERANK
        assert out["nrec"][g] == len(erased), (g, out["nrec"][g], len(erased))
        if out["rank"] is not None:
            assert out["rank"][g] == gs.rank[g], g
        if out["flags"] is not None:
            assert np.array_equal(out["flags"][g], gs.flags[g]), g
        if est != OK:
            continue
        assert out["ri"][g, : len(erased)].tolist() == erased, g
        assert np.array_equal(out["rec"][g, : len(erased)], gs.src[g][erased]), f"recovered rows of generation {g}"
        # the same through the oracle over the compacted rows
        keep = np.flatnonzero(gs.flags[g])
        co = None if gs.coeffs is None else gs.coeffs[g][keep]
        ost, oout, _ = oracle.decode(gs.k, gs.idx[g][keep], gs.rows[g][keep], co)
        assert ost == OK and np.array_equal(oout, gs.src[g]), g


def random_gens(oracle, rng, k, mr, L, G, r=None, n=None, p_sys=0.5, p_dep=0.25, fill=True):
    """Systematic rows (random indices, so repeats occur) and coded rows with
    explicit vectors: random ones, sparse ones, combinations of two earlier
    rows, zero vectors."""
    e, lg = oracle.tables()
    e, lg = e.astype(np.int64), lg.astype(np.int64)

    def scale(v, c):
        out = e[lg[v] + int(lg[c])].astype(np.uint8)
        out[v == 0] = 0
        return out if c else np.zeros_like(v)

    src = rng.integers(0, 256, (G, k, L), dtype=np.uint8)
    idx = np.zeros((G, mr), np.uint16)
    co = np.zeros((G, mr, k), np.uint8)
    for g in range(G):
        fresh = list(rng.permutation(k))
        for s in range(mr):
            if rng.random() < p_sys:
                # mostly a source not seen yet, now and then any source (a repeat, as a rule)
                idx[g, s] = fresh.pop() if (fresh and rng.random() > p_dep / 2) else rng.integers(0, k)
                co[g, s, idx[g, s]] = 1
                continue
            idx[g, s] = k + rng.integers(0, 256)
            u = rng.random()
            if u < p_dep and s >= 2:
                a, b = rng.integers(0, s, 2)
                co[g, s] = scale(co[g, a], int(rng.integers(1, 256))) ^ scale(co[g, b], int(rng.integers(0, 256)))
            elif u < p_dep + min(0.03, p_dep / 4):
                pass                                  # a zero vector
            elif u < p_dep + 0.2:
                first = int(rng.integers(0, k))       # first nonzero late, zeros among the rest
                co[g, s, first:] = rng.integers(0, 256, k - first) * (rng.random(k - first) < 0.6)
            else:
                co[g, s] = rng.integers(0, 256, k)
    # (the unit vectors written for systematic slots only fed the combinations)
    return Gens(oracle, k, k if r is None else r, L, src, idx, n, co, fill=fill)


# ---------------------------------------------------------------------------
# Planted dependencies
# ---------------------------------------------------------------------------
def _planted(oracle):
    """One generation per planted arrival order, k = 16, max_rows = 24."""
    k, mr, L = 16, 24, 100
    rng = np.random.default_rng(77)
    cases = planted_cases(rng, k)
    names = list(cases)
    G = len(names)
    src = rng.integers(0, 256, (G, k, L), dtype=np.uint8)
    idx = np.zeros((G, mr), np.uint16)
    co = np.zeros((G, mr, k), np.uint8)
    for g, name in enumerate(names):
        V = cases[name]
        for s in range(mr):
            nz = np.flatnonzero(V[s])
            if nz.size == 1 and V[s, nz[0]] == 1:
                idx[g, s] = nz[0]                     # a unit vector arrives as a systematic row
            else:
                idx[g, s] = k + 3 * s
                co[g, s] = V[s]
    return names, Gens(oracle, k, k, L, src, idx, None, co)


def test_planted_dependencies(qf, oracle):
    names, gs = _planted(oracle)
    by = dict(zip(names, range(gs.G)))
    g = by["e2 + e7, then systematic 2, then systematic 7"]
    assert gs.idx[g, :3].tolist() == [16, 2, 7] and gs.flags[g][:3].tolist() == [1, 1, 0]
    g = by["coded row with its first nonzero at column 5, then systematic 5"]
    assert gs.idx[g, 1] == 5 and gs.flags[g][:2].tolist() == [1, 1]
    g = by["rank k at slot 19, four rows behind it"]
    assert gs.flags[g][19] == 1 and not gs.flags[g][20:].any()
    g = by["combination of slots 1 and 3"]
    assert gs.flags[g][9] == 0
    g = by["zero vector"]
    assert gs.flags[g][4] == 0
    g = by["duplicated systematic index"]
    assert gs.flags[g][2] == 1 and gs.flags[g][11] == 0
    assert all(r == 16 for r in gs.rank)
    check_rank(gs, run_rank(qf, gs))
    check_decode(oracle, gs, run_decode(qf, gs))


def test_duplicated_cauchy_index_without_vectors(qf, oracle):
    """NULL row_coeffs, r = 8: 12 sources, then repairs 3, 5, 3 (a repeat), 0, 7, 1."""
    k, r, mr, L, G = 16, 8, 24, 100, 2
    rng = np.random.default_rng(8)
    src = rng.integers(0, 256, (G, k, L), dtype=np.uint8)
    idx = np.zeros((G, mr), np.uint16)
    for g in range(G):
        keep = rng.permutation(k)[:12]
        idx[g] = list(keep) + [k + 3, k + 5, k + 3, k + 0, k + 7, k + 1] + [k + 2, k + 4, k + 6, int(keep[0]),
                                                                            k + 5, int(keep[1])]
    gs = Gens(oracle, k, r, L, src, idx, None, None)
    for g in range(G):
        assert gs.flags[g].tolist() == [1] * 14 + [0, 1, 1] + [0] * 7 and gs.rank[g] == 16
    check_rank(gs, run_rank(qf, gs))
    check_decode(oracle, gs, run_decode(qf, gs))


# ---------------------------------------------------------------------------
# Shapes
# ---------------------------------------------------------------------------
def test_k_equal_one(qf, oracle):
    k, mr, L, G = 1, 3, 20, 3
    rng = np.random.default_rng(1)
    src = rng.integers(0, 256, (G, k, L), dtype=np.uint8)
    idx = np.array([[1, 5, 0], [0, 0, 9], [7, 7, 7]], np.uint16)
    co = np.array([[[0], [0x1D], [0]], [[0], [0], [3]], [[0], [0], [0]]], np.uint8)
    gs = Gens(oracle, k, 1, L, src, idx, None, co)
    assert [f.tolist() for f in gs.flags] == [[0, 1, 0], [1, 0, 0], [0, 0, 0]] and gs.rank == [1, 1, 0]
    check_rank(gs, run_rank(qf, gs))
    check_decode(oracle, gs, run_decode(qf, gs))


# k, max_rows, L, G, p_sys, p_dep
SHAPES = [
    (64, 80, 48, 4, 0.5, 0.1),       # one column per lane
    (65, 80, 48, 4, 0.5, 0.1),       # the second column of lane 0
    (100, 110, 37, 4, 0.6, 0.04),
    (16, 24, 1, 6, 0.4, 0.25),       # L = 1
    (16, 24, 1201, 4, 0.4, 0.25),    # a partial last unit after 75 whole ones
]


@pytest.mark.parametrize("k,mr,L,G,p_sys,p_dep", SHAPES)
def test_shapes(qf, oracle, k, mr, L, G, p_sys, p_dep):
    rng = np.random.default_rng(k * 100 + L)
    gs = random_gens(oracle, rng, k, mr, L, G, p_sys=p_sys, p_dep=p_dep)
    assert any(0 < f[: k].sum() < k for f in gs.flags), "no dependent row among the first k"
    assert any(r == k for r in gs.rank)
    check_rank(gs, run_rank(qf, gs))
    check_decode(oracle, gs, run_decode(qf, gs))


def test_k128_all_coded_130_rows(qf, oracle, gpu_ctx):
    """More than two ballot rounds of slots, e = 128 erased sources, 8 payload passes."""
    k, mr, L, G = 128, 130, 48, 2
    rng = np.random.default_rng(128)
    gs = random_gens(oracle, rng, k, mr, L, G, r=128, p_sys=0.0, p_dep=0.01)
    assert gs.rank == [k, k] and all(f.sum() == k and not f.all() for f in gs.flags)
    check_rank(gs, run_rank(qf, gs))
    gpu_ctx.sync()
    gpu_ctx.profile(True)
    out = run_decode(qf, gs)
    times = gpu_ctx.kernel_times()
    gpu_ctx.profile(False)
    assert times["k_rank_filter"][0] == 1 and times["k_decode_prepare"][0] == 1, times
    assert sum(v[0] for n, v in times.items() if n not in ("k_rank_filter", "k_decode_prepare")) == 8, times
    assert (out["nrec"] == 128).all()
    check_decode(oracle, gs, out)


def test_k255_rank_only(qf, oracle):
    k, mr, G = 255, 270, 2
    rng = np.random.default_rng(255)
    gs = random_gens(oracle, rng, k, mr, 16, G, r=1, p_sys=0.7, p_dep=0.2)
    assert all(r > 200 for r in gs.rank)
    check_rank(gs, run_rank(qf, gs))
    check_rank(gs, run_rank(qf, gs, want_flags=False))


def test_long_rows_bit_sliced_payload_pass(qf, oracle, gpu_ctx):
    k, mr, L, G = 16, 24, 2080, 3
    gs = random_gens(oracle, np.random.default_rng(2080), k, mr, L, G, p_sys=0.4)
    assert any(r == k for r in gs.rank)
    gpu_ctx.sync()
    gpu_ctx.profile(True)
    out = run_decode(qf, gs)
    times = gpu_ctx.kernel_times()
    gpu_ctx.profile(False)
    payload = [n for n in times if n not in ("k_rank_filter", "k_decode_prepare")]
    assert len(payload) == 1 and payload[0].startswith("qf_combine_bs"), times
    check_decode(oracle, gs, out)


def test_row_counts_null_n_rows_and_an_invalid_generation(qf, oracle):
    k, r, mr, L, G = 16, 16, 24, 53, 7
    rng = np.random.default_rng(5)
    n = [mr, 0, 1, k - 1, mr, mr, 9]
    gs = random_gens(oracle, rng, k, mr, L, G, r=r, n=n, p_sys=0.5)
    assert gs.valid == [True] * G
    got = run_rank(qf, gs)
    check_rank(gs, got)
    assert got[1][1] == 0 and got[1][2] <= 1 and got[1][3] <= k - 1
    out = run_decode(qf, gs)
    check_decode(oracle, gs, out)
    assert list(out["st"][1:4]) == [ENOTREADY] * 3
    # NULL n_rows: max_rows rows each
    full = random_gens(oracle, np.random.default_rng(6), k, mr, L, 3, r=r)
    check_rank(full, run_rank(qf, full, pass_n=False))
    check_decode(oracle, full, run_decode(qf, full, pass_n=False, want_rank=False, want_flags=False))
    # Cauchy-implicit rows, generation 1 with an index past k + r between valid ones
    r = 8
    src = rng.integers(0, 256, (3, k, L), dtype=np.uint8)
    idx = np.zeros((3, mr), np.uint16)
    for g in range(3):
        idx[g] = list(rng.permutation(k)[:10]) + [k + j for j in rng.permutation(r)] + [k + 1, 3, k + 2, 5, 7, 9]
    idx[1, 20] = k + r
    bad = Gens(oracle, k, r, L, src, idx, None, None)
    assert bad.valid == [True, False, True] and bad.rank[0] == k and bad.rank[2] == k
    got = run_rank(qf, bad)
    check_rank(bad, got)
    assert not got[0][1].any() and got[1][1] == 0
    out = run_decode(qf, bad)
    check_decode(oracle, bad, out)
    assert out["st"].tolist() == [OK, EINVAL, OK] and out["rank"][1] == 0 and not out["flags"][1].any()


def test_rank_short_of_k(qf, oracle):
    """QF_ENOTREADY with n_rec = 0; the rank and the flags are still reported."""
    k, mr, L, G = 16, 20, 40, 3
    rng = np.random.default_rng(3)
    src = rng.integers(0, 256, (G, k, L), dtype=np.uint8)
    idx = np.zeros((G, mr), np.uint16)
    co = np.zeros((G, mr, k), np.uint8)
    for g in range(G):
        # every vector inside the span of the first 11 + g sources
        for s in range(mr):
            if s % 3 == 0:
                idx[g, s] = rng.integers(0, 11 + g)
            else:
                idx[g, s] = k + s
                co[g, s, : 11 + g] = rng.integers(0, 256, 11 + g)
    gs = Gens(oracle, k, k, L, src, idx, None, co)
    assert gs.rank == [11, 12, 13]
    out = run_decode(qf, gs)
    assert (out["st"] == ENOTREADY).all() and (out["nrec"] == 0).all()
    assert out["rank"].tolist() == [11, 12, 13]
    check_decode(oracle, gs, out)


# ---------------------------------------------------------------------------
# Equivalence with qf_decode_batch where the first k candidates are independent
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("k,r", [(16, 8), (64, 16)])
@pytest.mark.parametrize("kind", ["explicit", "cauchy", "mixed"])
def test_equals_decode_batch_on_independent_rows(qf, oracle, kind, k, r):
    L, G = 100, 5
    mr = k + r
    rng = np.random.default_rng(k + len(kind))
    src = rng.integers(0, 256, (G, k, L), dtype=np.uint8)
    idx = np.zeros((G, mr), np.uint16)
    co = None if kind == "cauchy" else np.zeros((G, mr, k), np.uint8)
    for g in range(G):
        lost = int(rng.integers(1, r + 1))
        keep = list(rng.permutation(k)[: k - lost])
        if kind == "cauchy":
            coded = [k + int(j) for j in rng.permutation(r)]
        else:
            coded = [k + int(j) for j in rng.integers(0, 256, r)]
        if kind == "mixed":
            keep = keep + [keep[0]]                   # a repeated source: no candidate of either decode
        arr = keep + coded
        rng.shuffle(arr)
        arr = (arr + [int(keep[0])] * mr)[:mr]
        idx[g] = arr
        if co is not None:
            co[g] = rng.integers(0, 256, (mr, k))
    gs = Gens(oracle, k, r, L, src, idx, None, co, fill=False)
    for g in range(G):
        # the first k candidates (a source counts once) are exactly the innovative slots
        seen, cand = set(), []
        for s in range(mr):
            i = int(idx[g, s])
            if i < k and i in seen:
                continue
            seen.add(i) if i < k else None
            cand.append(s)
        assert gs.rank[g] == k and np.flatnonzero(gs.flags[g]).tolist() == cand[:k], g
    a = run_decode(qf, gs, innovative=False)
    b = run_decode(qf, gs, innovative=True)
    assert (a["st"] == OK).all()
    for key in ("rec", "ri", "nrec", "st"):
        assert np.array_equal(a[key], b[key]), key
    check_decode(oracle, gs, b)


# ---------------------------------------------------------------------------
# Two relays
# ---------------------------------------------------------------------------
def _two_relays(oracle, G):
    """k = 16, r = 8: relay A holds sources 0-7 and repairs 0-3, relay B
    sources 8-15 and repairs 4-7; the receiver gets 14 packets recoded by A,
    then 8 recoded by B.  -> (src, vectors (G, 22, k), rows (G, 22, L), relay
    A's vectors and rows, seeds)."""
    k, r, L = 16, 8, 100
    C = oracle.cauchy(k, r)
    src_all, vec_all, rows_all, held, seeds = [], [], [], [], []
    seed = 1
    while len(src_all) < G:
        assert seed <= 40
        rng = np.random.default_rng(seed)
        seed += 1
        src = rng.integers(0, 256, (k, L), dtype=np.uint8)
        VA = np.concatenate([np.eye(k, dtype=np.uint8)[:8], C[:4]])
        VB = np.concatenate([np.eye(k, dtype=np.uint8)[8:], C[4:]])
        MA = rng.integers(0, 256, (14, 12), dtype=np.uint8)
        MB = rng.integers(0, 256, (8, 12), dtype=np.uint8)
        V = np.concatenate([oracle.encode(VA, 14, MA), oracle.encode(VB, 8, MB)])
        if rank_ref.innovative(V)[1] != k:
            continue                                  # (did not happen for seeds 1-40)
        src_all.append(src)
        vec_all.append(V)
        rows_all.append(oracle.encode(src, 22, np.ascontiguousarray(V)))
        held.append((VA, oracle.encode(src, 12, np.ascontiguousarray(VA))))
        seeds.append(seed - 1)
    return np.stack(src_all), np.stack(vec_all), np.stack(rows_all), held, seeds


def test_two_relays(qf, oracle):
    k, L, G = 16, 100, 4
    src, V, rows, _, seeds = _two_relays(oracle, G)
    assert seeds == [1, 2, 3, 4]
    idx = np.broadcast_to(k + np.arange(22, dtype=np.uint16), (G, 22)).copy()
    for g in range(G):
        assert rank_ref.innovative(V[g])[1] == 16
        assert rank_ref.innovative(V[g][:16])[1] <= 14
    # the contrast: the first 16 rows are singular for today's decode
    first = Gens(oracle, k, 16, L, src, idx[:, :16], None, V[:, :16].copy(), fill=False)
    a = run_decode(qf, first, innovative=False)
    assert (a["st"] == ERANK).all(), a["st"]
    gs = Gens(oracle, k, 22, L, src, idx, None, V.copy())
    assert all(r == 16 for r in gs.rank)
    out = run_decode(qf, gs)
    assert (out["st"] == OK).all() and (out["nrec"] == 16).all()
    check_decode(oracle, gs, out)
    assert np.array_equal(out["rec"], src)


def test_objects_over_the_two_relay_packets(qf, oracle):
    k, L = 16, 100
    src, V, rows, held, _ = _two_relays(oracle, 1)
    src, V, rows = src[0], V[0], rows[0]
    flags, rank = rank_ref.innovative(V)
    assert rank == 16
    at = int(np.flatnonzero(np.cumsum(flags) == 16)[0])
    assert at >= 16
    pkts = [qf.Packet(100 + s, bytearray(rows[s].tobytes()), L, False, V[s].tobytes(), k) for s in range(22)]
    dec = qf.Decoder(k, max_len=L, innovative_only=True)
    plain = qf.Decoder(k, max_len=L)
    for s, p in enumerate(pkts):
        done = dec.add_packet(p)
        assert done == (s >= at), s
        assert dec.rank == int(np.cumsum(flags)[s])
        assert plain.add_packet(p) is False
    assert dec.is_decoded and not plain.is_decoded
    assert plain.rank <= 14
    got = dec.get_decoded_packets()
    assert len(got) == k
    for i, p in enumerate(got):
        assert bytes(p.data[:L]) == src[i].tobytes() and p.id == i, i
    # the mode cannot change once a packet is in
    from quicfuscate_amd import _lib as L_

    assert L_._lib().qf_decoder_set_innovative(plain.handle, 1) == L_.QF_EINVAL
    # a systematic packet that coded packets already span is dropped and reconstructed
    d2 = qf.Decoder(k, max_len=L, innovative_only=True)
    e27 = np.zeros(k, np.uint8)
    e27[2] = e27[7] = 1
    assert d2.add_packet(qf.Packet(50, bytearray((src[2] ^ src[7]).tobytes()), L, False, e27.tobytes(), k)) is False
    assert d2.add_packet(qf.Packet(2, bytearray(src[2].tobytes()), L, True)) is False and d2.rank == 2
    assert d2.add_packet(qf.Packet(7, bytearray(b"\xEE" * L), L, True)) is False and d2.rank == 2
    done = False
    for i in [j for j in range(k) if j not in (2, 7)]:
        done = d2.add_packet(qf.Packet(i, bytearray(src[i].tobytes()), L, True))
    assert done and d2.rank == k
    got = d2.get_decoded_packets()
    assert [p.id for p in got] == list(range(k))
    assert all(bytes(p.data[:L]) == src[i].tobytes() for i, p in enumerate(got))
    # relay A: its 12 rows plus 3 of its own recoded packets have rank 12
    VA, rowsA = held[0]
    rec = qf.Recoder(k, L, 15)
    assert rec.rank() == 0
    for s in range(12):
        if s < 8:
            rec.add_packet(qf.Packet(s, bytearray(rowsA[s].tobytes()), L, True))
        else:
            rec.add_packet(qf.Packet(200 + s, bytearray(rowsA[s].tobytes()), L, False, VA[s].tobytes(), k))
    assert rec.rank() == 12
    for p in rec.recode(3, seed=9):
        rec.add_packet(p)
    assert rec.count == 15 and rec.rank() == 12


# ---------------------------------------------------------------------------
# Call-level errors
# ---------------------------------------------------------------------------
def test_call_level_errors(qf, gpu_ctx):
    import torch

    from quicfuscate_amd import _lib as L_

    t = lambda n, dt=torch.uint8: torch.zeros(n, dtype=dt, device="cuda")   # noqa: E731
    idx, rk, st, fl = t(4096, torch.int16), t(1, torch.int32), t(1, torch.int32), t(4096)
    lib, ctx = L_._lib(), gpu_ctx.handle
    import ctypes

    def rank_status(k=8, r=0, max_rows=8, flags=0, coeffs=None):
        sh = L_.RankShape(k, r, max_rows, flags)
        return lib.qf_rank_batch(ctx, ctypes.byref(sh), 1, idx.data_ptr(), None, coeffs, fl.data_ptr(),
                                 rk.data_ptr(), st.data_ptr())

    assert rank_status() == 0
    assert rank_status(k=0) == L_.QF_EINVAL and rank_status(k=257) == L_.QF_EINVAL
    assert rank_status(max_rows=0) == L_.QF_EINVAL and rank_status(max_rows=4097) == L_.QF_EINVAL
    assert rank_status(flags=1) == L_.QF_EINVAL
    assert rank_status(k=200, r=57) == L_.QF_ERANGE
    assert rank_status(k=200, r=56) == 0
    assert rank_status(k=256, max_rows=4096) == 0
    co = t(8 * 200)
    assert rank_status(k=200, r=57, coeffs=co.data_ptr()) == 0      # vectors given: no Cauchy row is formed

    rows, rec, ri, nrec = t(64 * 48 + 16), t(64 * 48), t(64, torch.int16), t(1, torch.int32)

    def dec_status(k=8, r=4, Lb=32, max_rows=8, rs=48, rows_ptr=None, coeffs=None):
        sh = L_.DecodeShape(k, r, Lb, max_rows, rs, max_rows * rs, 48, min(k, r) * 48)
        return lib.qf_decode_innovative_batch(ctx, ctypes.byref(sh), 1, rows_ptr or rows.data_ptr(), idx.data_ptr(),
                                              None, coeffs, rec.data_ptr(), ri.data_ptr(), nrec.data_ptr(),
                                              st.data_ptr(), rk.data_ptr(), fl.data_ptr())

    assert dec_status() == 0
    assert dec_status(k=0) == L_.QF_EINVAL and dec_status(k=257) == L_.QF_EINVAL
    assert dec_status(max_rows=0) == L_.QF_EINVAL
    assert dec_status(Lb=0) == L_.QF_EINVAL
    assert dec_status(rows_ptr=rows.data_ptr() + 8) == L_.QF_EINVAL      # misaligned rows
    assert dec_status(rs=40) == L_.QF_EINVAL                             # misaligned stride
    assert dec_status(k=200, r=57, max_rows=1) == L_.QF_ERANGE
    gpu_ctx.sync()
