"""The streaming steps over a list on the MI355X: qf_gen_select_dev against
tests/select_ref.py, qf_decode_frames_sel_dev / qf_recode_frames_sel_dev byte
for byte against the dense calls over the gathered batch made on the host,
qf_stream_reset_dev, and polls that stay on the device end to end (parse ->
update -> append -> select with MARK -> listed decode -> reset of the list).

Every output buffer starts as 0xCC with guard bytes behind it, and the bytes a
call must not write are checked to still be 0xCC.  Unused list entries hold
0xFFFFFFFF.  tests/test_stream_select_cpu.py asserts that the inputs hold the
cases these tests are about."""
import ctypes

import numpy as np
import pytest

from tests import recv_ref, select_ref, store_ref
from tests import test_gpu_rank as K
from tests import test_gpu_recv_inplace as I
from tests import test_gpu_relay_inplace as R
from tests import test_gpu_stream_recv as S
from tests import test_gpu_wire_coded as W
from tests import test_stream_select_cpu as C

pytestmark = pytest.mark.gpu

FILL, FILL16, FILL32, NONE16 = 0xCC, 0xCCCC, 0xCCCCCCCC, 0xFFFF
OK, EINVAL, ENOTREADY = 0, -1, -3
UNUSED = select_ref.UNUSED

_r16, _dev, _filled, _host = W._r16, W._dev, W._filled, W._host


# ---------------------------------------------------------------------------
# select
# ---------------------------------------------------------------------------
def run_select(qf, G, t_rank, t_seen, min_rank, n_max, mark, with_match=True):
    t_sel, t_n, t_m = _filled(4 * n_max + 16), _filled(16), _filled(16)
    qf.gen_select(t_rank, t_sel, t_n, G=G, min_rank=min_rank, n_max=n_max, seen=t_seen, mark=mark,
                  n_match=t_m if with_match else None)
    qf.default_context().sync()
    sel, n, m = _host(t_sel, np.uint32), _host(t_n, np.uint32), _host(t_m, np.uint32)
    assert (n[1:] == FILL32).all() and (m[1 if with_match else 0:] == FILL32).all()
    assert n[0] <= n_max and (sel[n[0]:] == FILL32).all(), "entries behind n_sel were written"
    return sel[: n[0]].tolist(), int(m[0]) if with_match else None


@pytest.mark.parametrize("G", C.SELECT_G)
def test_select_against_the_reference(qf, gpu_ctx, G):
    k, rank, seen = C.select_inputs(G)
    t_rank = _dev(rank)
    n_all = select_ref.select(rank, None, k, G, False)[1]
    n_fresh = select_ref.select(rank, seen, k, G, False)[1]
    for use_seen, matches in ((False, n_all), (True, n_fresh)):
        for n_max in sorted({max(1, matches // 2), max(1, matches), matches + 3}):
            for mark in ((False, True) if use_seen else (False,)):
                t_seen = _dev(np.concatenate([seen, np.full(4, FILL32, np.uint32)])) if use_seen else None
                want, want_m, after = select_ref.select(rank, seen if use_seen else None, k, n_max, mark)
                got, got_m = run_select(qf, G, t_rank, t_seen, k, n_max, mark)
                assert got == want and got_m == want_m == matches, (use_seen, n_max, mark)
                if use_seen:
                    h = _host(t_seen, np.uint32)
                    assert (h[G:] == FILL32).all() and np.array_equal(h[:G], after), (n_max, mark)
                if mark:
                    # the overflow was left unmarked: the next call picks it up, the one after finds nothing
                    want2, m2, after2 = select_ref.select(rank, after, k, G, True)
                    got2, gm2 = run_select(qf, G, t_rank, t_seen, k, G, True, with_match=False)
                    assert got2 == want2 and len(want2) == m2 == matches - len(want)
                    assert np.array_equal(_host(t_seen, np.uint32)[:G], after2)
                    assert run_select(qf, G, t_rank, t_seen, k, G, True) == ([], 0)
    assert np.array_equal(_host(t_rank, np.uint32), rank)
    # the relay's rule: every generation whose rank grew
    want, want_m, _ = select_ref.select(rank, seen, 1, G, False)
    assert run_select(qf, G, t_rank, _dev(seen), 1, G, False) == (want, want_m)


def test_select_of_no_generation(qf, gpu_ctx):
    t_sel, t_n, t_m = _filled(16), _filled(16), _filled(16)
    qf.gen_select(None, t_sel, t_n, G=0, min_rank=1, n_max=2, n_match=t_m)
    gpu_ctx.sync()
    assert _host(t_n, np.uint32).tolist() == [0, FILL32, FILL32, FILL32]
    assert _host(t_m, np.uint32).tolist() == [0, FILL32, FILL32, FILL32] and (_host(t_sel) == FILL).all()


# ---------------------------------------------------------------------------
# listed decode and recode
# ---------------------------------------------------------------------------
class Up:
    """A store_ref.Store on the device, 64 bytes of 0xCC behind each array."""

    def __init__(self, st):
        self.st = st
        pad = np.full(64, FILL, np.uint8)
        self.host = {name: np.concatenate([np.ascontiguousarray(a).view(np.uint8).reshape(-1), pad])
                     for name, a in (("bytes", st.bytes), ("off", st.off), ("len", st.len), ("index", st.index),
                                     ("coeffs", st.coeffs))}
        self.t = {name: _dev(a) for name, a in self.host.items()}
        self.n = _dev(st.n.astype(np.uint32))

    def unchanged(self):
        for name, a in self.host.items():
            assert np.array_equal(_host(self.t[name]), a), f"the source array {name} was written"
        assert np.array_equal(_host(self.n, np.uint32), self.st.n)


VARIANTS = ("below", "clamped", "null", "zero")


def list_variant(sel, n_max, variant):
    """-> the list as the device sees it, the host value of *n_sel_dev (None: NULL)."""
    n_sel = {"below": n_max - 1, "clamped": n_max + 5, "null": None, "zero": 0}[variant]
    n = select_ref.used(sel, n_sel, n_max)
    return sel[:n] + [UNUSED] * (n_max - n), n_sel


def dec_outputs(n_max, k, em, cap, rec_gs):
    return I._outputs(n_max, k, em, cap, rec_gs)


def dec_call(qf, listed, src, t, shape, rec_rs, rec_gs, sel=None, n_sel=None, G_src=None):
    k, r, cap, Lb, n_max = shape
    kw = dict(max_rows=cap, src_gen_stride=src.st.gen_stride, rec_row_stride=rec_rs, rec_gen_stride=rec_gs,
              n_rows=src.n, rank=t["rank"], innovative=t["flags"], src_slot=t["slot"])
    a = (src.t["bytes"], src.t["off"], src.t["len"], src.t["index"], src.t["coeffs"], t["rec"], t["ri"], t["nrec"],
         t["st"], k, r, Lb)
    if listed:
        qf.decode_frames_sel(sel, n_sel, *a, n_max=n_max, G_src=G_src, **kw)
    else:
        qf.decode_frames(*a, G=n_max, **kw)
    qf.default_context().sync()
    return {key: _host(v).copy() for key, v in t.items()}


@pytest.mark.parametrize("k,r,cap,Lb,G_src,n_max,seed", C.SHAPES)
def test_listed_decode_equals_the_dense_call_over_the_gathered_batch(qf, gpu_ctx, k, r, cap, Lb, G_src, n_max, seed):
    st, _ = select_ref.listed_store(k, r, cap, Lb, G_src, seed)
    src = Up(st)
    sel0 = select_ref.special_list(np.random.default_rng(seed + 1), G_src, n_max)
    em = min(k, r)
    rec_rs = _r16(Lb) + 16
    rec_gs = em * rec_rs + 32
    shape = (k, r, cap, Lb, n_max)
    sizes = dict(st=4, nrec=4, rank=4, flags=cap, slot=2 * k, ri=2 * em, rec=rec_gs)
    for variant in VARIANTS:
        sel, n_sel = list_variant(sel0, n_max, variant)
        t_sel = _dev(np.array(sel + [UNUSED], np.uint32))
        t_n = None if n_sel is None else _dev(np.array([n_sel], np.uint32))
        got = dec_call(qf, True, src, dec_outputs(n_max, k, em, cap, rec_gs), shape, rec_rs, rec_gs, t_sel, t_n, G_src)
        src.unchanged()
        batch, invalid = select_ref.gathered(st, sel, n_sel, n_max)
        want = dec_call(qf, False, Up(batch), dec_outputs(n_max, k, em, cap, rec_gs), shape, rec_rs, rec_gs)
        n = select_ref.used(sel, n_sel, n_max)
        st_w, nrec_w = want["st"].view(np.int32), want["nrec"].view(np.uint32)
        for j in range(n):                                   # the inputs do what the test is about
            if sel[j] == 0:
                assert st_w[j] == OK and nrec_w[j] > 0, (variant, j)
            if sel[j] == 1 and G_src > 1:
                assert st_w[j] == ENOTREADY, (variant, j)
        assert (st_w[n:n_max] == ENOTREADY).all()
        for j in invalid:
            assert got["st"].view(np.int32)[j] == EINVAL and got["nrec"].view(np.uint32)[j] == 0, (variant, j)
            assert got["rank"].view(np.uint32)[j] == 0, (variant, j)
            assert (got["rec"][j * rec_gs: (j + 1) * rec_gs] == FILL).all(), (variant, j)
            for key, sz in sizes.items():                    # set aside: not compared with the dense call
                got[key][j * sz: (j + 1) * sz] = 0
                want[key][j * sz: (j + 1) * sz] = 0
        if variant in ("clamped", "null"):
            assert len(invalid) == 1
        for key in sizes:
            bad = np.flatnonzero(got[key] != want[key])
            assert bad.size == 0, f"{variant}: {key} differs from the dense call at bytes {bad[:6].tolist()}"
        if variant == "null":
            # no payload byte of a generation that is not listed is read
            other = [g for g in range(G_src) if g not in sel]
            if other:
                view = src.t["bytes"][: G_src * st.gen_stride].view(G_src, st.gen_stride)
                for g in other:
                    view[g] ^= 0x5A
                again = dec_call(qf, True, src, dec_outputs(n_max, k, em, cap, rec_gs), shape, rec_rs, rec_gs, t_sel,
                                 t_n, G_src)
                for j in invalid:
                    for key, sz in sizes.items():
                        again[key][j * sz: (j + 1) * sz] = 0
                for key in sizes:
                    assert np.array_equal(again[key], got[key]), f"{key} depends on a generation that is not listed"
                for g in other:
                    view[g] ^= 0x5A


@pytest.mark.parametrize("use_mix", [True, False], ids=["mix", "seed"])
@pytest.mark.parametrize("shape,m", [(0, 3), (1, 16), (1, 20)], ids=["k4_m3", "k64_m16", "k64_m20"])
def test_listed_recode_equals_the_dense_call_over_the_gathered_batch(qf, gpu_ctx, shape, m, use_mix):
    k, r, cap, Lb, G_src, n_max, seed = C.SHAPES[shape]
    st, _ = select_ref.listed_store(k, r, cap, Lb, G_src, seed)
    src = Up(st)
    rng = np.random.default_rng(seed + 2 + m)
    sel0 = select_ref.special_list(rng, G_src, n_max)
    ors = _r16(Lb) + 16
    ogs = m * ors + 48
    t_mix = _dev(rng.integers(0, 256, (n_max, m, cap), dtype=np.uint8)) if use_mix else None

    def call(listed, s, sel=None, n_sel=None, n_rows=None):
        t = dict(out=_filled(n_max * ogs + 64), oc=_filled(n_max * m * k + 64), ol=_filled(4 * n_max * m + 16),
                 st=_filled(4 * n_max + 16))
        a = (s.t["bytes"], s.t["off"], s.t["len"], s.t["index"], s.t["coeffs"], t["out"], t["oc"], t["st"], k, m, Lb)
        kw = dict(max_rows=cap, src_gen_stride=s.st.gen_stride, out_row_stride=ors, out_gen_stride=ogs, mix=t_mix,
                  seed=0x5EED + m, out_len=t["ol"])
        if listed:
            qf.recode_frames_sel(sel, n_sel, *a, n_max=n_max, G_src=G_src, n_rows=s.n, **kw)
        else:
            qf.recode_frames(*a, G=n_max, n_rows=n_rows, **kw)
        qf.default_context().sync()
        return {key: _host(v).copy() for key, v in t.items()}

    for variant in VARIANTS:
        sel, n_sel = list_variant(sel0, n_max, variant)
        t_sel = _dev(np.array(sel + [UNUSED], np.uint32))
        t_n = None if n_sel is None else _dev(np.array([n_sel], np.uint32))
        got = call(True, src, t_sel, t_n)
        src.unchanged()
        batch, invalid = select_ref.gathered(st, sel, n_sel, n_max)
        n_rows = batch.n.astype(np.uint32).copy()
        n_rows[invalid] = cap + 1                            # the dense call's QF_EINVAL generation: zero outputs
        want = call(False, Up(batch), n_rows=_dev(n_rows))
        n = select_ref.used(sel, n_sel, n_max)
        st_w = want["st"].view(np.int32)
        assert all(st_w[j] == OK for j in range(n) if sel[j] < G_src) and all(st_w[j] == EINVAL for j in invalid)
        assert (st_w[n:n_max] == ENOTREADY).all()
        rows = want["out"][: n_max * ogs].reshape(n_max, ogs)
        assert not rows[n:, : m * ors].reshape(n_max - n, m, ors)[:, :, :Lb].any(), "the dense call writes zero rows there"
        rows[n:] = FILL                                      # ... and the listed call must not write them
        if n:
            assert rows[:n, :Lb].any()
        for key in ("out", "oc", "ol", "st"):
            bad = np.flatnonzero(got[key] != want[key])
            assert bad.size == 0, f"{variant}: {key} differs from the dense call at bytes {bad[:6].tolist()}"


# ---------------------------------------------------------------------------
# reset
# ---------------------------------------------------------------------------
def test_reset_of_a_list(qf, oracle, gpu_ctx):
    k, G = 8, 6
    case = store_ref.stream_case(k)
    idx = [case["idx"][g % case["G"]] for g in range(G)]
    co = [case["co"][g % case["G"]] for g in range(G)]
    flags = [case["flags"][g % case["G"]] for g in range(G)]

    def fresh():
        st = S.States(qf, G, k)
        fl, rk, status = st.update([x[:5] for x in idx], [c[:5] for c in co])
        assert (status == OK).all() and all(st.bytes()[g].any() for g in range(G))
        guard = np.full(4, FILL32, np.uint32)
        return st, _dev(np.concatenate([np.arange(1, G + 1, dtype=np.uint32), guard])), \
            _dev(np.concatenate([np.arange(11, G + 11, dtype=np.uint32), guard]))

    st, t_sn, t_seen = fresh()
    snap = st.bytes()
    t_sel = _dev(np.array([4, 1, 4, G + 3, UNUSED, UNUSED], np.uint32))
    qf.stream_reset(t_sel, _dev(np.array([4], np.uint32)), k, n_max=6, G_src=G, state=st.t, store_n=t_sn, seen=t_seen)
    gpu_ctx.sync()
    now = st.bytes()                                         # (checks the guard behind the states)
    sn, seen = _host(t_sn, np.uint32), _host(t_seen, np.uint32)
    for g in range(G):
        if g in (1, 4):
            assert not now[g].any() and sn[g] == 0 and seen[g] == 0, g
        else:
            assert np.array_equal(now[g], snap[g]) and sn[g] == g + 1 and seen[g] == g + 11, g
    assert (sn[G:] == FILL32).all() and (seen[G:] == FILL32).all()
    # the update takes the reset states as empty, and goes on from the others
    fl, rk, status = st.update([x[:5] for x in idx], [c[:5] for c in co])
    assert (status == OK).all()
    for g in range(G):
        want = int(flags[g][:5].sum())
        if g in (1, 4):
            assert np.array_equal(fl[g], flags[g][:5]) and rk[g] == want, g
        else:
            assert not fl[g].any() and rk[g] == want, g
    # one pointer at a time, n_sel NULL: the other two are untouched
    for which in ("state", "store_n", "seen"):
        st, t_sn, t_seen = fresh()
        snap = st.bytes()
        kw = {which: dict(state=st.t, store_n=t_sn, seen=t_seen)[which]}
        qf.stream_reset(_dev(np.array([2, 0], np.uint32)), None, k, n_max=2, G_src=G, **kw)
        gpu_ctx.sync()
        now, sn, seen = st.bytes(), _host(t_sn, np.uint32), _host(t_seen, np.uint32)
        for g in range(G):
            hit = g in (0, 2)
            assert now[g].any() != (hit and which == "state"), (which, g)
            assert hit and which == "state" or np.array_equal(now[g], snap[g]), (which, g)
            assert sn[g] == (0 if hit and which == "store_n" else g + 1), (which, g)
            assert seen[g] == (0 if hit and which == "seen" else g + 11), (which, g)


# ---------------------------------------------------------------------------
# polls that stay on the device
# ---------------------------------------------------------------------------
def full_gens(oracle, rng, k, Lb, G, r):
    """S.shape_a_gens' traffic with every generation complete."""
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
    return K.Gens(oracle, k, r, Lb, recv_ref.tailed_sources(rng, G, k, Lb), idx, np.full(G, mr, np.uint32), co)


def completing_poll(gs, counts):
    """Per generation the poll whose rows bring its rank to k."""
    out = []
    for g in range(gs.G):
        at = int(np.flatnonzero(np.cumsum(gs.flags[g]) == gs.k)[0])
        out.append(int(np.flatnonzero(np.cumsum(counts[g]) > at)[0]))
    return out


def test_polls_select_decode_reset_on_the_device(qf, oracle, gpu_ctx):
    import torch

    G, k, Lb, r, NM, polls = 48, 8, 100, 8, 12, 4
    rng = np.random.default_rng(4808)
    gs = full_gens(oracle, rng, k, Lb, G, r)
    assert all(rk == k for rk in gs.rank)
    rx, lens = I.frame_gens(oracle, gs)
    one = I.run_inplace(qf, rx, R.run_headers(qf, rx), r)      # one decode over all frames of every generation
    assert (one["st"] == OK).all()
    keep = [np.flatnonzero(gs.flags[g][: gs.n[g]]).tolist() for g in range(G)]
    counts = store_ref.cuts(np.random.default_rng(48), [int(x) for x in gs.n], polls)
    assert max(np.bincount(completing_poll(gs, counts))) > NM, "no poll completes more generations than the list holds"
    em = min(k, r)
    rec_rs = _r16(Lb) + 16
    rec_gs = em * rec_rs
    ref = store_ref.Store(G, k, Lb, k)                         # shapes only
    dev = S.DevStore(qf, ref)
    st = S.States(qf, G, k)
    t_seen = torch.zeros(G, dtype=torch.int32, device="cuda")
    t_all = _dev(np.arange(G, dtype=np.uint32))

    for rnd in range(2):                                       # the second round: reset generations fill and decode again
        listed = []
        pos = [0] * G
        t_rk = None
        for t in range(polls + 3):
            if t < polls:
                hi = [pos[g] + counts[g][t] for g in range(G)]
                p = S.poll_of(oracle, rx, pos, hi)
                pos = hi
                h = R.run_headers(qf, p)
                t_fl, t_rk, t_st = _filled(G * p.mr + 64), _filled(4 * G + 16), _filled(4 * G + 16)
                qf.rank_update_batch(h["idx"], st.t, t_rk, t_st, k, max_rows=p.mr, G=G, n_rows=h["n"], row_coeffs=h["co"],
                                     innovative=t_fl)
                status = dev.append(h["frames"], p.mr * p.fs, h["ro"], h["rl"], h["idx"], h["co"], h["n"], t_fl, mr=p.mr)
                assert (status == OK).all() and (_host(t_st, np.int32)[:G] == OK).all()
            else:
                # after the last poll the overflow of NM drains: polls that bring nothing, so that
                # rank_dev is the states' (a reset generation is back at rank 0)
                t_rk, t_st = _filled(4 * G + 16), _filled(4 * G + 16)
                qf.rank_update_batch(_dev(np.zeros(G, np.uint16)), st.t, t_rk, t_st, k, max_rows=1, G=G,
                                     n_rows=_dev(np.zeros(G, np.uint32)), row_coeffs=_dev(np.zeros((G, k), np.uint8)))
            t_sel, t_n, t_m = _filled(4 * NM + 16), _filled(16), _filled(16)
            qf.gen_select(t_rk, t_sel, t_n, G=G, min_rank=k, n_max=NM, seen=t_seen, mark=True, n_match=t_m)
            o = I._outputs(NM, k, em, k, rec_gs)
            qf.decode_frames_sel(t_sel, t_n, dev.bytes, dev.off, dev.len, dev.index, dev.coeffs, o["rec"], o["ri"],
                                 o["nrec"], o["st"], k, r, Lb, n_max=NM, G_src=G, max_rows=k,
                                 src_gen_stride=ref.gen_stride, rec_row_stride=rec_rs, rec_gen_stride=rec_gs,
                                 n_rows=dev.n, rank=o["rank"], innovative=o["flags"], src_slot=o["slot"])
            qf.stream_reset(t_sel, t_n, k, n_max=NM, G_src=G, state=st.t, store_n=dev.n, seen=t_seen)
            gpu_ctx.sync()
            n = int(_host(t_n, np.uint32)[0])
            sel = _host(t_sel, np.uint32)[:n].tolist()
            assert n == min(int(_host(t_m, np.uint32)[0]), NM)
            out = I._collect(o, NM, k, em, k, Lb, rec_rs, rec_gs, ("rank", "flags", "slot"))
            assert (out["st"][n:] == ENOTREADY).all()
            now, sn, seen = st.bytes(), _host(dev.n, np.uint32), _host(t_seen, np.uint32)
            for j, g in enumerate(sel):
                e = int(one["nrec"][g])
                assert out["st"][j] == OK and out["nrec"][j] == e and out["rank"][j] == k, (rnd, t, g)
                assert np.array_equal(out["ri"][j, :e], one["ri"][g, :e]), (rnd, t, g)
                assert np.array_equal(out["rec"][j, :e], one["rec"][g, :e]), (rnd, t, g)
                # the store holds the innovative frames in arrival order: store slot c is frame keep[g][c]
                want = [NONE16 if s == NONE16 else keep[g].index(int(s)) for s in one["slot"][g]]
                assert out["slot"][j].tolist() == want, (rnd, t, g)
                # the reset: an empty state, an empty store, not seen
                assert not now[g].any() and sn[g] == 0 and seen[g] == 0, (rnd, t, g)
            listed += sel
        assert sorted(listed) == list(range(G)), f"round {rnd}: the lists are not every generation exactly once"
        # rows that arrived after a generation was delivered started it again: reset everything
        qf.stream_reset(t_all, None, k, n_max=G, G_src=G, state=st.t, store_n=dev.n, seen=t_seen)
        gpu_ctx.sync()
        assert not st.bytes().any() and not _host(dev.n).any() and not _host(t_seen).any()


# ---------------------------------------------------------------------------
# call-level errors, profile names
# ---------------------------------------------------------------------------
def test_call_level_errors(qf, gpu_ctx):
    import torch

    from quicfuscate_amd import _lib as L_

    z = lambda n: torch.zeros(n, dtype=torch.uint8, device="cuda")   # noqa: E731
    lib, ctx, EI = L_._lib(), gpu_ctx.handle, L_.QF_EINVAL
    rank, seen, sel, n_sel, n_match = z(64), z(64), z(64), z(16), z(16)
    p = lambda t: t.data_ptr() if t is not None else None            # noqa: E731

    def select(G=4, rank=rank, seen=seen, flags=0, n_max=4, sel=sel, n_sel=n_sel):
        return lib.qf_gen_select_dev(ctx, G, p(rank), p(seen), 1, flags, n_max, p(sel), p(n_sel), p(n_match))

    assert select() == 0 and select(seen=None) == 0 and select(flags=1) == 0 and select(G=0, rank=None) == 0
    assert select(flags=2) == EI and select(flags=1, seen=None) == EI and select(n_max=0) == EI
    assert select(rank=None) == EI and select(sel=None) == EI and select(n_sel=None) == EI

    k, cap, Lb, m = 8, 8, 32, 3
    src, ro, rl, ri, co = z(4 * cap * 48), z(4 * 4 * cap), z(4 * 4 * cap), z(2 * 4 * cap), z(4 * cap * k)
    rec, rix, nrec, st = z(4 * 4 * 48), z(2 * 4 * 4), z(16), z(16)

    def gsel(sel=sel, n_max=4, G_src=4):
        return L_.GenSel(p(sel), None, n_max, G_src)

    def dec(gs=None, k=k, Lb=Lb, src=src.data_ptr(), rs=48, ro=ro, st=st, null_sel=False):
        sh = L_.DecodeFramesShape(k, 4, Lb, cap, 0, 0, cap * 48, rs, 4 * rs)
        gs = gs or gsel()
        return lib.qf_decode_frames_sel_dev(ctx, ctypes.byref(sh), None if null_sel else ctypes.byref(gs), src, p(ro),
                                            p(rl), p(ri), None, p(co), p(rec), p(rix), p(nrec), p(st), None, None, None)

    assert dec() == 0
    assert dec(null_sel=True) == EI and dec(gsel(sel=None)) == EI and dec(gsel(n_max=0)) == EI and dec(gsel(G_src=0)) == EI
    assert dec(k=0) == EI and dec(k=257) == EI and dec(Lb=0) == EI and dec(rs=40) == EI
    assert dec(src=src.data_ptr() + 8) == EI and dec(ro=None) == EI and dec(st=None) == EI

    out, oc = z(4 * m * 48), z(4 * m * k)

    def rec_(gs=None, k=k, m=m, out=out, rs=48, null_sel=False):
        sh = L_.RecodeFramesShape(k, Lb, cap, m, 0, 0, cap * 48, rs, m * rs)
        gs = gs or gsel()
        return lib.qf_recode_frames_sel_dev(ctx, ctypes.byref(sh), None if null_sel else ctypes.byref(gs),
                                            src.data_ptr(), p(ro), p(rl), p(ri), None, p(co), None, 7, p(out), p(oc), None,
                                            p(st))

    assert rec_() == 0
    assert rec_(null_sel=True) == EI and rec_(gsel(sel=None)) == EI and rec_(gsel(n_max=0)) == EI
    assert rec_(gsel(G_src=0)) == EI and rec_(k=256) == EI and rec_(m=0) == EI and rec_(m=65) == EI
    assert rec_(out=None) == EI and rec_(rs=40) == EI

    state, sn = z(4 * qf.rank_state_bytes(k) + 16), z(16)

    def reset(gs=None, k=k, state=state.data_ptr(), sn=sn, seen=seen, null_sel=False):
        gs = gs or gsel()
        return lib.qf_stream_reset_dev(ctx, k, None if null_sel else ctypes.byref(gs), state, p(sn), p(seen))

    assert reset() == 0 and reset(state=None) == 0 and reset(sn=None, seen=None) == 0
    assert reset(k=0) == EI and reset(k=257) == EI and reset(state=None, sn=None, seen=None) == EI
    assert reset(state=state.data_ptr() + 8) == EI
    assert reset(null_sel=True) == EI and reset(gsel(sel=None)) == EI and reset(gsel(n_max=0)) == EI
    assert reset(gsel(G_src=0)) == EI
    gpu_ctx.sync()


def test_profile_names(qf, gpu_ctx):
    k, r, cap, Lb, G_src, n_max, seed = C.SHAPES[0]
    st, _ = select_ref.listed_store(k, r, cap, Lb, G_src, seed)
    src = Up(st)
    em, rec_rs = min(k, r), _r16(Lb) + 16
    t_rank, t_seen = _dev(st.n.astype(np.uint32)), _dev(np.zeros(G_src, np.uint32))
    t_sel, t_n = _filled(4 * n_max), _filled(4)
    o = I._outputs(n_max, k, em, cap, em * rec_rs)
    state = _dev(np.zeros(G_src * qf.rank_state_bytes(k), np.uint8))
    gpu_ctx.sync()
    gpu_ctx.profile(True)
    qf.gen_select(t_rank, t_sel, t_n, G=G_src, min_rank=k, n_max=n_max, seen=t_seen, mark=True)
    qf.decode_frames_sel(t_sel, t_n, src.t["bytes"], src.t["off"], src.t["len"], src.t["index"], src.t["coeffs"],
                         o["rec"], o["ri"], o["nrec"], o["st"], k, r, Lb, n_max=n_max, G_src=G_src, max_rows=cap,
                         src_gen_stride=st.gen_stride, rec_row_stride=rec_rs, rec_gen_stride=em * rec_rs, n_rows=src.n)
    qf.stream_reset(t_sel, t_n, k, n_max=n_max, G_src=G_src, state=state, seen=t_seen)
    times = gpu_ctx.kernel_times()
    gpu_ctx.profile(False)
    assert sorted(times) == ["k_combine_rows_at", "k_decode_prepare", "k_gen_select", "k_rank_filter", "k_sel_gather",
                             "k_stream_reset"], times
    assert times["k_gen_select"][0] == 1 and times["k_sel_gather"][0] == 1 and times["k_stream_reset"][0] == 1
