"""The in-place receive step on the MI355X: qf_parse_frame_headers_dev ->
qf_decode_frames_dev, byte for byte against the copy path
(qf_parse_frames_coded_dev -> qf_decode_innovative_batch) on the same frames,
against tests/recv_ref.py (rank_ref's filter, the oracle's decode) and against
the sources the traffic was built from, and two hops on the device.

Every output buffer starts as 0xCC and the bytes a call must not write are
checked to still be 0xCC.  Every byte of every input slot outside
[frame_off, frame_off + frame_len) is 0xCC as well, so a kernel that reads a
row past its length changes an output byte."""
import ctypes

import numpy as np
import pytest

from quicfuscate_amd import _lib as L
from tests import rank_ref, recv_ref
from tests import test_gpu_rank as K
from tests import test_gpu_relay_inplace as R
from tests import test_gpu_wire_coded as W

pytestmark = pytest.mark.gpu

FILL = 0xCC
FILL16 = 0xCCCC
FILL32 = 0xCCCCCCCC
NONE16 = 0xFFFF
OK, EINVAL, ENOTREADY = 0, -1, -3

_r16, _P, _dev, _filled, _host = W._r16, W._P, W._dev, W._filled, W._host


# ---------------------------------------------------------------------------
# frames, the two receive paths, the checks
# ---------------------------------------------------------------------------
def frame_gens(oracle, gs, lens=None, extra=0):
    """tests.test_gpu_rank.Gens -> R.Received in the payload-aligned layout:
    slot s of generation g carries the first lens[g][s] bytes of gs.rows[g, s]
    as a systematic (index < k) or a coded frame with its vector.  lens None:
    the row without its trailing zeros for two slots of three, L for the
    third.  Slots at and after gs.n[g] hold no frame.  -> rx, lens (G, mr)."""
    k, Lb, G, mr = gs.k, gs.L, gs.G, gs.mr
    P = _P(k)
    fs = P + _r16(Lb) + extra
    rx = R.Received(oracle, None, k, Lb, mr, fs, [[] for _ in range(G)], [Lb])
    out_lens = np.zeros((G, mr), np.uint32)
    for g in range(G):
        n_g = min(int(gs.n[g]), mr)
        for s in range(n_g):
            row = gs.rows[g, s]
            ln = int(lens[g][s]) if lens is not None else (recv_ref.trimmed_len(row) if (g + s) % 3 else Lb)
            i = int(gs.idx[g, s])
            if i < k:
                raw = oracle.packet_to_raw(True, row[:ln].tobytes())[1]
                off, pid = P - 1, k * (11 + s) + i
            else:
                raw = oracle.packet_to_raw(False, row[:ln].tobytes(), gs.coeffs[g, s].tobytes())[1]
                off, pid = P - 3 - k, 100000 + 7 * s
            rx.frames[g, s, off: off + len(raw)] = np.frombuffer(raw, np.uint8)
            rx.flen[g, s], rx.foff[g, s], rx.ids[g, s] = len(raw), off, pid
            out_lens[g, s] = ln
        rx.nfr[g] = n_g
    return rx, out_lens


def refs_of_gens(oracle, gs, lens, r=None):
    """recv_ref.decode_ref per generation of a framed Gens (a coded frame
    parses to index k)."""
    k = gs.k
    out = []
    for g in range(gs.G):
        n_g = min(int(gs.n[g]), gs.mr)
        idx = np.minimum(gs.idx[g, :n_g].astype(np.int64), k)
        pay = [gs.rows[g, s, : int(lens[g, s])].tobytes() for s in range(n_g)]
        out.append(recv_ref.decode_ref(oracle, k, gs.r if r is None else r, gs.L, idx, gs.coeffs[g][:n_g], pay))
    return out


def refs_of_received(oracle, rx, r):
    _, egens = rx.expected(oracle)
    return [recv_ref.decode_ref(oracle, rx.k, r, rx.L, e["idx"], e["vecs"],
                                [e["rows"][s, : e["len"][s]].tobytes() for s in range(e["n"])]) for e in egens]


def _outputs(G, k, em, mr, rec_gs):
    return dict(rec=_filled(G * rec_gs + 64), ri=_filled(2 * G * em + 16), nrec=_filled(4 * G + 16),
                st=_filled(4 * G + 16), rank=_filled(4 * G + 16), flags=_filled(G * mr + 64),
                slot=_filled(2 * G * k + 16))


def _collect(t, G, k, em, mr, Lb, rec_rs, rec_gs, nullable):
    """Host views of the outputs; the bytes behind and between them are 0xCC."""
    rec, ri = _host(t["rec"]), _host(t["ri"], np.uint16)
    nrec, st = _host(t["nrec"], np.uint32), _host(t["st"], np.int32)
    rank, flags, slot = _host(t["rank"], np.uint32), _host(t["flags"]), _host(t["slot"], np.uint16)
    assert (rec[G * rec_gs:] == FILL).all() and (ri[G * em:] == FILL16).all()
    assert (nrec[G:] == FILL32).all() and (st[G:].view(np.uint32) == FILL32).all()
    assert (rank[G if "rank" in nullable else 0:] == FILL32).all()
    assert (flags[G * mr if "flags" in nullable else 0:] == FILL).all()
    assert (slot[G * k if "slot" in nullable else 0:] == FILL16).all()
    rg = rec[: G * rec_gs].reshape(G, rec_gs)
    assert (rg[:, em * rec_rs:] == FILL).all(), "bytes after a generation's last recovered row were written"
    rrow = rg[:, : em * rec_rs].reshape(G, em, rec_rs)
    assert (rrow[:, :, Lb:] == FILL).all(), "bytes between L and rec_row_stride were written"
    out = dict(rec=rrow[:, :, :Lb].copy(), ri=ri[: G * em].reshape(G, em).copy(), nrec=nrec[:G].copy(),
               st=st[:G].copy(), rank=rank[:G].copy() if "rank" in nullable else None,
               flags=flags[: G * mr].reshape(G, mr).copy() if "flags" in nullable else None,
               slot=slot[: G * k].reshape(G, k).copy() if "slot" in nullable else None)
    # the device decode's rule: rows at and after n_rec, and every row of a
    # generation that is not QF_OK, are not written
    for g in range(G):
        keep = int(out["nrec"][g]) if out["st"][g] == OK else 0
        assert out["st"][g] == OK or out["nrec"][g] == 0, g
        assert (out["rec"][g, keep:] == FILL).all(), f"unrecovered rows of generation {g} were written"
        assert (out["ri"][g, keep:] == FILL16).all(), g
    return out


def run_inplace(qf, rx, h, r, *, rec_rs=None, gap=0, pass_n=True, nullable=("rank", "flags", "slot"), row_off=None,
                row_len=None, n_rows=None, idx=None, src_gen_stride=None):
    """decode_frames over the frame buffer of `h` (R.run_headers).  row_off /
    row_len / n_rows / idx: host arrays that replace the parser's."""
    G, mr, k, Lb = rx.G, rx.mr, rx.k, rx.L
    em = min(k, r)
    rec_rs = _r16(Lb) + 16 if rec_rs is None else rec_rs
    rec_gs = em * rec_rs + gap
    t = _outputs(G, k, em, mr, rec_gs)
    t_ro = h["ro"] if row_off is None else _dev(row_off)
    t_rl = h["rl"] if row_len is None else _dev(row_len)
    t_n = h["n"] if n_rows is None else _dev(n_rows)
    t_idx = h["idx"] if idx is None else _dev(idx)
    qf.decode_frames(h["frames"], t_ro, t_rl, t_idx, h["co"], t["rec"], t["ri"], t["nrec"], t["st"], k, r, Lb,
                     max_rows=mr, src_gen_stride=mr * rx.fs if src_gen_stride is None else src_gen_stride,
                     rec_row_stride=rec_rs, rec_gen_stride=rec_gs, G=G, n_rows=t_n if pass_n else None,
                     rank=t["rank"] if "rank" in nullable else None,
                     innovative=t["flags"] if "flags" in nullable else None,
                     src_slot=t["slot"] if "slot" in nullable else None)
    qf.default_context().sync()
    assert np.array_equal(_host(h["frames"]), rx.frames.reshape(-1)), "the source was written"
    return _collect(t, G, k, em, mr, Lb, rec_rs, rec_gs, nullable)


def run_copy(qf, rx, c, r, *, rec_rs=None, gap=0, pass_n=True, n_rows=None, idx=None):
    """decode_innovative_batch over the coded parser's rows (R.run_coded): the yardstick."""
    G, mr, k, Lb = rx.G, rx.mr, rx.k, rx.L
    em = min(k, r)
    rec_rs = _r16(Lb) + 16 if rec_rs is None else rec_rs
    rec_gs = em * rec_rs + gap
    t = _outputs(G, k, em, mr, rec_gs)
    t_n = c["n"] if n_rows is None else _dev(n_rows)
    t_idx = c["idx"] if idx is None else _dev(idx)
    qf.decode_innovative_batch(c["rows"], t_idx, t["rec"], t["ri"], t["nrec"], t["st"], k, r, Lb, max_rows=mr,
                               row_stride=c["rs"], rows_gen_stride=mr * c["rs"], rec_row_stride=rec_rs,
                               rec_gen_stride=rec_gs, G=G, n_rows=t_n if pass_n else None, row_coeffs=c["co"],
                               rank=t["rank"], innovative=t["flags"])
    qf.default_context().sync()
    return _collect(t, G, k, em, mr, Lb, rec_rs, rec_gs, ("rank", "flags"))


def same_as_copy(a, b):
    """Byte for byte, the unwritten 0xCC bytes included."""
    for key in ("rec", "ri", "nrec", "st", "rank", "flags"):
        if a[key] is not None:
            assert np.array_equal(a[key], b[key]), f"{key} differs from the copy path"


def check_refs(out, refs, rx=None, h=None, gens=None):
    """The outputs against recv_ref.decode_ref; with rx and h also the packet
    src_slot points at."""
    for g in (range(len(refs)) if gens is None else gens):
        ref = refs[g]
        e = len(ref["erased"])
        assert out["st"][g] == ref["status"], (g, out["st"][g], ref["status"])
        assert out["nrec"][g] == e, (g, out["nrec"][g], e)
        n = len(ref["flags"])
        if out["rank"] is not None:
            assert out["rank"][g] == ref["rank"], g
        if out["flags"] is not None:
            assert np.array_equal(out["flags"][g, :n], ref["flags"]) and not out["flags"][g, n:].any(), g
        if out["slot"] is not None:
            assert np.array_equal(out["slot"][g], ref["src_slot"]), (g, out["slot"][g], ref["src_slot"])
        if ref["status"] != OK:
            continue
        assert out["ri"][g, :e].tolist() == ref["erased"], g
        assert np.array_equal(out["rec"][g, :e], ref["rec"]), f"recovered rows of generation {g}"


def both_ways(qf, oracle, rx, r, refs, **kw):
    """headers -> decode_frames against the copy path on the same frames and
    against the reference."""
    h = R.run_headers(qf, rx)
    out = run_inplace(qf, rx, h, r, **kw)
    cp = run_copy(qf, rx, R.run_coded(qf, rx), r, **{key: v for key, v in kw.items() if key in ("rec_rs", "gap")})
    same_as_copy(out, cp)
    check_refs(out, refs)
    return h, out


def spread_sys_ids(rx, rng, repeats=1):
    """The systematic frames of each generation get distinct sources (ids with
    distinct id % k, as far as k reaches), but for `repeats` of them."""
    k = rx.k
    for g, gen in enumerate(rx.meta):
        slots = [s for s, m in enumerate(gen) if m[4] == "sys"]
        perm = [int(x) for x in rng.permutation(k)]
        for j, s in enumerate(slots):
            i = perm[j % k] if j >= repeats or j == 0 else perm[0]
            pid = k * (3 + s) + i
            raw, fl, off, _, kind = gen[s]
            gen[s] = (raw, fl, off, pid, kind)
            rx.ids[g, s] = pid


# ---------------------------------------------------------------------------
# 1. parity with the copy path
# ---------------------------------------------------------------------------
PARITY = [(4, 8, 6, 4), (13, 33, 20, 13), (16, 1, 20, 16), (64, 1200, 80, 64), (256, 16, 260, 128)]


@pytest.mark.parametrize("k,Lb,mr,r", PARITY)
def test_parity_with_the_copy_path(qf, oracle, gpu_ctx, k, Lb, mr, r):
    rng = np.random.default_rng(k * 977 + Lb)
    fs = _P(k) + _r16(Lb)
    lens = sorted({0, 1, 15, 16, 17, Lb} & set(range(Lb + 1)))

    def mix(count, n_sys, n_zero):
        kd = ["sys"] * n_sys + ["zero_vec"] * n_zero + ["any"] * (count - n_sys - n_zero)
        rng.shuffle(kd)
        return kd

    kinds = [mix(mr, (mr * 11) // 20, 1),           # systematic and coded rows, rank k before the last slot
             mix(mr, 0, 1),                         # all coded: e = k, QF_EINVAL where r < k
             mix(k - 1, k // 2, 0),                 # fewer frames than slots, rank short of k
             mix(mr - 2, (mr * 9) // 20, 1),
             mix(mr, (mr * 3) // 4, 2)]
    if k == 256:
        kinds = kinds[:3]                           # (the reference's elimination takes a second per generation)
    rx = R.Received(oracle, rng, k, Lb, mr, fs, kinds, lens)
    spread_sys_ids(rx, rng, repeats=2 if k > 4 else 1)
    refs = refs_of_received(oracle, rx, r)
    _, out = both_ways(qf, oracle, rx, r, refs)
    sts = [ref["status"] for ref in refs]
    assert sts[2] == ENOTREADY and sts[1] == (OK if r >= k else EINVAL), sts
    assert sts[0] == OK and 0 < out["nrec"][0] <= min(k, r), (sts, out["nrec"])
    assert 0 < out["rank"][2] < k and out["nrec"][2] == 0


# ---------------------------------------------------------------------------
# 2. recovered bytes are the originals
# ---------------------------------------------------------------------------
def tailed_gens(oracle, rng, k, mr, Lb, G, **kw):
    """K.random_gens with sources that end in zero tails of different lengths."""
    g0 = K.random_gens(oracle, rng, k, mr, Lb, G, **kw)
    return K.Gens(oracle, k, g0.r, Lb, recv_ref.tailed_sources(rng, G, k, Lb), g0.idx, g0.n, g0.coeffs)


def check_sources(gs, rx, h, out):
    """Every source of every QF_OK generation, through src_slot or rec_index,
    is the original; src_slot is the one innovative slot with that index."""
    ro = _host(h["ro"], np.uint32)[: gs.G * gs.mr].reshape(gs.G, gs.mr)
    rl = _host(h["rl"], np.uint32)[: gs.G * gs.mr].reshape(gs.G, gs.mr)
    region = rx.frames.reshape(gs.G, -1)
    n_ok = 0
    for g in range(gs.G):
        est, erased = gs.expected(g)
        assert out["st"][g] == est, (g, out["st"][g], est)
        if est != OK:
            assert (out["slot"][g] == NONE16).all(), g
            continue
        n_ok += 1
        assert out["ri"][g, : len(erased)].tolist() == erased, g
        for i in range(gs.k):
            c = int(out["slot"][g, i])
            if i in erased:
                assert c == NONE16, (g, i)
                pkt = out["rec"][g, erased.index(i)]
            else:
                inn = [s for s in np.flatnonzero(gs.flags[g]) if gs.idx[g, s] == i]
                assert [c] == inn, (g, i, c, inn)
                pkt = np.zeros(gs.L, np.uint8)
                pkt[: rl[g, c]] = region[g, ro[g, c]: ro[g, c] + rl[g, c]]
            assert np.array_equal(pkt, gs.src[g, i]), (g, i)
    return n_ok


def test_recovered_bytes_are_the_originals(qf, oracle, gpu_ctx):
    k, mr, Lb, G = 16, 24, 100, 8
    rng = np.random.default_rng(2100)
    gs = tailed_gens(oracle, rng, k, mr, Lb, G, p_sys=0.5, p_dep=0.25)
    assert any(0 < f[:k].sum() < k for f in gs.flags), "no dependent row among the first k"
    rx, lens = frame_gens(oracle, gs)
    assert (lens < Lb).sum() > G * mr // 4 and (lens == Lb).any()
    h, out = both_ways(qf, oracle, rx, k, refs_of_gens(oracle, gs, lens))
    K.check_decode(oracle, gs, out)
    assert check_sources(gs, rx, h, out) >= G // 2


def test_planted_arrival_orders(qf, oracle, gpu_ctx):
    k, Lb = 16, 100
    names, src, idx, co, V, rows = recv_ref.plant(oracle, np.random.default_rng(77), k, Lb)
    gs = K.Gens(oracle, k, k, Lb, src, idx, None, co)
    assert all(rk == k for rk in gs.rank)
    rx, lens = frame_gens(oracle, gs)
    h, out = both_ways(qf, oracle, rx, k, refs_of_gens(oracle, gs, lens))
    K.check_decode(oracle, gs, out)
    assert check_sources(gs, rx, h, out) == len(names)
    g = names.index("e2 + e7, then systematic 2, then systematic 7")
    assert out["slot"][g, 2] == 1 and out["slot"][g, 7] == NONE16


# ---------------------------------------------------------------------------
# 3. pass boundaries inside one wave
# ---------------------------------------------------------------------------
def test_pass_boundaries_inside_one_wave(qf, oracle, gpu_ctx):
    """k = 48, L = 16: one unit per generation, 64 generations per wave, and
    erasure counts on both sides of every pass boundary side by side, so the
    lanes of a wave differ in their output count in each of the three passes."""
    k, r, Lb, G, mr = 48, 48, 16, 130, 52
    counts = [0, 1, 15, 16, 17, 31, 32, 33, 48]
    rng = np.random.default_rng(4816)
    P = _P(k)
    fs = P + 16
    src = rng.integers(0, 256, (G, k, Lb), dtype=np.uint8)
    rx = R.Received(oracle, None, k, Lb, mr, fs, [[] for _ in range(G)], [Lb])
    erased_of, rows_of, idx_of, co_of = [], [], [], []
    for g in range(G):
        e = counts[g % len(counts)]
        perm = rng.permutation(k)
        erased = sorted(int(x) for x in perm[:e])
        arr = [int(x) for x in perm[e:]] + [k] * e
        rng.shuffle(arr)
        # behind the first k rows: a repeated source (when one arrived) and more coded rows
        arr += [arr[0] if arr[0] < k else k, k, k, k][: mr - k]
        for _ in range(20):                       # (random vectors: the first k rows are independent as a rule)
            co = rng.integers(0, 256, (mr, k), dtype=np.uint8)
            Vg = np.array([np.eye(k, dtype=np.uint8)[i] if i < k else co[s] for s, i in enumerate(arr)])
            rows = oracle.encode(src[g], mr, np.ascontiguousarray(Vg))
            st, dec, _ = oracle.decode(k, np.array(arr[:k], np.uint16), rows[:k], np.ascontiguousarray(Vg[:k]))
            if st == OK:
                break
        assert st == OK and np.array_equal(dec, src[g]), f"the first k rows of generation {g} are dependent"
        for s, i in enumerate(arr):
            pay = rows[s] if s < k else np.full(Lb, 0xEE, np.uint8)     # no row behind rank k reaches an output
            if i < k:
                rx.frames[g, s, P - 1] = 1
                rx.flen[g, s], rx.foff[g, s], rx.ids[g, s] = 1 + Lb, P - 1, k * (5 + s) + i
            else:
                rx.frames[g, s, P - 3 - k: P] = np.concatenate([[0, k >> 8, k & 255], co[s]]).astype(np.uint8)
                rx.flen[g, s], rx.foff[g, s], rx.ids[g, s] = 3 + k + Lb, P - 3 - k, 9000 + s
            rx.frames[g, s, P: P + Lb] = pay
        rx.nfr[g] = mr
        erased_of.append(erased)
    h = R.run_headers(qf, rx)
    assert (_host(h["n"], np.uint32)[:G] == mr).all() and (_host(h["st"], np.int32)[: G * mr] == OK).all()
    gpu_ctx.sync()
    gpu_ctx.profile(True)
    out = run_inplace(qf, rx, h, r)
    times = gpu_ctx.kernel_times()
    gpu_ctx.profile(False)
    assert times["k_rank_filter"][0] == 1 and times["k_decode_prepare"][0] == 1, times
    assert times["k_combine_rows_at"][0] == 3 and len(times) == 3, times
    same_as_copy(out, run_copy(qf, rx, R.run_coded(qf, rx), r))
    assert (out["st"] == OK).all() and (out["rank"] == k).all()
    for g in range(G):
        e = len(erased_of[g])
        assert out["nrec"][g] == e and out["ri"][g, :e].tolist() == erased_of[g], g
        assert np.array_equal(out["rec"][g, :e], src[g][erased_of[g]]), f"recovered rows of generation {g}"
        assert (out["flags"][g, :k] == 1).all() and not out["flags"][g, k:].any(), g
        assert [i for i in range(k) if out["slot"][g, i] == NONE16] == erased_of[g], g


# ---------------------------------------------------------------------------
# 4. all coded, many passes
# ---------------------------------------------------------------------------
def test_k128_all_coded_eight_passes(qf, oracle, gpu_ctx):
    k, mr, Lb, G = 128, 130, 48, 2
    rng = np.random.default_rng(128)
    gs = tailed_gens(oracle, rng, k, mr, Lb, G, r=128, p_sys=0.0, p_dep=0.01)
    assert gs.rank == [k, k] and all(f.sum() == k and not f.all() for f in gs.flags)
    rx, lens = frame_gens(oracle, gs)
    h = R.run_headers(qf, rx)
    gpu_ctx.sync()
    gpu_ctx.profile(True)
    out = run_inplace(qf, rx, h, 128)
    times = gpu_ctx.kernel_times()
    gpu_ctx.profile(False)
    assert times["k_combine_rows_at"][0] == 8 and len(times) == 3, times
    same_as_copy(out, run_copy(qf, rx, R.run_coded(qf, rx), 128))
    assert (out["nrec"] == 128).all() and (out["slot"] == NONE16).all()
    K.check_decode(oracle, gs, out)


def test_k64_eighty_coded_rows_planted_dependents(qf, oracle, gpu_ctx):
    """80 coded rows, 8 of the first 64 combinations of earlier ones: 64
    recovered in four passes from rows 0 .. 71 without the planted eight."""
    k, mr, Lb, G = 64, 80, 208, 3
    rng = np.random.default_rng(6480)
    co =rng.integers(0, 256, (G, mr, k), dtype=np.uint8)
    for g in range(G):
        for s in sorted(int(x) for x in rng.choice(np.arange(2, 64), 8, replace=False)):
            a, b = (int(x) for x in rng.choice(s, 2, replace=False))
            co[g, s] = oracle.encode(np.stack([co[g, a], co[g, b]]), 1, np.array([[0x35, 0xB2]], np.uint8))[0]
    idx = np.full((G, mr), k, np.uint16)
    gs = K.Gens(oracle, k, k, Lb, recv_ref.tailed_sources(rng, G, k, Lb), idx, None, co)
    for g in range(G):
        assert gs.rank[g] == k and gs.flags[g][:64].sum() == 56 and gs.flags[g][:72].sum() == 64, g
    rx, lens = frame_gens(oracle, gs)
    h, out = both_ways(qf, oracle, rx, k, refs_of_gens(oracle, gs, lens))
    assert (out["nrec"] == 64).all()
    K.check_decode(oracle, gs, out)


# ---------------------------------------------------------------------------
# 5. full and ragged paths
# ---------------------------------------------------------------------------
def test_full_and_ragged_paths(qf, oracle, gpu_ctx):
    k, mr, Lb, G = 16, 20, 208, 4
    rng = np.random.default_rng(208)
    gs = K.random_gens(oracle, rng, k, mr, Lb, G, p_sys=0.5, p_dep=0.2)
    assert all(rk == k for rk in gs.rank) and all(not f.all() for f in gs.flags)
    # every row full: the pipelined path
    full_lens = np.full((G, mr), Lb, np.uint32)
    rx, _ = frame_gens(oracle, gs, full_lens)
    _, full = both_ways(qf, oracle, rx, k, refs_of_gens(oracle, gs, full_lens))
    K.check_decode(oracle, gs, full)
    # one accepted row of 77 bytes per generation: the masked path (the row is then another row)
    lens = full_lens.copy()
    for g in range(G):
        lens[g, int(np.flatnonzero(gs.flags[g])[g + 1])] = 77
    rx2, _ = frame_gens(oracle, gs, lens)
    _, ragged = both_ways(qf, oracle, rx2, k, refs_of_gens(oracle, gs, lens))
    assert any(not np.array_equal(ragged["rec"][g], full["rec"][g]) for g in range(G) if full["nrec"][g])
    # only a non-innovative row is short: min_len is over the accepted rows, and the result is the full one
    lens = full_lens.copy()
    for g in range(G):
        lens[g, int(np.flatnonzero(gs.flags[g] == 0)[0])] = 5
    rx3, _ = frame_gens(oracle, gs, lens)
    _, third = both_ways(qf, oracle, rx3, k, refs_of_gens(oracle, gs, lens))
    for key in ("rec", "ri", "nrec", "st", "rank", "flags", "slot"):
        assert np.array_equal(third[key], full[key]), key


# ---------------------------------------------------------------------------
# 6. row counts and bad rows
# ---------------------------------------------------------------------------
def test_row_counts_and_bad_rows(qf, oracle, gpu_ctx):
    k, r, mr, Lb, G = 16, 16, 24, 53, 10
    rng = np.random.default_rng(653)
    gs = tailed_gens(oracle, rng, k, mr, Lb, G, r=r, p_sys=0.5, p_dep=0.2)
    assert all(rk == k for rk in gs.rank) and all(not f.all() for f in gs.flags)
    rx, lens = frame_gens(oracle, gs)
    h = R.run_headers(qf, rx)
    ro = _host(h["ro"], np.uint32)[: G * mr].reshape(G, mr).copy()
    rl = _host(h["rl"], np.uint32)[: G * mr].reshape(G, mr).copy()
    idx = _host(h["idx"], np.uint16)[: G * mr].reshape(G, mr).copy()
    n = _host(h["n"], np.uint32)[:G].copy()
    assert (n == mr).all() and np.array_equal(rl, lens)
    inn = lambda g, j: int(np.flatnonzero(gs.flags[g])[j])            # noqa: E731
    non = lambda g: int(np.flatnonzero(gs.flags[g] == 0)[0])         # noqa: E731
    n[1] = 0                                      # QF_ENOTREADY
    n[2] = k - 1                                  # QF_ENOTREADY, the rank reported
    n[3] = mr + 1                                 # clamped to max_rows
    coded = [s for s in range(mr) if idx[4, s] >= k]
    idx[4, coded[-1]] = k + 256                   # breaks index - k < 256
    rl[5, inn(5, 3)] = Lb + 1                     # an accepted row longer than L
    ro[6, inn(6, 0)] += 8
    ro[7, inn(7, 5)], rl[7, inn(7, 5)] = mr * rx.fs - 16, 17
    rl[8, non(8)] = Lb + 1                        # the offending row is not innovative
    got = run_inplace(qf, rx, h, r, row_off=ro, row_len=rl, n_rows=n, idx=idx)
    assert got["st"].tolist() == [OK, ENOTREADY, ENOTREADY, OK, EINVAL, EINVAL, EINVAL, EINVAL, EINVAL, OK]
    refs = refs_of_gens(oracle, gs, lens)
    # NULL n_rows: max_rows rows each, so generations 1 and 2 decode as well
    nul = run_inplace(qf, rx, h, r, pass_n=False, row_off=ro, row_len=rl, idx=idx)
    assert nul["st"].tolist() == [OK, OK, OK, OK, EINVAL, EINVAL, EINVAL, EINVAL, EINVAL, OK]
    check_refs(nul, refs, gens=(0, 1, 2, 3, 9))
    # generation 2 with its first k - 1 rows only
    pay = [gs.rows[2, s, : int(lens[2, s])].tobytes() for s in range(k - 1)]
    refs[2] = recv_ref.decode_ref(oracle, k, r, Lb, np.minimum(gs.idx[2, : k - 1].astype(np.int64), k),
                                  gs.coeffs[2][: k - 1], pay)
    refs[1] = recv_ref.decode_ref(oracle, k, r, Lb, [], gs.coeffs[1][:0], [])
    assert refs[2]["status"] == ENOTREADY and 0 < refs[2]["rank"] < k
    check_refs(got, refs, gens=(0, 1, 2, 3, 9))
    assert got["rank"][1] == 0 and not got["flags"][1].any()
    # the index rule: what qf_rank_batch writes for an invalid generation
    assert got["rank"][4] == 0 and not got["flags"][4].any() and got["nrec"][4] == 0
    # the geometry rules: n_rec 0, rec untouched (checked in run_inplace), no
    # src_slot; the rank and the flags depend on the vectors only
    for g in (5, 6, 7, 8):
        assert got["nrec"][g] == 0 and (got["slot"][g] == NONE16).all(), g
        assert got["rank"][g] == k and np.array_equal(got["flags"][g], gs.flags[g]), g
    assert (got["slot"][[1, 2, 4]] == NONE16).all()
    # the neighbours of the bad generations are the copy path's
    c = R.run_coded(qf, rx)
    cp = run_copy(qf, rx, c, r, n_rows=n, idx=idx)
    for g in (0, 1, 2, 3, 4, 9):
        for key in ("rec", "ri", "nrec", "st", "rank", "flags"):
            assert np.array_equal(got[key][g], cp[key][g]), (key, g)
    K.check_decode(oracle, K.Gens(oracle, k, r, Lb, gs.src[[0, 3, 9]], gs.idx[[0, 3, 9]], None, gs.coeffs[[0, 3, 9]]),
                   {key: (v[[0, 3, 9]] if v is not None else None) for key, v in got.items()})


# ---------------------------------------------------------------------------
# 7. wide strides, nullable outputs, NULL n_rows
# ---------------------------------------------------------------------------
def test_wide_strides_nullable_outputs_and_null_n_rows(qf, oracle, gpu_ctx):
    k, mr, Lb, G = 8, 12, 33, 3
    rng = np.random.default_rng(833)
    gs = tailed_gens(oracle, rng, k, mr, Lb, G, p_sys=0.5, p_dep=0.2)
    assert all(rk == k for rk in gs.rank)
    rx, lens = frame_gens(oracle, gs, extra=32)
    refs = refs_of_gens(oracle, gs, lens)
    assert any(ref["erased"] for ref in refs)
    # rows 48 bytes apart from their end and 80 bytes between generations
    h, wide = both_ways(qf, oracle, rx, k, refs, rec_rs=96, gap=80)
    plain = run_inplace(qf, rx, h, k)
    bare = run_inplace(qf, rx, h, k, nullable=())                       # rank, innovative and src_slot NULL
    no_n = run_inplace(qf, rx, h, k, pass_n=False)                      # NULL n_rows: max_rows
    for other in (plain, bare, no_n):
        for key in ("rec", "ri", "nrec", "st"):
            assert np.array_equal(wide[key], other[key]), key
    assert bare["rank"] is None and bare["flags"] is None and bare["slot"] is None
    assert np.array_equal(no_n["slot"], wide["slot"]) and np.array_equal(no_n["flags"], wide["flags"])
    # r below the erasure count of a generation: QF_EINVAL for it alone, as the copy path
    e_max = max(len(ref["erased"]) for ref in refs)
    if e_max > 1:
        small = refs_of_gens(oracle, gs, lens, r=e_max - 1)
        both_ways(qf, oracle, rx, e_max - 1, small)
        assert EINVAL in [ref["status"] for ref in small]


# ---------------------------------------------------------------------------
# 8. call-level errors
# ---------------------------------------------------------------------------
def test_decode_frames_call_level_errors(qf, gpu_ctx):
    import torch

    t = lambda n, dt=torch.uint8: torch.zeros(n, dtype=dt, device="cuda")   # noqa: E731
    src, ro, rl = t(1024 * 64 + 16), t(1024, torch.int32), t(1024, torch.int32)
    idx, co = t(1024, torch.int16), t(1024 * 256)
    rec, ri, nrec, st = t(128 * 48 + 16), t(256, torch.int16), t(1, torch.int32), t(1, torch.int32)
    rk, fl, sl = t(1, torch.int32), t(1024), t(256, torch.int16)
    rl += 32
    lib, ctx = L._lib(), gpu_ctx.handle
    ptrs = dict(src=src, ro=ro, rl=rl, idx=idx, co=co, rec=rec, ri=ri, nrec=nrec, st=st)

    def status(k=8, r=4, Lb=32, max_rows=8, flags=0, reserved=0, sgs=8 * 64, rrs=48, rgs=128 * 48, G_=1, handle=ctx,
               shape=True, null=(), shift=None, opt=True):
        sh = L.DecodeFramesShape(k, r, Lb, max_rows, flags, reserved, sgs, rrs, rgs)
        p = {nm: (None if nm in null else tt.data_ptr() + (8 if nm == shift else 0)) for nm, tt in ptrs.items()}
        return lib.qf_decode_frames_dev(handle, ctypes.byref(sh) if shape else None, G_, p["src"], p["ro"], p["rl"],
                                        p["idx"], None, p["co"], p["rec"], p["ri"], p["nrec"], p["st"],
                                        rk.data_ptr() if opt else None, fl.data_ptr() if opt else None,
                                        sl.data_ptr() if opt else None)

    E = L.QF_EINVAL
    assert status() == 0 and status(opt=False) == 0
    assert status(handle=None) == E and status(shape=False) == E
    assert status(k=0) == E and status(k=257) == E
    assert status(k=256, r=128, max_rows=4) == 0
    assert status(max_rows=0) == E and status(max_rows=1025) == E
    assert status(max_rows=1024, sgs=1024 * 64) == 0
    assert status(k=200, r=129, max_rows=4) == E                 # min(k, r) > 128
    assert status(k=128, r=1000, max_rows=4) == 0                # r bounds the recovered rows only
    assert status(Lb=0) == E
    assert status(flags=1) == E and status(reserved=1) == E
    assert status(Lb=64, rrs=48) == E                            # a stride shorter than L
    assert status(rrs=40) == E and status(rgs=128 * 48 + 8) == E and status(sgs=8 * 64 + 8) == E
    assert status(shift="src") == E and status(shift="rec") == E
    for nm in ptrs:
        assert status(null=(nm,)) == E, nm                       # every one of them is required
    assert status(r=0, null=("rec", "ri")) == 0                  # nothing can be recovered: no rec, no rec_index
    assert status(G_=0, null=tuple(ptrs)) == 0
    gpu_ctx.sync()
    assert st.cpu().numpy()[0] == ENOTREADY                      # source 0 eight times: rank 1


# ---------------------------------------------------------------------------
# 9. two hops on the device
# ---------------------------------------------------------------------------
def test_two_hops_on_the_device(qf, oracle, gpu_ctx):
    """Sender frames -> relay (parse_frame_headers, recode_frames into the
    output slots, frame_rows in place) -> receiver (parse_frame_headers,
    decode_frames).  The receiver also holds three systematic frames that
    reached it directly; every source comes back through src_slot or rec_index."""
    k, r, Lb, G, m, direct = 16, 6, 40, 4, 18, 3
    rng = np.random.default_rng(1609)
    P = _P(k)
    fs = P + _r16(Lb)
    src = recv_ref.tailed_sources(rng, G, k, Lb)
    rep = np.stack([oracle.encode(src[g], r) for g in range(G)])
    C = oracle.cauchy(k, r)
    n_held = k + r - 2
    rx = R.Received(oracle, rng, k, Lb, n_held, fs, [[] for _ in range(G)], [Lb])
    X, V, first = [], [], []
    for g in range(G):
        lost = set(rng.choice(k, 2, replace=False).tolist())
        arr = [i for i in range(k + r) if i not in lost]
        rng.shuffle(arr)
        for s, i in enumerate(arr):
            row = src[g, i] if i < k else rep[g, i - k]
            ln = recv_ref.trimmed_len(row) if i < k else Lb
            raw = oracle.packet_to_raw(i < k, row[:ln].tobytes(), None if i < k else C[i - k].tobytes())[1]
            off = P - 1 if i < k else P - 3 - k
            rx.frames[g, s, off: off + len(raw)] = np.frombuffer(raw, np.uint8)
            rx.flen[g, s], rx.foff[g, s], rx.ids[g, s] = len(raw), off, (5 * k + i if i < k else 1000 + i)
        rx.nfr[g] = n_held
        X.append(np.stack([src[g, i] if i < k else rep[g, i - k] for i in arr]))
        V.append(np.stack([np.eye(k, dtype=np.uint8)[i] if i < k else C[i - k] for i in arr]))
        first.append([s for s, i in enumerate(arr) if i < k][:direct])
    # the seed, chosen on the CPU: the recoded vectors of every generation have rank k
    seed = None
    for cand in range(1, 50):
        M = R.seeded_mix(oracle, G, m, n_held, cand)
        if all(rank_ref.innovative(oracle.encode(V[g], m, np.ascontiguousarray(M[g])))[1] == k for g in range(G)):
            seed = cand
            break
    assert seed is not None, "no seed gives every generation rank k"

    # relay
    h = R.run_headers(qf, rx)
    assert (_host(h["st"], np.int32)[: G * n_held] == OK).all() and (_host(h["n"], np.uint32)[:G] == n_held).all()
    t_out = _filled(G * m * fs)
    t_oc, t_ol, t_st = _filled(G * m * k), _filled(4 * G * m), _filled(4 * G)
    qf.recode_frames(h["frames"], h["ro"], h["rl"], h["idx"], h["co"], t_out[P:], t_oc, t_st, k, m, Lb,
                     max_rows=n_held, src_gen_stride=n_held * fs, out_row_stride=fs, out_gen_stride=m * fs, G=G,
                     n_rows=h["n"], seed=seed, out_len=t_ol)
    t_flen, t_foff = _filled(4 * G * m), _filled(4 * G * m)
    qf.frame_rows(None, t_out, t_flen, k, Lb, max_rows=m, frame_stride=fs, G=G, row_coeffs=t_oc, row_len=t_ol,
                  frame_off=t_foff, in_place=True)
    gpu_ctx.sync()
    assert (_host(t_st, np.int32) == OK).all()

    # receiver: per generation three of the sender's systematic frames, then the relay's m
    mr = direct + m
    frames = np.full((G, mr, fs), FILL, np.uint8)
    flen, foff = np.zeros((G, mr), np.uint32), np.zeros((G, mr), np.uint32)
    ids = np.zeros((G, mr), np.uint64)
    frames[:, direct:] = _host(t_out).reshape(G, m, fs)
    flen[:, direct:] = _host(t_flen, np.uint32).reshape(G, m)
    foff[:, direct:] = _host(t_foff, np.uint32).reshape(G, m)
    ids[:, direct:] = 7000 + np.arange(m, dtype=np.uint64)
    for g in range(G):
        for j, s in enumerate(first[g]):
            frames[g, j], flen[g, j], foff[g, j], ids[g, j] = rx.frames[g, s], rx.flen[g, s], rx.foff[g, s], rx.ids[g, s]
    rcv = R.Received(oracle, None, k, Lb, mr, fs, [[] for _ in range(G)], [Lb])
    rcv.frames, rcv.flen, rcv.foff, rcv.ids = frames, flen, foff, ids
    rcv.nfr = np.full(G, mr, np.uint32)
    h2 = R.run_headers(qf, rcv)
    assert (_host(h2["st"], np.int32)[: G * mr] == OK).all() and (_host(h2["n"], np.uint32)[:G] == mr).all()
    out = run_inplace(qf, rcv, h2, k)
    same_as_copy(out, run_copy(qf, rcv, R.run_coded(qf, rcv), k))
    assert (out["st"] == OK).all() and (out["rank"] == k).all() and (out["nrec"] == k - direct).all(), out
    ro = _host(h2["ro"], np.uint32)[: G * mr].reshape(G, mr)
    rl = _host(h2["rl"], np.uint32)[: G * mr].reshape(G, mr)
    region = frames.reshape(G, -1)
    for g in range(G):
        rix = out["ri"][g, : k - direct].tolist()
        for i in range(k):
            c = int(out["slot"][g, i])
            pkt = np.zeros(Lb, np.uint8)
            if c == NONE16:
                pkt[:] = out["rec"][g, rix.index(i)]
            else:
                assert c < direct
                pkt[: rl[g, c]] = region[g, ro[g, c]: ro[g, c] + rl[g, c]]
            assert np.array_equal(pkt, src[g, i]), (g, i)
        assert sum(1 for i in range(k) if out["slot"][g, i] != NONE16) == direct
