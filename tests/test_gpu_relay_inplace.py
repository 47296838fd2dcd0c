"""The in-place relay step on the MI355X: qf_parse_frame_headers_dev against
qf_parse_frames_coded_dev and the oracle's from_raw, qf_recode_frames_dev
against the CPU oracle (oracle.encode over the zero-padded rows and over the
vectors, with the fill_splitmix mix) and bit for bit against the three-call
pipeline (parse_frames_coded -> recode_batch) on the device, and one hop
frames in, frames out, decoded by a receiver.

Every output buffer starts as 0xCC and the bytes a call must not write are
checked to still be 0xCC.  Every byte of every input slot outside
[frame_off, frame_off + frame_len) is 0xCC as well, so a kernel that reads a
row past its length changes an output byte."""
import ctypes

import numpy as np
import pytest

from quicfuscate_amd import _lib as L
from tests import test_gpu_wire_coded as W

pytestmark = pytest.mark.gpu

FILL = 0xCC
FILL32 = 0xCCCCCCCC
OK, EINVAL, ENOTREADY = 0, -1, -3
BAD_KINDS = ("empty", "coeffs_truncated", "other_coeff_len", "payload_too_long", "past_slot")

_r16, _P, _dev, _filled, _host = W._r16, W._P, W._dev, W._filled, W._host


# ---------------------------------------------------------------------------
# received frames in the payload-aligned layout
# ---------------------------------------------------------------------------
def make_frame(oracle, rng, k, Lb, fs, kind, plen, aligned=True):
    """-> (raw bytes written at frame_off, frame_len, frame_off, id).  Valid
    kinds: sys, any, zero_vec.  aligned: the payload at byte P of the slot,
    else the frame at byte 0."""
    P = _P(k)
    pay = rng.integers(0, 256, Lb + 1, dtype=np.uint8).tobytes()
    vec = rng.integers(0, 256, k, dtype=np.uint8).tobytes()
    pid = int(rng.integers(0, 1 << 40))
    coded = oracle.packet_to_raw(False, pay[:plen], vec)[1]
    off_c = P - 3 - k if aligned else 0
    off = off_c
    if kind == "sys":
        raw = oracle.packet_to_raw(True, pay[:plen])[1]
        flen, off = len(raw), (P - 1 if aligned else 0)
    elif kind == "any":
        raw, flen = coded, len(coded)
    elif kind == "zero_vec":
        raw = oracle.packet_to_raw(False, pay[:plen], bytes(k))[1]
        flen = len(raw)
    elif kind == "empty":
        raw, flen = b"", 0
    elif kind == "coeffs_truncated":
        raw, flen = coded[: 3 + k - 1], 3 + k - 1
    elif kind == "other_coeff_len":
        raw = oracle.packet_to_raw(False, pay[:plen], vec + b"\x07")[1]   # k + 1 coefficients
        flen = len(raw)
    elif kind == "payload_too_long":
        sys_ = bool(pid & 1)
        raw = oracle.packet_to_raw(sys_, pay[: Lb + 1], None if sys_ else vec)[1]
        flen, off = len(raw), ((P - 1 if aligned else 0) if sys_ else off_c)
    else:   # past_slot: frame_off + frame_len is one more than the slot holds
        assert kind == "past_slot"
        raw, flen = coded[: fs - off], fs - off + 1
    assert off + len(raw) <= fs
    return raw, flen, off, pid


class Received:
    """G generations of mr frame slots, fs bytes each: `kinds[g]` lists the
    frame kinds in arrival order, payload lengths cycle through `lens`."""

    def __init__(self, oracle, rng, k, Lb, mr, fs, kinds, lens, aligned=True):
        G = len(kinds)
        self.k, self.L, self.mr, self.fs, self.G = k, Lb, mr, fs, G
        self.frames = np.full((G, mr, fs), FILL, np.uint8)
        self.flen = np.zeros((G, mr), np.uint32)
        self.foff = np.zeros((G, mr), np.uint32)
        self.ids = np.zeros((G, mr), np.uint64)
        self.nfr = np.array([len(kd) for kd in kinds], np.uint32)
        self.meta = []
        c = 0
        for g, kd in enumerate(kinds):
            gen = []
            for s, kind in enumerate(kd):
                plen = lens[c % len(lens)]
                c += 1
                raw, fl, off, pid = make_frame(oracle, rng, k, Lb, fs, kind, plen, aligned)
                self.frames[g, s, off: off + len(raw)] = np.frombuffer(raw, np.uint8)
                self.flen[g, s], self.foff[g, s], self.ids[g, s] = fl, off, pid
                gen.append((raw, fl, off, pid, kind))
            self.meta.append(gen)

    def expected(self, oracle, need_aligned=True):
        """By the oracle's from_raw: statuses (G, mr; FILL32 where no frame),
        and per generation the compacted rows (n, L) zero padded, vectors
        (n, k), indices, lengths and offsets into the generation's region."""
        st = np.full((self.G, self.mr), FILL32, np.uint32).view(np.int32)
        gens = []
        k, Lb = self.k, self.L
        for g, gen in enumerate(self.meta):
            rows, vecs, idx, ln, ro = [], [], [], [], []
            for s, (raw, fl, off, pid, kind) in enumerate(gen):
                est, is_sys, vec, pay = W._expected_parse(oracle, raw, fl, off, self.fs, k, Lb)
                hdr = 1 if is_sys else 3 + k
                if est == OK and need_aligned and (off + hdr) % 16:
                    est = EINVAL
                st[g, s] = est
                if est != OK:
                    continue
                v = np.zeros(k, np.uint8)
                if is_sys:
                    v[pid % k] = 1
                else:
                    v[:] = np.frombuffer(vec, np.uint8)
                rows.append(np.frombuffer(pay.ljust(Lb, b"\0"), np.uint8))
                vecs.append(v)
                idx.append(pid % k if is_sys else k)
                ln.append(len(pay))
                ro.append(s * self.fs + off + hdr)
            n = len(rows)
            gens.append(dict(n=n, rows=np.array(rows, np.uint8).reshape(n, Lb), vecs=np.array(vecs, np.uint8).reshape(n, k),
                             idx=np.array(idx, np.uint16), len=np.array(ln, np.uint32), off=np.array(ro, np.uint32)))
        return st, gens


def run_headers(qf, rx, pass_n=True):
    """parse_frame_headers over rx -> dict of device tensors and host views."""
    G, mr, k = rx.G, rx.mr, rx.k
    d = dict(frames=_dev(rx.frames), flen=_dev(rx.flen), foff=_dev(rx.foff), ids=_dev(rx.ids), nfr=_dev(rx.nfr),
             idx=_filled(2 * G * mr + 16), n=_filled(4 * G + 16), st=_filled(4 * G * mr + 16),
             co=_filled(G * mr * k + 64), rl=_filled(4 * G * mr + 16), ro=_filled(4 * G * mr + 16))
    qf.parse_frame_headers(d["frames"], d["flen"], d["ids"], d["idx"], d["n"], d["st"], d["co"], d["rl"], d["ro"],
                           k, rx.L, max_rows=mr, frame_stride=rx.fs, G=G, n_frames=d["nfr"] if pass_n else None,
                           frame_off=d["foff"])
    qf.default_context().sync()
    assert np.array_equal(_host(d["frames"]), rx.frames.reshape(-1)), "the frames were written"
    return d


def run_coded(qf, rx, pass_n=True):
    """parse_frames_coded over the same frames (the yardstick's first call)."""
    G, mr, k = rx.G, rx.mr, rx.k
    rs = _r16(rx.L)
    d = dict(frames=_dev(rx.frames), rows=_filled(G * mr * rs), rs=rs,
             idx=_filled(2 * G * mr + 16), n=_filled(4 * G + 16), st=_filled(4 * G * mr + 16),
             co=_filled(G * mr * k + 64), rl=_filled(4 * G * mr + 16))
    qf.parse_frames_coded(d["frames"], _dev(rx.flen), _dev(rx.ids), d["rows"], d["idx"], d["n"], d["st"], d["co"],
                          k, rx.L, max_rows=mr, frame_stride=rx.fs, row_stride=rs, rows_gen_stride=mr * rs, G=G,
                          n_frames=_dev(rx.nfr) if pass_n else None, frame_off=_dev(rx.foff), row_len=d["rl"])
    qf.default_context().sync()
    return d


# ---------------------------------------------------------------------------
# header parser
# ---------------------------------------------------------------------------
def _kinds_mixed(rng, count):
    kinds = ("sys", "any", "zero_vec", "any", "sys") + BAD_KINDS
    out = [kinds[i % len(kinds)] for i in range(count)]
    rng.shuffle(out)
    return out


# (4, 8, 300): more slots than the block has threads, so the compaction loop runs a second round and its
# prefix crosses waves
HEADER_CASES = [(4, 8, 6), (13, 33, 9), (14, 17, 9), (16, 1, 5), (64, 1200, 20), (256, 16, 5), (4, 8, 300)]


@pytest.mark.parametrize("k,Lb,mr", HEADER_CASES)
def test_parse_frame_headers_parity(qf, oracle, gpu_ctx, k, Lb, mr):
    rng = np.random.default_rng(k * 131 + Lb)
    fs = _P(k) + _r16(Lb + 1) + 16
    lens = sorted({0, 1, 15, 16, 17, Lb} & set(range(Lb + 1)))
    # generation 1 holds fewer frames than slots; together the generations see every kind
    kinds = [_kinds_mixed(rng, mr), _kinds_mixed(rng, mr - 2), _kinds_mixed(rng, mr)]
    if mr < 10:
        kinds[0] = ["sys", "empty", "any", "zero_vec", "any", "sys", "any", "sys", "any"][:mr]
        kinds[2] = list(BAD_KINDS[: mr - 1]) + ["sys"]
    rx = Received(oracle, rng, k, Lb, mr, fs, kinds, lens)
    est, egens = rx.expected(oracle)
    assert {kd for g in kinds for kd in g} >= {"sys", "any", "zero_vec"} | set(BAD_KINDS[: min(mr - 1, 5)])
    h = run_headers(qf, rx)
    c = run_coded(qf, rx)
    G = rx.G
    # the coded parser's outputs on the same buffers, untouched bytes included
    for name, dt in (("idx", np.uint16), ("n", np.uint32), ("st", np.uint32), ("co", np.uint8), ("rl", np.uint32)):
        assert np.array_equal(_host(h[name], dt), _host(c[name], dt)), name
    st = _host(h["st"], np.int32)
    assert (st[G * mr:].view(np.uint32) == FILL32).all()
    assert np.array_equal(st[: G * mr].reshape(G, mr), est)
    idx = _host(h["idx"], np.uint16)[: G * mr].reshape(G, mr)
    co = _host(h["co"])[: G * mr * k].reshape(G, mr, k)
    rl = _host(h["rl"], np.uint32)[: G * mr].reshape(G, mr)
    ro = _host(h["ro"], np.uint32)
    assert (ro[G * mr:] == FILL32).all()
    ro = ro[: G * mr].reshape(G, mr)
    n = _host(h["n"], np.uint32)
    assert (n[G:] == FILL32).all()
    for g, e in enumerate(egens):
        assert n[g] == e["n"]
        assert np.array_equal(idx[g, : e["n"]], e["idx"]) and np.array_equal(co[g, : e["n"]], e["vecs"])
        assert np.array_equal(rl[g, : e["n"]], e["len"])
        assert np.array_equal(ro[g, : e["n"]], e["off"]), (g, ro[g], e["off"])
        assert (ro[g, : e["n"]] % 16 == 0).all()
        assert (ro[g, e["n"]:] == FILL32).all() and (rl[g, e["n"]:] == FILL32).all()
        assert (idx[g, e["n"]:] == 0xCCCC).all() and (co[g, e["n"]:] == FILL).all()
    assert 0 < egens[0]["n"] < mr


def test_parse_frame_headers_misaligned_payloads(qf, oracle, gpu_ctx):
    """Frames at byte 0 of their slots: payloads at byte 1 or 3 + k.  Every
    otherwise valid frame is QF_EINVAL and nothing is compacted; the malformed
    ones keep the coded parser's status."""
    k, Lb, mr = 4, 8, 12
    rng = np.random.default_rng(77)
    kinds = [_kinds_mixed(rng, mr) for _ in range(3)]
    rx = Received(oracle, rng, k, Lb, mr, 48, kinds, [0, 1, 8, 5], aligned=False)
    est, egens = rx.expected(oracle)
    h = run_headers(qf, rx)
    c = run_coded(qf, rx)
    st = _host(h["st"], np.int32)[: 3 * mr].reshape(3, mr)
    stc = _host(c["st"], np.int32)[: 3 * mr].reshape(3, mr)
    assert np.array_equal(st, est)
    n_valid = 0
    for g in range(3):
        for s, kind in enumerate(kinds[g]):
            if kind in ("sys", "any", "zero_vec"):
                assert stc[g, s] == OK and st[g, s] == EINVAL
                n_valid += 1
            else:
                assert st[g, s] == stc[g, s] != OK
    assert n_valid >= 12
    assert (_host(h["n"], np.uint32)[:3] == 0).all()
    assert (_host(c["n"], np.uint32)[:3] > 0).all()
    for name in ("idx", "co", "rl", "ro"):
        assert (_host(h[name]) == FILL).all(), name


def test_parse_frame_headers_call_level_errors(qf, gpu_ctx):
    import torch

    t = lambda n, dt=torch.uint8: torch.zeros(n, dtype=dt, device="cuda")   # noqa: E731
    frames, flen, ids = t(1024 * 64 + 16), t(1024, torch.int32), t(1024, torch.int64)
    idx, n, st, co = t(1024, torch.int16), t(4, torch.int32), t(1024, torch.int32), t(1024 * 256)
    rl, ro = t(1024, torch.int32), t(1024, torch.int32)
    lib, ctx = L._lib(), gpu_ctx.handle
    ptrs = dict(frames=frames, flen=flen, ids=ids, idx=idx, n=n, co=co, rl=rl, ro=ro, st=st)

    def status(k=8, Lb=32, G_=1, max_rows=8, fs=64, handle=ctx, null=(), shift=None):
        p = {nm: (None if nm in null else tt.data_ptr() + (8 if nm == shift else 0)) for nm, tt in ptrs.items()}
        return lib.qf_parse_frame_headers_dev(handle, k, Lb, G_, max_rows, p["frames"], fs, p["flen"], None, p["ids"],
                                              None, p["idx"], p["n"], p["co"], p["rl"], p["ro"], p["st"])

    E = L.QF_EINVAL
    assert status() == 0
    assert status(handle=None) == E
    assert status(k=0) == E and status(k=257) == E
    assert status(k=256, max_rows=4) == 0
    assert status(max_rows=0) == E and status(max_rows=1025) == E
    assert status(max_rows=1024) == 0
    assert status(Lb=0) == E
    for nm in ptrs:
        assert status(null=(nm,)) == E, nm                       # every one of them is required
    assert status(shift="frames") == E
    assert status(fs=72) == E
    assert status(fs=(1 << 32) // 8 + 16) == E                   # row_off would not fit 32 bits
    assert status(G_=0, null=tuple(ptrs)) == 0
    gpu_ctx.sync()


# ---------------------------------------------------------------------------
# recode from the frame slots
# ---------------------------------------------------------------------------
def run_recode_frames(qf, rx, h, m, *, seed=0, mix=None, out_rs=None, out_gap=0, pass_n=True, want_len=True,
                      row_off=None, row_len=None, n_rows=None, src_gen_stride=None):
    """recode_frames over the frame buffer of `h` (run_headers).  row_off /
    row_len / n_rows: host arrays that replace the parser's.  -> out (G, m, L),
    vectors (G, m, k), out_len (G, m), status (G,); the bytes the call must not
    write are checked here, and that the source is unchanged."""
    G, mr, k, Lb = rx.G, rx.mr, rx.k, rx.L
    out_rs = _r16(Lb) + 16 if out_rs is None else out_rs
    out_gs = m * out_rs + out_gap
    t_out, t_oc = _filled(G * out_gs + 64), _filled(G * m * k + 64)
    t_ol, t_st = _filled(4 * G * m + 16), _filled(4 * G + 16)
    t_ro = h["ro"] if row_off is None else _dev(row_off)
    t_rl = h["rl"] if row_len is None else _dev(row_len)
    t_n = h["n"] if n_rows is None else _dev(n_rows)
    t_mix = _dev(np.ascontiguousarray(mix, np.uint8)) if mix is not None else None
    qf.recode_frames(h["frames"], t_ro, t_rl, h["idx"], h["co"], t_out, t_oc, t_st, k, m, Lb, max_rows=mr,
                     src_gen_stride=mr * rx.fs if src_gen_stride is None else src_gen_stride, out_row_stride=out_rs,
                     out_gen_stride=out_gs, G=G, n_rows=t_n if pass_n else None, mix=t_mix, seed=seed,
                     out_len=t_ol if want_len else None)
    qf.default_context().sync()
    assert np.array_equal(_host(h["frames"]), rx.frames.reshape(-1)), "the source was written"
    out, oc, ol, st = _host(t_out), _host(t_oc), _host(t_ol, np.uint32), _host(t_st, np.int32)
    assert (out[G * out_gs:] == FILL).all() and (oc[G * m * k:] == FILL).all()
    assert (st[G:].view(np.uint32) == FILL32).all()
    if want_len:
        assert (ol[G * m:] == FILL32).all()
    else:
        assert (ol == FILL32).all()
    og = out[: G * out_gs].reshape(G, out_gs)
    assert (og[:, m * out_rs:] == FILL).all(), "bytes after a generation's last row were written"
    orow = og[:, : m * out_rs].reshape(G, m, out_rs)
    assert (orow[:, :, Lb:] == FILL).all(), "bytes between L and out_row_stride were written"
    return orow[:, :, :Lb].copy(), oc[: G * m * k].reshape(G, m, k).copy(), ol[: G * m].reshape(G, m).copy(), st[:G].copy()


def run_three_call(qf, rx, c, m, seed):
    """recode_batch over the coded parser's rows: the yardstick's payload."""
    G, mr, k, Lb = rx.G, rx.mr, rx.k, rx.L
    ors = _r16(Lb) + 16
    t_out, t_oc, t_st = _filled(G * m * ors), _filled(G * m * k), _filled(4 * G)
    qf.recode_batch(c["rows"], c["idx"], t_out, t_oc, t_st, k, m, Lb, max_rows=mr, row_stride=c["rs"],
                    rows_gen_stride=mr * c["rs"], out_row_stride=ors, out_gen_stride=m * ors, G=G, n_rows=c["n"],
                    row_coeffs=c["co"], seed=seed)
    qf.default_context().sync()
    return (_host(t_out).reshape(G, m, ors)[:, :, :Lb], _host(t_oc).reshape(G, m, k), _host(t_st, np.int32))


def seeded_mix(oracle, G, m, mr, seed):
    return oracle.fill_splitmix(G * m * mr, seed).reshape(G, m, mr)


def check_oracle(oracle, egens, M, got, m, k, Lb, gens=None, bad=()):
    """got against oracle.encode over the zero-padded rows and the vectors."""
    out, oc, ol, st = got
    for g in (range(len(egens)) if gens is None else gens):
        e = egens[g]
        if e["n"] == 0 or g in bad:
            assert st[g] == (EINVAL if g in bad else ENOTREADY), (g, st[g])
            assert not out[g].any() and not oc[g].any() and not ol[g].any(), g
            continue
        Mn = np.ascontiguousarray(M[g][:, : e["n"]])
        assert st[g] == OK, (g, st[g])
        assert np.array_equal(out[g], oracle.encode(np.ascontiguousarray(e["rows"]), m, Mn)), f"payload of generation {g}"
        assert np.array_equal(oc[g], oracle.encode(np.ascontiguousarray(e["vecs"]), m, Mn)), f"vectors of generation {g}"
        assert (ol[g] == e["len"].max()).all(), (g, ol[g], e["len"])


def both_ways(qf, oracle, rx, m, seed, gens=None, **kw):
    """parse_frame_headers -> recode_frames against the oracle and, bit for
    bit, against parse_frames_coded -> recode_batch on the device."""
    _, egens = rx.expected(oracle)
    h = run_headers(qf, rx)
    got = run_recode_frames(qf, rx, h, m, seed=seed, **kw)
    check_oracle(oracle, egens, seeded_mix(oracle, rx.G, m, rx.mr, seed), got, m, rx.k, rx.L, gens=gens)
    ref = run_three_call(qf, rx, run_coded(qf, rx), m, seed)
    assert np.array_equal(got[0], ref[0]), "payload differs from the three-call pipeline"
    assert np.array_equal(got[1], ref[1]), "vectors differ from the three-call pipeline"
    assert np.array_equal(got[3], ref[2]), "statuses differ from the three-call pipeline"
    return h, egens, got


def test_recode_frames_small_ragged_rows(qf, oracle, gpu_ctx):
    """Three units per row with a partial last one, waves that straddle many
    generations, every edge length, and malformed frames between the valid
    ones so that row_off jumps."""
    k, mr, Lb, G, m = 5, 7, 37, 300, 6
    rng = np.random.default_rng(537)
    kinds = []
    for g in range(G):
        kd = [("sys", "any", "zero_vec", "any")[int(x)] for x in rng.integers(0, 4, mr)]
        for s in rng.choice(mr, 2 + g % 2, replace=False):
            kd[s] = BAD_KINDS[int(rng.integers(0, len(BAD_KINDS)))]
        kinds.append(kd)
    rx = Received(oracle, rng, k, Lb, mr, _P(k) + 48, kinds, [0, 1, 15, 16, 17, 36, 37])
    gpu_ctx.sync()
    gpu_ctx.profile(True)
    h, egens, got = both_ways(qf, oracle, rx, m, seed=41)
    times = gpu_ctx.kernel_times()
    gpu_ctx.profile(False)
    assert times["k_parse_frame_headers"][0] == 1 and times["k_combine_rows_at"][0] == 1, times
    assert times["k_recode_prepare"][0] == 2 and times["k_parse_frames_coded"][0] == 1, times    # the yardstick's too
    ro = _host(h["ro"], np.uint32)[: G * mr].reshape(G, mr)
    jumps = sum(1 for g in range(G) if egens[g]["n"] > 1 and (np.diff(ro[g, : egens[g]["n"]].astype(np.int64)) != rx.fs).any())
    assert jumps > G // 2
    assert {int(x) for e in egens for x in e["len"]} == {0, 1, 15, 16, 17, 36, 37}


@pytest.mark.parametrize("m", [1, 16, 17, 64])
def test_recode_frames_m_sweep(qf, oracle, gpu_ctx, m):
    k, mr, Lb, G = 16, 20, 48, 5
    rng = np.random.default_rng(1600 + m)
    kinds = [[("sys", "any")[int(x)] for x in rng.integers(0, 2, mr)] for _ in range(G)]
    kinds[1][3] = "empty"
    kinds[3] = kinds[3][:11]                      # an odd row count below max_rows
    rx = Received(oracle, rng, k, Lb, mr, _P(k) + 64, kinds, [48, 48, 48, 33, 48, 16])
    gpu_ctx.sync()
    gpu_ctx.profile(True)
    both_ways(qf, oracle, rx, m, seed=m)
    times = gpu_ctx.kernel_times()
    gpu_ctx.profile(False)
    assert times["k_combine_rows_at"][0] == (m + 15) // 16, times
    assert times["k_recode_prepare"][0] == 2, times    # one per pipeline


def test_recode_frames_real_size(qf, oracle, gpu_ctx):
    """k = 64, 64 held rows, m = 16, L = 1,200 in 1,280-byte slots: full rows
    (the pipelined path; 75 units per row, so waves span two generations) and,
    in the first generations, short rows among them (the masked path)."""
    k, mr, Lb, G, m = 64, 64, 1200, 64, 16
    rng = np.random.default_rng(1200)
    kinds = [[("sys", "any")[int(x)] for x in rng.integers(0, 2, mr)] for _ in range(G)]
    assert _P(k) + Lb == 1280
    lens = [Lb] * (4 * mr) + [Lb] * (G - 4) * mr
    for i in range(0, 4 * mr, 5):
        lens[i] = (0, 1, 15, 16, 17, 1199)[(i // 5) % 6]
    rx = Received(oracle, rng, k, Lb, mr, 1280, kinds, lens)
    sample = [0, 1, 2, 3, 4, 5, 31, 62, 63]
    both_ways(qf, oracle, rx, m, seed=12, gens=sample)


@pytest.mark.parametrize("m", [3, 7, 12, 16])
def test_recode_frames_full_rows_uneven_counts(qf, oracle, gpu_ctx, m):
    """Every row full, so whole waves take the pipelined path, at each of its
    output widths (4, 8, 12, 16): an odd max_rows, waves of 16 generations
    whose row counts differ (1 .. max_rows, odd and even), and one empty
    generation, whose wave takes the masked path."""
    k, mr, Lb, G = 16, 21, 64, 40
    rng = np.random.default_rng(6400 + m)
    counts = [1 + (5 * g) % mr for g in range(G)]
    counts[0], counts[17], counts[39] = mr, 0, mr
    assert {c % 2 for c in counts} == {0, 1} and 1 in counts
    kinds = [[("sys", "any")[int(x)] for x in rng.integers(0, 2, c)] for c in counts]
    rx = Received(oracle, rng, k, Lb, mr, _P(k) + 64, kinds, [Lb])
    _, _, got = both_ways(qf, oracle, rx, m, seed=70 + m)
    assert list(got[3]) == [ENOTREADY if c == 0 else OK for c in counts]


@pytest.mark.parametrize("Lb,lens", [(200, [200, 200, 200, 77]), (208, [208])], ids=["ragged", "full"])
def test_recode_frames_small_batch(qf, oracle, gpu_ctx, Lb, lens):
    """G = 1: fewer wave-items than CUs runs the same kernel (one wave, with
    lanes past the last unit), on the masked and on the pipelined path."""
    k, mr, m = 16, 20, 5
    rng = np.random.default_rng(Lb)
    rx = Received(oracle, rng, k, Lb, mr, _P(k) + 208, [["sys", "any"] * 10], lens)
    both_ways(qf, oracle, rx, m, seed=3)


def test_recode_frames_row_counts_bad_rows_and_out_len(qf, oracle, gpu_ctx):
    """n_rows of 0 and above max_rows; a row_len of L + 1, a row_off of 8 and a
    row_off + row_len one past src_gen_stride, each in a generation of its
    own: that generation alone is QF_EINVAL (QF_ENOTREADY for n = 0) with zero
    outputs and out_len 0, and its neighbours are exact."""
    k, mr, Lb, G, m = 16, 20, 53, 9, 18
    rng = np.random.default_rng(53)
    kinds = [[("sys", "any")[int(x)] for x in rng.integers(0, 2, mr)] for _ in range(G)]
    kinds[1] = []                                 # the parser itself reports 0 rows
    rx = Received(oracle, rng, k, Lb, mr, _P(k) + 64, kinds, [53, 17, 0, 53, 16, 1, 40])
    _, egens = rx.expected(oracle)
    h = run_headers(qf, rx)
    ro = _host(h["ro"], np.uint32)[: G * mr].reshape(G, mr).copy()
    rl = _host(h["rl"], np.uint32)[: G * mr].reshape(G, mr).copy()
    n = _host(h["n"], np.uint32)[:G].copy()
    assert list(n) == [mr, 0] + [mr] * (G - 2)
    n[3] = mr + 1
    rl[5, 4] = Lb + 1
    ro[6, 19] += 8
    assert ro[6, 19] % 16 == 8
    ro[7, 19], rl[7, 19] = mr * rx.fs - 16, 17
    rl[8, 2] = 0                                  # legal: the row contributes its vector only
    egens[8]["rows"][2] = 0
    egens[8]["len"][2] = 0
    n[2] = 7                                      # fewer rows than the parser found
    for key in ("rows", "vecs", "len"):
        egens[2][key] = egens[2][key][:7]
    egens[2]["n"] = 7
    got = run_recode_frames(qf, rx, h, m, seed=9, row_off=ro, row_len=rl, n_rows=n)
    assert list(got[3]) == [OK, ENOTREADY, OK, EINVAL, OK, EINVAL, EINVAL, EINVAL, OK]
    check_oracle(oracle, egens, seeded_mix(oracle, G, m, mr, 9), got, m, k, Lb, bad=(3, 5, 6, 7))
    # out_len is optional
    again = run_recode_frames(qf, rx, h, m, seed=9, row_off=ro, row_len=rl, n_rows=n, want_len=False)
    assert np.array_equal(again[0], got[0]) and np.array_equal(again[3], got[3])


def test_recode_frames_explicit_mix_wide_strides_and_null_n_rows(qf, oracle, gpu_ctx):
    k, mr, Lb, G, m = 8, 9, 33, 3, 17
    rng = np.random.default_rng(8)
    kinds = [[("sys", "any")[int(x)] for x in rng.integers(0, 2, mr)] for _ in range(G)]
    rx = Received(oracle, rng, k, Lb, mr, _P(k) + 48, kinds, [33, 1, 16, 17, 32, 0])
    _, egens = rx.expected(oracle)
    h = run_headers(qf, rx, pass_n=False)
    M = seeded_mix(oracle, G, m, mr, 77)
    # rows 48 bytes apart from their end and 80 bytes between generations
    seeded = run_recode_frames(qf, rx, h, m, seed=77, out_rs=96, out_gap=80)
    explicit = run_recode_frames(qf, rx, h, m, mix=M, seed=123, out_rs=96, out_gap=80)    # the seed is ignored
    no_n = run_recode_frames(qf, rx, h, m, seed=77, pass_n=False)                         # NULL n_rows: max_rows
    for a, b, c in zip(seeded, explicit, no_n):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    check_oracle(oracle, egens, M, seeded, m, k, Lb)


def test_recode_frames_call_level_errors(qf, gpu_ctx):
    import torch

    t = lambda n, dt=torch.uint8: torch.zeros(n, dtype=dt, device="cuda")   # noqa: E731
    src, ro, rl, idx, co = t(8 * 64 + 16), t(8, torch.int32), t(8, torch.int32), t(8, torch.int16), t(8 * 255)
    out, oc, ol, st = t(65 * 48 + 16), t(65 * 256), t(65, torch.int32), t(1, torch.int32)
    rl += 32
    lib, ctx = L._lib(), gpu_ctx.handle
    ptrs = dict(src=src, ro=ro, rl=rl, idx=idx, co=co, out=out, oc=oc, st=st)

    def status(k=8, m=4, Lb=32, max_rows=8, flags=0, reserved=0, sgs=8 * 64, ors=48, ogs=64 * 48, G_=1, handle=ctx,
               shape=True, null=(), shift=None):
        sh = L.RecodeFramesShape(k, Lb, max_rows, m, flags, reserved, sgs, ors, ogs)
        p = {nm: (None if nm in null else tt.data_ptr() + (8 if nm == shift else 0)) for nm, tt in ptrs.items()}
        return lib.qf_recode_frames_dev(handle, ctypes.byref(sh) if shape else None, G_, p["src"], p["ro"], p["rl"],
                                        p["idx"], None, p["co"], None, 5, p["out"], p["oc"], ol.data_ptr(), p["st"])

    E = L.QF_EINVAL
    assert status() == 0
    assert status(handle=None) == E and status(shape=False) == E
    assert status(m=65) == E and status(m=0) == E
    assert status(k=256) == E and status(k=0) == E
    assert status(max_rows=0) == E and status(max_rows=256) == E
    assert status(Lb=0) == E
    assert status(flags=1) == E and status(reserved=1) == E
    assert status(Lb=64, ors=48) == E                   # a stride shorter than L
    assert status(ors=40) == E and status(ogs=64 * 48 + 8) == E and status(sgs=8 * 64 + 8) == E
    assert status(shift="src") == E and status(shift="out") == E
    for nm in ptrs:
        assert status(null=(nm,)) == E, nm              # every one of them is required
    assert status(G_=0, null=tuple(ptrs)) == 0
    gpu_ctx.sync()
    assert st.cpu().numpy()[0] == OK


# ---------------------------------------------------------------------------
# one hop in place, then a receiver
# ---------------------------------------------------------------------------
def test_relay_in_place_round_trip(qf, oracle, gpu_ctx):
    """Relay: parse_frame_headers -> recode_frames into the output frame slots
    -> frame_rows in place with out_len.  Receiver: parse_frames_coded ->
    decode_innovative_batch recovers the sources."""
    import torch

    k, r, Lb, G, m = 8, 4, 40, 4, 10
    rng = np.random.default_rng(909)
    P = _P(k)
    rs = _r16(Lb)
    fs = P + rs
    src = rng.integers(0, 256, (G, k, Lb), dtype=np.uint8)
    rep = np.stack([oracle.encode(src[g], r) for g in range(G)])
    C = oracle.cauchy(k, r)
    n_held = k + r - 2
    rx = Received(oracle, rng, k, Lb, n_held, fs, [[] for _ in range(G)], [Lb])
    X, V = [], []
    for g in range(G):
        lost = set(rng.choice(k, 2, replace=False).tolist())
        arr = [i for i in range(k + r) if i not in lost]
        rng.shuffle(arr)
        for s, i in enumerate(arr):
            raw = oracle.packet_to_raw(i < k, (src[g, i] if i < k else rep[g, i - k]).tobytes(),
                                       None if i < k else C[i - k].tobytes())[1]
            off = P - 1 if i < k else P - 3 - k
            rx.frames[g, s, off: off + len(raw)] = np.frombuffer(raw, np.uint8)
            rx.flen[g, s], rx.foff[g, s], rx.ids[g, s] = len(raw), off, (5 * k + i if i < k else 1000 + i)
        rx.nfr[g] = n_held
        X.append(np.stack([src[g, i] if i < k else rep[g, i - k] for i in arr]))
        V.append(np.stack([np.eye(k, dtype=np.uint8)[i] if i < k else C[i - k] for i in arr]))
    # the seed, chosen on the CPU: the oracle decodes every generation from its first k recoded rows
    seed = None
    for cand in range(1, 50):
        M = seeded_mix(oracle, G, m, n_held, cand)
        if all(oracle.decode(k, k + np.arange(m), oracle.encode(X[g], m, np.ascontiguousarray(M[g])),
                             oracle.encode(V[g], m, np.ascontiguousarray(M[g])))[0] == OK for g in range(G)):
            seed = cand
            break
    assert seed is not None, "no seed decodes every generation"
    M = seeded_mix(oracle, G, m, n_held, seed)

    h = run_headers(qf, rx)
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
    assert (_host(t_st, np.int32) == OK).all() and (_host(t_ol, np.uint32) == Lb).all()
    out = _host(t_out).reshape(G, m, fs)
    olen, ooff = _host(t_flen, np.uint32).reshape(G, m), _host(t_foff, np.uint32).reshape(G, m)
    assert (olen == 3 + k + Lb).all() and (ooff == P - 3 - k).all()
    for g in range(G):
        epay = oracle.encode(X[g], m, np.ascontiguousarray(M[g]))
        evec = oracle.encode(V[g], m, np.ascontiguousarray(M[g]))
        for j in range(m):
            want = oracle.packet_to_raw(False, epay[j].tobytes(), evec[j].tobytes())[1]
            o = int(ooff[g, j])
            assert out[g, j, o: o + olen[g, j]].tobytes() == want, (g, j)
            assert (out[g, j, :o] == FILL).all() and (out[g, j, o + olen[g, j]:] == FILL).all()

    # receiver: the relay's frames alone
    ids = np.broadcast_to(7000 + np.arange(m, dtype=np.uint64), (G, m)).copy()
    d_rows, d_idx, d_n = _filled(G * m * rs), _filled(2 * G * m), _filled(4 * G)
    d_st, d_co = _filled(4 * G * m), _filled(G * m * k)
    qf.parse_frames_coded(t_out, t_flen, _dev(ids), d_rows, d_idx, d_n, d_st, d_co, k, Lb, max_rows=m,
                          frame_stride=fs, row_stride=rs, rows_gen_stride=m * rs, G=G, frame_off=t_foff)
    gpu_ctx.sync()
    assert (_host(d_st, np.int32) == OK).all() and (_host(d_n, np.uint32) == m).all()
    z = lambda n, dt=torch.uint8: torch.zeros(n, dtype=dt, device="cuda")   # noqa: E731
    rec, ri = z(G * k * rs), z(G * k, torch.int16)
    nrec, st, rank = z(G, torch.int32), _filled(4 * G), z(G, torch.int32)
    qf.decode_innovative_batch(d_rows, d_idx.view(torch.int16), rec, ri, nrec, st.view(torch.int32), k, k, Lb,
                               max_rows=m, row_stride=rs, rows_gen_stride=m * rs, rec_row_stride=rs,
                               rec_gen_stride=k * rs, G=G, n_rows=d_n.view(torch.int32), row_coeffs=d_co, rank=rank)
    gpu_ctx.sync()
    assert (_host(st, np.int32) == OK).all(), _host(st, np.int32)
    assert (rank.cpu().numpy() == k).all() and (nrec.cpu().numpy() == k).all()
    recv = rec.cpu().numpy().reshape(G, k, rs)
    rix = ri.cpu().numpy().view(np.uint16).reshape(G, k)
    for g in range(G):
        assert sorted(rix[g].tolist()) == list(range(k))
        for j in range(k):
            assert np.array_equal(recv[g, j, :Lb], src[g, rix[g, j]]), (g, j)
