"""Device framing of coded rows that carry their coefficient vectors
(qf_frame_rows_dev, qf_parse_frames_coded_dev) on the MI355X, byte for byte
against the oracle's restatement of Packet::to_raw / from_raw
(oracle/qf_oracle_wire.c): frames in the payload-aligned layout in copy mode
and in place, parse statuses, rows and vectors for systematic, Cauchy,
arbitrary-vector and malformed frames at slot offsets 0 and 0..15, and a relay
step (parse -> recode into the frame slots -> in-place framing) whose frames a
receiver parses and decodes with the rank-aware decode.  Every output buffer
starts as 0xCC, and every byte the calls must not write is checked to still
be 0xCC."""
import ctypes

import numpy as np
import pytest

from quicfuscate_amd import _lib as L

pytestmark = pytest.mark.gpu

FILL = 0xCC
FILL32 = 0xCCCCCCCC
G = 3


def _r16(x):
    return (x + 15) // 16 * 16


def _P(k):
    return (3 + k + 15) // 16 * 16


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()


def _filled(nbytes):
    import torch

    return torch.full((nbytes,), FILL, dtype=torch.uint8, device="cuda")


def _host(t, dtype=np.uint8):
    return t.cpu().numpy().view(dtype)


# ---------------------------------------------------------------------------
# frame_rows
# ---------------------------------------------------------------------------
class RowSet:
    """Rows a node holds, G generations of max_rows slots: systematic and coded
    slots mixed, random vectors with one all-zero vector, n_rows per generation
    with one of them 0, row lengths among {0, 1, 15, 16, 17, L} and one L + 1."""

    def __init__(self, k, Lb, mr, seed):
        rng = np.random.default_rng(seed)
        self.k, self.L, self.mr = k, Lb, mr
        self.rows = rng.integers(0, 256, (G, mr, Lb + 1), dtype=np.uint8)   # one byte more: the L + 1 slot
        coded = rng.random((G, mr)) < 0.5
        coded[:, 0], coded[:, 1] = False, True                              # both kinds in every generation
        self.idx = np.where(coded, k + rng.integers(0, 40, (G, mr)), rng.integers(0, k, (G, mr))).astype(np.uint16)
        self.coeffs = rng.integers(0, 256, (G, mr, k), dtype=np.uint8)
        self.coeffs[0, 1] = 0                                               # an all-zero vector is a legal row
        self.n = np.array([mr, 0, mr - 1], np.uint32)
        lens = sorted({0, 1, 15, 16, 17, Lb} & set(range(Lb + 1)))
        self.len = np.array([lens[i % len(lens)] for i in range(G * mr)], np.uint32).reshape(G, mr)
        self.len[0, 1] = Lb                                                 # the zero vector with a full payload
        self.len[2, 0] = Lb + 1                                             # too long: no frame
        self.len[2, 1] = 17 if Lb >= 17 else Lb


def _expected_frames(oracle, rs_, init, fs, vectors):
    """-> (frame buffer (G, mr, fs), frame_len (G, mr), frame_off (G, mr)) the
    call must leave, from `init` (what the buffer held before) and the oracle's
    to_raw bytes of every valid slot."""
    k, Lb, mr = rs_.k, rs_.L, rs_.mr
    P = _P(k)
    exp = init.copy()
    flen = np.zeros((G, mr), np.uint32)
    foff = np.zeros((G, mr), np.uint32)
    for g in range(G):
        for s in range(mr):
            rl, i = int(rs_.len[g, s]), int(rs_.idx[g, s])
            if s >= rs_.n[g] or rl > Lb:
                continue
            vec = None if i < k else vectors(g, s, i)
            if i >= k and vec is None:
                continue
            st, raw = oracle.packet_to_raw(i < k, rs_.rows[g, s, :rl].tobytes(), vec)
            assert st == 0
            off = P - 1 if i < k else P - 3 - k
            assert len(raw) == P - off + rl
            exp[g, s, off: off + len(raw)] = np.frombuffer(raw, np.uint8)
            flen[g, s], foff[g, s] = len(raw), off
    return exp, flen, foff


def _run_frame_rows(qf, rs_, fs, *, in_place, r=0, coeffs=True, pass_off=True):
    """-> (init, frames (G, mr, fs), frame_len, frame_off).  In place the test
    itself puts every payload at byte P of its slot and passes no rows."""
    k, Lb, mr = rs_.k, rs_.L, rs_.mr
    P = _P(k)
    stride = _r16(Lb) + 16
    rows = np.full((G, mr, stride), 0x3C, np.uint8)      # bytes past L of a row must not reach a frame
    rows[:, :, :Lb] = rs_.rows[:, :, :Lb]
    init = np.full((G, mr, fs), FILL, np.uint8)
    if in_place:
        for g in range(G):
            for s in range(mr):
                rl = min(int(rs_.len[g, s]), Lb)
                init[g, s, P: P + rl] = rs_.rows[g, s, :rl]
    tail = 64
    t_frames = _dev(np.concatenate([init.reshape(-1), np.full(tail, FILL, np.uint8)]))
    t_len, t_off = _filled(4 * G * mr + 16), _filled(4 * G * mr + 16)
    qf.frame_rows(None if in_place else _dev(rows), t_frames, t_len, k, Lb, r=r, max_rows=mr, row_stride=stride,
                  rows_gen_stride=mr * stride, frame_stride=fs, G=G, row_index=_dev(rs_.idx), n_rows=_dev(rs_.n),
                  row_coeffs=_dev(rs_.coeffs) if coeffs else None, row_len=_dev(rs_.len),
                  frame_off=t_off if pass_off else None, in_place=in_place)
    qf.default_context().sync()
    fr = _host(t_frames)
    assert (fr[G * mr * fs:] == FILL).all(), "bytes behind the last slot were written"
    fl, fo = _host(t_len, np.uint32), _host(t_off, np.uint32)
    assert (fl[G * mr:] == FILL32).all() and (fo[G * mr:] == FILL32).all()
    return init, fr[: G * mr * fs].reshape(G, mr, fs), fl[: G * mr].reshape(G, mr), fo[: G * mr].reshape(G, mr)


FRAME_CASES = [
    (4, 8, 6),
    (64, 1200, 20),
    (13, 33, 9),      # 3 + k = 16: a coded frame starts at slot byte 0
    (14, 17, 9),      # P jumps to 32
    (16, 1, 5),
    (256, 16, 5),
]


@pytest.mark.parametrize("in_place", [False, True], ids=["copy", "in_place"])
@pytest.mark.parametrize("k,Lb,mr", FRAME_CASES)
def test_frame_rows_parity(qf, oracle, gpu_ctx, k, Lb, mr, in_place):
    rs_ = RowSet(k, Lb, mr, seed=k * 7 + Lb)
    P = _P(k)
    assert L._lib().qf_frame_payload_offset(k) == P
    fs = P + _r16(Lb) + 16
    init, frames, flen, foff = _run_frame_rows(qf, rs_, fs, in_place=in_place)
    exp, elen, eoff = _expected_frames(oracle, rs_, init, fs, lambda g, s, i: rs_.coeffs[g, s].tobytes())
    assert np.array_equal(flen, elen)
    assert np.array_equal(foff, eoff)
    assert (flen[1] == 0).all() and flen[2, 0] == 0 and flen[2, mr - 1] == 0      # n = 0, L + 1, s >= n
    assert flen[0, 1] == 3 + k + Lb and not frames[0, 1, P - k: P].any()           # the zero vector's frame
    # every valid frame equals the oracle's to_raw bytes, and every other byte of
    # the buffer is what it was (0xCC; in place also the payloads the test put there)
    bad = np.argwhere(frames != exp)
    assert bad.size == 0, f"first differing byte (g, slot, byte): {bad[0]}"
    if not in_place:
        for g in range(G):
            for s in range(mr):
                o, n = int(foff[g, s]), int(flen[g, s])
                assert (frames[g, s, :o] == FILL).all() and (frames[g, s, o + n:] == FILL).all()


def test_frame_rows_without_frame_off_output(qf, oracle, gpu_ctx):
    rs_ = RowSet(13, 33, 9, seed=5)
    fs = _P(13) + 64
    init, frames, flen, foff = _run_frame_rows(qf, rs_, fs, in_place=False, pass_off=False)
    exp, elen, _ = _expected_frames(oracle, rs_, init, fs, lambda g, s, i: rs_.coeffs[g, s].tobytes())
    assert np.array_equal(flen, elen) and np.array_equal(frames, exp)
    assert (foff == FILL32).all()


@pytest.mark.parametrize("in_place", [False, True], ids=["copy", "in_place"])
def test_frame_rows_cauchy_headers_without_row_coeffs(qf, oracle, gpu_ctx, in_place):
    """NULL row_coeffs and r > 0: index k + j carries Cauchy row j of (k, r),
    and an index with j >= r gives no frame."""
    k, r, Lb, mr = 12, 5, 24, 10
    rs_ = RowSet(k, Lb, mr, seed=3)
    for g in range(G):
        rs_.idx[g, 1: 1 + r] = k + np.arange(r)       # every Cauchy row once
        rs_.idx[g, 6] = k + r                         # the first index without a row
        rs_.idx[g, 7] = k + r + 30
    rs_.len[0, 6] = rs_.len[0, 7] = Lb
    C = oracle.cauchy(k, r)
    fs = _P(k) + _r16(Lb) + 16
    init, frames, flen, foff = _run_frame_rows(qf, rs_, fs, in_place=in_place, r=r, coeffs=False)
    exp, elen, eoff = _expected_frames(oracle, rs_, init, fs,
                                       lambda g, s, i: C[i - k].tobytes() if i - k < r else None)
    assert np.array_equal(flen, elen) and np.array_equal(foff, eoff)
    assert flen[0, 6] == 0 and flen[0, 7] == 0 and (flen[0, 1: 1 + r] > 0).all()
    bad = np.argwhere(frames != exp)
    assert bad.size == 0, f"first differing byte (g, slot, byte): {bad[0]}"


# ---------------------------------------------------------------------------
# parse_frames_coded
# ---------------------------------------------------------------------------
KINDS = ("sys", "cauchy", "any", "zero_vec", "empty", "no_coeff_len", "coeffs_truncated", "other_coeff_len",
         "payload_too_long", "past_slot")


def _make_frames(oracle, rng, k, Lb, count, r, fs, offsets):
    """`count` received frames of one generation, the kinds of KINDS cycled in
    a random order: [(raw bytes, frame_len, frame_off, id, kind)].  Payload
    lengths cycle through the edges of the copy loops."""
    lens = sorted({0, 1, 15, 16, 17, 19, 20, 21, 35, 36, Lb} & set(range(Lb + 1)))
    C = oracle.cauchy(k, r) if r else None
    kinds = [KINDS[i % len(KINDS)] for i in range(count)]
    rng.shuffle(kinds)
    out = []
    for n, kind in enumerate(kinds):
        if kind == "cauchy" and not r:
            kind = "any"
        pl = lens[int(rng.integers(0, len(lens)))] if n >= len(lens) * 3 else lens[n % len(lens)]
        pay = rng.integers(0, 256, Lb + 1, dtype=np.uint8).tobytes()
        vec = rng.integers(0, 256, k, dtype=np.uint8)
        while C is not None and any(np.array_equal(vec, C[j]) for j in range(r)):
            vec = rng.integers(0, 256, k, dtype=np.uint8)
        pid = int(rng.integers(0, 1 << 40))
        off = int(rng.integers(0, 16)) if offsets else 0
        coded = oracle.packet_to_raw(False, pay[:pl], vec.tobytes())[1]
        if kind == "sys":
            raw = oracle.packet_to_raw(True, pay[:pl])[1]
            flen = len(raw)
        elif kind == "cauchy":
            raw = oracle.packet_to_raw(False, pay[:pl], C[int(rng.integers(0, r))].tobytes())[1]
            flen = len(raw)
        elif kind == "any":
            raw, flen = coded, len(coded)
        elif kind == "zero_vec":
            raw = oracle.packet_to_raw(False, pay[:pl], bytes(k))[1]
            flen = len(raw)
        elif kind == "empty":
            raw, flen = coded, 0
        elif kind == "no_coeff_len":
            raw, flen = coded, 2
        elif kind == "coeffs_truncated":
            raw, flen = coded, 3 + k - 1
        elif kind == "other_coeff_len":
            raw = oracle.packet_to_raw(False, pay[:pl], bytes(vec.tobytes()) + b"\x07")[1]   # k + 1 coefficients
            flen = len(raw)
        elif kind == "payload_too_long":
            raw = oracle.packet_to_raw(bool(n & 1), pay[: Lb + 1], None if n & 1 else vec.tobytes())[1]
            flen = len(raw)
        else:   # past_slot: frame_off + frame_len is one more than the slot holds
            raw, flen = coded[: fs - off], fs - off + 1
        assert off + len(raw) <= fs
        out.append((raw, flen, off, pid, kind))
    return out


def _expected_parse(oracle, raw, flen, off, fs, k, Lb):
    """-> (status, is_systematic, vector, payload) by the rule of the call:
    Packet::from_raw's errors, then the coefficient length, then the payload
    length; a frame that is empty or does not end inside its slot first."""
    if flen == 0 or off + flen > fs:
        return L.QF_EINVAL, None, None, None
    st, is_sys, co, pay = oracle.packet_from_raw(raw[:flen], block_size=1 << 20)
    if st:
        assert st in (oracle.FR_NO_COEFF_LEN, oracle.FR_COEFF_TRUNCATED)
        return L.QF_ETOOSMALL, None, None, None
    if not is_sys and len(co) != k:
        return L.QF_ERANGE, None, None, None
    if len(pay) > Lb:
        return L.QF_EINVAL, None, None, None
    return L.QF_OK, is_sys, co, pay


def _run_parse(qf, gens, k, Lb, mr, fs, offsets, pass_n=True, pass_len=True):
    """gens: per generation the list of _make_frames.  -> dict of host arrays."""
    rs = _r16(Lb) + 16
    fr = np.full((G, mr, fs), 0x5A, np.uint8)
    flen = np.zeros((G, mr), np.uint32)
    foff = np.zeros((G, mr), np.uint32)
    ids = np.zeros((G, mr), np.uint64)
    for g, frames in enumerate(gens):
        for s, (raw, ln, off, pid, _) in enumerate(frames):
            fr[g, s, off: off + len(raw)] = np.frombuffer(raw, np.uint8)
            flen[g, s], foff[g, s], ids[g, s] = ln, off, pid
    nfr = np.array([len(f) for f in gens], np.uint32)
    t_rows, t_idx, t_n = _filled(G * mr * rs + 64), _filled(2 * G * mr + 16), _filled(4 * G + 16)
    t_st, t_co, t_rl = _filled(4 * G * mr + 16), _filled(G * mr * k + 64), _filled(4 * G * mr + 16)
    qf.parse_frames_coded(_dev(fr), _dev(flen), _dev(ids), t_rows, t_idx, t_n, t_st, t_co, k, Lb, max_rows=mr,
                          frame_stride=fs, row_stride=rs, rows_gen_stride=mr * rs, G=G,
                          n_frames=_dev(nfr) if pass_n else None, frame_off=_dev(foff) if offsets else None,
                          row_len=t_rl if pass_len else None)
    qf.default_context().sync()
    rows, idx, n = _host(t_rows), _host(t_idx, np.uint16), _host(t_n, np.uint32)
    st, co, rl = _host(t_st, np.uint32), _host(t_co), _host(t_rl, np.uint32)
    assert (rows[G * mr * rs:] == FILL).all() and (idx[G * mr:] == 0xCCCC).all() and (n[G:] == FILL32).all()
    assert (st[G * mr:] == FILL32).all() and (co[G * mr * k:] == FILL).all() and (rl[G * mr:] == FILL32).all()
    return dict(rows=rows[: G * mr * rs].reshape(G, mr, rs), idx=idx[: G * mr].reshape(G, mr), n=n[:G],
                st=st[: G * mr].view(np.int32).reshape(G, mr), co=co[: G * mr * k].reshape(G, mr, k),
                rl=rl[: G * mr].reshape(G, mr))


def _check_parse(oracle, gens, got, k, Lb, mr, fs, with_len=True):
    for g, frames in enumerate(gens):
        slot = 0
        for s, (raw, ln, off, pid, kind) in enumerate(frames):
            est, is_sys, vec, pay = _expected_parse(oracle, raw, ln, off, fs, k, Lb)
            assert got["st"][g, s] == est, (g, s, kind, got["st"][g, s], est)
            if est != L.QF_OK:
                continue
            assert kind in ("sys", "cauchy", "any", "zero_vec"), kind
            row = got["rows"][g, slot]
            assert row[:Lb].tobytes() == pay.ljust(Lb, b"\0"), (g, s, kind, len(pay))
            assert (row[Lb:] == FILL).all(), "bytes between L and the row stride were written"
            if is_sys:
                want_vec = np.zeros(k, np.uint8)
                want_vec[pid % k] = 1
                assert got["idx"][g, slot] == pid % k
            else:
                want_vec = np.frombuffer(vec, np.uint8)
                assert got["idx"][g, slot] == k
            assert np.array_equal(got["co"][g, slot], want_vec), (g, s, kind)
            if with_len:
                assert got["rl"][g, slot] == len(pay)
            slot += 1
        assert got["n"][g] == slot
        # statuses of slots that hold no frame, and output slots >= n_rows, are untouched
        assert (got["st"][g, len(frames):].view(np.uint32) == FILL32).all()
        assert (got["rows"][g, slot:] == FILL).all() and (got["idx"][g, slot:] == 0xCCCC).all()
        assert (got["co"][g, slot:] == FILL).all() and (got["rl"][g, slot:] == FILL32).all()


# k, L, max_rows
PARSE_CASES = [
    (4, 8, 40),
    (64, 1200, 40),
    (13, 33, 40),
    (14, 17, 40),
    (16, 1, 40),
    (256, 16, 40),
    (4, 8, 300),      # more slots than the block's 256 threads: the slot loop and the cross-wave prefix
    (64, 64, 60),     # payload lengths 0, 19, 20, 21, 35, 36, 64: around the 16-byte fast path's guard
]


@pytest.mark.parametrize("offsets", [False, True], ids=["off0", "off0to15"])
@pytest.mark.parametrize("k,Lb,mr", PARSE_CASES)
def test_parse_frames_coded_parity(qf, oracle, gpu_ctx, k, Lb, mr, offsets):
    rng = np.random.default_rng(k * 31 + Lb + mr)
    r = min(4, 256 - k)
    fs = _r16(15 + 3 + k + 1 + Lb + 1)
    if mr == 300:     # n_frames NULL: every slot holds a frame
        gens = [_make_frames(oracle, rng, k, Lb, mr, r, fs, offsets) for _ in range(G)]
    else:
        gens = [_make_frames(oracle, rng, k, Lb, mr, r, fs, offsets), [],
                _make_frames(oracle, rng, k, Lb, mr - 3, r, fs, offsets)]
    seen = {(kind, len(raw)) for f in gens for (raw, _, _, _, kind) in f}
    assert {kd for kd, _ in seen} >= set(KINDS) - ({"cauchy"} if not r else set())
    got = _run_parse(qf, gens, k, Lb, mr, fs, offsets, pass_n=(mr != 300))
    _check_parse(oracle, gens, got, k, Lb, mr, fs)
    valid = sum(1 for (_, _, _, _, kind) in gens[0] if kind in ("sys", "cauchy", "any", "zero_vec"))
    assert got["n"][0] == valid and 0 < valid < len(gens[0])
    if mr != 300:
        assert got["n"][1] == 0


def test_parse_frames_coded_without_row_len_output(qf, oracle, gpu_ctx):
    k, Lb, mr = 13, 33, 40
    rng = np.random.default_rng(9)
    fs = _r16(15 + 3 + k + 1 + Lb + 1)
    gens = [_make_frames(oracle, rng, k, Lb, mr, 4, fs, True) for _ in range(G)]
    got = _run_parse(qf, gens, k, Lb, mr, fs, True, pass_len=False)
    assert (got["rl"] == FILL32).all()
    _check_parse(oracle, gens, got, k, Lb, mr, fs, with_len=False)


def test_cauchy_only_parser_rejects_arbitrary_vectors(qf, oracle, gpu_ctx):
    """The contrast this call exists for: qf_parse_frames_dev gives QF_ERANGE
    for a frame whose vector is not a Cauchy row (existing behaviour), the
    coded call accepts it."""
    k, r, Lb, mr = 4, 4, 8, 40
    rng = np.random.default_rng(44)
    fs = _r16(15 + 3 + k + 1 + Lb + 1)
    gens = [_make_frames(oracle, rng, k, Lb, mr, r, fs, False) for _ in range(G)]
    got = _run_parse(qf, gens, k, Lb, mr, fs, False)
    fr = np.full((G, mr, fs), 0x5A, np.uint8)
    flen = np.zeros((G, mr), np.uint32)
    ids = np.zeros((G, mr), np.uint64)
    for g, frames in enumerate(gens):
        for s, (raw, ln, off, pid, _) in enumerate(frames):
            fr[g, s, : len(raw)] = np.frombuffer(raw, np.uint8)
            flen[g, s], ids[g, s] = ln, pid
    rs = _r16(Lb)
    t_rows, t_idx, t_n, t_st = _filled(G * mr * rs), _filled(2 * G * mr), _filled(4 * G), _filled(4 * G * mr)
    t_fr, t_flen, t_ids = _dev(fr), _dev(flen), _dev(ids)
    L.check(L._lib().qf_parse_frames_dev(gpu_ctx.handle, k, r, Lb, G, mr, t_fr.data_ptr(), fs, t_flen.data_ptr(),
                                         t_ids.data_ptr(), None, t_rows.data_ptr(), rs, mr * rs, t_idx.data_ptr(),
                                         t_n.data_ptr(), t_st.data_ptr()), "parse")
    gpu_ctx.sync()
    old = _host(t_st, np.int32).reshape(G, mr)
    n_any = 0
    for g, frames in enumerate(gens):
        for s, (_, _, _, _, kind) in enumerate(frames):
            if kind in ("any", "zero_vec"):
                assert old[g, s] == L.QF_ERANGE and got["st"][g, s] == L.QF_OK
                n_any += 1
            elif kind in ("sys", "cauchy"):
                assert old[g, s] == L.QF_OK and got["st"][g, s] == L.QF_OK
    assert n_any >= 2 * G


# ---------------------------------------------------------------------------
# call-level errors, profile labels
# ---------------------------------------------------------------------------
def test_frame_rows_call_level_errors(qf, gpu_ctx):
    import torch

    t = lambda n, dt=torch.uint8: torch.zeros(n, dtype=dt, device="cuda")   # noqa: E731
    rows, frames, flen, co = t(1024 * 48 + 16), t(1024 * 80 + 16), t(1024, torch.int32), t(1024 * 256)
    lib, ctx = L._lib(), gpu_ctx.handle

    def status(k=8, r=0, Lb=32, max_rows=8, flags=0, reserved=0, rs=48, rgs=None, fs=64, G_=1, rows_p="d",
               frames_p="d", flen_p="d", coeffs=None, shape=True, handle=ctx):
        sh = L.FrameRowsShape(k, r, Lb, max_rows, flags, reserved, rs, max_rows * rs if rgs is None else rgs, fs)
        return lib.qf_frame_rows_dev(handle, ctypes.byref(sh) if shape else None, G_,
                                     rows.data_ptr() if rows_p == "d" else rows_p, None, None, coeffs, None,
                                     frames.data_ptr() if frames_p == "d" else frames_p,
                                     flen.data_ptr() if flen_p == "d" else flen_p, None)

    E = L.QF_EINVAL
    assert status() == 0                                         # Cauchy-less: every row is coded, index k, r = 0
    assert status(handle=None) == E and status(shape=False) == E
    assert status(k=0) == E and status(k=257) == E
    assert status(k=256, fs=272 + 32, max_rows=4, coeffs=co.data_ptr()) == 0
    assert status(max_rows=0) == E and status(max_rows=1025) == E
    assert status(max_rows=1024) == 0
    assert status(Lb=0) == E
    assert status(flags=2) == E and status(flags=3) == E         # unknown flags
    assert status(reserved=1) == E
    assert status(frames_p=None) == E and status(flen_p=None) == E
    assert status(rows_p=None) == E                              # copy mode reads the rows
    assert status(rows_p=None, flags=L.QF_FRAME_IN_PLACE) == 0   # in place does not
    assert status(rows_p=rows.data_ptr() + 8) == E               # misaligned pointers
    assert status(frames_p=frames.data_ptr() + 8) == E
    assert status(rs=40) == E and status(rgs=8 * 48 + 8) == E and status(fs=72) == E   # misaligned strides
    assert status(Lb=40, rs=32) == E                             # a row stride shorter than L
    assert status(fs=32) == E                                    # P + L = 16 + 32 > 32
    assert status(fs=48) == 0
    assert status(k=13, fs=32) == E and status(k=13, fs=48) == 0   # P = 16
    assert status(k=14, fs=48) == E and status(k=14, fs=64) == 0   # P = 32
    assert status(k=200, r=57, fs=256) == L.QF_ERANGE
    assert status(k=200, r=56, fs=256) == 0
    assert status(k=200, r=57, fs=256, coeffs=co.data_ptr()) == 0      # vectors given: no Cauchy row is formed
    assert status(G_=0, frames_p=None, flen_p=None, rows_p=None) == 0  # nothing to do
    gpu_ctx.sync()


def test_parse_frames_coded_call_level_errors(qf, gpu_ctx):
    import torch

    t = lambda n, dt=torch.uint8: torch.zeros(n, dtype=dt, device="cuda")   # noqa: E731
    frames, flen, ids = t(1024 * 64 + 16), t(1024, torch.int32), t(1024, torch.int64)
    rows, idx, n, st, co = t(1024 * 48 + 16), t(1024, torch.int16), t(4, torch.int32), t(1024, torch.int32), t(1024 * 256)
    lib, ctx = L._lib(), gpu_ctx.handle
    ptrs = dict(frames=frames, flen=flen, ids=ids, rows=rows, idx=idx, n=n, co=co, st=st)

    def status(k=8, Lb=32, G_=1, max_rows=8, fs=64, rs=48, rgs=None, handle=ctx, null=(), shift=None):
        p = {nm: (None if nm in null else tt.data_ptr() + (8 if nm == shift else 0)) for nm, tt in ptrs.items()}
        return lib.qf_parse_frames_coded_dev(handle, k, Lb, G_, max_rows, p["frames"], fs, p["flen"], None, p["ids"],
                                             None, p["rows"], rs, max_rows * rs if rgs is None else rgs, p["idx"],
                                             p["n"], p["co"], None, p["st"])

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
    assert status(shift="frames") == E and status(shift="rows") == E
    assert status(fs=72) == E and status(rs=40) == E and status(rgs=8 * 48 + 8) == E
    assert status(Lb=40, rs=32) == E
    assert status(G_=0, null=tuple(ptrs)) == 0
    gpu_ctx.sync()


def test_profile_labels(qf, oracle, gpu_ctx):
    rs_ = RowSet(4, 8, 6, seed=1)
    fs = _P(4) + 32
    gpu_ctx.sync()
    gpu_ctx.profile(True)
    _run_frame_rows(qf, rs_, fs, in_place=False)
    _run_frame_rows(qf, rs_, fs, in_place=True)
    rng = np.random.default_rng(1)
    pfs = _r16(15 + 3 + 4 + 1 + 8 + 1)
    _run_parse(qf, [_make_frames(oracle, rng, 4, 8, 12, 2, pfs, False) for _ in range(G)], 4, 8, 12, pfs, False)
    times = gpu_ctx.kernel_times()
    gpu_ctx.profile(False)
    assert times["k_frame_rows"][0] == 2 and times["k_parse_frames_coded"][0] == 1, times
    assert set(times) == {"k_frame_rows", "k_parse_frames_coded"}, times


# ---------------------------------------------------------------------------
# relay round trip on the device
# ---------------------------------------------------------------------------
def _relay_vectors(oracle, V_held, M, first3):
    """The receiver's vectors of one generation: 3 unit vectors, then the m
    recoded vectors M x V_held."""
    evec = oracle.encode(np.ascontiguousarray(V_held), M.shape[0], np.ascontiguousarray(M))
    units = np.zeros((len(first3), V_held.shape[1]), np.uint8)
    for n, i in enumerate(first3):
        units[n, i] = 1
    return evec, np.concatenate([units, evec])


def test_relay_round_trip_frames_in_frames_out(qf, oracle, gpu_ctx):
    """Sender: encode (8, 4), frame.  Two sources per generation are lost and
    the rest reordered.  Relay: parse, recode 12 packets straight into the
    frame slots, frame in place.  Receiver: 3 of the original systematic frames
    and the 12 relay frames, parse, rank-aware decode.  Every relay frame
    equals the oracle's to_raw of the CPU's seeded mix, and every recovered
    row its source."""
    import torch

    from tests import rank_ref

    k, r, Lb, Gn, m = 8, 4, 40, 4, 12
    rng = np.random.default_rng(808)
    rs = _r16(Lb)
    src = rng.integers(0, 256, (Gn, k, Lb), dtype=np.uint8)
    rep = np.stack([oracle.encode(src[g], r) for g in range(Gn)])
    C = oracle.cauchy(k, r)
    pad = ((0, 0), (0, 0), (0, rs - Lb))
    fs0 = _r16(3 + k + Lb)
    t_tx = _filled(Gn * (k + r) * fs0)
    t_txlen = _filled(4 * Gn * (k + r))
    sh = L.EncodeShape(k, r, Lb, 0, rs, k * rs, rs, r * rs)
    t_src, t_rep = _dev(np.pad(src, pad)), _dev(np.pad(rep, pad))
    L.check(L._lib().qf_frame_batch_dev(gpu_ctx.handle, ctypes.byref(sh), Gn, t_src.data_ptr(), t_rep.data_ptr(),
                                        t_tx.data_ptr(), fs0, t_txlen.data_ptr()), "frame_batch")
    gpu_ctx.sync()
    tx = _host(t_tx).reshape(Gn, k + r, fs0)
    txlen = _host(t_txlen, np.uint32).reshape(Gn, k + r)

    # the channel: 2 sources of every generation lost, the other 10 frames shuffled
    n_held = k + r - 2
    held = np.zeros((Gn, n_held), np.int64)
    rx = np.zeros((Gn, n_held, fs0), np.uint8)
    rxlen = np.zeros((Gn, n_held), np.uint32)
    rxid = np.zeros((Gn, n_held), np.uint64)
    for g in range(Gn):
        lost = set(rng.choice(k, 2, replace=False).tolist())
        arr = [i for i in range(k + r) if i not in lost]
        rng.shuffle(arr)
        held[g] = arr
        for s, i in enumerate(arr):
            rx[g, s], rxlen[g, s] = tx[g, i], txlen[g, i]
            rxid[g, s] = 5 * k + i if i < k else 1000 + i
    X = [np.stack([src[g, i] if i < k else rep[g, i - k] for i in held[g]]) for g in range(Gn)]
    V = [np.stack([np.eye(k, dtype=np.uint8)[i] if i < k else C[i - k] for i in held[g]]) for g in range(Gn)]
    first3 = [[int(i) for i in held[g] if i < k][:3] for g in range(Gn)]

    # the seed, chosen on the CPU: the receiver's vectors reach rank k in every generation
    seed = None
    for cand in range(1, 40):
        M = oracle.fill_splitmix(Gn * m * n_held, cand).reshape(Gn, m, n_held)
        if all(rank_ref.innovative(_relay_vectors(oracle, V[g], M[g], first3[g])[1])[1] == k for g in range(Gn)):
            seed = cand
            break
    assert seed is not None, "no seed under which the receiver's vectors reach rank k in every generation"
    M = oracle.fill_splitmix(Gn * m * n_held, seed).reshape(Gn, m, n_held)
    for g in range(Gn):
        assert rank_ref.innovative(_relay_vectors(oracle, V[g], M[g], first3[g])[1])[1] == k

    # relay: frames -> rows + vectors -> 12 recoded rows in frame slots -> headers
    dev = "cuda"
    z = lambda n, dt=torch.uint8: torch.zeros(n, dtype=dt, device=dev)   # noqa: E731
    r_rows, r_idx, r_n = _filled(Gn * n_held * rs), _filled(2 * Gn * n_held), _filled(4 * Gn)
    r_st, r_co = _filled(4 * Gn * n_held), _filled(Gn * n_held * k)
    qf.parse_frames_coded(_dev(rx), _dev(rxlen), _dev(rxid), r_rows, r_idx, r_n, r_st, r_co, k, Lb, max_rows=n_held,
                          frame_stride=fs0, row_stride=rs, rows_gen_stride=n_held * rs, G=Gn)
    gpu_ctx.sync()
    assert (_host(r_st, np.int32) == 0).all() and (_host(r_n, np.uint32) == n_held).all()
    P = qf.frame_payload_offset(k)
    assert P == 16
    fs = P + rs
    t_out = _filled(Gn * m * fs)
    t_oc, t_rst = z(Gn * m * k), z(Gn, torch.int32)
    qf.recode_batch(r_rows, r_idx, t_out[P:], t_oc, t_rst, k, m, Lb, max_rows=n_held, row_stride=rs,
                    rows_gen_stride=n_held * rs, out_row_stride=fs, out_gen_stride=m * fs, G=Gn, n_rows=r_n,
                    row_coeffs=r_co, seed=seed)
    t_olen, t_ooff = _filled(4 * Gn * m), _filled(4 * Gn * m)
    qf.frame_rows(None, t_out, t_olen, k, Lb, max_rows=m, frame_stride=fs, G=Gn, row_coeffs=t_oc,
                  frame_off=t_ooff, in_place=True)
    gpu_ctx.sync()
    assert (_host(t_rst, np.int32) == 0).all()
    out = _host(t_out).reshape(Gn, m, fs)
    olen = _host(t_olen, np.uint32).reshape(Gn, m)
    ooff = _host(t_ooff, np.uint32).reshape(Gn, m)
    assert (olen == 3 + k + Lb).all() and (ooff == P - 3 - k).all()
    for g in range(Gn):
        epay = oracle.encode(X[g], m, np.ascontiguousarray(M[g]))
        evec, _ = _relay_vectors(oracle, V[g], M[g], first3[g])
        for j in range(m):
            st, want = oracle.packet_to_raw(False, epay[j].tobytes(), evec[j].tobytes())
            assert st == 0
            o = int(ooff[g, j])
            assert out[g, j, o: o + olen[g, j]].tobytes() == want, (g, j)
            assert (out[g, j, :o] == FILL).all() and (out[g, j, o + olen[g, j]:] == FILL).all()

    # receiver: 3 original systematic frames (at slot byte 0), then the relay's 12 at their offsets
    n_rx = 3 + m
    rx2 = np.full((Gn, n_rx, fs), 0x5A, np.uint8)
    rx2len = np.zeros((Gn, n_rx), np.uint32)
    rx2off = np.zeros((Gn, n_rx), np.uint32)
    rx2id = np.zeros((Gn, n_rx), np.uint64)
    for g in range(Gn):
        for s, i in enumerate(first3[g]):
            rx2[g, s, : txlen[g, i]] = tx[g, i, : txlen[g, i]]
            rx2len[g, s], rx2id[g, s] = txlen[g, i], 9 * k + i
        rx2[g, 3:], rx2len[g, 3:], rx2off[g, 3:] = out[g], olen[g], ooff[g]
        rx2id[g, 3:] = 7000 + np.arange(m)
    d_rows, d_idx, d_n = _filled(Gn * n_rx * rs), _filled(2 * Gn * n_rx), _filled(4 * Gn)
    d_st, d_co = _filled(4 * Gn * n_rx), _filled(Gn * n_rx * k)
    qf.parse_frames_coded(_dev(rx2), _dev(rx2len), _dev(rx2id), d_rows, d_idx, d_n, d_st, d_co, k, Lb,
                          max_rows=n_rx, frame_stride=fs, row_stride=rs, rows_gen_stride=n_rx * rs, G=Gn,
                          frame_off=_dev(rx2off))
    gpu_ctx.sync()
    assert (_host(d_st, np.int32) == 0).all() and (_host(d_n, np.uint32) == n_rx).all()
    rec, ri = z(Gn * k * rs), z(Gn * k, torch.int16)
    nrec, st, rank = z(Gn, torch.int32), _filled(4 * Gn), z(Gn, torch.int32)
    qf.decode_innovative_batch(d_rows, d_idx.view(torch.int16), rec, ri, nrec, st.view(torch.int32), k, k, Lb,
                               max_rows=n_rx, row_stride=rs, rows_gen_stride=n_rx * rs, rec_row_stride=rs,
                               rec_gen_stride=k * rs, G=Gn, n_rows=d_n.view(torch.int32), row_coeffs=d_co, rank=rank)
    gpu_ctx.sync()
    assert (_host(st, np.int32) == L.QF_OK).all(), _host(st, np.int32)
    assert (rank.cpu().numpy() == k).all()
    recv = rec.cpu().numpy().reshape(Gn, k, rs)
    rix = ri.cpu().numpy().view(np.uint16).reshape(Gn, k)
    for g in range(Gn):
        erased = sorted(set(range(k)) - set(first3[g]))
        assert nrec.cpu().numpy()[g] == len(erased) == k - 3
        assert sorted(rix[g, : k - 3].tolist()) == erased
        for j in range(k - 3):
            assert np.array_equal(recv[g, j, :Lb], src[g, rix[g, j]]), (g, j)
