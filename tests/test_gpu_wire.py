"""Wire framing on the device (encoder.rs:18-152): frames byte-equal to the
oracle's restatement of Packet::to_raw (oracle/qf_oracle_wire.c), parse
statuses and payloads equal to the oracle's Packet::from_raw, and frames ->
parse -> decode recovers the sources, with lost, reordered and malformed
frames.  Below those, k_frame_batch and k_parse_frames at their length and
count edges against the model of tests/wire_ref.py: every payload and frame
length around the 16-byte blocks, more frame slots than the parser's block has
threads, every branch of the status rule, ids beyond 32 bits, wide strides,
optional pointers NULL, a second round of the framer's grid-stride loop, and
the argument checks of both calls."""
import ctypes

import numpy as np
import pytest

from quicfuscate_amd import _lib as L
from tests import wire_ref as WR

pytestmark = pytest.mark.gpu


def _r16(x):
    return (x + 15) // 16 * 16


def _frame_batch(qf, src, rep, k, r, Lb, G, fs):
    """src / rep: rows of round16(Lb) bytes."""
    import torch

    rs = _r16(Lb)
    frames = torch.full((G * (k + r) * fs,), 0xCC, dtype=torch.uint8, device="cuda")
    flen = torch.zeros(G * (k + r), dtype=torch.int32, device="cuda")
    sh = L.EncodeShape(k, r, Lb, 0, rs, k * rs, rs, r * rs)
    L.check(L._lib().qf_frame_batch_dev(qf.default_context().handle, ctypes.byref(sh), G, src.data_ptr(),
                                        rep.data_ptr(), frames.data_ptr(), fs, flen.data_ptr()), "frame")
    qf.default_context().sync()
    return frames.cpu().numpy().reshape(G, k + r, fs), flen.cpu().numpy().reshape(G, k + r)


@pytest.mark.parametrize("k,r,Lb", [(64, 16, 1200), (4, 2, 8), (7, 5, 33), (16, 1, 1)])
def test_frames_equal_to_raw(qf, oracle, gpu_ctx, k, r, Lb):
    import torch

    rng = np.random.default_rng(k + Lb)
    G = 3
    fs = (3 + k + Lb + 15) // 16 * 16
    src_np = rng.integers(0, 256, (G, k, Lb), dtype=np.uint8)
    rep_np = np.stack([oracle.encode(src_np[g], r) for g in range(G)])
    pad = _r16(Lb) - Lb
    src = torch.from_numpy(np.pad(src_np, ((0, 0), (0, 0), (0, pad))).reshape(-1)).cuda()
    rep = torch.from_numpy(np.pad(rep_np, ((0, 0), (0, 0), (0, pad))).reshape(-1)).cuda()
    frames, flen = _frame_batch(qf, src, rep, k, r, Lb, G, fs)
    C = oracle.cauchy(k, r)
    for g in range(G):
        for i in range(k + r):
            if i < k:
                st, want = oracle.packet_to_raw(True, src_np[g, i].tobytes())
            else:
                st, want = oracle.packet_to_raw(False, rep_np[g, i - k].tobytes(), bytes(C[i - k]))
            assert st == 0
            assert flen[g, i] == len(want)
            assert frames[g, i, : len(want)].tobytes() == want, (g, i)
            assert (frames[g, i, len(want):] == 0xCC).all()


def test_frames_parse_decode_round_trip(qf, oracle, gpu_ctx):
    import torch

    k, r, Lb, G = 64, 16, 1200, 6
    fs = (3 + k + Lb + 15) // 16 * 16
    rng = np.random.default_rng(77)
    src_np = rng.integers(0, 256, (G, k, Lb), dtype=np.uint8)
    rep_np = np.stack([oracle.encode(src_np[g], r) for g in range(G)])
    frames, flen = _frame_batch(qf, torch.from_numpy(src_np.reshape(-1)).cuda(),
                                torch.from_numpy(rep_np.reshape(-1)).cuda(), k, r, Lb, G, fs)
    max_rows = k + r + 8
    rx = np.zeros((G, max_rows, fs), np.uint8)
    rx_len = np.zeros((G, max_rows), np.uint32)
    rx_id = np.zeros((G, max_rows), np.uint64)
    n_fr = np.zeros(G, np.uint32)
    expect = []
    for g in range(G):
        keep = [i for i in range(k + r) if rng.random() > 0.15]
        rng.shuffle(keep)
        arr = []   # (frame bytes, len, id, expected status, row index if valid)
        for i in keep:
            arr.append((frames[g, i], flen[g, i], g * 1000 + i if i >= k else 5 * k + i, 0,
                        i if i < k else i))
        bad = frames[g, k].copy()
        arr.insert(int(rng.integers(0, len(arr) + 1)), (bad, 0, 1, L.QF_EINVAL, None))       # empty
        arr.insert(int(rng.integers(0, len(arr) + 1)), (bad, 2, 1, L.QF_ETOOSMALL, None))    # no coeff length
        arr.insert(int(rng.integers(0, len(arr) + 1)), (bad, 40, 1, L.QF_ETOOSMALL, None))   # coeffs truncated
        wrong = bad.copy()
        wrong[5] ^= 1
        arr.insert(int(rng.integers(0, len(arr) + 1)), (wrong, flen[g, k], 1, L.QF_ERANGE, None))  # not Cauchy
        short_k = bad.copy()
        short_k[2] = k - 1
        arr.insert(int(rng.integers(0, len(arr) + 1)), (short_k, flen[g, k], 1, L.QF_ERANGE, None))
        too_long = frames[g, 0].copy()
        arr.insert(int(rng.integers(0, len(arr) + 1)), (too_long, 1 + Lb + 1, 0, L.QF_EINVAL, None))
        n_fr[g] = len(arr)
        for s, (fb, ln, pid, st, ridx) in enumerate(arr):
            rx[g, s] = fb
            rx_len[g, s] = ln
            rx_id[g, s] = pid
        expect.append(arr)
    dev = "cuda"
    t_fr = torch.from_numpy(rx.reshape(-1)).to(dev)
    t_len = torch.from_numpy(rx_len.view(np.int32).reshape(-1)).to(dev)
    t_id = torch.from_numpy(rx_id.view(np.int64).reshape(-1)).to(dev)
    t_n = torch.from_numpy(n_fr.view(np.int32)).to(dev)
    rows = torch.zeros(G * max_rows * Lb, dtype=torch.uint8, device=dev)
    ridx = torch.zeros(G * max_rows, dtype=torch.int16, device=dev)
    nrows = torch.zeros(G, dtype=torch.int32, device=dev)
    fst = torch.full((G * max_rows,), 99, dtype=torch.int32, device=dev)
    L.check(L._lib().qf_parse_frames_dev(qf.default_context().handle, k, r, Lb, G, max_rows, t_fr.data_ptr(), fs,
                                         t_len.data_ptr(), t_id.data_ptr(), t_n.data_ptr(), rows.data_ptr(), Lb,
                                         max_rows * Lb, ridx.data_ptr(), nrows.data_ptr(), fst.data_ptr()), "parse")
    qf.default_context().sync()
    st = fst.cpu().numpy().reshape(G, max_rows)
    ri = ridx.cpu().numpy().view(np.uint16).reshape(G, max_rows)
    nr = nrows.cpu().numpy()
    rw = rows.cpu().numpy().reshape(G, max_rows, Lb)
    C = oracle.cauchy(k, r)
    for g in range(G):
        valid = [e for e in expect[g] if e[3] == 0]
        assert list(st[g, : n_fr[g]]) == [e[3] for e in expect[g]]
        # every status and payload follows the oracle's Packet::from_raw, plus the
        # batch rules (Cauchy row of this (k, r); payload <= L)
        for s_, (fb, ln, pid, want_st, _) in enumerate(expect[g]):
            os_, osys, oco, opay = oracle.packet_from_raw(fb[:ln].tobytes())
            if os_:
                exp = {oracle.FR_EMPTY: L.QF_EINVAL}.get(os_, L.QF_ETOOSMALL)
            elif not osys and (len(oco) != k or not any(bytes(C[j]) == oco for j in range(r))):
                exp = L.QF_ERANGE
            elif len(opay) > Lb:
                exp = L.QF_EINVAL
            else:
                exp = 0
            assert st[g, s_] == exp == want_st, (g, s_)
        assert nr[g] == len(valid)
        for s, (fb, ln, pid, _, i) in enumerate(valid):
            assert ri[g, s] == (pid % k if i < k else i)
            payload = src_np[g, i] if i < k else rep_np[g, i - k]
            assert (rw[g, s] == payload).all()
            assert rw[g, s].tobytes() == oracle.packet_from_raw(fb[:ln].tobytes())[3].ljust(Lb, b"\0")
    # decode straight from the parsed rows
    emax = min(k, r)
    rec = torch.empty(G * emax * Lb, dtype=torch.uint8, device=dev)
    rec_index = torch.empty(G * emax, dtype=torch.int16, device=dev)
    n_rec = torch.empty(G, dtype=torch.int32, device=dev)
    status = torch.empty(G, dtype=torch.int32, device=dev)
    qf.decode_batch(rows, ridx, rec, rec_index, n_rec, status, k, r, Lb, max_rows=max_rows, row_stride=Lb,
                    rows_gen_stride=max_rows * Lb, rec_row_stride=Lb, rec_gen_stride=emax * Lb, G=G, n_rows=nrows)
    qf.default_context().sync()
    stt, nrec = status.cpu().numpy(), n_rec.cpu().numpy()
    recv = rec.cpu().numpy().reshape(G, emax, Lb)
    idx = rec_index.cpu().numpy().view(np.uint16).reshape(G, emax)
    for g in range(G):
        got_src = {e[4] for e in expect[g] if e[3] == 0 and e[4] < k}
        n_rep = sum(1 for e in expect[g] if e[3] == 0 and e[4] >= k)
        if len(got_src) + n_rep < k:
            assert stt[g] == L.QF_ENOTREADY
            continue
        assert stt[g] == 0
        for m in range(nrec[g]):
            assert (recv[g, m] == src_np[g, idx[g, m]]).all()


# ---------------------------------------------------------------------------
# The two kernels at their length and count edges, against tests/wire_ref.py.
# Every buffer a call writes starts as poison (0xCC frames and counters, 0x5A
# rows, 99 statuses, 0xFFFF indices), and whole buffers are compared, so every
# byte the contract leaves alone is checked to still hold its poison.
# ---------------------------------------------------------------------------
def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()


def _filled(nbytes, byte):
    import torch

    return torch.full((max(nbytes, 16),), byte, dtype=torch.uint8, device="cuda")


def _host(t, dtype=np.uint8):
    return t.cpu().numpy().view(dtype)


def _same(got, want, what):
    """Whole-buffer equality; the first difference in the message."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        at = tuple(int(x) for x in np.argwhere(got != want)[0])
        raise AssertionError(f"{what}: first difference at {at}: got {got[at]}, want {want[at]}, "
                             f"{int((got != want).sum())} differ")


def _ptr(t, shift=0):
    return None if t is None else t.data_ptr() + shift


# ---- k_frame_batch -------------------------------------------------------
def _frame_call(gpu_ctx, k, r, Lb, src_np, rep_np, fs, *, gap=0, gen_gap=0, with_len=True, G=None):
    """src_np (G, k, Lb), rep_np (G, r, Lb) or None (rep_dev NULL) with row
    strides round16(Lb) + gap and generation strides gen_gap wider than the
    rows, the gaps 0xEE -> (frames (G * (k + r), fs), frame_len or None)."""
    import torch

    Gn = len(src_np) if G is None else G
    rs = _r16(Lb) + gap
    sgs, rgs = k * rs + gen_gap, r * rs + gen_gap
    t_src = _dev(WR.strided(src_np, rs, sgs))
    t_rep = None if rep_np is None else _dev(WR.strided(rep_np, rs, rgs))
    n = len(src_np) * (k + r)
    t_fr = _filled(n * fs, WR.FILL_FRAME)
    t_len = _filled(4 * n, WR.FILL_FRAME)
    sh = L.EncodeShape(k, r, Lb, 0, rs, sgs, rs, rgs)
    torch.cuda.synchronize()
    L.check(L._lib().qf_frame_batch_dev(gpu_ctx.handle, ctypes.byref(sh), Gn, _ptr(t_src), _ptr(t_rep), _ptr(t_fr),
                                        fs, _ptr(t_len) if with_len else None), "frame")
    gpu_ctx.sync()
    return _host(t_fr)[: n * fs].reshape(n, fs), _host(t_len, np.uint32)[:n]


def _expected_frames(raws, fs):
    buf = np.full((len(raws), fs), WR.FILL_FRAME, np.uint8)
    for f, raw in enumerate(raws):
        buf[f, : len(raw)] = np.frombuffer(raw, np.uint8)
    return buf, np.array([len(raw) for raw in raws], np.uint32)


@pytest.mark.parametrize("k,r", [(7, 5), (13, 3)])
def test_frame_batch_length_sweep(qf, oracle, gpu_ctx, k, r):
    """Every L in 1..40 with wide strides: (1 + L) % 16 and (3 + k + L) % 16 on
    every residue and on both sides of the 16-byte path's `+ 20` guard; at
    (13, 3) a repair's payload starts on a block boundary.  A read past L of a
    row would put the 0xEE of the stride gap into a frame."""
    rng = np.random.default_rng(100 * k + r)
    G = 2
    for Lb in range(1, 41):
        src = rng.integers(0, 256, (G, k, Lb), dtype=np.uint8)
        rep = rng.integers(0, 256, (G, r, Lb), dtype=np.uint8)
        fs = _r16(3 + k + Lb) + 16
        frames, flen = _frame_call(gpu_ctx, k, r, Lb, src, rep, fs, gap=16, gen_gap=32)
        want, want_len = _expected_frames(WR.frame_batch(oracle, k, r, Lb, src, rep), fs)
        _same(flen, want_len, f"frame_len at L = {Lb}")
        _same(frames, want, f"frames at L = {Lb}")


@pytest.mark.parametrize("k,r,Lb,with_len", [(255, 1, 20, True), (256, 0, 20, True), (1, 3, 16, True),
                                             (64, 16, 1200, False)])
def test_frame_batch_header_edges(qf, oracle, gpu_ctx, k, r, Lb, with_len):
    """The largest k with a repair, k = 256 (the high byte of the coefficient
    length; r = 0 and rep_dev NULL: no repair frame), k = 1, and frame_len_dev
    NULL."""
    rng = np.random.default_rng(k + Lb)
    G = 2
    src = rng.integers(0, 256, (G, k, Lb), dtype=np.uint8)
    rep = rng.integers(0, 256, (G, r, Lb), dtype=np.uint8) if r else None
    fs = _r16(3 + k + Lb)
    frames, flen = _frame_call(gpu_ctx, k, r, Lb, src, rep, fs, gap=16, gen_gap=32, with_len=with_len)
    want, want_len = _expected_frames(WR.frame_batch(oracle, k, r, Lb, src, rep), fs)
    _same(frames, want, "frames")
    if with_len:
        _same(flen, want_len, "frame_len")
    else:
        assert (flen.view(np.uint8) == WR.FILL_FRAME).all()


def test_frame_batch_second_loop_round(qf, oracle, gpu_ctx):
    """More 16-byte blocks than the capped grid has lanes (num_cus * 8 blocks
    of 256): the lanes of the first blocks come round a second time."""
    import torch

    k, r, Lb = 64, 16, 1200
    fs = _r16(3 + k + Lb)
    bpf = fs // 16
    lanes = torch.cuda.get_device_properties(0).multi_processor_count * 8 * 256
    G = lanes // ((k + r) * bpf) + 1 + 3    # 3 past the smallest G with G * 80 * 80 > lanes
    assert (G - 3) * (k + r) * bpf > lanes >= (G - 4) * (k + r) * bpf
    rng = np.random.default_rng(5)
    src = rng.integers(0, 256, (G, k, Lb), dtype=np.uint8)
    rep = rng.integers(0, 256, (G, r, Lb), dtype=np.uint8)
    frames, flen = _frame_call(gpu_ctx, k, r, Lb, src, rep, fs)
    want, want_len = WR.frame_batch_np(oracle, k, r, Lb, src, rep, fs)
    _same(flen, want_len.reshape(-1), "frame_len")
    assert np.array_equal(frames, want.reshape(-1, fs))


def test_frame_batch_no_ops(qf, oracle, gpu_ctx):
    """G = 0 and L = 0: QF_OK, nothing written."""
    k, r = 7, 5
    src = np.ones((2, k, 16), np.uint8)
    rep = np.ones((2, r, 16), np.uint8)
    frames, flen = _frame_call(gpu_ctx, k, r, 16, src, rep, 32, G=0)
    assert (frames == WR.FILL_FRAME).all() and (flen.view(np.uint8) == WR.FILL_FRAME).all()
    t_src, t_rep = _dev(src), _dev(rep)
    t_fr, t_len = _filled(2 * (k + r) * 32, WR.FILL_FRAME), _filled(4 * 2 * (k + r), WR.FILL_FRAME)
    sh = L.EncodeShape(k, r, 0, 0, 16, k * 16, 16, r * 16)
    assert L._lib().qf_frame_batch_dev(gpu_ctx.handle, ctypes.byref(sh), 2, _ptr(t_src), _ptr(t_rep), _ptr(t_fr),
                                       32, _ptr(t_len)) == L.QF_OK
    gpu_ctx.sync()
    assert (_host(t_fr) == WR.FILL_FRAME).all() and (_host(t_len) == WR.FILL_FRAME).all()


def test_frame_batch_call_level_errors(qf, gpu_ctx):
    """One case per clause of the call's argument checks; no case writes."""
    k0, r0, L0 = 14, 2, 32           # 3 + k + L = 49: a frame_stride of 48 is a multiple of 16 and one byte short
    G = 2
    t_src, t_rep = _filled(G * k0 * 48 + 256, 1), _filled(G * r0 * 48 + 256, 2)
    t_fr, t_len = _filled(G * 256 * 64 + 64, WR.FILL_FRAME), _filled(4 * G * 256, WR.FILL_FRAME)
    lib, ctx = L._lib(), gpu_ctx.handle

    def status(k=k0, r=r0, Lb=L0, fs=64, srs=48, sgs=k0 * 48, rrs=48, rgs=r0 * 48, handle=ctx, shape=True,
               src=0, rep=0, frames=0):
        sh = L.EncodeShape(k, r, Lb, 0, srs, sgs, rrs, rgs)
        p = [None if s is None else t.data_ptr() + s for t, s in ((t_src, src), (t_rep, rep), (t_fr, frames))]
        st = lib.qf_frame_batch_dev(handle, ctypes.byref(sh) if shape else None, G, p[0], p[1], p[2], fs,
                                    t_len.data_ptr())
        if st != 0:
            gpu_ctx.sync()
            assert (_host(t_fr) == WR.FILL_FRAME).all() and (_host(t_len) == WR.FILL_FRAME).all()
        return st

    E = L.QF_EINVAL
    assert status(handle=None) == E and status(shape=False) == E
    assert status(k=0) == E
    assert status(k=200, r=57) == L.QF_ERANGE                      # k + r = 257
    assert status(src=None) == E and status(frames=None) == E
    assert status(rep=None) == E                                   # r > 0 needs the repairs
    assert status(fs=3 + k0 + L0 - 1) == E                         # 48: aligned, one byte short
    assert status(fs=72) == E                                      # long enough, not a multiple of 16
    assert status(frames=8) == E and status(src=8) == E and status(rep=8) == E
    assert status(srs=56) == E and status(sgs=k0 * 48 + 8) == E
    assert status(rrs=56) == E and status(rgs=r0 * 48 + 8) == E
    # the same arguments without the fault are accepted
    assert status() == 0
    assert status(r=0, rep=None, rrs=56, rgs=8) == 0               # without repairs their strides do not matter
    gpu_ctx.sync()
    assert (_host(t_fr)[:16] != WR.FILL_FRAME).any()


# ---- k_parse_frames ------------------------------------------------------
def _parse_call(gpu_ctx, k, r, Lb, frames, lens, ids, n_frames, *, rs=None, rgs=None):
    """frames (G, max_rows, fs), lens / ids (G, max_rows), n_frames (G,) or
    None (n_frames_dev NULL) -> the device buffers after the call."""
    import torch

    Gn, mr, fs = frames.shape
    rs = _r16(Lb) + 16 if rs is None else rs
    rgs = mr * rs + 32 if rgs is None else rgs
    t_fr, t_len, t_id = _dev(frames), _dev(np.asarray(lens, np.uint32)), _dev(np.asarray(ids, np.uint64))
    t_n = None if n_frames is None else _dev(np.asarray(n_frames, np.uint32))
    t = dict(rows=_filled(Gn * rgs, WR.FILL_ROW), idx=_filled(2 * Gn * mr, 0xFF), n=_filled(4 * Gn, WR.FILL_FRAME),
             st=torch.full((Gn * mr,), WR.FILL_STATUS, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    L.check(L._lib().qf_parse_frames_dev(gpu_ctx.handle, k, r, Lb, Gn, mr, _ptr(t_fr), fs, _ptr(t_len), _ptr(t_id),
                                         _ptr(t_n), _ptr(t["rows"]), rs, rgs, _ptr(t["idx"]), _ptr(t["n"]),
                                         _ptr(t["st"])), "parse")
    gpu_ctx.sync()
    return dict(rows=_host(t["rows"])[: Gn * rgs].reshape(Gn, rgs), idx=_host(t["idx"], np.uint16)[: Gn * mr].reshape(Gn, mr),
                n=_host(t["n"], np.uint32)[:Gn], st=_host(t["st"], np.int32).reshape(Gn, mr), rs=rs, rgs=rgs)


def _check_parse(oracle, k, r, Lb, frames, lens, ids, n_frames, got):
    """Every output buffer, whole, against the model laid out in poison: rows
    and indices at or past n_rows, row bytes in [L, row_stride) and behind the
    rows, and statuses at or past the frame count stay poison.  -> the model."""
    Gn, mr, fs = frames.shape
    model = WR.parse_frames(oracle, k, r, Lb, mr, frames, lens, ids, n_frames)
    rs = got["rs"]
    st = np.full((Gn, mr), WR.FILL_STATUS, np.int32)
    idx = np.full((Gn, mr), WR.FILL_INDEX, np.uint16)
    rows = np.full((Gn, got["rgs"]), WR.FILL_ROW, np.uint8)
    for g, m in enumerate(model):
        st[g, : len(m["status"])] = m["status"]
        idx[g, : m["n_rows"]] = m["row_index"]
        for s in range(m["n_rows"]):
            rows[g, s * rs: s * rs + Lb] = m["rows"][s]
    _same(got["st"], st, "frame_status")
    _same(got["n"], np.array([m["n_rows"] for m in model], np.uint32), "n_rows")
    _same(got["idx"], idx, "row_index")
    _same(got["rows"], rows, "rows")
    return model


@pytest.mark.parametrize("k,r,Lb", [(4, 2, 8), (7, 5, 33), (13, 3, 33), (16, 1, 1), (255, 1, 20), (64, 16, 64),
                                    (64, 16, 1200)])
def test_parse_ragged_payloads_and_padding(qf, oracle, gpu_ctx, k, r, Lb):
    """Frames cut to payload lengths on both sides of every 16-byte block and of
    the `+ 20` guard, into rows with a wide stride: the payload, zeros up to
    L, poison behind."""
    rng = np.random.default_rng(k + Lb)
    G, mr = 3, k + r
    fs = _r16(3 + k + Lb)
    src = rng.integers(1, 256, (G, k, Lb), dtype=np.uint8)
    rep = rng.integers(1, 256, (G, r, Lb), dtype=np.uint8)
    raws = WR.frame_batch(oracle, k, r, Lb, src, rep)
    plens = sorted({0, 1, 15, 16, 17, 19, 20, 21, 35, 36, Lb - 1, Lb} & set(range(Lb + 1)))
    entries, cut = [], []
    for g in range(G):
        gen = []
        for i in range(mr):
            f = g * mr + i
            p = plens[(f + g) % len(plens)]
            ln = (1 if i < k else 3 + k) + p
            gen.append((raws[f][:ln], ln, (g + 1) * k + i))
            cut.append(p)
        entries.append(gen)
    frames, lens, ids, n = WR.place(entries, mr, fs)
    got = _parse_call(gpu_ctx, k, r, Lb, frames, lens, ids, n)
    model = _check_parse(oracle, k, r, Lb, frames, lens, ids, n, got)
    assert set(cut) == set(plens)
    rs = got["rs"]
    rows = got["rows"][:, : mr * rs].reshape(G, mr, rs)
    for g in range(G):
        assert model[g]["n_rows"] == mr and (got["st"][g] == 0).all()
        assert got["idx"][g].tolist() == list(range(mr))
        for i in range(mr):
            p = cut[g * mr + i]
            payload = src[g, i] if i < k else rep[g, i - k]
            assert (rows[g, i, :p] == payload[:p]).all(), (g, i)
            assert (rows[g, i, p:Lb] == 0).all(), (g, i)
            assert (rows[g, i, Lb:] == WR.FILL_ROW).all(), (g, i)
        assert (got["rows"][g, mr * rs:] == WR.FILL_ROW).all()


SLOT_K, SLOT_R, SLOT_L, SLOT_FS, SLOT_G = 4, 2, 8, 16, 3
# share of invalid frames per 64-slot wave; four waves make one 256-slot
# round of the parser's loop, and no two rounds look alike
SLOT_DENSITY = ("none", "all", "third", "half",
                "fifth", "none", "all", "some",
                "all", "third", "most", "none",
                "half", "some", "third", "all")


def _slot_loop_case(oracle, max_rows, seed=11):
    """(4, 2, 8) with max_rows frame slots a generation, invalid frames of all
    three error statuses mixed in by wave; the payload of a valid frame starts
    with its slot number.  -> frames, lens, ids, valid (G, max_rows)."""
    k, r, Lb, fs, G = SLOT_K, SLOT_R, SLOT_L, SLOT_FS, SLOT_G
    rng = np.random.default_rng(seed)
    C = WR.cauchy(oracle, k, r)
    entries = []
    valid = np.zeros((G, max_rows), bool)
    for g in range(G):
        gen = []
        for s in range(max_rows):
            d = SLOT_DENSITY[(s // 64 + 5 * g) % len(SLOT_DENSITY)]
            bad = {"none": False, "all": True, "third": s % 3 == 0, "half": s % 2 == 1, "fifth": s % 5 == 2,
                   "some": rng.random() < 0.3, "most": rng.random() < 0.7}[d]
            n = int(rng.integers(2, Lb + 1))
            payload = bytes([s & 0xFF, s >> 8]) + rng.integers(0, 256, n - 2, dtype=np.uint8).tobytes()
            pid = int(rng.integers(0, 2 ** 63)) * 2 + int(rng.integers(0, 2))
            j = int(rng.integers(0, r))
            sysf = b"\x01" + payload
            repf = bytes([0, 0, k]) + bytes(C[j]) + payload
            if not bad:
                raw = sysf if rng.random() < 0.6 else repf
                gen.append((raw, len(raw), pid))
            else:
                kind = (s + g) % 4
                if kind == 0:
                    gen.append((sysf, 0, pid))                                   # QF_EINVAL: empty
                elif kind == 1:
                    gen.append((repf, 2, pid))                                   # QF_ETOOSMALL
                elif kind == 2:
                    wrong = bytearray(repf)
                    wrong[3 + s % k] ^= 1 << (s % 8)
                    gen.append((bytes(wrong), len(wrong), pid))                  # QF_ERANGE
                else:
                    gen.append((b"\x01" + bytes(Lb + 1), 2 + Lb, pid))           # QF_EINVAL: payload L + 1
            valid[g, s] = not bad
        entries.append(gen)
    frames, lens, ids, _ = WR.place(entries, max_rows, fs)
    return frames, lens, ids, valid


def _slot_counts(max_rows):
    return [[max_rows, 0, 257], [max_rows + 5, 1, 256], None]


@pytest.mark.parametrize("max_rows", [300, 1024])
def test_parse_slot_loop_and_prefix(qf, oracle, gpu_ctx, max_rows):
    """More slots than the block's 256 threads: the loop's rounds carry `base`,
    and the waves of a round have different counts of accepted frames, so every
    part of the output slot (`base`, the waves in front, the lanes in front) is
    non-trivial.  Frame counts at max_rows, above it (clamped), 0, 1, 256 and
    257, and n_frames_dev NULL."""
    k, r, Lb = SLOT_K, SLOT_R, SLOT_L
    frames, lens, ids, valid = _slot_loop_case(oracle, max_rows)
    per_wave = [int(valid[0, w: w + 64].sum()) for w in range(0, max_rows - 63, 64)]
    assert 0 in per_wave and 64 in per_wave and len(set(per_wave)) >= 4
    assert len({int(valid[0, i: i + 256].sum()) for i in range(0, max_rows, 256)}) == (max_rows + 255) // 256
    for n_frames in _slot_counts(max_rows):
        got = _parse_call(gpu_ctx, k, r, Lb, frames, lens, ids, n_frames)
        model = _check_parse(oracle, k, r, Lb, frames, lens, ids, n_frames, got)
        rows = got["rows"][:, : max_rows * got["rs"]].reshape(SLOT_G, max_rows, got["rs"])
        for g in range(SLOT_G):
            nf = max_rows if n_frames is None else min(n_frames[g], max_rows)
            arrived = np.flatnonzero(valid[g, :nf])
            assert got["n"][g] == len(arrived) == model[g]["n_rows"]
            tags = rows[g, : len(arrived), 0].astype(np.int64) + 256 * rows[g, : len(arrived), 1].astype(np.int64)
            assert tags.tolist() == arrived.tolist(), g          # compacted in arrival order


def test_parse_is_deterministic(qf, oracle, gpu_ctx):
    """The slot-loop case twice into fresh poisoned buffers: the same bytes."""
    frames, lens, ids, _ = _slot_loop_case(oracle, 1024)
    n_frames = _slot_counts(1024)[0]
    a = _parse_call(gpu_ctx, SLOT_K, SLOT_R, SLOT_L, frames, lens, ids, n_frames)
    b = _parse_call(gpu_ctx, SLOT_K, SLOT_R, SLOT_L, frames, lens, ids, n_frames)
    for name in ("rows", "idx", "n", "st"):
        assert a[name].tobytes() == b[name].tobytes(), name
    assert a["n"][0] > 256


@pytest.mark.parametrize("k,r,Lb", [(7, 5, 33), (64, 16, 1200), (200, 56, 48)])
def test_parse_header_cases(qf, oracle, gpu_ctx, k, r, Lb):
    """The planted frames of wire_ref.header_cases shuffled among the valid
    frames of a generation."""
    rng = np.random.default_rng(k * Lb)
    G = 2
    fs = _r16(3 + k + Lb)
    cases = WR.header_cases(oracle, k, r, Lb, fs)
    src = rng.integers(0, 256, (G, k, Lb), dtype=np.uint8)
    rep = rng.integers(0, 256, (G, r, Lb), dtype=np.uint8)
    raws = WR.frame_batch(oracle, k, r, Lb, src, rep)
    entries = []
    for g in range(G):
        gen = list(cases)
        for i in range(k + r):
            raw = raws[g * (k + r) + i]
            gen.append((raw, len(raw), 1000 * g + i, L.QF_OK, "a valid frame"))
        order = rng.permutation(len(gen))
        entries.append([gen[o] for o in order])
    mr = len(entries[0]) + 3
    frames, lens, ids, n = WR.place(entries, mr, fs)
    got = _parse_call(gpu_ctx, k, r, Lb, frames, lens, ids, n)
    for g in range(G):
        for s, e in enumerate(entries[g]):
            assert got["st"][g, s] == e[3], (g, s, e[4])
    _check_parse(oracle, k, r, Lb, frames, lens, ids, n, got)
    assert set(np.unique(got["st"][:, : len(entries[0])]).tolist()) == {L.QF_OK, L.QF_EINVAL, L.QF_ERANGE,
                                                                         L.QF_ETOOSMALL}


@pytest.mark.parametrize("k,r,Lb", [(7, 5, 33), (100, 6, 16)])
def test_parse_64_bit_ids(qf, oracle, gpu_ctx, k, r, Lb):
    """row_index = id % k over the whole u64: at k = 7 the low 32 bits of
    2^32 + 3 give 3, the id gives 0."""
    id_list = [2 ** 32 + 3, 2 ** 63, 2 ** 64 - 1, 2 ** 32 * k + 1, 2 ** 32 - 1, 2 ** 32, 2 ** 63 + k, 2 ** 64 - k,
               0, k - 1, k, 0x0123456789ABCDEF, 0xFEDCBA9876543210, 3 * 2 ** 32 + 2, 2 ** 62 + 2 ** 31]
    rng = np.random.default_rng(k)
    fs = _r16(3 + k + Lb)
    entries = []
    for order in (id_list, id_list[::-1]):
        entries.append([(b"\x01" + rng.integers(0, 256, Lb, dtype=np.uint8).tobytes(), 1 + Lb, pid) for pid in order])
    mr = len(id_list) + 1
    frames, lens, ids, n = WR.place(entries, mr, fs)
    assert int(ids[0, 2]) == 2 ** 64 - 1
    got = _parse_call(gpu_ctx, k, r, Lb, frames, lens, ids, n)
    assert got["idx"][0, : len(id_list)].tolist() == [pid % k for pid in id_list]
    assert got["idx"][1, : len(id_list)].tolist() == [pid % k for pid in id_list[::-1]]
    if k == 7:
        assert got["idx"][0, 0] == 0 and (2 ** 32 + 3) % 2 ** 32 % k == 3
    _check_parse(oracle, k, r, Lb, frames, lens, ids, n, got)


def test_frame_parse_decode_round_trip_odd_shape(qf, oracle, gpu_ctx):
    """(7, 5, 33): frame, drop and shuffle, parse into rows with a wide stride,
    decode from those rows with the same strides: the erased sources back."""
    import torch

    k, r, Lb, G = 7, 5, 33, 8
    fs = _r16(3 + k + Lb)
    rng = np.random.default_rng(733)
    src = rng.integers(0, 256, (G, k, Lb), dtype=np.uint8)
    rep = np.stack([oracle.encode(src[g], r) for g in range(G)])
    sent, sent_len = _frame_call(gpu_ctx, k, r, Lb, src, rep, fs, gap=16, gen_gap=32)
    sent = sent.reshape(G, k + r, fs)
    sent_len = sent_len.reshape(G, k + r)
    mr = k + r
    entries, erased = [], []
    for g in range(G):
        first = int(rng.integers(0, k))            # at least one source to recover, at most r frames lost
        others = [i for i in range(k + r) if i != first]
        lost = {first} | set(rng.choice(others, size=int(rng.integers(0, r)), replace=False).tolist())
        keep = [i for i in range(k + r) if i not in lost]
        rng.shuffle(keep)
        entries.append([(sent[g, i, : sent_len[g, i]].tobytes(), int(sent_len[g, i]), 3 * k + i) for i in keep])
        erased.append(sorted(set(range(k)) - set(keep[:k])))    # the first k rows win (decoder.rs:678-701)
    frames, lens, ids, n = WR.place(entries, mr, fs)
    rs = _r16(Lb) + 16
    rgs = mr * rs + 32
    dev = "cuda"
    t_fr, t_len, t_id, t_n = _dev(frames), _dev(lens), _dev(ids), _dev(n)
    rows = _filled(G * rgs, WR.FILL_ROW)
    ridx = torch.full((G * mr,), -1, dtype=torch.int16, device=dev)
    nrows = torch.zeros(G, dtype=torch.int32, device=dev)
    fst = torch.full((G * mr,), WR.FILL_STATUS, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    L.check(L._lib().qf_parse_frames_dev(gpu_ctx.handle, k, r, Lb, G, mr, t_fr.data_ptr(), fs, t_len.data_ptr(),
                                         t_id.data_ptr(), t_n.data_ptr(), rows.data_ptr(), rs, rgs, ridx.data_ptr(),
                                         nrows.data_ptr(), fst.data_ptr()), "parse")
    emax = min(k, r)
    rec = _filled(G * emax * rs, WR.FILL_ROW)
    rec_index = torch.full((G * emax,), -1, dtype=torch.int16, device=dev)
    n_rec = torch.full((G,), -1, dtype=torch.int32, device=dev)
    status = torch.full((G,), WR.FILL_STATUS, dtype=torch.int32, device=dev)
    qf.decode_batch(rows, ridx, rec, rec_index, n_rec, status, k, r, Lb, max_rows=mr, row_stride=rs,
                    rows_gen_stride=rgs, rec_row_stride=rs, rec_gen_stride=emax * rs, G=G, n_rows=nrows, ctx=gpu_ctx)
    gpu_ctx.sync()
    assert nrows.cpu().tolist() == [len(e) for e in entries]
    recv = _host(rec)[: G * emax * rs].reshape(G, emax, rs)
    idx = _host(rec_index, np.uint16).reshape(G, emax)
    assert status.cpu().tolist() == [0] * G
    for g in range(G):
        assert n_rec[g].item() == len(erased[g]) >= 1
        assert sorted(idx[g, : len(erased[g])].tolist()) == erased[g]
        for m in range(len(erased[g])):
            assert (recv[g, m, :Lb] == src[g, idx[g, m]]).all(), (g, m)


def test_parse_frames_call_level_errors(qf, gpu_ctx):
    """One case per clause of the call's argument checks; no case writes."""
    import torch

    mr0 = 8
    bufs = dict(frames=_filled(1024 * 64 + 64, 0), flen=_filled(4 * 1024, 0), ids=_filled(8 * 1024, 0),
                rows=_filled(1024 * 64 + 64, WR.FILL_ROW), idx=_filled(2 * 1024, 0xFF), n=_filled(64, WR.FILL_FRAME),
                st=torch.full((1024,), WR.FILL_STATUS, dtype=torch.int32, device="cuda"))
    t_n = _dev(np.full(4, mr0, np.uint32))
    lib, ctx = L._lib(), gpu_ctx.handle

    def untouched():
        gpu_ctx.sync()
        return ((_host(bufs["rows"]) == WR.FILL_ROW).all() and (_host(bufs["idx"]) == 0xFF).all()
                and (_host(bufs["n"]) == WR.FILL_FRAME).all() and (_host(bufs["st"], np.int32) == WR.FILL_STATUS).all())

    def status(k=8, r=2, Lb=32, G_=1, max_rows=mr0, fs=64, rs=48, rgs=None, handle=ctx, null=(), shift=None,
               n_frames=True):
        p = {nm: (None if nm in null else t.data_ptr() + (8 if nm == shift else 0)) for nm, t in bufs.items()}
        st = lib.qf_parse_frames_dev(handle, k, r, Lb, G_, max_rows, p["frames"], fs, p["flen"], p["ids"],
                                     t_n.data_ptr() if n_frames else None, p["rows"], rs,
                                     max_rows * rs if rgs is None else rgs, p["idx"], p["n"], p["st"])
        if st != 0 or G_ == 0:
            assert untouched()
        return st

    E = L.QF_EINVAL
    assert status(handle=None) == E
    assert status(k=0) == E
    assert status(k=200, r=57) == L.QF_ERANGE                    # k + r = 257
    assert status(max_rows=0) == E and status(max_rows=1025) == E
    assert status(Lb=0) == E
    for nm in bufs:
        assert status(null=(nm,)) == E, nm                       # the seven required pointers
    assert status(fs=72) == E
    assert status(shift="frames") == E and status(shift="rows") == E
    assert status(rs=56) == E and status(rgs=mr0 * 48 + 8) == E
    assert status(Lb=32, rs=16) == E                             # a row stride of L - 16
    assert status(G_=0, null=tuple(bufs), n_frames=False) == 0   # nothing to do
    # the same arguments without the fault are accepted; n_frames_dev may be NULL
    assert status() == 0 and status(n_frames=False) == 0
    assert status(k=200, r=56, max_rows=4) == 0 and status(max_rows=1024, rs=48) == 0
    gpu_ctx.sync()
    assert (_host(bufs["st"], np.int32)[:mr0] != WR.FILL_STATUS).all()


def test_wire_profile_names(qf, oracle, gpu_ctx):
    """One call of each reports exactly its kernel."""
    k, r, Lb, fs = 4, 2, 8, 16
    src = np.ones((1, k, Lb), np.uint8)
    rep = np.ones((1, r, Lb), np.uint8)
    gpu_ctx.sync()
    gpu_ctx.profile(True)
    frames, flen = _frame_call(gpu_ctx, k, r, Lb, src, rep, fs)
    times = gpu_ctx.kernel_times()
    gpu_ctx.profile(False)
    assert set(times) == {"k_frame_batch"} and times["k_frame_batch"][0] == 1, times
    gpu_ctx.profile(True)
    _parse_call(gpu_ctx, k, r, Lb, frames.reshape(1, k + r, fs), flen.reshape(1, k + r),
                np.arange(k + r, dtype=np.uint64).reshape(1, k + r), None)
    times = gpu_ctx.kernel_times()
    gpu_ctx.profile(False)
    assert set(times) == {"k_parse_frames"} and times["k_parse_frames"][0] == 1, times
