"""Reference of the Cauchy wire framing calls -- TEST INFRASTRUCTURE ONLY.

qf_frame_batch_dev / qf_parse_frames_dev restated in plain numpy over the
oracle's Packet::to_raw / Packet::from_raw (oracle/qf_oracle_wire.c) plus the
batch rules written in include/qf_fec.h above the two calls.  Nothing here
touches the library under test.

frame_batch:     the frames of an encode batch, one oracle.packet_to_raw each.
frame_batch_np:  the same bytes laid out in a poisoned frame buffer by array
                 assignment, for a G at which one ctypes call per frame is too
                 slow (tests/test_wire_ref_cpu.py holds the two equal).
parse_frames:    status / n_rows / row_index / rows of every generation.
header_cases:    the planted frames of the header test: every branch of the
                 parser's status rule, at its edges.
place:           frames of their own lengths -> the slot arrays of a call."""
from __future__ import annotations

import numpy as np

OK, EINVAL, ERANGE, ETOOSMALL = 0, -1, -2, -7
FILL_FRAME, FILL_ROW, FILL_STATUS, FILL_INDEX = 0xCC, 0x5A, 99, 0xFFFF
FILL_GAP = 0xEE   # the stride gaps of src / rep


def r16(x: int) -> int:
    return (x + 15) // 16 * 16


def cauchy(oracle, k: int, r: int) -> np.ndarray:
    """oracle.cauchy with r = 0 allowed: (r, k)."""
    if r == 0:
        return np.zeros((0, k), np.uint8)
    C = oracle.cauchy(k, r)
    assert C is not None, (k, r)
    return C


# ---------------------------------------------------------------------------
# frame_batch
# ---------------------------------------------------------------------------
def frame_batch(oracle, k: int, r: int, L: int, src, rep) -> list:
    """src (G, k, L), rep (G, r, L) (None when r = 0) -> the G * (k + r) frames
    (bytes) in the order g * (k + r) + i, sources then repairs."""
    C = cauchy(oracle, k, r)
    out = []
    for g in range(len(src)):
        for i in range(k + r):
            if i < k:
                st, raw = oracle.packet_to_raw(True, src[g][i][:L].tobytes())
            else:
                st, raw = oracle.packet_to_raw(False, rep[g][i - k][:L].tobytes(), bytes(C[i - k]))
            assert st == 0, (g, i, st)
            out.append(raw)
    return out


def frame_batch_np(oracle, k: int, r: int, L: int, src, rep, frame_stride: int, fill: int = FILL_FRAME):
    """-> (frame buffer (G, k + r, frame_stride) with `fill` outside the frames'
    bytes, frame_len (G, k + r) u32)."""
    G = len(src)
    buf = np.full((G, k + r, frame_stride), fill, np.uint8)
    lens = np.empty((G, k + r), np.uint32)
    buf[:, :k, 0] = 1
    buf[:, :k, 1: 1 + L] = np.asarray(src)[:, :, :L]
    lens[:, :k] = 1 + L
    if r:
        buf[:, k:, 0] = 0
        buf[:, k:, 1] = k >> 8
        buf[:, k:, 2] = k & 0xFF
        buf[:, k:, 3: 3 + k] = cauchy(oracle, k, r)[None]
        buf[:, k:, 3 + k: 3 + k + L] = np.asarray(rep)[:, :, :L]
        lens[:, k:] = 3 + k + L
    return buf, lens


def strided(a, row_stride: int, gen_stride: int, fill: int = FILL_GAP) -> np.ndarray:
    """(G, n, L) rows -> the flat buffer with row i of generation g at
    g * gen_stride + i * row_stride, `fill` in every gap."""
    a = np.asarray(a, np.uint8)
    G, n, L = a.shape
    assert row_stride >= L and gen_stride >= n * row_stride
    buf = np.full((G, gen_stride), fill, np.uint8)
    for i in range(n):
        buf[:, i * row_stride: i * row_stride + L] = a[:, i]
    return buf.reshape(-1)


# ---------------------------------------------------------------------------
# parse_frames
# ---------------------------------------------------------------------------
def frame_rule(oracle, k: int, r: int, L: int, frame_stride: int, slot, length: int, pid: int, C=None):
    """The decision for one frame: (status, row index, payload bytes).  slot:
    the frame slot's bytes (at least min(length, frame_stride) of them)."""
    length = int(length)
    if length == 0 or length > frame_stride:
        return EINVAL, None, None
    raw = slot[:length].tobytes() if isinstance(slot, np.ndarray) else bytes(slot[:length])
    assert len(raw) == length
    st, sys_, coeffs, payload = oracle.packet_from_raw(raw, block_size=1 << 20)
    if st:
        return (EINVAL if st == oracle.FR_EMPTY else ETOOSMALL), None, None
    if sys_:
        idx = int(pid) % k
    else:
        C = cauchy(oracle, k, r) if C is None else C
        j = next((j for j in range(r) if bytes(C[j]) == coeffs), None) if len(coeffs) == k else None
        if j is None:
            return ERANGE, None, None
        idx = k + j
    if len(payload) > L:
        return EINVAL, None, None
    return OK, idx, payload


def parse_frames(oracle, k: int, r: int, L: int, max_rows: int, frames, lens, ids, n_frames=None) -> list:
    """frames (G, max_rows, frame_stride), lens / ids (G, max_rows), n_frames
    (G,) or None (max_rows everywhere; counts above max_rows are clamped) ->
    per generation a dict: status (the generation's frame count of them),
    n_rows, row_index (n_rows,) u16, rows (n_rows, L) zero padded."""
    frames = np.asarray(frames)
    G, mr, fs = frames.shape
    assert mr == max_rows
    C = cauchy(oracle, k, r)
    out = []
    for g in range(G):
        nf = max_rows if n_frames is None else min(int(n_frames[g]), max_rows)
        status, index, rows = [], [], []
        for s in range(nf):
            st, idx, payload = frame_rule(oracle, k, r, L, fs, frames[g, s], lens[g][s], int(ids[g][s]), C)
            status.append(st)
            if st == OK:
                index.append(idx)
                row = np.zeros(L, np.uint8)
                row[: len(payload)] = np.frombuffer(payload, np.uint8)
                rows.append(row)
        out.append(dict(status=np.array(status, np.int32), n_rows=len(rows), row_index=np.array(index, np.uint16),
                        rows=np.array(rows, np.uint8).reshape(len(rows), L)))
    return out


def place(entries, max_rows: int, frame_stride: int, fill: int = FILL_FRAME):
    """entries: per generation a list of (frame bytes, length, id, ...) -> the
    arrays of a call: frames (G, max_rows, frame_stride) with `fill` behind the
    bytes given, lens (G, max_rows) u32, ids (G, max_rows) u64, n_frames (G,)."""
    G = len(entries)
    frames = np.full((G, max_rows, frame_stride), fill, np.uint8)
    lens = np.zeros((G, max_rows), np.uint32)
    ids = np.zeros((G, max_rows), np.uint64)
    n = np.zeros(G, np.uint32)
    for g, gen in enumerate(entries):
        assert len(gen) <= max_rows
        n[g] = len(gen)
        for s, e in enumerate(gen):
            b = np.frombuffer(bytes(e[0]), np.uint8)[:frame_stride]
            frames[g, s, : len(b)] = b
            lens[g, s] = e[1]
            ids[g, s] = e[2]
    return frames, lens, ids, n


# ---------------------------------------------------------------------------
# the planted header cases
# ---------------------------------------------------------------------------
def header_cases(oracle, k: int, r: int, L: int, frame_stride: int, seed: int = 0) -> list:
    """-> [(frame bytes, length, id, expected status, what it probes)].  The
    expected status is written down here from the rule in qf_fec.h, not taken
    from parse_frames: tests/test_wire_ref_cpu.py holds the two against each
    other.  Entries a shape cannot express are left out."""
    assert r >= 1 and frame_stride >= 3 + k + L and frame_stride % 16 == 0
    rng = np.random.default_rng(1000 * k + L + seed)
    C = cauchy(oracle, k, r)
    rows = {bytes(C[j]) for j in range(r)}

    def pay(n):
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()

    def sysf(n):
        return b"\x01" + pay(n)

    def rep(vec, n, first=0, cl=k):
        return bytes([first, cl >> 8, cl & 0xFF]) + bytes(vec) + pay(n)

    def vec_status(vec):
        return OK if bytes(vec) in rows else ERANGE

    out = []
    add = lambda raw, ln, pid, st, what: out.append((raw, ln, pid, st, what))   # noqa: E731
    # the first byte: 1 is systematic, everything else a repair (encoder.rs:28)
    add(sysf(L), 1 + L, 3 * k + 1, OK, "first byte 1")
    for first in (0, 2, 0xFF):
        add(rep(C[0], L, first=first), 3 + k + L, 7, OK, f"first byte {first:#x}, a valid repair behind it")
    # lengths
    add(sysf(L), 0, 1, EINVAL, "length 0")
    add(sysf(0), 1, 2 * k + (k - 1), OK, "length 1: systematic, empty payload")
    add(rep(C[0], L), 1, 1, ETOOSMALL, "length 1, a repair")
    add(rep(C[0], L), 2, 1, ETOOSMALL, "length 2: no coefficient length")
    add(rep(C[0], L), 3 + k - 1, 1, ETOOSMALL, "length 3 + k - 1: coefficients truncated")
    add(rep(C[r - 1], 0), 3 + k, 1, OK, "length 3 + k: repair, empty payload")
    full = rep(C[0], frame_stride - 3 - k)
    add(full, frame_stride, 1, OK if frame_stride - 3 - k <= L else EINVAL, "length == frame_stride, a valid repair")
    other_cl = rep(C[0], frame_stride - 3 - k, cl=k + 1)
    add(other_cl, frame_stride, 1, ERANGE, "length == frame_stride, coefficient length k + 1: still parsed")
    add(other_cl, frame_stride + 1, 1, EINVAL, "length == frame_stride + 1: not parsed")
    # the coefficient length is a big-endian u16
    hi = rep(C[0], frame_stride - 3 - k, cl=256 + k)
    add(hi, min(3 + k + L, 3 + 256 + k - 1), 1, ETOOSMALL, "coefficient length 256 + k, frame shorter than that")
    if 3 + 256 + k <= frame_stride:
        add(hi, 3 + 256 + k, 1, ERANGE, "coefficient length 256 + k, frame long enough")
    add(rep(C[0], L, cl=k - 1), 3 + k + L, 1, ERANGE, "coefficient length k - 1")
    add(rep(C[0], L, cl=k + 1), 3 + k + L, 1, ERANGE, "coefficient length k + 1")
    # the Cauchy row range
    add(rep(C[r - 1], L), 3 + k + L, 1, OK, "Cauchy row j = r - 1, the last one inside")
    if k + r + 1 <= 256:
        add(rep(cauchy(oracle, k, r + 1)[r], L), 3 + k + L, 1, ERANGE, "Cauchy row j = r, the first one outside")
    if 255 - k > r:
        add(rep(cauchy(oracle, k, 256 - k)[255 - k], L), 3 + k + L, 1, ERANGE, "Cauchy row j = 255 - k")
    zero_c0 = C[0].copy()
    zero_c0[0] = 0
    add(rep(zero_c0, L), 3 + k + L, 1, ERANGE, "c0 == 0")
    for pos in sorted({0, 1, k - 1} & set(range(k))):
        v = C[min(1, r - 1)].copy()
        v[pos] ^= 1
        add(rep(v, L), 3 + k + L, 1, vec_status(v), f"coefficient {pos} flipped")
    if k > 1 and 3 + k + L + 1 <= frame_stride:
        v = C[0].copy()
        v[k // 2] ^= 0x80
        add(rep(v, L + 1), 3 + k + L + 1, 1, ERANGE, "not a Cauchy row and payload L + 1: QF_ERANGE wins")
    add(sysf(L + 1), 2 + L, 5, EINVAL, "systematic, payload L + 1")
    # accepted companions, so that a third of the list compacts into rows: the
    # repairs in turn with short payloads, sources with ids across the columns
    lens = [n for n in (L, L - 1, 1, 17, 16, 15, 20, 19, 21) if 0 <= n <= L]
    n_ok = sum(1 for e in out if e[3] == OK)
    i = 0
    while 2 * n_ok < len(out) - n_ok:
        n = lens[i % len(lens)]
        if i % 2:
            add(rep(C[i % r], n), 3 + k + n, 1, OK, f"companion: repair {i % r}, payload {n}")
        else:
            add(sysf(n), 1 + n, 11 * k + (5 * i) % k, OK, f"companion: source, payload {n}")
        n_ok += 1
        i += 1
    return out
