"""Reference of the flat-poll ingest -- TEST INFRASTRUCTURE ONLY.

A flat poll is N frame slots in arrival order plus one u32 generation tag per
frame (qf_parse_poll_headers_dev).  This module holds, in plain numpy:

group:       the grouping rule: the touched generations (a frame tagged below
             G_src) ascending, the first n_max of them listed; per entry the
             frame numbers in arrival order, or none and QF_ETOOSMALL when the
             generation has more than max_rows frames; the per-frame statuses
             that follow from the tags alone (QF_EINVAL for a tag >= G_src,
             QF_ENOTREADY for an unlisted or an overflowed generation).
frame_rule:  qf_parse_frame_headers_dev's decision for one frame.
ingest:      both together: every output of qf_parse_poll_headers_dev.
dense_poll:  the host-sorted dense poll qf_parse_frame_headers_dev takes: one
             region of max_rows slots per list entry, the entry's frames copied
             there in arrival order.  It is what a receiver did on the host
             before the ingest existed.
make_poll:   the seeded polls of tests/test_gpu_poll_ingest.py."""
from __future__ import annotations

import functools

import numpy as np

FILL, FILL16, FILL32 = 0xCC, 0xCCCC, 0xCCCCCCCC
OK, EINVAL, ERANGE, ENOTREADY, ETOOSMALL = 0, -1, -2, -3, -7


def r16(x: int) -> int:
    return (x + 15) // 16 * 16


def payload_offset(k: int) -> int:
    return r16(3 + k)


class Poll:
    """N_max slots of fs bytes, 0xCC outside the frames' bytes."""

    def __init__(self, k: int, L: int, N_max: int, fs: int | None = None):
        self.k, self.L, self.N_max = k, L, N_max
        self.P = payload_offset(k)
        self.fs = self.P + r16(L) if fs is None else fs
        self.frames = np.full((N_max, self.fs), FILL, np.uint8)
        self.flen = np.zeros(N_max, np.uint32)
        self.foff = np.zeros(N_max, np.uint32)
        self.ids = np.zeros(N_max, np.uint64)
        self.gen = np.full(N_max, 0xFFFFFFFF, np.uint32)
        self.kind = [""] * N_max

    def put_sys(self, f: int, gen: int, pid: int, payload: np.ndarray, off: int | None = None):
        off = self.P - 1 if off is None else off
        raw = np.concatenate([np.array([1], np.uint8), payload.astype(np.uint8)])
        self._put(f, gen, pid, raw, off, "sys")

    def put_coded(self, f: int, gen: int, pid: int, vec: np.ndarray, payload: np.ndarray, off: int | None = None,
                  cl: int | None = None):
        off = self.P - 3 - self.k if off is None else off
        cl = len(vec) if cl is None else cl
        raw = np.concatenate([np.array([0, cl >> 8, cl & 0xFF], np.uint8), vec.astype(np.uint8), payload.astype(np.uint8)])
        self._put(f, gen, pid, raw, off, "coded")

    def _put(self, f, gen, pid, raw, off, kind):
        assert off + len(raw) <= self.fs
        self.frames[f, off: off + len(raw)] = raw
        self.flen[f], self.foff[f], self.ids[f], self.gen[f], self.kind[f] = len(raw), off, pid, gen, kind


def frame_rule(p: Poll, f: int):
    """-> status, index, payload start in the slot, payload length (the last three valid for QF_OK)."""
    k, flen, foff = p.k, int(p.flen[f]), int(p.foff[f])
    if flen == 0 or foff + flen > p.fs:
        return EINVAL, 0, 0, 0
    fr = p.frames[f, foff:]
    if fr[0] == 1:
        off, idx = 1, int(p.ids[f] % np.uint64(k))
    elif flen < 3:
        return ETOOSMALL, 0, 0, 0
    else:
        cl = (int(fr[1]) << 8) | int(fr[2])
        if flen < 3 + cl:
            return ETOOSMALL, 0, 0, 0
        if cl != k:
            return ERANGE, 0, 0, 0
        off, idx = 3 + cl, k
    plen, pay = flen - off, foff + off
    if plen > p.L or pay % 16:
        return EINVAL, 0, 0, 0
    return OK, idx, pay, plen


def group(gen, N: int, G_src: int, n_max: int, max_rows: int):
    """-> sel (list), n_match, entries (per listed entry: frame numbers ascending, [] when overflowed),
    entry_status (n_max,), tag_status (N,): QF_EINVAL / QF_ENOTREADY / None (the frame is parsed)."""
    gen = np.asarray(gen, np.uint32)[:N]
    touched = sorted({int(t) for t in gen if t < G_src})
    sel = touched[:n_max]
    pos = {g: j for j, g in enumerate(sel)}
    members = [[] for _ in sel]
    for f in range(N):                                   # ascending f: the arrival order
        if int(gen[f]) in pos:
            members[pos[int(gen[f])]].append(f)
    entry_status = np.full(n_max, OK, np.int32)
    entries = []
    for j, m in enumerate(members):
        if len(m) > max_rows:
            entry_status[j] = ETOOSMALL
            entries.append([])
        else:
            entries.append(m)
    tag_status = []
    for f in range(N):
        t = int(gen[f])
        if t >= G_src:
            tag_status.append(EINVAL)
        elif t not in pos or entry_status[pos[t]] != OK:
            tag_status.append(ENOTREADY)
        else:
            tag_status.append(None)
    return sel, len(touched), entries, entry_status, tag_status


class Ingested:
    """The outputs of qf_parse_poll_headers_dev, 0xCC where the call writes nothing."""

    def __init__(self, p: Poll, n_frames, G_src: int, n_max: int, max_rows: int):
        k = p.k
        N = p.N_max if n_frames is None else min(int(n_frames), p.N_max)
        self.N, self.n_max, self.max_rows = N, n_max, max_rows
        sel, self.n_match, self.entries, self.entry_status, tag_status = group(p.gen, N, G_src, n_max, max_rows)
        self.n_sel = len(sel)
        self.sel = np.full(n_max, FILL32, np.uint32)
        self.sel[: len(sel)] = sel
        self.row_off = np.full((n_max, max_rows), FILL32, np.uint32)
        self.row_len = np.full((n_max, max_rows), FILL32, np.uint32)
        self.row_index = np.full((n_max, max_rows), FILL16, np.uint16)
        self.row_coeffs = np.full((n_max, max_rows, k), FILL, np.uint8)
        self.n_rows = np.zeros(n_max, np.uint32)
        self.frame_status = np.full(p.N_max, FILL32, np.uint32).view(np.int32)
        self.row_frame = [[] for _ in range(n_max)]      # frame number of each compacted row
        for f in range(N):
            if tag_status[f] is not None:
                self.frame_status[f] = tag_status[f]
        for j, m in enumerate(self.entries):
            c = 0
            for f in m:
                st, idx, pay, plen = frame_rule(p, f)
                self.frame_status[f] = st
                if st != OK:
                    continue
                self.row_off[j, c], self.row_len[j, c], self.row_index[j, c] = f * p.fs + pay, plen, idx
                if idx < k:
                    self.row_coeffs[j, c] = 0
                    self.row_coeffs[j, c, idx] = 1
                else:
                    self.row_coeffs[j, c] = p.frames[f, pay - k: pay]
                self.row_frame[j].append(f)
                c += 1
            self.n_rows[j] = c


def ingest(p: Poll, n_frames, G_src: int, n_max: int, max_rows: int) -> Ingested:
    return Ingested(p, n_frames, G_src, n_max, max_rows)


def dense_poll(p: Poll, entries, G: int, max_rows: int, gens=None):
    """The host sort: region j (or region gens[j] of G) of max_rows slots holds the frames entries[j]
    in order -> frames (G, max_rows, fs), flen, foff, ids (G, max_rows), n_frames (G,)."""
    frames = np.full((G, max_rows, p.fs), FILL, np.uint8)
    flen = np.zeros((G, max_rows), np.uint32)
    foff = np.zeros((G, max_rows), np.uint32)
    ids = np.zeros((G, max_rows), np.uint64)
    nfr = np.zeros(G, np.uint32)
    for j, m in enumerate(entries):
        g = j if gens is None else int(gens[j])
        assert len(m) <= max_rows
        for s, f in enumerate(m):
            frames[g, s], flen[g, s], foff[g, s], ids[g, s] = p.frames[f], p.flen[f], p.foff[f], p.ids[f]
        nfr[g] = len(m)
    return frames, flen, foff, ids, nfr


# the shapes of the device tests: (k, max_rows); L, G_src and N are shared
SHAPES = [(5, 6), (64, 6), (64, 70), (100, 6), (200, 6)]
L_POLL, G_POLL, N_POLL = 40, 23, 300
BAD_KINDS = ("empty", "past_slot", "long", "short", "truncated", "wrong_k", "unaligned")
BAD_STATUS = dict(empty=EINVAL, past_slot=EINVAL, long=EINVAL, short=ETOOSMALL, truncated=ETOOSMALL, wrong_k=ERANGE,
                  unaligned=EINVAL)
GEN_EXACT, GEN_OVER, GEN_HEAVY, GEN_CASES = 3, 7, 12, 5       # max_rows frames, max_rows + 1, many, the special rows
UNTOUCHED = (0, 9, 22)


def _bad_frame(p: Poll, rng, f: int, gen: int, kind: str):
    k, L, P = p.k, p.L, p.P
    vec = rng.integers(1, 256, k).astype(np.uint8)
    pay = rng.integers(0, 256, L, dtype=np.uint8)
    if kind == "empty":
        p.put_coded(f, gen, 5, vec, pay[:7])
        p.flen[f] = 0
    elif kind == "past_slot":
        p.put_coded(f, gen, 5, vec, pay[: p.fs - P])
        p.flen[f] += 1                                    # frame_off + frame_len is one more than the slot holds
    elif kind == "long":
        p.put_sys(f, gen, 5, rng.integers(0, 256, L + 1, dtype=np.uint8))
    elif kind == "short":
        p.put_coded(f, gen, 5, vec, pay[:0])
        p.flen[f] = 2
    elif kind == "truncated":
        p.put_coded(f, gen, 5, vec, pay[:0])
        p.flen[f] = 3 + k - 1
    elif kind == "wrong_k":
        p.put_coded(f, gen, 5, vec, pay[:9], cl=k + 1)
    else:
        assert kind == "unaligned"
        p.put_sys(f, gen, 5, pay[:9], off=P - 2)
    p.kind[f] = kind


@functools.lru_cache(maxsize=None)
def make_poll(k: int, max_rows: int, seed: int) -> Poll:
    """One seeded poll of N_POLL frames over G_POLL generations (tests/test_poll_ingest_cpu.py asserts the
    cases it holds)."""
    rng = np.random.default_rng(seed * 1000 + k * 7 + max_rows)
    L, G_src, N = L_POLL, G_POLL, N_POLL
    p = Poll(k, L, N)
    tags = []
    free = [g for g in range(G_src) if g not in UNTOUCHED + (GEN_EXACT, GEN_OVER, GEN_HEAVY, GEN_CASES)]
    tags += [GEN_EXACT] * max_rows + [GEN_OVER] * (max_rows + 1)
    tags += [GEN_CASES] * 6
    tags += [G_src, 0xFFFFFFFF, G_src + 5]
    # the invalid frames, in one generation when they fit beside a valid one
    nb = min(len(BAD_KINDS), max_rows - 1)
    bad_of = {free[0]: list(BAD_KINDS[:nb]), free[1]: list(BAD_KINDS[nb:])}
    tags += [free[0]] * (nb + 1) + [free[1]] * (len(BAD_KINDS) - nb + 1)
    for g in free[2:]:
        tags += [g] * int(rng.integers(1, min(max_rows, 12)))
    heavy = (N - len(tags)) * 2 // 3 if max_rows < 64 else 0
    tags += [GEN_HEAVY] * heavy                                    # far above max_rows
    tags += [int(x) for x in rng.integers(G_src, 1 << 32, N - len(tags), dtype=np.uint64)]
    assert len(tags) == N
    order = rng.permutation(N)
    tags = [tags[int(i)] for i in order]
    case_step = 0
    seen_vec = {}
    c = 0
    for f, t in enumerate(tags):
        # every second frame that is ingested has one of the boundary lengths
        ln = int(rng.integers(0, L + 1))
        if t < G_src and t not in (GEN_OVER, GEN_HEAVY) and not bad_of.get(t):
            ln = (L, 0, 1, 15, 16, 17)[(c // 2) % 6] if c % 2 == 0 else ln
            c += 1
        pay = rng.integers(0, 256, ln, dtype=np.uint8)
        if t >= G_src:
            p.put_sys(f, t, int(rng.integers(0, 1 << 40)), pay)
            continue
        if bad_of.get(t):
            _bad_frame(p, rng, f, t, bad_of[t].pop(0))
            continue
        if t == GEN_CASES:
            # coded v, systematic c, v again, c again (another id), the zero vector, v + e_c
            step, case_step = case_step, case_step + 1
            c = 2 % k
            v = seen_vec.setdefault(t, rng.integers(1, 256, k).astype(np.uint8))
            if step in (0, 2):
                p.put_coded(f, t, 900 + step, v, pay)
            elif step in (1, 3):
                p.put_sys(f, t, c + k * (4 + step), pay)
            elif step == 4:
                p.put_coded(f, t, 904, np.zeros(k, np.uint8), pay)
            else:
                w = v.copy()
                w[c] ^= 1
                p.put_coded(f, t, 905, w, pay)
            continue
        if rng.random() < 0.5:
            p.put_sys(f, t, int(rng.integers(0, 1 << 40)), pay)
        else:
            p.put_coded(f, t, int(rng.integers(0, 1 << 40)), rng.integers(0, 256, k).astype(np.uint8), pay)
    assert not any(bad_of.values())
    return p
