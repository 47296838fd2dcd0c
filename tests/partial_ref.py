"""Reference of the partial decode -- TEST INFRASTRUCTURE ONLY.

partial_ref: what qf_decode_partial_frames_dev must report for one generation
whose rows are given as payloads of their own lengths at offsets of a source
region.  With A the innovative slots (tests/rank_ref.py), S the sources with a
systematic slot in A, E the other sources (ascending) and the c coded slots of
A, the coded rows' columns over E are brought to reduced row echelon form,
scanning the columns left to right; a row that is zero at every column without
a pivot determines its pivot's source.  The model also produces what the
control kernel hands to the payload pass (the recorded slots, bound, min_len)
and check_records() states the contract that keeps that pass inside its
buffers.  Plain numpy with the oracle's exp / log tables."""
from __future__ import annotations

import numpy as np

from tests import rank_ref

OK, EINVAL, ENOTREADY = 0, -1, -3
NONE16 = 0xFFFF

_MUL = None


def mul_table() -> np.ndarray:
    """(256, 256) products of GF(2^8) from rank_ref's tables."""
    global _MUL
    if _MUL is None:
        e, lg = rank_ref._tables()
        a = np.arange(256)
        m = e[(lg[a][:, None] + lg[a][None, :])].astype(np.uint8)
        m[0, :] = 0
        m[:, 0] = 0
        _MUL = m
    return _MUL


def _inv(x: int) -> int:
    e, lg = rank_ref._tables()
    return int(e[255 - lg[x]])


def rref(M: np.ndarray, ncols: int):
    """Reduced row echelon form of M's first ncols columns, in place over all
    columns: pivots left to right, rows swapped into place.  -> pivot column of
    each pivot row (rows 0 .. len - 1), free columns."""
    mul = mul_table()
    rows = M.shape[0]
    piv, free = [], []
    rr = 0
    for c in range(ncols):
        nz = np.flatnonzero(M[rr:, c]) if rr < rows else np.zeros(0, np.int64)
        if nz.size == 0:
            free.append(c)
            continue
        p = rr + int(nz[0])
        if p != rr:
            M[[rr, p]] = M[[p, rr]]
        M[rr] = mul[_inv(int(M[rr, c]))][M[rr]]
        for m in range(rows):
            f = int(M[m, c])
            if m != rr and f:
                M[m] ^= mul[f][M[rr]]
        piv.append(c)
        rr += 1
    return piv, free


def partial_ref(k: int, r: int, L: int, idx, coeffs, payloads, offs=None, src_gen_stride=None) -> dict:
    """-> status, flags (n,), rank, D (ascending source indices), rec (len(D),
    L), src_slot (k,) u16, recorded (the slots the payload pass is given,
    arrival order), bound, min_len.  idx (n,), coeffs (n, k), payloads n byte
    strings; offs (n,) and src_gen_stride: where the rows lie (None: row rules
    not checked beyond the length)."""
    idx = np.asarray(idx, np.int64)
    n = len(idx)
    out = dict(status=OK, flags=np.zeros(n, np.uint8), rank=0, D=[], rec=np.zeros((0, L), np.uint8),
               src_slot=np.full(k, NONE16, np.uint16), recorded=[], bound=0, min_len=0)
    if n and not ((idx < k) | (idx - k < 256)).all():
        out["status"] = EINVAL          # the filter's rule as well: rank 0, no flags
        return out
    lens = [len(bytes(p)) for p in payloads]
    V = rank_ref.vectors(k, r, idx, np.asarray(coeffs, np.uint8).reshape(n, k), None) if n else np.zeros((0, k), np.uint8)
    if n:
        out["flags"], out["rank"] = rank_ref.innovative(V)
    bad = any(ln > L for ln in lens)
    if offs is not None:
        bad = bad or any(int(o) % 16 or int(o) + ln > src_gen_stride for o, ln in zip(offs, lens))
    if bad:
        out["status"] = EINVAL          # the vectors still give rank and flags
        return out
    A = [int(s) for s in np.flatnonzero(out["flags"])]
    have = {int(idx[s]): s for s in A if idx[s] < k}
    coded = [s for s in A if idx[s] >= k]
    c = len(coded)
    if c > min(k, 128):
        out["status"] = EINVAL
        return out
    E = [i for i in range(k) if i not in have]
    Sx = sorted(have)
    D, rows_of_D, M = [], [], None
    if c:
        M = np.concatenate([V[coded][:, E], V[coded][:, Sx], np.eye(c, dtype=np.uint8)], axis=1)
        piv, free = rref(M, len(E))
        assert len(piv) == c, "the innovative rows are independent"
        for m, pc in enumerate(piv):
            if not M[m, free].any():
                D.append(E[pc])
                rows_of_D.append(m)
        assert D == sorted(D)
    if len(D) > min(k, r):
        out["status"] = EINVAL
        return out
    out["status"] = OK if out["rank"] == k else ENOTREADY
    for i, s in have.items():
        out["src_slot"][i] = s
    if D:
        mul = mul_table()
        nE = len(E)
        slot_col = {have[i]: nE + p for p, i in enumerate(Sx)}
        slot_col.update({s: k + q for q, s in enumerate(coded)})
        W = M[rows_of_D]
        rec = np.zeros((len(D), L), np.uint8)
        for s in A:
            co = W[:, slot_col[s]]
            if not co.any():
                continue
            out["recorded"].append(s)
            row = np.zeros(L, np.uint8)
            row[: lens[s]] = np.frombuffer(bytes(payloads[s]), np.uint8)
            rec ^= mul[co][:, row]
        out["D"], out["rec"] = D, rec
        out["bound"] = len(out["recorded"])
        out["min_len"] = min(lens[s] for s in out["recorded"])
    return out


def check_records(ref: dict, offs, lens, src_gen_stride: int) -> None:
    """The contract of the payload pass's records: every recorded row's whole
    16-byte units lie inside the region, min_len is no longer than any recorded
    row, and a generation that delivers nothing records nothing."""
    if not ref["D"] or ref["status"] not in (OK, ENOTREADY):
        assert ref["recorded"] == [] and ref["bound"] == 0 and ref["min_len"] == 0
        return
    assert ref["bound"] == len(ref["recorded"]) >= 1
    for s in ref["recorded"]:
        assert int(offs[s]) % 16 == 0
        assert int(offs[s]) + 16 * ((int(lens[s]) + 15) // 16) <= src_gen_stride, s
        assert ref["min_len"] <= int(lens[s])


def encode_rows(V, src) -> np.ndarray:
    """(n, k) vectors x (k, L) sources -> (n, L) rows."""
    mul = mul_table()
    V = np.asarray(V, np.uint8)
    out = np.zeros((V.shape[0], src.shape[1]), np.uint8)
    for i in range(src.shape[0]):
        nz = np.flatnonzero(V[:, i])
        if nz.size:
            out[nz] ^= mul[V[nz, i]][:, src[i]]
    return out


def over(rng, k: int, support) -> np.ndarray:
    """A vector with random nonzero coefficients on `support`, zero elsewhere."""
    v = np.zeros(k, np.uint8)
    v[list(support)] = rng.integers(1, 256, len(support), dtype=np.uint8)
    return v


def unit(k: int, i: int) -> np.ndarray:
    v = np.zeros(k, np.uint8)
    v[i] = 1
    return v


class Gen:
    """One generation built from vectors in arrival order: a unit vector with
    coefficient 1 arrives as a systematic row, any other as a coded row with
    its vector.  The sources end in zero bytes of different lengths and a row's
    length is L (one slot in three) or the row without its trailing zeros, so
    that short and long rows occur (src given: an all-zero source makes rows of
    length 0)."""

    def __init__(self, rng, k: int, L: int, vecs, n=None, src=None):
        self.k, self.L = k, L
        vecs = [np.asarray(v, np.uint8) for v in vecs]
        self.V = np.stack(vecs) if vecs else np.zeros((0, k), np.uint8)
        self.n = len(vecs) if n is None else n
        if src is None:
            src = rng.integers(1, 256, (k, L), dtype=np.uint8)
            for i in range(k):
                z = (5 * i + int(rng.integers(0, 3))) % (L // 2 + 1)
                if z:
                    src[i, L - z:] = 0
        self.src = src
        m = len(vecs)
        self.idx = np.zeros(m, np.uint16)
        self.coeffs = np.zeros((m, k), np.uint8)
        for s, v in enumerate(vecs):
            nz = np.flatnonzero(v)
            if nz.size == 1 and v[nz[0]] == 1:
                self.idx[s] = nz[0]
                self.coeffs[s] = rng.integers(0, 256, k, dtype=np.uint8)   # ignored for a systematic row
            else:
                self.idx[s] = k + (3 * s) % 256
                self.coeffs[s] = v
        self.rows = encode_rows(self.V, src)
        self.lens = np.array([L if s % 3 == 0 else _trimmed(self.rows[s]) for s in range(m)], np.uint32)

    def payloads(self):
        return [self.rows[s, : int(self.lens[s])].tobytes() for s in range(self.n)]

    def ref(self, r: int, offs=None, src_gen_stride=None) -> dict:
        return partial_ref(self.k, r, self.L, self.idx[: self.n], self.coeffs[: self.n], self.payloads(),
                           None if offs is None else offs[: self.n], src_gen_stride)


def _trimmed(row) -> int:
    nz = np.flatnonzero(row)
    return int(nz[-1]) + 1 if nz.size else 0


def planted(rng, k: int = 16) -> dict:
    """name -> (vectors in arrival order, determined sources, undetermined
    sources) of the incomplete generations the issue lists, k = 16, S = every
    source but 3, 7, 9, 12."""
    assert k == 16
    out_of_S = [3, 7, 9, 12]
    S = [i for i in range(k) if i not in out_of_S]
    sysS = [unit(k, i) for i in S]
    dup = [unit(k, S[2]), unit(k, S[5])]                # repeated systematic rows in between
    cases = {}
    cases["one row over S + {3}"] = (sysS + dup + [over(rng, k, S + [3])], [3], [7, 9, 12])
    cases["two rows over S + {3, 7}"] = ([over(rng, k, S[:4] + [3, 7])] + sysS + [over(rng, k, S + [3, 7])], [3, 7],
                                         [9, 12])
    cases["one row over S + {3, 7}"] = (sysS[:6] + [over(rng, k, S + [3, 7])] + sysS[6:] + dup, [], out_of_S)
    a, b = over(rng, k, S + [3, 7]), over(rng, k, S + [3, 7])
    dep = (mul_table()[5][a] ^ b).astype(np.uint8)      # in the span of a and b: not innovative
    cases["two over S + {3, 7}, one over S + {9, 12}"] = (sysS + [a, b, dep, over(rng, k, S + [9, 12])], [3, 7],
                                                          [9, 12])
    S8 = list(range(8))
    cases["dense rows, fewer than the unknowns"] = (
        [unit(k, i) for i in S8] + [rng.integers(1, 256, k, dtype=np.uint8) for _ in range(5)], [], list(range(8, 16)))
    cases["systematic row after the rows that determine it"] = (
        sysS + [over(rng, k, S + [3]), unit(k, 3)], [3], [7, 9, 12])
    cases["no rows"] = ([], [], list(range(k)))
    cases["systematic rows only"] = (sysS + dup, [], out_of_S)
    return cases


def span_rank_with(V, i: int) -> int:
    """rank(V u {e_i}) by rank_ref."""
    V = np.asarray(V, np.uint8)
    e = np.zeros((1, V.shape[1]), np.uint8)
    e[0, i] = 1
    return rank_ref.innovative(np.concatenate([V, e]))[1]
