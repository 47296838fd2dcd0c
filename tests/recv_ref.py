"""Reference of the in-place receive step -- TEST INFRASTRUCTURE ONLY.

decode_ref: what qf_decode_frames_dev must report for one generation whose
rows are given as payloads of their own lengths: the rows zero padded to L,
the innovative filter of tests/rank_ref.py over the vectors, the oracle's
decode over the innovative rows, and src_slot (the innovative slot that
carries source i as a systematic row, 0xFFFF for a recovered source).
plant: one generation per planted arrival order of tests.test_rank_cpu, the
sources with zero tails of different lengths."""
from __future__ import annotations

import numpy as np

from tests import rank_ref

OK, EINVAL, ENOTREADY = 0, -1, -3
NONE16 = 0xFFFF


def pad_rows(payloads, L: int) -> np.ndarray:
    """Payloads (bytes-likes of at most L bytes) -> (n, L) zero padded."""
    rows = np.zeros((len(payloads), L), np.uint8)
    for s, p in enumerate(payloads):
        b = np.frombuffer(bytes(p), np.uint8)
        assert len(b) <= L
        rows[s, : len(b)] = b
    return rows


def decode_ref(oracle, k: int, r: int, L: int, idx, coeffs, payloads) -> dict:
    """-> status, flags (n,), rank, erased (ascending source indices), rec
    (len(erased), L), src_slot (k,) u16.  idx (n,), coeffs (n, k), payloads n
    byte strings; every index >= k needs index - k < 256."""
    idx = np.asarray(idx, np.int64)
    n = len(idx)
    out = dict(status=OK, flags=np.zeros(n, np.uint8), rank=0, erased=[], rec=np.zeros((0, L), np.uint8),
               src_slot=np.full(k, NONE16, np.uint16))
    if n and not ((idx < k) | (idx - k < 256)).all():
        out["status"] = EINVAL
        return out
    if n == 0:
        out["status"] = ENOTREADY
        return out
    V = rank_ref.vectors(k, r, idx, coeffs, None)
    out["flags"], out["rank"] = rank_ref.innovative(V)
    if out["rank"] < k:
        out["status"] = ENOTREADY
        return out
    keep = np.flatnonzero(out["flags"])
    have = {int(idx[s]): int(s) for s in keep if idx[s] < k}
    erased = [i for i in range(k) if i not in have]
    if len(erased) > min(k, r, 128):
        out["status"] = EINVAL
        return out
    rows = pad_rows(payloads, L)
    st, dec, _ = oracle.decode(k, idx[keep].astype(np.uint16), rows[keep], np.ascontiguousarray(np.asarray(coeffs)[keep]))
    assert st == OK, "the innovative rows have rank k"
    out["erased"] = erased
    out["rec"] = dec[erased].reshape(len(erased), L)
    for i, s in have.items():
        out["src_slot"][i] = s
    return out


def tailed_sources(rng, G: int, k: int, L: int) -> np.ndarray:
    """(G, k, L) random sources; source i of generation g ends in (3 g + 5 i) %
    (L // 2 + 1) zero bytes, so its frame may carry fewer than L bytes."""
    src = rng.integers(1, 256, (G, k, L), dtype=np.uint8)
    for g in range(G):
        for i in range(k):
            z = (3 * g + 5 * i) % (L // 2 + 1)
            if z:
                src[g, i, L - z:] = 0
    return src


def trimmed_len(row: np.ndarray) -> int:
    nz = np.flatnonzero(row)
    return int(nz[-1]) + 1 if nz.size else 0


def plant(oracle, rng, k: int = 16, L: int = 100):
    """-> names, src (G, k, L), idx (G, 24), coeffs (G, 24, k), V (G, 24, k),
    rows (G, 24, L) = V x src: tests.test_gpu_rank._planted with tailed sources."""
    from tests.test_rank_cpu import planted_cases

    cases = planted_cases(rng, k)
    names = list(cases)
    G, mr = len(names), 24
    src = tailed_sources(rng, G, k, L)
    idx = np.zeros((G, mr), np.uint16)
    co = np.zeros((G, mr, k), np.uint8)
    rows = np.zeros((G, mr, L), np.uint8)
    Vs = np.zeros((G, mr, k), np.uint8)
    for g, name in enumerate(names):
        V = cases[name]
        Vs[g] = V
        for s in range(mr):
            nz = np.flatnonzero(V[s])
            if nz.size == 1 and V[s, nz[0]] == 1:
                idx[g, s] = nz[0]                     # a unit vector arrives as a systematic row
                co[g, s, nz[0]] = 1
            else:
                idx[g, s] = k + 3 * s
                co[g, s] = V[s]
        rows[g] = oracle.encode(src[g], mr, np.ascontiguousarray(V))
    return names, src, idx, co, Vs, rows
