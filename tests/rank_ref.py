"""Reference of the innovative-row rule -- TEST INFRASTRUCTURE ONLY.

innovative(V): the rows of V (n x k, GF(2^8)) in arrival order; a row is
innovative iff it is not in the span of the rows before it.  Plain numpy
elimination with the oracle's exp / log tables: each row is reduced by the
stored normalised pivot rows, and the first nonzero column of what is left
becomes the new pivot.  Importing this module needs nothing built; the first
call loads the oracle (the `oracle` fixture builds it)."""
from __future__ import annotations

import numpy as np

_TAB = None


def _tables():
    global _TAB
    if _TAB is None:
        from tests import oracle_py

        e, lg = oracle_py.tables()
        _TAB = (e.astype(np.int64), lg.astype(np.int64))
    return _TAB


def _scale(row: np.ndarray, c: int) -> np.ndarray:
    """c * row over GF(2^8), c != 0."""
    e, lg = _tables()
    out = e[lg[row] + int(lg[c])].astype(np.uint8)
    out[row == 0] = 0
    return out


def innovative(V) -> tuple[np.ndarray, int]:
    """-> (flags (n,) uint8, rank)."""
    e, lg = _tables()
    V = np.asarray(V, np.uint8)
    n, k = V.shape
    flags = np.zeros(n, np.uint8)
    pivots: list[tuple[int, np.ndarray]] = []   # (pivot column, row with a 1 there), arrival order
    for s in range(n):
        v = V[s].copy()
        for col, row in pivots:
            if v[col]:
                v ^= _scale(row, int(v[col]))
        nz = np.flatnonzero(v)
        if nz.size == 0:
            continue
        col = int(nz[0])
        inv = int(e[255 - lg[v[col]]])
        pivots.append((col, _scale(v, inv)))
        flags[s] = 1
    return flags, len(pivots)


def vectors(k: int, r: int, idx, coeffs, cauchy) -> np.ndarray:
    """The n x k vectors of one generation's slots: idx (n,), coeffs (n, k) or
    None, cauchy = the (r, k) Cauchy matrix or None."""
    idx = np.asarray(idx)
    V = np.zeros((len(idx), k), np.uint8)
    for s, i in enumerate(idx.tolist()):
        if i < k:
            V[s, i] = 1
        elif coeffs is not None:
            V[s] = coeffs[s]
        else:
            V[s] = cauchy[i - k]
    return V
