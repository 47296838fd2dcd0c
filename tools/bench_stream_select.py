#!/usr/bin/env python3
"""Timing of the streaming steps over a list: qf_gen_select_dev +
qf_decode_frames_sel_dev / qf_recode_frames_sel_dev over the n complete
generations of a row store of G, and qf_stream_reset_dev, against the dense
calls a caller runs today.

    python tools/bench_stream_select.py --out profiles/stream_select_bench.json

Workload: k = 64, L = 1,200, G = 65,536, cap = 64, the rows of shape (a) of
tools/bench_recv_inplace.py (64 patterns tiled).  The store holds the k
innovative rows of n generations spread evenly over the G and the first k / 2
of the others; n = G/64, G/16, G/4; the list is sized n_max = n and n_max = G.
  (i)    qf_decode_frames_dev over all G generations of the store (today's call)
  (ii)   qf_decode_frames_dev over a store of the n complete generations alone
  (iii)  qf_decode_frames_dev over n_max - n generations with n_rows = 0
  (iv)   a device-to-device copy of the metadata bytes k_sel_gather moves
The same for the recode at m = 16 (seeded mix), and the reset against
hipMemsetAsync of the same bytes.  Before it times anything it asserts that the
listed decode's outputs are the dense call's (i) for the listed generations and
the listed recode's those of (ii).
Times: device events over windows of >= 0.5 s after a warm-up, medians with
min-max over the repetitions, steps alternated in one process; per-kernel times
from qf_ctx_profile.  Prints one JSON line."""
from __future__ import annotations

import argparse
import ctypes
import json
import statistics
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tools"))

import bench_recv_inplace as B  # noqa: E402

SHAPE = "a_51sys_26coded_r16"
M = 16
med = statistics.median


def _hip():
    """The HIP runtime the process already holds (torch's)."""
    import torch

    return ctypes.CDLL(str(Path(torch.__file__).parent / "lib" / "libamdhip64.so"))


class Store:
    """The store of G generations with n complete ones, the store of those n alone, the outputs."""

    def __init__(self, qf, ctx, G, n):
        import torch

        K, n_sys, n_front, n_behind, planted, r, L, _, pool = B.SHAPES[SHAPE]
        assert G % pool == 0 and G % n == 0
        self.qf, self.ctx, self.K, self.L, self.G, self.n, self.r = qf, ctx, K, L, G, n, r
        self.cap = cap = K
        self.rs = rs = (L + 15) // 16 * 16
        self.gs = gs = cap * rs
        self.dev = dev = f"cuda:{ctx.device}"
        rng = np.random.default_rng(2031)
        pats = B.patterns(qf, rng, K, n_sys, n_front, n_behind, planted, pool)
        # per pattern the store of its k innovative rows in arrival order; a half-filled one is its first k / 2
        byt = rng.integers(0, 256, (pool, cap, rs), dtype=np.uint8)
        byt[:, :, L:] = 0
        off = np.tile(np.arange(cap, dtype=np.uint32) * rs, (pool, 1))
        ln = np.full((pool, cap), L, np.uint32)
        idx = np.zeros((pool, cap), np.uint16)
        co = np.zeros((pool, cap, K), np.uint8)
        for p, (pi, pv, pf) in enumerate(pats):
            rows = np.flatnonzero(pf)
            assert len(rows) == K
            idx[p], co[p] = pi[rows], pv[rows]
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(pool, -1)).to(dev)   # noqa: E731
        pool_t = [up(byt), up(off), up(ln), up(idx), up(co)]
        self.comp = comp = torch.arange(0, G, G // n, device=dev)
        pat = comp % pool
        tile = G // pool
        # (the half-filled generations hold all k rows' bytes; n_rows says how many count)
        self.big = [t.repeat(tile, 1) for t in pool_t]
        self.big_n = torch.full((G,), K // 2, dtype=torch.int32, device=dev)
        self.big_n[comp] = K
        self.small = [t[pat].contiguous() for t in pool_t]
        self.small_n = torch.full((n,), K, dtype=torch.int32, device=dev)
        self.zero_n = torch.zeros(G, dtype=torch.int32, device=dev)
        self.seen = torch.zeros(G, dtype=torch.int32, device=dev)
        self.sel = torch.zeros(G, dtype=torch.int32, device=dev)
        self.n_sel = torch.zeros(1, dtype=torch.int32, device=dev)
        self.n_match = torch.zeros(1, dtype=torch.int32, device=dev)
        self.em = em = min(K, r)
        z = lambda nb: torch.zeros(nb, dtype=torch.uint8, device=dev)   # noqa: E731
        self.z = z
        self.rec, self.ri, self.nrec, self.st = z(G * em * rs), z(2 * G * em), z(4 * G), z(4 * G)
        self.out, self.oc, self.ol = z(G * M * rs), z(G * M * K), z(4 * G * M)
        self.sb = qf.rank_state_bytes(K)
        self.state = z(G * self.sb)

    # the calls
    def select(self, n_max):
        self.qf.gen_select(self.big_n, self.sel, self.n_sel, G=self.G, min_rank=self.K, n_max=n_max, seen=self.seen,
                           n_match=self.n_match, ctx=self.ctx)

    def _dec_kw(self):
        return dict(max_rows=self.cap, src_gen_stride=self.gs, rec_row_stride=self.rs, rec_gen_stride=self.em * self.rs,
                    ctx=self.ctx)

    def _rec_kw(self):
        return dict(max_rows=self.cap, src_gen_stride=self.gs, out_row_stride=self.rs, out_gen_stride=M * self.rs,
                    seed=0x5EED, out_len=self.ol, ctx=self.ctx)

    def dense_decode(self, arrays, n_rows, G):
        b, o, l, i, c = arrays
        self.qf.decode_frames(b, o, l, i, c, self.rec, self.ri, self.nrec, self.st, self.K, self.r, self.L, G=G,
                              n_rows=n_rows, **self._dec_kw())

    def listed_decode(self, n_max):
        b, o, l, i, c = self.big
        self.qf.decode_frames_sel(self.sel, self.n_sel, b, o, l, i, c, self.rec, self.ri, self.nrec, self.st, self.K,
                                  self.r, self.L, n_max=n_max, G_src=self.G, n_rows=self.big_n, **self._dec_kw())

    def dense_recode(self, arrays, n_rows, G):
        b, o, l, i, c = arrays
        self.qf.recode_frames(b, o, l, i, c, self.out, self.oc, self.st, self.K, M, self.L, G=G, n_rows=n_rows,
                              **self._rec_kw())

    def listed_recode(self, n_max):
        b, o, l, i, c = self.big
        self.qf.recode_frames_sel(self.sel, self.n_sel, b, o, l, i, c, self.out, self.oc, self.st, self.K, M, self.L,
                                  n_max=n_max, G_src=self.G, n_rows=self.big_n, **self._rec_kw())

    def reset(self):
        self.qf.stream_reset(self.sel, self.n_sel, self.K, n_max=self.n, G_src=self.G, state=self.state,
                             store_n=self.zero_n, seen=self.seen, ctx=self.ctx)

    def gather_bytes(self):
        """Metadata bytes k_sel_gather reads (and writes): offsets, lengths, indices, vectors, counts."""
        return self.n * (self.K * (4 + 4 + 2 + self.K) + 4)

    def check(self):
        import torch

        G, n, K, em, rs = self.G, self.n, self.K, self.em, self.rs
        self.select(G)
        self.ctx.sync()
        assert int(self.n_sel[0]) == n == int(self.n_match[0]) and torch.equal(self.sel[:n].long(), self.comp)
        keep = lambda *ts: [t.clone() for t in ts]   # noqa: E731
        self.dense_decode(self.big, self.big_n, G)
        self.ctx.sync()
        d_rec, d_ri, d_nrec, d_st = keep(self.rec, self.ri, self.nrec, self.st)
        stv = d_st.view(torch.int32)
        assert (stv[self.comp] == 0).all() and int((stv == -3).sum()) == G - n
        for n_max in (n, G):
            for t in (self.rec, self.ri, self.nrec, self.st):
                t.zero_()
            self.select(n_max)
            self.listed_decode(n_max)
            self.ctx.sync()
            for got, want, w in ((self.rec, d_rec, em * rs), (self.ri, d_ri, 2 * em), (self.nrec, d_nrec, 4),
                                 (self.st, d_st, 4)):
                assert torch.equal(got.view(G, w)[:n], want.view(G, w)[self.comp]), "listed decode differs from the dense call"
            assert (self.st.view(torch.int32)[n:n_max] == -3).all()
        del d_rec, d_ri, d_nrec, d_st
        self.dense_recode(self.small, self.small_n, n)
        self.ctx.sync()
        d_out, d_oc, d_ol, d_st = keep(self.out[: n * M * rs], self.oc[: n * M * K], self.ol[: 4 * n * M], self.st[: 4 * n])
        assert (d_st.view(torch.int32) == 0).all() and d_out.any()
        for n_max in (n, G):
            for t in (self.out, self.oc, self.ol, self.st):
                t.zero_()
            self.select(n_max)
            self.listed_recode(n_max)
            self.ctx.sync()
            for got, want in ((self.out, d_out), (self.oc, d_oc), (self.ol, d_ol), (self.st, d_st)):
                assert torch.equal(got[: want.numel()], want), "listed recode differs from the dense call"
        del d_out, d_oc, d_ol, d_st
        torch.cuda.empty_cache()


def run(qf, ctx, hip, G, n, reps):
    import torch

    s = Store(qf, ctx, G, n)
    s.check()
    stream = torch.cuda.current_stream().cuda_stream
    meta = torch.zeros(2 * s.gather_bytes(), dtype=torch.uint8, device=s.dev)

    def copy_meta():
        e = hip.hipMemcpyAsync(ctypes.c_void_p(meta.data_ptr() + s.gather_bytes()), ctypes.c_void_p(meta.data_ptr()),
                               ctypes.c_size_t(s.gather_bytes()), 3, ctypes.c_void_p(stream))
        assert e == 0, f"hipMemcpyAsync: {e}"

    def memsets():
        for t, nb in ((s.state, n * s.sb), (s.zero_n, 4 * n), (s.seen, 4 * n)):
            e = hip.hipMemsetAsync(ctypes.c_void_p(t.data_ptr()), 0, ctypes.c_size_t(nb), ctypes.c_void_p(stream))
            assert e == 0, f"hipMemsetAsync: {e}"

    steps = {
        "select": lambda: s.select(n),
        "dec_i_dense_all": lambda: s.dense_decode(s.big, s.big_n, G),
        "dec_ii_dense_complete_only": lambda: s.dense_decode(s.small, s.small_n, n),
        "dec_iii_dense_empty": lambda: s.dense_decode(s.big, s.zero_n, G - n),
        "iv_copy_metadata": copy_meta,
        "dec_listed_nmax_n": lambda: (s.select(n), s.listed_decode(n)),
        "dec_listed_nmax_G": lambda: (s.select(G), s.listed_decode(G)),
        "rec_i_dense_all": lambda: s.dense_recode(s.big, s.big_n, G),
        "rec_ii_dense_complete_only": lambda: s.dense_recode(s.small, s.small_n, n),
        "rec_iii_dense_empty": lambda: s.dense_recode(s.big, s.zero_n, G - n),
        "rec_listed_nmax_n": lambda: (s.select(n), s.listed_recode(n)),
        "rec_listed_nmax_G": lambda: (s.select(G), s.listed_recode(G)),
        "reset_listed": lambda: (s.select(n), s.reset()),
        "reset_memsets": memsets,
    }
    t = {name: [] for name in steps}
    ks = {name: {} for name in ("dec_listed_nmax_n", "dec_listed_nmax_G", "rec_listed_nmax_n", "rec_listed_nmax_G",
                                "dec_i_dense_all", "dec_ii_dense_complete_only", "reset_listed")}
    for _ in range(reps):
        for name, fn in steps.items():
            t[name].append(round(B.timed(fn, ctx), 5))
            if name in ks:
                for kn, ms in B.kernel_split(fn, ctx).items():
                    ks[name].setdefault(kn, []).append(ms)
    m = {name: med(v) for name, v in t.items()}
    out = {
        "shape": {"k": s.K, "L": s.L, "G": G, "cap": s.cap, "r": s.r, "m": M, "complete": n,
                  "rows_of_the_others": s.K // 2, "store_row_stride": s.rs, "gathered_metadata_bytes": s.gather_bytes(),
                  "reset_bytes": n * (s.sb + 8)},
        "outputs_checked": "listed decode = qf_decode_frames_dev over all G for the listed generations; listed recode = "
                           "qf_recode_frames_dev over the complete generations alone; n_max = n and n_max = G",
        "ms": t, "ms_median": m, "ms_min_max": {name: B.spread(v) for name, v in t.items()},
        "kernels_ms": {name: {kn: med(v) for kn, v in d.items()} for name, d in ks.items()},
    }
    for kind in ("dec", "rec"):
        ii = t[f"{kind}_ii_dense_complete_only"]
        spread_ii = (max(ii) - min(ii)) / med(ii)
        for nm, iii in (("n", 0.0), ("G", m[f"{kind}_iii_dense_empty"])):
            listed = m[f"{kind}_listed_nmax_{nm}"]
            bound = med(ii) * (1 + spread_ii) + iii + 2 * m["iv_copy_metadata"] + m["select"]
            out[f"{kind}_nmax_{nm}"] = {
                "select_plus_listed_ms": listed, "i_ms": m[f"{kind}_i_dense_all"], "ii_ms": med(ii),
                "ii_relative_spread": round(spread_ii, 5), "iii_ms": iii, "iv_ms": m["iv_copy_metadata"],
                "select_ms": m["select"], "ratio_to_i": round(listed / m[f"{kind}_i_dense_all"], 4),
                "ratio_to_ii": round(listed / med(ii), 4),
                "expectation": "select + listed call <= (ii) * (1 + (ii)'s relative min-max spread) + (iii) + 2 * (iv) + select",
                "expected_ms_at_most": round(bound, 5), "expectation_met": bool(listed <= bound),
            }
    out["reset"] = {"select_plus_reset_ms": m["reset_listed"], "select_ms": m["select"],
                    "k_stream_reset_ms": out["kernels_ms"]["reset_listed"].get("k_stream_reset"),
                    "memsets_ms": m["reset_memsets"]}
    del s, meta
    torch.cuda.empty_cache()
    return out


def main():
    import torch

    from quicfuscate_amd import fec as qf

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--generations", type=int, default=65536)
    ap.add_argument("--fractions", default="64,16,4", help="n = G / each")
    ap.add_argument("--out", default="profiles/stream_select_bench.json")
    a = ap.parse_args()
    assert torch.cuda.is_available()
    ctx = qf.default_context()
    hip = _hip()
    prop = torch.cuda.get_device_properties(0)
    res = {"tool": "tools/bench_stream_select.py", "device": torch.cuda.get_device_name(0),
           "arch": getattr(prop, "gcnArchName", ""), "compute_units": prop.multi_processor_count,
           "timing": f"device events, windows of >= 0.5 s after a warm-up, {a.reps} repetitions, steps alternated in "
                     "one process; per-kernel times from qf_ctx_profile; medians with min-max",
           "yardsticks": "(i) qf_decode_frames_dev / qf_recode_frames_dev over all G generations of the store; (ii) over a "
                         "store of the n complete generations alone; (iii) over n_max - n generations with n_rows = 0; "
                         "(iv) hipMemcpyAsync device to device of the gathered metadata bytes; hipMemsetAsync of the "
                         "reset's bytes",
           "runs": {}}
    G = a.generations
    for f in (int(x) for x in a.fractions.split(",")):
        key = f"n_G_over_{f}"
        res["runs"][key] = r = run(qf, ctx, hip, G, G // f, a.reps)
        for which in ("dec_nmax_n", "dec_nmax_G", "rec_nmax_n", "rec_nmax_G"):
            d = r[which]
            print(f"{key} {which}: {d['select_plus_listed_ms']:.4f} ms, {d['ratio_to_i']} of (i), {d['ratio_to_ii']} of (ii), "
                  f"bound {d['expected_ms_at_most']} ({'met' if d['expectation_met'] else 'not met'})", file=sys.stderr,
                  flush=True)
    # the crossover: the n / G above which the dense call over all G is the cheaper one
    for which in ("dec_nmax_n", "dec_nmax_G", "rec_nmax_n", "rec_nmax_G"):
        pts = [(1 / int(k.rsplit("_", 1)[1]), v[which]["ratio_to_i"]) for k, v in res["runs"].items()]
        pts.sort()
        below = [f for f, q in pts if q < 1]
        above = [f for f, q in pts if q >= 1]
        res.setdefault("crossover_n_over_G", {})[which] = {
            "listed_cheaper_up_to": max(below) if below else None, "dense_cheaper_from": min(above) if above else None}
    Path(a.out).parent.mkdir(exist_ok=True, parents=True)
    Path(a.out).write_text(json.dumps(res, indent=1))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
