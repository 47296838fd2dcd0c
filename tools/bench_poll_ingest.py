#!/usr/bin/env python3
"""Timing of the streaming receiver's step into a poll from a flat poll buffer
(DESIGN 3.16): qf_parse_poll_headers_dev + qf_rank_update_sel_batch +
qf_store_append_sel_dev against the dense sequence a caller ran before,
qf_parse_frame_headers_dev + qf_rank_update_batch + qf_store_append_dev over
all G generations on the same poll pre-sorted by the host.

    python tools/bench_poll_ingest.py --out profiles/poll_ingest_bench.json

Workload: k = 64, L = 1,200, frame_stride 1,280, G = 65,536, max_rows 4, cap 4.
A poll of N = 2 n frames, one systematic and one coded frame for each of n
generations spread evenly over the G, in a random arrival order; n = G/64,
G/16, G/4; the list is sized n_max = n.
  (i)    the dense sequence over all G (the host sort is NOT counted; its host
         time, a numpy stable sort and one gather copy into the G * max_rows *
         frame_stride buffer, is reported separately)
  (ii)   the dense sequence over the n touched generations alone (a dense poll,
         states and stores of n generations): the work itself, without the list
  (iii)  a device-to-device copy of the payload bytes the append moves
Every sequence starts with the same qf_stream_reset_dev over the touched
generations (state and store count), so that each pass ingests the same rows;
that call is timed alone and subtracted.  Before it times anything the tool
asserts that the states and the stores of the flat path and of (i) are
identical.
Times: device events over windows of >= 0.5 s after a warm-up, medians with
min-max over the repetitions, steps alternated in one process; per-kernel times
from qf_ctx_profile.  Prints one JSON line."""
from __future__ import annotations

import argparse
import ctypes
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tools"))

import bench_recv_inplace as B  # noqa: E402

K, L, MR, CAP = 64, 1200, 4, 4
med = statistics.median


def _hip():
    """The HIP runtime the process already holds (torch's)."""
    import torch

    return ctypes.CDLL(str(Path(torch.__file__).parent / "lib" / "libamdhip64.so"))


class Side:
    """Rank states, rank array and row store of G generations."""

    def __init__(self, qf, dev, G):
        import torch

        z = lambda nb: torch.zeros(nb, dtype=torch.uint8, device=dev)   # noqa: E731
        self.G = G
        self.sb = qf.rank_state_bytes(K)
        self.rs = (L + 15) // 16 * 16
        self.state, self.rank = z(G * self.sb), z(4 * G)
        self.store, self.s_off, self.s_len = z(G * CAP * self.rs), z(4 * G * CAP), z(4 * G * CAP)
        self.s_idx, self.s_co, self.s_n = z(2 * G * CAP), z(G * CAP * K), z(4 * G)

    def arrays(self):
        return (self.state, self.rank, self.store, self.s_off, self.s_len, self.s_idx, self.s_co, self.s_n)


class Rows:
    """The outputs of a header parse over `slots` generations or entries."""

    def __init__(self, dev, slots, frames):
        import torch

        z = lambda nb: torch.zeros(nb, dtype=torch.uint8, device=dev)   # noqa: E731
        self.idx, self.n, self.co = z(2 * slots * MR), z(4 * slots), z(slots * MR * K)
        self.rl, self.ro, self.est, self.fst = z(4 * slots * MR), z(4 * slots * MR), z(4 * slots), z(4 * frames)
        self.fl, self.st, self.ast = z(slots * MR), z(4 * slots), z(4 * slots)


class Poll:
    def __init__(self, qf, ctx, G, n):
        import torch

        self.qf, self.ctx, self.G, self.n = qf, ctx, G, n
        self.N = N = 2 * n
        self.dev = dev = f"cuda:{ctx.device}"
        self.P = P = qf.frame_payload_offset(K)
        self.fs = fs = P + (L + 15) // 16 * 16
        assert fs == 1280
        rng = np.random.default_rng(2032 + n)
        touched = np.arange(0, G, G // n, dtype=np.uint32)
        order = rng.permutation(N)
        gen = np.repeat(touched, 2)[order]
        coded = (np.tile(np.array([0, 1]), n)[order]).astype(bool)
        frames = rng.integers(0, 256, (N, fs), dtype=np.uint8)
        frames[~coded, P - 1] = 1
        frames[coded, P - 3 - K: P - K] = (0, K >> 8, K & 0xFF)
        flen = np.where(coded, 3 + K + L, 1 + L).astype(np.uint32)
        foff = np.where(coded, P - 3 - K, P - 1).astype(np.uint32)
        ids = rng.integers(0, 1 << 40, N).astype(np.uint64)
        # the host sort (not counted in the yardstick; timed here on its own)
        dense_host = np.zeros((G * MR, fs), np.uint8)
        t0 = time.perf_counter()
        by_gen = np.argsort(gen, kind="stable")
        g_sorted = gen[by_gen]
        first = np.searchsorted(g_sorted, g_sorted, side="left")
        slot = g_sorted.astype(np.int64) * MR + (np.arange(N) - first)
        dense_host[slot] = frames[by_gen]
        self.host_sort_ms = (time.perf_counter() - t0) * 1e3
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)   # noqa: E731
        self.frames, self.flen, self.foff, self.ids, self.gen = up(frames), up(flen), up(foff), up(ids), up(gen)
        self.n_frames = up(np.array([N], np.uint32))
        # (i): G regions; (ii): the n touched generations alone
        meta = lambda a, regions, at: self._scatter(a, regions, at)   # noqa: E731
        at_G = slot
        rank_of = {int(g): j for j, g in enumerate(touched)}
        at_n = np.array([rank_of[int(g)] for g in g_sorted], np.int64) * MR + (np.arange(N) - first)
        self.d_frames = up(dense_host)
        del dense_host
        self.d_flen, self.d_foff, self.d_ids = (up(meta(x[by_gen], G, at_G)) for x in (flen, foff, ids))
        nfr = np.zeros(G, np.uint32)
        nfr[touched] = 2
        self.d_nfr = up(nfr)
        small = np.zeros((n * MR, fs), np.uint8)
        small[at_n] = frames[by_gen]
        self.s_frames = up(small)
        del small
        self.s_flen, self.s_foff, self.s_ids = (up(meta(x[by_gen], n, at_n)) for x in (flen, foff, ids))
        self.s_nfr = up(np.full(n, 2, np.uint32))
        self.touched = up(touched)
        self.n_touched = up(np.array([n], np.uint32))
        self.ident = up(np.arange(n, dtype=np.uint32))
        self.sel, self.n_sel = up(np.zeros(n, np.uint32)), up(np.zeros(1, np.uint32))
        self.flat, self.dense, self.only = Side(qf, dev, G), Side(qf, dev, G), Side(qf, dev, n)
        self.r_flat, self.r_dense, self.r_only = Rows(dev, n, N), Rows(dev, G, G * MR), Rows(dev, n, n * MR)

    @staticmethod
    def _scatter(vals, regions, at):
        out = np.zeros(regions * MR, vals.dtype)
        out[at] = vals
        return out

    # the steps
    def reset(self, side, sel, G_src):
        self.qf.stream_reset(sel, self.n_touched, K, n_max=self.n, G_src=G_src, state=side.state, store_n=side.s_n,
                             ctx=self.ctx)

    def dense_parse(self, r, frames, flen, foff, ids, nfr, G):
        self.qf.parse_frame_headers(frames, flen, ids, r.idx, r.n, r.fst, r.co, r.rl, r.ro, K, L, max_rows=MR,
                                    frame_stride=self.fs, G=G, n_frames=nfr, frame_off=foff, ctx=self.ctx)

    def dense_update(self, r, side):
        self.qf.rank_update_batch(r.idx, side.state, side.rank, r.st, K, max_rows=MR, G=side.G, n_rows=r.n,
                                  row_coeffs=r.co, innovative=r.fl, ctx=self.ctx)

    def dense_append(self, r, side, frames):
        self.qf.store_append(frames, r.ro, r.rl, r.idx, r.co, side.store, side.s_off, side.s_len, side.s_idx, side.s_co,
                             side.s_n, r.ast, K, L, max_rows=MR, cap=CAP, src_gen_stride=MR * self.fs,
                             store_row_stride=side.rs, store_gen_stride=CAP * side.rs, G=side.G, n_rows=r.n, take=r.fl,
                             ctx=self.ctx)

    def ingest(self):
        r = self.r_flat
        self.qf.parse_poll_headers(self.frames, self.flen, self.ids, self.gen, self.sel, self.n_sel, r.idx, r.n, r.co,
                                   r.rl, r.ro, r.est, r.fst, K, L, max_rows=MR, frame_stride=self.fs, N_max=self.N,
                                   G_src=self.G, n_max=self.n, n_frames=self.n_frames, frame_off=self.foff, ctx=self.ctx)

    def listed_update(self):
        r, side = self.r_flat, self.flat
        self.qf.rank_update_sel_batch(self.sel, self.n_sel, r.idx, side.state, r.st, K, max_rows=MR, n_max=self.n,
                                      G_src=self.G, n_rows=r.n, row_coeffs=r.co, innovative=r.fl, rank=side.rank,
                                      ctx=self.ctx)

    def listed_append(self):
        r, side = self.r_flat, self.flat
        self.qf.store_append_sel(self.sel, self.n_sel, self.frames, r.ro, r.rl, r.idx, r.co, side.store, side.s_off,
                                 side.s_len, side.s_idx, side.s_co, side.s_n, r.ast, K, L, max_rows=MR, cap=CAP,
                                 src_bytes=self.N * self.fs, store_row_stride=side.rs, store_gen_stride=CAP * side.rs,
                                 n_max=self.n, G_src=self.G, n_rows=r.n, take=r.fl, ctx=self.ctx)

    def seq_flat(self):
        self.reset(self.flat, self.touched, self.G)
        self.ingest()
        self.listed_update()
        self.listed_append()

    def seq_dense(self):
        self.reset(self.dense, self.touched, self.G)
        self.dense_parse(self.r_dense, self.d_frames, self.d_flen, self.d_foff, self.d_ids, self.d_nfr, self.G)
        self.dense_update(self.r_dense, self.dense)
        self.dense_append(self.r_dense, self.dense, self.d_frames)

    def seq_only(self):
        self.reset(self.only, self.ident, self.n)
        self.dense_parse(self.r_only, self.s_frames, self.s_flen, self.s_foff, self.s_ids, self.s_nfr, self.n)
        self.dense_update(self.r_only, self.only)
        self.dense_append(self.r_only, self.only, self.s_frames)

    def check(self):
        import torch

        self.seq_flat()
        self.seq_dense()
        self.seq_only()
        self.ctx.sync()
        i32 = lambda t: t.view(torch.int32)   # noqa: E731
        assert int(i32(self.n_sel)[0]) == self.n and torch.equal(i32(self.sel), i32(self.touched))
        for r in (self.r_flat, self.r_dense, self.r_only):
            assert (i32(r.st) == 0).all() and (i32(r.ast) == 0).all()
        assert (i32(self.r_flat.fst) == 0).all() and (i32(self.r_flat.est) == 0).all()
        for a, b in zip(self.flat.arrays(), self.dense.arrays()):
            assert torch.equal(a, b), "the flat path's states or stores differ from the dense sequence's"
        self.taken = int(i32(self.flat.s_n).sum())
        assert self.n < self.taken <= self.N and int(i32(self.only.s_n).sum()) == self.taken
        # a second pass leaves the same bytes: the reset restores the starting point
        keep = [t.clone() for t in self.flat.arrays()]
        self.seq_flat()
        self.ctx.sync()
        assert all(torch.equal(a, b) for a, b in zip(self.flat.arrays(), keep))


def run(qf, ctx, hip, G, n, reps):
    import torch

    p = Poll(qf, ctx, G, n)
    p.check()
    stream = torch.cuda.current_stream().cuda_stream
    moved = p.taken * p.flat.rs
    scratch = torch.zeros(2 * moved, dtype=torch.uint8, device=p.dev)

    def copy():
        e = hip.hipMemcpyAsync(ctypes.c_void_p(scratch.data_ptr() + moved), ctypes.c_void_p(scratch.data_ptr()),
                               ctypes.c_size_t(moved), 3, ctypes.c_void_p(stream))
        assert e == 0, f"hipMemcpyAsync: {e}"

    steps = {"reset": lambda: p.reset(p.flat, p.touched, G), "flat": p.seq_flat, "i_dense_all": p.seq_dense,
             "ii_dense_touched_only": p.seq_only, "iii_copy": copy}
    t = {name: [] for name in steps}
    ks = {name: {} for name in ("flat", "i_dense_all", "ii_dense_touched_only")}
    for _ in range(reps):
        for name, fn in steps.items():
            t[name].append(round(B.timed(fn, ctx), 5))
            if name in ks:
                for kn, ms in B.kernel_split(fn, ctx).items():
                    ks[name].setdefault(kn, []).append(ms)
    m = {name: med(v) for name, v in t.items()}
    km = {name: {kn: med(v) for kn, v in d.items()} for name, d in ks.items()}
    rel = lambda v: (max(v) - min(v)) / med(v)   # noqa: E731
    rate = moved / m["iii_copy"]                  # bytes per ms of the plain copy
    net = {name: m[name] - m["reset"] for name in ("flat", "i_dense_all", "ii_dense_touched_only")}
    N = p.N
    # metadata the list adds: tags, the zeroed counts and cursors (written and read), the frame numbers
    # (written and read), the list itself (written by the select, read by every later kernel)
    ingest_meta = 4 * N + 2 * 4 * (G + n) + 2 * 4 * N + 4 * 4 * n
    flat_k, only_k = km["flat"], km["ii_dense_touched_only"]
    ingest_ms = sum(flat_k.get(x, 0.0) for x in ("k_poll_count", "k_gen_select", "k_poll_place", "k_poll_headers"))
    rows = {}

    def row(name, got, yard, yard_runs, extra_bytes, what):
        bound = yard * (1 + rel(yard_runs)) + extra_bytes / rate
        rows[name] = {"ms": round(got, 5), "yardstick_ms": round(yard, 5), "yardstick_relative_spread": round(rel(yard_runs), 5),
                      "added_metadata_bytes": extra_bytes, "expected_ms_at_most": round(bound, 5),
                      "expectation": what, "expectation_met": bool(got <= bound)}

    row("ingest", ingest_ms, only_k["k_parse_frame_headers"], ks["ii_dense_touched_only"]["k_parse_frame_headers"],
        ingest_meta, "k_poll_count + k_gen_select + k_poll_place + k_poll_headers <= k_parse_frame_headers over the touched "
                     "generations alone * (1 + its spread) + tags, counts, cursors, frame numbers and list at the copy's rate")
    row("listed_update", flat_k["k_rank_update_sel"], only_k["k_rank_update"], ks["ii_dense_touched_only"]["k_rank_update"],
        4 * n + 4 * n, "k_rank_update_sel <= k_rank_update over the touched generations alone * (1 + its spread) + the "
                       "list and the dense rank entries at the copy's rate")
    row("listed_append", flat_k["k_store_prepare_sel"] + flat_k["k_store_rows_sel"],
        only_k["k_store_prepare"] + only_k["k_store_rows"],
        [a + b for a, b in zip(ks["ii_dense_touched_only"]["k_store_prepare"], ks["ii_dense_touched_only"]["k_store_rows"])],
        2 * 4 * n, "k_store_prepare_sel + k_store_rows_sel <= the dense pair over the touched generations alone * (1 + "
                   "its spread) + the list, read by both kernels, at the copy's rate")
    copy_ratio = flat_k["k_store_rows_sel"] / m["iii_copy"]
    desc = 8 * p.taken + 8 * n + 4 * n
    copy_bound = 1 + desc / moved + rel(t["iii_copy"])
    out = {
        "shape": {"k": K, "L": L, "frame_stride": p.fs, "G": G, "max_rows": MR, "cap": CAP, "touched": n, "frames": N,
                  "n_max": n, "rows_appended": p.taken, "payload_bytes_appended": moved},
        "states_and_stores_checked": "identical between the flat path and the dense sequence over all G, every byte of "
                                     "the rank states, the rank array, the five store arrays and store_n",
        "ms": t, "ms_median": m, "ms_min_max": {name: B.spread(v) for name, v in t.items()},
        "ms_median_without_reset": {name: round(v, 5) for name, v in net.items()},
        "kernels_ms": km,
        "ratio_flat_to_i_dense_all": round(net["flat"] / net["i_dense_all"], 4),
        "ratio_flat_to_ii_dense_touched_only": round(net["flat"] / net["ii_dense_touched_only"], 4),
        "rows": rows,
        "listed_append_to_copy": {"k_store_rows_sel_ms": flat_k["k_store_rows_sel"], "copy_ms": m["iii_copy"],
                                  "ratio": round(copy_ratio, 4), "descriptor_bytes": desc,
                                  "expectation": "k_store_rows_sel : copy <= 1 + descriptor bytes / bytes moved + the copy's "
                                                 "relative min-max spread",
                                  "expected_ratio_at_most": round(copy_bound, 4), "expectation_met": bool(copy_ratio <= copy_bound)},
        "poll_buffer_bytes": {"flat": N * p.fs + 4 * N, "dense": G * MR * p.fs},
        "host_sort_ms_not_counted": round(p.host_sort_ms, 3),
    }
    del p, scratch
    torch.cuda.empty_cache()
    return out


def main():
    import torch

    from quicfuscate_amd import fec as qf

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--generations", type=int, default=65536)
    ap.add_argument("--fractions", default="64,16,4", help="n = G / each")
    ap.add_argument("--out", default="profiles/poll_ingest_bench.json")
    a = ap.parse_args()
    assert torch.cuda.is_available()
    ctx = qf.default_context()
    hip = _hip()
    prop = torch.cuda.get_device_properties(0)
    res = {"tool": "tools/bench_poll_ingest.py", "device": torch.cuda.get_device_name(0),
           "arch": getattr(prop, "gcnArchName", ""), "compute_units": prop.multi_processor_count,
           "timing": f"device events, windows of >= 0.5 s after a warm-up, {a.reps} repetitions, steps alternated in one "
                     "process; per-kernel times from qf_ctx_profile; medians with min-max; every sequence starts with the "
                     "same qf_stream_reset_dev over the touched generations, timed alone and subtracted",
           "yardsticks": "(i) qf_parse_frame_headers_dev + qf_rank_update_batch + qf_store_append_dev over all G on the poll "
                         "pre-sorted by the host (the host sort is not counted; host_sort_ms_not_counted is a numpy stable "
                         "sort and one gather copy); (ii) the same three calls over the touched generations alone; (iii) "
                         "hipMemcpyAsync device to device of the payload bytes the append moves",
           "runs": {}}
    G = a.generations
    for f in (int(x) for x in a.fractions.split(",")):
        key = f"n_G_over_{f}"
        res["runs"][key] = r = run(qf, ctx, hip, G, G // f, a.reps)
        print(f"{key}: flat {r['ms_median_without_reset']['flat']} ms, {r['ratio_flat_to_i_dense_all']} of (i), "
              f"{r['ratio_flat_to_ii_dense_touched_only']} of (ii); " +
              ", ".join(f"{k_} {'met' if v['expectation_met'] else 'not met'}" for k_, v in r["rows"].items()) +
              f"; append:copy {r['listed_append_to_copy']['ratio']}", file=sys.stderr, flush=True)
    pts = sorted((1 / int(k_.rsplit("_", 1)[1]), v["ratio_flat_to_i_dense_all"]) for k_, v in res["runs"].items())
    below = [f for f, q in pts if q < 1]
    above = [f for f, q in pts if q >= 1]
    res["crossover_n_over_G"] = {"flat_cheaper_up_to": max(below) if below else None,
                                 "dense_cheaper_from": min(above) if above else None}
    Path(a.out).parent.mkdir(exist_ok=True, parents=True)
    Path(a.out).write_text(json.dumps(res, indent=1))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
