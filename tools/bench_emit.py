#!/usr/bin/env python3
"""Timing of the send step: qf_emit_frames_sel_dev behind
qf_recode_frames_sel_dev for n listed generations of a row store of G.

    python tools/bench_emit.py --out profiles/emit_bench.json

Workload: tools/bench_stream_select.py's store (k = 64, 1,200-byte rows, G =
65,536), m = 16 recoded rows per listed generation, n = G/64, G/16, G/4, the
list sized n_max = n, the queue N_max = n * m.  Reported:
  (a) k_emit_frames against one contiguous device-to-device hipMemcpyAsync of
      the frames' bytes (n * m * (3 + k + L)), with the expectation
      ratio <= 1 + record bytes / bytes moved + the copy's relative spread
      (record bytes: 16 per frame; bytes moved: read + written);
  (b) the whole call against qf_frame_rows_dev in copy mode over the same
      n_max x m grid (the way to the same bytes without this call), and against
      the listed recode in front of it;
  (c) the host step it replaces, by wall clock: the four downloads (n_sel,
      status, ids, frame_len) plus a vectorised numpy scan for the slots that
      hold a frame; and, with a budget that lets each generation emit 1 .. m
      frames, the whole grid's device-to-host copy against the compact queue's.
The calls are timed without the budget arrays (with them a repeated call emits
nothing); they cost two loads per entry in k_emit_count and one store in
k_emit_place.  Before it times anything the tool asserts the call's outputs:
every frame, length, offset, id and packet id against qf_frame_rows_dev's grid
and the inputs on the device, a sample of entries against tests/emit_ref.py,
and with a budget the counts, sent and a second call that emits nothing.
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
import bench_stream_select as S  # noqa: E402

med = statistics.median
M = S.M


class Emit:
    """The store of bench_stream_select, its listed recode, the queue and the grid."""

    def __init__(self, qf, ctx, G, n):
        import torch

        self.s = s = S.Store(qf, ctx, G, n)
        self.qf, self.ctx, self.G, self.n = qf, ctx, G, n
        K, L, z = s.K, s.L, s.z
        self.P = qf.frame_payload_offset(K)
        self.fs = self.P + s.rs
        self.N = N = n * M
        i32 = lambda c: torch.zeros(c, dtype=torch.int32, device=s.dev)   # noqa: E731
        i64 = lambda c: torch.zeros(c, dtype=torch.int64, device=s.dev)   # noqa: E731
        self.frames, self.flen, self.foff, self.fid, self.fpkt = z(N * self.fs), i32(N), i32(N), i64(N), i64(N)
        self.nfr, self.left, self.first, self.count, self.est = i32(1), i32(1), i32(n), i32(n), i32(n)
        self.grid, self.glen, self.goff = z(N * self.fs), i32(N), i32(N)
        self.ids = torch.arange(n, dtype=torch.int64, device=s.dev) * 3 + (1 << 40)
        self.rank, self.sent = i32(G), i32(G)

    def emit(self, budget=False):
        s, n = self.s, self.n
        self.qf.emit_frames_sel(s.sel, s.n_sel, s.out, self.ids, self.frames, self.flen, self.foff, self.fid, self.fpkt,
                                self.nfr, self.first, self.count, self.est, s.K, s.L, n_max=n, G_src=self.G, max_rows=M,
                                N_max=self.N, row_stride=s.rs, rows_gen_stride=M * s.rs, frame_stride=self.fs,
                                row_coeffs=s.oc, row_len=s.ol, in_status=s.st, n_left=self.left,
                                rank=self.rank if budget else None, sent=self.sent if budget else None, ctx=self.ctx)

    def frame_rows(self):
        s, n = self.s, self.n
        self.qf.frame_rows(s.out, self.grid, self.glen, s.K, s.L, max_rows=M, row_stride=s.rs, rows_gen_stride=M * s.rs,
                           frame_stride=self.fs, G=n, row_coeffs=s.oc, row_len=s.ol, frame_off=self.goff, ctx=self.ctx)

    def check(self):
        import torch

        from tests import emit_ref as R

        s, n, N, fs = self.s, self.n, self.N, self.fs
        K, L, rs = s.K, s.L, s.rs
        s.select(n)
        s.listed_recode(n)
        self.ctx.sync()
        assert int(s.n_sel[0]) == n and (s.st.view(torch.int32)[:n] == 0).all()
        for t in (self.frames, self.grid):
            t.fill_(0xCC)
        self.emit()
        self.frame_rows()
        self.ctx.sync()
        # every frame: all entries emit m frames, so queue slot j * m + s is grid slot (j, s)
        assert int(self.nfr[0]) == N and int(self.left[0]) == 0 and (self.est == 0).all() and (self.count == M).all()
        assert torch.equal(self.first, torch.arange(n, dtype=torch.int32, device=s.dev) * M)
        assert torch.equal(self.frames, self.grid), "an emitted frame differs from qf_frame_rows_dev's"
        assert torch.equal(self.flen, self.glen) and torch.equal(self.foff, self.goff)
        assert (self.flen == 3 + K + L).all() and (self.foff == self.P - 3 - K).all()
        assert torch.equal(self.fid, self.ids.repeat_interleave(M)) and (self.fpkt == 0).all()
        fr = self.frames.view(N, fs)
        assert torch.equal(fr[:, self.P: self.P + L], s.out[: N * rs].view(N, rs)[:, :L])
        assert torch.equal(fr[:, self.P - K: self.P], s.oc[: N * K].view(N, K))
        # a sample of entries against the model
        h = lambda t, dt=np.uint8: t.cpu().numpy().view(dt)   # noqa: E731
        sample = sorted({0, 1, n // 3, n // 2, n - 2, n - 1} & set(range(n)))
        rows = np.concatenate([h(s.out[j * M * rs: (j + 1) * M * rs]) for j in sample])
        c = R.Call(K, L, M, len(sample), self.G, len(sample) * M, rs, M * rs, fs, [int(s.sel[j]) for j in sample], rows,
                   [int(self.ids[j]) for j in sample],
                   row_coeffs=np.concatenate([h(s.oc[j * M * K: (j + 1) * M * K]) for j in sample]),
                   row_len=np.concatenate([h(s.ol[4 * j * M: 4 * (j + 1) * M], np.uint32) for j in sample]),
                   in_status=np.zeros(len(sample), np.int32))
        want = c.model()
        for t, j in enumerate(sample):
            assert np.array_equal(h(self.frames[j * M * fs: (j + 1) * M * fs]), want["frames"][t * M * fs: (t + 1) * M * fs]), j
            assert np.array_equal(h(self.flen[j * M: (j + 1) * M], np.uint32), want["frame_len"][t * M: (t + 1) * M])
        # with a budget: 1 .. m frames per generation, then nothing
        sel = s.sel[:n].long()
        self.rank[sel] = torch.arange(n, dtype=torch.int32, device=s.dev) % M + 1
        self.sent.zero_()
        self.frames.fill_(0xCC)
        self.emit(budget=True)
        self.ctx.sync()
        assert torch.equal(self.count, self.rank[sel]) and torch.equal(self.sent[sel], self.rank[sel])
        self.n_budget = int(self.nfr[0])
        assert self.n_budget == int(self.count.sum()) and int(self.sent.sum()) == self.n_budget
        assert (fr[self.n_budget:] == 0xCC).all() and torch.equal(self.fid[: self.n_budget],
                                                                 self.ids.repeat_interleave(self.count.long()))
        self.frames.fill_(0xCC)
        self.emit(budget=True)
        self.ctx.sync()
        assert int(self.nfr[0]) == 0 and (self.count == 0).all() and (self.frames == 0xCC).all()
        self.emit()
        self.ctx.sync()


def host_step(e, pinned):
    """What a host does without the call: the four arrays down, a scan for the grid slots that hold a frame;
    then the grid's device-to-host copy against the compact queue's (the budgeted call's length)."""
    import torch

    s, n = e.s, e.n
    t0 = time.perf_counter()
    n_sel = int(s.n_sel.cpu()[0])
    st = s.st[: 4 * n].cpu().numpy().view(np.int32)
    ids = e.ids.cpu().numpy()
    flen = e.glen.cpu().numpy().reshape(n, M)
    t1 = time.perf_counter()
    ok = (np.arange(n) < n_sel) & (st == 0) & (ids < (1 << 62))
    jj, ss = np.nonzero((flen > 0) & ok[:, None])
    slot = jj * M + ss
    t2 = time.perf_counter()
    assert slot.size == n * M
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    pinned.copy_(e.grid, non_blocking=True)
    torch.cuda.synchronize()
    t4 = time.perf_counter()
    nb = e.n_budget * e.fs
    pinned[:nb].copy_(e.frames[:nb], non_blocking=True)
    torch.cuda.synchronize()
    t5 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t4 - t3) * 1e3, (t5 - t4) * 1e3


def run(qf, ctx, hip, G, n, reps):
    import torch

    e = Emit(qf, ctx, G, n)
    s = e.s
    e.check()
    stream = torch.cuda.current_stream().cuda_stream
    nbytes = e.N * (3 + s.K + s.L)
    a, b = torch.zeros(nbytes, dtype=torch.uint8, device=s.dev), torch.zeros(nbytes, dtype=torch.uint8, device=s.dev)
    pinned = torch.empty(e.N * e.fs, dtype=torch.uint8, pin_memory=True)

    def copy():
        err = hip.hipMemcpyAsync(ctypes.c_void_p(b.data_ptr()), ctypes.c_void_p(a.data_ptr()), ctypes.c_size_t(nbytes), 3,
                                 ctypes.c_void_p(stream))
        assert err == 0, f"hipMemcpyAsync: {err}"

    steps = {"copy_same_bytes": copy, "emit": e.emit, "frame_rows_grid": e.frame_rows,
             "listed_recode": lambda: s.listed_recode(n)}
    t = {name: [] for name in steps}
    ks, host = {}, []
    for _ in range(reps):
        for name, fn in steps.items():
            t[name].append(round(B.timed(fn, ctx), 5))
        for kn, ms in B.kernel_split(e.emit, ctx).items():
            ks.setdefault(kn, []).append(ms)
        ctx.sync()
        host.append(host_step(e, pinned))
    m = {name: med(v) for name, v in t.items()}
    kms = {kn: med(v) for kn, v in ks.items()}
    cp = t["copy_same_bytes"]
    spread = (max(cp) - min(cp)) / med(cp)
    rec_share = 16 / (2 * (3 + s.K + s.L))
    fr = kms["k_emit_frames"]
    bound = 1 + rec_share + spread
    hm = lambda i: med([x[i] for x in host])   # noqa: E731
    out = {
        "shape": {"k": s.K, "L": s.L, "G": G, "m": M, "listed": n, "n_max": n, "N_max": e.N, "frame_stride": e.fs,
                  "frames": e.N, "frame_bytes": nbytes, "record_bytes": 16 * e.N, "frames_with_budget_1_to_m": e.n_budget},
        "outputs_checked": "every frame, length, offset, id and packet id against qf_frame_rows_dev's grid and the inputs; a "
                           "sample against tests/emit_ref.py; with a budget the counts and sent, and a second call emits "
                           "nothing and writes no frame byte",
        "ms": t, "ms_median": m, "ms_min_max": {name: B.spread(v) for name, v in t.items()},
        "kernels_ms": kms, "kernels_ms_min_max": {kn: B.spread(v) for kn, v in ks.items()},
        "a_frames_against_copy": {
            "k_emit_frames_ms": fr, "copy_ms": med(cp), "copy_relative_spread": round(spread, 5),
            "ratio": round(fr / med(cp), 4), "GBps_read_plus_written": round(2 * nbytes / fr / 1e6, 1),
            "expectation": "ratio <= 1 + record bytes / bytes moved + the copy's relative min-max spread",
            "expected_ratio_at_most": round(bound, 4), "expectation_met": bool(fr / med(cp) <= bound)},
        "b_call_against_frame_rows": {
            "emit_ms": m["emit"], "k_emit_count_ms": kms["k_emit_count"], "k_emit_place_ms": kms["k_emit_place"],
            "frame_rows_grid_ms": m["frame_rows_grid"], "ratio": round(m["emit"] / m["frame_rows_grid"], 4),
            "listed_recode_ms": m["listed_recode"], "ratio_to_listed_recode": round(m["emit"] / m["listed_recode"], 4)},
        "c_host_step_replaced": {
            "downloads_ms": hm(0), "scan_ms": hm(1), "host_ms": med([x[0] + x[1] for x in host]),
            "host_ms_min_max": B.spread([round(x[0] + x[1], 4) for x in host]),
            "grid_to_host_ms": hm(2), "grid_bytes": e.N * e.fs, "queue_to_host_ms": hm(3),
            "queue_bytes": e.n_budget * e.fs, "emit_ms": m["emit"],
            "note": "host wall time; the copies go to pinned host memory; the queue is the budgeted call's (1 .. m "
                    "frames per generation), the grid the n_max x m slots a host copies down whole without it"},
    }
    del e, s, a, b, pinned
    torch.cuda.empty_cache()
    return out


def main():
    import torch

    from quicfuscate_amd import fec as qf

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--generations", type=int, default=65536)
    ap.add_argument("--fractions", default="64,16,4", help="n = G / each")
    ap.add_argument("--out", default="profiles/emit_bench.json")
    a = ap.parse_args()
    assert torch.cuda.is_available()
    ctx = qf.default_context()
    hip = S._hip()
    prop = torch.cuda.get_device_properties(0)
    res = {"tool": "tools/bench_emit.py", "device": torch.cuda.get_device_name(0),
           "arch": getattr(prop, "gcnArchName", ""), "compute_units": prop.multi_processor_count,
           "timing": f"device events, windows of >= 0.5 s after a warm-up, {a.reps} repetitions, steps alternated in one "
                     "process; per-kernel times from qf_ctx_profile; medians with min-max; the host step by wall clock",
           "runs": {}}
    G = a.generations
    for f in (int(x) for x in a.fractions.split(",")):
        key = f"n_G_over_{f}"
        res["runs"][key] = r = run(qf, ctx, hip, G, G // f, a.reps)
        ra, rb, rc = r["a_frames_against_copy"], r["b_call_against_frame_rows"], r["c_host_step_replaced"]
        print(f"{key}: frames {ra['k_emit_frames_ms']:.4f} ms, {ra['ratio']} of the copy (bound "
              f"{ra['expected_ratio_at_most']}, {'met' if ra['expectation_met'] else 'not met'}); call {rb['emit_ms']:.4f} ms, "
              f"{rb['ratio']} of frame_rows, {rb['ratio_to_listed_recode']} of the recode; host step {rc['host_ms']:.3f} ms, "
              f"grid down {rc['grid_to_host_ms']:.2f} ms, queue down {rc['queue_to_host_ms']:.2f} ms",
              file=sys.stderr, flush=True)
    Path(a.out).parent.mkdir(exist_ok=True, parents=True)
    Path(a.out).write_text(json.dumps(res, indent=1))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
