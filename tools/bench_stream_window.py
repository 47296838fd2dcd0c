#!/usr/bin/env python3
"""Timing of the generation window in front of the flat-poll ingest (DESIGN
3.17): qf_gen_window_dev against qf_parse_poll_headers_dev on the same poll,
and against the host scan it replaces.

    python tools/bench_stream_window.py --out profiles/stream_window_bench.json

Workload: k = 64, L = 1,200, frame_stride 1,280, G_src = 65,536, max_rows 4.  A
poll of N = 2 n frames, one systematic and one coded frame for each of n slots
spread evenly over the ring, in a random arrival order; n = G/64, G/16, G/4.
Every slot of the window holds an open generation (id = 2^40 + slot); the frames
of about a tenth of the touched slots carry the id one ring further on, so those
slots are displaced and listed as evicted, the rest are current.
  (i)   qf_parse_poll_headers_dev on the same poll with the tags the window
        wrote (n_max = n), in the same process, alternated with the window
        call.  Both are a memset plus five dependent launches and the window
        moves fewer bytes, so the expectation is
        window <= ingest * (1 + the ingest's relative min-max spread).
  (ii)  the host scan: the ids downloaded, a numpy modulo, per-slot maximum and
        compare against a host copy of the window, the tags uploaded.  Host
        wall time, reported beside the device time, not folded into a ratio.
The window call changes the window, so every timed pass starts with a device
copy of the prepared window over it; that copy is timed alone and subtracted.
Before it times anything the tool asserts that the device window, tags,
statuses and evict list equal the host scan's.
Times: device events over windows of >= 0.5 s after a warm-up, medians with
min-max over the repetitions, steps alternated in one process; per-kernel times
from qf_ctx_profile.  Prints one JSON line."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tools"))

import bench_poll_ingest as P  # noqa: E402
import bench_recv_inplace as B  # noqa: E402

K, L, MR = P.K, P.L, P.MR
CLOSED = np.uint64(1 << 63)
BASE = 1 << 40
med = statistics.median


def host_scan(ids, win, G):
    """The window rules in numpy over valid ids -> window, tags, statuses, evicted slots, displaced ids."""
    slot = (ids % np.uint64(G)).astype(np.int64)
    newest = np.zeros(G, np.uint64)
    np.maximum.at(newest, slot, ids + np.uint64(1))
    held = win & ~CLOSED
    replaced = (newest != 0) & ((win == 0) | (newest > held))
    evicted = np.flatnonzero(replaced & (win != 0) & (win >> np.uint64(63) == 0))
    new = np.where(replaced, newest, win)
    cur = new[slot]
    same = ids + np.uint64(1) == (cur & ~CLOSED)
    closed = cur >> np.uint64(63) != 0
    tags = np.where(same & ~closed, slot, 0xFFFFFFFF).astype(np.uint32)
    status = np.where(same, np.where(closed, -9, 0), -8).astype(np.int32)
    return new, tags, status, evicted.astype(np.uint32), held[evicted] - np.uint64(1)


class Poll:
    def __init__(self, qf, ctx, G, n):
        import torch

        self.qf, self.ctx, self.G, self.n = qf, ctx, G, n
        self.N = N = 2 * n
        self.dev = dev = f"cuda:{ctx.device}"
        Pp = qf.frame_payload_offset(K)
        self.fs = fs = Pp + (L + 15) // 16 * 16
        assert fs == 1280
        rng = np.random.default_rng(2033 + n)
        touched = np.arange(0, G, G // n, dtype=np.uint64)
        order = rng.permutation(N)
        slot = np.repeat(touched, 2)[order]
        coded = (np.tile(np.array([0, 1]), n)[order]).astype(bool)
        frames = rng.integers(0, 256, (N, fs), dtype=np.uint8)
        frames[~coded, Pp - 1] = 1
        frames[coded, Pp - 3 - K: Pp - K] = (0, K >> 8, K & 0xFF)
        flen = np.where(coded, 3 + K + L, 1 + L).astype(np.uint32)
        foff = np.where(coded, Pp - 3 - K, Pp - 1).astype(np.uint32)
        pkt = rng.integers(0, 1 << 40, N).astype(np.uint64)
        # the window: every slot open with cycle 0; a tenth of the touched slots get frames of cycle 1
        self.win0_host = (np.uint64(BASE + 1) + np.arange(G, dtype=np.uint64)).astype(np.uint64)
        assert BASE % G == 0
        moved_on = np.zeros(G, bool)
        moved_on[touched[rng.permutation(n)[: max(1, n // 10)]].astype(np.int64)] = True
        self.displaced = int(moved_on.sum())
        self.ids_host = (np.uint64(BASE) + slot + np.where(moved_on[slot.astype(np.int64)], np.uint64(G), np.uint64(0))
                         ).astype(np.uint64)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)   # noqa: E731
        z = lambda nb: torch.zeros(nb, dtype=torch.uint8, device=dev)                                # noqa: E731
        self.frames, self.flen, self.foff, self.pkt = up(frames), up(flen), up(foff), up(pkt)
        self.ids, self.n_frames = up(self.ids_host), up(np.array([N], np.uint32))
        self.win0, self.win = up(self.win0_host), up(self.win0_host)
        self.nem = min(N, G)
        self.gen, self.fst = z(4 * N), z(4 * N)
        self.esel, self.nev, self.eid = z(4 * self.nem), z(4), z(8 * self.nem)
        self.sel, self.n_sel = z(4 * n), z(4)
        self.rows = P.Rows(dev, n, N)

    def restore(self):
        self.win.copy_(self.win0)

    def window(self):
        self.qf.gen_window(self.ids, self.win, self.gen, self.fst, self.esel, self.nev, G_src=self.G, N_max=self.N,
                           n_evict_max=self.nem, n_frames=self.n_frames, evict_id=self.eid, ctx=self.ctx)

    def seq_window(self):
        self.restore()
        self.window()

    def ingest(self):
        r = self.rows
        self.qf.parse_poll_headers(self.frames, self.flen, self.pkt, self.gen, self.sel, self.n_sel, r.idx, r.n, r.co, r.rl,
                                   r.ro, r.est, r.fst, K, L, max_rows=MR, frame_stride=self.fs, N_max=self.N, G_src=self.G,
                                   n_max=self.n, n_frames=self.n_frames, frame_off=self.foff, ctx=self.ctx)

    def scan(self):
        """(ii): the ids come down, the host decides, the tags go up -> host ms."""
        import torch

        self.ctx.sync()
        t0 = time.perf_counter()
        ids = self.ids.cpu().numpy().view(np.uint64)
        new, tags, status, evicted, _ = host_scan(ids, self.win_host, self.G)
        self.tags_up = torch.from_numpy(tags).to(self.dev)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        self.scan_evicted = len(evicted)
        return ms

    def check(self):
        import torch

        self.seq_window()
        self.ctx.sync()
        host = lambda t, dt: t.cpu().numpy().view(dt)   # noqa: E731
        new, tags, status, evicted, displaced = host_scan(self.ids_host, self.win0_host, self.G)
        nev = int(host(self.nev, np.uint32)[0])
        assert nev == len(evicted) == self.displaced
        assert np.array_equal(host(self.win, np.uint64), new), "the device window differs from the host scan's"
        assert np.array_equal(host(self.gen, np.uint32), tags) and np.array_equal(host(self.fst, np.int32), status)
        assert (status == 0).all()
        assert np.array_equal(host(self.esel, np.uint32)[:nev], evicted)
        assert np.array_equal(host(self.eid, np.uint64)[:nev], displaced)
        self.ingest()
        self.ctx.sync()
        i32 = lambda t: t.view(torch.int32)   # noqa: E731
        assert int(i32(self.n_sel)[0]) == self.n and (i32(self.rows.fst) == 0).all() and (i32(self.rows.est) == 0).all()
        self.win_host = self.win0_host.copy()


def run(qf, ctx, G, n, reps):
    import torch

    p = Poll(qf, ctx, G, n)
    p.check()
    steps = {"restore": p.restore, "window": p.seq_window, "i_ingest": p.ingest}
    t = {name: [] for name in steps}
    ks = {"window": {}, "i_ingest": {}}
    scan = []
    for _ in range(reps):
        for name, fn in steps.items():
            t[name].append(round(B.timed(fn, ctx), 5))
            if name in ks:
                for kn, ms in B.kernel_split(fn, ctx).items():
                    ks[name].setdefault(kn, []).append(ms)
        scan.append(round(p.scan(), 4))
    m = {name: med(v) for name, v in t.items()}
    km = {name: {kn: med(v) for kn, v in d.items()} for name, d in ks.items()}
    rel = lambda v: (max(v) - min(v)) / med(v)   # noqa: E731
    win_runs = [round(a - b, 5) for a, b in zip(t["window"], t["restore"])]
    win_ms = m["window"] - m["restore"]
    bound = m["i_ingest"] * (1 + rel(t["i_ingest"]))
    N = p.N
    out = {
        "shape": {"k": K, "L": L, "frame_stride": p.fs, "G_src": G, "max_rows": MR, "touched": n, "frames": N,
                  "n_evict_max": p.nem, "slots_displaced": p.displaced},
        "outputs_checked": "the window, the tags, the statuses, the evict list and the displaced ids equal the host scan's; "
                           "the ingest lists every touched slot and accepts every frame",
        "ms": t, "ms_median": m, "ms_min_max": {name: B.spread(v) for name, v in t.items()},
        "window_ms_without_restore": round(win_ms, 5), "window_ms_without_restore_runs": win_runs,
        "kernels_ms": km,
        "row_i_ingest": {"window_ms": round(win_ms, 5), "yardstick_ms": round(m["i_ingest"], 5),
                         "yardstick_relative_spread": round(rel(t["i_ingest"]), 5), "expected_ms_at_most": round(bound, 5),
                         "expectation": "qf_gen_window_dev (net of the window restore) <= qf_parse_poll_headers_dev on the "
                                        "same poll * (1 + its relative min-max spread)",
                         "expectation_met": bool(win_ms <= bound)},
        "row_ii_host_scan": {"host_ms": scan, "host_ms_median": med(scan), "host_ms_min_max": B.spread(scan),
                             "what": "download of the ids, numpy modulo, per-slot maximum and compare against a host "
                                     "window, upload of the tags; host wall time, no ratio"},
    }
    del p
    torch.cuda.empty_cache()
    return out


def main():
    import torch

    from quicfuscate_amd import fec as qf

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--generations", type=int, default=65536)
    ap.add_argument("--fractions", default="64,16,4", help="n = G / each")
    ap.add_argument("--out", default="profiles/stream_window_bench.json")
    a = ap.parse_args()
    assert torch.cuda.is_available()
    ctx = qf.default_context()
    prop = torch.cuda.get_device_properties(0)
    res = {"tool": "tools/bench_stream_window.py", "device": torch.cuda.get_device_name(0),
           "arch": getattr(prop, "gcnArchName", ""), "compute_units": prop.multi_processor_count,
           "timing": f"device events, windows of >= 0.5 s after a warm-up, {a.reps} repetitions, steps alternated in one "
                     "process; per-kernel times from qf_ctx_profile; medians with min-max; every window pass starts with a "
                     "device copy of the prepared window, timed alone and subtracted",
           "yardsticks": "(i) qf_parse_poll_headers_dev on the same poll with the window's tags, n_max = n; (ii) the host "
                         "scan the window replaces, host wall time",
           "runs": {}}
    G = a.generations
    for f in (int(x) for x in a.fractions.split(",")):
        key = f"n_G_over_{f}"
        res["runs"][key] = r = run(qf, ctx, G, G // f, a.reps)
        row = r["row_i_ingest"]
        print(f"{key}: window {row['window_ms']} ms, ingest {row['yardstick_ms']} ms (at most {row['expected_ms_at_most']}): "
              f"{'met' if row['expectation_met'] else 'not met'}; host scan {r['row_ii_host_scan']['host_ms_median']} ms",
              file=sys.stderr, flush=True)
    Path(a.out).parent.mkdir(exist_ok=True, parents=True)
    Path(a.out).write_text(json.dumps(res, indent=1))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
