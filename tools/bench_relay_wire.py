#!/usr/bin/env python3
"""Timing of the device wire step of a relay: k_parse_frames_coded,
k_frame_rows and the frames-in, frames-out relay step.

    python tools/bench_relay_wire.py --out profiles/relay_wire_bench.json

Shape: k = 64, 64 held rows per generation (51 systematic + 13 coded), m = 16
recoded packets, L = 1,200, G = 65,536.
  (1) k_parse_frames_coded against its yardstick, k_parse_frames, on the same
      buffer of pure-Cauchy frames (51 systematic + 13 Cauchy repairs of
      (64, 16) per generation, frames at byte 0 of their slots): both calls
      accept those frames.  Expectation: the new median is at most the
      yardstick's median x (1 + extra bytes / yardstick bytes) plus the
      yardstick's own min-max spread; the extra bytes are the k vector bytes
      and the 4 length bytes per row.  Also the new kernel on the relay's real
      input (arbitrary vectors, payload-aligned slots with frame_off).
  (2) k_frame_rows on the same m = 16 rows per generation, in place and in
      copy mode, with each mode's bytes moved over 8 TB/s.
  (3) The relay step: parse, recode into the frame slots, in-place framing;
      call times, kernel times and the share of the two wire kernels.
Times are device events over windows of at least 0.5 s after a warm-up,
repetitions alternated with the yardstick in one process; per-kernel times
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

K, R, L, G, M = 64, 16, 1200, 65536, 16
N_SYS, N_CODED = 51, 13
HELD = N_SYS + N_CODED
POOL = 64          # distinct generation patterns, tiled over the batch
HBM_TBPS = 8.0


def timed(fn, ctx, min_s=0.5, warmup=2):
    """ms per call of fn over a window of >= min_s (device events)."""
    import torch

    for _ in range(warmup):
        fn()
    ctx.sync()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    calls, total = 0, 0.0
    n = 1
    while total < min_s * 1e3:
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        total += e0.elapsed_time(e1)
        calls += n
        n = min(64, n * 2)
    return total / calls


def kernel_split(fn, ctx, calls=4):
    """{kernel: ms per call} with the context's profiling on."""
    ctx.sync()
    ctx.profile(True)
    for _ in range(calls):
        fn()
    times = ctx.kernel_times()
    ctx.profile(False)
    return {n: round(ms / calls, 5) for n, (_, ms) in times.items()}


def frame_pool(qf, rng, fs, aligned):
    """POOL generations of HELD frames each, 51 systematic and 13 coded in a
    shuffled order -> (frames (POOL, HELD, fs), len, off, ids).  aligned: the
    payload-aligned layout with arbitrary vectors (a relay's input from an
    upstream relay); else frames at byte 0 with Cauchy rows of (K, R)."""
    P = qf.frame_payload_offset(K)
    C = np.frombuffer(qf.cauchy_coefficients(K, R), np.uint8).reshape(R, K)
    fr = np.zeros((POOL, HELD, fs), np.uint8)
    ln = np.zeros((POOL, HELD), np.uint32)
    off = np.zeros((POOL, HELD), np.uint32)
    ids = np.zeros((POOL, HELD), np.uint64)
    for g in range(POOL):
        sys_idx = rng.permutation(K)[:N_SYS]
        order = rng.permutation(HELD)
        for what, s in enumerate(order):
            pay = rng.integers(0, 256, L, dtype=np.uint8)
            if what < N_SYS:
                head = np.array([1], np.uint8)
                ids[g, s] = 7 * K + int(sys_idx[what])
            else:
                vec = rng.integers(0, 256, K, dtype=np.uint8) if aligned else C[what - N_SYS]
                head = np.concatenate([np.array([0, K >> 8, K & 0xFF], np.uint8), vec])
                ids[g, s] = 100000 + what
            o = P - len(head) if aligned else 0
            fr[g, s, o: o + len(head)] = head
            fr[g, s, o + len(head): o + len(head) + L] = pay
            ln[g, s], off[g, s] = len(head) + L, o
    return fr, ln, off, ids


def main():
    import torch

    from quicfuscate_amd import _lib as Lb
    from quicfuscate_amd import fec as qf

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="profiles/relay_wire_bench.json")
    a = ap.parse_args()
    assert torch.cuda.is_available()
    ctx = qf.default_context()
    lib = Lb._lib()
    dev = f"cuda:{ctx.device}"
    rng = np.random.default_rng(2027)
    P = qf.frame_payload_offset(K)
    fs = P + L                      # 1,280: also round_up(3 + K + L, 16), the yardstick's slot
    assert fs % 16 == 0 and fs >= 3 + K + L
    tile = G // POOL

    def up(x):
        return torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).to(dev).repeat(tile)

    y_fr, y_ln, _, y_ids = frame_pool(qf, rng, fs, aligned=False)
    r_fr, r_ln, r_off, r_ids = frame_pool(qf, rng, fs, aligned=True)
    t_yfr, t_yln, t_yids = up(y_fr), up(y_ln), up(y_ids)
    t_rfr, t_rln, t_roff, t_rids = up(r_fr), up(r_ln), up(r_off), up(r_ids)
    z = lambda n: torch.zeros(n, dtype=torch.uint8, device=dev)   # noqa: E731
    rows, idx, n_rows, fst = z(G * HELD * L), z(2 * G * HELD), z(4 * G), z(4 * G * HELD)
    coeffs, row_len = z(G * HELD * K), z(4 * G * HELD)
    pkw = dict(max_rows=HELD, frame_stride=fs, row_stride=L, rows_gen_stride=HELD * L, G=G, ctx=ctx)

    def parse_new_cauchy():
        qf.parse_frames_coded(t_yfr, t_yln, t_yids, rows, idx, n_rows, fst, coeffs, K, L, row_len=row_len, **pkw)

    def parse_old_cauchy():
        Lb.check(lib.qf_parse_frames_dev(ctx.handle, K, R, L, G, HELD, t_yfr.data_ptr(), fs, t_yln.data_ptr(),
                                         t_yids.data_ptr(), None, rows.data_ptr(), L, HELD * L, idx.data_ptr(),
                                         n_rows.data_ptr(), fst.data_ptr()), "parse_frames")

    def parse_relay():
        qf.parse_frames_coded(t_rfr, t_rln, t_rids, rows, idx, n_rows, fst, coeffs, K, L, frame_off=t_roff,
                              row_len=row_len, **pkw)

    out_frames, out_coeffs, rstat = z(G * M * fs), z(G * M * K), z(4 * G)
    out_len, out_off = z(4 * G * M), z(4 * G * M)
    dense, copy_frames = z(G * M * L), z(G * M * fs)
    seed = 12345

    def recode():
        qf.recode_batch(rows, idx, out_frames[P:], out_coeffs, rstat, K, M, L, max_rows=HELD, row_stride=L,
                        rows_gen_stride=HELD * L, out_row_stride=fs, out_gen_stride=M * fs, G=G, n_rows=n_rows,
                        row_coeffs=coeffs, seed=seed, ctx=ctx)

    def frame_in_place():
        qf.frame_rows(None, out_frames, out_len, K, L, max_rows=M, frame_stride=fs, G=G, row_coeffs=out_coeffs,
                      frame_off=out_off, in_place=True, ctx=ctx)

    def frame_copy():
        qf.frame_rows(dense, copy_frames, out_len, K, L, max_rows=M, row_stride=L, rows_gen_stride=M * L,
                      frame_stride=fs, G=G, row_coeffs=out_coeffs, frame_off=out_off, ctx=ctx)

    def relay_step():
        parse_relay()
        recode()
        frame_in_place()

    # the rows both framing modes work on: the recoder's output, also dense for copy mode
    parse_relay()
    recode()
    qf.recode_batch(rows, idx, dense, out_coeffs, rstat, K, M, L, max_rows=HELD, row_stride=L,
                    rows_gen_stride=HELD * L, out_row_stride=L, out_gen_stride=M * L, G=G, n_rows=n_rows,
                    row_coeffs=coeffs, seed=seed, ctx=ctx)
    frame_in_place()
    frame_copy()
    ctx.sync()
    assert (fst.view(torch.int32) == 0).all() and (n_rows.view(torch.int32) == HELD).all()
    assert (rstat.view(torch.int32) == 0).all()
    assert torch.equal(out_frames, copy_frames), "in-place and copy-mode frames differ"
    # both parsers give the same rows and indices on the Cauchy frames, up to the
    # index of a repair (k + j against k) -- and the new one the vectors
    parse_old_cauchy()
    ctx.sync()
    rows_old, n_old = rows.clone(), n_rows.clone()
    parse_new_cauchy()
    ctx.sync()
    assert torch.equal(rows, rows_old) and torch.equal(n_rows, n_old), "parsers disagree on the Cauchy frames"
    del rows_old, n_old

    prop = torch.cuda.get_device_properties(0)
    res = {"tool": "tools/bench_relay_wire.py", "device": torch.cuda.get_device_name(0),
           "arch": getattr(prop, "gcnArchName", ""), "compute_units": prop.multi_processor_count,
           "timing": f"device events, windows of >= 0.5 s after a warm-up, {a.reps} repetitions alternated in one "
                     "process; per-kernel times from qf_ctx_profile; medians unless a list is given",
           "shape": {"k": K, "held_rows": HELD, "systematic": N_SYS, "coded": N_CODED, "m": M, "L": L, "G": G,
                     "frame_stride": fs, "payload_offset": P, "patterns": POOL},
           "outputs_checked": "in-place frames == copy-mode frames; both parsers' rows and counts equal on the "
                              "Cauchy frames; every status QF_OK"}
    series = {n: [] for n in ("parse_new_call", "parse_old_call", "parse_new_kernel", "parse_old_kernel",
                              "parse_relay_call", "parse_relay_kernel", "frame_in_place_call", "frame_copy_call",
                              "frame_in_place_kernel", "frame_copy_kernel", "recode_call", "relay_step_call")}
    relay_kernels = []
    for _ in range(a.reps):
        series["parse_new_call"].append(round(timed(parse_new_cauchy, ctx), 4))
        series["parse_old_call"].append(round(timed(parse_old_cauchy, ctx), 4))
        series["parse_new_kernel"].append(kernel_split(parse_new_cauchy, ctx)["k_parse_frames_coded"])
        series["parse_old_kernel"].append(kernel_split(parse_old_cauchy, ctx)["k_parse_frames"])
        series["parse_relay_call"].append(round(timed(parse_relay, ctx), 4))
        series["parse_relay_kernel"].append(kernel_split(parse_relay, ctx)["k_parse_frames_coded"])
        series["frame_in_place_call"].append(round(timed(frame_in_place, ctx), 4))
        series["frame_copy_call"].append(round(timed(frame_copy, ctx), 4))
        series["frame_in_place_kernel"].append(kernel_split(frame_in_place, ctx)["k_frame_rows"])
        series["frame_copy_kernel"].append(kernel_split(frame_copy, ctx)["k_frame_rows"])
        series["recode_call"].append(round(timed(recode, ctx), 4))
        series["relay_step_call"].append(round(timed(relay_step, ctx), 4))
        relay_kernels.append(kernel_split(relay_step, ctx))
    med = statistics.median

    # (1) parse against the yardstick
    n_fr = G * HELD
    y_bytes = int(y_ln.astype(np.int64).sum()) * tile + n_fr * (4 + 8) + n_fr * (L + 2 + 4) + 4 * G
    extra = n_fr * (K + 4)
    ylo, yhi = min(series["parse_old_kernel"]), max(series["parse_old_kernel"])
    bound = med(series["parse_old_kernel"]) * (1 + extra / y_bytes) + (yhi - ylo)
    res["parse"] = {
        "yardstick": "k_parse_frames (unchanged) on the same pure-Cauchy frames and buffers, alternated",
        "new_kernel_ms": series["parse_new_kernel"], "yardstick_kernel_ms": series["parse_old_kernel"],
        "new_call_ms": series["parse_new_call"], "yardstick_call_ms": series["parse_old_call"],
        "new_kernel_ms_median": med(series["parse_new_kernel"]),
        "yardstick_kernel_ms_median": med(series["parse_old_kernel"]),
        "yardstick_kernel_ms_min_max": [ylo, yhi],
        "yardstick_bytes": y_bytes, "extra_bytes": extra, "extra_bytes_fraction": round(extra / y_bytes, 5),
        "ratio_new_to_yardstick": round(med(series["parse_new_kernel"]) / med(series["parse_old_kernel"]), 4),
        "expected_at_most_ms": round(bound, 5),
        "expectation_met": bool(med(series["parse_new_kernel"]) <= bound),
        "relay_input": "arbitrary vectors, payload-aligned slots with frame_off",
        "relay_input_kernel_ms": series["parse_relay_kernel"],
        "relay_input_kernel_ms_median": med(series["parse_relay_kernel"]),
        "relay_input_call_ms": series["parse_relay_call"],
        "relay_input_GiBps_of_rows": round(n_fr * L / 2**30 / (med(series["parse_relay_kernel"]) * 1e-3), 1),
    }
    # (2) framing, in place against copy mode
    n_out = G * M
    b_in_place = n_out * (K + (3 + K) + 4 + 4)
    b_copy = b_in_place + n_out * 2 * L
    res["frame_rows"] = {
        "rows_per_generation": M,
        "in_place_kernel_ms": series["frame_in_place_kernel"], "copy_kernel_ms": series["frame_copy_kernel"],
        "in_place_call_ms": series["frame_in_place_call"], "copy_call_ms": series["frame_copy_call"],
        "in_place_kernel_ms_median": med(series["frame_in_place_kernel"]),
        "copy_kernel_ms_median": med(series["frame_copy_kernel"]),
        "in_place_bytes": b_in_place, "copy_bytes": b_copy,
        "in_place_ms_at_8TBps": round(b_in_place / (HBM_TBPS * 1e12) * 1e3, 5),
        "copy_ms_at_8TBps": round(b_copy / (HBM_TBPS * 1e12) * 1e3, 5),
        "copy_to_in_place": round(med(series["frame_copy_kernel"]) / med(series["frame_in_place_kernel"]), 3),
    }
    # (3) the relay step
    names = sorted({n for t in relay_kernels for n in t})
    kmed = {n: med(t.get(n, 0.0) for t in relay_kernels) for n in names}
    wire = kmed.get("k_parse_frames_coded", 0.0) + kmed.get("k_frame_rows", 0.0)
    total = sum(kmed.values())
    res["relay_step"] = {
        "sequence": "qf_parse_frames_coded_dev, qf_recode_batch into the frame slots, qf_frame_rows_dev in place",
        "step_call_ms": series["relay_step_call"], "step_call_ms_median": med(series["relay_step_call"]),
        "parse_call_ms_median": med(series["parse_relay_call"]),
        "recode_call_ms": series["recode_call"], "recode_call_ms_median": med(series["recode_call"]),
        "frame_in_place_call_ms_median": med(series["frame_in_place_call"]),
        "kernels_ms": relay_kernels, "kernels_ms_median": kmed,
        "kernels_ms_sum": round(total, 5), "wire_kernels_ms": round(wire, 5),
        "wire_share_of_kernel_time": round(wire / total, 4),
        "input_rows_GiBps": round(n_fr * L / 2**30 / (med(series["relay_step_call"]) * 1e-3), 1),
    }
    Path(a.out).parent.mkdir(exist_ok=True, parents=True)
    Path(a.out).write_text(json.dumps(res, indent=1))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
