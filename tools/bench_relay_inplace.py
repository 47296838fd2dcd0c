#!/usr/bin/env python3
"""Timing of the in-place relay step against the three-call step
of DESIGN 3.11, frames in and frames out on the device.

    python tools/bench_relay_inplace.py --out profiles/relay_inplace_bench.json

  new        qf_parse_frame_headers_dev -> qf_recode_frames_dev (rows read in
             their frame slots) -> qf_frame_rows_dev in place
  yardstick  qf_parse_frames_coded_dev -> qf_recode_batch -> qf_frame_rows_dev
             in place (unchanged code)
Shapes: k = 64, 64 held rows (51 systematic + 13 coded), m = 16, L = 1,200,
G = 65,536, frame_stride 1,280 (the shape of relay_wire_bench.json), and
(196, 196, 59) at L = 9,000, G = 566, where the yardstick's payload runs the
bit-sliced kernels.  The input is a relay's: arbitrary vectors in
payload-aligned slots with frame_off.

Both steps run alternated in one process; times are device events over windows
of at least 0.5 s after a warm-up, medians with min-max over the repetitions;
per-kernel times from qf_ctx_profile.  The tool asserts that both steps leave
identical output frames, frame_len, out_coeffs and statuses.  It records
  (a) new step : yardstick step;
  (b) k_combine_rows_at : the yardstick's payload kernel on the same
      generations, with the expectation ratio <= 1 + added descriptor bytes /
      yardstick bytes + the yardstick's own relative min-max spread, and
      whether it is met.
Prints one JSON line."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

# k, systematic, coded, m, L, G, distinct generation patterns (tiled over the batch)
SHAPES = {
    "k64_m16_L1200": (64, 51, 13, 16, 1200, 65536, 64),
    "k196_m59_L9000": (196, 150, 46, 59, 9000, 566, 2),
}
FIXED = ("k_parse_frame_headers", "k_parse_frames_coded", "k_recode_prepare", "k_frame_rows")


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


def frame_pool(qf, rng, K, n_sys, n_coded, L, pool, fs):
    """`pool` generations of held frames, systematic and coded (arbitrary
    vectors) in a shuffled order, in the payload-aligned layout."""
    P = qf.frame_payload_offset(K)
    held = n_sys + n_coded
    fr = np.zeros((pool, held, fs), np.uint8)
    ln = np.zeros((pool, held), np.uint32)
    off = np.zeros((pool, held), np.uint32)
    ids = np.zeros((pool, held), np.uint64)
    for g in range(pool):
        sys_idx = rng.permutation(K)[:n_sys]
        for what, s in enumerate(rng.permutation(held)):
            pay = rng.integers(0, 256, L, dtype=np.uint8)
            if what < n_sys:
                head = np.array([1], np.uint8)
                ids[g, s] = 7 * K + int(sys_idx[what])
            else:
                vec = rng.integers(0, 256, K, dtype=np.uint8)
                head = np.concatenate([np.array([0, K >> 8, K & 0xFF], np.uint8), vec])
                ids[g, s] = 100000 + what
            o = P - len(head)
            fr[g, s, o: o + len(head)] = head
            fr[g, s, P: P + L] = pay
            ln[g, s], off[g, s] = len(head) + L, o
    return fr, ln, off, ids


def spread(v):
    return [min(v), max(v)]


def run_shape(qf, ctx, name, reps, G_override=None):
    import torch

    K, n_sys, n_coded, M, L, G, pool = SHAPES[name]
    if G_override:
        G = max(pool, G_override // pool * pool)
    held = n_sys + n_coded
    dev = f"cuda:{ctx.device}"
    rng = np.random.default_rng(2028)
    P = qf.frame_payload_offset(K)
    fs = (P + L + 15) // 16 * 16
    rs = (L + 15) // 16 * 16
    tile = G // pool
    assert tile * pool == G

    def up(x):
        return torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).to(dev).repeat(tile)

    fr, ln, off, ids = frame_pool(qf, rng, K, n_sys, n_coded, L, pool, fs)
    t_fr, t_ln, t_off, t_ids = up(fr), up(ln), up(off), up(ids)
    z = lambda n: torch.zeros(n, dtype=torch.uint8, device=dev)   # noqa: E731
    seed = 12345
    # yardstick buffers
    rows, y_idx, y_n, y_fst = z(G * held * rs), z(2 * G * held), z(4 * G), z(4 * G * held)
    y_co, y_rl = z(G * held * K), z(4 * G * held)
    y_out, y_oc, y_st = z(G * M * fs), z(G * M * K), z(4 * G)
    y_flen, y_foff = z(4 * G * M), z(4 * G * M)
    # new step's buffers
    n_idx, n_n, n_fst = z(2 * G * held), z(4 * G), z(4 * G * held)
    n_co, n_rl, n_ro = z(G * held * K), z(4 * G * held), z(4 * G * held)
    n_out, n_oc, n_st, n_ol = z(G * M * fs), z(G * M * K), z(4 * G), z(4 * G * M)
    n_flen, n_foff = z(4 * G * M), z(4 * G * M)

    def y_parse():
        qf.parse_frames_coded(t_fr, t_ln, t_ids, rows, y_idx, y_n, y_fst, y_co, K, L, max_rows=held, frame_stride=fs,
                              row_stride=rs, rows_gen_stride=held * rs, G=G, frame_off=t_off, row_len=y_rl, ctx=ctx)

    def y_recode():
        qf.recode_batch(rows, y_idx, y_out[P:], y_oc, y_st, K, M, L, max_rows=held, row_stride=rs,
                        rows_gen_stride=held * rs, out_row_stride=fs, out_gen_stride=M * fs, G=G, n_rows=y_n,
                        row_coeffs=y_co, seed=seed, ctx=ctx)

    def y_frame():
        qf.frame_rows(None, y_out, y_flen, K, L, max_rows=M, frame_stride=fs, G=G, row_coeffs=y_oc,
                      frame_off=y_foff, in_place=True, ctx=ctx)

    def n_parse():
        qf.parse_frame_headers(t_fr, t_ln, t_ids, n_idx, n_n, n_fst, n_co, n_rl, n_ro, K, L, max_rows=held,
                               frame_stride=fs, G=G, frame_off=t_off, ctx=ctx)

    def n_recode():
        qf.recode_frames(t_fr, n_ro, n_rl, n_idx, n_co, n_out[P:], n_oc, n_st, K, M, L, max_rows=held,
                         src_gen_stride=held * fs, out_row_stride=fs, out_gen_stride=M * fs, G=G, n_rows=n_n,
                         seed=seed, out_len=n_ol, ctx=ctx)

    def n_frame():
        qf.frame_rows(None, n_out, n_flen, K, L, max_rows=M, frame_stride=fs, G=G, row_coeffs=n_oc, row_len=n_ol,
                      frame_off=n_foff, in_place=True, ctx=ctx)

    def y_step():
        y_parse()
        y_recode()
        y_frame()

    def n_step():
        n_parse()
        n_recode()
        n_frame()

    y_step()
    n_step()
    ctx.sync()
    assert (y_fst.view(torch.int32) == 0).all() and (y_n.view(torch.int32) == held).all()
    assert torch.equal(n_fst, y_fst) and torch.equal(n_n, y_n) and torch.equal(n_idx, y_idx)
    assert torch.equal(n_co, y_co) and torch.equal(n_rl, y_rl)
    assert (y_st.view(torch.int32) == 0).all() and torch.equal(n_st, y_st), "statuses differ"
    assert torch.equal(n_out, y_out), "output frames differ"
    assert torch.equal(n_flen, y_flen) and torch.equal(n_foff, y_foff), "frame_len / frame_off differ"
    assert torch.equal(n_oc, y_oc), "out_coeffs differ"
    assert (n_ol.view(torch.int32) == L).all()

    s = {n: [] for n in ("new_step", "yard_step", "new_parse", "yard_parse", "new_recode", "yard_recode")}
    nk, yk = [], []
    for _ in range(reps):
        s["new_step"].append(round(timed(n_step, ctx), 4))
        s["yard_step"].append(round(timed(y_step, ctx), 4))
        s["new_parse"].append(round(timed(n_parse, ctx), 4))
        s["yard_parse"].append(round(timed(y_parse, ctx), 4))
        s["new_recode"].append(round(timed(n_recode, ctx), 4))
        s["yard_recode"].append(round(timed(y_recode, ctx), 4))
        nk.append(kernel_split(n_step, ctx))
        yk.append(kernel_split(y_step, ctx))
    med = statistics.median

    def payload(t):
        return round(sum(ms for n, ms in t.items() if n not in FIXED), 5)

    n_pay, y_pay = [payload(t) for t in nk], [payload(t) for t in yk]
    y_pay_names = sorted({n for t in yk for n in t if n not in FIXED})
    passes = (M + 15) // 16
    y_bytes = G * held * L + G * M * L + G * passes * (held + 1) * 16
    added = G * passes * (((held + 1) // 2 + 1) * 48 - (held + 1) * 16) + 4 * G
    y_spread = (max(y_pay) - min(y_pay)) / med(y_pay)
    bound = 1 + added / y_bytes + y_spread
    ratio_b = med(n_pay) / med(y_pay)
    kmed = lambda ks: {n: med(t.get(n, 0.0) for t in ks) for n in sorted({n for t in ks for n in t})}   # noqa: E731
    return {
        "shape": {"k": K, "held_rows": held, "systematic": n_sys, "coded": n_coded, "m": M, "L": L, "G": G,
                  "frame_stride": fs, "payload_offset": P, "patterns": pool},
        "outputs_checked": "both steps: identical output frames, frame_len, frame_off, out_coeffs and statuses; the "
                           "two parsers' row_index, n_rows, row_coeffs, row_len and frame_status equal",
        "step": {
            "new_call_ms": s["new_step"], "yardstick_call_ms": s["yard_step"],
            "new_call_ms_median": med(s["new_step"]), "new_call_ms_min_max": spread(s["new_step"]),
            "yardstick_call_ms_median": med(s["yard_step"]), "yardstick_call_ms_min_max": spread(s["yard_step"]),
            "ratio_new_to_yardstick": round(med(s["new_step"]) / med(s["yard_step"]), 4),
            "input_rows_GiBps_new": round(G * held * L / 2**30 / (med(s["new_step"]) * 1e-3), 1),
            "input_rows_GiBps_yardstick": round(G * held * L / 2**30 / (med(s["yard_step"]) * 1e-3), 1),
        },
        "calls": {
            "new_parse_ms_median": med(s["new_parse"]), "yardstick_parse_ms_median": med(s["yard_parse"]),
            "new_parse_ms_min_max": spread(s["new_parse"]), "yardstick_parse_ms_min_max": spread(s["yard_parse"]),
            "new_recode_ms_median": med(s["new_recode"]), "yardstick_recode_ms_median": med(s["yard_recode"]),
            "new_recode_ms_min_max": spread(s["new_recode"]), "yardstick_recode_ms_min_max": spread(s["yard_recode"]),
        },
        "kernels_ms_median": {"new": kmed(nk), "yardstick": kmed(yk)},
        "kernels_ms": {"new": nk, "yardstick": yk},
        "payload_kernel": {
            "new": "k_combine_rows_at", "yardstick": y_pay_names, "passes": passes,
            "new_ms": n_pay, "yardstick_ms": y_pay,
            "new_ms_median": med(n_pay), "yardstick_ms_median": med(y_pay),
            "new_ms_min_max": spread(n_pay), "yardstick_ms_min_max": spread(y_pay),
            "ratio_new_to_yardstick": round(ratio_b, 4),
            "yardstick_bytes": y_bytes, "added_descriptor_bytes": added,
            "added_bytes_fraction": round(added / y_bytes, 5),
            "yardstick_relative_spread": round(y_spread, 5),
            "expectation": "ratio <= 1 + added descriptor bytes / yardstick bytes + the yardstick's relative "
                           "min-max spread",
            "expected_ratio_at_most": round(bound, 4),
            "expectation_met": bool(ratio_b <= bound),
        },
    }


def main():
    import torch

    from quicfuscate_amd import fec as qf

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--generations", type=int, default=0, help="override G (a smoke run)")
    ap.add_argument("--out", default="profiles/relay_inplace_bench.json")
    a = ap.parse_args()
    assert torch.cuda.is_available()
    ctx = qf.default_context()
    prop = torch.cuda.get_device_properties(0)
    res = {"tool": "tools/bench_relay_inplace.py", "device": torch.cuda.get_device_name(0),
           "arch": getattr(prop, "gcnArchName", ""), "compute_units": prop.multi_processor_count,
           "timing": f"device events, windows of >= 0.5 s after a warm-up, {a.reps} repetitions, the two steps "
                     "alternated in one process; per-kernel times from qf_ctx_profile; medians with min-max",
           "new_step": "qf_parse_frame_headers_dev, qf_recode_frames_dev from the frame slots into the output "
                       "frame slots, qf_frame_rows_dev in place with out_len",
           "yardstick_step": "qf_parse_frames_coded_dev, qf_recode_batch into the output frame slots, "
                             "qf_frame_rows_dev in place",
           "shapes": {}}
    for name in a.shapes.split(","):
        res["shapes"][name] = run_shape(qf, ctx, name, a.reps, a.generations)
        torch.cuda.empty_cache()
    Path(a.out).parent.mkdir(exist_ok=True, parents=True)
    Path(a.out).write_text(json.dumps(res, indent=1))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
