#!/usr/bin/env python3
"""Timing of qf_decode_innovative_batch / k_rank_filter.

    python tools/bench_rank.py --out bench_outputs/rank_bench.json

Two shapes at k = 64, L = 1,200, G = 65,536:
  (a) mostly_systematic  77 rows: 51 distinct systematic rows and 26 coded rows
      with explicit random vectors in a shuffled arrival order, 13 of the coded
      rows needed; the first 64 candidates are independent (checked on the
      host with qf_gf256_rank).  Yardstick: qf_decode_batch with the same
      vectors on the same buffers, alternated with the new call in this
      process; its outputs must be identical.
  (b) all_coded_dependent  80 coded rows, 8 of the first 64 planted as
      combinations of earlier rows: qf_decode_batch cannot decode it
      (QF_ERANK, asserted), so the times are absolute, plus the ratio of its
      filter time to (a)'s.
Per shape: the call time by device events over a window of at least 0.5 s
after a warm-up, and the per-kernel times (qf_ctx_profile): k_rank_filter,
k_decode_prepare and the payload kernel by name.  The payload kernel of (a)
must carry the yardstick's name, and its time is compared with the
yardstick's own run-to-run spread.  Prints one JSON line."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

K, L, G = 64, 1200, 65536
POOL = 64          # distinct generation patterns, tiled over the batch
CONTROL = ("k_rank_filter", "k_decode_prepare")


def _r16(x):
    return (x + 15) // 16 * 16


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


def patterns_a(qf, rng):
    """POOL patterns of (idx (77,), vectors (77, K)): the 51 systematic rows and
    13 coded rows shuffled over the first 64 slots, 13 more coded rows behind them."""
    out = []
    while len(out) < POOL:
        sys_idx = rng.permutation(K)[:51]
        order = np.concatenate([rng.permutation(64), 64 + np.arange(13)])
        idx = np.zeros(77, np.uint16)
        vec = np.zeros((77, K), np.uint8)
        full = np.zeros((77, K), np.uint8)
        for pos, what in zip(order, range(77)):
            if what < 51:
                idx[pos] = sys_idx[what]
                full[pos, sys_idx[what]] = 1
            else:
                idx[pos] = K + what
                vec[pos] = full[pos] = rng.integers(0, 256, K)
        rank, flags = qf.gf_rank(full, K)
        # the first 64 candidates (all rows are distinct candidates here) are independent
        if rank == K and sum(flags[:K]) == K:
            out.append((idx, vec))
    return out


def patterns_b(qf, rng):
    """POOL patterns of 80 coded rows, 8 of the first 64 combinations of two earlier rows."""
    mul_row = {}

    def mul(c, v):
        if c not in mul_row:
            mul_row[c] = np.array([qf.gf_mul(c, x) for x in range(256)], np.uint8)
        return mul_row[c][v]

    out = []
    while len(out) < POOL:
        vec = rng.integers(0, 256, (80, K), dtype=np.uint8)
        planted = sorted(rng.choice(np.arange(2, K), 8, replace=False).tolist())
        for s in planted:
            a, b = rng.choice(s, 2, replace=False)
            vec[s] = mul(int(rng.integers(1, 256)), vec[a]) ^ mul(int(rng.integers(1, 256)), vec[b])
        rank, flags = qf.gf_rank(vec, K)
        if rank == K and sum(flags[:K]) == K - 8 and not any(flags[s] for s in planted):
            out.append(((K + np.arange(80)).astype(np.uint16), vec))
    return out


def bench_shape(qf, ctx, pats, r, reps, yardstick):
    import torch

    from quicfuscate_amd import _lib as Lb

    dev = f"cuda:{ctx.device}"
    mr = len(pats[0][0])
    rs = _r16(L)
    em = min(K, r)
    rows = torch.empty(G * mr * rs, dtype=torch.uint8, device=dev)
    Lb.check(Lb._lib().qf_fill_splitmix_dev(ctx.handle, rows.data_ptr(), rows.numel(), 1, 0), "fill")
    idx = np.stack([p[0] for p in pats])
    vec = np.stack([p[1] for p in pats])
    t_idx = torch.from_numpy(idx.view(np.int16).reshape(-1)).to(dev).repeat(G // POOL)
    t_vec = torch.from_numpy(vec.reshape(-1)).to(dev).repeat(G // POOL)

    def outputs():
        return (torch.zeros(G * em * rs, dtype=torch.uint8, device=dev), torch.zeros(G * em, dtype=torch.int16, device=dev),
                torch.zeros(G, dtype=torch.int32, device=dev), torch.full((G,), 77, dtype=torch.int32, device=dev))

    kw = dict(max_rows=mr, row_stride=rs, rows_gen_stride=mr * rs, rec_row_stride=rs, rec_gen_stride=em * rs, G=G,
              row_coeffs=t_vec, ctx=ctx)
    n_out = outputs()
    rank = torch.zeros(G, dtype=torch.int32, device=dev)

    def new():
        qf.decode_innovative_batch(rows, t_idx, *n_out, K, r, L, rank=rank, **kw)

    y_out = outputs()

    def old():
        qf.decode_batch(rows, t_idx, *y_out, K, r, L, **kw)

    torch.cuda.synchronize()
    res = {"k": K, "r": r, "max_rows": mr, "L": L, "G": G, "patterns": POOL, "new_call_ms": [], "new_kernels_ms": []}
    if yardstick:
        res.update({"yardstick": "qf_decode_batch, same explicit vectors, same buffers, alternated in this process",
                    "yardstick_call_ms": [], "yardstick_kernels_ms": []})
    for _ in range(reps):   # alternated: the spread is the run-to-run spread of both
        res["new_call_ms"].append(round(timed(new, ctx), 4))
        if yardstick:
            res["yardstick_call_ms"].append(round(timed(old, ctx), 4))
        res["new_kernels_ms"].append(kernel_split(new, ctx))
        if yardstick:
            res["yardstick_kernels_ms"].append(kernel_split(old, ctx))
    if not yardstick:
        old()
    ctx.sync()
    assert (n_out[3].cpu().numpy() == 0).all() and (rank.cpu().numpy() == K).all()
    if yardstick:
        for a, b, what in zip(n_out, y_out, ("rec", "rec_index", "n_rec", "status")):
            assert torch.equal(a, b), f"{what} differs from qf_decode_batch's"
        res["outputs_identical_to_yardstick"] = True
    else:
        assert (y_out[3].cpu().numpy() == Lb.QF_ERANK).all()
        res["qf_decode_batch_status"] = "QF_ERANK for every generation"
    res["recovered_rows_per_generation"] = int(n_out[2].cpu().numpy()[0])

    def payload(t):
        names = [n for n in t if n not in CONTROL]
        assert len(names) == 1, t
        return names[0], t[names[0]]

    med = statistics.median
    pn = [payload(t) for t in res["new_kernels_ms"]]
    res.update({
        "filter_ms": med(t["k_rank_filter"] for t in res["new_kernels_ms"]),
        "prepare_ms": med(t["k_decode_prepare"] for t in res["new_kernels_ms"]),
        "payload_kernel": pn[0][0], "payload_ms": med(v for _, v in pn),
        "call_ms": med(res["new_call_ms"]),
    })
    res["filter_to_prepare"] = round(res["filter_ms"] / res["prepare_ms"], 4)
    if yardstick:
        py = [payload(t) for t in res["yardstick_kernels_ms"]]
        ylo, yhi = min(v for _, v in py), max(v for _, v in py)
        res.update({
            "yardstick_prepare_ms": med(t["k_decode_prepare"] for t in res["yardstick_kernels_ms"]),
            "yardstick_payload_kernel": py[0][0], "yardstick_payload_ms_min_max": [ylo, yhi],
            "yardstick_call_ms_median": med(res["yardstick_call_ms"]),
            "call_vs_yardstick": round(res["call_ms"] / med(res["yardstick_call_ms"]), 4),
            "payload_kernel_same_name": all(n == py[0][0] for n, _ in pn + py),
            "payload_ms_within_yardstick_spread": bool(ylo <= res["payload_ms"] <= yhi),
        })
    return res


def main():
    import torch

    from quicfuscate_amd import fec as qf

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="bench_outputs/rank_bench.json")
    a = ap.parse_args()
    assert torch.cuda.is_available()
    ctx = qf.default_context()
    rng = np.random.default_rng(2026)
    prop = torch.cuda.get_device_properties(0)
    res = {"tool": "tools/bench_rank.py", "device": torch.cuda.get_device_name(0),
           "arch": getattr(prop, "gcnArchName", ""), "compute_units": prop.multi_processor_count,
           "timing": f"device events, windows of >= 0.5 s after a warm-up, {a.reps} repetitions alternated with "
                     "the yardstick in one process; medians unless a list is given",
           "shapes": {}}
    res["shapes"]["a_mostly_systematic"] = bench_shape(qf, ctx, patterns_a(qf, rng), 26, a.reps, True)
    res["shapes"]["b_all_coded_dependent"] = bench_shape(qf, ctx, patterns_b(qf, rng), 64, a.reps, False)
    sa, sb = res["shapes"]["a_mostly_systematic"], res["shapes"]["b_all_coded_dependent"]
    res["filter_b_to_filter_a"] = round(sb["filter_ms"] / sa["filter_ms"], 3)
    Path(a.out).parent.mkdir(exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
