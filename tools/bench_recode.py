#!/usr/bin/env python3
"""Timing of qf_recode_batch against its yardsticks.

    python tools/bench_recode.py --out bench_outputs/recode_bench.json

Per shape (k, n, m, L, G; the n rows held are systematic rows plus Cauchy
repairs): the call time by device events over a window of at least 0.5 s
after a warm-up, the per-kernel times (qf_ctx_profile), GiB/s of input rows,
the fraction of the 8 TB/s HBM roof the algorithmic payload bytes reach, and
the prepare : payload ratio.  The yardstick runs in the same process,
alternated with the recode windows: the general decode (qf_decode_batch with
explicit coefficient vectors) at the same k, n, L and G with m outputs, whose
payload pass is the same kernel over the same bytes and whose control kernel
(k_decode_prepare) eliminates where k_recode_prepare only multiplies.
Prints one JSON line."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

HBM_ROOF = 8e12
# k, n held rows, coded rows among them (Cauchy repairs), r, m, L, G
SHAPES = {
    "k64_m16_L1200": (64, 64, 13, 16, 16, 1200, 65536),              # C3: 51 systematic + 13 repairs
    "k196_m59_L9000": (196, 196, 39, 59, 59, 9000, int(1e9 // (196 * 9000))),   # C5, G of bench.py's shape leg
}


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


def bench_shape(qf, ctx, k, n, ncoded, r, m, L, G, reps):
    import torch

    from quicfuscate_amd import _lib as Lb

    dev = f"cuda:{ctx.device}"
    rs = _r16(L)
    rows = torch.empty(G * n * rs, dtype=torch.uint8, device=dev)
    Lb.check(Lb._lib().qf_fill_splitmix_dev(ctx.handle, rows.data_ptr(), rows.numel(), 1, 0), "fill")
    # recode inputs: n - ncoded systematic rows then ncoded Cauchy repairs (implicit vectors)
    idx = np.concatenate([np.arange(n - ncoded), k + np.arange(ncoded)]).astype(np.uint16)
    t_idx = torch.from_numpy(np.tile(idx, G).view(np.int16)).to(dev)
    out = torch.empty(G * m * rs, dtype=torch.uint8, device=dev)
    oc = torch.empty(G * m * k, dtype=torch.uint8, device=dev)
    st = torch.empty(G, dtype=torch.int32, device=dev)
    seed = [0]

    def recode():
        seed[0] += 1
        qf.recode_batch(rows, t_idx, out, oc, st, k, m, L, r=r, max_rows=n, row_stride=rs, rows_gen_stride=n * rs,
                        out_row_stride=rs, out_gen_stride=m * rs, G=G, seed=seed[0], ctx=ctx)

    # yardstick: m erased sources, n - m systematic rows then m repairs with explicit (Cauchy) vectors
    e = min(m, k)
    didx = np.concatenate([np.arange(e, k), k + np.arange(e)])[:n].astype(np.uint16)
    C = np.frombuffer(qf.cauchy_coefficients(k, e), np.uint8).reshape(e, k)
    rc = np.zeros((n, k), np.uint8)
    rc[k - e: k] = C
    t_didx = torch.from_numpy(np.tile(didx, G).view(np.int16)).to(dev)
    t_rc = torch.from_numpy(rc.reshape(-1)).to(dev).repeat(G)
    rec = torch.empty(G * e * rs, dtype=torch.uint8, device=dev)
    ri = torch.empty(G * e, dtype=torch.int16, device=dev)
    nrec = torch.empty(G, dtype=torch.int32, device=dev)
    dst = torch.empty(G, dtype=torch.int32, device=dev)

    def decode():
        qf.decode_batch(rows, t_didx, rec, ri, nrec, dst, k, e, L, max_rows=n, row_stride=rs, rows_gen_stride=n * rs,
                        rec_row_stride=rs, rec_gen_stride=e * rs, G=G, row_coeffs=t_rc, ctx=ctx)

    torch.cuda.synchronize()
    res = {"k": k, "n": n, "coded_rows": ncoded, "m": m, "L": L, "G": G, "recode_call_ms": [],
           "decode_call_ms": [], "recode_kernels_ms": [], "decode_kernels_ms": []}
    for _ in range(reps):   # alternated: the spread is the run-to-run spread of both
        res["recode_call_ms"].append(round(timed(recode, ctx), 4))
        res["decode_call_ms"].append(round(timed(decode, ctx), 4))
        res["recode_kernels_ms"].append(kernel_split(recode, ctx))
        res["decode_kernels_ms"].append(kernel_split(decode, ctx))
    ctx.sync()
    assert (st.cpu().numpy() == 0).all() and (dst.cpu().numpy() == 0).all() and (nrec.cpu().numpy() == e).all()
    passes = (m + 15) // 16
    payload_bytes = (n + m) * L * G                     # every input row once, every output row once
    prepare_bytes = G * (2 * n + passes * (n + 1) * 16 + m * k + 12)   # indices, records, vectors, status words
    call = min(res["recode_call_ms"]) * 1e-3
    prep = min(t["k_recode_prepare"] for t in res["recode_kernels_ms"])
    pay = min(sum(v for n_, v in t.items() if n_ != "k_recode_prepare") for t in res["recode_kernels_ms"])
    dprep = min(t.get("k_decode_prepare", 0.0) for t in res["decode_kernels_ms"])
    dpay = min(sum(v for n_, v in t.items() if n_ != "k_decode_prepare") for t in res["decode_kernels_ms"])
    res.update({
        "payload_bytes": payload_bytes, "prepare_bytes": prepare_bytes, "payload_passes": passes,
        "input_GiBps": round(n * L * G / call / 2**30, 1),
        "hbm_roof_fraction": round(payload_bytes / call / HBM_ROOF, 4),
        "hbm_roof_fraction_payload_kernel": round((passes * n + m) * L * G / (pay * 1e-3) / HBM_ROOF, 4),
        "prepare_ms": prep, "payload_ms": round(pay, 5), "prepare_to_payload": round(prep / pay, 4),
        "yardstick_decode_prepare_ms": dprep, "yardstick_decode_payload_ms": round(dpay, 5),
        "payload_vs_yardstick": round(pay / dpay, 4), "prepare_vs_yardstick": round(prep / dprep, 4) if dprep else None,
    })
    return res


def main():
    import torch

    from quicfuscate_amd import fec as qf

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default="bench_outputs/recode_bench.json")
    a = ap.parse_args()
    assert torch.cuda.is_available()
    ctx = qf.default_context()
    hashes = {}
    hp = REPO / "quicfuscate_amd" / "lib" / "kernel_hashes.json"
    if hp.exists():
        hashes = {n: h for n, h in json.loads(hp.read_text()).items() if n.startswith("qf_combine_bs")}
    res = {"tool": "tools/bench_recode.py", "device": torch.cuda.get_device_name(0), "hbm_roof_Bps": HBM_ROOF,
           "payload_kernel_hashes": hashes, "shapes": {}}
    for name in a.shapes.split(","):
        res["shapes"][name] = bench_shape(qf, ctx, *SHAPES[name], a.reps)
    Path(a.out).parent.mkdir(exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
