#!/usr/bin/env python3
"""Timing of the in-place receive step against the copy path of
DESIGN 3.11, frames in and recovered rows out on the device.

    python tools/bench_recv_inplace.py --out profiles/recv_inplace_bench.json

  new        qf_parse_frame_headers_dev -> qf_decode_frames_dev (rows read in
             their frame slots)
  yardstick  qf_parse_frames_coded_dev -> qf_decode_innovative_batch (unchanged
             code)
Shapes (k = 64, L = 1,200, G = 65,536, frame_stride 1,280, 64 distinct patterns
tiled; the patterns of tools/bench_rank.py, framed in the payload-aligned
layout):
  a          51 systematic + 26 coded rows, 13 recovered, r = 16
  b          80 coded rows, 8 of the first 64 dependent, 64 recovered, r = 64
  long       (196, 59) at L = 9,000, G = 566: 137 systematic + 59 coded rows, 59
             recovered; the yardstick's payload runs the bit-sliced kernel there
and shape a once more with r = 64 (four passes launched, three with nothing to
write) against r = 16, the new call alone.

Both steps run alternated in one process; times are device events over windows
of at least 0.5 s after a warm-up, medians with min-max over the repetitions;
per-kernel times from qf_ctx_profile.  The tool asserts that both steps leave
identical rec, rec_index, n_rec and status.  It records
  (a) new step : yardstick step (the headline);
  (b) k_combine_rows_at : the yardstick's payload kernel on the same
      generations, the bytes each side's payload pass moves, and the
      expectation ratio <= 1 + added descriptor bytes / yardstick bytes + the
      yardstick's own relative min-max spread, and whether it is met.
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

FIXED = ("k_parse_frame_headers", "k_parse_frames_coded", "k_rank_filter", "k_decode_prepare")


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


def patterns(qf, rng, K, n_sys, n_coded_front, n_behind, planted, pool):
    """`pool` patterns of (idx, vectors, flags): n_sys distinct systematic rows
    and n_coded_front coded rows shuffled over the first slots, `planted` of
    the coded ones combinations of two earlier rows, n_behind more coded rows
    behind them; explicit random vectors.  The rank is K and, without planted
    rows, the first K rows are independent."""
    mul_row = {}

    def mul(c, v):
        if c not in mul_row:
            mul_row[c] = np.array([qf.gf_mul(c, x) for x in range(256)], np.uint8)
        return mul_row[c][v]

    front = n_sys + n_coded_front
    mr = front + n_behind
    out = []
    while len(out) < pool:
        sys_idx = rng.permutation(K)[:n_sys]
        order = np.concatenate([rng.permutation(front), front + np.arange(n_behind)])
        idx = np.zeros(mr, np.uint16)
        vec = np.zeros((mr, K), np.uint8)
        for pos, what in zip(order, range(mr)):
            if what < n_sys:
                idx[pos] = sys_idx[what]
                vec[pos, sys_idx[what]] = 1
            else:
                idx[pos] = K
                vec[pos] = rng.integers(0, 256, K)
        spots = sorted(rng.choice(np.arange(2, front), planted, replace=False).tolist()) if planted else []
        for s in spots:
            a, b = rng.choice(s, 2, replace=False)
            idx[s] = K
            vec[s] = mul(int(rng.integers(1, 256)), vec[a]) ^ mul(int(rng.integers(1, 256)), vec[b])
        rank, flags = qf.gf_rank(vec, K)
        if rank == K and not any(flags[s] for s in spots) and (planted or sum(flags[:K]) == K):
            out.append((idx, vec, np.array(flags, np.uint8)))
    return out


def frame_pool(qf, rng, K, L, fs, pats):
    """The patterns' rows as frames in the payload-aligned layout, random payloads."""
    P = qf.frame_payload_offset(K)
    pool, mr = len(pats), len(pats[0][0])
    fr = np.zeros((pool, mr, fs), np.uint8)
    ln = np.zeros((pool, mr), np.uint32)
    off = np.zeros((pool, mr), np.uint32)
    ids = np.zeros((pool, mr), np.uint64)
    for g, (idx, vec, _) in enumerate(pats):
        for s in range(mr):
            if idx[s] < K:
                head = np.array([1], np.uint8)
                ids[g, s] = 7 * K + int(idx[s])
            else:
                head = np.concatenate([np.array([0, K >> 8, K & 0xFF], np.uint8), vec[s]])
                ids[g, s] = 100000 + s
            o = P - len(head)
            fr[g, s, o: o + len(head)] = head
            fr[g, s, P: P + L] = rng.integers(0, 256, L, dtype=np.uint8)
            ln[g, s], off[g, s] = len(head) + L, o
    return fr, ln, off, ids


def spread(v):
    return [min(v), max(v)]


# name: k, systematic, coded among the first rows, coded behind them, planted dependents, r, L, G, patterns
SHAPES = {
    "a_51sys_26coded_r16": (64, 51, 13, 13, 0, 16, 1200, 65536, 64),
    "b_80coded_r64": (64, 0, 64, 16, 8, 64, 1200, 65536, 64),
    "long_k196_r59_L9000": (196, 137, 59, 0, 0, 59, 9000, 566, 2),
}


class Step:
    """Buffers and the two receive sequences of one shape."""

    def __init__(self, qf, ctx, name, G_override=0, r_override=0):
        import torch

        K, n_sys, n_front, n_behind, planted, r, L, G, pool = SHAPES[name]
        if G_override:
            G = max(pool, G_override // pool * pool)
        self.r = r = r_override or r
        self.K, self.L, self.G, self.pool = K, L, G, pool
        self.qf, self.ctx = qf, ctx
        rng = np.random.default_rng(2029)
        self.pats = patterns(qf, rng, K, n_sys, n_front, n_behind, planted, pool)
        self.mr = mr = len(self.pats[0][0])
        self.P = P = qf.frame_payload_offset(K)
        self.fs = fs = (P + L + 15) // 16 * 16
        self.rs = rs = (L + 15) // 16 * 16
        dev = f"cuda:{ctx.device}"
        tile = G // pool
        assert tile * pool == G

        def up(x):
            return torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).to(dev).repeat(tile)

        fr, ln, off, ids = frame_pool(qf, rng, K, L, fs, self.pats)
        self.t_fr, self.t_ln, self.t_off, self.t_ids = up(fr), up(ln), up(off), up(ids)
        z = lambda n: torch.zeros(n, dtype=torch.uint8, device=dev)   # noqa: E731
        em = min(K, r)
        self.em = em
        # yardstick buffers
        self.rows, self.y_idx, self.y_n, self.y_fst = z(G * mr * rs), z(2 * G * mr), z(4 * G), z(4 * G * mr)
        self.y_co, self.y_rl = z(G * mr * K), z(4 * G * mr)
        self.y_rec, self.y_ri, self.y_nrec, self.y_st = z(G * em * rs), z(2 * G * em), z(4 * G), z(4 * G)
        # the new step's
        self.n_idx, self.n_n, self.n_fst = z(2 * G * mr), z(4 * G), z(4 * G * mr)
        self.n_co, self.n_rl, self.n_ro = z(G * mr * K), z(4 * G * mr), z(4 * G * mr)
        self.n_rec, self.n_ri, self.n_nrec, self.n_st = z(G * em * rs), z(2 * G * em), z(4 * G), z(4 * G)
        self.n_slot = z(2 * G * K)

    def y_parse(self):
        self.qf.parse_frames_coded(self.t_fr, self.t_ln, self.t_ids, self.rows, self.y_idx, self.y_n, self.y_fst,
                                   self.y_co, self.K, self.L, max_rows=self.mr, frame_stride=self.fs,
                                   row_stride=self.rs, rows_gen_stride=self.mr * self.rs, G=self.G,
                                   frame_off=self.t_off, row_len=self.y_rl, ctx=self.ctx)

    def y_decode(self):
        self.qf.decode_innovative_batch(self.rows, self.y_idx, self.y_rec, self.y_ri, self.y_nrec, self.y_st, self.K,
                                        self.r, self.L, max_rows=self.mr, row_stride=self.rs,
                                        rows_gen_stride=self.mr * self.rs, rec_row_stride=self.rs,
                                        rec_gen_stride=self.em * self.rs, G=self.G, n_rows=self.y_n,
                                        row_coeffs=self.y_co, ctx=self.ctx)

    def n_parse(self):
        self.qf.parse_frame_headers(self.t_fr, self.t_ln, self.t_ids, self.n_idx, self.n_n, self.n_fst, self.n_co,
                                    self.n_rl, self.n_ro, self.K, self.L, max_rows=self.mr, frame_stride=self.fs,
                                    G=self.G, frame_off=self.t_off, ctx=self.ctx)

    def n_decode(self):
        self.qf.decode_frames(self.t_fr, self.n_ro, self.n_rl, self.n_idx, self.n_co, self.n_rec, self.n_ri,
                              self.n_nrec, self.n_st, self.K, self.r, self.L, max_rows=self.mr,
                              src_gen_stride=self.mr * self.fs, rec_row_stride=self.rs,
                              rec_gen_stride=self.em * self.rs, G=self.G, n_rows=self.n_n, src_slot=self.n_slot,
                              ctx=self.ctx)

    def y_step(self):
        self.y_parse()
        self.y_decode()

    def n_step(self):
        self.n_parse()
        self.n_decode()

    def check(self, recovered):
        import torch

        self.y_step()
        self.n_step()
        self.ctx.sync()
        assert (self.y_fst.view(torch.int32) == 0).all() and (self.y_n.view(torch.int32) == self.mr).all()
        assert torch.equal(self.n_fst, self.y_fst) and torch.equal(self.n_n, self.y_n)
        assert torch.equal(self.n_idx, self.y_idx) and torch.equal(self.n_co, self.y_co)
        assert torch.equal(self.n_rl, self.y_rl)
        assert (self.y_st.view(torch.int32) == 0).all() and torch.equal(self.n_st, self.y_st), "statuses differ"
        assert (self.y_nrec.view(torch.int32) == recovered).all() and torch.equal(self.n_nrec, self.y_nrec)
        assert torch.equal(self.n_ri, self.y_ri), "rec_index differs"
        assert torch.equal(self.n_rec, self.y_rec), "recovered rows differ"


def run_shape(qf, ctx, name, reps, G_override=0):
    K, n_sys, n_front, n_behind, planted, r, L, G, pool = SHAPES[name]
    st = Step(qf, ctx, name, G_override)
    G, mr = st.G, st.mr
    recovered = K - n_sys
    st.check(recovered)
    s = {n: [] for n in ("new_step", "yard_step", "new_parse", "yard_parse", "new_decode", "yard_decode")}
    nk, yk = [], []
    for _ in range(reps):
        s["new_step"].append(round(timed(st.n_step, ctx), 4))
        s["yard_step"].append(round(timed(st.y_step, ctx), 4))
        s["new_parse"].append(round(timed(st.n_parse, ctx), 4))
        s["yard_parse"].append(round(timed(st.y_parse, ctx), 4))
        s["new_decode"].append(round(timed(st.n_decode, ctx), 4))
        s["yard_decode"].append(round(timed(st.y_decode, ctx), 4))
        nk.append(kernel_split(st.n_step, ctx))
        yk.append(kernel_split(st.y_step, ctx))
    med = statistics.median

    def payload(t):
        return round(sum(ms for n, ms in t.items() if n not in FIXED), 5)

    n_pay, y_pay = [payload(t) for t in nk], [payload(t) for t in yk]
    y_pay_names = sorted({n for t in yk for n in t if n not in FIXED})
    passes = (min(K, r) + 15) // 16
    active = (recovered + 15) // 16                       # passes with a row to write
    # rows each payload pass reads per generation: the yardstick every slot up
    # to its last accepted one, the in-place pass the accepted ones
    y_rows = statistics.mean(int(np.flatnonzero(p[2])[-1]) + 1 for p in st.pats)
    n_rows = K
    y_bytes = int(G * (active * (y_rows * L + (mr + 1) * 16) + recovered * L))
    n_rec_bytes = ((min(K, mr) + 1) // 2 + 1) * 48
    n_bytes = int(G * (active * (n_rows * L + n_rec_bytes) + recovered * L + 8))
    added = int(G * (active * (n_rec_bytes - (mr + 1) * 16) + 8))
    y_spread = (max(y_pay) - min(y_pay)) / med(y_pay)
    bound = 1 + added / y_bytes + y_spread
    ratio_b = med(n_pay) / med(y_pay)
    kmed = lambda ks: {n: med(t.get(n, 0.0) for t in ks) for n in sorted({n for t in ks for n in t})}   # noqa: E731
    return {
        "shape": {"k": K, "r": r, "rows": mr, "systematic": n_sys, "coded": mr - n_sys, "planted_dependent": planted,
                  "recovered": recovered, "L": L, "G": G, "frame_stride": st.fs, "payload_offset": st.P,
                  "patterns": pool},
        "outputs_checked": "both steps: identical rec, rec_index, n_rec and status, every status QF_OK; the two "
                           "parsers' row_index, n_rows, row_coeffs, row_len and frame_status equal",
        "step": {
            "new_call_ms": s["new_step"], "yardstick_call_ms": s["yard_step"],
            "new_call_ms_median": med(s["new_step"]), "new_call_ms_min_max": spread(s["new_step"]),
            "yardstick_call_ms_median": med(s["yard_step"]), "yardstick_call_ms_min_max": spread(s["yard_step"]),
            "ratio_new_to_yardstick": round(med(s["new_step"]) / med(s["yard_step"]), 4),
            "saved_ms": round(med(s["yard_step"]) - med(s["new_step"]), 4),
        },
        "calls": {
            "new_parse_ms_median": med(s["new_parse"]), "yardstick_parse_ms_median": med(s["yard_parse"]),
            "new_parse_ms_min_max": spread(s["new_parse"]), "yardstick_parse_ms_min_max": spread(s["yard_parse"]),
            "new_decode_ms_median": med(s["new_decode"]), "yardstick_decode_ms_median": med(s["yard_decode"]),
            "new_decode_ms_min_max": spread(s["new_decode"]), "yardstick_decode_ms_min_max": spread(s["yard_decode"]),
        },
        "kernels_ms_median": {"new": kmed(nk), "yardstick": kmed(yk)},
        "kernels_ms": {"new": nk, "yardstick": yk},
        "payload_kernel": {
            "new": "k_combine_rows_at", "yardstick": y_pay_names, "passes_launched": passes,
            "passes_with_output": active,
            "new_ms": n_pay, "yardstick_ms": y_pay,
            "new_ms_median": med(n_pay), "yardstick_ms_median": med(y_pay),
            "new_ms_min_max": spread(n_pay), "yardstick_ms_min_max": spread(y_pay),
            "ratio_new_to_yardstick": round(ratio_b, 4),
            "rows_read_per_pass": {"new": n_rows, "yardstick": y_rows},
            "new_bytes": n_bytes, "yardstick_bytes": y_bytes, "new_to_yardstick_bytes": round(n_bytes / y_bytes, 4),
            "added_descriptor_bytes": added, "added_bytes_fraction": round(added / y_bytes, 5),
            "yardstick_relative_spread": round(y_spread, 5),
            "expectation": "ratio <= 1 + added descriptor bytes / yardstick bytes + the yardstick's relative "
                           "min-max spread",
            "expected_ratio_at_most": round(bound, 4),
            "expectation_met": bool(ratio_b <= bound),
        },
    }


def run_unused_passes(qf, ctx, reps, G_override=0):
    """Shape a with r = 64 (four passes launched, one with rows to write)
    against r = 16: what the three empty passes cost."""
    import torch

    name = "a_51sys_26coded_r16"
    res = {}
    ref = None
    for r in (16, 64):
        st = Step(qf, ctx, name, G_override, r_override=r)
        st.n_step()
        ctx.sync()
        assert (st.n_st.view(torch.int32) == 0).all() and (st.n_nrec.view(torch.int32) == 13).all()
        rec = st.n_rec.view(st.G, st.em, st.rs)[:, :13].clone()
        if ref is None:
            ref = rec
        else:
            assert torch.equal(rec, ref), "the recovered rows depend on r"
        t = [round(timed(st.n_decode, ctx), 4) for _ in range(reps)]
        ks = [kernel_split(st.n_decode, ctx) for _ in range(reps)]
        res[f"r{r}"] = {"decode_call_ms": t, "decode_call_ms_median": statistics.median(t),
                        "decode_call_ms_min_max": spread(t),
                        "k_combine_rows_at_ms_median": statistics.median(k["k_combine_rows_at"] for k in ks),
                        "k_decode_prepare_ms_median": statistics.median(k["k_decode_prepare"] for k in ks),
                        "passes_launched": (min(st.K, r) + 15) // 16}
        del st, rec
        torch.cuda.empty_cache()
    res["three_empty_passes_payload_ms"] = round(res["r64"]["k_combine_rows_at_ms_median"] -
                                                 res["r16"]["k_combine_rows_at_ms_median"], 5)
    res["call_ms_difference"] = round(res["r64"]["decode_call_ms_median"] - res["r16"]["decode_call_ms_median"], 4)
    return res


def main():
    import torch

    from quicfuscate_amd import fec as qf

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--generations", type=int, default=0, help="override G (a smoke run)")
    ap.add_argument("--out", default="profiles/recv_inplace_bench.json")
    a = ap.parse_args()
    assert torch.cuda.is_available()
    ctx = qf.default_context()
    prop = torch.cuda.get_device_properties(0)
    res = {"tool": "tools/bench_recv_inplace.py", "device": torch.cuda.get_device_name(0),
           "arch": getattr(prop, "gcnArchName", ""), "compute_units": prop.multi_processor_count,
           "timing": f"device events, windows of >= 0.5 s after a warm-up, {a.reps} repetitions, the two steps "
                     "alternated in one process; per-kernel times from qf_ctx_profile; medians with min-max",
           "new_step": "qf_parse_frame_headers_dev, qf_decode_frames_dev from the frame slots",
           "yardstick_step": "qf_parse_frames_coded_dev, qf_decode_innovative_batch",
           "shapes": {}}
    for name in a.shapes.split(","):
        res["shapes"][name] = run_shape(qf, ctx, name, a.reps, a.generations)
        print(f"{name}: step ratio {res['shapes'][name]['step']['ratio_new_to_yardstick']}", file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
    res["unused_passes"] = run_unused_passes(qf, ctx, a.reps, a.generations)
    Path(a.out).parent.mkdir(exist_ok=True, parents=True)
    Path(a.out).write_text(json.dumps(res, indent=1))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
