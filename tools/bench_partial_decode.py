#!/usr/bin/env python3
"""Timing of the partial decode over a list:
qf_decode_partial_frames_sel_dev over n incomplete generations of a row store
of G, against qf_decode_frames_sel_dev over n complete generations that
recover the same number of rows.

    python tools/bench_partial_decode.py --out profiles/partial_decode_bench.json

Workload: k = 64, L = 1,200, G = 65,536, cap = 64, r = 16, 64 patterns tiled,
n = G/64 and G/16 listed generations spread evenly over the G.
  partial    each generation holds 52 systematic and 8 coded rows; 4 of the
             coded rows lie over the held sources and one further source each
             (4 determined sources), the other 4 over the held sources and the
             8 remaining unknowns (they determine nothing)
  yardstick  each generation holds 60 systematic and 4 dense coded rows: rank
             k, 4 recovered rows; code the partial decode does not touch
Before it times anything it asserts the partial call's outputs against
tests/partial_ref.py and the sources, and the yardstick's against the sources.
Times: device events over windows of >= 0.5 s after a warm-up, medians with
min-max over the repetitions, the two steps alternated in one process;
per-kernel times from qf_ctx_profile.  Expectation (reported, not a gate):
partial <= yardstick * (1 + the yardstick's relative min-max spread).  Prints
one JSON line."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tools"))

import bench_recv_inplace as B  # noqa: E402
from tests import partial_ref as P  # noqa: E402

K, L, R, CAP, POOL = 64, 1200, 16, 64, 64
N_SYS, N_CODED, N_DET = 52, 8, 4
med = statistics.median


def partial_pattern(rng):
    """52 systematic rows and 8 coded rows in a random arrival order -> vectors, the determined sources."""
    perm = rng.permutation(K)
    S, E = sorted(perm[:N_SYS].tolist()), sorted(perm[N_SYS:].tolist())
    det = E[:N_DET]
    vecs = [P.unit(K, i) for i in S]
    vecs += [P.over(rng, K, S + [i]) for i in det]
    vecs += [P.over(rng, K, S + E[N_DET:]) for _ in range(N_CODED - N_DET)]
    return [vecs[i] for i in rng.permutation(len(vecs))], det


def complete_pattern(rng):
    """60 systematic rows and 4 dense coded rows in a random arrival order."""
    perm = rng.permutation(K)
    vecs = [P.unit(K, i) for i in perm[: K - N_DET]] + [rng.integers(1, 256, K, dtype=np.uint8) for _ in range(N_DET)]
    return [vecs[i] for i in rng.permutation(len(vecs))]


class Store:
    """A row store of G generations tiled from POOL patterns, on the device."""

    def __init__(self, ctx, G, gens):
        import torch

        self.G, self.gens = G, gens
        self.rs = rs = (L + 15) // 16 * 16
        self.gs = CAP * rs
        dev = f"cuda:{ctx.device}"
        byt = np.zeros((POOL, CAP, rs), np.uint8)
        off = np.tile(np.arange(CAP, dtype=np.uint32) * rs, (POOL, 1))
        ln = np.full((POOL, CAP), L, np.uint32)
        idx = np.zeros((POOL, CAP), np.uint16)
        co = np.zeros((POOL, CAP, K), np.uint8)
        n = np.zeros(POOL, np.uint32)
        for p, g in enumerate(gens):
            m = len(g.idx)
            byt[p, :m, :L], idx[p, :m], co[p, :m], n[p] = g.rows, np.minimum(g.idx, K), g.coeffs, m
        tile = G // POOL
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(POOL, -1)).to(dev).repeat(tile, 1)  # noqa: E731
        self.arrays = [up(byt), up(off), up(ln), up(idx), up(co)]
        self.n_rows = up(n)


def refs_of(gens):
    return [P.partial_ref(K, R, L, np.minimum(g.idx, K), g.coeffs, [g.rows[s].tobytes() for s in range(len(g.idx))])
            for g in gens]


def run(qf, ctx, G, n, reps):
    import torch

    dev = f"cuda:{ctx.device}"
    rng = np.random.default_rng(2033)
    pgens, dets = [], []
    for _ in range(POOL):
        vecs, det = partial_pattern(rng)
        g = P.Gen(rng, K, L, vecs, src=rng.integers(0, 256, (K, L), dtype=np.uint8))
        pgens.append(g)
        dets.append(det)
    cgens = [P.Gen(rng, K, L, complete_pattern(rng), src=rng.integers(0, 256, (K, L), dtype=np.uint8))
             for _ in range(POOL)]
    part, comp = Store(ctx, G, pgens), Store(ctx, G, cgens)
    rs, em = part.rs, min(K, R)
    sel = torch.arange(0, G, G // n, device=dev, dtype=torch.int32)
    n_sel = torch.full((1,), n, dtype=torch.int32, device=dev)
    z = lambda nb: torch.zeros(nb, dtype=torch.uint8, device=dev)   # noqa: E731
    rec, ri, nrec, st, slot, rank = z(n * em * rs), z(2 * n * em), z(4 * n), z(4 * n), z(2 * n * K), z(4 * n)
    kw = dict(n_max=n, G_src=G, max_rows=CAP, src_gen_stride=part.gs, rec_row_stride=rs, rec_gen_stride=em * rs,
              src_slot=slot, rank=rank, ctx=ctx)

    def partial():
        qf.decode_partial_frames_sel(sel, n_sel, *part.arrays, rec, ri, nrec, st, K, R, L, n_rows=part.n_rows, **kw)

    def yardstick():
        qf.decode_frames_sel(sel, n_sel, *comp.arrays, rec, ri, nrec, st, K, R, L, n_rows=comp.n_rows, **kw)

    def outputs():
        ctx.sync()
        h = lambda t, dt: t.cpu().numpy().view(dt)   # noqa: E731
        return (h(rec, np.uint8).reshape(n, em, rs), h(ri, np.uint16).reshape(n, em), h(nrec, np.uint32),
                h(st, np.int32), h(slot, np.uint16).reshape(n, K), h(rank, np.uint32))

    # correctness first: the partial call against the model and the sources, the yardstick against the sources
    prefs = refs_of(pgens)
    for p, (ref, det) in enumerate(zip(prefs, dets)):
        assert ref["D"] == det and ref["status"] == P.ENOTREADY and ref["rank"] == N_SYS + N_CODED
        assert ref["bound"] == N_SYS + N_DET, "the determined sources use the held systematic rows and their own coded row"
    pat = (np.arange(0, G, G // n) % POOL)
    partial()
    o_rec, o_ri, o_nrec, o_st, o_slot, o_rank = outputs()
    assert (o_st == P.ENOTREADY).all() and (o_nrec == N_DET).all() and (o_rank == N_SYS + N_CODED).all()
    for j in range(n):
        ref, g = prefs[pat[j]], pgens[pat[j]]
        assert o_ri[j, :N_DET].tolist() == ref["D"] and np.array_equal(o_slot[j], ref["src_slot"]), j
        assert np.array_equal(o_rec[j, :N_DET, :L], ref["rec"]) and np.array_equal(ref["rec"], g.src[ref["D"]]), j
    yardstick()
    o_rec, o_ri, o_nrec, o_st, o_slot, o_rank = outputs()
    assert (o_st == P.OK).all() and (o_nrec == N_DET).all() and (o_rank == K).all()
    for j in range(0, n, max(1, n // 256)):
        g = cgens[pat[j]]
        assert np.array_equal(o_rec[j, :N_DET, :L], g.src[o_ri[j, :N_DET]]), j
    steps = {"partial_listed": partial, "yardstick_full_decode_listed": yardstick}
    t = {name: [] for name in steps}
    ks = {name: {} for name in steps}
    for _ in range(reps):
        for name, fn in steps.items():
            t[name].append(round(B.timed(fn, ctx), 5))
            for kn, ms in B.kernel_split(fn, ctx).items():
                ks[name].setdefault(kn, []).append(ms)
    y = t["yardstick_full_decode_listed"]
    spread = (max(y) - min(y)) / med(y)
    bound = med(y) * (1 + spread)
    pm = med(t["partial_listed"])
    out = {
        "shape": {"k": K, "L": L, "r": R, "G_src": G, "cap": CAP, "listed": n,
                  "partial_rows": f"{N_SYS} systematic + {N_CODED} coded, {N_DET} sources determined, "
                                  f"{N_SYS + N_DET} rows read",
                  "yardstick_rows": f"{K - N_DET} systematic + {N_DET} coded, rank k, {N_DET} recovered, {K} rows read"},
        "outputs_checked": "partial: status, n_rec, rec_index, src_slot and rows against tests/partial_ref.py and the "
                           "sources for every listed generation; yardstick: rows against the sources",
        "ms": t, "ms_median": {name: med(v) for name, v in t.items()},
        "ms_min_max": {name: B.spread(v) for name, v in t.items()},
        "kernels_ms": {name: {kn: med(v) for kn, v in d.items()} for name, d in ks.items()},
        "expectation": "partial <= yardstick * (1 + the yardstick's relative min-max spread)",
        "yardstick_relative_spread": round(spread, 5), "expected_ms_at_most": round(bound, 5),
        "ratio_to_yardstick": round(pm / med(y), 4), "expectation_met": bool(pm <= bound),
    }
    del part, comp
    torch.cuda.empty_cache()
    return out


def main():
    import torch

    from quicfuscate_amd import fec as qf

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--generations", type=int, default=65536)
    ap.add_argument("--fractions", default="64,16", help="n = G / each")
    ap.add_argument("--out", default="profiles/partial_decode_bench.json")
    a = ap.parse_args()
    assert torch.cuda.is_available()
    ctx = qf.default_context()
    prop = torch.cuda.get_device_properties(0)
    res = {"tool": "tools/bench_partial_decode.py", "device": torch.cuda.get_device_name(0),
           "arch": getattr(prop, "gcnArchName", ""), "compute_units": prop.multi_processor_count,
           "timing": f"device events, windows of >= 0.5 s after a warm-up, {a.reps} repetitions, the two steps alternated "
                     "in one process; per-kernel times from qf_ctx_profile; medians with min-max",
           "yardstick": "qf_decode_frames_sel_dev over the same number of complete generations, each recovering as many "
                        "rows as the partial call delivers",
           "runs": {}}
    G = a.generations
    for f in (int(x) for x in a.fractions.split(",")):
        key = f"n_G_over_{f}"
        res["runs"][key] = d = run(qf, ctx, G, G // f, a.reps)
        print(f"{key}: partial {d['ms_median']['partial_listed']:.4f} ms, yardstick "
              f"{d['ms_median']['yardstick_full_decode_listed']:.4f} ms, ratio {d['ratio_to_yardstick']}, bound "
              f"{d['expected_ms_at_most']} ({'met' if d['expectation_met'] else 'not met'})", file=sys.stderr, flush=True)
    Path(a.out).parent.mkdir(exist_ok=True, parents=True)
    Path(a.out).write_text(json.dumps(res, indent=1))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
