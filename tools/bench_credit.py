#!/usr/bin/env python3
"""Timing of the feedback calls: qf_credit_update_dev and
qf_rank_report_sel_dev over a window of G generations with N reports.

    python tools/bench_credit.py --out profiles/credit_bench.json

Workload: G = 65,536 slots, k = 64, every slot open, ranks 0 .. k, rho = 5/4,
cap = 4 k, N = G/64, G/16, G/4 reports for distinct slots (three in four for
the held generation, the rest stale or early).  Reported:
  (a) qf_credit_update_dev against qf_gen_select_dev over the same G (rank
      against sent, min_rank 1: the parent's closest dense pass over the slots),
      with the expectation  credit <= select + one memset of G u32 measured
      alone + the select's own min-max spread;
  (b) the host step it replaces, by wall clock: rank, sent, the window and the
      reports down, the rule in vectorised numpy, the credit up;
  (c) qf_rank_report_sel_dev against qf_gen_window_sel_dev over the same list
      of N entries (both one kernel with a lane per entry; the report call
      without and with QF_REPORT_APPEND, which adds a 4-byte device copy).
Before it times anything the tool asserts both calls' outputs against
tests/credit_ref.py, and the numpy rule of (b) against the call.  Times: device
events over windows of >= 0.5 s after a warm-up, medians with min-max over the
repetitions, steps alternated in one process; per-kernel times from
qf_ctx_profile.  Prints one JSON line."""
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
K, NUM, DEN = 64, 5, 4
CAP = 4 * K
BASE = 1 << 40


def host_rule(win, rank, sent, rep, n, owner, peer, credit):
    """The rule of qf_credit_update_dev in vectorised numpy (every slot open, every id < 2^62) -> credit;
    owner, peer are the host's copy of the state and are updated."""
    G = win.size
    rep = rep[:n]
    ok = (rep["rank"] <= K) & (rep["reserved"] == 0)
    slot = (rep["id"] % np.uint64(G)).astype(np.int64)
    ok &= win[slot] == rep["id"] + np.uint64(1)
    fresh = np.zeros(G, np.int64)
    np.maximum.at(fresh, slot[ok], rep["rank"][ok].astype(np.int64) + 1)
    mine = owner == win
    p = np.where(mine, peer, 0)
    prev = np.where(mine, credit, 0).astype(np.int64)
    r = np.minimum(rank, K).astype(np.int64)
    p = np.maximum(p, fresh - 1)
    c = np.maximum(prev, (r * NUM + DEN - 1) // DEN)
    ask = sent.astype(np.int64) + (np.maximum(r - p, 0) * NUM + DEN - 1) // DEN
    c = np.where(fresh > 0, np.maximum(c, ask), c)
    c = np.where(p >= K, sent, np.minimum(c, CAP))
    owner[:], peer[:] = win, p
    return c.astype(np.uint32)


def run(qf, ctx, hip, G, N, reps):
    import torch

    from tests import credit_ref as C

    rng = np.random.default_rng(G + N)
    dev = "cuda"
    win_h = (np.arange(G, dtype=np.uint64) + np.uint64(BASE + G + 1))
    rank_h = rng.integers(0, K + 1, G).astype(np.uint32)
    sent_h = (rng.random(G) * (rank_h + 1)).astype(np.uint32)
    slots = rng.permutation(G)[:N]
    rep_h = np.zeros(N, C.REPORT)
    cyc = rng.choice([1, 1, 1, 0, 2], N)
    rep_h["id"] = (BASE + cyc * G + slots).astype(np.uint64)
    rep_h["rank"] = rng.integers(0, K + 1, N)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)   # noqa: E731
    win, rank, sent, rep = up(win_h), up(rank_h), up(sent_h), up(rep_h)
    n_rep = up(np.array([N], np.uint32))
    state = torch.zeros(16 * G, dtype=torch.uint8, device=dev)
    credit = torch.full((4 * G,), 0xCC, dtype=torch.uint8, device=dev)
    status = torch.full((4 * N,), 0xCC, dtype=torch.uint8, device=dev)
    sel, n_sel = torch.zeros(G, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    work = torch.zeros(G, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    h = lambda t, dt=np.uint8: t.cpu().numpy().view(dt)   # noqa: E731

    def update():
        qf.credit_update(win, rank, sent, state, credit, K, G=G, num=NUM, den=DEN, cap=CAP, N_max=N, reports=rep,
                         n_reports=n_rep, report_status=status, ctx=ctx)

    def select():
        qf.gen_select(rank, sel, n_sel, G=G, min_rank=1, n_max=G, seen=sent, ctx=ctx)

    def memset():
        err = hip.hipMemsetAsync(ctypes.c_void_p(work.data_ptr()), 0, ctypes.c_size_t(4 * G), ctypes.c_void_p(stream))
        assert err == 0, f"hipMemsetAsync: {err}"

    # the call against the model: a first call, then a second one from the state it left
    c = C.CreditCall(K, NUM, DEN, CAP, win_h, rank_h, sent_h, rep_h, N, N)
    want = c.model()
    update()
    ctx.sync()
    assert np.array_equal(h(credit, np.uint32), want["credit"]) and np.array_equal(h(status, np.int32), want["status"])
    assert np.array_equal(h(state), want["state"].view(np.uint8))
    want2 = c.model(want)
    update()
    ctx.sync()
    assert np.array_equal(h(credit, np.uint32), want2["credit"]) and np.array_equal(h(state), want2["state"].view(np.uint8))
    n_ok = int((want["status"] == 0).sum())
    # the host's numpy rule gives the same credit
    owner, peer = np.zeros(G, np.uint64), np.zeros(G, np.int64)
    hc = host_rule(win_h, rank_h, sent_h, rep_h, N, owner, peer, np.zeros(G, np.uint32))
    assert np.array_equal(hc, want["credit"])
    assert np.array_equal(host_rule(win_h, rank_h, sent_h, rep_h, N, owner, peer, hc), want2["credit"])

    def host_step():
        t0 = time.perf_counter()
        rk, sn = h(rank, np.uint32), h(sent, np.uint32)
        wn, rp = h(win, np.uint64), h(rep).view(C.REPORT)
        n = int(h(n_rep, np.uint32)[0])
        t1 = time.perf_counter()
        out = host_rule(wn, rk, sn, rp, n, owner, peer, hc)
        t2 = time.perf_counter()
        credit.copy_(torch.from_numpy(out.view(np.uint8)), non_blocking=False)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        return (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3

    # (c): a list of N slots, every third entry closed at the receiver
    rwin_h = win_h.copy()
    rwin_h[slots[::3]] |= np.uint64(C.CLOSED)
    rwin = up(rwin_h)
    lst, n_lst = up(slots.astype(np.uint32)), up(np.array([N], np.uint32))
    reports = torch.full((16 * N,), 0xCC, dtype=torch.uint8, device=dev)
    n_out, n_left = up(np.zeros(1, np.uint32)), up(np.zeros(1, np.uint32))
    ids = torch.zeros(N, dtype=torch.int64, device=dev)

    def report(append=False):
        qf.rank_report_sel(lst, n_lst, rwin, rank, reports, n_out, K, n_max=N, G_src=G, N_max=N, n_left=n_left,
                           append=append, ctx=ctx)

    def report_append():
        n_out.zero_()
        report(True)

    def zero_only():
        n_out.zero_()

    def window_sel():
        qf.gen_window_sel(lst, n_lst, rwin, n_max=N, G_src=G, ids=ids, ctx=ctx)

    rc = C.ReportCall(K, slots.astype(np.uint32), rwin_h, rank_h, N, n_sel=N)
    rw = rc.model()
    report()
    ctx.sync()
    assert np.array_equal(h(reports), rw["reports"].view(np.uint8)) and int(h(n_out, np.uint32)[0]) == N
    assert int(h(n_left, np.uint32)[0]) == 0

    steps = {"credit_update": update, "gen_select": select, "memset_G_u32": memset, "rank_report_sel": report,
             "rank_report_sel_append_with_zeroing": report_append, "zeroing_alone": zero_only,
             "gen_window_sel": window_sel}
    t = {name: [] for name in steps}
    ks, host = {}, []
    for _ in range(reps):
        for name, fn in steps.items():
            t[name].append(round(B.timed(fn, ctx), 5))
        for fn in (update, report):
            for kn, ms in B.kernel_split(fn, ctx).items():
                ks.setdefault(kn, []).append(ms)
        ctx.sync()
        host.append(host_step())
        update()
    m = {name: med(v) for name, v in t.items()}
    sp = max(t["gen_select"]) - min(t["gen_select"])
    bound = m["gen_select"] + m["memset_G_u32"] + sp
    hm = lambda i: med([x[i] for x in host])   # noqa: E731
    return {
        "shape": {"k": K, "G": G, "reports": N, "reports_ok": n_ok, "rho": f"{NUM}/{DEN}", "cap": CAP},
        "outputs_checked": "credit, state and report statuses of two consecutive calls and the reports of the list "
                           "against tests/credit_ref.py; the host's numpy rule against the call",
        "ms": t, "ms_median": m, "ms_min_max": {name: B.spread(v) for name, v in t.items()},
        "kernels_ms": {kn: med(v) for kn, v in ks.items()},
        "kernels_ms_min_max": {kn: B.spread(v) for kn, v in ks.items()},
        "a_credit_against_select": {
            "credit_update_ms": m["credit_update"], "gen_select_ms": m["gen_select"], "memset_ms": m["memset_G_u32"],
            "gen_select_spread_ms": round(sp, 5), "ratio_to_select": round(m["credit_update"] / m["gen_select"], 4),
            "expectation": "credit_update <= gen_select + memset of G u32 alone + the select's min-max spread",
            "expected_ms_at_most": round(bound, 5), "expectation_met": bool(m["credit_update"] <= bound)},
        "b_host_step_replaced": {
            "downloads_ms": hm(0), "numpy_rule_ms": hm(1), "upload_ms": hm(2),
            "host_ms": med([sum(x) for x in host]), "host_ms_min_max": B.spread([round(sum(x), 4) for x in host]),
            "credit_update_ms": m["credit_update"], "note": "host wall time, pageable host memory"},
        "c_report_against_window_sel": {
            "rank_report_sel_ms": m["rank_report_sel"], "gen_window_sel_ms": m["gen_window_sel"],
            "ratio": round(m["rank_report_sel"] / m["gen_window_sel"], 4),
            "append_ms_less_zeroing": round(m["rank_report_sel_append_with_zeroing"] - m["zeroing_alone"], 5)},
    }


def main():
    import torch

    from quicfuscate_amd import fec as qf

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--generations", type=int, default=65536)
    ap.add_argument("--fractions", default="64,16,4", help="N = G / each")
    ap.add_argument("--out", default="profiles/credit_bench.json")
    a = ap.parse_args()
    assert torch.cuda.is_available()
    ctx = qf.default_context()
    hip = S._hip()
    prop = torch.cuda.get_device_properties(0)
    res = {"tool": "tools/bench_credit.py", "device": torch.cuda.get_device_name(0),
           "arch": getattr(prop, "gcnArchName", ""), "compute_units": prop.multi_processor_count,
           "timing": f"device events, windows of >= 0.5 s after a warm-up, {a.reps} repetitions, steps alternated in one "
                     "process; per-kernel times from qf_ctx_profile; medians with min-max; the host step by wall clock",
           "runs": {}}
    G = a.generations
    for f in (int(x) for x in a.fractions.split(",")):
        key = f"N_G_over_{f}"
        res["runs"][key] = r = run(qf, ctx, hip, G, G // f, a.reps)
        ra, rb, rc = r["a_credit_against_select"], r["b_host_step_replaced"], r["c_report_against_window_sel"]
        print(f"{key}: credit {ra['credit_update_ms']:.4f} ms, select {ra['gen_select_ms']:.4f}, memset "
              f"{ra['memset_ms']:.4f}, bound {ra['expected_ms_at_most']:.4f}: "
              f"{'met' if ra['expectation_met'] else 'not met'}; host step {rb['host_ms']:.3f} ms; report "
              f"{rc['rank_report_sel_ms']:.4f} ms, {rc['ratio']} of window_sel", file=sys.stderr, flush=True)
    Path(a.out).parent.mkdir(exist_ok=True, parents=True)
    Path(a.out).write_text(json.dumps(res, indent=1))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
