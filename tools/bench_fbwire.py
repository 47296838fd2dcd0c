#!/usr/bin/env python3
"""Timing of the feedback packets' calls: qf_frame_reports_dev,
qf_parse_report_frames_dev and qf_report_closed_dev.

    python tools/bench_fbwire.py --out profiles/fbwire_bench.json

Workload: G = 65,536 slots, k = 64, N = G/64, G/16, G/4 records of which one in
eight is a hole, max_len 1,200 (119 entries per packet).  Reported:
  (a) the pack's and the parse's kernels against the parent's closest two-launch
      prefix step, k_emit_count + k_emit_place of qf_emit_frames_sel_dev over
      the same number of entries (per-kernel times from qf_ctx_profile, in the
      same process), with the expectations
        pack  <= pair + the pair's own min-max spread
        parse <= pair + that spread + one k_report_sel launch measured alone;
  (b) qf_report_closed_dev against qf_gen_select_dev + qf_rank_report_sel_dev
      over the same G and list, with the expectation
        closed <= their sum + one memset of G u32 + one k_report_sel launch;
  (c) the host step the pack and the parse replace, by wall clock: the records
      down, a numpy pack, and on the other side a numpy parse and the upload.
Before it times anything the tool asserts the three calls' outputs against
tests/fbwire_ref.py, and the numpy pack and parse of (c) against the calls.
Times: device events over windows of >= 0.5 s after a warm-up, medians with
min-max over the repetitions, steps alternated in one process; per-kernel times
from qf_ctx_profile over 8 calls, the pack's both as the first profiled call of
a repetition ("first:", not compared) and as the last.  Prints one JSON line."""
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
K, MAX_LEN, STRIDE = 64, 1200, 1200
PER = (MAX_LEN - 3) // 10
BASE = 1 << 40
ECLOSED = -9


def host_pack(rep, n):
    """The sendable records of rep[:n] as packets of at most PER entries -> (slots [P, STRIDE] u8, lengths)."""
    r = rep[:n]
    r = r[(r["id"] < np.uint64(1 << 62)) & (r["rank"] <= K) & (r["reserved"] == 0)]
    S_ = r.size
    P = -(-S_ // PER)
    ent = np.zeros((P * PER, 10), np.uint8)
    ent[:S_, :8] = r["id"].astype(">u8").view(np.uint8).reshape(-1, 8)
    ent[:S_, 8:] = r["rank"].astype(">u2").view(np.uint8).reshape(-1, 2)
    out = np.zeros((P, STRIDE), np.uint8)
    cnt = np.minimum(PER, S_ - PER * np.arange(P)).astype(np.uint16)
    out[:, 0] = 2
    out[:, 1:3] = cnt.astype(">u2").view(np.uint8).reshape(-1, 2)
    out[:, 3: 3 + 10 * PER] = ent.reshape(P, PER * 10)
    return out, (3 + 10 * cnt.astype(np.uint32))


def host_parse(slots, lens, dtype):
    """The inverse, for well-formed packets -> records."""
    cnt = (lens - 3) // 10
    ent = slots[:, 3: 3 + 10 * PER].reshape(-1, PER, 10)
    keep = np.arange(PER)[None, :] < cnt[:, None]
    ent = ent[keep]
    out = np.zeros(ent.shape[0], dtype)
    out["id"] = np.ascontiguousarray(ent[:, :8]).view(">u8").reshape(-1)
    out["rank"] = np.ascontiguousarray(ent[:, 8:]).view(">u2").reshape(-1)
    return out


def run(qf, ctx, hip, G, N, reps):
    import torch

    from tests import credit_ref as C
    from tests import fbwire_ref as F

    rng = np.random.default_rng(G + N)
    dev = "cuda"
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)   # noqa: E731
    h = lambda t, dt=np.uint8: t.cpu().numpy().view(dt)   # noqa: E731
    filled = lambda n: torch.full((n,), 0xCC, dtype=torch.uint8, device=dev)   # noqa: E731
    one = lambda v=0: up(np.array([v], np.uint32))   # noqa: E731
    stream = torch.cuda.current_stream().cuda_stream
    # N records for distinct slots, one in eight a hole
    slots = rng.permutation(G)[:N]
    rep_h = np.zeros(N, C.REPORT)
    rep_h["id"] = (BASE + G + slots).astype(np.uint64)
    rep_h["rank"] = rng.integers(0, K + 1, N)
    rep_h[7::8] = (C.U64MAX, 0, 0)
    S_ = N - len(rep_h[7::8])
    F_max = -(-S_ // PER)
    rep, n_rep = up(rep_h), one(N)
    pkts, pkt_len, n_pkts, n_left, n_skip = filled(F_max * STRIDE), filled(4 * F_max), one(), one(), one()

    def pack():
        qf.frame_reports(rep, n_rep, pkts, pkt_len, n_pkts, K, N_max=N, max_len=MAX_LEN, F_max=F_max, stride=STRIDE,
                         n_left=n_left, n_skipped=n_skip, ctx=ctx)

    back, n_back, b_left = filled(16 * N), one(), one()
    p_st, p_first, p_cnt = filled(4 * F_max), filled(4 * F_max), filled(4 * F_max)

    def parse():
        qf.parse_report_frames(pkts, pkt_len, n_pkts, back, n_back, K, N_max=N, max_len=MAX_LEN, F_max=F_max,
                               stride=STRIDE, n_left=b_left, pkt_status=p_st, pkt_first=p_first, pkt_count=p_cnt, ctx=ctx)

    pc = F.PackCall(K, MAX_LEN, F_max, STRIDE, rep_h, N)
    want = pc.model()
    pack()
    ctx.sync()
    got = dict(pkts=h(pkts), pkt_len=h(pkt_len, np.uint32), n_pkts=h(n_pkts, np.uint32), n_left=h(n_left, np.uint32),
               n_skipped=h(n_skip, np.uint32))
    for key in want:
        assert np.array_equal(got[key], want[key]), f"frame_reports: {key}"
    qc = F.ParseCall(K, MAX_LEN, F_max, STRIDE, got["pkts"], got["pkt_len"], N, n_pkts=F_max)
    wantp = qc.model()
    parse()
    ctx.sync()
    gotp = dict(reports=h(back).view(C.REPORT), n_reports=h(n_back, np.uint32), n_left=h(b_left, np.uint32),
                pkt_status=h(p_st, np.int32), pkt_first=h(p_first, np.uint32), pkt_count=h(p_cnt, np.uint32))
    for key in wantp:
        assert np.array_equal(gotp[key], wantp[key]), f"parse_report_frames: {key}"
    # the host's numpy pack and parse give the same bytes and records
    hs, hl = host_pack(rep_h, N)
    sl = got["pkts"].reshape(F_max, STRIDE)
    assert np.array_equal(hl, got["pkt_len"]) and all(np.array_equal(hs[p, :hl[p]], sl[p, :hl[p]]) for p in range(F_max))
    assert np.array_equal(host_parse(sl, got["pkt_len"], C.REPORT), gotp["reports"][:S_])

    def host_step():
        t0 = time.perf_counter()
        r = h(rep).view(C.REPORT)
        n = int(h(n_rep, np.uint32)[0])
        t1 = time.perf_counter()
        s, ln = host_pack(r, n)
        t2 = time.perf_counter()
        recs = host_parse(s, ln, C.REPORT)
        t3 = time.perf_counter()
        back[: 16 * recs.size].copy_(torch.from_numpy(recs.view(np.uint8)), non_blocking=False)
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        return tuple((b - a) * 1e3 for a, b in ((t0, t1), (t1, t2), (t2, t3), (t3, t4)))

    # (a): the parent's two-launch prefix over N entries: one systematic row of 16 bytes per entry
    P = qf.frame_payload_offset(K)
    fs = P + 16
    e_sel, e_nsel = up(np.arange(N, dtype=np.uint32)), one(N)
    e_rows, e_ids = filled(16 * N), up(rep_h["id"] & np.uint64((1 << 62) - 1))
    e_idx = up((np.arange(N) % K).astype(np.uint16))
    e = {key: filled(n) for key, n in dict(frames=N * fs, frame_len=4 * N, frame_off=4 * N, frame_id=8 * N, frame_pkt=8 * N,
                                           n_frames=4, n_left=4, entry_first=4 * N, entry_count=4 * N,
                                           entry_status=4 * N).items()}

    def emit():
        qf.emit_frames_sel(e_sel, e_nsel, e_rows, e_ids, e["frames"], e["frame_len"], e["frame_off"], e["frame_id"],
                           e["frame_pkt"], e["n_frames"], e["entry_first"], e["entry_count"], e["entry_status"], K, 16,
                           n_max=N, G_src=N, max_rows=1, N_max=N, row_stride=16, rows_gen_stride=16, frame_stride=fs,
                           row_index=e_idx, n_left=e["n_left"], ctx=ctx)

    emit()
    ctx.sync()
    assert int(h(e["n_frames"], np.uint32)[0]) == N

    # (b): frames of N closed generations (and as many that the window contradicts) against select + report
    win_h = np.arange(G, dtype=np.uint64) + np.uint64(BASE + G + 1)
    win_h[slots] |= np.uint64(C.CLOSED)
    fid_h = np.concatenate([BASE + G + slots, BASE + G + rng.permutation(G)[:N]]).astype(np.uint64)
    fst_h = np.full(2 * N, ECLOSED, np.int32)
    win, fid, fst, n_fr = up(win_h), up(fid_h), up(fst_h), one(2 * N)
    c_rep, c_n, c_left = filled(16 * G), one(), one()

    def closed():
        qf.report_closed(fid, fst, n_fr, win, c_rep, c_n, K, G_src=G, F_max=2 * N, N_max=G, n_left=c_left, ctx=ctx)

    cc = F.ClosedCall(K, win_h, fid_h, fst_h, G, n_frames=2 * N)
    wantc = cc.model()
    closed()
    ctx.sync()
    assert np.array_equal(h(c_rep), wantc["reports"].view(np.uint8)) and int(h(c_n, np.uint32)[0]) == wantc["n_reports"][0]
    n_marked = int(wantc["n_reports"][0])
    flags = up(cc.flags())
    zero_rank = torch.zeros(G, dtype=torch.int32, device=dev)
    s_sel, s_n = torch.zeros(G, dtype=torch.int32, device=dev), one()
    work = torch.zeros(G, dtype=torch.int32, device=dev)

    def select():
        qf.gen_select(flags, s_sel, s_n, G=G, min_rank=1, n_max=G, ctx=ctx)

    def report():
        qf.rank_report_sel(s_sel, s_n, win, zero_rank, c_rep, c_n, K, n_max=G, G_src=G, N_max=G, n_left=c_left, ctx=ctx)

    def memset():
        err = hip.hipMemsetAsync(ctypes.c_void_p(work.data_ptr()), 0, ctypes.c_size_t(4 * G), ctypes.c_void_p(stream))
        assert err == 0, f"hipMemsetAsync: {err}"

    select()
    report()
    ctx.sync()
    assert np.array_equal(h(c_rep), wantc["reports"].view(np.uint8))

    steps = {"frame_reports": pack, "parse_report_frames": parse, "emit_frames_sel": emit, "report_closed": closed,
             "gen_select": select, "rank_report_sel": report, "memset_G_u32": memset}
    t = {name: [] for name in steps}
    ks, host = {}, []
    for _ in range(reps):
        for name, fn in steps.items():
            t[name].append(round(B.timed(fn, ctx), 5))
        # The pack is profiled twice, in front of the others and behind them: the first profiled call behind the
        # timed windows carries a start-up cost that the average over its few calls shows (kept as "first:").
        for tag, fn in (("first:", pack), ("", parse), ("", emit), ("closed:", closed), ("", report), ("", pack)):
            for kn, ms in B.kernel_split(fn, ctx, calls=8).items():
                ks.setdefault(tag + kn, []).append(ms)
        ctx.sync()
        host.append(host_step())
    m = {name: med(v) for name, v in t.items()}
    km = {kn: med(v) for kn, v in ks.items()}
    pair = [a + b for a, b in zip(ks["k_emit_count"], ks["k_emit_place"])]
    pack_k = [a + b for a, b in zip(ks["k_fbw_count"], ks["k_fbw_pack"])]
    parse_k = [a + b + c for a, b, c in zip(ks["k_fbr_count"], ks["k_fbr_place"], ks["k_fbr_records"])]
    sp = max(pair) - min(pair)
    pack_bound = med(pair) + sp
    parse_bound = pack_bound + km["k_report_sel"]
    sel_sp = max(t["gen_select"]) - min(t["gen_select"])
    closed_bound = m["gen_select"] + m["rank_report_sel"] + m["memset_G_u32"] + km["k_report_sel"]
    hm = lambda i: med([x[i] for x in host])   # noqa: E731
    return {
        "shape": {"k": K, "G": G, "records": N, "sendable": S_, "max_len": MAX_LEN, "entries_per_packet": PER,
                  "packets": F_max, "closed_frames": 2 * N, "closed_marked": n_marked},
        "outputs_checked": "every output of the three calls against tests/fbwire_ref.py; the host's numpy pack and parse "
                           "against the calls; select + report over the model's flags against report_closed",
        "ms": t, "ms_median": m, "ms_min_max": {name: B.spread(v) for name, v in t.items()},
        "kernels_ms": km, "kernels_ms_min_max": {kn: B.spread(v) for kn, v in ks.items()},
        "a_pack_and_parse_against_the_emit_prefix": {
            "emit_count_plus_place_ms": round(med(pair), 5), "pair_min_max": B.spread([round(x, 5) for x in pair]),
            "pair_spread_ms": round(sp, 5), "pack_kernels_ms": round(med(pack_k), 5),
            "pack_min_max": B.spread([round(x, 5) for x in pack_k]),
            "pack_expectation": "k_fbw_count + k_fbw_pack <= k_emit_count + k_emit_place + the pair's min-max spread",
            "pack_expected_ms_at_most": round(pack_bound, 5), "pack_expectation_met": bool(med(pack_k) <= pack_bound),
            "parse_kernels_ms": round(med(parse_k), 5), "parse_min_max": B.spread([round(x, 5) for x in parse_k]),
            "report_sel_alone_ms": km["k_report_sel"],
            "parse_expectation": "the three parse kernels <= the pair + its spread + one k_report_sel measured alone",
            "parse_expected_ms_at_most": round(parse_bound, 5), "parse_expectation_met": bool(med(parse_k) <= parse_bound),
            "pack_call_ms": m["frame_reports"], "parse_call_ms": m["parse_report_frames"]},
        "b_report_closed_against_its_parts": {
            "report_closed_ms": m["report_closed"], "gen_select_ms": m["gen_select"],
            "rank_report_sel_ms": m["rank_report_sel"], "memset_ms": m["memset_G_u32"],
            "report_sel_kernel_ms": km["k_report_sel"], "gen_select_spread_ms": round(sel_sp, 5),
            "expectation": "report_closed <= gen_select + rank_report_sel + memset of G u32 + one k_report_sel launch",
            "expected_ms_at_most": round(closed_bound, 5), "expectation_met": bool(m["report_closed"] <= closed_bound)},
        "c_host_step_replaced": {
            "download_ms": hm(0), "numpy_pack_ms": hm(1), "numpy_parse_ms": hm(2), "upload_ms": hm(3),
            "host_ms": med([sum(x) for x in host]), "host_ms_min_max": B.spread([round(sum(x), 4) for x in host]),
            "pack_plus_parse_calls_ms": round(m["frame_reports"] + m["parse_report_frames"], 5),
            "note": "host wall time, pageable host memory"},
    }


def main():
    import torch

    from quicfuscate_amd import fec as qf

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--generations", type=int, default=65536)
    ap.add_argument("--fractions", default="64,16,4", help="N = G / each")
    ap.add_argument("--out", default="profiles/fbwire_bench.json")
    a = ap.parse_args()
    assert torch.cuda.is_available()
    ctx = qf.default_context()
    hip = S._hip()
    prop = torch.cuda.get_device_properties(0)
    res = {"tool": "tools/bench_fbwire.py", "device": torch.cuda.get_device_name(0),
           "arch": getattr(prop, "gcnArchName", ""), "compute_units": prop.multi_processor_count,
           "timing": f"device events, windows of >= 0.5 s after a warm-up, {a.reps} repetitions, steps alternated in one "
                     "process; per-kernel times from qf_ctx_profile; medians with min-max; the host step by wall clock",
           "runs": {}}
    G = a.generations
    for f in (int(x) for x in a.fractions.split(",")):
        key = f"N_G_over_{f}"
        res["runs"][key] = r = run(qf, ctx, hip, G, G // f, a.reps)
        ra, rb, rc = (r["a_pack_and_parse_against_the_emit_prefix"], r["b_report_closed_against_its_parts"],
                      r["c_host_step_replaced"])
        print(f"{key}: emit pair {ra['emit_count_plus_place_ms']:.4f} ms; pack {ra['pack_kernels_ms']:.4f} (<= "
              f"{ra['pack_expected_ms_at_most']:.4f}: {'met' if ra['pack_expectation_met'] else 'not met'}); parse "
              f"{ra['parse_kernels_ms']:.4f} (<= {ra['parse_expected_ms_at_most']:.4f}: "
              f"{'met' if ra['parse_expectation_met'] else 'not met'}); closed {rb['report_closed_ms']:.4f} (<= "
              f"{rb['expected_ms_at_most']:.4f}: {'met' if rb['expectation_met'] else 'not met'}); host step "
              f"{rc['host_ms']:.3f} ms", file=sys.stderr, flush=True)
    Path(a.out).parent.mkdir(exist_ok=True, parents=True)
    Path(a.out).write_text(json.dumps(res, indent=1))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
