#!/usr/bin/env python3
"""Timing of the delivery step: qf_deliver_frames_sel_dev over the
outputs of qf_decode_frames_sel_dev for the n complete generations of a row
store of G.

    python tools/bench_deliver.py --out profiles/deliver_bench.json

Workload: tools/bench_stream_select.py's store (k = 64, L = 1,200, G = 65,536,
cap = 64, 51 stored + 13 recovered sources per listed generation), n = G/64,
G/16, G/4, the list sized n_max = n.  Reported:
  (a) k_deliver_rows_sel against one contiguous device-to-device hipMemcpyAsync
      of the bytes it copies (n * k * L), with the expectation
      ratio <= 1 + record bytes / bytes moved + the copy's relative spread
      (record bytes: 16 per packet; bytes moved: read + written, 2 * n * k * L);
  (b) the whole call (k_deliver_prepare_sel + k_deliver_rows_sel) against
      select + the listed decode in front of it;
  (c) the host step it replaces, at every n: the five downloads (sel, src_slot,
      rec_index, n_rec, status) plus the address-building loop as vectorised
      numpy, no payload copies; host wall time.
The calls are timed without a delivered state (with one, a repeated call
delivers nothing); the state costs five 8-byte words per entry in the control
kernel.  Before it times anything the tool asserts the call's outputs: every
entry against the decode's outputs and the store on the device, a sample of
entries against tests/deliver_ref.py, and a second call with a state delivers
nothing.
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


class Deliver:
    """The store of bench_stream_select, the listed decode with src_slot, the deliver call's buffers."""

    def __init__(self, qf, ctx, G, n):
        import torch

        self.s = s = S.Store(qf, ctx, G, n)
        self.qf, self.ctx, self.G, self.n = qf, ctx, G, n
        K, rs = s.K, s.rs
        z = s.z
        self.slot = z(2 * n * K)
        self.out, self.out_len, self.out_state = z(n * K * rs), z(4 * n * K), z(n * K)
        self.n_out, self.n_known, self.status = z(4 * n), z(4 * n), z(4 * n)
        self.ids = torch.arange(n, dtype=torch.int64, device=s.dev) + (1 << 40)
        self.state = z(8 * qf.QF_DELIVERED_WORDS * G)

    def decode(self):
        s, n = self.s, self.n
        b, o, l, i, c = s.big
        self.qf.decode_frames_sel(s.sel, s.n_sel, b, o, l, i, c, s.rec, s.ri, s.nrec, s.st, s.K, s.r, s.L, n_max=n,
                                  G_src=self.G, n_rows=s.big_n, src_slot=self.slot, **s._dec_kw())

    def deliver(self, state=False):
        s, n = self.s, self.n
        b, o, l, _, _ = s.big
        self.qf.deliver_frames_sel(s.sel, s.n_sel, b, o, l, s.rec, s.ri, s.nrec, s.st, self.slot, self.out, self.out_len,
                                   self.out_state, self.n_out, self.status, s.K, s.em, s.L, n_max=n, G_src=self.G,
                                   max_rows=s.cap, src_gen_stride=s.gs, rec_row_stride=s.rs, rec_gen_stride=s.em * s.rs,
                                   out_row_stride=s.rs, out_gen_stride=s.K * s.rs, n_known=self.n_known,
                                   ids=self.ids if state else None, delivered=self.state if state else None, ctx=self.ctx)

    def check(self):
        """The outputs against the decode's outputs and the store (every entry, on the device), against the
        model (a sample), and the state's effect.  -> stored, recovered sources per listed generation."""
        import torch

        from tests import deliver_ref as R

        s, n, G = self.s, self.n, self.G
        K, rs, em, L, cap = s.K, s.rs, s.em, s.L, s.cap
        s.select(n)
        self.decode()
        self.deliver()
        self.ctx.sync()
        sel = s.sel[:n].long()
        assert (s.st.view(torch.int32)[:n] == 0).all() and (self.status.view(torch.int32) == 0).all()
        assert (self.n_out.view(torch.int32) == K).all() and (self.n_known.view(torch.int32) == K).all()
        slot = self.slot.view(torch.int16)[: n * K].view(n, K).long() & 0xFFFF
        nrec = s.nrec.view(torch.int32)[:n].long()
        ri = s.ri.view(torch.int16)[: n * em].view(n, em).long() & 0xFFFF
        stored = slot != 0xFFFF
        assert ((~stored).sum(1) == nrec).all()
        pos = torch.zeros(n, K, dtype=torch.long, device=s.dev)
        rows = torch.arange(n, device=s.dev)
        for m in range(em):
            ok = nrec > m
            pos[rows[ok], ri[ok, m]] = m
        want_state = torch.where(stored, 1, 2).to(torch.uint8)
        assert torch.equal(self.out_state.view(n, K), want_state)
        assert (self.out_len.view(torch.int32) == L).all()
        store = s.big[0].view(G, cap, rs)
        rec = s.rec[: n * em * rs].view(n, em, rs)
        out = self.out.view(n, K, rs)
        step = max(1, (1 << 28) // (K * rs))           # entries per piece: the expected rows of a piece fit 256 MiB
        for j0 in range(0, n, step):
            j1 = min(n, j0 + step)
            a = store[sel[j0:j1, None], slot[j0:j1].clamp(max=cap - 1)]
            b = rec[rows[j0:j1, None], pos[j0:j1]]
            b[:, :, L:] = 0
            want = torch.where(stored[j0:j1, :, None], a, b)
            assert torch.equal(out[j0:j1], want), "a delivered packet differs from its stored or recovered row"
        # a sample of entries against the model, as a dense call over copies of their generations
        sample = sorted({0, 1, n // 3, n // 2, n - 2, n - 1} & set(range(n)))
        sh = R.Shape(K, em, L, cap, s.gs, rs, em * rs, rs, K * rs)
        h = lambda t, dt: t.cpu().numpy().view(dt)   # noqa: E731
        gens = [int(sel[j]) for j in sample]
        dec = dict(rec=np.concatenate([h(rec[j], np.uint8).reshape(-1) for j in sample]),
                   rec_index=np.stack([h(s.ri[2 * j * em: 2 * (j + 1) * em], np.uint16) for j in sample]),
                   n_rec=np.array([int(nrec[j]) for j in sample], np.uint32), dec_status=np.zeros(len(sample), np.int32),
                   src_slot=np.stack([h(self.slot[2 * j * K: 2 * (j + 1) * K], np.uint16) for j in sample]))
        src = np.concatenate([h(store[g], np.uint8).reshape(-1) for g in gens])
        off = np.stack([h(s.big[1][g], np.uint32) for g in gens])
        ln = np.stack([h(s.big[2][g], np.uint32) for g in gens])
        want = R.deliver(sh, len(sample), src, off, ln, dec["rec"], dec["rec_index"], dec["n_rec"], dec["dec_status"],
                         dec["src_slot"])
        for t, j in enumerate(sample):
            assert np.array_equal(h(out[j], np.uint8).reshape(-1), want["out"][t * sh.out_gs: (t + 1) * sh.out_gs]), j
            assert np.array_equal(h(self.out_len[4 * j * K: 4 * (j + 1) * K], np.uint32), want["out_len"][t * K: (t + 1) * K])
        # with a state: the first call delivers everything, the second nothing and leaves the output alone
        self.state.zero_()
        self.deliver(state=True)
        self.ctx.sync()
        assert (self.n_out.view(torch.int32) == K).all()
        self.out.fill_(0xCC)
        self.deliver(state=True)
        self.ctx.sync()
        assert (self.n_out.view(torch.int32) == 0).all() and (self.out == 0xCC).all() and (self.out_state == 3).all()
        self.deliver()
        self.ctx.sync()
        return int(stored[0].sum()), int(nrec[0])


def host_step(d):
    """What a host does today to find the packets: the five small arrays down, then per source the address
    and the length (vectorised numpy; the rec row of a recovered source through an inverse of rec_index)."""
    s, n = d.s, d.n
    K, em = s.K, s.em
    t0 = time.perf_counter()
    sel = s.sel[:n].cpu().numpy().view(np.uint32).astype(np.int64)
    slot = d.slot.cpu().numpy().view(np.uint16).reshape(n, K).astype(np.int64)
    ri = s.ri[: 2 * n * em].cpu().numpy().view(np.uint16).reshape(n, em).astype(np.int64)
    nrec = s.nrec[: 4 * n].cpu().numpy().view(np.uint32).astype(np.int64)
    st = s.st[: 4 * n].cpu().numpy().view(np.int32)
    t1 = time.perf_counter()
    off = d.row_off_host
    ln = d.row_len_host
    stored = slot != 0xFFFF
    pos = np.zeros((n, K), np.int64)
    valid = np.arange(em)[None, :] < nrec[:, None]
    jj, mm = np.nonzero(valid)
    pos[jj, ri[jj, mm]] = mm
    c = np.where(stored, slot, 0)
    at = np.where(stored, sel[:, None] * s.gs + off[sel[:, None], c], np.arange(n)[:, None] * (em * s.rs) + pos * s.rs)
    length = np.where(stored, ln[sel[:, None], c], s.L)
    ok = st == 0
    t2 = time.perf_counter()
    assert ok.all() and at.shape == length.shape
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3


def run(qf, ctx, hip, G, n, reps):
    import torch

    d = Deliver(qf, ctx, G, n)
    s = d.s
    n_stored, n_recovered = d.check()
    # (the store's offsets and lengths are host knowledge in a caller's loop: not part of the timed downloads)
    d.row_off_host = s.big[1].cpu().numpy().view(np.uint32).reshape(G, s.cap).astype(np.int64)
    d.row_len_host = s.big[2].cpu().numpy().view(np.uint32).reshape(G, s.cap).astype(np.int64)
    stream = torch.cuda.current_stream().cuda_stream
    nbytes = n * s.K * s.L
    a, b = torch.zeros(nbytes, dtype=torch.uint8, device=s.dev), torch.zeros(nbytes, dtype=torch.uint8, device=s.dev)

    def copy():
        e = hip.hipMemcpyAsync(ctypes.c_void_p(b.data_ptr()), ctypes.c_void_p(a.data_ptr()), ctypes.c_size_t(nbytes), 3,
                               ctypes.c_void_p(stream))
        assert e == 0, f"hipMemcpyAsync: {e}"

    steps = {"copy_same_bytes": copy, "deliver": d.deliver, "select_plus_listed_decode": lambda: (s.select(n), d.decode())}
    t = {name: [] for name in steps}
    ks, host = {}, []
    for _ in range(reps):
        for name, fn in steps.items():
            t[name].append(round(B.timed(fn, ctx), 5))
        for kn, ms in B.kernel_split(d.deliver, ctx).items():
            ks.setdefault(kn, []).append(ms)
        ctx.sync()
        host.append(host_step(d))
    m = {name: med(v) for name, v in t.items()}
    kms = {kn: med(v) for kn, v in ks.items()}
    cp = t["copy_same_bytes"]
    spread = (max(cp) - min(cp)) / med(cp)
    rec_share = 16 / (2 * s.L)
    rows = kms["k_deliver_rows_sel"]
    bound = 1 + rec_share + spread
    out = {
        "shape": {"k": s.K, "L": s.L, "G": G, "cap": s.cap, "listed": n, "n_max": n, "stored_per_generation": n_stored,
                  "recovered_per_generation": n_recovered, "bytes_copied": nbytes, "record_bytes": 16 * n * s.K},
        "outputs_checked": "every entry against the decode's outputs and the store; a sample against tests/deliver_ref.py; "
                           "a second call with a state delivers nothing and writes no output byte",
        "ms": t, "ms_median": m, "ms_min_max": {name: B.spread(v) for name, v in t.items()},
        "kernels_ms": kms, "kernels_ms_min_max": {kn: B.spread(v) for kn, v in ks.items()},
        "a_rows_against_copy": {
            "k_deliver_rows_sel_ms": rows, "copy_ms": med(cp), "copy_relative_spread": round(spread, 5),
            "ratio": round(rows / med(cp), 4), "GBps_read_plus_written": round(2 * nbytes / rows / 1e6, 1),
            "expectation": "ratio <= 1 + record bytes / bytes moved + the copy's relative min-max spread",
            "expected_ratio_at_most": round(bound, 4), "expectation_met": bool(rows / med(cp) <= bound)},
        "b_call_against_decode": {
            "deliver_ms": m["deliver"], "k_deliver_prepare_sel_ms": kms["k_deliver_prepare_sel"],
            "select_plus_listed_decode_ms": m["select_plus_listed_decode"],
            "ratio": round(m["deliver"] / m["select_plus_listed_decode"], 4)},
        "c_host_step_replaced": {
            "downloads_ms": med([x for x, _ in host]), "address_loop_ms": med([y for _, y in host]),
            "host_ms": med([x + y for x, y in host]), "host_ms_min_max": B.spread([round(x + y, 4) for x, y in host]),
            "deliver_ms": m["deliver"], "note": "host wall time, vectorised numpy, no payload copies; the deliver call's "
                                                 "time includes the payload copy into the output"},
    }
    del d, s, a, b
    torch.cuda.empty_cache()
    return out


def main():
    import torch

    from quicfuscate_amd import fec as qf

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--generations", type=int, default=65536)
    ap.add_argument("--fractions", default="64,16,4", help="n = G / each")
    ap.add_argument("--out", default="profiles/deliver_bench.json")
    a = ap.parse_args()
    assert torch.cuda.is_available()
    ctx = qf.default_context()
    hip = S._hip()
    prop = torch.cuda.get_device_properties(0)
    res = {"tool": "tools/bench_deliver.py", "device": torch.cuda.get_device_name(0),
           "arch": getattr(prop, "gcnArchName", ""), "compute_units": prop.multi_processor_count,
           "timing": f"device events, windows of >= 0.5 s after a warm-up, {a.reps} repetitions, steps alternated in one "
                     "process; per-kernel times from qf_ctx_profile; medians with min-max; the host step by wall clock",
           "runs": {}}
    G = a.generations
    for f in (int(x) for x in a.fractions.split(",")):
        key = f"n_G_over_{f}"
        res["runs"][key] = r = run(qf, ctx, hip, G, G // f, a.reps)
        ra, rb, rc = r["a_rows_against_copy"], r["b_call_against_decode"], r["c_host_step_replaced"]
        print(f"{key}: rows {ra['k_deliver_rows_sel_ms']:.4f} ms, {ra['ratio']} of the copy (bound {ra['expected_ratio_at_most']}, "
              f"{'met' if ra['expectation_met'] else 'not met'}); call {rb['deliver_ms']:.4f} ms, {rb['ratio']} of select + "
              f"decode; host step {rc['host_ms']:.3f} ms", file=sys.stderr, flush=True)
    Path(a.out).parent.mkdir(exist_ok=True, parents=True)
    Path(a.out).write_text(json.dumps(res, indent=1))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
