#!/usr/bin/env python3
"""Timing of the streaming receive step: generations that fill
over T polls through qf_rank_update_batch and qf_store_append_dev, against the
one-shot kernels over the same rows.

    python tools/bench_stream_recv.py --out profiles/stream_recv_bench.json

Workload: k = 64, L = 1,200, G = 65,536, frame_stride 1,280, shapes (a) and (b)
of tools/bench_recv_inplace.py (64 patterns tiled); each generation's rows are
dealt over T = 4 and T = 8 polls in arrival order, ceil(rows / T) slots per
poll.  Every poll is parsed once up front (qf_parse_frame_headers_dev); a
streamed pass zeroes the states and the store counts and runs update + append
for every poll.
  yardstick  qf_rank_batch over the whole sequence (k_rank_filter), and for the
             payload a device-to-device hipMemcpyAsync of the bytes the appends
             of a pass move, poll by poll
It records the sum over the polls of k_rank_update against k_rank_filter, the
update call when no generation has a row (the idle cost), k_store_rows against
the copy, the state bytes a poll loads and stores, and the two expectations of
DESIGN 3.14 with "met" or "not met".  Before it times anything it asserts that
the streamed flags and ranks are the one-shot call's, and that
qf_decode_frames_dev over the store gives the rec, rec_index, n_rec and status
of qf_decode_frames_dev over all frames.
Times: device events over windows of >= 0.5 s after a warm-up, medians with
min-max over the repetitions, steps alternated in one process; per-kernel times
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
sys.path.insert(0, str(REPO / "tools"))

import bench_recv_inplace as B  # noqa: E402

SHAPES = ("a_51sys_26coded_r16", "b_80coded_r64")


def _hip():
    """The HIP runtime the process already holds (torch's)."""
    import torch

    return ctypes.CDLL(str(Path(torch.__file__).parent / "lib" / "libamdhip64.so"))


class Stream:
    """One shape dealt over T polls: the parsed polls, the states, the store."""

    def __init__(self, qf, ctx, name, T, G_override=0):
        import torch

        K, n_sys, n_front, n_behind, planted, r, L, G, pool = B.SHAPES[name]
        if G_override:
            G = max(pool, G_override // pool * pool)
        self.qf, self.ctx, self.K, self.L, self.G, self.T, self.r = qf, ctx, K, L, G, T, r
        rng = np.random.default_rng(2029)
        self.pats = B.patterns(qf, rng, K, n_sys, n_front, n_behind, planted, pool)
        self.mr = mr = len(self.pats[0][0])
        P = qf.frame_payload_offset(K)
        self.fs = fs = (P + L + 15) // 16 * 16
        self.rs = rs = (L + 15) // 16 * 16
        self.dev = dev = f"cuda:{ctx.device}"
        tile = G // pool
        z = lambda n: torch.zeros(n, dtype=torch.uint8, device=dev)   # noqa: E731
        self.z = z

        def up(x):
            return torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).to(dev).repeat(tile)

        fr, ln, off, ids = B.frame_pool(qf, rng, K, L, fs, self.pats)
        self.t_fr = up(fr)
        t_ln, t_off, t_ids = up(ln), up(off), up(ids)
        # the whole sequence, parsed: the one-shot calls' inputs
        self.f = self._parse(self.t_fr, t_ln, t_off, t_ids, mr)
        self.f_fl, self.f_rk, self.f_st = z(G * mr), z(4 * G), z(4 * G)
        # the polls
        self.cut = [mr * t // T for t in range(T + 1)]
        self.mp = mp = max(b - a for a, b in zip(self.cut, self.cut[1:]))
        self.polls = []
        for a, b in zip(self.cut, self.cut[1:]):
            c = b - a

            def part(t, width):
                out = z(G * mp * width).view(G, mp, width)
                out[:, :c] = t.view(G, mr, width)[:, a:b]
                return out.view(-1)

            frames = part(self.t_fr, fs)
            p = self._parse(frames, part(t_ln, 4), part(t_off, 4), part(t_ids, 8), mp,
                            n_frames=torch.full((G,), c, dtype=torch.int32, device=dev))
            p["frames"], p["c"], p["fl"] = frames, c, z(G * mp)
            self.polls.append(p)
        del t_ln, t_off, t_ids
        self.sb = qf.rank_state_bytes(K)
        self.state = z(G * self.sb)
        self.u_rk, self.u_st, self.a_st = z(4 * G), z(4 * G), z(4 * G)
        self.n_zero = torch.zeros(G, dtype=torch.int32, device=dev)
        self.idle_fl = z(G * mp)
        self.store, self.s_off, self.s_len = z(G * K * rs), z(4 * G * K), z(4 * G * K)
        self.s_idx, self.s_co = z(2 * G * K), z(G * K * K)
        self.s_n = torch.zeros(G, dtype=torch.int32, device=dev)
        # rows each poll appends (the innovative ones), and the state bytes each poll moves
        flags = np.stack([p[2] for p in self.pats]).astype(np.int64)          # (pool, mr)
        idx = np.stack([p[0] for p in self.pats]).astype(np.int64)
        self.taken, self.state_loaded, self.state_stored = [], [], []
        nu = np.zeros(pool, np.int64)
        nb = np.zeros(pool, np.int64)

        def body(nb_):                                                        # U map + piv dwords + B dwords
            g4 = (nb_ + 3) // 4
            return 32 + 4 * g4 + 4 * g4 * K

        for a, b in zip(self.cut, self.cut[1:]):
            f = flags[:, a:b]
            sysr = idx[:, a:b] < K
            self.taken.append(int(f.sum()) * tile)
            held = nu + nb
            loaded = 16 + np.where((held > 0) & (held < K), body(nb), 0)
            # (a systematic row that lands on a pivot moves a row from B's pivot to U: counted as nu here)
            nu2, nb2 = nu + (f * sysr).sum(1), nb + (f * ~sysr).sum(1)
            stored = np.where(nu2 + nb2 != held, 16 + body(nb2), 0)
            self.state_loaded.append(int(loaded.sum()) * tile)
            self.state_stored.append(int(stored.sum()) * tile)
            nu, nb = nu2, nb2

    def _parse(self, frames, flen, foff, ids, mr, n_frames=None):
        G, K, z = self.G, self.K, self.z
        p = dict(idx=z(2 * G * mr), n=z(4 * G), fst=z(4 * G * mr), co=z(G * mr * K), rl=z(4 * G * mr), ro=z(4 * G * mr))
        self.qf.parse_frame_headers(frames, flen, ids, p["idx"], p["n"], p["fst"], p["co"], p["rl"], p["ro"], K, self.L,
                                    max_rows=mr, frame_stride=self.fs, G=G, n_frames=n_frames, frame_off=foff,
                                    ctx=self.ctx)
        self.ctx.sync()
        return p

    # the yardstick
    def one_shot(self):
        f = self.f
        self.qf.rank_batch(f["idx"], self.f_rk, self.f_st, self.K, max_rows=self.mr, G=self.G, n_rows=f["n"],
                           row_coeffs=f["co"], innovative=self.f_fl, ctx=self.ctx)

    # the streamed step
    def reset(self):
        self.state.zero_()
        self.s_n.zero_()

    def update(self, p, idle=False):
        self.qf.rank_update_batch(p["idx"], self.state, self.u_rk, self.u_st, self.K, max_rows=self.mp, G=self.G,
                                  n_rows=self.n_zero if idle else p["n"], row_coeffs=p["co"],
                                  innovative=self.idle_fl if idle else p["fl"], ctx=self.ctx)

    def append(self, p):
        K, rs = self.K, self.rs
        self.qf.store_append(p["frames"], p["ro"], p["rl"], p["idx"], p["co"], self.store, self.s_off, self.s_len,
                             self.s_idx, self.s_co, self.s_n, self.a_st, K, self.L, max_rows=self.mp, cap=K,
                             src_gen_stride=self.mp * self.fs, store_row_stride=rs, store_gen_stride=K * rs, G=self.G,
                             n_rows=p["n"], take=p["fl"], ctx=self.ctx)

    def appends(self):
        self.s_n.zero_()
        for p in self.polls:
            self.append(p)

    def stream_pass(self):
        self.reset()
        for p in self.polls:
            self.update(p)
            self.append(p)

    def idle_update(self):
        self.update(self.polls[0], idle=True)

    def copies(self, hip, stream):
        """The bytes the appends of one pass move, poll by poll, as plain copies."""
        at = 0
        for p, taken in zip(self.polls, self.taken):
            nbytes = taken * self.rs
            e = hip.hipMemcpyAsync(ctypes.c_void_p(self.store.data_ptr() + at), ctypes.c_void_p(p["frames"].data_ptr()),
                                   ctypes.c_size_t(nbytes), 3, ctypes.c_void_p(stream))
            assert e == 0, f"hipMemcpyAsync: {e}"
            at += nbytes

    def check(self):
        """Streamed flags and ranks = the one-shot call's; decode over the store =
        decode over all frames."""
        import torch

        G, K, mr, mp, L, rs, r = self.G, self.K, self.mr, self.mp, self.L, self.rs, self.r
        self.one_shot()
        self.stream_pass()
        self.ctx.sync()
        assert (self.f_st.view(torch.int32) == 0).all() and (self.u_st.view(torch.int32) == 0).all()
        assert (self.a_st.view(torch.int32) == 0).all()
        got = torch.cat([p["fl"].view(G, mp)[:, : p["c"]] for p in self.polls], dim=1)
        assert torch.equal(got, self.f_fl.view(G, mr)), "streamed flags differ from qf_rank_batch's"
        assert torch.equal(self.u_rk, self.f_rk) and (self.f_rk.view(torch.int32) == K).all(), "ranks differ"
        assert (self.s_n == K).all()
        em = min(K, r)
        z = self.z
        outs = []
        for src, ro, rl, idx, co, n, rows, sgs in (
                (self.t_fr, self.f["ro"], self.f["rl"], self.f["idx"], self.f["co"], self.f["n"], mr, mr * self.fs),
                (self.store, self.s_off, self.s_len, self.s_idx, self.s_co, self.s_n, K, K * rs)):
            rec, ri, nrec, st = z(G * em * rs), z(2 * G * em), z(4 * G), z(4 * G)
            self.qf.decode_frames(src, ro, rl, idx, co, rec, ri, nrec, st, K, r, L, max_rows=rows, src_gen_stride=sgs,
                                  rec_row_stride=rs, rec_gen_stride=em * rs, G=G, n_rows=n, ctx=self.ctx)
            self.ctx.sync()
            assert (st.view(torch.int32) == 0).all()
            outs.append((rec, ri, nrec, st))
        for a, b, what in zip(outs[0], outs[1], ("rec", "rec_index", "n_rec", "status")):
            assert torch.equal(a, b), f"{what} of the decode over the store differs"
        del outs
        torch.cuda.empty_cache()


def run(qf, ctx, hip, name, T, reps, G_override=0):
    import torch

    st = Stream(qf, ctx, name, T, G_override)
    st.check()
    stream = torch.cuda.current_stream().cuda_stream
    copy_pass = lambda: st.copies(hip, stream)   # noqa: E731
    med = statistics.median
    t = {n: [] for n in ("one_shot_call", "idle_update_call", "appends_calls", "copies", "stream_pass", "reset")}
    ks = {n: [] for n in ("k_rank_filter", "k_rank_update", "k_rank_update_idle", "k_store_prepare", "k_store_rows")}
    for _ in range(reps):
        t["one_shot_call"].append(round(B.timed(st.one_shot, ctx), 4))
        ks["k_rank_filter"].append(B.kernel_split(st.one_shot, ctx)["k_rank_filter"])
        # (updates on full states cost less than on filling ones: the kernel time
        # of filling states comes from the profiled passes below)
        t["stream_pass"].append(round(B.timed(st.stream_pass, ctx), 4))
        t["reset"].append(round(B.timed(st.reset, ctx), 4))
        k = B.kernel_split(st.stream_pass, ctx)
        for n in ("k_rank_update", "k_store_prepare", "k_store_rows"):
            ks[n].append(round(k[n], 5))
        st.stream_pass()
        t["idle_update_call"].append(round(B.timed(st.idle_update, ctx), 4))
        ks["k_rank_update_idle"].append(B.kernel_split(st.idle_update, ctx)["k_rank_update"])
        t["appends_calls"].append(round(B.timed(st.appends, ctx), 4))
        t["copies"].append(round(B.timed(copy_pass, ctx), 4))
    moved = sum(st.taken) * st.rs                       # payload bytes an append pass reads, and writes
    desc = sum(st.taken) * 8 + st.G * T * 8             # the records k_store_rows reads beside them
    copy_rate = moved / (med(t["copies"]) * 1e-3)       # bytes per second (read + write of `moved` each)
    state_bytes = sum(st.state_loaded) + sum(st.state_stored)
    spread_f = (max(ks["k_rank_filter"]) - min(ks["k_rank_filter"])) / med(ks["k_rank_filter"])
    # the state goes one way per byte, the copy moves each byte both ways: the copy's
    # rate in bytes of traffic per second is 2 * moved / time
    upd_bound = med(ks["k_rank_filter"]) * (1 + spread_f) + state_bytes / (2 * copy_rate) * 1e3
    spread_c = (max(t["copies"]) - min(t["copies"])) / med(t["copies"])
    app_bound = 1 + desc / (2 * moved) + spread_c
    app_ratio = med(ks["k_store_rows"]) / med(t["copies"])
    return {
        "shape": {"k": st.K, "L": st.L, "G": st.G, "rows": st.mr, "polls": T, "slots_per_poll": st.mp,
                  "frame_stride": st.fs, "state_bytes_per_generation": st.sb, "store_row_stride": st.rs, "cap": st.K},
        "outputs_checked": "streamed flags and ranks equal qf_rank_batch's; qf_decode_frames_dev over the store gives "
                           "the rec, rec_index, n_rec and status of the same call over all frames",
        "ms": t,
        "ms_median": {n: med(v) for n, v in t.items()},
        "ms_min_max": {n: B.spread(v) for n, v in t.items()},
        "kernels_ms_per_pass": ks,
        "kernels_ms_per_pass_median": {n: med(v) for n, v in ks.items()},
        "kernels_ms_per_pass_min_max": {n: B.spread(v) for n, v in ks.items()},
        "update": {
            "sum_over_polls_ms": med(ks["k_rank_update"]), "one_shot_ms": med(ks["k_rank_filter"]),
            "ratio": round(med(ks["k_rank_update"]) / med(ks["k_rank_filter"]), 4),
            "idle_poll_kernel_ms": med(ks["k_rank_update_idle"]), "idle_poll_call_ms": med(t["idle_update_call"]),
            "state_bytes_loaded_per_poll": st.state_loaded, "state_bytes_stored_per_poll": st.state_stored,
            "state_bytes_over_the_polls": state_bytes,
            "copy_traffic_bytes_per_s": round(2 * copy_rate), "one_shot_relative_spread": round(spread_f, 5),
            "expectation": "sum of k_rank_update over the polls <= k_rank_filter * (1 + its relative min-max spread) + "
                           "state bytes loaded and stored / the copy's traffic rate",
            "expected_ms_at_most": round(upd_bound, 4),
            "expectation_met": bool(med(ks["k_rank_update"]) <= upd_bound),
        },
        "append": {
            "rows_appended_per_poll": st.taken, "payload_bytes_moved": moved, "descriptor_bytes_read": desc,
            "k_store_rows_ms": med(ks["k_store_rows"]), "k_store_prepare_ms": med(ks["k_store_prepare"]),
            "copy_ms": med(t["copies"]),
            "k_store_rows_GBps_read_plus_write": round(2 * moved / (med(ks["k_store_rows"]) * 1e-3) / 1e9, 1),
            "copy_GBps_read_plus_write": round(2 * copy_rate / 1e9, 1),
            "ratio_k_store_rows_to_copy": round(app_ratio, 4), "copy_relative_spread": round(spread_c, 5),
            "expectation": "k_store_rows : copy <= 1 + descriptor bytes / bytes moved + the copy's relative min-max spread",
            "expected_ratio_at_most": round(app_bound, 4),
            "expectation_met": bool(app_ratio <= app_bound),
        },
    }


def main():
    import torch

    from quicfuscate_amd import fec as qf

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--polls", default="4,8")
    ap.add_argument("--generations", type=int, default=0, help="override G (a smoke run)")
    ap.add_argument("--out", default="profiles/stream_recv_bench.json")
    a = ap.parse_args()
    assert torch.cuda.is_available()
    ctx = qf.default_context()
    hip = _hip()
    prop = torch.cuda.get_device_properties(0)
    res = {"tool": "tools/bench_stream_recv.py", "device": torch.cuda.get_device_name(0),
           "arch": getattr(prop, "gcnArchName", ""), "compute_units": prop.multi_processor_count,
           "timing": f"device events, windows of >= 0.5 s after a warm-up, {a.reps} repetitions, steps alternated in "
                     "one process; per-kernel times from qf_ctx_profile, per streamed pass (all polls); medians "
                     "with min-max",
           "streamed_step": "per poll qf_rank_update_batch then qf_store_append_dev (take = the update's flags) on "
                            "polls parsed up front by qf_parse_frame_headers_dev",
           "yardstick": "qf_rank_batch over the whole sequence; hipMemcpyAsync device to device of the bytes the "
                        "appends move, poll by poll",
           "runs": {}}
    for name in a.shapes.split(","):
        for T in (int(x) for x in a.polls.split(",")):
            key = f"{name}_T{T}"
            res["runs"][key] = run(qf, ctx, hip, name, T, a.reps, a.generations)
            u, p = res["runs"][key]["update"], res["runs"][key]["append"]
            print(f"{key}: update {u['ratio']} of one-shot ({'met' if u['expectation_met'] else 'not met'}), "
                  f"append {p['ratio_k_store_rows_to_copy']} of the copy ({'met' if p['expectation_met'] else 'not met'})",
                  file=sys.stderr, flush=True)
            torch.cuda.empty_cache()
    Path(a.out).parent.mkdir(exist_ok=True, parents=True)
    Path(a.out).write_text(json.dumps(res, indent=1))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
