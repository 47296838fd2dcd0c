"""The feedback packets on the MI355X: qf_frame_reports_dev,
qf_parse_report_frames_dev and qf_report_closed_dev against tests/fbwire_ref.py
over the case tables, their call-level errors, and the loop with both
directions as bytes: source -> relay -> receiver with real calls throughout,
the receiver's reports, re-reports and packets and the relay's parse and credit
update on the device, the test playing both networks.

Every output buffer starts as 0xCC with guard bytes behind it and is compared
whole with the model's, so the bytes a call must not write are checked too.
Every case runs twice and every byte of the two runs is equal."""
import ctypes

import numpy as np
import pytest

from tests import credit_ref as C
from tests import emit_ref as R
from tests import fbwire_ref as F
from tests.test_gpu_emit import Dev, DevNode, _body, _dev, _guarded, _h, call, same

pytestmark = pytest.mark.gpu

OK, EINVAL = F.OK, F.EINVAL
GUARD = 64


def _one(v):
    return None if v is None else _dev(np.array([v], np.uint32))


def _outs(before, nulls=()):
    return {key: _guarded(before[key]) for key in before if key not in nulls}


def _download(t, before):
    return {key: _body(t[key], before[key]) if key in t else before[key].copy() for key in before}


def _unchanged(pairs):
    for t, a in pairs:
        if t is not None:
            assert np.array_equal(_h(t), np.ascontiguousarray(a).view(np.uint8).reshape(-1)), "an input was written"


def _twice(run, before, want, what):
    """run(t) twice from the same buffers: equal to each other and to the model."""
    got = []
    for _ in range(2):
        t = _outs(before, what[1])
        run(t)
        got.append(_download(t, before))
    same(got[0], want, what[0])
    for key in want:
        assert np.array_equal(got[0][key].view(np.uint8), got[1][key].view(np.uint8)), f"{key}: two runs differ"
    return want


def pack_call(qf, c, d, t):
    qf.frame_reports(d["reports"], d["n_reports"], t["pkts"], t["pkt_len"], t["n_pkts"], c.k, N_max=c.N_max,
                     max_len=c.max_len, F_max=c.F_max, stride=c.stride, n_left=t.get("n_left"),
                     n_skipped=t.get("n_skipped"))
    qf.default_context().sync()


def pack_against_model(qf, c, before=None):
    before = before or c.blank()
    d = dict(reports=_dev(c.reports), n_reports=_one(c.n_reports))
    want = _twice(lambda t: pack_call(qf, c, d, t), before, c.model(before), ("frame_reports", c.nulls))
    _unchanged([(d["reports"], c.reports)])
    return want


def parse_call(qf, c, d, t):
    qf.parse_report_frames(d["pkts"], d["pkt_len"], d["n_pkts"], t["reports"], t["n_reports"], c.k, N_max=c.N_max,
                           max_len=c.max_len, F_max=c.F_max, stride=c.stride, n_left=t.get("n_left"),
                           pkt_status=t.get("pkt_status"), pkt_first=t.get("pkt_first"), pkt_count=t.get("pkt_count"),
                           append=c.append)
    qf.default_context().sync()


def parse_against_model(qf, c, before=None):
    before = before or c.blank()
    d = dict(pkts=_dev(c.pkts), pkt_len=_dev(c.pkt_len), n_pkts=_one(c.n_pkts))
    want = _twice(lambda t: parse_call(qf, c, d, t), before, c.model(before), ("parse_report_frames", c.nulls))
    _unchanged([(d["pkts"], c.pkts), (d["pkt_len"], c.pkt_len)])
    return want


def closed_call(qf, c, d, t):
    qf.report_closed(d["frame_id"], d["frame_status"], d["n_frames"], d["win"], t["reports"], t["n_reports"], c.k,
                     G_src=c.G_src, F_max=c.F_max, N_max=c.N_max, n_left=t.get("n_left"), append=c.append)
    qf.default_context().sync()


def closed_against_model(qf, c, before=None):
    before = before or c.blank()
    d = dict(frame_id=_dev(c.frame_id), frame_status=_dev(c.frame_status), n_frames=_one(c.n_frames), win=_dev(c.win))
    want = _twice(lambda t: closed_call(qf, c, d, t), before, c.model(before), ("report_closed", c.nulls))
    _unchanged([(d["frame_id"], c.frame_id), (d["frame_status"], c.frame_status), (d["win"], c.win)])
    return want


# ---------------------------------------------------------------------------
# 1: the case tables
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(F.pack_cases()))
def test_pack_cases_against_the_model(qf, gpu_ctx, name):
    c = F.pack_cases()[name]
    want = pack_against_model(qf, c)
    if name == "S_full_plus_1":
        assert (want["n_pkts"][0], want["n_left"][0]) == (2, 1)
    if name == "non_sendable_between":
        assert (want["n_pkts"][0], want["n_skipped"][0]) == (2, 3)
    if name == "max_len65535":
        assert want["pkt_len"].tolist() == [65533, 13]
    if name == "id_bytes_differ":
        assert want["pkts"][3:13].tobytes() == bytes.fromhex("0123456789ABCDEF0003")
    if name == "k256_rank256":
        assert want["pkts"][11:13].tobytes() == b"\x01\x00" and want["n_skipped"][0] == 1


@pytest.mark.parametrize("name", sorted(F.parse_cases()))
def test_parse_cases_against_the_model(qf, gpu_ctx, name):
    c, before = F.parse_cases()[name]
    want = parse_against_model(qf, c, before)
    if name == "lengths":
        assert want["pkt_status"].tolist() == [EINVAL] * 9 + [OK]
    if name == "append_crosses_N_max":
        assert (want["n_reports"][0], want["n_left"][0]) == (12, 4)
    if name == "one_packet_6553":
        assert want["n_reports"][0] == 6553


def test_parsed_values_are_judged_by_the_credit_update(qf, gpu_ctx):
    c, before = F.parse_cases()["values_pass"]
    d = dict(pkts=_dev(c.pkts), pkt_len=_dev(c.pkt_len), n_pkts=_one(c.n_pkts))
    t = _outs(before)
    parse_call(qf, c, d, t)
    same(_download(t, before), c.model(before), "parse_report_frames")
    G, k = 3, c.k
    win, zero = np.zeros(G, np.uint64), np.zeros(G, np.uint32)
    cc = C.CreditCall(k, 1, 1, 16, win, zero, zero, _body(t["reports"], before["reports"]), 5, c.N_max)
    cb = cc.blank()
    ct = _outs(cb)
    qf.credit_update(_dev(win), _dev(zero), _dev(zero), ct["state"], ct["credit"], k, G=G, num=1, den=1, cap=16,
                     N_max=c.N_max, reports=t["reports"], n_reports=t["n_reports"], report_status=ct["status"])
    gpu_ctx.sync()
    got = _download(ct, cb)
    same(got, cc.model(cb), "credit_update over the parsed records")
    assert got["status"][:5].tolist() == [EINVAL, EINVAL, EINVAL, EINVAL, C.ENOTREADY]


@pytest.mark.parametrize("name", sorted(F.closed_cases()))
def test_closed_cases_against_the_model(qf, gpu_ctx, name):
    c, before = F.closed_cases()[name]
    want = closed_against_model(qf, c, before)
    if name == "five_frames_one_generation":
        assert want["n_reports"][0] == 1
    if name == "window_contradicts":
        assert want["n_reports"][0] == 1 and want["reports"]["id"][0] == c.frame_id[4]
    if name == "append_overflow":
        assert (want["n_reports"][0], want["n_left"][0]) == (8, 1)


# ---------------------------------------------------------------------------
# 2: the call-level errors write nothing
# ---------------------------------------------------------------------------
def _shifted(t, off):
    import torch

    return torch.zeros(t.numel() + off, dtype=torch.uint8, device="cuda")[off:]


def _refused(qf, fn):
    with pytest.raises(qf.QfError) as e:
        fn()
    assert e.value.status == EINVAL
    qf.default_context().sync()


def _p(t):
    return None if t is None else t.data_ptr()


SHAPE = dict(k=4, max_len=33, F_max=3, stride=48, N_max=12)
BAD_SHAPES = [dict(k=0), dict(k=257), dict(max_len=12), dict(max_len=65536), dict(F_max=0), dict(N_max=0),
              dict(stride=40), dict(stride=32), dict(max_len=49)]


def test_frame_reports_refuses_and_writes_nothing(qf, gpu_ctx):
    from quicfuscate_amd import _lib as L

    c = F.PackCall(4, 33, 3, 48, F.pack_cases()["n_reports_null"].reports[:8], n_reports=8, N_max=12)
    c.reports = np.concatenate([c.reports, F.poisoned(4, F.REPORT)])
    before = c.blank()
    d = dict(reports=_dev(c.reports), n_reports=_one(8))
    t = _outs(before)
    ptrs = dict(reports=d["reports"], pkts=t["pkts"], pkt_len=t["pkt_len"], n_pkts=t["n_pkts"])

    def go(**kw):
        a = {**SHAPE, **{key: v for key, v in kw.items() if key in SHAPE}}
        p = {**ptrs, **{key: v for key, v in kw.items() if key in ptrs}}
        qf.frame_reports(p["reports"], d["n_reports"], p["pkts"], p["pkt_len"], p["n_pkts"], a["k"], N_max=a["N_max"],
                         max_len=a["max_len"], F_max=a["F_max"], stride=a["stride"], n_left=t["n_left"],
                         n_skipped=t["n_skipped"])

    bad = BAD_SHAPES + [dict(reports=None), dict(pkts=None), dict(pkt_len=None), dict(n_pkts=None),
                        dict(reports=_shifted(d["reports"], 8)), dict(pkts=t["pkts"][8:])]
    for kw in bad:
        _refused(qf, lambda kw=kw: go(**kw))
    lib = L._lib()
    tail = (12, _p(d["reports"]), _p(d["n_reports"]), _p(t["pkts"]), _p(t["pkt_len"]), _p(t["n_pkts"]), None, None)
    for flags in (1, 2):
        sh = L.ReportWireShape(4, 33, 3, flags, 48)
        assert lib.qf_frame_reports_dev(gpu_ctx.handle, ctypes.byref(sh), *tail) == EINVAL
    sh = L.ReportWireShape(4, 33, 3, 0, 48)
    assert lib.qf_frame_reports_dev(gpu_ctx.handle, ctypes.byref(sh), (1 << 24) + 1, *tail[1:]) == EINVAL   # N_max
    assert lib.qf_frame_reports_dev(None, ctypes.byref(sh), *tail) == EINVAL
    assert lib.qf_frame_reports_dev(gpu_ctx.handle, None, *tail) == EINVAL
    gpu_ctx.sync()
    same(_download(t, before), before, "a refused frame_reports")
    go()                                       # ... and the same buffers are good for a call
    gpu_ctx.sync()
    same(_download(t, before), c.model(before), "frame_reports after the refusals")


def test_parse_report_frames_refuses_and_writes_nothing(qf, gpu_ctx):
    from quicfuscate_amd import _lib as L

    c, _ = F.parse_cases()["append_crosses_N_max"]
    before = c.blank(8)
    d = dict(pkts=_dev(c.pkts), pkt_len=_dev(c.pkt_len), n_pkts=_one(c.n_pkts))
    t = _outs(before)
    ptrs = dict(pkts=d["pkts"], pkt_len=d["pkt_len"], reports=t["reports"], n_reports=t["n_reports"])

    def go(**kw):
        a = {**SHAPE, **{key: v for key, v in kw.items() if key in SHAPE}}
        p = {**ptrs, **{key: v for key, v in kw.items() if key in ptrs}}
        qf.parse_report_frames(p["pkts"], p["pkt_len"], d["n_pkts"], p["reports"], p["n_reports"], a["k"],
                               N_max=a["N_max"], max_len=a["max_len"], F_max=a["F_max"], stride=a["stride"],
                               n_left=t["n_left"], pkt_status=t["pkt_status"], pkt_first=t["pkt_first"],
                               pkt_count=t["pkt_count"], append=True)

    bad = BAD_SHAPES + [dict(pkts=None), dict(pkt_len=None), dict(reports=None), dict(n_reports=None),
                        dict(reports=t["reports"][8:]), dict(pkts=_shifted(d["pkts"], 8))]
    for kw in bad:
        _refused(qf, lambda kw=kw: go(**kw))
    lib = L._lib()
    tail = (_p(d["pkts"]), _p(d["pkt_len"]), _p(d["n_pkts"]), 12, _p(t["reports"]), _p(t["n_reports"]), None, None, None,
            None)
    for flags in (2, 3):
        sh = L.ReportWireShape(4, 33, 3, flags, 48)
        assert lib.qf_parse_report_frames_dev(gpu_ctx.handle, ctypes.byref(sh), *tail) == EINVAL
    sh = L.ReportWireShape(4, 33, 3, 1, 48)
    assert lib.qf_parse_report_frames_dev(gpu_ctx.handle, ctypes.byref(sh), *tail[:3], (1 << 24) + 1, *tail[4:]) == EINVAL
    assert lib.qf_parse_report_frames_dev(None, ctypes.byref(sh), *tail) == EINVAL
    assert lib.qf_parse_report_frames_dev(gpu_ctx.handle, None, *tail) == EINVAL
    gpu_ctx.sync()
    same(_download(t, before), before, "a refused parse_report_frames")
    go()
    gpu_ctx.sync()
    same(_download(t, before), c.model(before), "parse_report_frames after the refusals")


def test_report_closed_refuses_and_writes_nothing(qf, gpu_ctx):
    from quicfuscate_amd import _lib as L

    c, _ = F.closed_cases()["append_mid"]
    before = c.blank(3)
    d = dict(frame_id=_dev(c.frame_id), frame_status=_dev(c.frame_status), n_frames=_one(c.n_frames), win=_dev(c.win))
    t = _outs(before)
    base = dict(k=c.k, G_src=c.G_src, F_max=c.F_max, N_max=c.N_max)
    ptrs = dict(frame_id=d["frame_id"], frame_status=d["frame_status"], win=d["win"], reports=t["reports"],
                n_reports=t["n_reports"])

    def go(**kw):
        a = {**base, **{key: v for key, v in kw.items() if key in base}}
        p = {**ptrs, **{key: v for key, v in kw.items() if key in ptrs}}
        qf.report_closed(p["frame_id"], p["frame_status"], d["n_frames"], p["win"], p["reports"], p["n_reports"], a["k"],
                         G_src=a["G_src"], F_max=a["F_max"], N_max=a["N_max"], n_left=t["n_left"], append=True)

    bad = [dict(k=0), dict(k=257), dict(G_src=0), dict(F_max=0), dict(N_max=0),
           dict(frame_id=None), dict(frame_status=None), dict(win=None), dict(reports=None), dict(n_reports=None),
           dict(win=_shifted(d["win"], 4)), dict(reports=t["reports"][8:])]
    for kw in bad:
        _refused(qf, lambda kw=kw: go(**kw))
    lib = L._lib()
    args = lambda flags: (c.k, c.G_src, c.F_max, _p(d["frame_id"]), _p(d["frame_status"]), _p(d["n_frames"]),   # noqa: E731
                          _p(d["win"]), c.N_max, flags, _p(t["reports"]), _p(t["n_reports"]), _p(t["n_left"]))
    assert lib.qf_report_closed_dev(gpu_ctx.handle, *args(2)) == EINVAL            # an unknown flag
    assert lib.qf_report_closed_dev(None, *args(1)) == EINVAL
    assert lib.qf_report_closed_dev(gpu_ctx.handle, c.k, (1 << 24) + 1, *args(1)[2:]) == EINVAL   # G_src
    gpu_ctx.sync()
    same(_download(t, before), before, "a refused report_closed")
    go()
    gpu_ctx.sync()
    same(_download(t, before), c.model(before), "report_closed after the refusals")


# ---------------------------------------------------------------------------
# 3: the loop on the device, both directions as bytes
# ---------------------------------------------------------------------------
class FbNode(DevNode):
    """DevNode whose ingest keeps the window call's per-frame status on the device (its body is DevNode.ingest's)."""

    def ingest(self, t, N, fs):
        qf, T, rc = self.qf, self.T, self.rc
        k, G, mr = R.K_LOOP, R.G_LOOP, R.MR_LOOP
        f = lambda n: T._filled(n + GUARD)   # noqa: E731
        gen, fst, esel, nev = f(4 * N), f(4 * N), f(4 * G), f(4)
        qf.gen_window(t["frame_id"], self.win, gen, fst, esel, nev, G_src=G, N_max=N, n_evict_max=G,
                      n_frames=t["n_frames"])
        qf.stream_reset(esel, nev, k, n_max=G, G_src=G, state=rc.state, store_n=rc.n, seen=self.sent)
        qf.stream_reset(esel, nev, k, n_max=G, G_src=G, seen=rc.rank)
        d = dict(sel=f(4 * G), n_sel=f(4), n_match=f(4), idx=f(2 * G * mr), n=f(4 * G), co=f(G * mr * k),
                 rl=f(4 * G * mr), ro=f(4 * G * mr), est=f(4 * G), fst=f(4 * N))
        qf.parse_poll_headers(t["frames"], t["frame_len"], t["frame_pkt"], gen, d["sel"], d["n_sel"], d["idx"], d["n"],
                              d["co"], d["rl"], d["ro"], d["est"], d["fst"], k, R.L_LOOP, max_rows=mr, frame_stride=fs,
                              N_max=N, G_src=G, n_max=G, n_frames=t["n_frames"], frame_off=t["frame_off"],
                              n_match=d["n_match"])
        _, _, st, ast = rc.listed_poll(d["sel"], d["n_sel"], G, d, mr, t["frames"], N * fs, rank_sel=False)
        n = int(_h(d["n_sel"], np.uint32)[0])
        assert (st[:n] == OK).all() and (ast[:n] == OK).all()
        self.win_status = fst


def test_the_loop_on_the_device_with_both_directions_as_bytes(qf, oracle, gpu_ctx):
    import torch

    from tests import deliver_ref as DR
    from tests import test_gpu_deliver as TD
    from tests import test_gpu_partial_decode as D

    num, den, delay, mask = F.NUM_LOOP, F.DEN_LOOP, F.DELAY_LOOP, F.MASK_LOOP
    spec, polls, stats = F.fb_loop(oracle, num, den, delay, mask, True)
    assert sorted(stats["delivered"]) == list(range(R.GENS_LOOP)) and stats["rereported"]
    k, Lb, G, M, rs, fs = R.K_LOOP, R.L_LOOP, R.G_LOOP, R.M_RELAY, spec.rs, spec.fs
    NR, FM, ML, SS = F.N_REPORTS, F.F_LOOP, F.MAX_LEN_LOOP, F.STRIDE_LOOP
    sh = DR.loop_shape()
    relay, rx = FbNode(qf), FbNode(qf)
    f = lambda n: relay.T._filled(n + GUARD)   # noqa: E731
    fb_state = _guarded(np.zeros(G, C.STATE))
    t_credit = _guarded(np.full(G, C.FILL32, np.uint32))
    nothing = F.PackCall(k, ML, FM, SS, F.poisoned(NR, F.REPORT), 0).blank()
    nothing["n_pkts"][:] = 0
    line = [{key: _guarded(nothing[key]) for key in ("pkts", "pkt_len", "n_pkts")} for _ in range(delay)]
    emitted, left = {}, {}
    for p, model in enumerate(polls):
        gens = model["gens"]
        a, b = spec.source_calls(gens)
        before = a.blank()
        t1 = {key: _guarded(before[key]) for key in before}
        call(qf, a, Dev(a), t1)
        call(qf, b, Dev(b), t1)
        drop = spec.drop_list(gens)
        if drop:
            t1["frame_len"][: 4 * R.N_SRC].view(torch.int32)[torch.tensor(drop, device="cuda")] = 0
        relay.ingest(t1, R.N_SRC, fs)
        # the relay: the packets that arrive now to records, against the model on the downloaded packets
        back = line.pop(0)
        pc = F.ParseCall(k, ML, FM, SS, _h(back["pkts"])[: FM * SS], _h(back["pkt_len"], np.uint32)[:FM], NR,
                         n_pkts=int(_h(back["n_pkts"], np.uint32)[0]))
        pb = pc.blank()
        tp = _outs(pb)
        qf.parse_report_frames(back["pkts"], back["pkt_len"], back["n_pkts"], tp["reports"], tp["n_reports"], k, N_max=NR,
                               max_len=ML, F_max=FM, stride=SS, n_left=tp["n_left"], pkt_status=tp["pkt_status"],
                               pkt_first=tp["pkt_first"], pkt_count=tp["pkt_count"])
        qf.default_context().sync()
        got = _download(tp, pb)
        same(got, pc.model(pb), f"poll {p}, the relay's parse")
        same(got, model["parse_out"], f"poll {p}, the relay's parse against the loop")
        # ... and records and ranks to credit
        rc = relay.rc
        cc = C.CreditCall(k, num, den, C.CAP_LOOP, _h(relay.win, np.uint64)[:G], _h(rc.rank, np.uint32)[:G],
                          _h(relay.sent, np.uint32).copy(), got["reports"], int(got["n_reports"][0]), NR)
        cb = dict(state=_h(fb_state)[: 16 * G].view(C.STATE).copy(), credit=_h(t_credit, np.uint32)[:G].copy(),
                  status=np.full(NR, C.FILL32, np.uint32).view(np.int32))
        t_status = _guarded(cb["status"])
        qf.credit_update(relay.win, rc.rank, relay.sent, fb_state, t_credit, k, G=G, num=num, den=den, cap=C.CAP_LOOP,
                         N_max=NR, reports=tp["reports"], n_reports=tp["n_reports"], report_status=t_status)
        qf.default_context().sync()
        got = {key: _body(v, cb[key]) for key, v in dict(state=fb_state, credit=t_credit, status=t_status).items()}
        same(got, cc.model(cb), f"poll {p}, the relay's credit")
        same(got, model["credit_out"], f"poll {p}, the relay's credit against the loop")
        # select over sent with the credit where the rank was, the listed recode, the ids, the emit
        t_sel, t_nsel, t_ids = f(4 * G), f(4), f(8 * G)
        out, oc, ol, st = f(G * M * rs), f(G * M * k), f(4 * G * M), f(4 * G)
        qf.gen_select(t_credit, t_sel, t_nsel, G=G, min_rank=1, n_max=G, seen=relay.sent)
        qf.recode_frames_sel(t_sel, t_nsel, rc.bytes, rc.off, rc.len, rc.index, rc.coeffs, out, oc, st, k, M, Lb,
                             n_max=G, G_src=G, max_rows=k, src_gen_stride=rc.gs, out_row_stride=rs,
                             out_gen_stride=M * rs, n_rows=rc.n, seed=C.poll_seed(p), out_len=ol)
        qf.gen_window_sel(t_sel, t_nsel, relay.win, n_max=G, G_src=G, ids=t_ids)
        qf.default_context().sync()
        c = spec.relay_call(_h(t_sel, np.uint32)[:G], int(_h(t_nsel, np.uint32)[0]), _h(out)[: G * M * rs],
                            _h(oc)[: G * M * k], _h(ol, np.uint32)[: G * M], _h(st, np.int32)[:G],
                            _h(t_ids, np.uint64)[:G], _h(t_credit, np.uint32)[:G], _h(relay.sent, np.uint32).copy())
        before = c.blank()
        t2 = {key: _guarded(before[key]) for key in before if key != "sent"}
        qf.emit_frames_sel(t_sel, t_nsel, out, t_ids, t2["frames"], t2["frame_len"], t2["frame_off"], t2["frame_id"],
                           t2["frame_pkt"], t2["n_frames"], t2["entry_first"], t2["entry_count"], t2["entry_status"], k, Lb,
                           n_max=G, G_src=G, max_rows=M, N_max=R.N_RELAY, row_stride=rs, rows_gen_stride=M * rs,
                           frame_stride=fs, row_coeffs=oc, row_len=ol, in_status=st, rank=t_credit, sent=relay.sent,
                           n_left=t2["n_left"])
        qf.default_context().sync()
        got = {key: _body(t2[key], before[key]) for key in t2}
        got["sent"] = _h(relay.sent, np.uint32).copy()
        same(got, c.model(before), f"poll {p}, the relay's emit")
        same(got, model["q2"], f"poll {p}, the relay's emit against the loop")
        assert (got["sent"] <= C.CAP_LOOP).all()
        # the forward network: the second hop's drops by each generation's running frame count
        drop = []
        for q in range(int(got["n_frames"][0])):
            g = int(got["frame_id"][q]) - R.BASE_LOOP
            if C.dropped2(g, emitted.get(g, 0)):
                drop.append(q)
            emitted[g] = emitted.get(g, 0) + 1
        assert drop == model["drops"], p
        if drop:
            t2["frame_len"][: 4 * R.N_RELAY].view(torch.int32)[torch.tensor(drop, device="cuda")] = 0
        # the receiver: ingest, select the complete generations, decode, close, deliver, reset
        rx.ingest(t2, R.N_RELAY, fs)
        rc = rx.rc
        t_sel, t_nsel, t_ids = f(4 * G), f(4), f(8 * G)
        qf.gen_select(rc.rank, t_sel, t_nsel, G=G, min_rank=k, n_max=G, seen=rx.sent, mark=True)
        t = D._out_buffers(G, k, sh.e_max, k, sh.rec_gs)
        qf.decode_frames_sel(t_sel, t_nsel, rc.bytes, rc.off, rc.len, rc.index, rc.coeffs, t["rec"], t["ri"], t["nrec"],
                             t["st"], k, k, Lb, n_max=G, G_src=G, max_rows=k, src_gen_stride=rc.gs,
                             rec_row_stride=sh.rec_rs, rec_gen_stride=sh.rec_gs, n_rows=rc.n, src_slot=t["slot"])
        qf.gen_window_sel(t_sel, t_nsel, rx.win, n_max=G, G_src=G, ids=t_ids, close=True)
        o = TD.outputs(sh, G)
        qf.deliver_frames_sel(t_sel, t_nsel, rc.bytes, rc.off, rc.len, t["rec"], t["ri"], t["nrec"], t["st"], t["slot"],
                              o["out"], o["out_len"], o["out_state"], o["n_out"], o["status"], k, sh.e_max, Lb, n_max=G,
                              G_src=G, max_rows=k, src_gen_stride=rc.gs, rec_row_stride=sh.rec_rs,
                              rec_gen_stride=sh.rec_gs, out_row_stride=sh.out_rs, out_gen_stride=sh.out_gs, ids=t_ids)
        qf.stream_reset(t_sel, t_nsel, k, n_max=G, G_src=G, state=rc.state, store_n=rc.n, seen=rx.sent)
        qf.stream_reset(t_sel, t_nsel, k, n_max=G, G_src=G, seen=rc.rank)
        # the two report calls, the re-report appended behind them, the pack
        ra, rb = model["report_calls"]
        rep = {key: _guarded(v) for key, v in ra.blank().items()}
        qf.rank_report_sel(t_sel, t_nsel, rx.win, rc.rank, rep["reports"], rep["n_reports"], k, n_max=G, G_src=G,
                           N_max=NR, n_left=rep["n_left"])
        d_sel, d_nsel = f(4 * G), f(4)
        qf.gen_select(rc.rank, d_sel, d_nsel, G=G, min_rank=1, n_max=G)
        qf.rank_report_sel(d_sel, d_nsel, rx.win, rc.rank, rep["reports"], rep["n_reports"], k, n_max=G, G_src=G,
                           N_max=NR, n_left=rep["n_left"], append=True)
        qf.default_context().sync()
        mid = _download(rep, ra.blank())
        same(mid, model["report_out"][1], f"poll {p}, the receiver's reports against the loop")
        qf.report_closed(t2["frame_id"], rx.win_status, t2["n_frames"], rx.win, rep["reports"], rep["n_reports"], k,
                         G_src=G, F_max=R.N_RELAY, N_max=NR, n_left=rep["n_left"], append=True)
        qf.default_context().sync()
        n_frames = int(_h(t2["n_frames"], np.uint32)[0])
        status = _h(rx.win_status, np.int32)[: R.N_RELAY]
        assert np.array_equal(status[:n_frames], model["frame_status"][:n_frames]), p
        rcall = F.ClosedCall(k, _h(rx.win, np.uint64)[:G], _h(t2["frame_id"], np.uint64)[: R.N_RELAY], status, NR,
                             n_frames=n_frames, append=True)
        got = _download(rep, ra.blank())
        same(got, rcall.model(mid), f"poll {p}, the receiver's re-report")
        same(got, model["closed_out"], f"poll {p}, the receiver's re-report against the loop")
        fc = F.PackCall(k, ML, FM, SS, got["reports"], int(got["n_reports"][0]), NR)
        fb = fc.blank()
        tf = _outs(fb)
        qf.frame_reports(rep["reports"], rep["n_reports"], tf["pkts"], tf["pkt_len"], tf["n_pkts"], k, N_max=NR, max_len=ML,
                         F_max=FM, stride=SS, n_left=tf["n_left"], n_skipped=tf["n_skipped"])
        qf.default_context().sync()
        got = _download(tf, fb)
        same(got, fc.model(fb), f"poll {p}, the receiver's packets")
        same(got, model["pack_out"], f"poll {p}, the receiver's packets against the loop")
        # the back network: a dropped packet arrives with length 0
        drop = [j for j in range(int(got["n_pkts"][0])) if F.dropped_fb(mask, p, j)]
        assert drop == model["fb_drops"], p
        if drop:
            tf["pkt_len"][: 4 * FM].view(torch.int32)[torch.tensor(drop, device="cuda")] = 0
        line.append(tf)
        n_done = int(_h(t_nsel, np.uint32)[0])
        assert _h(t_sel, np.uint32)[:n_done].tolist() == model["done"], p
        ids, lens = _h(t_ids, np.uint64), _h(o["out_len"], np.uint32)
        state, data = _h(o["out_state"]), _h(o["out"])
        assert (_h(o["status"], np.int32)[:n_done] == OK).all() and (_h(o["n_out"], np.uint32)[:n_done] == k).all()
        for j in range(n_done):
            g = int(ids[j]) - R.BASE_LOOP
            for i in range(k):
                assert state[j * k + i] in (DR.STORED, DR.RECOVERED) and lens[j * k + i] == Lb
                assert (g, i) not in left, f"source {i} of generation {g} left twice"
                at = j * sh.out_gs + i * sh.out_rs
                left[(g, i)] = data[at: at + Lb].copy()
    # the receiver's deliver outputs are the 12 x 4 sources, each exactly once
    assert sorted(left) == [(g, i) for g in range(R.GENS_LOOP) for i in range(k)]
    for (g, i), row in left.items():
        assert np.array_equal(row, spec.src[g, i]), (g, i)
    assert emitted == stats["emitted"]


def test_profile_names(qf, gpu_ctx):
    c = F.pack_cases()["S_per_plus_1"]
    pc, pbefore = F.parse_cases()["append_base0"]
    rc, rbefore = F.closed_cases()["append_mid"]
    gpu_ctx.sync()
    gpu_ctx.profile(True)
    pack_against_model(qf, c)
    parse_against_model(qf, pc, pbefore)
    closed_against_model(qf, rc, rbefore)
    names = gpu_ctx.kernel_times()
    gpu_ctx.profile(False)
    assert set(names) == {"k_fbw_count", "k_fbw_pack", "k_fbr_count", "k_fbr_place", "k_fbr_records", "k_closed_mark",
                          "k_gen_select", "k_report_sel"}, names
