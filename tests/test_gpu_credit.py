"""The feedback calls on the MI355X: qf_credit_update_dev and
qf_rank_report_sel_dev against tests/credit_ref.py over the case tables, their
call-level errors, and the lossy hop: source -> relay -> receiver with real
calls throughout, the relay's budget from qf_credit_update_dev and the
receiver's reports from qf_rank_report_sel_dev, the test playing the network.

Every output buffer starts as 0xCC (the feedback state as the case sets it)
with guard bytes behind it and is compared whole with the model's, so the bytes
a call must not write are checked too.  Every case runs twice and every byte
of the two runs is equal."""
import numpy as np
import pytest

from tests import credit_ref as C
from tests import emit_ref as R
from tests.test_gpu_emit import Dev, DevNode, _body, _dev, _guarded, _h, call, same

pytestmark = pytest.mark.gpu

OK, EINVAL = C.OK, C.EINVAL
GUARD = 64


def _download(t, before):
    return {key: _body(t[key], before[key]) for key in t}


def credit_call(qf, c, t, d):
    qf.credit_update(d["win"], d["rank"], d["sent"], t["state"], t["credit"], c.k, G=c.G, num=c.num, den=c.den,
                     cap=c.cap, N_max=c.N_max, reports=d["reports"], n_reports=d["n_reports"],
                     report_status=t["status"] if c.status else None)
    qf.default_context().sync()


def credit_inputs(c):
    return dict(win=_dev(c.win), rank=_dev(c.rank), sent=_dev(c.sent),
                reports=None if c.N_max == 0 else _dev(c.reports),
                n_reports=None if c.n_reports is None else _dev(np.array([c.n_reports], np.uint32)))


def credit_against_model(qf, c, before):
    """The call twice from the same buffers: equal to each other and to the model; the inputs are only read."""
    d = credit_inputs(c)
    runs = []
    for _ in range(2):
        t = {key: _guarded(before[key]) for key in before}
        credit_call(qf, c, t, d)
        runs.append(_download(t, before))
    want = c.model(before)
    same(runs[0], want, "credit_update")
    for key in want:
        assert np.array_equal(runs[0][key].view(np.uint8), runs[1][key].view(np.uint8)), f"{key}: two runs differ"
    for key, a in (("win", c.win), ("rank", c.rank), ("sent", c.sent), ("reports", c.reports)):
        if d[key] is not None:
            assert np.array_equal(_h(d[key]), np.ascontiguousarray(a).view(np.uint8).reshape(-1)), "an input was written"
    return want


def report_call(qf, c, t, d, n_left=True):
    qf.rank_report_sel(d["sel"], d["n_sel"], d["win"], d["rank"], t["reports"], t["n_reports"], c.k, n_max=c.n_max,
                       G_src=c.G_src, N_max=c.N_max, n_left=t["n_left"] if n_left else None, append=c.append)
    qf.default_context().sync()


def report_inputs(c):
    return dict(sel=_dev(c.sel), win=_dev(c.win), rank=_dev(c.rank),
                n_sel=None if c.n_sel is None else _dev(np.array([c.n_sel], np.uint32)))


def report_against_model(qf, c, before, n_left=True):
    d = report_inputs(c)
    runs = []
    for _ in range(2):
        t = {key: _guarded(before[key]) for key in before}
        report_call(qf, c, t, d, n_left)
        runs.append(_download(t, before))
    want = c.model(before)
    if not n_left:
        want["n_left"] = before["n_left"]
    same(runs[0], want, "rank_report_sel")
    for key in want:
        assert np.array_equal(runs[0][key].view(np.uint8), runs[1][key].view(np.uint8)), f"{key}: two runs differ"
    for key, a in (("sel", c.sel), ("win", c.win), ("rank", c.rank)):
        assert np.array_equal(_h(d[key]), np.ascontiguousarray(a).view(np.uint8).reshape(-1)), "an input was written"
    return want


# ---------------------------------------------------------------------------
# 1: the case tables
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(C.credit_cases()))
def test_credit_cases_against_the_model(qf, gpu_ctx, name):
    c, before = C.credit_cases()[name]
    want = credit_against_model(qf, c, before)
    if name == "one_slot_many_waves":          # reports of one slot in three waves: the maximum wins
        assert want["state"]["peer"].tolist() == [0, 57, 0, 0, 0] and want["credit"].tolist() == [0, 60, 0, 0, 0]
    if name == "id_edges":
        assert want["status"].tolist() == [OK, EINVAL, EINVAL, EINVAL]
    if name == "n_reports_mid":
        assert (want["status"][17:] == -858993460).all()


@pytest.mark.parametrize("name", sorted(C.credit_sequences()))
def test_credit_sequences_against_the_model(qf, gpu_ctx, name):
    state = credit = None
    outs = []
    for c in C.credit_sequences()[name]:
        o = credit_against_model(qf, c, c.blank(state, credit))
        state, credit = o["state"], o["credit"]
        outs.append(o)
    if name == "restart":                      # the slot's entry changed: the old peer and credit are gone
        assert outs[0]["credit"].tolist() == [6, 6, 3, 0] and outs[1]["credit"].tolist() == [6, 2, 3, 0]
        assert outs[1]["state"]["peer"][1] == 0
    if name == "repeat":
        assert [int(o["credit"][2]) for o in outs] == [5, 7, 7, 7, 7]


def test_without_redundancy_and_reports_the_credit_is_the_rank(qf, gpu_ctx):
    c, _ = C.make_credit(130, 64, 1, 1, 1 << 20, 0, 301)
    want = credit_against_model(qf, c, c.blank())
    assert np.array_equal(want["credit"], np.where(c.win == 0, 0, np.minimum(c.rank, 64)))


@pytest.mark.parametrize("name", sorted(C.report_cases()))
def test_report_cases_against_the_model(qf, gpu_ctx, name):
    c, before, n_left = C.report_cases()[name]
    want = report_against_model(qf, c, before, n_left)
    if name == "overflow":
        assert (want["n_reports"][0], want["n_left"][0]) == (12, 8)
    if name == "append_base_above":
        assert np.array_equal(want["reports"], before["reports"]) and want["n_left"][0] == 20


# ---------------------------------------------------------------------------
# 2: the call-level errors write nothing
# ---------------------------------------------------------------------------
def _shifted(t, off):
    """A buffer as large as t that starts off bytes behind an aligned address."""
    import torch

    return torch.zeros(t.numel() + off, dtype=torch.uint8, device="cuda")[off:]


def _refused(qf, fn):
    with pytest.raises(qf.QfError) as e:
        fn()
    assert e.value.status == EINVAL
    qf.default_context().sync()


def test_credit_update_refuses_and_writes_nothing(qf, gpu_ctx):
    c, before = C.make_credit(23, 4, 3, 2, 16, 40, 400)
    d = credit_inputs(c)
    t = {key: _guarded(before[key]) for key in before}
    base = dict(k=c.k, G=c.G, num=3, den=2, cap=16, N_max=c.N_max)
    ptrs = dict(win=d["win"], rank=d["rank"], sent=d["sent"], fb_state=t["state"], credit=t["credit"],
                reports=d["reports"])

    def call(**kw):
        a = {**base, **{key: v for key, v in kw.items() if key in base}}
        p = {**ptrs, **{key: v for key, v in kw.items() if key in ptrs}}
        qf.credit_update(p["win"], p["rank"], p["sent"], p["fb_state"], p["credit"], a["k"], G=a["G"], num=a["num"],
                         den=a["den"], cap=a["cap"], N_max=a["N_max"], reports=p["reports"], n_reports=d["n_reports"],
                         report_status=t["status"])

    bad = [dict(k=0), dict(k=257), dict(den=0), dict(num=1, den=2), dict(num=65536, den=1), dict(cap=0),
           dict(cap=(1 << 20) + 1), dict(G=0), dict(win=None), dict(rank=None), dict(sent=None),
           dict(fb_state=None), dict(credit=None), dict(reports=None), dict(win=_shifted(d["win"], 4)),
           dict(reports=_shifted(d["reports"], 8)), dict(fb_state=t["state"][8:])]
    for kw in bad:
        _refused(qf, lambda kw=kw: call(**kw))
    import ctypes

    from quicfuscate_amd import _lib as L
    for sh in (L.CreditShape(4, 3, 2, 16, 1, 0), L.CreditShape(4, 3, 2, 16, 0, 1)):   # flags, reserved
        assert L._lib().qf_credit_update_dev(gpu_ctx.handle, ctypes.byref(sh), c.G, d["win"].data_ptr(),
                                             d["rank"].data_ptr(), d["sent"].data_ptr(), 0, None, None,
                                             t["state"].data_ptr(), t["credit"].data_ptr(), None) == EINVAL
    sh = L.CreditShape(4, 3, 2, 16, 0, 0)                                             # G above 2^24
    assert L._lib().qf_credit_update_dev(gpu_ctx.handle, ctypes.byref(sh), (1 << 24) + 1, d["win"].data_ptr(),
                                         d["rank"].data_ptr(), d["sent"].data_ptr(), 0, None, None,
                                         t["state"].data_ptr(), t["credit"].data_ptr(), None) == EINVAL
    assert L._lib().qf_credit_update_dev(gpu_ctx.handle, None, c.G, d["win"].data_ptr(), d["rank"].data_ptr(),
                                         d["sent"].data_ptr(), 0, None, None, t["state"].data_ptr(),
                                         t["credit"].data_ptr(), None) == EINVAL
    gpu_ctx.sync()
    same(_download(t, before), before, "a refused credit_update")
    call()                                     # ... and the same buffers are good for a call
    gpu_ctx.sync()
    same(_download(t, before), c.model(before), "credit_update after the refusals")


def test_rank_report_sel_refuses_and_writes_nothing(qf, gpu_ctx):
    c = C.make_report(4, 20, 23, 30, 401, append=True)
    before = c.blank(3)
    d = report_inputs(c)
    t = {key: _guarded(before[key]) for key in before}
    base = dict(k=c.k, n_max=c.n_max, G_src=c.G_src, N_max=c.N_max)
    ptrs = dict(sel=d["sel"], win=d["win"], rank=d["rank"], reports=t["reports"], n_reports=t["n_reports"])

    def call(**kw):
        a = {**base, **{key: v for key, v in kw.items() if key in base}}
        p = {**ptrs, **{key: v for key, v in kw.items() if key in ptrs}}
        qf.rank_report_sel(p["sel"], None, p["win"], p["rank"], p["reports"], p["n_reports"], a["k"], n_max=a["n_max"],
                           G_src=a["G_src"], N_max=a["N_max"], n_left=t["n_left"], append=True)

    bad = [dict(k=0), dict(k=257), dict(n_max=0), dict(G_src=0), dict(N_max=0), dict(win=None), dict(rank=None),
           dict(reports=None), dict(n_reports=None), dict(reports=t["reports"][8:])]
    for kw in bad:
        _refused(qf, lambda kw=kw: call(**kw))
    import ctypes

    from quicfuscate_amd import _lib as L
    gs = L.GenSel(d["sel"].data_ptr(), None, c.n_max, c.G_src)
    args = (d["win"].data_ptr(), d["rank"].data_ptr(), c.N_max)
    outs = (t["reports"].data_ptr(), t["n_reports"].data_ptr(), t["n_left"].data_ptr())
    lib = L._lib()
    assert lib.qf_rank_report_sel_dev(gpu_ctx.handle, c.k, ctypes.byref(gs), *args, 2, *outs) == EINVAL   # unknown flag
    assert lib.qf_rank_report_sel_dev(gpu_ctx.handle, c.k, None, *args, 0, *outs) == EINVAL
    gs0 = L.GenSel(None, None, c.n_max, c.G_src)
    assert lib.qf_rank_report_sel_dev(gpu_ctx.handle, c.k, ctypes.byref(gs0), *args, 0, *outs) == EINVAL
    gpu_ctx.sync()
    same(_download(t, before), before, "a refused rank_report_sel")
    call()
    gpu_ctx.sync()
    same(_download(t, before), c.model(before), "rank_report_sel after the refusals")


# ---------------------------------------------------------------------------
# 3: the lossy hop on the device
# ---------------------------------------------------------------------------
def test_the_lossy_hop_on_the_device(qf, oracle, gpu_ctx):
    import torch

    from tests import deliver_ref as DR
    from tests import test_gpu_deliver as TD
    from tests import test_gpu_partial_decode as D

    num, den = 1, 1                            # no blind redundancy: without the reports 2 of 12 arrive
    spec, polls, stats = C.lossy_loop(oracle, num, den, True)
    assert sorted(stats["delivered"]) == list(range(R.GENS_LOOP))
    k, Lb, G, M, rs, fs = R.K_LOOP, R.L_LOOP, R.G_LOOP, R.M_RELAY, spec.rs, spec.fs
    NR = C.N_REPORTS
    sh = DR.loop_shape()
    relay, rx = DevNode(qf), DevNode(qf)
    f = lambda n: relay.T._filled(n + GUARD)   # noqa: E731
    fb_state = _guarded(np.zeros(G, C.STATE))
    t_credit = _guarded(np.full(G, C.FILL32, np.uint32))
    # the report buffer as it arrives at the relay: what the receiver wrote in the poll before
    back = dict(reports=_guarded(C.poisoned(NR, C.REPORT)), n_reports=_guarded(np.zeros(1, np.uint32)))
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
        # the relay: the credit from the ranks and last poll's reports, against the model on its downloaded inputs
        rc = relay.rc
        cc = C.CreditCall(k, num, den, C.CAP_LOOP, _h(relay.win, np.uint64)[:G], _h(rc.rank, np.uint32)[:G],
                          _h(relay.sent, np.uint32).copy(), _h(back["reports"])[: 16 * NR].view(C.REPORT),
                          int(_h(back["n_reports"], np.uint32)[0]), NR)
        cb = dict(state=_h(fb_state)[: 16 * G].view(C.STATE).copy(), credit=_h(t_credit, np.uint32)[:G].copy(),
                  status=np.full(NR, C.FILL32, np.uint32).view(np.int32))
        t_status = _guarded(cb["status"])
        qf.credit_update(relay.win, rc.rank, relay.sent, fb_state, t_credit, k, G=G, num=num, den=den, cap=C.CAP_LOOP,
                         N_max=NR, reports=back["reports"], n_reports=back["n_reports"], report_status=t_status)
        qf.default_context().sync()
        got = _download(dict(state=fb_state, credit=t_credit, status=t_status), cb)
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
        # the network: the second hop's drops by each generation's running frame count
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
        # the two report calls: the completed list, then every open generation that holds a row
        ra, rb = model["report_calls"]
        rep = {key: _guarded(v) for key, v in ra.blank().items()}
        qf.rank_report_sel(t_sel, t_nsel, rx.win, rc.rank, rep["reports"], rep["n_reports"], k, n_max=G, G_src=G,
                           N_max=NR, n_left=rep["n_left"])
        d_sel, d_nsel = f(4 * G), f(4)
        qf.gen_select(rc.rank, d_sel, d_nsel, G=G, min_rank=1, n_max=G)
        qf.rank_report_sel(d_sel, d_nsel, rx.win, rc.rank, rep["reports"], rep["n_reports"], k, n_max=G, G_src=G,
                           N_max=NR, n_left=rep["n_left"], append=True)
        qf.default_context().sync()
        n_done = int(_h(t_nsel, np.uint32)[0])
        assert _h(t_sel, np.uint32)[:n_done].tolist() == model["done"], p
        # both calls against the model on the receiver's downloaded window, ranks and lists, and against the loop
        win, rank = _h(rx.win, np.uint64)[:G], _h(rc.rank, np.uint32)[:G]
        n_dead = int(_h(d_nsel, np.uint32)[0])
        ca = C.ReportCall(k, _h(t_sel, np.uint32)[:G], win, rank, NR, n_sel=n_done)
        cb2 = C.ReportCall(k, _h(d_sel, np.uint32)[:G], win, rank, NR, n_sel=n_dead, append=True)
        got = _download(rep, ra.blank())
        same(got, cb2.model(ca.model()), f"poll {p}, the receiver's reports")
        same(got, model["report_out"][1], f"poll {p}, the receiver's reports against the loop")
        back = rep                               # ... reach the relay in the next poll, losslessly
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
    c, before = C.credit_cases()["N65"]
    r, rbefore, _ = C.report_cases()["append_base_mid"]
    gpu_ctx.sync()
    gpu_ctx.profile(True)
    credit_against_model(qf, c, before)
    report_against_model(qf, r, rbefore)
    names = gpu_ctx.kernel_times()
    gpu_ctx.profile(False)
    assert set(names) == {"k_credit_reports", "k_credit_apply", "k_report_sel"}, names
