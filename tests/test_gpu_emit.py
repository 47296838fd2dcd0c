"""The send step on the MI355X: qf_emit_frames_sel_dev against
tests/emit_ref.py at the shape edges, over lists with every kind of entry, at
the queue's edges, with the budget across calls, at the scan's and the copy
grid's edges, and with its outputs fed unmodified into the next hop's window
and poll calls.

Every output buffer starts as 0xCC with guard bytes behind it and is compared
whole with the model's, so the bytes a call must not write are checked too;
rows outside their length are 0xCC as well, so a kernel that copies a row past
its length changes a frame byte.  Every case runs twice and every byte of the
two runs is equal."""
import numpy as np
import pytest

from tests import emit_ref as R

pytestmark = pytest.mark.gpu

FILL, GUARD = R.FILL, 64
OK, EINVAL, ENOTREADY = R.OK, R.EINVAL, R.ENOTREADY
KEYS = ("frames", "frame_len", "frame_off", "frame_id", "frame_pkt", "n_frames", "n_left", "entry_first",
        "entry_count", "entry_status")
GROUPS_PER_CU = 16     # kEmitGroupsPerCu (qf_kernels.h): the copy's grid bound, workgroups of four waves per CU
PER_BLOCK = 64         # kEmitPerBlock (qf_kernels.h): entries of one scan block


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _opt(a):
    return None if a is None else _dev(a)


def _guarded(a):
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return _dev(np.concatenate([raw, np.full(GUARD, FILL, np.uint8)]))


def _body(t, like):
    """A guarded device buffer's bytes as `like`'s type; the guard must be 0xCC."""
    h = t.cpu().numpy()
    assert (h[like.nbytes:] == FILL).all(), "bytes behind an output were written"
    return h[: like.nbytes].view(like.dtype).copy()


class Dev:
    """A Call's inputs on the device."""

    def __init__(self, c):
        self.sel, self.rows, self.ids = _dev(c.sel), _dev(c.rows), _dev(c.ids)
        self.n_sel = None if c.n_sel is None else _dev(np.array([c.n_sel], np.uint32))
        self.ri, self.nr, self.co = _opt(c.row_index), _opt(c.n_rows), _opt(c.row_coeffs)
        self.rl, self.st, self.rank = _opt(c.row_len), _opt(c.in_status), _opt(c.rank)
        self.inputs = [(self.sel, c.sel), (self.rows, c.rows), (self.ids, c.ids), (self.ri, c.row_index),
                       (self.nr, c.n_rows), (self.co, c.row_coeffs), (self.rl, c.row_len), (self.st, c.in_status),
                       (self.rank, c.rank)]

    def unchanged(self):
        for t, a in self.inputs:
            if t is not None:
                assert np.array_equal(t.cpu().numpy(), np.ascontiguousarray(a).view(np.uint8).reshape(-1)), \
                    "an input was written"


def call(qf, c, d, t, n_left=True):
    """One call over a Call's device inputs d into the device buffers t."""
    qf.emit_frames_sel(d.sel, d.n_sel, d.rows, d.ids, t["frames"], t["frame_len"], t["frame_off"], t["frame_id"],
                       t["frame_pkt"], t["n_frames"], t["entry_first"], t["entry_count"], t["entry_status"], c.k, c.L,
                       n_max=c.n_max, G_src=c.G_src, max_rows=c.max_rows, N_max=c.N_max, row_stride=c.row_stride,
                       rows_gen_stride=c.rows_gen_stride, frame_stride=c.frame_stride, row_index=d.ri, n_rows=d.nr,
                       row_coeffs=d.co, row_len=d.rl, in_status=d.st, rank=d.rank, sent=t.get("sent"),
                       n_left=t["n_left"] if n_left else None, append=c.append)
    qf.default_context().sync()
    d.unchanged()


def launch(qf, c, d, before, n_left=True):
    """One call from the buffers `before` -> every output buffer, downloaded."""
    t = {key: _guarded(before[key]) for key in before}
    call(qf, c, d, t, n_left)
    return {key: _body(t[key], before[key]) for key in before}


def same(got, want, what):
    for key in want:
        bad = np.flatnonzero(got[key].reshape(-1) != want[key].reshape(-1))
        assert bad.size == 0, f"{what}: {key} differs from the model at {bad[:6].tolist()}"


def against_model(qf, c, before=None, n_left=True):
    """The call twice from the same buffers: equal to each other and to the model."""
    before = before or c.blank()
    d = Dev(c)
    got = launch(qf, c, d, before, n_left)
    again = launch(qf, c, d, before, n_left)
    want = c.model(before)
    if not n_left:
        want["n_left"] = before["n_left"]
    for key in want:
        bad = np.flatnonzero(got[key].reshape(-1) != want[key].reshape(-1))
        assert bad.size == 0, f"{key} differs from the model at {bad[:6].tolist()}"
        assert np.array_equal(got[key], again[key]), f"{key}: two runs differ"
    return want


# ---------------------------------------------------------------------------
# 1: shapes, lists, the queue, the budget
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.cases()))
def test_cases_against_the_model(qf, gpu_ctx, name):
    c = R.cases()[name]
    before = c.blank(5) if name == "stale_n_frames" else None   # without append a stale length is ignored
    want = against_model(qf, c, before)
    st = want["entry_status"].tolist()
    if name.startswith(("k", "L")):
        assert set(st) == {OK} and want["n_frames"][0] > 0 and want["n_left"][0] == 0
    if name == "list":
        assert st == [OK, EINVAL, EINVAL, EINVAL, R.ERANK, EINVAL, OK, ENOTREADY, ENOTREADY]
    if name == "list_coded_without_vectors":
        assert st == [OK, EINVAL, OK]
    if name == "cutoff":
        assert st == [OK, OK] + [ENOTREADY] * 4 and (want["n_frames"][0], want["n_left"][0]) == (7, 10)
    if name == "exact_fit":
        assert set(st) == {OK} and (want["n_frames"][0], want["n_left"][0]) == (10, 0)
    if name == "stale_n_frames":
        assert want["n_frames"][0] == 10 and want["entry_first"].tolist() == [0, 5]
    if name == "budget":                       # rank - sent of 0 and below n_j, and sent above rank
        assert want["entry_count"].tolist() == [0, 3, 2, 0, 0] and want["sent"].tolist() == [3, 4, 2, 0, 5]
    if name == "budget_above_rows":            # rank - sent = 4, 2, 3, 1 against n_j = 2, 5, 1, 0
        assert want["entry_count"].tolist() == [2, 2, 1, 0] and want["sent"].tolist() == [7, 2, 1, 0]
        assert set(st) == {OK} and (want["n_frames"][0], want["n_left"][0]) == (5, 0)


@pytest.mark.parametrize("name", sorted(R.APPEND_BASES))
def test_append(qf, gpu_ctx, name):
    c, before = R.append_case(name)
    want = against_model(qf, c, before, n_left=name != "base_mid")
    base = min(R.APPEND_BASES[name], c.N_max)
    assert want["n_frames"][0] == (10 if base == 0 else 8 if base == 3 else c.N_max)
    assert (want["frames"].reshape(c.N_max, -1)[:base] == FILL).all()


def test_the_budget_across_calls(qf, gpu_ctx):
    c = R.cases()["budget_overflow"]
    first = against_model(qf, c)
    assert first["entry_count"].tolist() == [1, 2, 3, 0] and first["n_left"][0] == 4
    assert first["entry_status"].tolist() == [OK, OK, OK, ENOTREADY]
    c.sent = first["sent"]                    # the overflowed entry kept its sent: it leaves now
    second = against_model(qf, c)
    assert second["entry_count"].tolist() == [0, 0, 0, 4] and second["sent"].tolist() == c.rank.tolist()
    c.sent = second["sent"]                   # unchanged ranks: nothing is emitted, no frame byte is written
    third = against_model(qf, c)
    assert third["n_frames"][0] == 0 and (third["frames"] == FILL).all() and set(third["entry_status"]) == {OK}


# ---------------------------------------------------------------------------
# 2: the scale edges at tiny rows
# ---------------------------------------------------------------------------
def test_scan_blocks_and_grid_rounds(qf, gpu_ctx):
    import torch

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    one_round = cus * GROUPS_PER_CU * 16          # frames of one round of the bounded grid
    cs = R.scale_cases(PER_BLOCK, one_round + 64)
    want = against_model(qf, cs["scan_blocks"])
    assert want["n_left"][0] > 0 and (want["entry_status"] == OK).sum() > 2 * PER_BLOCK
    want = against_model(qf, cs["grid_rounds"])
    assert want["n_frames"][0] > one_round and want["n_left"][0] == 0


# ---------------------------------------------------------------------------
# 3: the hop on the device: source -> relay -> receiver with real calls
# ---------------------------------------------------------------------------
class DevNode:
    """A relay or receiver on the device: the window, the rank states and row store, sent / seen."""

    def __init__(self, qf):
        import torch

        from tests import test_gpu_poll_ingest as T

        self.qf, self.T = qf, T
        self.rc = T.Receiver(qf, R.G_LOOP, R.K_LOOP, R.L_LOOP, R.K_LOOP, 0)
        self.win = _guarded(np.zeros(R.G_LOOP, np.uint64))
        self.sent = torch.zeros(R.G_LOOP, dtype=torch.int32, device="cuda")      # the receiver's seen

    def ingest(self, t, N, fs):
        """A queue's device buffers, as the emit call left them, through the window, the ingest, the listed
        update and the append.  No value comes to the host in between."""
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


def _h(t, dt=np.uint8):
    return t.cpu().numpy().view(dt)


def test_the_hop_on_the_device(qf, oracle, gpu_ctx):
    import torch

    from tests import deliver_ref as DR
    from tests import test_gpu_deliver as TD
    from tests import test_gpu_partial_decode as D

    spec, polls, stats = R.loop_model(oracle)
    k, Lb, G, M, rs, fs = R.K_LOOP, R.L_LOOP, R.G_LOOP, R.M_RELAY, spec.rs, spec.fs
    sh = DR.loop_shape()
    assert (DR.K_LOOP, DR.L_LOOP, DR.G_LOOP) == (k, Lb, G)
    relay, rx = DevNode(qf), DevNode(qf)
    f = lambda n: relay.T._filled(n + GUARD)   # noqa: E731
    left = {}
    for p, gens in enumerate(R.SCHED):
        # the source's two calls into one queue, each against the model; then the first hop's drops
        a, b = spec.source_calls(gens)
        before = a.blank()
        t1 = {key: _guarded(before[key]) for key in before}
        call(qf, a, Dev(a), t1)
        mid = a.model(before)
        same({key: _body(t1[key], before[key]) for key in before}, mid, f"poll {p}, the source's packets")
        call(qf, b, Dev(b), t1)
        same({key: _body(t1[key], before[key]) for key in before}, b.model(mid), f"poll {p}, the source's repairs")
        drop = spec.drop_list(gens)
        if drop:
            t1["frame_len"][: 4 * R.N_SRC].view(torch.int32)[torch.tensor(drop, device="cuda")] = 0
        relay.ingest(t1, R.N_SRC, fs)
        # the relay: select over sent, the listed recode, the ids, the emit with the budget
        rc = relay.rc
        t_sel, t_nsel, t_ids = f(4 * G), f(4), f(8 * G)
        out, oc, ol, st = f(G * M * rs), f(G * M * k), f(4 * G * M), f(4 * G)
        qf.gen_select(rc.rank, t_sel, t_nsel, G=G, min_rank=1, n_max=G, seen=relay.sent)
        qf.recode_frames_sel(t_sel, t_nsel, rc.bytes, rc.off, rc.len, rc.index, rc.coeffs, out, oc, st, k, M, Lb,
                             n_max=G, G_src=G, max_rows=k, src_gen_stride=rc.gs, out_row_stride=rs,
                             out_gen_stride=M * rs, n_rows=rc.n, seed=R.SEED_LOOP + p, out_len=ol)
        qf.gen_window_sel(t_sel, t_nsel, relay.win, n_max=G, G_src=G, ids=t_ids)
        qf.default_context().sync()
        # the call's inputs as they are on the device -> the model
        c = spec.relay_call(_h(t_sel, np.uint32)[:G], int(_h(t_nsel, np.uint32)[0]), _h(out)[: G * M * rs],
                            _h(oc)[: G * M * k], _h(ol, np.uint32)[: G * M], _h(st, np.int32)[:G],
                            _h(t_ids, np.uint64)[:G], _h(rc.rank, np.uint32)[:G], _h(relay.sent, np.uint32).copy())
        before = c.blank()
        t2 = {key: _guarded(before[key]) for key in before if key != "sent"}
        qf.emit_frames_sel(t_sel, t_nsel, out, t_ids, t2["frames"], t2["frame_len"], t2["frame_off"], t2["frame_id"],
                           t2["frame_pkt"], t2["n_frames"], t2["entry_first"], t2["entry_count"], t2["entry_status"], k, Lb,
                           n_max=G, G_src=G, max_rows=M, N_max=R.N_RELAY, row_stride=rs, rows_gen_stride=M * rs,
                           frame_stride=fs, row_coeffs=oc, row_len=ol, in_status=st, rank=rc.rank, sent=relay.sent,
                           n_left=t2["n_left"])
        qf.default_context().sync()
        got = {key: _body(t2[key], before[key]) for key in t2}
        got["sent"] = _h(relay.sent, np.uint32).copy()
        want = c.model(before)
        same(got, want, f"poll {p}, the relay's emit")
        # ... and the models' loop saw the same call
        q2 = polls[p]["q2"]
        assert c.n_sel == len(polls[p]["listed"]) and np.array_equal(got["entry_count"], q2["entry_count"]), p
        assert np.array_equal(got["frames"], q2["frames"]) and got["n_left"][0] == q2["n_left"][0], p
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
        qf.default_context().sync()
        n_done = int(_h(t_nsel, np.uint32)[0])
        assert _h(t_sel, np.uint32)[:n_done].tolist() == polls[p]["done"], p
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
    # the receiver's deliver outputs are the sources' bytes, each exactly once
    assert sorted(left) == [(g, i) for g in range(R.GENS_LOOP) for i in range(k)]
    for (g, i), row in left.items():
        assert np.array_equal(row, spec.src[g, i]), (g, i)


def test_profile_names(qf, gpu_ctx):
    c = R.cases()["k13"]
    gpu_ctx.sync()
    gpu_ctx.profile(True)
    against_model(qf, c)
    names = gpu_ctx.kernel_times()
    gpu_ctx.profile(False)
    assert set(names) == {"k_emit_count", "k_emit_place", "k_emit_frames"}, names
