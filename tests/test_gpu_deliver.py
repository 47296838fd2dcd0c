"""The delivery step on the MI355X: qf_deliver_frames_dev and its listed form
against tests/deliver_ref.py, on synthetic decode outputs at the shape edges,
on the outputs of the decode calls fed straight in, across calls that share a
delivered state, and in the streaming loop with deliver steps 1b and 7a.

Every output buffer starts as 0xCC with guard bytes behind it and is compared
whole with a buffer built by the model, so the bytes a call must not write are
checked too.  Every byte of a source region outside the rows is 0xCC and so is
rec outside its rows, so a kernel that reads a row past its length changes an
output byte."""
import numpy as np
import pytest

from tests import deliver_ref as R
from tests import partial_ref as P
from tests import poll_ref as PR
from tests import test_gpu_partial_decode as D
from tests import test_gpu_poll_ingest as T
from tests import test_gpu_stream_window as SW

pytestmark = pytest.mark.gpu

FILL, GUARD, NONE16 = T.FILL, T.GUARD, T.NONE16
OK, EINVAL, ENOTREADY = 0, -1, -3
_r16, _dev, _filled, _host, _body = T._r16, T._dev, T._filled, T._host, T._body
KEYS = ("out", "out_len", "out_state", "n_out", "n_known", "status")
GROUPS_PER_CU = 16     # kDeliverGroupsPerCu (qf_kernels.h): the copy's grid bound, workgroups of four waves per CU
BOUND_MARGIN = 2       # the stride case still makes a second round with a bound up to this many times that


shape_cases = R.shape_cases


# ---------------------------------------------------------------------------
# a call on the device
# ---------------------------------------------------------------------------
class Dev:
    """A Call's inputs on the device; the state with guard bytes behind it."""

    def __init__(self, c):
        d = c.dec
        self.src, self.off, self.len = _dev(c.src), _dev(c.row_off), _dev(c.row_len)
        self.rec = None if d["rec"] is None else _dev(d["rec"])
        self.ri = None if d["rec_index"] is None else _dev(d["rec_index"])
        self.nrec, self.st, self.slot = _dev(d["n_rec"]), _dev(d["dec_status"]), _dev(d["src_slot"])
        self.ids = None if c.ids is None else _dev(np.asarray(c.ids, np.uint64))
        self.state = None if c.delivered is None else SW._guarded(np.asarray(c.delivered, np.uint64))
        self.sel = None if c.sel is None else _dev(np.asarray(c.sel, np.uint32))
        self.n_sel = None if c.n_sel is None else _dev(np.array([c.n_sel], np.uint32))
        self.inputs = [(self.src, c.src), (self.off, c.row_off), (self.len, c.row_len), (self.rec, d["rec"]),
                       (self.ri, d["rec_index"]), (self.nrec, d["n_rec"]), (self.st, d["dec_status"]),
                       (self.slot, d["src_slot"]), (self.ids, None if c.ids is None else np.asarray(c.ids, np.uint64)),
                       (self.sel, None if c.sel is None else np.asarray(c.sel, np.uint32))]

    def unchanged(self):
        for t, a in self.inputs:
            if t is not None:
                assert np.array_equal(_host(t), np.ascontiguousarray(a).view(np.uint8).reshape(-1)), "an input was written"


def outputs(sh, G):
    k = sh.k
    return dict(out=_filled(G * sh.out_gs + GUARD), out_len=_filled(4 * G * k + GUARD), out_state=_filled(G * k + GUARD),
                n_out=_filled(4 * G + GUARD), n_known=_filled(4 * G + GUARD), status=_filled(4 * G + GUARD))


def launch(qf, c, d, t, n_known=True, **over):
    """One call over the device copies d into the output tensors t."""
    sh = c.sh
    kw = dict(max_rows=sh.max_rows, src_gen_stride=sh.src_gs, rec_row_stride=sh.rec_rs, rec_gen_stride=sh.rec_gs,
              out_row_stride=sh.out_rs, out_gen_stride=sh.out_gs, ids=d.ids, delivered=d.state,
              n_known=t["n_known"] if n_known else None)
    args = [d.src, d.off, d.len, d.rec, d.ri, d.nrec, d.st, d.slot, t["out"], t["out_len"], t["out_state"], t["n_out"],
            t["status"], sh.k, sh.e_max, sh.L]
    if c.sel is None:
        kw["G"] = c.G
        kw.update(over)
        qf.deliver_frames(*args, **kw)
    else:
        kw.update(n_max=c.G, G_src=c.G_src)
        kw.update(over)
        qf.deliver_frames_sel(d.sel, d.n_sel, *args, **kw)
    qf.default_context().sync()


def host(t, d):
    h = {key: _host(t[key]).copy() for key in KEYS}
    h["delivered"] = None if d.state is None else _body(d.state, d.state.numel() - GUARD, np.uint64).reshape(-1, R.WORDS)
    return h


def same(got, want, what, n_known=True):
    """Whole buffers (guards included) against the model's."""
    for key in KEYS:
        if key == "n_known" and not n_known:
            assert (got[key] == FILL).all()
            continue
        w = np.ascontiguousarray(want[key]).view(np.uint8).reshape(-1)
        bad = np.flatnonzero(got[key] != w)
        assert bad.size == 0, f"{what}: {key} differs at bytes {bad[:6].tolist()}"
    if want["delivered"] is None:
        assert got["delivered"] is None
    else:
        assert np.array_equal(got["delivered"], want["delivered"]), f"{what}: the state differs"


def against_model(qf, c, n_known=True, d=None):
    d = Dev(c) if d is None else d
    t = outputs(c.sh, c.G)
    launch(qf, c, d, t, n_known=n_known)
    d.unchanged()
    got = host(t, d)
    want = c.model(into=R.poisoned(c.sh, c.G, GUARD))
    same(got, want, "against the model", n_known)
    return got, want, d


# ---------------------------------------------------------------------------
# 1: the shape edges
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(shape_cases()))
def test_shapes_against_the_model(qf, gpu_ctx, name):
    c = shape_cases()[name]
    got, want, _ = against_model(qf, c)
    st = want["out_state"][: c.G * c.sh.k]
    assert (want["status"][: c.G] == OK).all() and (st == R.STORED).any()
    if name.startswith("k") and c.sh.k >= 64:
        assert (st == R.RECOVERED).any() and (st == R.EARLIER).any() and (st == R.UNKNOWN).any()
    if name.startswith("L"):
        lens = set(want["out_len"][: c.G * c.sh.k].tolist())
        assert {1, c.sh.L} <= lens
    if name == "slots_above_255":
        assert want["n_out"][:2].tolist() == [4, 1]


def test_no_n_known_and_no_state(qf, gpu_ctx):
    c = shape_cases()["k65"]
    against_model(qf, c, n_known=False)
    c.delivered, c.ids = None, None
    _, want, _ = against_model(qf, c)
    assert not (want["out_state"][: c.G * c.sh.k] == R.EARLIER).any()


# ---------------------------------------------------------------------------
# 2: the decode calls' outputs fed straight in
# ---------------------------------------------------------------------------
def _store(rng, k, Lb):
    """Eight stored generations: complete, partial, empty, one with a bad row."""
    gens = [D.complete_gen(rng, k, Lb, 5), D.determined_gen(rng, k, Lb, 10, 2, n_loose=1)[0], P.Gen(rng, k, Lb, []),
            D.determined_gen(rng, k, Lb, 12, 0, n_loose=2)[0], D.complete_gen(rng, k, Lb, 0),
            D.determined_gen(rng, k, Lb, 6, 4)[0], D.determined_gen(rng, k, Lb, 3, 1, n_dense=2)[0],
            D.complete_gen(rng, k, Lb, 3)]
    b = D.Batch(gens, mr=24)
    b.off[6, 2] += 8          # generation 6: the decode answers QF_EINVAL
    return b


def _decode(qf, b, dv, r, partial, sel=None, n_sel=None):
    """A decode call over the store -> its device outputs (passed on as they are) and the strides."""
    k, Lb, mr = b.k, b.L, b.mr
    em = min(k, r)
    G = b.G if sel is None else len(sel)
    rec_rs = _r16(Lb) + 16
    rec_gs = em * rec_rs + 48
    t = D._out_buffers(G, k, em, mr, rec_gs)
    kw = dict(max_rows=mr, src_gen_stride=b.gs, rec_row_stride=rec_rs, rec_gen_stride=rec_gs, n_rows=dv["n"],
              src_slot=t["slot"])
    args = (dv["src"], dv["off"], dv["len"], dv["idx"], dv["co"], t["rec"], t["ri"], t["nrec"], t["st"], k, r, Lb)
    if sel is None:
        (qf.decode_partial_frames if partial else qf.decode_frames)(*args, G=G, **kw)
    else:
        (qf.decode_partial_frames_sel if partial else qf.decode_frames_sel)(
            _dev(np.asarray(sel, np.uint32)), None if n_sel is None else _dev(np.array([n_sel], np.uint32)), *args,
            n_max=G, G_src=b.G, **kw)
    return t, R.Shape(k, em, Lb, mr, b.gs, rec_rs, rec_gs, _r16(Lb), k * _r16(Lb) + 16)


def _deliver_decoded(qf, b, dv, t, sh, sel=None, n_sel=None, ids=None, state=None):
    """deliver over a decode's device outputs -> host outputs, the model over the host copies of those outputs."""
    G = b.G if sel is None else len(sel)
    k, em = b.k, sh.e_max
    o = outputs(sh, G)
    t_state = None if state is None else SW._guarded(state)
    kw = dict(max_rows=sh.max_rows, src_gen_stride=sh.src_gs, rec_row_stride=sh.rec_rs, rec_gen_stride=sh.rec_gs,
              out_row_stride=sh.out_rs, out_gen_stride=sh.out_gs, ids=None if ids is None else _dev(ids),
              delivered=t_state, n_known=o["n_known"])
    args = (dv["src"], dv["off"], dv["len"], t["rec"], t["ri"], t["nrec"], t["st"], t["slot"], o["out"], o["out_len"],
            o["out_state"], o["n_out"], o["status"], k, em, b.L)
    if sel is None:
        qf.deliver_frames(*args, G=G, **kw)
    else:
        qf.deliver_frames_sel(_dev(np.asarray(sel, np.uint32)), None if n_sel is None else _dev(np.array([n_sel], np.uint32)),
                              *args, n_max=G, G_src=b.G, **kw)
    qf.default_context().sync()
    got = {key: _host(o[key]).copy() for key in KEYS}
    got["delivered"] = None if state is None else _body(t_state, 8 * state.size, np.uint64).reshape(-1, R.WORDS)
    dec = dict(rec=_host(t["rec"]), rec_index=_host(t["ri"], np.uint16)[: G * em].reshape(G, em),
               n_rec=_host(t["nrec"], np.uint32)[:G], dec_status=_host(t["st"], np.int32)[:G],
               src_slot=_host(t["slot"], np.uint16)[: G * k].reshape(G, k))
    c = R.Call(sh, G, b.src.reshape(-1), b.off, b.len, dec, ids=ids, delivered=state, sel=sel, n_sel=n_sel, G_src=b.G)
    want = c.model(into=R.poisoned(sh, G, GUARD))
    same(got, want, "over the decode's outputs")
    return got, want


@pytest.mark.parametrize("partial", [False, True], ids=["decode_frames_sel", "decode_partial_frames_sel"])
@pytest.mark.parametrize("count", [4, "null"])
def test_listed_decode_outputs_fed_straight_in(qf, gpu_ctx, partial, count):
    rng = np.random.default_rng(21)
    k, Lb, r = 16, 100, 8
    b = _store(rng, k, Lb)
    dv = b.device()
    sel = [0, 1, 6, 9, 3]      # complete, partial, QF_EINVAL from the decode, an invalid entry, unused (or listed)
    n_sel = None if count == "null" else count
    t, sh = _decode(qf, b, dv, r, partial, sel, n_sel)
    ids = np.array([100, 101, 106, 109, 103], np.uint64)
    got, want = _deliver_decoded(qf, b, dv, t, sh, sel, n_sel, ids=ids, state=np.zeros((b.G, R.WORDS), np.uint64))
    st = want["status"][:5].tolist()
    assert st == [OK, OK, ENOTREADY, EINVAL, ENOTREADY if n_sel == 4 else OK]
    n_out = want["n_out"][:5].tolist()
    assert n_out[0] == k and n_out[2:4] == [0, 0]
    # the partial decode reports what an incomplete generation holds; the full decode nothing
    assert n_out[1] == (12 if partial else 0) and n_out[4] == (0 if n_sel == 4 or not partial else 12)
    for i, data in want["packets"][0]:
        assert np.array_equal(np.frombuffer(data, np.uint8), b.gens[0].src[i][: len(data)])
        assert not b.gens[0].src[i][len(data):].any()
    assert np.array_equal(np.flatnonzero(want["delivered"][:, 0]), [0, 1] if partial and n_sel == 4 else
                          [0, 1, 3] if partial else [0])


def test_duplicates_without_a_state(qf, gpu_ctx):
    rng = np.random.default_rng(22)
    b = _store(rng, 16, 100)
    dv = b.device()
    sel = [1, 1, 0, 1]
    t, sh = _decode(qf, b, dv, 8, True, sel)
    got, want = _deliver_decoded(qf, b, dv, t, sh, sel)
    assert want["n_out"][:4].tolist() == [12, 12, 16, 12]
    assert np.array_equal(got["out"][: sh.out_gs], got["out"][3 * sh.out_gs: 4 * sh.out_gs])


@pytest.mark.parametrize("partial", [False, True])
def test_dense_decode_outputs(qf, gpu_ctx, partial):
    rng = np.random.default_rng(23)
    b = _store(rng, 16, 100)
    dv = b.device()
    t, sh = _decode(qf, b, dv, 8, partial)
    ids = np.arange(b.G, dtype=np.uint64) + np.uint64(7)
    got, want = _deliver_decoded(qf, b, dv, t, sh, ids=ids, state=np.zeros((b.G, R.WORDS), np.uint64))
    assert want["status"][:8].tolist() == [OK, OK, OK, OK, OK, OK, ENOTREADY, OK]
    assert [want["n_out"][g] for g in (0, 4, 7)] == [16, 16, 16] and (want["n_out"][1] > 0) == partial


# ---------------------------------------------------------------------------
# 3: the delivered state across calls
# ---------------------------------------------------------------------------
def _grown(rng, sh, G, first_specs):
    """The same generations with one further stored source and one further recovered source each."""
    specs = []
    for spec in first_specs:
        known = set(spec["stored"]) | set(spec["D"])
        free = [i for i in range(sh.k) if i not in known]
        used = {s for s, _ in spec["stored"].values()}
        slot = next(s for s in range(sh.max_rows) if s not in used)
        stored = dict(spec["stored"])
        stored[free[0]] = (slot, 5)
        specs.append(dict(stored=stored, D=spec["D"] + [free[1]], status=ENOTREADY))
    return specs


def test_a_second_call_and_later_rows(qf, gpu_ctx):
    rng = np.random.default_rng(31)
    sh = R.simple_shape(70, 4, 40, 80)
    G = 4
    first = [dict(stored={i: (79 - i, 40 - i % 3) for i in range(g, 70, 7)}, D=[1 + g + 7 * m for m in range(2)],
                  status=ENOTREADY) for g in range(G)]
    c = R.synth(rng, sh, first)
    c.ids = np.array([900, 901, 902, 903], np.uint64)
    c.delivered = np.zeros((G, R.WORDS), np.uint64)
    got1, want1, d = against_model(qf, c)
    assert (want1["n_out"][:G] == 12).all()
    # the same inputs again: nothing leaves, out and the state stay as they are
    c.delivered = want1["delivered"]
    got2, want2, _ = against_model(qf, c, d=d)
    assert not want2["n_out"][:G].any() and (want2["n_known"][:G] == 12).all()
    assert set(want2["out_state"][: G * 70].tolist()) == {R.UNKNOWN, R.EARLIER}
    assert (got2["out"] == FILL).all() and np.array_equal(got2["delivered"], got1["delivered"])
    # more rows arrive: only the new sources leave
    c3 = R.synth(rng, sh, _grown(rng, sh, G, first))
    c3.ids, c3.delivered = c.ids, want1["delivered"]
    _, want3, _ = against_model(qf, c3)
    assert (want3["n_out"][:G] == 2).all() and (want3["n_known"][:G] == 14).all()
    # a changed id restarts the mask of that slot
    c3.ids = np.array([900, 905, 902, 903], np.uint64)
    _, want4, _ = against_model(qf, c3)
    assert want4["n_out"][:G].tolist() == [2, 14, 2, 2] and int(want4["delivered"][1, 0]) == 906
    # no ids: the tag word is neither read nor written, the caller zeroes a reset generation's words
    c3.ids = None
    c3.delivered = want1["delivered"].copy()
    c3.delivered[2] = 0
    c3.delivered[3, 0] = 12345
    _, want5, _ = against_model(qf, c3)
    assert want5["n_out"][:G].tolist() == [2, 2, 14, 2] and want5["delivered"][:, 0].tolist() == [901, 902, 0, 12345]


def test_bad_ids(qf, gpu_ctx):
    c = R.inconsistent_call("none")
    c.ids = np.array([(1 << 64) - 1, 1 << 62, (1 << 62) - 1], np.uint64)
    _, want, _ = against_model(qf, c)
    assert want["status"][:3].tolist() == [EINVAL, EINVAL, OK] and not want["delivered"][:2].any()


# ---------------------------------------------------------------------------
# 4: inconsistent inputs
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("what", R.INCONSISTENT)
def test_inconsistent_inputs(qf, gpu_ctx, what):
    c = R.inconsistent_call(what)
    _, want, _ = against_model(qf, c)
    assert want["status"][:3].tolist() == [OK, EINVAL, OK] and want["n_out"][:3].tolist() == [4, 0, 4]
    assert not want["delivered"][1].any()
    # the same through a list
    c.sel, c.n_sel, c.G_src = [2, 1, 0], None, 3
    c.ids = np.array([7, 6, 5], np.uint64)
    d = c.dec
    for key in ("rec_index", "n_rec", "dec_status", "src_slot"):
        d[key] = d[key][::-1].copy()
    d["rec"] = d["rec"].reshape(3, -1)[::-1].copy().reshape(-1)
    _, want, _ = against_model(qf, c)
    assert want["status"][:3].tolist() == [OK, EINVAL, OK]


# ---------------------------------------------------------------------------
# 5: the copy's grid bound, determinism
# ---------------------------------------------------------------------------
def test_more_quads_than_waves(qf, gpu_ctx):
    """More entries than the copy launches waves for (k = 4: one quad per entry), so the waves stride;
    sized at BOUND_MARGIN times the bound, so raising the bound a little does not empty the case."""
    import torch

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    G = BOUND_MARGIN * cus * GROUPS_PER_CU * 4 + 101
    rng = np.random.default_rng(41)
    sh = R.Shape(4, 1, 16, 4, 64, 16, 16, 16, 64)
    specs = [dict(stored={i: ((i + g) % 4, 16 if (g + i) % 5 else 3) for i in range(4) if (g >> i) & 1 or g % 16 == 0},
                  D=[g % 4] if not ((g >> (g % 4)) & 1 or g % 16 == 0) else [], status=ENOTREADY) for g in range(G)]
    c = R.synth(rng, sh, specs)
    _, want, _ = against_model(qf, c)
    assert want["n_out"][G - 101: G].sum() > 100


def test_two_runs_give_identical_bytes(qf, gpu_ctx):
    c = shape_cases()["k129"]
    a, _, _ = against_model(qf, c)
    b, _, _ = against_model(qf, c)
    for key in KEYS:
        assert np.array_equal(a[key], b[key]), key
    assert np.array_equal(a["delivered"], b["delivered"])


# ---------------------------------------------------------------------------
# 6: call-level QF_EINVAL, G == 0, profile names
# ---------------------------------------------------------------------------
def test_call_level_einval(qf, gpu_ctx):
    """Every refusal of the two calls, through the C ABI as it is (the Python
    wrappers check buffer sizes first).  No refused call writes anything."""
    import ctypes

    import torch

    c = R.inconsistent_call("none")
    sh = c.sh
    d = Dev(c)
    t = outputs(sh, c.G)
    lib = qf.L._lib()
    fields = dict(k=sh.k, e_max=sh.e_max, L=sh.L, max_rows=sh.max_rows, flags=0, reserved=0, src_gen_stride=sh.src_gs,
                  rec_row_stride=sh.rec_rs, rec_gen_stride=sh.rec_gs, out_row_stride=sh.out_rs, out_gen_stride=sh.out_gs)
    ptrs = dict(src=d.src, row_off=d.off, row_len=d.len, rec=d.rec, rec_index=d.ri, n_rec=d.nrec, dec_status=d.st,
                src_slot=d.slot, ids=d.ids, delivered=d.state, out=t["out"], out_len=t["out_len"],
                out_state=t["out_state"], n_out=t["n_out"], n_known=t["n_known"], status=t["status"])
    t_sel = _dev(np.array([2, 0, 1], np.uint32))

    def raw(G=c.G, sel="dense", shape=True, **over):
        f = dict(fields)
        f.update({key: v for key, v in over.items() if key in f})
        p = dict(ptrs)
        p.update({key: v for key, v in over.items() if key in p})
        s = qf.L.DeliverShape(*f.values())
        args = [None if x is None else x.data_ptr() for x in p.values()]
        ctx = qf.default_context().handle
        if isinstance(sel, str):
            return lib.qf_deliver_frames_dev(ctx, ctypes.byref(s) if shape else None, G, *args)
        return lib.qf_deliver_frames_sel_dev(ctx, ctypes.byref(s) if shape else None,
                                             None if sel is None else ctypes.byref(sel), *args)

    def off(x, by):
        """x at an offset of `by` bytes in a buffer that is long enough."""
        return torch.cat([x, torch.zeros(64, dtype=torch.uint8, device="cuda")])[by:]

    bad = dict(k=0, e_max=129, L=0, max_rows=0, flags=1, reserved=1)
    for key, v in bad.items():
        assert raw(**{key: v}) == EINVAL, key
    assert raw(k=257) == EINVAL and raw(max_rows=1025) == EINVAL and raw(G=(1 << 24) + 1) == EINVAL
    for key in ("src_gen_stride", "rec_row_stride", "rec_gen_stride", "out_row_stride", "out_gen_stride"):
        assert raw(**{key: fields[key] + 8}) == EINVAL, key
    assert raw(rec_row_stride=16) == EINVAL and raw(out_row_stride=16) == EINVAL
    assert raw(out_gen_stride=sh.k * sh.out_rs - 16) == EINVAL and raw(shape=False) == EINVAL
    nullable = ("ids", "delivered", "n_known")
    for key in ptrs:
        if key not in nullable:
            assert raw(**{key: None}) == EINVAL, key
    for key in ("src", "rec", "out"):
        assert raw(**{key: off(ptrs[key], 8)}) == EINVAL, key
    assert raw(delivered=off(d.state, 4)) == EINVAL
    # the list's rules
    gs = qf.L.GenSel(t_sel.data_ptr(), None, 3, 3)
    for sel in (None, qf.L.GenSel(None, None, 3, 3), qf.L.GenSel(t_sel.data_ptr(), None, 0, 3),
                qf.L.GenSel(t_sel.data_ptr(), None, 3, 0)):
        assert raw(sel=sel) == EINVAL
    # G == 0 is QF_OK; nothing was written by any of these calls
    assert raw(G=0) == OK
    qf.default_context().sync()
    for key in KEYS:
        assert (_host(t[key]) == FILL).all(), key
    assert not _host(d.state)[: 8 * 3 * R.WORDS].any()
    # the three nullable pointers, one at a time and together; rec and rec_index may be NULL when e_max is 0
    for key in nullable:
        assert raw(**{key: None}) == OK, key
    assert raw(ids=None, delivered=None, n_known=None) == OK
    assert raw(e_max=0, rec=None, rec_index=None, n_rec=_dev(np.zeros(3, np.uint32))) == OK
    assert raw(sel=gs) == OK
    qf.default_context().sync()
    against_model(qf, c)


def test_profile_names(qf, gpu_ctx):
    c = R.inconsistent_call("none")
    gpu_ctx.sync()
    gpu_ctx.profile(True)
    against_model(qf, c)
    dense = gpu_ctx.kernel_times()
    gpu_ctx.profile(False)
    assert set(dense) == {"k_deliver_prepare", "k_deliver_rows"}, dense
    c.sel, c.G_src = [0, 1, 2], 3
    gpu_ctx.profile(True)
    against_model(qf, c)
    listed = gpu_ctx.kernel_times()
    gpu_ctx.profile(False)
    assert set(listed) == {"k_deliver_prepare_sel", "k_deliver_rows_sel"}, listed


# ---------------------------------------------------------------------------
# 7: the loop of INTEGRATION.md with deliver steps 1b and 7a
# ---------------------------------------------------------------------------
def test_the_loop_delivers_every_determined_source_once(qf, oracle, gpu_ctx):
    import torch

    k, r, Lb, G, N, mr = R.K_LOOP, R.R_LOOP, R.L_LOOP, R.G_LOOP, R.N_LOOP, R.MR_LOOP
    sh = R.loop_shape()
    em = sh.e_max
    src, stream, polls, last, stats = R.loop_model()
    rc = T.Receiver(qf, G, k, Lb, k, 0)
    assert (rc.gs, rc.rs) == (sh.src_gs, sh.out_rs)
    seen = torch.zeros(G, dtype=torch.int32, device="cuda")
    t_win = SW._guarded(np.zeros(G, np.uint64))
    t_state = SW._guarded(np.zeros((G, R.WORDS), np.uint64))
    fs = PR.payload_offset(k) + _r16(Lb)
    left = {}

    def decode_over(t_sel, t_nsel, partial):
        t = D._out_buffers(G, k, em, k, sh.rec_gs)
        (qf.decode_partial_frames_sel if partial else qf.decode_frames_sel)(
            t_sel, t_nsel, rc.bytes, rc.off, rc.len, rc.index, rc.coeffs, t["rec"], t["ri"], t["nrec"], t["st"], k, r, Lb,
            n_max=G, G_src=G, max_rows=k, src_gen_stride=rc.gs, rec_row_stride=sh.rec_rs, rec_gen_stride=sh.rec_gs,
            n_rows=rc.n, src_slot=t["slot"])
        return t

    def deliver_over(step, t_sel, t_nsel, t, t_ids, what):
        """The deliver call over a decode's device outputs, against the model's step."""
        o = outputs(sh, G)
        qf.deliver_frames_sel(t_sel, t_nsel, rc.bytes, rc.off, rc.len, t["rec"], t["ri"], t["nrec"], t["st"], t["slot"],
                              o["out"], o["out_len"], o["out_state"], o["n_out"], o["status"], k, em, Lb, n_max=G, G_src=G,
                              max_rows=k, src_gen_stride=rc.gs, rec_row_stride=sh.rec_rs, rec_gen_stride=sh.rec_gs,
                              out_row_stride=sh.out_rs, out_gen_stride=sh.out_gs, ids=t_ids, delivered=t_state,
                              n_known=o["n_known"])
        qf.default_context().sync()
        got = {key: _body(o[key], o[key].numel() - GUARD) for key in KEYS}
        for key in KEYS:
            want = np.ascontiguousarray(step.res[key]).view(np.uint8).reshape(-1)
            bad = np.flatnonzero(got[key] != want)
            assert bad.size == 0, f"{what}: {key} differs from the model at bytes {bad[:6].tolist()}"
        assert np.array_equal(_body(t_state, 8 * G * R.WORDS, np.uint64).reshape(G, R.WORDS), step.res["delivered"]), what
        lens, state = got["out_len"].view(np.uint32), got["out_state"]
        for j, (s, g) in enumerate(step.listed):
            for i in range(k):
                if state[j * k + i] in (R.STORED, R.RECOVERED):
                    assert (g, i) not in left, f"{what}: source {i} of generation {g} left twice"
                    at = j * sh.out_gs + i * sh.out_rs
                    left[(g, i)] = got["out"][at: at + int(lens[j * k + i])].tobytes()

    for poll, q in enumerate(polls):
        n = len(q.take)
        # 1: the window; 1a: the partial decode over the evict list; 1b: deliver, with evict_id as the ids
        d, h = SW.run_window(qf, None, q.ids, n, G, G, t_win=t_win)
        SW.check_window(h, q.w)
        t = decode_over(d["esel"], d["nev"], True)
        deliver_over(q.evict, d["esel"], d["nev"], t, d["eid"][: 8 * G], f"poll {poll}, step 1b")
        qf.stream_reset(d["esel"], d["nev"], k, n_max=G, G_src=G, state=rc.state, store_n=rc.n, seen=seen)
        qf.stream_reset(d["esel"], d["nev"], k, n_max=G, G_src=G, seen=rc.rank)
        # 2 .. 5: the ingest, the listed update and append
        p = PR.Poll(k, Lb, N, fs)
        for f, (g, (i, v)) in enumerate(q.take):
            if i < k:
                p.put_sys(f, 0, k * (g + 1) + i, q.rows[f])
            else:
                p.put_coded(f, 0, 5000 + i, v, q.rows[f])
        p.gen[:] = q.w.frame_gen
        fp = T.FlatPoll(p, n)
        fp.gen = d["gen"][: 4 * N]
        di, hi = T.run_ingest(qf, fp, G, G, mr)
        T.check_against_reference(hi, PR.ingest(p, n, G, G, mr))
        _, _, st, ast = rc.listed_poll(di["sel"], di["n_sel"], G, di, mr, fp.frames, N * fs, rank_sel=False)
        assert (st == T.OK).all() and (ast == T.OK).all()
        # 6, 7: select and the full decode; 8: close, which writes the ids; 7a: deliver; 9: the two resets
        t_sel, t_nsel, t_ids = _filled(4 * G + GUARD), _filled(4 + GUARD), _filled(8 * G + GUARD)
        qf.gen_select(rc.rank, t_sel, t_nsel, G=G, min_rank=k, n_max=G, seen=seen, mark=True)
        t = decode_over(t_sel, t_nsel, False)
        qf.gen_window_sel(t_sel, t_nsel, t_win, n_max=G, G_src=G, ids=t_ids, close=True)
        qf.default_context().sync()
        n_done = int(_body(t_nsel, 4, np.uint32)[0])
        assert _body(t_sel, 4 * G, np.uint32)[:n_done].tolist() == q.done.sel, poll
        deliver_over(q.done, t_sel, t_nsel, t, t_ids[: 8 * G], f"poll {poll}, step 7a")
        qf.stream_reset(t_sel, t_nsel, k, n_max=G, G_src=G, state=rc.state, store_n=rc.n, seen=seen)
        qf.stream_reset(t_sel, t_nsel, k, n_max=G, G_src=G, seen=rc.rank)
        qf.default_context().sync()
        assert np.array_equal(_body(t_win, 8 * G, np.uint64), q.win_after), poll
        # a deadline flush: every slot that holds a row, nothing is reset or closed
        for step in ([q.flush] if q.flush is not None else []) + ([last.flush] if poll == len(polls) - 1 else []):
            t_sel, t_nsel, t_ids = _filled(4 * G + GUARD), _filled(4 + GUARD), _filled(8 * G + GUARD)
            qf.gen_select(rc.rank, t_sel, t_nsel, G=G, min_rank=1, n_max=G)
            t = decode_over(t_sel, t_nsel, True)
            qf.gen_window_sel(t_sel, t_nsel, t_win, n_max=G, G_src=G, ids=t_ids)
            qf.default_context().sync()
            assert _body(t_sel, 4 * G, np.uint32)[: int(_body(t_nsel, 4, np.uint32)[0])].tolist() == step.sel, poll
            deliver_over(step, t_sel, t_nsel, t, t_ids[: 8 * G], f"poll {poll}, flush")
    R.check_exactly_once(src, left, stats["determined"])
    R.check_loop_stats(stats)
