"""The partial decode on the MI355X: qf_decode_partial_frames_dev and its
listed form against tests/partial_ref.py, against qf_decode_frames_dev on
complete generations, and in the streaming loop in front of the resets of the
displaced generations.

Every output buffer starts as 0xCC and is compared byte for byte with a buffer
built from the model, so the bytes a call must not write are checked too.  The
truth for payloads is the generated sources.  Every byte of a source region
outside the rows is 0xCC, so a kernel that reads a row past its length changes
an output byte."""
import numpy as np
import pytest

from tests import partial_ref as P
from tests import poll_ref as PR
from tests import test_gpu_poll_ingest as T
from tests import test_gpu_stream_window as SW
from tests import window_ref as WR

pytestmark = pytest.mark.gpu

FILL, GUARD, NONE16 = T.FILL, T.GUARD, T.NONE16
OK, EINVAL, ENOTREADY = 0, -1, -3
_r16, _dev, _filled, _host = T._r16, T._dev, T._filled, T._host


# ---------------------------------------------------------------------------
# a batch of generations where they lie, the calls, the expected buffers
# ---------------------------------------------------------------------------
class Batch:
    """Generations (partial_ref.Gen, one k and L) as the calls take them: slot s
    of a generation lies at offset (mr - 1 - s) * rs of its region (so the
    arrival order is not the address order), 0xCC around every row and in the
    metadata of the slots at and above n."""

    def __init__(self, gens, mr=None, full_len=False):
        self.gens, self.G = gens, len(gens)
        self.k, self.L = gens[0].k, gens[0].L
        self.mr = mr = max(max(len(g.idx) for g in gens), 1) if mr is None else mr
        self.rs = _r16(self.L) + 16
        self.gs = mr * self.rs + 32
        G, k = self.G, self.k
        self.src = np.full((G, self.gs), FILL, np.uint8)
        self.off = np.full((G, mr), 0xCCCCCCCC, np.uint32)
        self.len = np.full((G, mr), 0xCCCCCCCC, np.uint32)
        self.idx = np.full((G, mr), 0xCCCC, np.uint16)
        self.co = np.full((G, mr, k), FILL, np.uint8)
        self.n = np.array([g.n for g in gens], np.uint32)
        for j, g in enumerate(gens):
            m = len(g.idx)
            assert m <= mr and (g.k, g.L) == (k, self.L)
            for s in range(m):
                ln = self.L if full_len else int(g.lens[s])
                self.off[j, s], self.len[j, s] = (mr - 1 - s) * self.rs, ln
                self.src[j, self.off[j, s]: self.off[j, s] + ln] = g.rows[s, :ln]
            self.idx[j, :m], self.co[j, :m] = g.idx, g.coeffs

    def refs(self, r):
        out = []
        for j, g in enumerate(self.gens):
            n = int(self.n[j])
            pay = []
            for s in range(n):
                ln = int(self.len[j, s])
                pay.append(g.rows[s, :ln].tobytes() if ln <= self.L else bytes(ln))
            ref = P.partial_ref(self.k, r, self.L, self.idx[j, :n], self.co[j, :n], pay, self.off[j, :n], self.gs)
            P.check_records(ref, self.off[j], self.len[j], self.gs)
            out.append(ref)
        return out

    def device(self):
        return dict(src=_dev(self.src), off=_dev(self.off), len=_dev(self.len), idx=_dev(self.idx), co=_dev(self.co),
                    n=_dev(self.n))


def _out_buffers(G, k, em, mr, rec_gs):
    return dict(rec=_filled(G * rec_gs + GUARD), ri=_filled(2 * G * em + GUARD), nrec=_filled(4 * G + GUARD),
                st=_filled(4 * G + GUARD), rank=_filled(4 * G + GUARD), flags=_filled(G * mr + GUARD),
                slot=_filled(2 * G * k + GUARD))


KEYS = ("rec", "ri", "nrec", "st", "rank", "flags", "slot")


def run(qf, b, r, *, partial=True, dev=None, sel=None, n_sel=None, G_src=None, with_n=True):
    """One call -> the seven raw output buffers on the host.  sel: the listed
    form over b as the source arrays (sel a host list, n_sel a count or None)."""
    k, Lb, mr = b.k, b.L, b.mr
    em = min(k, r)
    G = b.G if sel is None else len(sel)
    rec_rs = _r16(Lb) + 16
    rec_gs = em * rec_rs + 48
    d = b.device() if dev is None else dev
    t = _out_buffers(G, k, em, mr, rec_gs)
    kw = dict(max_rows=mr, src_gen_stride=b.gs, rec_row_stride=rec_rs, rec_gen_stride=rec_gs,
              n_rows=d["n"] if with_n else None, rank=t["rank"], innovative=t["flags"], src_slot=t["slot"])
    args = (d["src"], d["off"], d["len"], d["idx"], d["co"], t["rec"], t["ri"], t["nrec"], t["st"], k, r, Lb)
    if sel is None:
        (qf.decode_partial_frames if partial else qf.decode_frames)(*args, G=G, **kw)
    else:
        t_sel = _dev(np.asarray(sel, np.uint32))
        t_n = None if n_sel is None else _dev(np.array([n_sel], np.uint32))
        (qf.decode_partial_frames_sel if partial else qf.decode_frames_sel)(t_sel, t_n, *args, n_max=G,
                                                                            G_src=b.G if G_src is None else G_src, **kw)
    qf.default_context().sync()
    assert np.array_equal(_host(d["src"]), b.src.reshape(-1)), "the source was written"
    return {key: _host(t[key]).copy() for key in KEYS}, (rec_rs, rec_gs)


def expected(refs, k, r, Lb, mr, rec_rs, rec_gs):
    """The seven buffers as the model says they must be, 0xCC where nothing is written."""
    G, em = len(refs), min(k, r)
    rec = np.full(G * rec_gs + GUARD, FILL, np.uint8)
    ri = np.full(G * em + GUARD // 2, 0xCCCC, np.uint16)
    nrec = np.full(G + GUARD // 4, 0xCCCCCCCC, np.uint32)
    st = np.full(G + GUARD // 4, 0xCCCCCCCC, np.uint32).view(np.int32)
    rank = np.full(G + GUARD // 4, 0xCCCCCCCC, np.uint32)
    flags = np.full(G * mr + GUARD, FILL, np.uint8)
    slot = np.full(G * k + GUARD // 2, 0xCCCC, np.uint16)
    for g, ref in enumerate(refs):
        for m, i in enumerate(ref["D"]):
            rec[g * rec_gs + m * rec_rs: g * rec_gs + m * rec_rs + Lb] = ref["rec"][m]
            ri[g * em + m] = i
        nrec[g], st[g], rank[g] = len(ref["D"]), ref["status"], ref["rank"]
        flags[g * mr: (g + 1) * mr] = 0
        flags[g * mr: g * mr + len(ref["flags"])] = ref["flags"]
        slot[g * k: (g + 1) * k] = ref["src_slot"]
    return dict(rec=rec, ri=ri.view(np.uint8), nrec=nrec.view(np.uint8), st=st.view(np.uint8), rank=rank.view(np.uint8),
                flags=flags, slot=slot.view(np.uint8))


def same(got, want, what):
    for key in KEYS:
        bad = np.flatnonzero(got[key] != want[key])
        assert bad.size == 0, f"{what}: {key} differs at bytes {bad[:6].tolist()}"


def against_model(qf, b, r, **kw):
    """The call against the model byte for byte, and the delivered rows against the sources."""
    got, (rec_rs, rec_gs) = run(qf, b, r, **kw)
    refs = b.refs(r)
    same(got, expected(refs, b.k, r, b.L, b.mr, rec_rs, rec_gs), "against the model")
    for g, ref in zip(b.gens, refs):
        assert np.array_equal(ref["rec"], g.src[ref["D"]]), "the model's rows are not the sources"
    return refs


def sys_rows(k, S):
    return [P.unit(k, i) for i in S]


def complete_gen(rng, k, Lb, e):
    """A generation of rank k: the systematic rows of all but e sources, some of
    them twice, e + 2 dense coded rows and a dependent one, in a random order."""
    E = sorted(rng.choice(k, e, replace=False).tolist())
    vecs = sys_rows(k, [i for i in range(k) if i not in E])
    vecs += [vecs[int(rng.integers(0, len(vecs)))] for _ in range(2)] if vecs else []
    coded = [rng.integers(1, 256, k, dtype=np.uint8) for _ in range(e + 2 if e else 0)]
    if len(coded) >= 2:
        coded.append(P.mul_table()[7][coded[0]] ^ coded[1])
    vecs += coded
    order = rng.permutation(len(vecs))
    return P.Gen(rng, k, Lb, [vecs[i] for i in order])


# ---------------------------------------------------------------------------
# 1: complete generations against the existing call
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("Lb", [16, 100])
@pytest.mark.parametrize("k", [1, 5, 16, 64, 65, 130])
def test_complete_generations_equal_the_full_decode(qf, gpu_ctx, k, Lb):
    rng = np.random.default_rng(1000 * k + Lb)
    r = min(k, 20)
    G = 3 if k >= 64 else 6
    # (a coded row that arrives first makes a later systematic row redundant: up to e + 3 recovered rows)
    e_top = r if r == k else r - 3
    gens = [complete_gen(rng, k, Lb, int(rng.integers(0, e_top + 1)) if j else e_top) for j in range(G)]
    b = Batch(gens)
    dev = b.device()
    part, _ = run(qf, b, r, dev=dev)
    full, _ = run(qf, b, r, dev=dev, partial=False)
    same(part, full, "against qf_decode_frames_dev")
    refs = against_model(qf, b, r, dev=dev)
    assert all(ref["status"] == OK and ref["rank"] == k for ref in refs)
    assert any(ref["D"] for ref in refs) and any(not f.all() for f in (ref["flags"] for ref in refs) if len(f))


# ---------------------------------------------------------------------------
# 2: planted incomplete generations
# ---------------------------------------------------------------------------
def test_planted_incomplete_generations(qf, gpu_ctx):
    k, Lb = 16, 100
    rng = np.random.default_rng(5)
    cases = P.planted(rng, k)
    b = Batch([P.Gen(rng, k, Lb, vecs) for vecs, _, _ in cases.values()])
    refs = against_model(qf, b, k)
    for (name, (_, det, undet)), ref in zip(cases.items(), refs):
        assert ref["D"] == det and not set(undet) & set(ref["D"]), name
        assert ref["status"] == ENOTREADY, name
    by = dict(zip(cases, refs))
    assert by["no rows"]["rank"] == 0
    only = by["systematic rows only"]
    assert only["bound"] == 0 and (only["src_slot"] != NONE16).sum() == 12
    late = by["systematic row after the rows that determine it"]
    assert late["src_slot"][3] == NONE16 and not late["flags"][-1]


# ---------------------------------------------------------------------------
# 3: the boundaries the kernel loops over
# ---------------------------------------------------------------------------
def determined_gen(rng, k, Lb, n_sys, n_det, n_loose=0, n_dense=0):
    """n_sys systematic rows, n_det coded rows over S and one further source
    each, n_loose over S and two further sources each (these determine
    nothing), n_dense dense rows; coded rows first, then a shuffle of the rest."""
    S = list(range(0, 2 * n_sys, 2))[:n_sys] if 2 * n_sys <= k else list(range(n_sys))
    rest = [i for i in range(k) if i not in S]
    coded = [P.over(rng, k, S[: 1 + (7 * t) % max(len(S), 1)] + [rest[t]]) for t in range(n_det)]
    coded += [P.over(rng, k, S[:3] + rest[n_det + 2 * t: n_det + 2 * t + 2]) for t in range(n_loose)]
    coded += [rng.integers(1, 256, k, dtype=np.uint8) for _ in range(n_dense)]
    vecs = coded[: len(coded) // 2] + sys_rows(k, S) + coded[len(coded) // 2:]
    return P.Gen(rng, k, Lb, vecs), [rest[t] for t in range(n_det)]


@pytest.mark.parametrize("k", [64, 65])
def test_lane_loop_edge(qf, gpu_ctx, k):
    rng = np.random.default_rng(k)
    pairs = [determined_gen(rng, k, 100, k - 20, 6, n_loose=4), determined_gen(rng, k, 100, k - 1, 1),
             determined_gen(rng, k, 100, 0, 0, n_dense=k - 1), determined_gen(rng, k, 100, k - 9, 3, n_loose=3)]
    refs = against_model(qf, Batch([g for g, _ in pairs]), 16)
    for ref, (_, det) in zip(refs, pairs):
        assert ref["D"] == det
    assert refs[1]["status"] == OK and all(ref["status"] == ENOTREADY for ref in refs[:1] + refs[2:])


@pytest.mark.parametrize("nd", [16, 17])
def test_pass_edge(qf, gpu_ctx, nd):
    rng = np.random.default_rng(nd)
    pairs = [determined_gen(rng, 64, 100, 40, nd, n_loose=2), determined_gen(rng, 64, 100, 40, 3)]
    refs = against_model(qf, Batch([g for g, _ in pairs]), 32)
    assert len(refs[0]["D"]) == nd and len(refs[1]["D"]) == 3


def test_more_than_128_unknown_columns(qf, gpu_ctx):
    rng = np.random.default_rng(200)
    g, det = determined_gen(rng, 200, 48, 60, 4, n_loose=2, n_dense=4)
    assert len(g.idx) == 70
    refs = against_model(qf, Batch([g]), 16)
    assert refs[0]["D"] == det and refs[0]["rank"] == 70 and refs[0]["status"] == ENOTREADY


def test_more_coded_rows_than_matrix_rows(qf, gpu_ctx):
    rng = np.random.default_rng(129)
    k = 200
    a = P.Gen(rng, k, 16, [rng.integers(1, 256, k, dtype=np.uint8) for _ in range(129)])
    b128 = P.Gen(rng, k, 16, [rng.integers(1, 256, k, dtype=np.uint8) for _ in range(128)])
    refs = against_model(qf, Batch([a, b128]), 16)
    assert refs[0]["status"] == EINVAL and refs[0]["rank"] == 129
    assert refs[1]["status"] == ENOTREADY and refs[1]["rank"] == 128 and refs[1]["D"] == []


def test_more_determined_sources_than_the_capacity(qf, gpu_ctx):
    rng = np.random.default_rng(3)
    r = 2
    over_cap, _ = determined_gen(rng, 16, 100, 10, r + 1)
    at_cap, det = determined_gen(rng, 16, 100, 10, r)
    refs = against_model(qf, Batch([over_cap, at_cap]), r)
    assert refs[0]["status"] == EINVAL and refs[0]["D"] == [] and refs[0]["rank"] == 13
    assert refs[1]["status"] == ENOTREADY and refs[1]["D"] == det


def test_full_and_ragged_payload_paths(qf, gpu_ctx):
    """L = 112 with every row at its full length: whole waves of the payload
    pass take the path without masks; the same generations at their own
    lengths take the ragged one."""
    rng = np.random.default_rng(112)
    gens = [determined_gen(rng, 16, 112, 10, 1 + j % 4, n_loose=1)[0] for j in range(24)]
    for full_len in (True, False):
        refs = Batch(gens, full_len=full_len).refs(16)
        short = sum(ref["min_len"] < 112 for ref in refs)
        assert short == 0 if full_len else short >= 12
        against_model(qf, Batch(gens, full_len=full_len), 16)


def test_rows_of_length_zero(qf, gpu_ctx):
    rng = np.random.default_rng(8)
    k, Lb = 16, 100
    src = rng.integers(1, 256, (k, Lb), dtype=np.uint8)
    src[2] = 0
    S = list(range(10))
    vecs = sys_rows(k, S) + [P.over(rng, k, [1, 2, 12]), P.over(rng, k, [2, 13])]
    g = P.Gen(rng, k, Lb, vecs, src=src)
    assert g.lens[2] == 0
    zero = P.Gen(rng, k, Lb, sys_rows(k, [4]) + [P.over(rng, k, [4, 5])], src=np.zeros((k, Lb), np.uint8))
    assert zero.lens[1] == 0
    refs = against_model(qf, Batch([g, zero]), k)
    assert refs[0]["D"] == [12, 13] and refs[0]["min_len"] == 0 and 2 in refs[0]["recorded"]
    assert refs[1]["D"] == [5] and refs[1]["min_len"] == 0


def test_many_slots_few_innovative(qf, gpu_ctx):
    rng = np.random.default_rng(290)
    k, Lb = 16, 40
    S = list(range(9))
    mul = P.mul_table()
    base = sys_rows(k, S) + [P.over(rng, k, S + [9, 10])]
    vecs = list(base)
    while len(vecs) < 283:
        a, c = base[int(rng.integers(0, len(base)))], base[int(rng.integers(0, len(base)))]
        vecs.append(a if rng.integers(0, 2) else (mul[int(rng.integers(1, 256))][a] ^ c).astype(np.uint8))
    vecs += [P.over(rng, k, S[:4] + [9, 10]), P.unit(k, 9), P.over(rng, k, [3, 11])]
    vecs += [vecs[int(rng.integers(0, len(vecs)))] for _ in range(290 - len(vecs))]
    g = P.Gen(rng, k, Lb, vecs)
    assert len(g.idx) == 290
    refs = against_model(qf, Batch([g, complete_gen(rng, k, Lb, 4)], mr=300), k)
    assert refs[0]["D"] == [9, 10, 11] and refs[0]["rank"] == 12 and refs[0]["flags"].sum() == 12


# ---------------------------------------------------------------------------
# 4: bad rows
# ---------------------------------------------------------------------------
def test_bad_rows(qf, gpu_ctx):
    rng = np.random.default_rng(4)
    k, Lb = 16, 100
    gens = [determined_gen(rng, k, Lb, 10, 2)[0] for _ in range(4)]
    b = Batch(gens)
    b.off[0, 3] += 8                              # an unaligned offset
    b.len[1, 5] = Lb + 1                          # a row longer than L
    b.off[2, 11], b.len[2, 11] = b.gs - 16, 17    # a row past the region
    refs = against_model(qf, b, k)
    for ref in refs[:3]:
        assert ref["status"] == EINVAL and ref["rank"] == 12 and ref["flags"].sum() == 12
        assert (ref["src_slot"] == NONE16).all() and ref["D"] == []
    assert refs[3]["status"] == ENOTREADY and len(refs[3]["D"]) == 2


# ---------------------------------------------------------------------------
# 5: the listed form
# ---------------------------------------------------------------------------
def _invalid_entry(rng, k, Lb):
    """What k_sel_gather makes of an invalid entry: one slot of index 0xFFFF and length 0."""
    g = P.Gen(rng, k, Lb, [P.unit(k, 0)])
    g.idx[0], g.coeffs[0], g.rows[0], g.lens[0] = 0xFFFF, 0, 0, 0
    return g


@pytest.mark.parametrize("count", ["null", 6, 0, 99])
def test_listed_form_equals_the_dense_call(qf, gpu_ctx, count):
    rng = np.random.default_rng(55)
    k, Lb, r = 16, 100, 8
    store = [determined_gen(rng, k, Lb, 10, 2, n_loose=1)[0], complete_gen(rng, k, Lb, 5), P.Gen(rng, k, Lb, []),
             determined_gen(rng, k, Lb, 12, 0, n_loose=2)[0], complete_gen(rng, k, Lb, 0),
             determined_gen(rng, k, Lb, 6, 4)[0], determined_gen(rng, k, Lb, 3, 1, n_dense=2)[0]]
    mr = 24
    src = Batch(store, mr=mr)
    sel = [3, 3, 9, 0, 6, 2, 5, 1]               # a duplicate, an invalid entry (>= G_src)
    n = len(sel) if count == "null" else min(count, len(sel))
    unused = P.Gen(rng, k, Lb, [])
    gathered = Batch([(store[s] if s < len(store) else _invalid_entry(rng, k, Lb)) if j < n else unused
                      for j, s in enumerate(sel)], mr=mr)
    listed, strides = run(qf, src, r, sel=sel, n_sel=None if count == "null" else count)
    dense, _ = run(qf, gathered, r)
    same(listed, dense, "the listed form against the dense call on the gathered batch")
    refs = gathered.refs(r)
    same(listed, expected(refs, k, r, Lb, mr, *strides), "the listed form against the model")
    if n > 2:
        assert refs[2]["status"] == EINVAL and refs[2]["rank"] == 0
    for ref in refs[n:]:
        assert ref["status"] == ENOTREADY and ref["rank"] == 0 and (ref["src_slot"] == NONE16).all()


# ---------------------------------------------------------------------------
# 6, 7: many random generations of mixed rank; two runs
# ---------------------------------------------------------------------------
def random_gen(rng, k, Lb):
    n = int(rng.integers(0, 2 * k + 1))
    vecs = []
    for _ in range(n):
        kind = int(rng.integers(0, 5))
        if kind < 2:
            vecs.append(P.unit(k, int(rng.integers(0, k))))
        elif kind < 4:
            vecs.append(P.over(rng, k, rng.choice(k, int(rng.integers(2, 5)), replace=False).tolist()))
        else:
            vecs.append(rng.integers(0, 256, k, dtype=np.uint8))
    return P.Gen(rng, k, Lb, vecs)


@pytest.fixture(scope="module")
def random_batch():
    rng = np.random.default_rng(300)
    return Batch([random_gen(rng, 12, 40) for _ in range(300)], mr=24)


def test_300_random_generations(qf, gpu_ctx, random_batch):
    refs = against_model(qf, random_batch, 12)
    st = [ref["status"] for ref in refs]
    assert st.count(OK) >= 20 and st.count(ENOTREADY) >= 100
    partial = [ref for ref in refs if ref["status"] == ENOTREADY and ref["D"]]
    assert len(partial) >= 20 and any(ref["bound"] < ref["rank"] for ref in partial)
    # without n_rows every generation has max_rows slots
    full = Batch(random_batch.gens[:40], mr=24)
    for j, g in enumerate(full.gens):
        assert full.n[j] == len(g.idx)
    keep = [g for g in full.gens if len(g.idx) == 24]
    if keep:
        against_model(qf, Batch(keep, mr=24), 12, with_n=False)


def test_two_runs_give_identical_bytes(qf, gpu_ctx, random_batch):
    dev = random_batch.device()
    a, _ = run(qf, random_batch, 12, dev=dev)
    b, _ = run(qf, random_batch, 12, dev=dev)
    same(a, b, "two runs")


# ---------------------------------------------------------------------------
# 8: the loop, with the partial decode in front of the resets
# ---------------------------------------------------------------------------
K_LOOP, R_LOOP, L_LOOP, G_LOOP, GENS_LOOP, N_LOOP, MR_LOOP = 8, 4, 48, 5, 24, 24, 12
BASE_LOOP = (1 << 40) + 2


def _loop_stream(rng):
    """Per wire generation the frames that survive, (source index or k + j, vector): the systematic
    frames and four sparse repairs, some dropped; three polls per generation, two generations a poll."""
    k = K_LOOP
    gens = []
    for g in range(GENS_LOOP):
        frames = [(i, P.unit(k, i)) for i in range(k)]
        frames += [(k + j, P.over(rng, k, rng.choice(k, 3, replace=False).tolist())) for j in range(R_LOOP)]
        loss = (0.0, 0.25, 0.45)[g % 3]
        gens.append([f for f in frames if rng.random() >= loss])
    return gens


class Slot:
    """The model of one slot's store: the innovative rows in arrival order."""

    def __init__(self):
        self.idx, self.vec, self.pay = [], [], []

    def add(self, i, v, row):
        from tests import rank_ref

        vec = P.unit(K_LOOP, i) if i < K_LOOP else v
        if rank_ref.innovative(np.stack(self.vec + [vec]))[1] > len(self.vec):
            self.idx.append(i)
            self.vec.append(vec)
            self.pay.append(row)

    def ref(self):
        co = np.stack(self.vec) if self.vec else np.zeros((0, K_LOOP), np.uint8)
        return P.partial_ref(K_LOOP, R_LOOP, L_LOOP, np.array(self.idx, np.int64), co, [p.tobytes() for p in self.pay])


def _delivered(out, j, snap, s, k, Lb, em, rec_rs, rec_gs):
    """source index -> packet of entry j, through src_slot (the store) or rec_index (rec)."""
    got = {}
    slot = out["slot"].view(np.uint16)[j * k: (j + 1) * k]
    for i in range(k):
        if slot[i] != NONE16:
            c = int(slot[i])
            assert snap["index"][s, c] == i
            ln, off = int(snap["len"][s, c]), int(snap["off"][s, c])
            row = np.zeros(Lb, np.uint8)
            row[:ln] = snap["bytes"][s, off: off + ln]
            got[i] = row
    nrec = int(out["nrec"].view(np.uint32)[j])
    for m in range(nrec):
        i = int(out["ri"].view(np.uint16)[j * em + m])
        assert i not in got
        got[i] = out["rec"][j * rec_gs + m * rec_rs: j * rec_gs + m * rec_rs + Lb]
    return got


class LoopPoll:
    """One poll of the loop under the model alone: the frames taken, the window call's outputs, what the
    displaced slots' stores determine, the slots that complete."""


def loop_model():
    """-> src (GENS, k, L), the polls, the flush (slots, their generations, their references).  Generation
    g's surviving frames go out in polls g, g + 1 and g + 2; it is displaced by generation g + G."""
    k, G, N = K_LOOP, G_LOOP, N_LOOP
    rng = np.random.default_rng(24)
    stream = _loop_stream(rng)
    src = rng.integers(1, 256, (GENS_LOOP, k, L_LOOP), dtype=np.uint8)
    win = np.zeros(G, np.uint64)
    slots = [Slot() for _ in range(G)]
    holds = [None] * G                     # the wire generation a slot's store belongs to
    polls = []
    for poll in range(GENS_LOOP + 2):
        q = LoopPoll()
        take = []
        for g in range(max(0, poll - 2), min(poll + 1, GENS_LOOP)):
            fr = stream[g]
            third = -(-len(fr) // 3)
            take += [(g, f) for f in fr[(poll - g) * third: (poll - g + 1) * third]]
        q.take = [take[i] for i in rng.permutation(len(take))]
        assert len(q.take) <= N
        q.ids = np.full(N, BASE_LOOP, np.uint64)
        q.ids[: len(q.take)] = [BASE_LOOP + g for g, _ in q.take]
        q.w = WR.window(win, q.ids, len(q.take), G, G)
        win = q.w.win
        q.evicted = [(s, holds[s], slots[s].ref()) for s in q.w.evicted]
        for s in q.w.evicted:
            slots[s], holds[s] = Slot(), None
        q.rows = []
        for f, (g, (i, v)) in enumerate(q.take):
            row = P.encode_rows(v[None, :], src[g])[0]
            q.rows.append(row)
            if q.w.frame_status[f] == WR.OK:
                s = int(q.w.frame_gen[f])
                assert holds[s] in (None, g)
                holds[s] = g
                slots[s].add(i, v, row)
        q.done = [(s, holds[s]) for s in range(G) if len(slots[s].idx) == k]
        for s, _ in q.done:
            slots[s], holds[s] = Slot(), None
        win, _ = WR.window_sel(win, [s for s, _ in q.done], len(q.done), G, G, True)
        q.win_after = win
        polls.append(q)
    flush = [(s, holds[s], slots[s].ref()) for s in range(G) if slots[s].idx]
    return src, stream, polls, flush


def test_the_loop_saves_what_displaced_generations_hold(qf, oracle, gpu_ctx):
    import torch

    k, r, Lb, G, N, mr = K_LOOP, R_LOOP, L_LOOP, G_LOOP, N_LOOP, MR_LOOP
    em = min(k, r)
    src, stream, polls, flush = loop_model()
    rc = T.Receiver(qf, G, k, Lb, k, 0)
    seen = torch.zeros(G, dtype=torch.int32, device="cuda")
    t_win = SW._guarded(np.zeros(G, np.uint64))
    fs = PR.payload_offset(k) + _r16(Lb)
    rec_rs = _r16(Lb) + 16
    rec_gs = em * rec_rs
    saved, completed = {}, {}
    nothing = P.partial_ref(k, r, Lb, [], np.zeros((0, k), np.uint8), [])

    def partial_over(t_sel, t_nsel):
        t = _out_buffers(G, k, em, k, rec_gs)
        qf.decode_partial_frames_sel(t_sel, t_nsel, rc.bytes, rc.off, rc.len, rc.index, rc.coeffs, t["rec"], t["ri"],
                                     t["nrec"], t["st"], k, r, Lb, n_max=G, G_src=G, max_rows=k, src_gen_stride=rc.gs,
                                     rec_row_stride=rec_rs, rec_gen_stride=rec_gs, n_rows=rc.n, rank=t["rank"],
                                     innovative=t["flags"], src_slot=t["slot"])
        qf.default_context().sync()
        return {key: _host(t[key]).copy() for key in KEYS}

    def check_saved(out, listed, snap):
        """The entries of a partial decode over the listed slots against the model of their stores."""
        refs = [ref for _, _, ref in listed] + [nothing] * (G - len(listed))
        same(out, expected(refs, k, r, Lb, k, rec_rs, rec_gs), "the partial decode over the store")
        for j, (s, g, ref) in enumerate(listed):
            got = _delivered(out, j, snap, s, k, Lb, em, rec_rs, rec_gs)
            want = {i for i in range(k) if ref["src_slot"][i] != NONE16} | set(ref["D"])
            assert set(got) == want, (g, sorted(got), sorted(want))
            for i, row in got.items():
                assert np.array_equal(row, src[g, i]), (g, i)
            assert ref["status"] == ENOTREADY and g not in saved and g not in completed
            saved[g] = (sorted(got), len(ref["D"]))

    for poll, q in enumerate(polls):
        n = len(q.take)
        # the window, then the partial decode over the evict list, then the two resets
        d, h = SW.run_window(qf, None, q.ids, n, G, G, t_win=t_win)
        SW.check_window(h, q.w)
        snap = rc.snapshot()
        check_saved(partial_over(d["esel"], d["nev"]), q.evicted, snap)
        qf.stream_reset(d["esel"], d["nev"], k, n_max=G, G_src=G, state=rc.state, store_n=rc.n, seen=seen)
        qf.stream_reset(d["esel"], d["nev"], k, n_max=G, G_src=G, seen=rc.rank)
        # the ingest, the listed update and append
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
        # select, the full decode, close, the two resets: the completed generations come out as before
        t_sel, t_nsel = _filled(4 * G + GUARD), _filled(4 + GUARD)
        qf.gen_select(rc.rank, t_sel, t_nsel, G=G, min_rank=k, n_max=G, seen=seen, mark=True)
        t = _out_buffers(G, k, em, k, rec_gs)
        qf.decode_frames_sel(t_sel, t_nsel, rc.bytes, rc.off, rc.len, rc.index, rc.coeffs, t["rec"], t["ri"], t["nrec"],
                             t["st"], k, r, Lb, n_max=G, G_src=G, max_rows=k, src_gen_stride=rc.gs,
                             rec_row_stride=rec_rs, rec_gen_stride=rec_gs, n_rows=rc.n, src_slot=t["slot"])
        snap = rc.snapshot()
        qf.gen_window_sel(t_sel, t_nsel, t_win, n_max=G, G_src=G, close=True)
        qf.stream_reset(t_sel, t_nsel, k, n_max=G, G_src=G, state=rc.state, store_n=rc.n, seen=seen)
        qf.stream_reset(t_sel, t_nsel, k, n_max=G, G_src=G, seen=rc.rank)
        qf.default_context().sync()
        n_done = int(T._body(t_nsel, 4, np.uint32)[0])
        assert T._body(t_sel, 4 * G, np.uint32)[:n_done].tolist() == [s for s, _ in q.done], poll
        out = {key: _host(t[key]).copy() for key in ("rec", "ri", "nrec", "st", "slot")}
        for j, (s, g) in enumerate(q.done):
            assert out["st"].view(np.int32)[j] == OK
            got = _delivered(out, j, snap, s, k, Lb, em, rec_rs, rec_gs)
            assert sorted(got) == list(range(k)) and all(np.array_equal(got[i], src[g, i]) for i in range(k)), g
            assert g not in saved and g not in completed
            completed[g] = poll
        assert np.array_equal(T._body(t_win, 8 * G, np.uint64), q.win_after), poll
    # the flush at the end of the stream: every slot that still holds a row
    t_sel, t_nsel = _filled(4 * G + GUARD), _filled(4 + GUARD)
    qf.gen_select(rc.rank, t_sel, t_nsel, G=G, min_rank=1, n_max=G)
    qf.default_context().sync()
    snap = rc.snapshot()
    assert int(T._body(t_nsel, 4, np.uint32)[0]) == len(flush)
    assert T._body(t_sel, 4 * G, np.uint32)[: len(flush)].tolist() == [s for s, _, _ in flush]
    check_saved(partial_over(t_sel, t_nsel), flush, snap)
    # every generation came out one way or the other, with what the model says it holds
    assert sorted(list(saved) + list(completed)) == [g for g in range(GENS_LOOP) if stream[g]]
    check_loop_stats(saved, completed)


def check_loop_stats(saved, completed):
    """The stream holds what the test is about (tests/test_partial_decode_cpu.py runs this on the model)."""
    assert len(completed) >= 8 and len(saved) >= 5
    assert any(nd for _, nd in saved.values()), "no displaced generation had a source determined by coded rows"
    assert any(len(have) < K_LOOP for have, _ in saved.values())


# ---------------------------------------------------------------------------
# 9: profile names
# ---------------------------------------------------------------------------
def test_profile_names(qf, gpu_ctx):
    rng = np.random.default_rng(9)
    b = Batch([determined_gen(rng, 16, 100, 10, 2)[0] for _ in range(4)])
    gpu_ctx.sync()
    gpu_ctx.profile(True)
    run(qf, b, 16)
    dense = gpu_ctx.kernel_times()
    gpu_ctx.profile(False)
    assert set(dense) == {"k_rank_filter", "k_partial_prepare", "k_combine_rows_at"}, dense
    assert dense["k_partial_prepare"][0] == 1 and dense["k_combine_rows_at"][0] == 1
    gpu_ctx.profile(True)
    run(qf, b, 16, sel=[1, 0])
    listed = gpu_ctx.kernel_times()
    gpu_ctx.profile(False)
    assert set(listed) == {"k_sel_gather", "k_rank_filter", "k_partial_prepare", "k_combine_rows_at"}, listed
