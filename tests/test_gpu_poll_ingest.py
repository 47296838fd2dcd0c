"""The flat-poll ingest on the MI355X: qf_parse_poll_headers_dev against
tests/poll_ref.py and against qf_parse_frame_headers_dev over the host-sorted
poll; qf_rank_update_sel_batch and qf_store_append_sel_dev against
qf_rank_update_batch and qf_store_append_dev over the host-sorted dense poll,
three polls in sequence; and the whole loop, flat poll -> ingest -> listed
update -> listed append -> select -> listed decode -> the two resets, until
every generation is decoded.

Every output starts as 0xCC with guard bytes behind it, the bytes a call must
not write are checked to still be 0xCC, and the sources are checked to be
unchanged.  The polls are tests/poll_ref.py's; tests/test_poll_ingest_cpu.py
asserts that they hold the cases these tests are about."""
import numpy as np
import pytest

from tests import poll_ref as PR
from tests import recv_ref
from tests import test_gpu_rank as K
from tests import test_gpu_recv_inplace as I
from tests import test_gpu_wire_coded as W

pytestmark = pytest.mark.gpu

FILL, FILL16, FILL32, NONE16 = 0xCC, 0xCCCC, 0xCCCCCCCC, 0xFFFF
OK, EINVAL, ENOTREADY, ETOOSMALL = 0, -1, -3, -7
GUARD = 64

_r16, _dev, _filled, _host = W._r16, W._dev, W._filled, W._host


def _body(t, nbytes, dtype=np.uint8):
    """The first nbytes of a guarded device buffer as dtype; the guard behind them must be 0xCC."""
    h = _host(t)
    assert (h[nbytes:] == FILL).all(), "bytes behind an output were written"
    return h[:nbytes].view(dtype).copy()


class FlatPoll:
    """A poll_ref.Poll on the device."""

    def __init__(self, p, n_frames="null"):
        self.p = p
        self.frames, self.flen, self.foff = _dev(p.frames), _dev(p.flen), _dev(p.foff)
        self.ids, self.gen = _dev(p.ids), _dev(p.gen)
        self.n_frames = None if n_frames == "null" else _dev(np.array([n_frames], np.uint32))

    def unchanged(self):
        p = self.p
        for t, a in ((self.frames, p.frames), (self.flen, p.flen), (self.foff, p.foff), (self.ids, p.ids), (self.gen, p.gen)):
            assert np.array_equal(_host(t), np.ascontiguousarray(a).view(np.uint8).reshape(-1)), "a source array was written"


def run_ingest(qf, fp, G_src, n_max, mr):
    p = fp.p
    k, N = p.k, p.N_max
    d = dict(sel=_filled(4 * n_max + GUARD), n_sel=_filled(4 + GUARD), n_match=_filled(4 + GUARD),
             idx=_filled(2 * n_max * mr + GUARD), n=_filled(4 * n_max + GUARD), co=_filled(n_max * mr * k + GUARD),
             rl=_filled(4 * n_max * mr + GUARD), ro=_filled(4 * n_max * mr + GUARD), est=_filled(4 * n_max + GUARD),
             fst=_filled(4 * N + GUARD))
    qf.parse_poll_headers(fp.frames, fp.flen, fp.ids, fp.gen, d["sel"], d["n_sel"], d["idx"], d["n"], d["co"], d["rl"],
                          d["ro"], d["est"], d["fst"], k, p.L, max_rows=mr, frame_stride=p.fs, N_max=N, G_src=G_src,
                          n_max=n_max, n_frames=fp.n_frames, frame_off=fp.foff, n_match=d["n_match"])
    qf.default_context().sync()
    fp.unchanged()
    h = dict(sel=_body(d["sel"], 4 * n_max, np.uint32), n_sel=int(_body(d["n_sel"], 4, np.uint32)[0]),
             n_match=int(_body(d["n_match"], 4, np.uint32)[0]),
             idx=_body(d["idx"], 2 * n_max * mr, np.uint16).reshape(n_max, mr), n=_body(d["n"], 4 * n_max, np.uint32),
             co=_body(d["co"], n_max * mr * k).reshape(n_max, mr, k),
             rl=_body(d["rl"], 4 * n_max * mr, np.uint32).reshape(n_max, mr),
             ro=_body(d["ro"], 4 * n_max * mr, np.uint32).reshape(n_max, mr), est=_body(d["est"], 4 * n_max, np.int32),
             fst=_body(d["fst"], 4 * N, np.int32))
    return d, h


def check_against_reference(h, ref):
    assert h["n_sel"] == ref.n_sel and h["n_match"] == ref.n_match
    for key, want in (("sel", ref.sel), ("n", ref.n_rows), ("est", ref.entry_status), ("fst", ref.frame_status),
                      ("ro", ref.row_off), ("rl", ref.row_len), ("idx", ref.row_index), ("co", ref.row_coeffs)):
        bad = np.argwhere(h[key] != want)
        assert bad.size == 0, f"{key} differs from the reference at {bad[:4].tolist()}"


def dense_headers(qf, p, entries, G, mr, gens=None):
    """qf_parse_frame_headers_dev over the host-sorted poll -> device tensors, host views."""
    k = p.k
    fr, fl, fo, ids, nfr = PR.dense_poll(p, entries, G, mr, gens)
    d = dict(frames=_dev(fr), flen=_dev(fl), foff=_dev(fo), ids=_dev(ids), nfr=_dev(nfr),
             idx=_filled(2 * G * mr + GUARD), n=_filled(4 * G + GUARD), st=_filled(4 * G * mr + GUARD),
             co=_filled(G * mr * k + GUARD), rl=_filled(4 * G * mr + GUARD), ro=_filled(4 * G * mr + GUARD))
    qf.parse_frame_headers(d["frames"], d["flen"], d["ids"], d["idx"], d["n"], d["st"], d["co"], d["rl"], d["ro"], k, p.L,
                           max_rows=mr, frame_stride=p.fs, G=G, n_frames=d["nfr"], frame_off=d["foff"])
    qf.default_context().sync()
    h = dict(idx=_body(d["idx"], 2 * G * mr, np.uint16).reshape(G, mr), n=_body(d["n"], 4 * G, np.uint32),
             st=_body(d["st"], 4 * G * mr, np.int32).reshape(G, mr), co=_body(d["co"], G * mr * k).reshape(G, mr, k),
             rl=_body(d["rl"], 4 * G * mr, np.uint32).reshape(G, mr), ro=_body(d["ro"], 4 * G * mr, np.uint32).reshape(G, mr))
    return d, h


@pytest.mark.parametrize("n_max", [PR.G_POLL, 8], ids=["list_fits", "list_full"])
@pytest.mark.parametrize("k,mr", PR.SHAPES)
def test_ingest_against_the_reference_and_the_dense_parser(qf, gpu_ctx, k, mr, n_max):
    G_src = PR.G_POLL
    p = PR.make_poll(k, mr, 1)
    ref = PR.ingest(p, None, G_src, n_max, mr)
    fp = FlatPoll(p)
    d, h = run_ingest(qf, fp, G_src, n_max, mr)
    check_against_reference(h, ref)
    # two runs give identical bytes
    d2, h2 = run_ingest(qf, fp, G_src, n_max, mr)
    for key in h:
        assert np.array_equal(h[key], h2[key]), f"{key} differs between two runs"
    # the dense parser over the host-sorted poll, entry by entry
    _, dh = dense_headers(qf, p, ref.entries, n_max, mr)
    for j in range(ref.n_sel):
        n = int(h["n"][j])
        assert n == dh["n"][j], j
        assert np.array_equal(h["rl"][j, :n], dh["rl"][j, :n]) and np.array_equal(h["idx"][j, :n], dh["idx"][j, :n]), j
        assert np.array_equal(h["co"][j, :n], dh["co"][j, :n]), j
        for s, f in enumerate(ref.entries[j]):
            assert h["fst"][f] == dh["st"][j, s], (j, s, f)
        for c, f in enumerate(ref.row_frame[j]):
            s = ref.entries[j].index(f)
            assert int(h["ro"][j, c]) - f * p.fs == int(dh["ro"][j, c]) - s * p.fs, (j, c)


@pytest.mark.parametrize("n_frames", [0, PR.N_POLL + 7, 150, "null"])
def test_ingest_frame_counts(qf, gpu_ctx, n_frames):
    k, mr, G_src, n_max = 64, 6, PR.G_POLL, PR.G_POLL
    p = PR.make_poll(k, mr, 2)
    ref = PR.ingest(p, None if n_frames == "null" else n_frames, G_src, n_max, mr)
    assert ref.N == {0: 0, PR.N_POLL + 7: PR.N_POLL, 150: 150, "null": PR.N_POLL}[n_frames]
    d, h = run_ingest(qf, FlatPoll(p, n_frames), G_src, n_max, mr)
    check_against_reference(h, ref)
    if n_frames == 0:
        assert h["n_sel"] == 0 and not h["n"].any() and (h["fst"].view(np.uint32) == FILL32).all()


# ---------------------------------------------------------------------------
# listed update and append against the dense calls
# ---------------------------------------------------------------------------
class Receiver:
    """Rank states, a persistent rank array and a row store of G generations on the device."""

    def __init__(self, qf, G, k, Lb, cap, rank_fill):
        import torch

        self.qf, self.G, self.k, self.L, self.cap = qf, G, k, Lb, cap
        self.sb = qf.rank_state_bytes(k)
        self.rs = _r16(Lb)
        self.gs = cap * self.rs + 32
        self.state = torch.zeros(G * self.sb + GUARD, dtype=torch.uint8, device="cuda")
        self.state[G * self.sb:] = FILL
        self.rank = torch.full((4 * G + GUARD,), rank_fill, dtype=torch.uint8, device="cuda")
        self.rank[4 * G:] = FILL
        self.bytes = _filled(G * self.gs + GUARD)
        self.off, self.len = _filled(4 * G * cap + GUARD), _filled(4 * G * cap + GUARD)
        self.index, self.coeffs = _filled(2 * G * cap + GUARD), _filled(G * cap * k + GUARD)
        self.n = torch.zeros(G, dtype=torch.int32, device="cuda")

    def snapshot(self):
        G, cap, k = self.G, self.cap, self.k
        return dict(state=_body(self.state, G * self.sb).reshape(G, self.sb), rank=_body(self.rank, 4 * G, np.uint32),
                    bytes=_body(self.bytes, G * self.gs).reshape(G, self.gs),
                    off=_body(self.off, 4 * G * cap, np.uint32).reshape(G, cap),
                    len=_body(self.len, 4 * G * cap, np.uint32).reshape(G, cap),
                    index=_body(self.index, 2 * G * cap, np.uint16).reshape(G, cap),
                    coeffs=_body(self.coeffs, G * cap * k).reshape(G, cap * k), n=_host(self.n, np.uint32).copy())

    def dense_poll(self, rows, mr, sgs):
        """qf_rank_update_batch + qf_store_append_dev over a dense poll's rows -> flags, rank, statuses."""
        qf, G = self.qf, self.G
        t_fl, t_st, t_ast = _filled(G * mr + GUARD), _filled(4 * G + GUARD), _filled(4 * G + GUARD)
        qf.rank_update_batch(rows["idx"], self.state, self.rank, t_st, self.k, max_rows=mr, G=G, n_rows=rows["n"],
                             row_coeffs=rows["co"], innovative=t_fl)
        qf.store_append(rows["frames"], rows["ro"], rows["rl"], rows["idx"], rows["co"], self.bytes, self.off, self.len,
                        self.index, self.coeffs, self.n, t_ast, self.k, self.L, max_rows=mr, cap=self.cap,
                        src_gen_stride=sgs, store_row_stride=self.rs, store_gen_stride=self.gs, G=G, n_rows=rows["n"],
                        take=t_fl)
        qf.default_context().sync()
        return (_body(t_fl, G * mr).reshape(G, mr), _body(t_st, 4 * G, np.int32), _body(t_ast, 4 * G, np.int32))

    def listed_poll(self, sel, n_sel, n_max, rows, mr, src, src_bytes, rank_sel=True):
        """qf_rank_update_sel_batch + qf_store_append_sel_dev -> flags, rank_sel, statuses (compact)."""
        qf, G = self.qf, self.G
        t_fl, t_st, t_ast = _filled(n_max * mr + GUARD), _filled(4 * n_max + GUARD), _filled(4 * n_max + GUARD)
        t_rs = _filled(4 * n_max + GUARD) if rank_sel else None
        qf.rank_update_sel_batch(sel, n_sel, rows["idx"], self.state, t_st, self.k, max_rows=mr, n_max=n_max, G_src=G,
                                 n_rows=rows["n"], row_coeffs=rows["co"], innovative=t_fl, rank_sel=t_rs, rank=self.rank)
        qf.store_append_sel(sel, n_sel, src, rows["ro"], rows["rl"], rows["idx"], rows["co"], self.bytes, self.off,
                            self.len, self.index, self.coeffs, self.n, t_ast, self.k, self.L, max_rows=mr, cap=self.cap,
                            src_bytes=src_bytes, store_row_stride=self.rs, store_gen_stride=self.gs, n_max=n_max, G_src=G,
                            n_rows=rows["n"], take=t_fl)
        qf.default_context().sync()
        return (_body(t_fl, n_max * mr).reshape(n_max, mr), _body(t_rs, 4 * n_max, np.uint32) if rank_sel else None,
                _body(t_st, 4 * n_max, np.int32), _body(t_ast, 4 * n_max, np.int32))


@pytest.mark.parametrize("k,mr", [(5, 6), (64, 70), (100, 6), (200, 6)])
def test_listed_update_and_append_against_the_dense_calls(qf, gpu_ctx, k, mr):
    G, Lb, n_max = PR.G_POLL, PR.L_POLL, PR.G_POLL
    dense = Receiver(qf, G, k, Lb, k, 0)
    flat = Receiver(qf, G, k, Lb, k, FILL)          # its rank array is written for listed generations only
    for seed in (1, 2, 3):
        p = PR.make_poll(k, mr, seed)
        ref = PR.ingest(p, None, G, n_max, mr)
        listed = [int(g) for g in ref.sel[: ref.n_sel]]
        before = flat.snapshot()
        fp = FlatPoll(p)
        d, h = run_ingest(qf, fp, G, n_max, mr)
        check_against_reference(h, ref)
        fl, rsel, st, ast = flat.listed_poll(d["sel"], d["n_sel"], n_max, d, mr, fp.frames, p.N_max * p.fs)
        fp.unchanged()
        # the same poll sorted by the host into G regions, through the dense calls
        dd, dh = dense_headers(qf, p, ref.entries, G, mr, gens=listed)
        dfl, dst, dast = dense.dense_poll(dd, mr, mr * p.fs)
        a, b = flat.snapshot(), dense.snapshot()
        for j, g in enumerate(listed):
            assert np.array_equal(fl[j], dfl[g]), (seed, j, g)
            assert st[j] == dst[g] == OK and ast[j] == dast[g] == OK, (seed, j, g)
            assert rsel[j] == a["rank"][g] == b["rank"][g], (seed, j, g)
            for key in ("state", "bytes", "off", "len", "index", "coeffs", "n"):
                assert np.array_equal(a[key][g], b[key][g]), (seed, key, g)
        assert any(fl[j].any() for j in range(len(listed)))
        # every byte of an unlisted generation is untouched
        for g in range(G):
            if g not in listed:
                for key in a:
                    assert np.array_equal(a[key][g], before[key][g]), (seed, key, g)
        # unused entries
        for j in range(ref.n_sel, n_max):
            assert not fl[j].any() and st[j] == OK and ast[j] == OK and rsel[j] == 0, j
    for g in PR.UNTOUCHED:
        assert a["rank"][g] == FILL32 and not a["state"][g].any() and (a["bytes"][g] == FILL).all()


@pytest.mark.parametrize("variant", ["below", "clamped", "null", "zero"])
def test_invalid_and_unused_list_entries(qf, gpu_ctx, variant):
    """The ingest's rows under a list of the caller's: entry 1 replaced by a
    generation >= G_src, and counts below n_max, above it, NULL and zero."""
    k, mr, G, Lb = 64, 6, PR.G_POLL, PR.L_POLL
    p = PR.make_poll(k, mr, 1)
    n_max = PR.ingest(p, None, G, G, mr).n_sel            # the list is exactly full: NULL uses every entry
    ref = PR.ingest(p, None, G, n_max, mr)
    fp = FlatPoll(p)
    d, h = run_ingest(qf, fp, G, n_max, mr)
    sel = h["sel"].copy()
    assert ref.n_rows[1] > 0
    sel[1] = G + 3
    n_sel = dict(below=n_max - 2, clamped=n_max + 5, null=None, zero=0)[variant]
    used = n_max if n_sel is None else min(n_sel, n_max)
    flat = Receiver(qf, G, k, Lb, k, FILL)
    before = flat.snapshot()
    t_sel = _dev(sel)
    t_n = None if n_sel is None else _dev(np.array([n_sel], np.uint32))
    fl, rsel, st, ast = flat.listed_poll(t_sel, t_n, n_max, d, mr, fp.frames, p.N_max * p.fs)
    assert np.array_equal(_host(t_sel, np.uint32), sel), "the list was written"
    # the dense calls over the entries that count
    dense = Receiver(qf, G, k, Lb, k, 0)
    keep = [j for j in range(used) if j != 1]
    dd, dh = dense_headers(qf, p, [ref.entries[j] for j in keep], G, mr, gens=[sel[j] for j in keep])
    dfl, dst, dast = dense.dense_poll(dd, mr, mr * p.fs)
    a, b = flat.snapshot(), dense.snapshot()
    for j in range(n_max):
        if j in keep:
            g = int(sel[j])
            assert np.array_equal(fl[j], dfl[g]) and st[j] == OK and ast[j] == OK and rsel[j] == b["rank"][g], j
            for key in ("state", "bytes", "off", "len", "index", "coeffs", "n"):
                assert np.array_equal(a[key][g], b[key][g]), (key, g)
        else:
            want = EINVAL if j < used else OK
            assert not fl[j].any() and st[j] == want and ast[j] == want and rsel[j] == 0, (j, st[j], ast[j])
    touched = {int(sel[j]) for j in keep}
    for g in range(G):
        if g not in touched:
            for key in a:
                assert np.array_equal(a[key][g], before[key][g]), (key, g)
    if variant == "zero":
        assert not touched


# ---------------------------------------------------------------------------
# the whole loop
# ---------------------------------------------------------------------------
def complete_gens(oracle, rng, k, Lb, G, r):
    """G generations that all reach rank k: k - e systematic rows, two of them
    repeated, and 2 e random coded rows, shuffled -> K.Gens (a coded row has index k)."""
    e = max(2, k // 4)
    mr = (k - e) + 2 + 2 * e
    idx = np.full((G, mr), k, np.uint16)
    co = np.zeros((G, mr, k), np.uint8)
    for g in range(G):
        have = [int(x) for x in rng.permutation(k)[: k - e]]
        kinds = have + have[:2] + [k] * (2 * e)
        for s, j in enumerate(rng.permutation(mr)):
            i = kinds[int(j)]
            idx[g, s] = i
            if i < k:
                co[g, s, i] = 1
            else:
                co[g, s] = rng.integers(0, 256, k)
    return K.Gens(oracle, k, r, Lb, recv_ref.tailed_sources(rng, G, k, Lb), idx, None, co)


def test_the_loop_from_flat_polls_to_decoded_generations(qf, oracle, gpu_ctx):
    import torch

    k, Lb, G, r, mr, N_max, n_max = 8, 100, 7, 4, 3, 24, 4
    rng = np.random.default_rng(816)
    gs = complete_gens(oracle, rng, k, Lb, G, r)
    assert all(rk == k for rk in gs.rank) and not all(f.all() for f in gs.flags)
    rx, lens = I.frame_gens(oracle, gs)
    # one arrival order over all generations, each generation's own order kept
    nxt = [0] * G
    pool = [g for g in range(G) for _ in range(int(gs.n[g]))]
    arrival = []
    for i in rng.permutation(len(pool)):
        g = pool[int(i)]
        arrival.append((g, nxt[g]))
        nxt[g] += 1
    rc = Receiver(qf, G, k, Lb, k, 0)
    seen = torch.zeros(G, dtype=torch.int32, device="cuda")
    em = min(k, r)
    rec_rs = _r16(Lb) + 16
    rec_gs = em * rec_rs
    done, polls, full = {}, 0, 0
    queue = arrival
    while queue:
        polls += 1
        assert polls < 200
        # the ring: at most N_max frames and at most mr of a generation per poll (a generation with
        # more would be refused as a whole, again and again), the rest waits in order; frames of
        # delivered generations are dropped
        take, wait, count = [], [], {}
        for g, s in queue:
            if g in done:
                continue
            if len(take) < N_max and count.get(g, 0) < mr and (g, "blocked") not in count:
                take.append((g, s))
                count[g] = count.get(g, 0) + 1
            else:
                wait.append((g, s))
                count[(g, "blocked")] = 1
        if not take:
            break
        p = PR.Poll(k, Lb, N_max, rx.fs)
        for f, (g, s) in enumerate(take):
            p.frames[f], p.flen[f], p.foff[f], p.ids[f], p.gen[f] = rx.frames[g, s], rx.flen[g, s], rx.foff[g, s], rx.ids[g, s], g
        fp = FlatPoll(p, len(take))
        d, h = run_ingest(qf, fp, G, n_max, mr)
        check_against_reference(h, PR.ingest(p, len(take), G, n_max, mr))
        # frames whose generation did not fit the list are presented again, in front
        queue = [take[f] for f in range(len(take)) if h["fst"][f] == ENOTREADY] + wait
        assert all(h["fst"][f] in (OK, ENOTREADY) for f in range(len(take))) and (h["est"] == OK).all()
        full += h["n_match"] > h["n_sel"]
        fl, rsel, st, ast = rc.listed_poll(d["sel"], d["n_sel"], n_max, d, mr, fp.frames, N_max * rx.fs, rank_sel=False)
        assert (st == OK).all() and (ast == OK).all()
        t_sel, t_nsel = _filled(4 * n_max + GUARD), _filled(4 + GUARD)
        qf.gen_select(rc.rank, t_sel, t_nsel, G=G, min_rank=k, n_max=n_max, seen=seen, mark=True)
        t = I._outputs(n_max, k, em, k, rec_gs)
        qf.decode_frames_sel(t_sel, t_nsel, rc.bytes, rc.off, rc.len, rc.index, rc.coeffs, t["rec"], t["ri"], t["nrec"],
                             t["st"], k, r, Lb, n_max=n_max, G_src=G, max_rows=k, src_gen_stride=rc.gs,
                             rec_row_stride=rec_rs, rec_gen_stride=rec_gs, n_rows=rc.n, src_slot=t["slot"])
        snap = rc.snapshot()
        qf.stream_reset(t_sel, t_nsel, k, n_max=n_max, G_src=G, state=rc.state, store_n=rc.n, seen=seen)
        qf.stream_reset(t_sel, t_nsel, k, n_max=n_max, G_src=G, seen=rc.rank)
        qf.default_context().sync()
        n_done = int(_body(t_nsel, 4, np.uint32)[0])
        finished = _body(t_sel, 4 * n_max, np.uint32)[:n_done]
        out = I._collect(t, n_max, k, em, k, Lb, rec_rs, rec_gs, ("slot",))
        after = rc.snapshot()
        for j, g in enumerate(int(x) for x in finished):
            assert g not in done and snap["rank"][g] == k and snap["n"][g] == k and out["st"][j] == OK, (j, g)
            rix = out["ri"][j, : out["nrec"][j]].tolist()
            rows = np.zeros((k, Lb), np.uint8)
            for i in range(k):
                c = int(out["slot"][j, i])
                if c == NONE16:
                    rows[i] = out["rec"][j, rix.index(i)]
                else:
                    assert snap["index"][g, c] == i
                    ln, off = int(snap["len"][g, c]), int(snap["off"][g, c])
                    rows[i, :ln] = snap["bytes"][g, off: off + ln]
            assert np.array_equal(rows, gs.src[g]), f"generation {g} was not recovered"
            # the oracle is the judge: its decode of the stored rows gives the same sources
            co = snap["coeffs"][g].reshape(k, k)
            pay = np.zeros((k, Lb), np.uint8)
            for c in range(k):
                ln, off = int(snap["len"][g, c]), int(snap["off"][g, c])
                pay[c, :ln] = snap["bytes"][g, off: off + ln]
            assert np.array_equal(oracle.encode(gs.src[g], k, np.ascontiguousarray(co)), pay), g
            done[g] = polls
            # both resets took: the state, the count, seen and the persistent rank are zero again
            assert not after["state"][g].any() and after["n"][g] == 0 and after["rank"][g] == 0, g
        assert _host(seen, np.uint32)[[int(x) for x in finished]].sum() == 0
    assert sorted(done) == list(range(G)), done
    assert full and len(set(done.values())) > 1, (full, done)


def test_profile_names(qf, gpu_ctx):
    k, mr, G, Lb = 64, 6, PR.G_POLL, PR.L_POLL
    p = PR.make_poll(k, mr, 3)
    fp = FlatPoll(p)
    rc = Receiver(qf, G, k, Lb, k, 0)
    gpu_ctx.sync()
    gpu_ctx.profile(True)
    d, h = run_ingest(qf, fp, G, G, mr)
    rc.listed_poll(d["sel"], d["n_sel"], G, d, mr, fp.frames, p.N_max * p.fs)
    times = gpu_ctx.kernel_times()
    gpu_ctx.profile(False)
    assert sorted(times) == ["k_gen_select", "k_poll_count", "k_poll_headers", "k_poll_place", "k_rank_update_sel",
                             "k_store_prepare_sel", "k_store_rows_sel"], times
    assert all(v[0] == 1 for v in times.values()), times
