"""Later rounds of the persistent loops and the second workspace chunk of
the r > 16 decode, on the MI355X.

The batches here are sized (tests/rounds_ref.py, from the actual CU count)
so that the capped grids stride into a third, partly filled round, or the
decode's workspace holds less than the batch.  The CPU oracle cannot run
thousands of generations in a test, so the truth comes from

* the round trip against the source: sources filled on the device, encoded
  by the library, the erased sources set aside and their slots overwritten
  with repair rows (row_index says which; arrival order is free), decoded;
  the recovered rows must be the rows set aside, status 0, n_rec = the
  generation's own erasure count, rec_index the erased indices ascending, the
  bytes between L and the row stride and every row past n_rec untouched;
  the repairs of 8 seeded generations (0, G - 1 and one of every round or
  chunk among them) equal the oracle's, so the encode is not its own witness;
* tiling a fully checked base of 251 generations (a prime: no grid stride or
  chunk is a multiple of it) along G: generation g must give what the
  oracle-checked generation g % 251 gave;
* and, on top of one of those, variant against variant on the same input."""
import numpy as np
import pytest

from tests import rounds_ref as rr
from tests.test_gpu_decode import _path, _r16, check, make_batch, run_decode

pytestmark = pytest.mark.gpu

SEED = 0x524F554E
PAT = 0x5A
STEP = 16384          # (generation, row) pairs per indexing step


def _ncu(torch):
    return torch.cuda.get_device_properties(0).multi_processor_count


def _sync(torch, qf):
    qf.default_context().sync()
    torch.cuda.synchronize()


def _set(qf, path=None, **opts):
    """The default context's options: creation-time values, then a decode
    path of test_gpu_decode._path, then `opts`."""
    qf.reset_default_options()
    if path:
        _path(None, path)
    qf.set_default_options(encode_small=0, **opts)


def _fill(torch, qf, n, seed):
    from quicfuscate_amd import _lib as Lb

    buf = torch.empty(n, dtype=torch.uint8, device="cuda")
    Lb.check(Lb._lib().qf_fill_splitmix_dev(qf.default_context().handle, buf.data_ptr(), n, seed, 0), "fill")
    return buf


def _profiled(torch, qf, fn):
    """fn() with per-kernel timing on: {kernel name: launches}."""
    ctx = qf.default_context()
    _sync(torch, qf)
    ctx.profile(True)
    try:
        fn()
        _sync(torch, qf)
        return {n: v[0] for n, v in ctx.kernel_times().items()}
    finally:
        ctx.profile(False)


def _part_bounds(items_of, rnd, G):
    """Generation ranges of the grid rounds: round i holds the generations
    whose first item lies in [i rnd, (i + 1) rnd)."""
    first = np.array([items_of(g) for g in range(G + 1)])
    n = -(-items_of(G) // rnd)
    cuts = [int(np.searchsorted(first, i * rnd, side="left")) for i in range(n)] + [G]
    return [(lo, hi) for lo, hi in zip(cuts[:-1], cuts[1:]) if hi > lo]


def _sample(G, bounds, seed, extra=()):
    """8 seeded generations (more when there are more parts): 0, G - 1, the
    extras and one inside every part."""
    rng = np.random.default_rng(seed)
    s = {0, G - 1, *extra}
    for lo, hi in bounds:
        s.add(int(rng.integers(lo, hi)))
    while len(s) < 8:
        s.add(int(rng.integers(0, G)))
    return sorted(s)


class _Batch:
    pass


def _encode(torch, qf, b, *, zero_tail=True):
    """Repairs of b's sources, rows of 16 * padded units (zero tails where the
    bit-sliced encode runs), prefilled 0xA5; returns (rep, launches by kernel)."""
    rep = torch.full((b.G * b.r * b.Lp,), 0xA5, dtype=torch.uint8, device="cuda")
    names = _profiled(torch, qf, lambda: qf.encode_batch(
        b.rows, rep, b.k, b.r, b.L, src_row_stride=b.rs, src_gen_stride=b.k * b.rs, rep_row_stride=b.Lp,
        rep_gen_stride=b.r * b.Lp, G=b.G, zero_tail=zero_tail))
    return rep, names


def _sources(torch, qf, case, G, seed):
    b = _Batch()
    b.k, b.r, b.L, b.G = case.k, case.r, case.L, G
    b.rs, b.Lp, b.rrs = rr.r16(case.L), case.rep_row(), rr.r16(case.L) + 16
    # (the bytes of a source row between L and its stride are random too: no kernel may use them)
    b.rows = _fill(torch, qf, G * b.k * b.rs, seed)
    return b


def _oracle_sample(oracle, b, rep, gens):
    """The library's repairs of `gens` against the oracle (before the erasure)."""
    srcv, repv = b.rows.view(b.G, b.k, b.rs), rep.view(b.G, b.r, b.Lp)
    for g in gens:
        want = oracle.encode(srcv[g].cpu().numpy(), b.r, L=b.L)
        assert np.array_equal(repv[g, :, :b.L].cpu().numpy(), want), f"generation {g}: repairs differ from the oracle"


def _erase(torch, b, rep, own_e, seed):
    """Per generation own_e[g] seeded sources set aside (b.saved, packed) and
    their slots overwritten with distinct seeded repairs, in place."""
    G, k, r, L = b.G, b.k, b.r, b.L
    rng = np.random.default_rng(seed)
    e_hi = int(own_e.max())
    valid = np.arange(e_hi)[None, :] < own_e[:, None]
    er = np.where(valid, np.argsort(rng.random((G, k)), axis=1)[:, :e_hi], k)
    er.sort(axis=1)                                   # ascending, the padding (k) last
    rp = np.argsort(rng.random((G, r)), axis=1)[:, :e_hi]
    gi, ji = np.nonzero(valid)
    ridx = np.tile(np.arange(k, dtype=np.uint16), (G, 1))
    ridx[gi, er[gi, ji]] = (k + rp[gi, ji]).astype(np.uint16)
    dev = "cuda"
    b.e_hi, b.N = e_hi, len(gi)
    b.g_t, b.j_t = torch.from_numpy(gi).to(dev), torch.from_numpy(ji).to(dev)
    b.e_t = torch.from_numpy(er[gi, ji]).to(dev)
    p_t = torch.from_numpy(rp[gi, ji]).to(dev)
    b.er_t, b.valid_t = torch.from_numpy(er).to(dev), torch.from_numpy(valid).to(dev)
    b.own_e_t = torch.from_numpy(own_e.astype(np.int32)).to(dev)
    b.row_index = torch.from_numpy(ridx.view(np.int16)).to(dev)
    b.saved = torch.empty((b.N, b.rs), dtype=torch.uint8, device=dev)
    srcv, repv = b.rows.view(G, k, b.rs), rep.view(G, r, b.Lp)
    for s in range(0, b.N, STEP):
        sl = slice(s, s + STEP)
        b.saved[sl] = srcv[b.g_t[sl], b.e_t[sl]]
        srcv[b.g_t[sl], b.e_t[sl], :L] = repv[b.g_t[sl], p_t[sl], :L]
    torch.cuda.synchronize()


def _own_e(case, G, seed):
    e = np.resize(np.array(case.own_e, np.int64), G)
    np.random.default_rng(seed).shuffle(e)
    return e


class _Out:
    pass


def _decode(torch, qf, b):
    G, k, r, L = b.G, b.k, b.r, b.L
    em = min(k, r)
    o = _Out()
    # (min(k, r) rows of slack behind the last generation: compared between variants, never to be written)
    o.rec = torch.full((G * b.e_hi * b.rrs + em * b.rrs,), PAT, dtype=torch.uint8, device="cuda")
    o.rec_index = torch.full((G * em,), -1, dtype=torch.int16, device="cuda")
    o.n_rec = torch.full((G,), -1, dtype=torch.int32, device="cuda")
    o.status = torch.full((G,), 99, dtype=torch.int32, device="cuda")
    o.names = _profiled(torch, qf, lambda: qf.decode_batch(
        b.rows, b.row_index, o.rec, o.rec_index, o.n_rec, o.status, k, r, L, max_rows=k, row_stride=b.rs,
        rows_gen_stride=k * b.rs, rec_row_stride=b.rrs, rec_gen_stride=b.e_hi * b.rrs, G=G))
    return o


def _check(torch, b, o):
    """The round trip's assertions on one decode's outputs."""
    G, L = b.G, b.L
    em = min(b.k, b.r)
    bad = torch.nonzero(o.status != 0)
    assert bad.numel() == 0, ("status", bad[:8].flatten().tolist(), o.status[bad[:8].flatten()].tolist())
    assert torch.equal(o.n_rec, b.own_e_t), "recovered counts"
    ri = o.rec_index.view(G, em)[:, :b.e_hi].long() & 0xFFFF
    assert bool(((ri == b.er_t) | ~b.valid_t).all()), "recovered indices"
    recv = o.rec[: G * b.e_hi * b.rrs].view(G, b.e_hi, b.rrs)
    assert bool((o.rec[G * b.e_hi * b.rrs:] == PAT).all()), "bytes behind the last generation written"
    for s in range(0, b.N, STEP):
        sl = slice(s, s + STEP)
        got = recv[b.g_t[sl], b.j_t[sl]]
        same = (got[:, :L] == b.saved[sl, :L]).all(dim=1)
        if not bool(same.all()):
            w = int(torch.nonzero(~same)[0]) + s
            raise AssertionError(f"recovered bytes: generation {int(b.g_t[w])}, row {int(b.j_t[w])} "
                                 f"(source {int(b.e_t[w])}); {int((~same).sum())} rows of this step differ")
        assert bool((got[:, L:] == PAT).all()), "bytes past L of a recovered row written"
    for g0 in range(0, G, 1024):
        untouched = (recv[g0:g0 + 1024] == PAT).all(dim=2)
        assert bool((untouched | b.valid_t[g0:g0 + 1024]).all()), "a row past n_rec written"


def _same(torch, a, o, what):
    for f in ("rec", "rec_index", "n_rec", "status"):
        assert torch.equal(getattr(a, f), getattr(o, f)), (what, f)


def _round_trip_batch(torch, qf, oracle, case, G, bounds, *, seed, extra=(), zero_tail=True):
    """Sources, library repairs (oracle-checked sample), erasures in place."""
    b = _sources(torch, qf, case, G, seed)
    rep, enc_names = _encode(torch, qf, b, zero_tail=zero_tail)
    _oracle_sample(oracle, b, rep, _sample(G, bounds, seed + 1, extra))
    _erase(torch, b, rep, _own_e(case, G, seed + 2), seed + 3)
    return b, enc_names


def _cmb_names(names):
    return {n for n in names if n.startswith("qf_combine_bs")}


# ---------------------------------------------------------------------------
# A. the bit-sliced payload pass (qf_combine_bs_*) past two rounds
# ---------------------------------------------------------------------------
def _payload_case(torch, qf, oracle, name, path, variants):
    """variants: [(options, expected payload kernel)], decoding one input; each
    satisfies the round trip and equals the first."""
    case = rr.CASES[name]
    ncu = _ncu(torch)
    G = case.G(ncu)
    rnd = case.rnd(ncu)
    assert rr.wraps(case.items(G), rnd), (G, ncu)
    _set(qf)
    b, _ = _round_trip_batch(torch, qf, oracle, case, G, _part_bounds(case.items, rnd, G),
                             seed=SEED + sum(name.encode()))
    first = None
    for opts, want in variants:
        _set(qf, path, **opts)
        o = _decode(torch, qf, b)
        assert want is not None and _cmb_names(o.names) == {want}, (opts, want, sorted(o.names))
        _check(torch, b, o)
        if first is None:
            first = o
        else:
            _same(torch, first, o, opts)
            del o
    # the variants ran different kernels: none of the options is a no-op
    assert len({w for _, w in variants}) == len(variants)


# (64, 16) has a fused decode: "default_1wave" would run no payload pass, so
# its place is taken by the two-kernel syndrome path
@pytest.mark.parametrize("path", ["general_bs", "syn_bs"])
def test_payload_pass_rounds_one_pass(qf, oracle, gpu_ctx, path):
    """(64, 16), 12 erased, L = 2,100 (ipg = 2: the magic division, a partial
    last unit): 'j' with combine_jump = 1, 'm' with 0."""
    import torch

    _payload_case(torch, qf, oracle, "cmb_one_pass", path,
                  [(dict(combine_jump=j), rr.cmb_kernel(e_max=16, jump=j)) for j in (1, 0)])


@pytest.mark.parametrize("path", ["general_bs", "syn_bs"])
def test_payload_pass_rounds_one_item_per_generation(qf, oracle, gpu_ctx, path):
    """(64, 16) at L = 96 with combine_bs_min_q = 1: Q = 3, ipg = 1, one mostly
    idle item per generation, the item index is the generation index."""
    import torch

    _payload_case(torch, qf, oracle, "cmb_min_q", path,
                  [(dict(combine_jump=j, combine_bs_min_q=1), rr.cmb_kernel(e_max=16, jump=j)) for j in (1, 0)])


@pytest.mark.parametrize("path", ["general_bs", "default_1wave"])
def test_payload_pass_rounds_wide(qf, oracle, gpu_ctx, path):
    """(40, 20), 17 erased: one 24-output pass (combine_wide = 1) or two
    16-output passes in the pass-major launch (0)."""
    import torch

    _payload_case(torch, qf, oracle, "cmb_wide", path,
                  [(dict(combine_wide=w), rr.cmb_kernel(e_max=20, wide=w)) for w in (1, 0)])


@pytest.mark.parametrize("path", ["general_bs", "default_1wave"])
def test_payload_pass_rounds_pass_major(qf, oracle, gpu_ctx, path):
    """(80, 40), three record passes, the generations' own e 5, 20 or 40 (the
    upper passes idle in a third of them each): 'J', 'P', 'V', 'Q'."""
    import torch

    _payload_case(torch, qf, oracle, "cmb_pass_major", path,
                  [(dict(combine_jump=j, combine_xcd=x), rr.cmb_kernel(e_max=40, jump=j, xcd=x))
                   for j, x in ((1, 0), (0, 0), (1, 1), (0, 1))])


@pytest.mark.parametrize("path", ["general_bs", "default_1wave"])
def test_payload_pass_rounds_pm24(qf, oracle, gpu_ctx, path):
    """(100, 64), own e over {3, 30, 48, 49, 55, 64}: three 24-output passes
    (combine_pm24 = 1; the third serves only e >= 49) or four 16-output ones."""
    import torch

    _payload_case(torch, qf, oracle, "cmb_pm24", path,
                  [(dict(combine_pm24=p), rr.cmb_kernel(e_max=64, pm24=p)) for p in (1, 0)])


# ---------------------------------------------------------------------------
# B. the other persistent loops
# ---------------------------------------------------------------------------
def _joint_G(cases, ncu):
    """The smallest G at which every (items, round) of `cases` wraps."""
    G = max(c.G(ncu) for c in cases)
    while not all(rr.wraps(c.items(G), c.rnd(ncu)) for c in cases):
        G += 1
    return G


def test_capped_grids_of_the_generated_kernels(qf, oracle, gpu_ctx):
    """(64, 16) at L = 1,200, zero-tail rows: the encode with
    enc_blocks_per_cu = 1 and the fused decode (13 erased) with
    dec_blocks_per_cu = 1 stride over their items; each equals its uncapped
    run bit for bit and satisfies the round trip."""
    import torch

    enc, dec = rr.CASES["enc_capped"], rr.CASES["dec_capped"]
    ncu = _ncu(torch)
    G = _joint_G([enc, dec], ncu)
    k, r = enc.k, enc.r
    _set(qf)
    b = _sources(torch, qf, enc, G, SEED + 10)
    reps = []
    for cap in (0, 1):
        _set(qf, enc_blocks_per_cu=cap)
        rep, names = _encode(torch, qf, b)
        assert set(names) == {rr.kernel("E", k, r)}, names
        reps.append(rep)
    assert torch.equal(reps[0], reps[1]), "capped encode differs from the uncapped one"
    rep = reps[1]
    del reps
    assert bool((rep.view(G, r, b.Lp)[:, :, b.L:] == 0).all()), "zero tails"
    bounds = _part_bounds(enc.items, enc.rnd(ncu), G)
    _oracle_sample(oracle, b, rep, _sample(G, bounds, SEED + 11))
    _erase(torch, b, rep, _own_e(dec, G, SEED + 12), SEED + 13)
    del rep
    outs = []
    for cap in (0, 1):
        _set(qf, dec_blocks_per_cu=cap)
        o = _decode(torch, qf, b)
        assert rr.kernel("C", k, r) in o.names and not _cmb_names(o.names), o.names
        _check(torch, b, o)
        outs.append(o)
    _same(torch, outs[0], outs[1], "capped fused decode against the uncapped one")


def test_capped_grids_of_the_merged_c5_kernels(qf, oracle, gpu_ctx):
    """(160, 48) at L = 2,048: the merged encode (a block is one item's
    passes) with enc_blocks_per_cu = 1, and the r > 16 decode's syndrome
    kernels with dec_blocks_per_cu = 1: shared-row 'Z', pass-major FFT 'Y'
    (synw_shared = 0) and pass-major plain 'X' (and fft_kernels = 0)."""
    import torch

    enc, dec = rr.CASES["c5_enc_capped"], rr.CASES["c5_dec_capped"]
    ncu = _ncu(torch)
    k, r = enc.k, enc.r
    z_waves = rr.spec_of("Z", k, r).waves
    z_items, z_rnd = dec.items, (lambda n: rr.merged_round(n, 1, z_waves))
    G = _joint_G([enc, dec], ncu)
    while not rr.wraps(z_items(G), z_rnd(ncu)) or not all(rr.wraps(c.items(G), c.rnd(ncu)) for c in (enc, dec)):
        G += 1
    _set(qf)
    b = _sources(torch, qf, dec, G, SEED + 20)
    reps = []
    for cap in (0, 1):
        _set(qf, enc_blocks_per_cu=cap, encode_merged=1)
        rep, names = _encode(torch, qf, b)
        assert set(names) == {rr.kernel("N", k, r)}, names
        reps.append(rep)
    assert torch.equal(reps[0], reps[1]), "capped merged encode differs from the uncapped one"
    rep = reps[1]
    del reps
    _oracle_sample(oracle, b, rep, _sample(G, _part_bounds(dec.items, dec.rnd(ncu), G), SEED + 21))
    _erase(torch, b, rep, _own_e(dec, G, SEED + 22), SEED + 23)
    del rep
    ran = set()
    first = None
    for shared, fft in ((1, 1), (0, 1), (0, 0)):
        want = rr.synw_kernel(k, r, shared=shared, fft=fft)
        for cap in (0, 1):
            _set(qf, synw_shared=shared, fft_kernels=fft, dec_blocks_per_cu=cap)
            o = _decode(torch, qf, b)
            assert want in o.names, (shared, fft, cap, want, sorted(o.names))
            _check(torch, b, o)
            if first is None:
                first = o
            else:
                _same(torch, first, o, (shared, fft, cap))
                del o
        ran.add(want)
    assert len(ran) == 3, ran


def _tiled_inputs(torch, k, r, L, gens, max_rows, G):
    """The host arrays of run_decode for the base generations, repeated along
    G on the device: generation g is base generation g % len(gens)."""
    B = len(gens)
    rs = _r16(L) + 16
    rgs = max_rows * rs
    rows = np.zeros((B, rgs), np.uint8)
    ridx = np.zeros((B, max_rows), np.uint16)
    nrows = np.zeros(B, np.uint32)
    for g, (arr, rw, _) in enumerate(gens):
        nrows[g] = len(arr)
        ridx[g, : len(arr)] = arr
        for s in range(len(arr)):
            rows[g, s * rs: s * rs + L] = rw[s]
    sel = torch.arange(G, device="cuda") % B
    t_rows = torch.from_numpy(rows).cuda()[sel].reshape(-1)
    t_idx = torch.from_numpy(ridx.view(np.int16)).cuda()[sel].reshape(-1)
    t_n = torch.from_numpy(nrows.view(np.int32)).cuda()[sel].contiguous()
    return t_rows, t_idx, t_n, rs, rgs


@pytest.mark.parametrize("lanes", [1, 0])
def test_prepare_grid_rounds(qf, oracle, gpu_ctx, lanes):
    """The split-phase decode's acceptance pass on a grid capped by
    prepare_grid = 4: one generation per lane (k_decode_prepare_lu_lanes, G >=
    2,048: rounds of 512 generations) and one per wave (prepare_lanes = 0:
    rounds of 16), against the same call with prepare_grid = 0 and against the
    oracle-checked base of 251 generations (duplicates, short generations,
    repair indices out of range)."""
    import torch

    k, r, L, B = 64, 16, 48, 251
    max_rows = k + r + 4
    rng = np.random.default_rng(SEED + 30)
    src, gens = make_batch(oracle, rng, k, r, L, B, max_rows, dup_prob=0.03, trim_prob=0.05)
    for g in range(11, B, 37):           # a repair index past k + r: EINVAL
        arr, rows, rc = gens[g]
        if arr:
            arr = list(arr)
            arr[len(arr) // 2] = k + r + 3
            gens[g] = (arr, rows, rc)
    bad = {g for g in range(11, B, 37) if gens[g][0]}
    good = [g for g in range(B) if g not in bad]
    _set(qf, "default_1wave", prepare_lanes=lanes)
    base = run_decode(qf, k, r, L, B, max_rows, gens, False)
    check(oracle, k, L, src[good], [gens[g] for g in good],
          (np.concatenate([base[0][g * base[5]:(g + 1) * base[5]] for g in good]), base[1][good], base[2][good],
           base[3][good], base[4], base[5]), False)
    assert all(base[3][g] == -1 for g in bad) and {0, -1, -3} <= set(base[3].tolist())

    grid = 4
    rnd = rr.prepare_round(grid, bool(lanes))
    G = rr.tiled_G(rnd, B, at_least=2048)
    assert rr.wraps(G, rnd) and G >= 2048 and G % B
    t_rows, t_idx, t_n, rs, rgs = _tiled_inputs(torch, k, r, L, gens, max_rows, G)
    rrs, rec_gs, em = base[4], base[5], min(k, r)
    ctx = qf.default_context()
    outs = {}
    for pg in (grid, 0):
        _set(qf, "default_1wave", prepare_lanes=lanes, prepare_grid=pg)
        t_rec = torch.full((G * rec_gs + 64,), PAT, dtype=torch.uint8, device="cuda")
        t_recidx = torch.zeros(G * em, dtype=torch.int16, device="cuda")
        t_nrec = torch.zeros(G, dtype=torch.int32, device="cuda")
        t_status = torch.full((G,), 77, dtype=torch.int32, device="cuda")
        landed = torch.cuda.Event()
        landed.record()
        torch.cuda.synchronize()
        ctx.set_payload_wait(landed)      # the split phase: only then is the acceptance grid capped
        try:
            qf.decode_batch(t_rows, t_idx, t_rec, t_recidx, t_nrec, t_status, k, r, L, max_rows=max_rows,
                            row_stride=rs, rows_gen_stride=rgs, rec_row_stride=rrs, rec_gen_stride=rec_gs,
                            G=G, n_rows=t_n)
            _sync(torch, qf)
        finally:
            ctx.set_payload_wait(None)
        outs[pg] = (t_rec, t_recidx, t_nrec, t_status)
    for x, y in zip(outs[grid], outs[0]):
        assert torch.equal(x, y), "prepare_grid = 4 differs from the uncapped acceptance pass"
    rec, recidx, nrec, status = (t.cpu().numpy() for t in outs[grid])
    sel = np.arange(G) % B
    assert np.array_equal(status, base[3][sel]) and np.array_equal(nrec, base[2][sel])
    recidx = recidx.view(np.uint16).reshape(G, em)
    live = np.arange(em)[None, :] < nrec[:, None]
    assert np.array_equal(np.where(live, recidx, 0), np.where(live, base[1][sel], 0))
    recv = rec[: G * rec_gs].reshape(G, rec_gs)[:, : em * rrs].reshape(G, em, rrs)
    basev = base[0][: B * rec_gs].reshape(B, rec_gs)[:, : em * rrs].reshape(B, em, rrs)[sel]
    assert np.array_equal(recv[live], basev[live]), "recovered rows (to the row stride) differ from the base's"
    assert (recv[~live] == PAT).all()


def test_combine_slots_and_uniform_rounds(qf, oracle, gpu_ctx):
    """(16, 16) at L = 1,200 with bitsliced = 0, combine_bs = 0 and
    combine_split = 0: k_combine_uniform (encode) and k_combine_slots (decode)
    on grids of num_cus * occupancy blocks, sized for the occupancy's bound.
    The encode equals the bit-sliced encode of the same sources; the decode
    satisfies the round trip."""
    import torch

    case = rr.CASES["slots_uniform"]
    ncu = _ncu(torch)
    G = case.G(ncu)
    rnd = case.rnd(ncu)
    assert rr.wraps(case.items(G), rnd)
    general = dict(combine_split=0)
    _set(qf, "general", **general)
    b = _sources(torch, qf, case, G, SEED + 40)
    rep, names = _encode(torch, qf, b, zero_tail=False)
    pd = qf.default_context().option("encode_pd")
    assert set(names) == {f"k_combine_uniform<16,1,{pd}>"}, names
    _set(qf)
    rep_bs, names = _encode(torch, qf, b, zero_tail=False)
    assert set(names) <= {rr.kernel("E", case.k, case.r), rr.kernel("e", case.k, case.r)} and names, names
    assert torch.equal(rep, rep_bs), "general encode differs from the bit-sliced one"
    del rep_bs
    _oracle_sample(oracle, b, rep, _sample(G, _part_bounds(case.items, rnd, G), SEED + 41))
    _erase(torch, b, rep, _own_e(case, G, SEED + 42), SEED + 43)
    del rep
    _set(qf, "general", **general)
    o = _decode(torch, qf, b)
    assert "k_combine_slots<1>" in o.names and "k_combine_slots_split" not in o.names, o.names
    _check(torch, b, o)


# ---------------------------------------------------------------------------
# C. the second workspace chunk of the r > 16 decode (decode_cauchy_enc)
# ---------------------------------------------------------------------------
def _chunk_case(torch, qf, oracle, name, stage_kernel):
    case = rr.CASES[name]
    G, chunk = case.fixed_G, case.chunk
    assert G > chunk and G % chunk != 0
    _set(qf)
    b, _ = _round_trip_batch(torch, qf, oracle, case, G, [(0, chunk), (chunk, G)], seed=SEED + sum(name.encode()),
                             extra=(chunk - 1, chunk))
    o = _decode(torch, qf, b)
    # one launch of the syndrome stage per workspace chunk
    assert o.names.get(stage_kernel) == 2, (stage_kernel, o.names)
    _check(torch, b, o)


def test_decode_second_chunk_gather_path(qf, oracle, gpu_ctx):
    """(128, 20) at L = 1,200 (rows below 128 padded units: sources gathered,
    encode kernels, repairs XORed in), e = 20, G = 5,700 against chunks of
    5,667 generations: the records, bounds, slot maps, counts and rows of
    generations 5,667 .. 5,699 come through the g0 > 0 terms."""
    import torch

    _chunk_case(torch, qf, oracle, "chunk_gather", "k_gather_sources")


def test_decode_second_chunk_synw_path(qf, oracle, gpu_ctx):
    """(196, 59) at L = 2,040 (syndromes read through the slot map), own e over
    {3, 20, 40, 59} so that upper passes are skipped on both sides of the
    boundary, G = 8,900 against chunks of 8,886.  The full form is kept: every
    generation has its own 196 rows (3.6 GB), no shared row memory."""
    import torch

    _chunk_case(torch, qf, oracle, "chunk_synw", rr.synw_kernel(196, 59))


def test_decode_synw_off(qf, oracle, gpu_ctx):
    """decode_synw = 0 on long rows: the gather path instead of the slot-map
    syndrome kernels, bit-exact against the oracle."""
    k, r, L, G = 196, 59, 2040, 6
    rng = np.random.default_rng(SEED + 50)
    src, gens = make_batch(oracle, rng, k, r, L, G, k + r)
    ctx = qf.default_context()
    ran = {}
    for synw in (0, 1):
        _set(qf, decode_synw=synw)
        ctx.sync()
        ctx.profile(True)
        out = run_decode(qf, k, r, L, G, k + r, gens, False)
        ran[synw] = set(ctx.kernel_times())
        ctx.profile(False)
        check(oracle, k, L, src, gens, out, False)
    assert "k_gather_sources" in ran[0] and "k_xor_repairs" in ran[0], ran[0]
    assert not any(n.startswith("qf_cauchy_synw") for n in ran[0]), ran[0]
    assert rr.synw_kernel(k, r) in ran[1] and "k_gather_sources" not in ran[1], ran[1]


# ---------------------------------------------------------------------------
# B (continued). k_combine_rows_at through the received-frames calls
# ---------------------------------------------------------------------------
ROWS_AT = dict(k=8, mr=12, Lb=1200, B=251, extra=64)      # frame stride 16 + 1,200 + 64 = 1,280


def rows_at_base(oracle):
    """251 generations of 12 frame slots: systematic and coded rows, dependent
    ones, generations short of rank, payloads that end mid-unit (the sources
    end in zero tails, two slots of three carry the trimmed row)."""
    from tests import test_gpu_recv_inplace as RI

    k, mr, Lb, B = (ROWS_AT[x] for x in ("k", "mr", "Lb", "B"))
    rng = np.random.default_rng(SEED + 60)
    gs = RI.tailed_gens(oracle, rng, k, mr, Lb, B, p_sys=0.5, p_dep=0.25)
    rx, lens = RI.frame_gens(oracle, gs, extra=ROWS_AT["extra"])
    assert rx.fs == 1280
    return gs, rx, lens


def rows_at_recode_gens(gs, lens):
    """The rows as the recode reference (test_gpu_relay_inplace.check_oracle)
    takes them: zero padded to L, a unit vector for a systematic row."""
    out = []
    for g in range(gs.G):
        n = min(int(gs.n[g]), gs.mr)
        rows = np.zeros((n, gs.L), np.uint8)
        vecs = np.zeros((n, gs.k), np.uint8)
        for s in range(n):
            rows[s, : lens[g, s]] = gs.rows[g, s, : lens[g, s]]
            if gs.idx[g, s] < gs.k:
                vecs[s, gs.idx[g, s]] = 1
            else:
                vecs[s] = gs.coeffs[g, s]
        out.append(dict(n=n, rows=rows, vecs=vecs, len=lens[g, :n].astype(np.uint32)))
    return out


class _Rx:
    pass


def _tile_received(torch, rx, h, sel_np):
    """The frame buffer and the parsed header arrays of the base, repeated
    along G on the device (generation g is base generation sel[g])."""
    B, mr, k, fs = rx.G, rx.mr, rx.k, rx.fs
    sel = torch.from_numpy(sel_np).cuda()
    t = _Rx()
    t.G, t.mr, t.k, t.L, t.fs = len(sel_np), mr, k, rx.L, fs
    t.frames = rx.frames[sel_np]

    def rep(x, per):
        return x[: B * per].view(B, per)[sel].reshape(-1).contiguous()

    ht = dict(frames=rep(h["frames"], mr * fs), ro=rep(h["ro"], 4 * mr), rl=rep(h["rl"], 4 * mr),
              idx=rep(h["idx"], 2 * mr), co=rep(h["co"], mr * k), n=rep(h["n"], 4))
    return t, ht


def test_combine_rows_at_rounds(qf, oracle, gpu_ctx):
    """qf_decode_frames_dev and qf_recode_frames_dev (k_combine_rows_at on
    num_cus * occupancy blocks) over a base of 251 generations tiled along G
    past two rounds: every output of generation g equals the base's for
    g % 251, and the base equals the copy path, recv_ref and the recode
    reference.  (The launch splits a batch whose records exceed 2 GiB:
    g_max = 0x7FFFFFFF / coef_gen_stride is 8.9 M generations for this decode,
    240-byte records, and 6.4 M for the recode, 336-byte records; a batch that
    crosses it would need 100 GB of frames and is not built.)"""
    import torch

    from tests import test_gpu_recv_inplace as RI
    from tests import test_gpu_relay_inplace as R

    k, mr, Lb, B = (ROWS_AT[x] for x in ("k", "mr", "Lb", "B"))
    r, m = k, 6
    _set(qf)
    gs, rx, lens = rows_at_base(oracle)
    refs = RI.refs_of_gens(oracle, gs, lens)
    sts = [ref["status"] for ref in refs]
    assert {RI.OK, RI.ENOTREADY} <= set(sts) and sts.count(RI.OK) > B // 4, sts
    assert any(0 < f[:k].sum() < k for f in gs.flags), "no dependent row among the first k"
    assert (lens % 16 != 0).any() and (lens == Lb).any()
    h, out = RI.both_ways(qf, oracle, rx, r, refs)
    mix = R.seeded_mix(oracle, B, m, mr, SEED + 61)
    egens = rows_at_recode_gens(gs, lens)
    got = R.run_recode_frames(qf, rx, h, m, mix=mix)
    R.check_oracle(oracle, egens, mix, got, m, k, Lb)

    ncu = _ncu(torch)
    rnd = rr.occ_round(ncu)
    G = rr.gens_for(lambda g: rr.unit_waves(Lb, g), rnd, avoid=B)
    assert rr.wraps(rr.unit_waves(Lb, G), rnd) and G % B
    sel = np.arange(G) % B
    rx_t, h_t = _tile_received(torch, rx, h, sel)
    out_t = RI.run_inplace(qf, rx_t, h_t, r)
    for key, v in out.items():
        assert np.array_equal(out_t[key], v[sel]), f"decode_frames: {key} differs from the tiled base"
    got_t = R.run_recode_frames(qf, rx_t, h_t, m, mix=mix[sel])
    for name, a, b in zip(("payload", "vectors", "out_len", "status"), got_t, got):
        assert np.array_equal(a, b[sel]), f"recode_frames: {name} differs from the tiled base"
