"""qf_recode_batch on the MI355X, bit for bit against the CPU oracle.

A recoded payload row is a GF(2^8) matrix product of the mix matrix M (m x n)
with the n rows held, and its coefficient vector the same product with the
n x k matrix V of the held rows' vectors (unit rows, Cauchy rows, explicit
rows): both are oracle.encode(X, m, coeff=M).  The seeded mix is
oracle.fill_splitmix's stream."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENT = 0xA5
OK, EINVAL, ENOTREADY = 0, -1, -3


def _r16(x):
    return (x + 15) // 16 * 16


class Inputs:
    """Rows held by a relay, G generations: rows (G, max_rows, L), idx
    (G, max_rows), n (G,), coeffs (G, max_rows, k) or None (Cauchy rows of
    (k, r) for indices >= k)."""

    def __init__(self, k, r, L, rows, idx, n, coeffs):
        self.k, self.r, self.L = k, r, L
        self.rows, self.idx, self.n, self.coeffs = rows, np.asarray(idx, np.uint16), np.asarray(n, np.uint32), coeffs
        self.G, self.max_rows = rows.shape[0], rows.shape[1]

    def vectors(self, oracle, g):
        """V (n x k) of generation g; None when a coded row has no vector."""
        n = int(self.n[g])
        V = np.zeros((n, self.k), np.uint8)
        C = oracle.cauchy(self.k, self.r) if (self.coeffs is None and self.r) else None
        for s in range(n):
            i = int(self.idx[g, s])
            if i < self.k:
                V[s, i] = 1
            elif self.coeffs is not None:
                V[s] = self.coeffs[g, s]
            elif i - self.k < self.r:
                V[s] = C[i - self.k]
            else:
                return None
        return V


def make_inputs(rng, k, max_rows, L, G, kind, r=0, n=None):
    """kind: "sys" all systematic (distinct where max_rows <= k), "cauchy"
    indices k + j with implicit Cauchy rows, "explicit" coded rows with random
    vectors, "mixed" systematic (one index duplicated) and explicit rows."""
    rows = rng.integers(0, 256, (G, max_rows, L), dtype=np.uint8)
    idx = np.zeros((G, max_rows), np.uint16)
    coeffs = None
    for g in range(G):
        if kind == "sys":
            idx[g] = rng.permutation(max(k, max_rows))[:max_rows] % k
        elif kind == "cauchy":
            idx[g] = k + rng.integers(0, r, max_rows)
        elif kind == "explicit":
            idx[g] = k + rng.integers(0, 300, max_rows)
        else:
            coded = rng.random(max_rows) < 0.4
            idx[g] = np.where(coded, k + rng.integers(0, 40, max_rows), rng.integers(0, k, max_rows))
            if max_rows >= 2:
                idx[g, -1] = idx[g, 0] = rng.integers(0, k)   # a duplicated systematic index
    if kind in ("explicit", "mixed"):
        coeffs = rng.integers(0, 256, (G, max_rows, k), dtype=np.uint8)
        coeffs[:, :, 0] = 0            # zero coefficients take the log-form path's zero case
        if kind == "explicit":
            coeffs[0, 0] = 0           # and a whole zero vector
    n = np.full(G, max_rows, np.uint32) if n is None else np.asarray(n, np.uint32)
    return Inputs(k, r, L, rows, idx, n, coeffs)


def run_recode(qf, inp, m, *, mix=None, seed=0, out_rs=None, out_gap=0, pass_n=True):
    """-> out (G, m, L), vectors (G, m, k), status (G,).  Bytes the call must
    not write (row tails up to the stride, gaps between generations, the
    buffers' ends) are checked against a sentinel here, for every case."""
    import torch

    k, L, G, mr = inp.k, inp.L, inp.G, inp.max_rows
    rs = _r16(L) + 16
    rows = np.zeros((G, mr, rs), np.uint8)
    rows[:, :, :L] = inp.rows
    rows[:, :, L:] = 0x3C            # bytes past L of an input row must not reach the output
    out_rs = _r16(L) + 16 if out_rs is None else out_rs
    out_gs = m * out_rs + out_gap
    dev = "cuda"
    t_rows = torch.from_numpy(rows.reshape(-1)).to(dev)
    t_idx = torch.from_numpy(inp.idx.view(np.int16).reshape(-1)).to(dev)
    t_n = torch.from_numpy(inp.n.view(np.int32)).to(dev) if pass_n else None
    t_coef = torch.from_numpy(inp.coeffs.reshape(-1)).to(dev) if inp.coeffs is not None else None
    t_mix = torch.from_numpy(np.ascontiguousarray(mix, np.uint8).reshape(-1)).to(dev) if mix is not None else None
    t_out = torch.full((G * out_gs + 64,), SENT, dtype=torch.uint8, device=dev)
    t_oc = torch.full((G * m * k + 64,), SENT, dtype=torch.uint8, device=dev)
    t_st = torch.full((G + 4,), 77, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    qf.recode_batch(t_rows, t_idx, t_out, t_oc, t_st, k, m, L, r=inp.r, max_rows=mr, row_stride=rs,
                    rows_gen_stride=mr * rs, out_row_stride=out_rs, out_gen_stride=out_gs, G=G, n_rows=t_n,
                    row_coeffs=t_coef, mix=t_mix, seed=seed)
    qf.default_context().sync()
    out, oc, st = t_out.cpu().numpy(), t_oc.cpu().numpy(), t_st.cpu().numpy()
    assert (out[G * out_gs:] == SENT).all() and (oc[G * m * k:] == SENT).all() and (st[G:] == 77).all()
    og = out[: G * out_gs].reshape(G, out_gs)
    assert (og[:, m * out_rs:] == SENT).all(), "bytes after a generation's last row were written"
    orow = og[:, : m * out_rs].reshape(G, m, out_rs)
    assert (orow[:, :, L:] == SENT).all(), "bytes between L and out_row_stride were written"
    return orow[:, :, :L].copy(), oc[: G * m * k].reshape(G, m, k).copy(), st[:G].copy()


def seeded_mix(oracle, G, m, max_rows, seed):
    return oracle.fill_splitmix(G * m * max_rows, seed).reshape(G, m, max_rows)


def expected(oracle, inp, g, m, M):
    """(status, payload rows (m, L), vectors (m, k)) of generation g under mix M (m, max_rows)."""
    n = int(inp.n[g])
    zero = (np.zeros((m, inp.L), np.uint8), np.zeros((m, inp.k), np.uint8))
    if n == 0:
        return (ENOTREADY,) + zero
    if n > inp.max_rows:
        return (EINVAL,) + zero
    V = inp.vectors(oracle, g)
    if V is None:
        return (EINVAL,) + zero
    Mn = np.ascontiguousarray(M[:, :n])
    return OK, oracle.encode(np.ascontiguousarray(inp.rows[g, :n]), m, Mn), oracle.encode(V, m, Mn)


def check(oracle, inp, m, M, got, gens=None):
    out, oc, st = got
    for g in (range(inp.G) if gens is None else gens):
        est, erows, evec = expected(oracle, inp, g, m, M[g])
        assert st[g] == est, (g, st[g], est)
        assert np.array_equal(out[g], erows), f"payload of generation {g}"
        assert np.array_equal(oc[g], evec), f"coefficient vectors of generation {g}"


# k, max_rows, m, L, G, kind, r
PARITY = [
    (4, 3, 2, 16, 2, "mixed", 0),          # a relay holding fewer than k rows
    (16, 16, 1, 37, 5, "mixed", 0),        # tail unit
    (64, 64, 16, 1200, 5, "mixed", 0),     # 75 units per row: a wave spans two generations
    (32, 40, 17, 208, 5, "mixed", 0),      # second pass with one live output
    (32, 40, 33, 208, 5, "explicit", 0),
    (32, 40, 64, 208, 5, "mixed", 0),
    (255, 255, 16, 64, 2, "cauchy255", 1),  # k + r at the 256 limit
]


@pytest.mark.parametrize("k,max_rows,m,L,G,kind,r", PARITY)
def test_recode_parity(qf, oracle, k, max_rows, m, L, G, kind, r):
    rng = np.random.default_rng(k * 1000 + m)
    if kind == "cauchy255":
        # 253 distinct sources, a duplicate, and the one Cauchy repair (index 255) in the middle
        inp = make_inputs(rng, k, max_rows, L, G, "sys", r=r)
        inp.idx[:, 100] = k
        inp.idx[:, 7] = inp.idx[:, 200]
    else:
        inp = make_inputs(rng, k, max_rows, L, G, kind, r=r)
    seed = 0x1234 + m
    got = run_recode(qf, inp, m, seed=seed, pass_n=(k != 16))   # n_rows NULL: max_rows rows each
    check(oracle, inp, m, seeded_mix(oracle, G, m, max_rows, seed), got)


def test_recode_parity_many_generations(qf, oracle, gpu_ctx):
    """More wave-items than CUs: the ordinary payload kernel, not the split
    one.  An oracle sample of 16 seeded generations plus the first and last."""
    k, max_rows, m, L, G = 64, 64, 16, 1200, 300
    rng = np.random.default_rng(300)
    inp = make_inputs(rng, k, max_rows, L, G, "mixed")
    gpu_ctx.sync()
    gpu_ctx.profile(True)
    got = run_recode(qf, inp, m, seed=99)
    times = gpu_ctx.kernel_times()
    gpu_ctx.profile(False)
    assert times["k_recode_prepare"][0] == 1, times
    assert [n for n in times if n != "k_recode_prepare"] == ["k_combine_slots<1>"], times
    assert (got[2] == OK).all()
    sample = sorted({0, G - 1} | set(np.random.default_rng(7).choice(G, 16, replace=False).tolist()))
    assert len(sample) >= 16
    check(oracle, inp, m, seeded_mix(oracle, G, m, max_rows, 99), got, gens=sample)


def test_recode_long_rows_both_payload_kernels(qf, oracle, gpu_ctx, qf_opts):
    """Rows long enough for the bit-sliced payload kernel; the same call with
    combine_bs = 0 runs k_combine_slots.  Both equal the oracle."""
    k, max_rows, m, L, G = 32, 32, 5, 9000, 3
    rng = np.random.default_rng(9000)
    inp = make_inputs(rng, k, max_rows, L, G, "mixed")
    M = seeded_mix(oracle, G, m, max_rows, 5)
    want = [expected(oracle, inp, g, m, M[g]) for g in range(G)]
    for bs in (1, 0):
        qf_opts(combine_bs=bs)
        gpu_ctx.sync()
        gpu_ctx.profile(True)
        out, oc, st = run_recode(qf, inp, m, seed=5)
        times = gpu_ctx.kernel_times()
        gpu_ctx.profile(False)
        assert times["k_recode_prepare"][0] == 1, times
        payload = [n for n in times if n != "k_recode_prepare"]
        assert len(payload) == 1 and times[payload[0]][0] == 1, times
        if bs:
            assert payload[0].startswith("qf_combine_bs_r16"), times
        else:
            assert payload[0] == "k_combine_slots_split", times   # 3 x 563 units: under one item per CU
        for g in range(G):
            assert st[g] == want[g][0] == OK
            assert np.array_equal(out[g], want[g][1]) and np.array_equal(oc[g], want[g][2]), (bs, g)


def test_recode_profile_labels_short_rows(qf, gpu_ctx):
    """One k_recode_prepare and one payload launch per 16 outputs."""
    inp = make_inputs(np.random.default_rng(1), 16, 16, 100, 4, "sys")
    gpu_ctx.sync()
    gpu_ctx.profile(True)
    run_recode(qf, inp, 20, seed=1)
    times = gpu_ctx.kernel_times()
    gpu_ctx.profile(False)
    assert times == {"k_recode_prepare": (1, times["k_recode_prepare"][1]),
                     "k_combine_slots_split": (2, times["k_combine_slots_split"][1])}, times


@pytest.mark.parametrize("kind", ["sys", "cauchy", "explicit", "mixed"])
def test_recode_input_kinds(qf, oracle, kind):
    k, max_rows, m, L, G = 24, 20, 7, 45, 3
    inp = make_inputs(np.random.default_rng(len(kind)), k, max_rows, L, G, kind, r=8)
    got = run_recode(qf, inp, m, seed=42)
    assert (got[2] == OK).all()
    check(oracle, inp, m, seeded_mix(oracle, G, m, max_rows, 42), got)


def test_recode_per_generation_row_counts_and_statuses(qf, oracle):
    """n_rows of 0, 1, an odd count and max_rows; a generation with a coded
    index >= k + r and no coefficients; one with n > max_rows.  The bad
    generations get their status and zero outputs, their neighbours QF_OK and
    the right bytes."""
    k, r, max_rows, m, L, G = 16, 8, 20, 18, 53, 7
    rng = np.random.default_rng(5)
    inp = make_inputs(rng, k, max_rows, L, G, "cauchy", r=r, n=[max_rows, 0, 1, 13, max_rows, max_rows + 1, 7])
    inp.idx[:, 0] = np.arange(G) % k           # a systematic row first
    inp.idx[4, 9] = k + r                      # generation 4: no Cauchy row for this index
    inp.idx[6, 12] = k + r + 5                 # past n_rows[6] = 7: not looked at
    M = seeded_mix(oracle, G, m, max_rows, 11)
    got = run_recode(qf, inp, m, seed=11)
    assert list(got[2]) == [OK, ENOTREADY, OK, OK, EINVAL, EINVAL, OK]
    for g in (1, 4, 5):
        assert not got[0][g].any() and not got[1][g].any()
    check(oracle, inp, m, M, got)


def test_recode_explicit_mix_equals_seeded_and_identity(qf, oracle):
    k, max_rows, m, L, G = 16, 12, 12, 80, 3
    rng = np.random.default_rng(8)
    inp = make_inputs(rng, k, max_rows, L, G, "mixed")
    M = seeded_mix(oracle, G, m, max_rows, 77)
    seeded = run_recode(qf, inp, m, seed=77)
    explicit = run_recode(qf, inp, m, mix=M, seed=123)      # the seed is ignored with a mix
    for a, b in zip(seeded, explicit):
        assert np.array_equal(a, b)
    check(oracle, inp, m, M, explicit)
    # identity mix: the inputs and their vectors come back unchanged
    eye = np.broadcast_to(np.eye(m, max_rows, dtype=np.uint8), (G, m, max_rows))
    out, oc, st = run_recode(qf, inp, m, mix=eye)
    assert (st == OK).all()
    assert np.array_equal(out, inp.rows)
    for g in range(G):
        assert np.array_equal(oc[g], inp.vectors(oracle, g))


def test_recode_untouched_bytes_with_wide_strides(qf, oracle):
    """Output rows 48 bytes apart from their end and 80 bytes between
    generations: run_recode checks every byte outside the m x L outputs."""
    inp = make_inputs(np.random.default_rng(3), 8, 9, 33, 3, "mixed")
    got = run_recode(qf, inp, 17, seed=3, out_rs=96, out_gap=80)
    check(oracle, inp, 17, seeded_mix(oracle, 3, 17, 9, 3), got)


def test_recode_call_level_errors(qf, gpu_ctx):
    import torch

    from quicfuscate_amd import _lib as L

    inp = make_inputs(np.random.default_rng(2), 8, 8, 32, 1, "sys")
    t = lambda n, dt=torch.uint8: torch.zeros(n, dtype=dt, device="cuda")   # noqa: E731
    rows, idx, out, oc, st = t(8 * 48), t(8, torch.int16), t(65 * 48), t(65 * 256), t(1, torch.int32)

    def status(k=8, m=4, Lb=32, r=0, max_rows=8, rs=48, ors=48):
        try:
            qf.recode_batch(rows, idx, out, oc, st, k, m, Lb, r=r, max_rows=max_rows, row_stride=rs,
                            rows_gen_stride=8 * 48, out_row_stride=ors, out_gen_stride=64 * 48, G=1)
        except qf.QfError as e:
            return e.status
        return 0

    assert status() == 0
    assert status(m=65) == L.QF_EINVAL and status(m=0) == L.QF_EINVAL
    assert status(k=256) == L.QF_EINVAL
    assert status(Lb=0) == L.QF_EINVAL
    assert status(Lb=40, rs=32) == L.QF_EINVAL          # a stride shorter than L
    assert status(ors=40) == L.QF_EINVAL                # not 16-byte aligned
    assert status(k=200, r=57) == L.QF_ERANGE
    assert status(k=200, r=56) == 0
    gpu_ctx.sync()


# ---------------------------------------------------------------------------
# Round trips through the existing encode and decode
# ---------------------------------------------------------------------------
def _decode_rows(qf, k, L, rows, vecs):
    """qf_decode_batch over coded rows alone (indices k + j, explicit vectors):
    rows (G, n, L), vecs (G, n, k) -> (status, recovered sources (G, k, L))."""
    import torch

    G, n, _ = rows.shape
    rs = _r16(L)
    padded = np.zeros((G, n, rs), np.uint8)
    padded[:, :, :L] = rows
    idx = np.broadcast_to(k + np.arange(n, dtype=np.uint16), (G, n)).copy()
    dev = "cuda"
    t_rows = torch.from_numpy(padded.reshape(-1)).to(dev)
    t_idx = torch.from_numpy(idx.view(np.int16).reshape(-1)).to(dev)
    t_coef = torch.from_numpy(np.ascontiguousarray(vecs).reshape(-1)).to(dev)
    t_rec = torch.zeros(G * k * rs, dtype=torch.uint8, device=dev)
    t_ri = torch.zeros(G * k, dtype=torch.int16, device=dev)
    t_nrec = torch.zeros(G, dtype=torch.int32, device=dev)
    t_st = torch.full((G,), 77, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    qf.decode_batch(t_rows, t_idx, t_rec, t_ri, t_nrec, t_st, k, n, L, max_rows=n, row_stride=rs,
                    rows_gen_stride=n * rs, rec_row_stride=rs, rec_gen_stride=k * rs, G=G, row_coeffs=t_coef)
    qf.default_context().sync()
    assert (t_nrec.cpu().numpy() == k).all()
    assert (t_ri.cpu().numpy().reshape(G, k) == np.arange(k)).all()
    return t_st.cpu().numpy(), t_rec.cpu().numpy().reshape(G, k, rs)[:, :, :L]


def _pick_seed(oracle, inp, m, first):
    """The first seed >= `first` under which the oracle decodes every
    generation from its first k recoded rows (a random k x k matrix over
    GF(2^8) is singular with probability about 0.4 %).  CPU only."""
    k = inp.k
    for seed in range(first, first + 50):
        M = seeded_mix(oracle, inp.G, m, inp.max_rows, seed)
        sts = []
        for g in range(inp.G):
            _, erows, evec = expected(oracle, inp, g, m, M[g])
            sts.append(oracle.decode(k, k + np.arange(m), erows, evec)[0])
        if all(s == OK for s in sts):
            return seed, sts
    raise AssertionError("no seed decodes every generation")


def test_recode_round_trip_two_hops(qf, oracle):
    """Encode (16, 8), drop 4 sources, recode the 20 held rows into 18,
    decode the recoded rows alone; then recode those 18 into 17 (a second
    hop, explicit vectors) and decode again.  Both give the sources."""
    import torch

    k, r, L, G = 16, 8, 100, 4
    rng = np.random.default_rng(16)
    src = rng.integers(0, 256, (G, k, L), dtype=np.uint8)
    rs = _r16(L)
    sp = np.zeros((G, k, rs), np.uint8)
    sp[:, :, :L] = src
    t_src = torch.from_numpy(sp.reshape(-1)).cuda()
    t_rep = torch.zeros(G * r * rs, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    qf.encode_batch(t_src, t_rep, k, r, L, src_row_stride=rs, src_gen_stride=k * rs, rep_row_stride=rs,
                    rep_gen_stride=r * rs, G=G)
    qf.default_context().sync()
    rep = t_rep.cpu().numpy().reshape(G, r, rs)[:, :, :L]
    held_rows = np.zeros((G, 20, L), np.uint8)
    held_idx = np.zeros((G, 20), np.uint16)
    for g in range(G):
        keep = sorted(rng.choice(k, k - 4, replace=False).tolist())
        arr = keep + [k + j for j in range(r)]
        rng.shuffle(arr)
        held_idx[g] = arr
        held_rows[g] = np.stack([src[g, a] if a < k else rep[g, a - k] for a in arr])
    hop1 = Inputs(k, r, L, held_rows, held_idx, np.full(G, 20), None)
    seed1, sts = _pick_seed(oracle, hop1, 18, 1)
    assert all(s == OK for s in sts)
    out1, vec1, st1 = run_recode(qf, hop1, 18, seed=seed1)
    assert (st1 == OK).all()
    check(oracle, hop1, 18, seeded_mix(oracle, G, 18, 20, seed1), (out1, vec1, st1))
    st, rec = _decode_rows(qf, k, L, out1, vec1)
    assert (st == OK).all() and np.array_equal(rec, src)
    # second hop
    hop2 = Inputs(k, 0, L, out1, np.broadcast_to(k + np.arange(18, dtype=np.uint16), (G, 18)).copy(),
                  np.full(G, 18), vec1)
    seed2, sts = _pick_seed(oracle, hop2, 17, 100)
    assert all(s == OK for s in sts)
    out2, vec2, st2 = run_recode(qf, hop2, 17, seed=seed2)
    assert (st2 == OK).all()
    st, rec = _decode_rows(qf, k, L, out2, vec2)
    assert (st == OK).all() and np.array_equal(rec, src)


def test_recoder_packets_through_the_wire_into_decoder(qf, oracle):
    """Recoder -> Packet.to_raw / from_raw -> Decoder recovers the k packets."""
    k, n, L, cap = 8, 12, 50, 12
    rng = np.random.default_rng(88)
    src = rng.integers(0, 256, (k, L), dtype=np.uint8)
    enc = qf.Encoder(k, n, max_len=64)
    for i in range(k):
        enc.add_source_packet(qf.Packet(i, bytearray(src[i].tobytes()), L, True))
    repairs = enc.generate_repairs(0, n - k)
    assert len(repairs) == n - k
    held = [qf.Packet(i, bytearray(src[i].tobytes()), L, True) for i in (6, 1, 3, 0, 7, 4)] + repairs
    rec = qf.Recoder(k, 64, cap)
    assert rec.recode(3, 1) == []
    for p in held:
        rec.add_packet(p)
    with pytest.raises(qf.QfError):
        rec.add_packet(qf.Packet(99, bytearray(L), L, False))      # a coded packet without coefficients
    # the seed under which the oracle decodes the first k recoded packets
    idx = np.zeros((1, cap), np.uint16)
    co = np.zeros((1, cap, k), np.uint8)
    rows = np.zeros((1, cap, L), np.uint8)
    for s, p in enumerate(held):
        idx[0, s] = p.id % k if p.is_systematic else k
        rows[0, s] = np.frombuffer(p.payload(), np.uint8)
        if not p.is_systematic:
            co[0, s] = np.frombuffer(p.coefficients, np.uint8)
    inp = Inputs(k, 0, L, rows, idx, [len(held)], co)
    count = 10
    seed, sts = _pick_seed(oracle, inp, count, 1)
    assert sts == [OK]
    pkts = rec.recode(count, seed, first_id=1000)
    assert len(pkts) == count
    _, erows, evec = expected(oracle, inp, 0, count, seeded_mix(oracle, 1, count, cap, seed)[0])
    dec = qf.Decoder(k, max_len=64)
    done = False
    for j, p in enumerate(pkts):
        assert not p.is_systematic and p.coeff_len == k and p.id == 1000 + j and p.len == L
        assert p.payload() == erows[j].tobytes() and p.coefficients == evec[j].tobytes()
        q = qf.Packet.from_raw(p.id, p.to_raw())
        assert not q.is_systematic and q.coefficients == p.coefficients and q.payload() == p.payload()
        done = dec.add_packet(q)
        if done:
            assert j == k - 1
            break
    assert done and dec.is_decoded
    got = dec.get_decoded_packets()
    assert len(got) == k
    for i, p in enumerate(got):
        assert bytes(p.data[:L]) == src[i].tobytes(), i
