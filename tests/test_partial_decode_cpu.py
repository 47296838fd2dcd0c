"""The partial decode without a device: both calls are exported, declared and
bound with the header's arities, a NULL context or shape fails before any
device work, the Python mirrors check every buffer before the library sees a
pointer, and the model the device tests compare with (tests/partial_ref.py)
agrees with recv_ref.decode_ref (the oracle's decode) at rank k and, below it,
delivers true sources only and leaves out only sources that the rows do not
determine.  CPU only."""
import ctypes
import re

import numpy as np
import pytest

from quicfuscate_amd import _lib as L
from tests import partial_ref as P
from tests import rank_ref, recv_ref

DENSE, LISTED = "qf_decode_partial_frames_dev", "qf_decode_partial_frames_sel_dev"


@pytest.mark.parametrize("name", [DENSE, LISTED])
def test_symbol_is_exported_declared_and_bound(name):
    assert name in L.header_symbols()
    assert name in L._SIGS
    assert hasattr(L._lib(), name)


@pytest.mark.parametrize("name, mirrored", [(DENSE, "qf_decode_frames_dev"), (LISTED, "qf_decode_frames_sel_dev")])
def test_signature_has_the_header_argument_count(name, mirrored):
    txt = re.sub(r"/\*.*?\*/", " ", L.HEADER.read_text(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", txt, flags=re.S)
    assert m
    assert len(L._SIGS[name][1]) == len(m.group(1).split(",")) == 16
    # the same pointers in the same order as the call it mirrors
    assert L._SIGS[name] == L._SIGS[mirrored]
    m2 = re.search(r"\bint\s+" + mirrored + r"\s*\((.*?)\)\s*;", txt, flags=re.S)
    assert re.sub(r"\s+", " ", m.group(1)).strip() == re.sub(r"\s+", " ", m2.group(1)).strip()


def test_abi_version_stays_1():
    assert re.search(r"#define\s+QF_ABI_VERSION\s+1\b", L.HEADER.read_text())


def test_null_context_shape_or_list_fails_before_any_device_work():
    lib = L._lib()
    sh = L.DecodeFramesShape(4, 4, 16, 4, 0, 0, 128, 16, 64)
    nulls = [None] * 13
    fake = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    assert lib.qf_decode_partial_frames_dev(None, ctypes.byref(sh), 1, *nulls) == L.QF_EINVAL
    assert lib.qf_decode_partial_frames_dev(fake, None, 1, *nulls) == L.QF_EINVAL
    sel = L.GenSel(None, None, 1, 1)
    assert lib.qf_decode_partial_frames_sel_dev(None, ctypes.byref(sh), ctypes.byref(sel), *nulls) == L.QF_EINVAL
    assert lib.qf_decode_partial_frames_sel_dev(fake, None, ctypes.byref(sel), *nulls) == L.QF_EINVAL
    assert lib.qf_decode_partial_frames_sel_dev(fake, ctypes.byref(sh), None, *nulls) == L.QF_EINVAL
    # a list without entries (sel_dev NULL) is refused before the context is touched
    assert lib.qf_decode_partial_frames_sel_dev(fake, ctypes.byref(sh), ctypes.byref(sel), *nulls) == L.QF_EINVAL


@pytest.mark.parametrize("listed", [False, True])
def test_mirror_rejects_undersized_buffers(listed):
    import torch

    from quicfuscate_amd import fec

    k, r, n, Lb, G = 16, 6, 20, 100, 3
    Gs = 5 if listed else G          # the listed call's inputs hold G_src generations
    fs, rrs = 144, 112
    src = torch.zeros(Gs * n * fs, dtype=torch.uint8)
    off = torch.zeros(Gs * n, dtype=torch.int32)
    ln = torch.zeros(Gs * n, dtype=torch.int32)
    idx = torch.zeros(Gs * n, dtype=torch.int16)
    co = torch.zeros(Gs * n * k, dtype=torch.uint8)
    rec = torch.zeros(G * r * rrs, dtype=torch.uint8)
    ri = torch.zeros(G * r, dtype=torch.int16)
    nrec = torch.zeros(G, dtype=torch.int32)
    st = torch.zeros(G, dtype=torch.int32)
    sel = torch.zeros(G, dtype=torch.int32)
    kw = dict(max_rows=n, src_gen_stride=n * fs, rec_row_stride=rrs, rec_gen_stride=r * rrs)

    def call(src=src, off=off, ln=ln, idx=idx, co=co, rec=rec, ri=ri, nrec=nrec, st=st, sel=sel, n_sel=None,
             **extra):
        if listed:
            fec.decode_partial_frames_sel(sel, n_sel, src, off, ln, idx, co, rec, ri, nrec, st, k, r, Lb, n_max=G,
                                          G_src=Gs, **kw, **extra)
        else:
            fec.decode_partial_frames(src, off, ln, idx, co, rec, ri, nrec, st, k, r, Lb, G=G, **kw, **extra)

    with pytest.raises(ValueError, match="src"):
        call(src=src[:-1])
    with pytest.raises(ValueError, match="row_off"):
        call(off=off[:-1])
    with pytest.raises(ValueError, match="row_len"):
        call(ln=ln[:-1])
    with pytest.raises(ValueError, match="row_index"):
        call(idx=idx[:-1])
    with pytest.raises(ValueError, match="row_coeffs"):
        call(co=co[:-1])
    # the last recovered row needs only L of its stride
    with pytest.raises(ValueError, match="rec:"):
        call(rec=rec[: (G * r - 1) * rrs + Lb - 1])
    with pytest.raises(ValueError, match="rec_index"):
        call(ri=ri[:-1])
    with pytest.raises(ValueError, match="n_rec"):
        call(nrec=nrec[:-1])
    with pytest.raises(ValueError, match="status"):
        call(st=st[:-1])
    with pytest.raises(ValueError, match="n_rows"):
        call(n_rows=torch.zeros(Gs - 1, dtype=torch.int32))
    with pytest.raises(ValueError, match="rank"):
        call(rank=torch.zeros(G - 1, dtype=torch.int32))
    with pytest.raises(ValueError, match="innovative"):
        call(innovative=torch.zeros(G * n - 1, dtype=torch.uint8))
    with pytest.raises(ValueError, match="src_slot"):
        call(src_slot=torch.zeros(G * k - 1, dtype=torch.int16))
    if listed:
        with pytest.raises(ValueError, match="sel"):
            call(sel=sel[:-1])
        with pytest.raises(ValueError, match="n_sel"):
            call(n_sel=torch.zeros(0, dtype=torch.int32))


def test_model_equals_the_full_decode_at_rank_k(oracle):
    """The planted arrival orders of the in-place receive tests, all of rank k:
    the model's every output is recv_ref.decode_ref's (the oracle's decode)."""
    k, Lb = 16, 100
    names, src, idx, co, V, rows = recv_ref.plant(oracle, np.random.default_rng(77), k, Lb)
    assert len(names) >= 6
    for g, name in enumerate(names):
        lens = [recv_ref.trimmed_len(rows[g, s]) if s % 3 else Lb for s in range(24)]
        pay = [rows[g, s, : lens[s]].tobytes() for s in range(24)]
        for r in (k, 3):
            full = recv_ref.decode_ref(oracle, k, r, Lb, idx[g], co[g], pay)
            part = P.partial_ref(k, r, Lb, idx[g], co[g], pay)
            assert part["status"] == full["status"], (name, r)
            assert part["rank"] == full["rank"] == k and np.array_equal(part["flags"], full["flags"]), name
            assert part["D"] == full["erased"], name
            assert np.array_equal(part["rec"], full["rec"]), name
            if full["status"] == recv_ref.OK:
                assert np.array_equal(part["src_slot"], full["src_slot"]), name
                assert np.array_equal(part["rec"], src[g][part["D"]]), name
            else:
                # the full decode reports no slot for a generation that is not QF_OK
                assert full["status"] == recv_ref.EINVAL and (part["src_slot"] == P.NONE16).all(), name
    # the encoder of this module against the oracle's
    assert np.array_equal(P.encode_rows(V[0], src[0]), rows[0])


def _check_incomplete(gen, ref, name):
    V = gen.V[: gen.n]
    flags, rank = rank_ref.innovative(V) if gen.n else (np.zeros(0, np.uint8), 0)
    assert ref["rank"] == rank and np.array_equal(ref["flags"], flags), name
    assert ref["status"] == (P.OK if rank == gen.k else P.ENOTREADY), name
    S = {int(gen.idx[s]) for s in np.flatnonzero(flags) if gen.idx[s] < gen.k}
    assert {i for i in range(gen.k) if ref["src_slot"][i] != P.NONE16} == S, name
    for i in S:
        s = int(ref["src_slot"][i])
        assert flags[s] and gen.idx[s] == i, name
        assert gen.payloads()[s] == gen.src[i, : int(gen.lens[s])].tobytes() and not gen.src[i, int(gen.lens[s]):].any()
    assert not S & set(ref["D"]) and ref["D"] == sorted(ref["D"]), name
    # every delivered row is the true source ...
    assert np.array_equal(ref["rec"], gen.src[ref["D"]]), name
    # ... and every source left out is one the rows do not determine
    for i in range(gen.k):
        if i in S or i in ref["D"]:
            assert gen.n == 0 or P.span_rank_with(V, i) == rank, (name, i)
        else:
            assert gen.n == 0 or P.span_rank_with(V, i) == rank + 1, (name, i)


def test_model_on_the_planted_incomplete_generations(oracle):
    k, Lb = 16, 100
    rng = np.random.default_rng(5)
    seen_both = [0, 0]
    for name, (vecs, det, undet) in P.planted(rng, k).items():
        gen = P.Gen(rng, k, Lb, vecs)
        ref = gen.ref(k)
        _check_incomplete(gen, ref, name)
        assert ref["D"] == det, name
        assert not set(undet) & set(ref["D"]), name
        seen_both[0] += len(det)
        seen_both[1] += len(undet)
        offs = np.arange(len(vecs), dtype=np.uint32) * 112
        P.check_records(ref, offs, gen.lens, max(len(vecs), 1) * 112)
    assert min(seen_both) > 0
    ref = P.Gen(rng, k, Lb, P.planted(rng, k)["systematic rows only"][0]).ref(k)
    assert ref["bound"] == 0 and ref["recorded"] == [] and (ref["src_slot"] != P.NONE16).sum() == 12
    # only the rows that some output uses are recorded
    vecs = [P.unit(k, i) for i in range(12)] + [P.over(rng, k, [0, 1, 12]), P.over(rng, k, [2, 13, 14])]
    ref = P.Gen(rng, k, Lb, vecs).ref(k)
    assert ref["D"] == [12] and ref["recorded"] == [0, 1, 12]


def test_model_on_random_generations_of_mixed_rank(oracle):
    rng = np.random.default_rng(9)
    ranks = set()
    for t in range(60):
        k = int(rng.choice([1, 5, 16, 33]))
        n = int(rng.integers(0, 2 * k + 1))
        vecs = []
        for s in range(n):
            kind = rng.integers(0, 4)
            if kind < 2:
                vecs.append(P.unit(k, int(rng.integers(0, k))))
            elif kind == 2:
                vecs.append(P.over(rng, k, rng.choice(k, int(rng.integers(1, min(k, 4) + 1)), replace=False).tolist()))
            else:
                vecs.append(rng.integers(0, 256, k, dtype=np.uint8))
        gen = P.Gen(rng, k, 40, vecs)
        ref = gen.ref(k)
        _check_incomplete(gen, ref, t)
        P.check_records(ref, np.arange(n, dtype=np.uint32) * 48, gen.lens, max(n, 1) * 48)
        ranks.add(ref["rank"] == k)
    assert ranks == {True, False}


def test_loop_model_holds_the_cases_the_device_test_is_about(oracle):
    """The stream of the device loop test under the model alone: generations are displaced incomplete,
    some with sources that only their coded rows determine, others complete, and a flush is left."""
    from tests import test_gpu_partial_decode as G

    src, stream, polls, flush = G.loop_model()
    saved, completed = {}, {}
    for poll, q in enumerate(polls):
        for s, g, ref in q.evicted:
            have = sorted({i for i in range(G.K_LOOP) if ref["src_slot"][i] != P.NONE16} | set(ref["D"]))
            assert ref["status"] == P.ENOTREADY and np.array_equal(ref["rec"], src[g][ref["D"]])
            saved[g] = (have, len(ref["D"]))
        for s, g in q.done:
            completed[g] = poll
    assert flush and sum(len(q.evicted) for q in polls) >= 5
    for s, g, ref in flush:
        saved[g] = (sorted({i for i in range(G.K_LOOP) if ref["src_slot"][i] != P.NONE16} | set(ref["D"])), len(ref["D"]))
    assert sorted(list(saved) + list(completed)) == [g for g in range(G.GENS_LOOP) if stream[g]]
    assert len(set(saved) & set(completed)) == 0
    G.check_loop_stats(saved, completed)


def test_model_statuses(oracle):
    k, Lb = 4, 8
    rng = np.random.default_rng(4)
    co = rng.integers(1, 256, (6, k), dtype=np.uint8)
    pay = [bytes(Lb)] * 6
    assert P.partial_ref(k, k, Lb, [], co[:0], [])["status"] == P.ENOTREADY
    assert P.partial_ref(k, k, Lb, [0, 1, 0, 1], co[:4], pay[:4])["status"] == P.ENOTREADY
    # a coded index with index - k >= 256: rank 0 and no flags, as the filter reports it
    ref = P.partial_ref(k, k, Lb, [0, 1, 2, k + 256], co[:4], pay[:4])
    assert ref["status"] == P.EINVAL and ref["rank"] == 0 and not ref["flags"].any()
    # more determined sources than min(k, r): the vectors still give rank and flags
    ref = P.partial_ref(k, 1, Lb, [k, k + 1, 0, 1], co[:4], pay[:4])
    assert ref["status"] == P.EINVAL and ref["rank"] == k and ref["D"] == []
    # the row rules
    for offs, lens in (([0, 8], [8, 8]), ([0, 16], [8, 9]), ([0, 32], [8, 8])):
        ref = P.partial_ref(k, k, Lb, [0, 1], co[:2], [bytes(n) for n in lens], np.array(offs), 32 + 7)
        assert ref["status"] == P.EINVAL and ref["rank"] == 2 and (ref["src_slot"] == P.NONE16).all()
