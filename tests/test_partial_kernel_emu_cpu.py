"""k_partial_prepare without a device: the kernel's own source, compiled for
the host behind tests/kernel_emu (64 lanes as 64 threads that meet at the
wave's collectives), as a stand-alone program under the host address and
undefined-behaviour sanitizers with every buffer and the LDS block at its exact
size, over the shapes of the device test.  Its statuses, lists and counts equal
tests/partial_ref.py's, and its pair records keep the contract that holds
k_combine_rows_at inside its buffers (qf_kernels.h, PrepareArgs): a fault there
is a GPU fault, so it is checked here first.  A model of the payload pass over
those records gives the sources.  CPU only."""
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import partial_ref as P
from tests import rank_ref
from tests import test_gpu_partial_decode as D

REPO = Path(__file__).resolve().parents[1]
CSRC = REPO / "quicfuscate_amd" / "csrc"
EMU = REPO / "tests" / "kernel_emu"
LDS_DECL = "    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];\n"


def _clangxx():
    for cand in ("/opt/rocm/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++")):
        if cand and Path(cand).exists():
            return cand
    raise RuntimeError("no host C++ compiler")


@pytest.fixture(scope="module")
def emu(tmp_path_factory, oracle):
    d = tmp_path_factory.mktemp("partial_emu")
    text = (CSRC / "qf_partial.hip").read_text()
    assert text.count(LDS_DECL) == 1, "the kernel's dynamic LDS declaration has changed"
    (d / "qf_partial_emu.inc").write_text(text.replace(LDS_DECL, "    uint8_t* lds = emu_lds;\n"))
    exe = d / "partial_prepare_emu"
    cmd = [_clangxx(), "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           f"-I{d}", f"-I{EMU}", f"-I{CSRC}", f"-I{REPO / 'include'}", "-pthread",
           str(EMU / "partial_prepare_main.cpp"), "-o", str(exe)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    return exe


def run_emu(exe, b, r):
    """The kernel over a device-test Batch with the model's flags -> the model's references."""
    k, mr, G, Lb = b.k, b.mr, b.G, b.L
    em = min(k, r)
    passes = (em + 15) // 16
    stride = ((min(k, mr) + 1) // 2 + 1) * 48
    refs = b.refs(r)
    e, lg = rank_ref._tables()
    explog = np.zeros(768, np.uint8)
    m = min(len(e), 512)
    explog[:m] = e[:m]
    explog[512:] = lg[:256]
    flags = np.zeros((G, mr), np.uint8)
    for g, ref in enumerate(refs):
        flags[g, : len(ref["flags"])] = ref["flags"]
    fin, fout = exe.parent / "in.bin", exe.parent / "out.bin"
    with open(fin, "wb") as f:
        f.write(struct.pack("<8I2Q", k, em, mr, G, Lb, passes, 256, 0, b.gs, stride))
        for a in (explog, b.idx, b.n, b.co, flags, b.off, b.len):
            f.write(np.ascontiguousarray(a).tobytes())
    res = subprocess.run([str(exe), str(fin), str(fout)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    raw = fout.read_bytes()
    pos = 0

    def take(n, dt):
        nonlocal pos
        a = np.frombuffer(raw, dt, n, pos)
        pos += n * np.dtype(dt).itemsize
        return a

    st, nout, bound, minlen = take(G, np.int32), take(G, np.uint32), take(G, np.uint32), take(G, np.uint32)
    ri = take(G * em, np.uint16).reshape(G, em)
    slot = take(G * k, np.uint16).reshape(G, k)
    coef = take(max(passes, 1) * G * stride, np.uint8).reshape(max(passes, 1), G, stride)
    assert pos == len(raw)
    mul = P.mul_table()
    npairs = stride // 48
    for g, ref in enumerate(refs):
        nd, nb = len(ref["D"]), int(bound[g])
        assert st[g] == ref["status"] and nout[g] == nd, (g, st[g], ref["status"], nout[g], ref["D"])
        assert ri[g, :nd].tolist() == ref["D"] and (ri[g, nd:] == 0xCCCC).all(), g
        assert np.array_equal(slot[g], ref["src_slot"]), g
        assert nb == ref["bound"] and minlen[g] == ref["min_len"], (g, nb, ref["bound"], minlen[g], ref["min_len"])
        rec = np.zeros((nd, Lb), np.uint8)
        for ps in range(passes):
            pairs = coef[ps, g].reshape(npairs, 48)
            head = pairs[:, :16].copy().view(np.uint32)
            offs, lens = head[:, :2].reshape(-1).tolist(), head[:, 2:].reshape(-1).tolist()
            cf = pairs[:, 16:].reshape(2 * npairs, 16)
            # the recorded rows, in arrival order; behind them zero records at the last one's offset
            assert offs[:nb] == [int(b.off[g, s]) for s in ref["recorded"]], (g, ps)
            assert lens[:nb] == [int(b.len[g, s]) for s in ref["recorded"]], (g, ps)
            last = offs[nb - 1] if nb else 0
            assert all(o == last for o in offs[nb:]) and not any(lens[nb:]) and not cf[nb:].any(), (g, ps)
            for t in range(2 * npairs):
                # every unit the payload pass may load: the row's own, and on the path without masks the
                # units below min_len of every record a lane can reach
                assert offs[t] % 16 == 0 and offs[t] + 16 * ((lens[t] + 15) // 16) <= b.gs, (g, ps, t)
                assert offs[t] + int(minlen[g]) // 16 * 16 <= b.gs, (g, ps, t)
                assert t >= nb or lens[t] >= minlen[g], (g, ps, t)
            for t in range(nb):
                row = np.zeros(Lb, np.uint8)
                row[: lens[t]] = b.src[g, offs[t]: offs[t] + lens[t]]
                for q in range(16):
                    if ps * 16 + q < nd:
                        rec[ps * 16 + q] ^= mul[int(cf[t, q])][row]
                    else:
                        assert cf[t, q] == 0, (g, ps, t, q)
        assert np.array_equal(rec, ref["rec"]) and np.array_equal(rec, b.gens[g].src[ref["D"]]), g
    return refs


def test_planted_and_boundary_generations(emu):
    rng = np.random.default_rng(5)
    run_emu(emu, D.Batch([P.Gen(rng, 16, 100, vecs) for vecs, _, _ in P.planted(rng, 16).values()]), 16)
    for k in (64, 65):
        rng = np.random.default_rng(k)
        gens = [D.determined_gen(rng, k, 100, k - 20, 6, n_loose=4)[0], D.determined_gen(rng, k, 100, k - 1, 1)[0],
                D.determined_gen(rng, k, 100, 0, 0, n_dense=k - 1)[0], D.determined_gen(rng, k, 100, k - 9, 3, n_loose=3)[0]]
        run_emu(emu, D.Batch(gens), 16)
    for nd in (16, 17):
        rng = np.random.default_rng(nd)
        refs = run_emu(emu, D.Batch([D.determined_gen(rng, 64, 100, 40, nd, n_loose=2)[0],
                                     D.determined_gen(rng, 64, 100, 40, 3)[0]]), 32)
        assert len(refs[0]["D"]) == nd
    rng = np.random.default_rng(3)
    refs = run_emu(emu, D.Batch([D.determined_gen(rng, 16, 100, 10, 3)[0], D.determined_gen(rng, 16, 100, 10, 2)[0]]), 2)
    assert [ref["status"] for ref in refs] == [P.EINVAL, P.ENOTREADY]


def test_wide_generations(emu):
    rng = np.random.default_rng(200)
    refs = run_emu(emu, D.Batch([D.determined_gen(rng, 200, 48, 60, 4, n_loose=2, n_dense=4)[0]]), 16)
    assert len(refs[0]["D"]) == 4 and refs[0]["rank"] == 70
    rng = np.random.default_rng(129)
    refs = run_emu(emu, D.Batch([P.Gen(rng, 200, 16, [rng.integers(1, 256, 200, dtype=np.uint8) for _ in range(n)])
                                 for n in (129, 128)]), 16)
    assert [ref["status"] for ref in refs] == [P.EINVAL, P.ENOTREADY]
    # k = 256 with the largest slot count: the largest LDS block
    rng = np.random.default_rng(256)
    run_emu(emu, D.Batch([D.determined_gen(rng, 256, 16, 200, 5, n_loose=3)[0]], mr=1024), 128)


def test_lengths_and_bad_rows(emu):
    rng = np.random.default_rng(112)
    gens = [D.determined_gen(rng, 16, 112, 10, 1 + j % 4, n_loose=1)[0] for j in range(8)]
    assert all(ref["min_len"] == 112 for ref in run_emu(emu, D.Batch(gens, full_len=True), 16))
    assert any(ref["min_len"] < 112 for ref in run_emu(emu, D.Batch(gens), 16))
    rng = np.random.default_rng(8)
    src = rng.integers(1, 256, (16, 100), dtype=np.uint8)
    src[2] = 0
    g = P.Gen(rng, 16, 100, D.sys_rows(16, list(range(10))) + [P.over(rng, 16, [1, 2, 12]), P.over(rng, 16, [2, 13])], src=src)
    refs = run_emu(emu, D.Batch([g]), 16)
    assert refs[0]["min_len"] == 0 and refs[0]["D"] == [12, 13]
    rng = np.random.default_rng(4)
    b = D.Batch([D.determined_gen(rng, 16, 100, 10, 2)[0] for _ in range(4)])
    b.off[0, 3] += 8
    b.len[1, 5] = 101
    b.off[2, 11], b.len[2, 11] = b.gs - 16, 17
    refs = run_emu(emu, b, 16)
    assert [ref["status"] for ref in refs] == [P.EINVAL] * 3 + [P.ENOTREADY]


def test_complete_and_random_generations(emu):
    for k in (1, 5, 16, 65, 130):
        rng = np.random.default_rng(1000 * k + 100)
        r = min(k, 20)
        e_top = r if r == k else r - 3
        refs = run_emu(emu, D.Batch([D.complete_gen(rng, k, 100, e_top), D.complete_gen(rng, k, 100, e_top // 2)]), r)
        assert all(ref["status"] == P.OK for ref in refs)
    rng = np.random.default_rng(300)
    refs = run_emu(emu, D.Batch([D.random_gen(rng, 12, 40) for _ in range(100)], mr=24), 12)
    assert {ref["status"] for ref in refs} == {P.OK, P.ENOTREADY}
    rng = np.random.default_rng(77)
    run_emu(emu, D.Batch([D.random_gen(rng, 33, 24) for _ in range(12)], mr=70), 0)      # r = 0: no pass, no capacity
    rng = np.random.default_rng(78)
    run_emu(emu, D.Batch([D.random_gen(rng, 40, 24) for _ in range(12)], mr=90), 9)
