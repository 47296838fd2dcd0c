"""The read bounds of csrc/qf_wire_dev.h without a device: frame_head and
vector_block, the header's own source compiled for the host behind
tests/kernel_emu, as a stand-alone program under the host address and
undefined-behaviour sanitizers.  The frame slots are one heap block of exactly
N * frame_stride bytes and row_coeffs one of exactly n * k, so a read a few
bytes past the last slot, which no device test sees because its buffers are
larger and which is a GPU fault in production, ends the program here.  Both
callers' rules run: the header parsers' (the payload at a multiple of 16, the
readable bytes end with the vector) and the coded parser's (any payload start,
they end with the payload).  Statuses, indices, payload bounds and vectors
equal tests/poll_ref.py's frame rule and test_gpu_wire_coded's _expected_parse
over the oracle.  CPU only."""
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import poll_ref as R
from tests import test_gpu_wire_coded as W

REPO = Path(__file__).resolve().parents[1]
CSRC = REPO / "quicfuscate_amd" / "csrc"
EMU = REPO / "tests" / "kernel_emu"
L_EMU = 32          # a multiple of 16: a full systematic frame ends on its slot's last byte
KS = (1, 15, 16, 17, 20, 33, 36)


def _clangxx():
    for cand in ("/opt/rocm/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++")):
        if cand and Path(cand).exists():
            return cand
    raise RuntimeError("no host C++ compiler")


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    d = tmp_path_factory.mktemp("wire_dev_emu")
    exe = d / "wire_dev_emu"
    cmd = [_clangxx(), "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           f"-I{EMU}", f"-I{CSRC}", f"-I{REPO / 'include'}", "-pthread", str(EMU / "wire_dev_main.cpp"), "-o", str(exe)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    return exe


def make_slots(k, last):
    """Frame slots of P + L_EMU bytes, the smallest that reach each branch; the last slot holds a coded
    frame with an empty payload whose vector ends on the buffer's last byte, a full systematic frame, or
    the first two bytes of a coded frame."""
    rng = np.random.default_rng(100 * k + (last == "sys"))
    L = L_EMU
    P = R.payload_offset(k)
    vec = lambda: rng.integers(1, 256, k).astype(np.uint8)
    pay = lambda n: rng.integers(0, 256, n, dtype=np.uint8)
    puts = []
    puts.append(lambda p, f: p.put_coded(f, 0, 7, vec(), pay(L)))                      # the sender's layout
    puts.append(lambda p, f: p.put_sys(f, 0, 3 * k + k // 2, pay(L)))                  # row 1: unaligned for odd k
    puts.append(lambda p, f: p.put_coded(f, 0, 8, vec(), pay(0), off=p.fs - 3 - k))    # vector ends with the slot
    for n in (0, 1, 2, 3, 4, 16, 17):    # around the 20-byte rule: `end` 0 .. 4 bytes behind the vector
        puts.append(lambda p, f, n=n: p.put_coded(f, 0, 9, vec(), pay(n)))
    puts.append(lambda p, f: p.put_sys(f, 0, k - 1, pay(0)))
    puts.append(lambda p, f: p.put_sys(f, 0, 5, pay(9), off=P - 2))                    # payload not at a multiple of 16
    puts.append(lambda p, f: p.put_coded(f, 0, 5, vec(), pay(5), off=P - 3 - k + 1))   # ... a coded one, one byte on
    puts.append(lambda p, f: p.put_sys(f, 0, 5, pay(L + 1), off=max(P - 17, 0)))       # longer than a row
    puts.append(lambda p, f: p.put_coded(f, 0, 5, vec(), pay(9), cl=k + 1))            # another k
    puts.append(lambda p, f: p.put_coded(f, 0, 10, np.zeros(k, np.uint8), pay(L)))
    bad = ("empty", "past_slot", "short", "truncated")
    N = len(puts) + len(bad) + 1
    p = R.Poll(k, L, N)
    assert p.fs == P + L
    for f, put in enumerate(puts):
        put(p, f)
    for j, kind in enumerate(bad):
        R._bad_frame(p, rng, len(puts) + j, 0, kind)
    if last == "coded":
        p.put_coded(N - 1, 0, 11, vec(), pay(0), off=p.fs - 3 - k)
    elif last == "sys":
        p.put_sys(N - 1, 0, 2 * k + k - 1, pay(L))
    else:
        # two bytes of a coded frame's header on the slot's last two: the length is not there to read
        p.frames[N - 1, p.fs - 2:] = 0
        p.flen[N - 1], p.foff[N - 1], p.gen[N - 1], p.kind[N - 1] = 2, p.fs - 2, 0, "short"
    assert p.foff[N - 1] + p.flen[N - 1] == p.fs
    return p


def expected(oracle, p, f, header_rule):
    """-> status, index, payload start, payload length, vector (the last four for QF_OK)."""
    k = p.k
    if header_rule:
        st, idx, pay, plen = R.frame_rule(p, f)
    else:
        foff = int(p.foff[f])
        st, is_sys, _, body = W._expected_parse(oracle, p.frames[f, foff:].tobytes(), int(p.flen[f]), foff, p.fs, k, p.L)
        if st == R.OK:
            idx = int(p.ids[f] % np.uint64(k)) if is_sys else k
            pay, plen = foff + (1 if is_sys else 3 + k), len(body)
    if st != R.OK:
        return st, None, None, None, None
    v = np.zeros(k, np.uint8)
    if idx < k:
        v[idx] = 1
    else:
        v[:] = p.frames[f, pay - k: pay]
    return st, idx, pay, plen, v


def run_emu(exe, oracle, p, header_rule):
    k, N = p.k, p.N_max
    fin, fout = exe.parent / "in.bin", exe.parent / "out.bin"
    with open(fin, "wb") as f:
        f.write(struct.pack("<6IQ", k, p.L, N, int(header_rule), int(not header_rule), 0, p.fs))
        for a in (p.flen, p.foff, p.ids, p.frames):
            f.write(np.ascontiguousarray(a).tobytes())
    res = subprocess.run([str(exe), str(fin), str(fout)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    raw = fout.read_bytes()
    st = np.frombuffer(raw, np.int32, N, 0)
    idx, pay, plen = (np.frombuffer(raw, np.uint32, N, 4 * N * j) for j in (1, 2, 3))
    n = int(np.frombuffer(raw, np.uint32, 1, 16 * N)[0])
    co = np.frombuffer(raw, np.uint8, n * k, 16 * N + 4).reshape(n, k)
    assert len(raw) == 16 * N + 4 + n * k
    slot, seen = 0, []
    for f in range(N):
        e_st, e_idx, e_pay, e_plen, e_v = expected(oracle, p, f, header_rule)
        assert st[f] == e_st, (k, f, p.kind[f], st[f], e_st)
        seen.append(e_st)
        if e_st != R.OK:
            continue
        assert (idx[f], pay[f], plen[f]) == (e_idx, e_pay, e_plen), (k, f)
        assert np.array_equal(co[slot], e_v), (k, f, slot)
        slot += 1
    assert slot == n
    return seen


@pytest.mark.parametrize("last", ["coded", "sys", "short"])
@pytest.mark.parametrize("k", KS)
def test_wire_dev_read_bounds(emu, oracle, k, last):
    p = make_slots(k, last)
    for header_rule in (True, False):
        seen = run_emu(emu, oracle, p, header_rule)
        # every status of the rule occurs, and the last slot's frame is read to the buffer's last byte
        assert {R.OK, R.EINVAL, R.ETOOSMALL, R.ERANGE} <= set(seen)
        assert seen[-1] == (R.ETOOSMALL if last == "short" else R.OK)
    # the two rules differ where they should: the systematic frame whose payload is not at a multiple of 16
    f = [i for i in range(p.N_max) if p.kind[i] == "sys" and (int(p.foff[i]) + 1) % 16][0]
    assert expected(oracle, p, f, True)[0] == R.EINVAL and expected(oracle, p, f, False)[0] == R.OK
