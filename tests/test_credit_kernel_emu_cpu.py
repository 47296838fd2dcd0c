"""k_report_sel, k_credit_reports and k_credit_apply without a device: the
kernels' own source (csrc/qf_credit.hip, unchanged), compiled for the host
behind tests/kernel_emu (the lanes of a block as host threads), as a
stand-alone program under the host address and undefined-behaviour sanitizers,
with every buffer and the workspace at their exact sizes, over the cases of the
device test.  Every output equals tests/credit_ref.py's: a read or write past a
buffer there is a GPU fault, so it is checked here first.  Nothing is loaded
into Python.  CPU only."""
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import credit_ref as C

REPO = Path(__file__).resolve().parents[1]
CSRC = REPO / "quicfuscate_amd" / "csrc"
EMU = REPO / "tests" / "kernel_emu"
NULL = 0xFFFFFFFF


def _clangxx():
    for cand in ("/opt/rocm/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++")):
        if cand and Path(cand).exists():
            return cand
    raise RuntimeError("no host C++ compiler")


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    d = tmp_path_factory.mktemp("credit_emu")
    exe = d / "credit_emu"
    cmd = [_clangxx(), "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-DQF_KERNEL_EMU", f"-I{EMU}", f"-I{CSRC}", f"-I{REPO / 'include'}", "-pthread",
           str(EMU / "credit_main.cpp"), "-o", str(exe)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    return exe


def _run(exe, head, parts, want, keys):
    fin, fout = exe.parent / "in.bin", exe.parent / "out.bin"
    with open(fin, "wb") as f:
        f.write(struct.pack("<12I", *(list(head) + [0] * (12 - len(head)))))
        for a in parts:
            f.write(np.ascontiguousarray(a).tobytes())
    res = subprocess.run([str(exe), str(fin), str(fout)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    raw = fout.read_bytes()
    pos = 0
    for key in keys:
        w = want[key]
        g = np.frombuffer(raw, np.uint8, w.nbytes, pos)
        pos += w.nbytes
        bad = np.flatnonzero(g != w.view(np.uint8).reshape(-1))
        assert bad.size == 0, f"{key} differs from the model at bytes {bad[:6].tolist()}"
    assert pos == len(raw)
    return want


def run_credit(exe, c, before):
    """The two kernels over a CreditCall from `before` -> the model's result; every output compared."""
    keys = ("state", "credit") + (("status",) if c.status and c.N_max else ())
    head = [0, c.G, c.N_max, c.k, c.num, c.den, c.cap, NULL if c.n_reports is None else c.n_reports,
            int("status" in keys)]
    parts = [c.win, c.rank, c.sent] + ([c.reports] if c.N_max else []) + [before[key] for key in keys]
    return _run(exe, head, parts, c.model(before), keys)


def run_report(exe, c, before, n_left=True):
    keys = ("reports", "n_reports") + (("n_left",) if n_left else ())
    head = [1, c.k, c.n_max, c.G_src, c.N_max, int(c.append), NULL if c.n_sel is None else c.n_sel, int(n_left)]
    return _run(exe, head, [c.sel, c.win, c.rank] + [before[key] for key in keys], c.model(before), keys)


@pytest.mark.parametrize("name", sorted(C.credit_cases()))
def test_credit_cases(emu, name):
    c, before = C.credit_cases()[name]
    run_credit(emu, c, before)


@pytest.mark.parametrize("name", sorted(C.credit_sequences()))
def test_credit_sequences(emu, name):
    state = credit = None
    for c in C.credit_sequences()[name]:
        o = run_credit(emu, c, c.blank(state, credit))
        state, credit = o["state"], o["credit"]


@pytest.mark.parametrize("name", sorted(C.report_cases()))
def test_report_cases(emu, name):
    c, before, n_left = C.report_cases()[name]
    run_report(emu, c, before, n_left)


def test_the_lossy_loops_calls(emu, oracle):
    spec, polls, stats = C.lossy_loop(oracle, 1, 1, True)
    state = credit = None
    for p in polls:
        c = p["credit_call"]
        o = run_credit(emu, c, c.blank(state, credit))
        state, credit = o["state"], o["credit"]
        assert np.array_equal(credit, p["credit_out"]["credit"])
        (ra, rb), (oa, ob) = p["report_calls"], p["report_out"]
        run_report(emu, ra, ra.blank())
        run_report(emu, rb, oa)
