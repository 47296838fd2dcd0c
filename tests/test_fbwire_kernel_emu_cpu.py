"""The six kernels of csrc/qf_fbwire.hip without a device: the kernels' own
source, unchanged, compiled for the host behind tests/kernel_emu (the lanes of
a block as host threads), as a stand-alone program under the host address and
undefined-behaviour sanitizers, with every buffer and every part of the
workspace at their exact sizes, over the case tables of the device test and
every feedback call of the loop.  Every output equals tests/fbwire_ref.py's
byte for byte: a read or write past a buffer there is a GPU fault, so it is
checked here first.  Of qf_report_closed_dev the program runs k_closed_mark and
compares the flags; the select and report kernels behind it are those of
qf_select.hip and qf_credit.hip, and the whole call is compared on the device.
Nothing is loaded into Python.  CPU only."""
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import fbwire_ref as F

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
    d = tmp_path_factory.mktemp("fbwire_emu")
    exe = d / "fbwire_emu"
    cmd = [_clangxx(), "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-DQF_KERNEL_EMU", f"-I{EMU}", f"-I{CSRC}", f"-I{REPO / 'include'}", "-pthread",
           str(EMU / "fbwire_main.cpp"), "-o", str(exe)]
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


def _n(v):
    return NULL if v is None else v


def run_pack(exe, c, before=None):
    before = before or c.blank()
    keys = [key for key in ("pkts", "pkt_len", "n_pkts", "n_left", "n_skipped") if key not in c.nulls]
    head = [0, c.k, c.max_len, c.F_max, c.stride, c.N_max, _n(c.n_reports), int("n_left" in keys), int("n_skipped" in keys)]
    assert len(c.reports) == c.N_max
    return _run(exe, head, [c.reports] + [before[key] for key in keys], c.model(before), keys)


def run_parse(exe, c, before=None):
    before = before or c.blank()
    keys = [key for key in ("reports", "n_reports", "n_left", "pkt_status", "pkt_first", "pkt_count") if key not in c.nulls]
    head = [1, c.k, c.max_len, c.F_max, c.stride, c.N_max, _n(c.n_pkts), int(c.append)] + \
           [int(key in keys) for key in ("n_left", "pkt_status", "pkt_first", "pkt_count")]
    return _run(exe, head, [c.pkts, c.pkt_len] + [before[key] for key in keys], c.model(before), keys)


def run_mark(exe, c):
    head = [2, c.G_src, c.F_max, _n(c.n_frames)]
    return _run(exe, head, [c.frame_id, c.frame_status, c.win], dict(flags=c.flags()), ["flags"])


@pytest.mark.parametrize("name", sorted(F.pack_cases()))
def test_pack_cases(emu, name):
    run_pack(emu, F.pack_cases()[name])


@pytest.mark.parametrize("name", sorted(F.parse_cases()))
def test_parse_cases(emu, name):
    c, before = F.parse_cases()[name]
    run_parse(emu, c, before)


@pytest.mark.parametrize("name", sorted(F.closed_cases()))
def test_closed_mark_cases(emu, name):
    run_mark(emu, F.closed_cases()[name][0])


def test_the_loops_feedback_calls(emu):
    _, polls, _ = F.loop_cached(F.NUM_LOOP, F.DEN_LOOP, F.DELAY_LOOP, F.MASK_LOOP, True)
    for p in polls:
        run_parse(emu, p["parse_call"])
        run_mark(emu, p["closed_call"])
        run_pack(emu, p["pack_call"])
