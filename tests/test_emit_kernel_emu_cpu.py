"""k_emit_count, k_emit_place and k_emit_frames without a device: the kernels'
own source (csrc/qf_emit.hip, unchanged), compiled for the host behind
tests/kernel_emu (the lanes of a block as host threads that meet at the wave's
collectives), as a stand-alone program under the host address and
undefined-behaviour sanitizers, with every buffer and the workspace at their
exact sizes, over the shapes of the device test plus the inconsistent inputs.
Every output equals tests/emit_ref.py's: a read or write past a buffer there is
a GPU fault, so it is checked here first.  Nothing is loaded into Python.  CPU
only."""
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import emit_ref as R

REPO = Path(__file__).resolve().parents[1]
CSRC = REPO / "quicfuscate_amd" / "csrc"
EMU = REPO / "tests" / "kernel_emu"
OUT_KEYS = ("frames", "frame_len", "frame_off", "frame_id", "frame_pkt", "n_frames", "n_left", "entry_first",
            "entry_count", "entry_status")


def _clangxx():
    for cand in ("/opt/rocm/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++")):
        if cand and Path(cand).exists():
            return cand
    raise RuntimeError("no host C++ compiler")


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    d = tmp_path_factory.mktemp("emit_emu")
    exe = d / "emit_emu"
    cmd = [_clangxx(), "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-DQF_KERNEL_EMU", f"-I{EMU}", f"-I{CSRC}", f"-I{REPO / 'include'}", "-pthread",
           str(EMU / "emit_main.cpp"), "-o", str(exe)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    return exe


def run_emu(exe, c, before=None, n_left=True, grid_cap=2):
    """The three kernels over a Call -> the model's result; every output compared."""
    before = before or c.blank()
    fin, fout = exe.parent / "in.bin", exe.parent / "out.bin"
    opt = [c.row_index, c.n_rows, c.row_coeffs, c.row_len, c.in_status]
    with open(fin, "wb") as f:
        f.write(struct.pack("<16I4Q", c.k, c.L, c.max_rows, c.n_max, c.G_src, c.N_max, int(c.append),
                            0xFFFFFFFF if c.n_sel is None else c.n_sel, *[x is not None for x in opt],
                            c.rank is not None, n_left, grid_cap, c.row_stride, c.rows_gen_stride, c.frame_stride,
                            c.rows.size))
        parts = [c.rows, c.sel, c.ids] + [x for x in opt if x is not None]
        if c.rank is not None:
            parts += [c.rank, c.sent]
        parts += [before[key] for key in OUT_KEYS if key != "n_left" or n_left]
        for a in parts:
            f.write(np.ascontiguousarray(a).tobytes())
    res = subprocess.run([str(exe), str(fin), str(fout)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    raw = fout.read_bytes()
    want = c.model(before)
    pos = 0
    for key in OUT_KEYS + ("sent",):
        if (key == "n_left" and not n_left) or (key == "sent" and c.sent is None):
            continue
        w = want[key]
        g = np.frombuffer(raw, w.dtype, w.size, pos)
        pos += w.nbytes
        bad = np.argwhere(g != w.reshape(-1))
        assert bad.size == 0, f"{key} differs from the model at {bad[:6].reshape(-1).tolist()}"
    assert pos == len(raw)
    return want


@pytest.mark.parametrize("name", sorted(R.cases()))
def test_the_device_tests_cases(emu, name):
    c = R.cases()[name]
    want = run_emu(emu, c)
    if name.startswith(("k", "L")):
        assert (want["entry_status"] == R.OK).all() and want["n_frames"][0] > 0 and want["n_left"][0] == 0


def test_statuses_of_the_list_cases(emu):
    OK, EINVAL, ENOTREADY = R.OK, R.EINVAL, R.ENOTREADY
    cs = R.cases()
    assert run_emu(emu, cs["list"])["entry_status"].tolist() == [OK, EINVAL, EINVAL, EINVAL, R.ERANK, EINVAL, OK,
                                                                 ENOTREADY, ENOTREADY]
    assert run_emu(emu, cs["list_coded_without_vectors"])["entry_status"].tolist() == [OK, EINVAL, OK]
    assert run_emu(emu, cs["list_coded_row_unused"])["entry_status"].tolist() == [OK, OK, OK]
    want = run_emu(emu, cs["cutoff"])
    assert want["entry_status"].tolist() == [OK, OK, ENOTREADY, ENOTREADY, ENOTREADY, ENOTREADY]
    assert (want["n_frames"][0], want["n_left"][0]) == (7, 10)
    want = run_emu(emu, cs["exact_fit"])
    assert (want["n_frames"][0], want["n_left"][0]) == (10, 0)
    want = run_emu(emu, cs["cutoff_first"])
    assert (want["n_frames"][0], want["n_left"][0]) == (0, 10)
    assert run_emu(emu, cs["budget"])["entry_count"].tolist() == [0, 3, 2, 0, 0]
    want = run_emu(emu, cs["budget_above_rows"])   # the count is n_j, not rank - sent; sent advances by n_j only
    assert want["entry_count"].tolist() == [2, 2, 1, 0] and want["sent"].tolist() == [7, 2, 1, 0]


@pytest.mark.parametrize("name", sorted(R.APPEND_BASES))
def test_append(emu, name):
    c, before = R.append_case(name)
    want = run_emu(emu, c, before)
    base = min(R.APPEND_BASES[name], c.N_max)
    assert want["n_frames"][0] >= base
    assert (want["frames"].reshape(c.N_max, -1)[:base] == R.FILL).all()


def test_a_second_call_and_the_overflowed_entry(emu):
    c = R.cases()["budget_overflow"]
    first = run_emu(emu, c)
    assert first["entry_count"].tolist() == [1, 2, 3, 0] and first["n_left"][0] == 4
    c.sent = first["sent"]
    second = run_emu(emu, c, n_left=False)
    assert second["entry_count"].tolist() == [0, 0, 0, 4] and second["sent"].tolist() == c.rank.tolist()
    c.sent = second["sent"]
    third = run_emu(emu, c)                   # unchanged ranks: nothing is emitted, no frame byte written
    assert third["n_frames"][0] == 0 and (third["frames"] == R.FILL).all()


def test_scan_blocks_and_the_strided_copy(emu):
    c = R.scale_cases()["scan_blocks"]
    want = run_emu(emu, c, grid_cap=1)       # one workgroup strides over every quad
    assert want["n_left"][0] > 0 and (want["entry_status"] == R.OK).sum() > 2 * 64
    c.N_max = 2000
    run_emu(emu, c, grid_cap=1 << 20)        # everything fits; a grid as large as the work
