"""k_deliver_prepare and k_deliver_rows without a device: the kernels' own
source, compiled for the host behind tests/kernel_emu (the lanes of a block as
host threads that meet at the wave's collectives), as a stand-alone program
under the host address and undefined-behaviour sanitizers, with every buffer,
the workspace and the LDS block at their exact sizes, over the shapes of the
device test plus the inconsistent inputs.  Every output equals
tests/deliver_ref.py's: a read or write past a buffer there is a GPU fault, so
it is checked here first.  CPU only."""
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import deliver_ref as R

REPO = Path(__file__).resolve().parents[1]
CSRC = REPO / "quicfuscate_amd" / "csrc"
EMU = REPO / "tests" / "kernel_emu"
LDS_DECL = "    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];\n"
OK, EINVAL, ENOTREADY = R.OK, R.EINVAL, R.ENOTREADY


def _clangxx():
    for cand in ("/opt/rocm/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++")):
        if cand and Path(cand).exists():
            return cand
    raise RuntimeError("no host C++ compiler")


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    d = tmp_path_factory.mktemp("deliver_emu")
    text = (CSRC / "qf_deliver.hip").read_text()
    assert text.count(LDS_DECL) == 1, "the kernel's dynamic LDS declaration has changed"
    (d / "qf_deliver_emu.inc").write_text(text.replace(LDS_DECL, "    uint8_t* lds = emu_lds;\n"))
    exe = d / "deliver_prepare_emu"
    cmd = [_clangxx(), "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-DQF_KERNEL_EMU", f"-I{d}", f"-I{EMU}", f"-I{CSRC}", f"-I{REPO / 'include'}", "-pthread",
           str(EMU / "deliver_prepare_main.cpp"), "-o", str(exe)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    return exe


def _span(G, gs, rows, rs, L):
    return 0 if G == 0 or rows == 0 else (G - 1) * gs + (rows - 1) * rs + L


def run_emu(exe, c, n_known=True, grid_cap=2):
    """Both kernels over a Call -> the model's result; every output compared."""
    sh, Gn = c.sh, c.G
    k, em = sh.k, sh.e_max
    G_src = Gn if c.sel is None else c.G_src
    d = c.dec
    # exact sizes: the source generations, rec and out to the end of their last row's last 16-byte unit
    src = np.ascontiguousarray(c.src[: G_src * sh.src_gs])
    rec_bytes = _span(Gn, sh.rec_gs, em, sh.rec_rs, R.r16(sh.L)) if d["rec"] is not None else 0
    out_bytes = _span(Gn, sh.out_gs, k, sh.out_rs, R.r16(sh.L))
    fin, fout = exe.parent / "in.bin", exe.parent / "out.bin"
    n_sel = 0xFFFFFFFF if c.n_sel is None else c.n_sel
    with open(fin, "wb") as f:
        f.write(struct.pack("<12I8Q", k, em, sh.L, sh.max_rows, Gn, G_src, c.sel is not None, n_sel, c.ids is not None,
                            c.delivered is not None, n_known, grid_cap, sh.src_gs, sh.rec_rs, sh.rec_gs, sh.out_rs,
                            sh.out_gs, src.size, rec_bytes, out_bytes))
        parts = [src, np.asarray(c.row_off, np.uint32), np.asarray(c.row_len, np.uint32)]
        if rec_bytes:
            parts.append(np.asarray(d["rec"][:rec_bytes], np.uint8))
        if em:
            parts.append(np.asarray(d["rec_index"], np.uint16))
        parts += [np.asarray(d["n_rec"], np.uint32), np.asarray(d["dec_status"], np.int32), np.asarray(d["src_slot"], np.uint16)]
        if c.sel is not None:
            parts.append(np.asarray(c.sel, np.uint32))
        if c.ids is not None:
            parts.append(np.asarray(c.ids, np.uint64))
        if c.delivered is not None:
            parts.append(np.asarray(c.delivered, np.uint64))
        for a in parts:
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

    got = dict(out=take(out_bytes, np.uint8), out_len=take(Gn * k, np.uint32), out_state=take(Gn * k, np.uint8),
               n_out=take(Gn, np.uint32))
    if n_known:
        got["n_known"] = take(Gn, np.uint32)
    got["status"] = take(Gn, np.int32)
    if c.delivered is not None:
        got["delivered"] = take(G_src * R.WORDS, np.uint64).reshape(G_src, R.WORDS)
    cnt = take(Gn, np.uint32)
    assert pos == len(raw)
    want = c.model()
    for key, g in got.items():
        w = want[key].reshape(-1)[: g.size] if key == "out" else want[key]
        bad = np.argwhere(np.asarray(g).reshape(-1) != np.asarray(w).reshape(-1))
        assert bad.size == 0, f"{key} differs from the model at {bad[:6].reshape(-1).tolist()}"
    assert np.array_equal(cnt, want["n_out"]), "the counts the copy is given"
    return want


@pytest.mark.parametrize("name", sorted(R.shape_cases()))
def test_the_device_tests_shapes(emu, name):
    c = R.shape_cases()[name]
    want = run_emu(emu, c)
    assert (want["status"] == OK).all() and want["n_out"].sum() > 0
    if name.startswith("L"):
        assert {1, c.sh.L} <= set(want["out_len"].tolist())
    if name.startswith("k") and c.sh.k >= 64:
        st = set(want["out_state"].tolist())
        assert st == {R.UNKNOWN, R.STORED, R.RECOVERED, R.EARLIER}


@pytest.mark.parametrize("what", R.INCONSISTENT)
def test_inconsistent_inputs(emu, what):
    c = R.inconsistent_call(what)
    want = run_emu(emu, c)
    assert want["status"].tolist() == [OK, EINVAL, OK]
    # through a list, with an invalid entry, an unused one and an entry the decode refused
    d = c.dec
    order = [2, 1, 0, 1, 0]
    dec = dict(rec=np.concatenate([d["rec"].reshape(3, -1)[g] for g in order]),
               rec_index=d["rec_index"][order], n_rec=d["n_rec"][order],
               dec_status=np.array([OK, OK, EINVAL, OK, OK], np.int32), src_slot=d["src_slot"][order])
    listed = R.Call(c.sh, 5, c.src, c.row_off, c.row_len, dec, ids=np.array([7, 6, 5, 6, 5], np.uint64),
                    delivered=c.delivered, sel=[2, 1, 0, 7, 0], n_sel=4, G_src=3)
    want = run_emu(emu, listed)
    assert want["status"].tolist() == [OK, EINVAL, ENOTREADY, EINVAL, ENOTREADY]


def test_states_ids_and_the_strided_copy(emu):
    c = R.shape_cases()["k129"]
    run_emu(emu, c, n_known=False, grid_cap=1)          # one workgroup strides over every quad
    c.ids = None
    run_emu(emu, c)                                      # the tag is neither read nor written
    c.delivered = None
    run_emu(emu, c, grid_cap=1 << 20)                    # a grid as large as the work
    bad = R.inconsistent_call("none")
    bad.ids = np.array([(1 << 64) - 1, 1 << 62, (1 << 62) - 1], np.uint64)
    assert run_emu(emu, bad)["status"].tolist() == [EINVAL, EINVAL, OK]
    # duplicates without a state, n_sel NULL
    c = R.inconsistent_call("none")
    d = c.dec
    order = [1, 1, 0]
    dec = dict(rec=np.concatenate([d["rec"].reshape(3, -1)[g] for g in order]), rec_index=d["rec_index"][order],
               n_rec=d["n_rec"][order], dec_status=d["dec_status"][order], src_slot=d["src_slot"][order])
    want = run_emu(emu, R.Call(c.sh, 3, c.src, c.row_off, c.row_len, dec, sel=order, G_src=3))
    assert want["n_out"].tolist() == [4, 4, 4]
