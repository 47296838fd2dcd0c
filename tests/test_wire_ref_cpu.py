"""tests/wire_ref.py, the model tests/test_gpu_wire.py compares the Cauchy wire
framing kernels with, held against itself without a device: the array frame
builder equals the per-frame oracle path, the planted header cases carry the
statuses the model gives them, reach all four statuses and leave a third of
the frames accepted at every shape the GPU tests use, and hand-written frames
with hand-written outputs pin the model.  CPU only."""
import numpy as np
import pytest

from tests import wire_ref as WR

# the shapes of test_parse_header_cases in tests/test_gpu_wire.py
HEADER_SHAPES = [(7, 5, 33), (64, 16, 1200), (200, 56, 48)]


@pytest.mark.parametrize("k,r,Lb", [(7, 5, 33), (13, 3, 16), (1, 3, 16), (255, 1, 20), (256, 0, 20), (64, 16, 1200)])
def test_array_frame_builder_equals_the_per_frame_oracle_path(oracle, k, r, Lb):
    rng = np.random.default_rng(k + Lb)
    G = 2
    fs = WR.r16(3 + k + Lb) + 16
    src = rng.integers(0, 256, (G, k, Lb), dtype=np.uint8)
    rep = rng.integers(0, 256, (G, r, Lb), dtype=np.uint8)
    raws = WR.frame_batch(oracle, k, r, Lb, src, rep if r else None)
    buf, lens = WR.frame_batch_np(oracle, k, r, Lb, src, rep if r else None, fs)
    assert len(raws) == G * (k + r)
    buf, lens = buf.reshape(-1, fs), lens.reshape(-1)
    for f, raw in enumerate(raws):
        assert lens[f] == len(raw) == (1 + Lb if f % (k + r) < k else 3 + k + Lb)
        assert buf[f, : len(raw)].tobytes() == raw, f
        assert (buf[f, len(raw):] == WR.FILL_FRAME).all()


def test_strided_rows_and_gaps():
    a = np.arange(2 * 3 * 5, dtype=np.uint8).reshape(2, 3, 5)
    buf = WR.strided(a, 16, 64).reshape(2, 64)
    for g in range(2):
        for i in range(3):
            assert (buf[g, 16 * i: 16 * i + 5] == a[g, i]).all()
            assert (buf[g, 16 * i + 5: 16 * i + 16] == WR.FILL_GAP).all()
        assert (buf[g, 48:] == WR.FILL_GAP).all()


@pytest.mark.parametrize("k,r,Lb", HEADER_SHAPES + [(4, 2, 8), (1, 3, 16), (13, 3, 32)])
def test_header_cases_statuses_and_accepted_share(oracle, k, r, Lb):
    fs = WR.r16(3 + k + Lb)
    cases = WR.header_cases(oracle, k, r, Lb, fs)
    frames, lens, ids, n = WR.place([cases], len(cases) + 2, fs)
    model = WR.parse_frames(oracle, k, r, Lb, len(cases) + 2, frames, lens, ids, n)[0]
    assert len(model["status"]) == len(cases)
    for s, (raw, ln, pid, st, what) in enumerate(cases):
        assert model["status"][s] == st, what
    statuses = {e[3] for e in cases}
    assert statuses == {WR.OK, WR.EINVAL, WR.ERANGE, WR.ETOOSMALL}
    n_ok = sum(1 for e in cases if e[3] == WR.OK)
    assert 3 * n_ok >= len(cases)
    assert model["n_rows"] == n_ok
    # the probes the list is there for
    what = " | ".join(e[4] for e in cases)
    for probe in ("first byte 0x2", "first byte 0xff", "length 0", "length 1:", "length 2", "length 3 + k - 1",
                  "length 3 + k:", "length == frame_stride,", "frame_stride + 1", "256 + k, frame shorter",
                  "coefficient length k - 1", "coefficient length k + 1", "j = r - 1", "c0 == 0",
                  "coefficient 0 flipped", "payload L + 1"):
        assert probe in what, probe
    if k > 1:
        assert "coefficient 1 flipped" in what or k == 2
        assert f"coefficient {k - 1} flipped" in what
    if k + r < 256:
        assert "j = r," in what
    if Lb >= 256:
        assert "256 + k, frame long enough" in what


def _gf_mul(a, b):
    """GF(2^8) product, polynomial 0x11D, bit by bit."""
    p = 0
    while b:
        if b & 1:
            p ^= a
        a <<= 1
        if a & 0x100:
            a ^= 0x11D
        b >>= 1
    return p


def test_hand_written_frames(oracle):
    """k = 4, r = 2, L = 8, frame_stride = 16.  Cauchy row j, column i is the
    inverse of i ^ (k + j): row 1 = 1/5, 1/4, 1/7, 1/6."""
    k, r, Lb, fs, mr = 4, 2, 8, 16, 6
    row1 = [167, 71, 186, 122]
    for i, c in enumerate(row1):
        assert _gf_mul(c, i ^ 5) == 1
    frames = np.full((1, mr, fs), 0xCC, np.uint8)
    lens = np.zeros((1, mr), np.uint32)
    ids = np.zeros((1, mr), np.uint64)

    def put(s, raw, ln, pid):
        frames[0, s, : len(raw)] = raw
        lens[0, s] = ln
        ids[0, s] = pid

    put(0, [1, 0xAA, 0xBB], 3, 2 ** 32 + 3)                          # source, column (2^32 + 3) % 4 = 3
    put(1, [0, 0, 4] + row1 + [0x11, 0x22, 0x33, 0x44], 10, 9)       # repair 1, the last payload byte not sent
    put(2, [0, 0, 4, 167, 71, 186, 123, 0x11], 8, 9)                 # the last coefficient off by one bit
    put(3, [0, 0], 2, 9)                                             # no coefficient length
    put(4, [1], 0, 9)                                                # empty
    put(5, [1] + [7] * 9, 10, 2 ** 64 - 1)                           # payload of 9 > L
    got = WR.parse_frames(oracle, k, r, Lb, mr, frames, lens, ids, None)[0]
    assert got["status"].tolist() == [0, 0, WR.ERANGE, WR.ETOOSMALL, WR.EINVAL, WR.EINVAL]
    assert got["n_rows"] == 2
    assert got["row_index"].tolist() == [3, 5]
    assert got["rows"].tolist() == [[0xAA, 0xBB, 0, 0, 0, 0, 0, 0], [0x11, 0x22, 0x33, 0, 0, 0, 0, 0]]
    # the frame count: clamped to max_rows, and frames behind it not looked at
    assert WR.parse_frames(oracle, k, r, Lb, mr, frames, lens, ids, [mr + 5])[0]["status"].tolist() == \
        got["status"].tolist()
    one = WR.parse_frames(oracle, k, r, Lb, mr, frames, lens, ids, [1])[0]
    assert one["status"].tolist() == [0] and one["n_rows"] == 1 and one["row_index"].tolist() == [3]
    none = WR.parse_frames(oracle, k, r, Lb, mr, frames, lens, ids, [0])[0]
    assert none["status"].tolist() == [] and none["n_rows"] == 0 and none["rows"].shape == (0, Lb)
    # a length above the stride is refused before the frame is looked at
    lens[0, 0] = fs + 1
    assert WR.parse_frames(oracle, k, r, Lb, mr, frames, lens, ids, [1])[0]["status"].tolist() == [WR.EINVAL]
    # the same frames through frame_batch: what the framer must write for them
    src = np.zeros((1, k, Lb), np.uint8)
    src[0, 3, :2] = [0xAA, 0xBB]
    rep = np.zeros((1, r, Lb), np.uint8)
    rep[0, 1, :3] = [0x11, 0x22, 0x33]
    raws = WR.frame_batch(oracle, k, r, Lb, src, rep)
    assert raws[3] == bytes([1, 0xAA, 0xBB, 0, 0, 0, 0, 0, 0])
    assert raws[5] == bytes([0, 0, 4] + row1 + [0x11, 0x22, 0x33, 0, 0, 0, 0, 0])
