"""The send step without a device: qf_emit_frames_sel_dev is exported, declared
and bound with the header's argument count, a NULL context and every bad field
fail before any device work, the Python mirror checks every buffer,
tests/emit_ref.py's frame bytes are fec.Packet.to_raw's for every row kind, the
model gives what the header states on hand-written lists, and the loop source ->
relay -> receiver under the models alone stays within the conditions the device
test relies on.  CPU only."""
import ctypes
import re

import numpy as np
import pytest

from quicfuscate_amd import _lib as L
from tests import emit_ref as R

E = L.QF_EINVAL
OK, EINVAL, ENOTREADY = R.OK, R.EINVAL, R.ENOTREADY


def test_symbol_is_exported_with_the_header_argument_count():
    lib = L._lib()
    name = "qf_emit_frames_sel_dev"
    assert name in L.header_symbols() and hasattr(lib, name) and name in L._SIGS
    txt = re.sub(r"/\*.*?\*/", " ", L.HEADER.read_text(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", txt, flags=re.S)
    assert m and len(L._SIGS[name][1]) == len(m.group(1).split(",")) == 22
    assert re.search(r"#define\s+QF_EMIT_APPEND\s+1u", L.HEADER.read_text()) and L.QF_EMIT_APPEND == 1
    assert ctypes.sizeof(L.EmitShape) == 6 * 4 + 3 * 8
    assert (R.OK, R.EINVAL, R.ENOTREADY, R.ERANK) == (L.QF_OK, L.QF_EINVAL, L.QF_ENOTREADY, L.QF_ERANK)


def test_null_context_and_bad_fields():
    lib = L._lib()
    keep = ctypes.create_string_buffer(64)
    ctx = ctypes.cast(keep, ctypes.c_void_p)
    mem = ctypes.create_string_buffer(1 << 16)
    p = (ctypes.addressof(mem) + 15) // 16 * 16
    names = ("rows", "row_index", "n_rows", "row_coeffs", "row_len", "in_status", "ids", "rank", "sent", "frames",
             "frame_len", "frame_off", "frame_id", "frame_pkt", "n_frames", "n_left", "entry_first", "entry_count",
             "entry_status")
    good_sel = L.GenSel(p, None, 4, 9)

    def status(handle=ctx, sel=good_sel, k=13, Lb=20, mr=5, N=10, flags=0, reserved=0, rs=32, gs=160, fs=48, **ptrs):
        a = {n: p + 2048 * (i + 1) for i, n in enumerate(names)}
        a.update(ptrs)
        sh = L.EmitShape(k, Lb, mr, N, flags, reserved, rs, gs, fs)
        return lib.qf_emit_frames_sel_dev(handle, ctypes.byref(sh), ctypes.byref(sel) if sel else None,
                                          *[a[n] for n in names])

    # every check comes before the context is touched (a fake context would crash otherwise)
    assert status(handle=None) == E and status(sel=None) == E
    assert lib.qf_emit_frames_sel_dev(ctx, None, ctypes.byref(good_sel), *[p] * 19) == E
    assert status(sel=L.GenSel(None, None, 4, 9)) == E and status(sel=L.GenSel(p, None, 0, 9)) == E
    assert status(sel=L.GenSel(p, None, 4, 0)) == E and status(sel=L.GenSel(p, None, (1 << 24) + 1, 9)) == E
    assert status(k=0) == E and status(k=257, fs=512) == E and status(Lb=0) == E
    assert status(mr=0) == E and status(mr=1025) == E and status(N=0) == E
    assert status(flags=2) == E and status(flags=3) == E and status(reserved=1) == E
    assert status(rs=40) == E and status(gs=168) == E and status(fs=56) == E      # strides % 16
    assert status(rs=16) == E                                                      # row_stride < L
    assert status(fs=32) == E                                                      # frame_stride < P + L = 36
    assert status(N=(1 << 32) // 48 + 1) == E                                      # N_max * frame_stride > 2^32
    assert status(rows=p + 8) == E and status(frames=p + 2048 * 10 + 8) == E       # not 16-byte aligned
    assert status(rank=None) == E and status(sent=None) == E                       # one budget array without the other
    assert status(row_index=None, row_coeffs=None) == E
    for nm in names:
        if nm not in ("row_index", "n_rows", "row_coeffs", "row_len", "in_status", "rank", "sent", "n_left"):
            assert status(**{nm: None}) == E, nm
    del keep, mem


def test_mirror_rejects_undersized_buffers():
    import torch

    from quicfuscate_amd import fec

    k, Lb, mr, n_max, G_src, N = 13, 20, 5, 3, 4, 10
    rs, gs, fs = 32, 160, 48
    u8 = lambda n: torch.zeros(n, dtype=torch.uint8)            # noqa: E731
    i32 = lambda n: torch.zeros(n, dtype=torch.int32)           # noqa: E731
    i64 = lambda n: torch.zeros(n, dtype=torch.int64)           # noqa: E731
    pos = dict(sel=i32(n_max), n_sel=i32(1), rows=u8(2 * gs + 4 * rs + 32), ids=i64(n_max),
               frames=u8((N - 1) * fs + 16 + Lb), frame_len=i32(N), frame_off=i32(N), frame_id=i64(N), frame_pkt=i64(N),
               n_frames=i32(1), entry_first=i32(n_max), entry_count=i32(n_max), entry_status=i32(n_max))
    opt = dict(row_index=torch.zeros(n_max * mr, dtype=torch.int16), n_rows=i32(n_max), row_coeffs=u8(n_max * mr * k),
               row_len=i32(n_max * mr), in_status=i32(n_max), rank=i32(G_src), sent=i32(G_src), n_left=i32(1))
    for key in list(pos) + list(opt):
        a, o = dict(pos), dict(opt)
        (a if key in a else o)[key] = (a if key in a else o)[key][:-1]
        with pytest.raises(ValueError, match=key):
            fec.emit_frames_sel(*a.values(), k, Lb, n_max=n_max, G_src=G_src, max_rows=mr, N_max=N, row_stride=rs,
                                rows_gen_stride=gs, frame_stride=fs, **o)


@pytest.mark.parametrize("k", R.SHAPE_K)
def test_frame_bytes_are_packet_to_raw(k):
    from quicfuscate_amd import fec

    rng = np.random.default_rng(k)
    c = R.make_call(k, 17, 5, 2, seed=k, lens="ragged")
    o = c.model()
    P, fs = c.P, c.frame_stride
    frames = o["frames"].reshape(c.N_max, fs)
    kinds = set()
    for j in range(c.n_max):
        for s in range(c.max_rows):
            q = int(o["entry_first"][j]) + s
            idx, rlen = int(c.row_index[j, s]), int(c.row_len[j, s])
            r0 = j * c.rows_gen_stride + s * c.row_stride
            pay = bytearray(c.rows[r0: r0 + rlen].tobytes())
            pkt = fec.Packet(int(rng.integers(0, 1 << 30)) * k + idx % k, pay, rlen, idx < k,
                             None if idx < k else bytes(c.row_coeffs[j, s]), 0 if idx < k else k)
            raw = pkt.to_raw()
            off, ln = int(o["frame_off"][q]), int(o["frame_len"][q])
            assert ln == len(raw) and off + ln == P + rlen and bytes(frames[q, off: off + ln]) == raw
            # nothing of the slot outside the frame is written
            assert (frames[q, :off] == R.FILL).all() and (frames[q, off + ln:] == R.FILL).all()
            assert int(o["frame_pkt"][q]) == (idx if idx < k else 0) and int(o["frame_id"][q]) == int(c.ids[j])
            back = fec.Packet.from_raw(int(o["frame_pkt"][q]), raw)
            assert back.is_systematic == (idx < k) and bytes(back.payload()) == bytes(pay)
            kinds.add((idx < k, rlen == 0, rlen == c.L))
    assert {(True, False, False), (False, False, False)} <= kinds


def test_the_model_on_the_hand_written_lists():
    cs = R.cases()
    o = cs["list"].model()
    assert o["entry_status"].tolist() == [OK, EINVAL, EINVAL, EINVAL, R.ERANK, EINVAL, OK, ENOTREADY, ENOTREADY]
    assert o["entry_count"].tolist() == [5, 0, 0, 0, 0, 0, 5, 0, 0]
    assert o["entry_first"].tolist() == [0] + [R.NONE32] * 5 + [5] + [R.NONE32] * 2
    assert (o["n_frames"][0], o["n_left"][0]) == (10, 0) and (o["frame_len"][10:] == 0xCCCCCCCC).all()
    o = cs["cutoff"].model()
    assert o["entry_status"].tolist() == [OK, OK] + [ENOTREADY] * 4 and o["entry_count"].tolist() == [5, 2, 0, 0, 0, 0]
    assert (o["n_frames"][0], o["n_left"][0]) == (7, 10)
    assert (o["frames"].reshape(8, -1)[7] == R.FILL).all()
    o = cs["budget"].model()
    assert o["entry_count"].tolist() == [0, 3, 2, 0, 0] and o["sent"].tolist() == [3, 4, 2, 0, 5]
    assert o["entry_status"].tolist() == [OK] * 5 and o["entry_first"].tolist() == [R.NONE32, 0, 3, R.NONE32, R.NONE32]
    c = cs["budget_above_rows"]                 # rank - sent = 4, 2, 3, 1 against n_j = 2, 5, 1, 0
    o = c.model()
    assert o["entry_count"].tolist() == [2, 2, 1, 0] and o["sent"].tolist() == [7, 2, 1, 0]
    assert o["entry_status"].tolist() == [OK] * 4 and o["n_frames"][0] == 5 and o["n_left"][0] == 0
    for name, (n_frames, first) in dict(base0=(10, [0, 4, 5]), base_mid=(8, [3, 7, R.NONE32]),
                                        base_full=(12, [R.NONE32] * 3), base_above=(12, [R.NONE32] * 3)).items():
        c, before = R.append_case(name)
        o = c.model(before)
        assert o["n_frames"][0] == n_frames and o["entry_first"].tolist() == first, name
    c, before = R.append_case("base_mid")
    assert c.model(before)["n_left"][0] == 5 and c.model(before)["entry_status"].tolist() == [OK, OK, ENOTREADY]


def test_the_loop_under_the_models(oracle):
    """Source -> relay -> receiver with every step a model: the conditions the device loop relies on."""
    spec, polls, stats = R.loop_model(oracle)
    # with the committed seeds and drop mask every generation reaches rank k at the receiver
    assert sorted(stats["delivered"]) == list(range(R.GENS_LOOP))
    n_dropped = sum(len(spec.drop_list(p["gens"])) for p in polls)
    assert n_dropped >= R.GENS_LOOP // 2
    # the relay never emits more than rank frames per generation, and in the end exactly rank = k
    for g in range(R.GENS_LOOP):
        assert stats["emitted"][g] <= stats["final_rank"][g] <= R.K_LOOP
        assert stats["emitted"][g] == R.K_LOOP
    # at least one poll overflows the relay's queue, and the next call emits what it left over
    over = [i for i, p in enumerate(polls) if p["q2"]["n_left"][0] > 0]
    assert over
    for i in over:
        q2, nxt = polls[i]["q2"], polls[i + 1]
        late = [(s, g) for j, (s, g) in enumerate(polls[i]["listed"]) if q2["entry_status"][j] == ENOTREADY]
        assert late and int(q2["n_left"][0]) == sum(
            int(polls[i]["call"].entries()[1][j]) for j, _ in enumerate(polls[i]["listed"]) if q2["entry_status"][j] == ENOTREADY)
        for s, g in late:
            j = [x for x, _ in nxt["listed"]].index(s)
            assert nxt["listed"][j] == (s, g) and nxt["q2"]["entry_status"][j] == OK and nxt["q2"]["entry_count"][j] > 0
    # the source's second call appends behind the first, and the queue is what the next hop's models read
    two = next(p for p in polls if len(p["gens"]) == 2)
    assert two["q1"]["n_frames"][0] == 2 * (R.K_LOOP + R.R_SRC)
    assert (two["q1"]["frame_pkt"][: 2 * R.K_LOOP] == np.tile(np.arange(R.K_LOOP), 2)).all()
    assert (two["q1"]["frame_pkt"][2 * R.K_LOOP: 12] == 0).all()
