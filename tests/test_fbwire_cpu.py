"""Properties of tests/fbwire_ref.py, the models of qf_frame_reports_dev,
qf_parse_report_frames_dev and qf_report_closed_dev, and of the loop with the
back channel as bytes under them: what the device test then holds the library
to.  CPU only; the one library symbol used is the host function
qf_report_frame_capacity."""
import numpy as np
import pytest

from tests import credit_ref as C
from tests import emit_ref as E
from tests import fbwire_ref as F

OK, EINVAL = F.OK, F.EINVAL
ALL = list(range(E.GENS_LOOP))
CHOSEN = (F.NUM_LOOP, F.DEN_LOOP, F.DELAY_LOOP, F.MASK_LOOP)


def test_the_known_answer():
    want = bytes.fromhex("020002" "0000000000000005" "0003" "3FFFFFFFFFFFFFFF" "0100")
    assert len(want) == 23
    assert F.packet([(5, 3), ((1 << 62) - 1, 256)]) == want
    c = F.PackCall(256, 23, 1, 32, F.records([(5, 3, 0), ((1 << 62) - 1, 256, 0)]))
    o = c.model()
    assert o["pkts"][:23].tobytes() == want and (o["pkts"][23:] == F.FILL).all()
    assert (o["pkt_len"][0], o["n_pkts"][0], o["n_left"][0], o["n_skipped"][0]) == (23, 1, 0, 0)
    back = F.ParseCall(256, 23, 1, 32, o["pkts"], o["pkt_len"], 2, n_pkts=1).model()
    assert back["reports"].tolist() == [(5, 3, 0), ((1 << 62) - 1, 256, 0)] and back["pkt_status"][0] == OK


def test_the_capacity_through_the_library(qf):
    want = {0: 0, 12: 0, 13: 1, 22: 1, 23: 2, 1200: 119, 65535: 6553, 65536: 0}
    for max_len, per in want.items():
        assert qf.report_frame_capacity(max_len) == per == F.capacity(max_len), max_len


@pytest.mark.parametrize("name", sorted(F.pack_cases()))
def test_pack_then_parse_returns_the_sendable_records_in_order(name):
    c = F.pack_cases()[name]
    o = c.model()
    N, ent = c.sent()
    P = int(o["n_pkts"][0])
    kept = ent[: c.F_max * c.per]
    assert P == min(-(-len(ent) // c.per), c.F_max)
    if "n_left" not in c.nulls:
        assert o["n_left"][0] == len(ent) - len(kept)
    if "n_skipped" not in c.nulls:
        assert o["n_skipped"][0] == N - len(ent)
    # no byte of a slot outside [0, pkt_len), no slot and no length at or beyond P
    sl = o["pkts"].reshape(c.F_max, c.stride)
    for p in range(c.F_max):
        ln = int(o["pkt_len"][p]) if p < P else 0
        assert (sl[p, ln:] == F.FILL).all()
    assert (o["pkt_len"][P:] == F.FILL32).all() and (o["pkt_len"][:P] <= c.max_len).all()
    back = F.ParseCall(c.k, c.max_len, c.F_max, c.stride, o["pkts"], o["pkt_len"], max(len(kept), 1), n_pkts=P).model()
    assert int(back["n_reports"][0]) == len(kept) and back["n_left"][0] == 0
    assert back["reports"][: len(kept)].tolist() == [(x, r, 0) for x, r in kept]
    assert (back["pkt_status"][:P] == OK).all()
    assert back["pkt_first"][:P].tolist() == [p * c.per for p in range(P)]


def test_the_parse_model():
    cs = F.parse_cases()
    c, before = cs["lengths"]
    o = c.model(before)
    assert o["pkt_status"].tolist() == [EINVAL] * 9 + [OK] and o["n_reports"][0] == 2
    c, before = cs["c_disagrees"]
    assert c.model(before)["pkt_status"].tolist() == [EINVAL, EINVAL, EINVAL, OK]
    c, before = cs["byte_0"]
    assert c.model(before)["pkt_status"].tolist() == [EINVAL, EINVAL, OK]
    c, before = cs["c_0_len_3"]
    assert c.model(before)["pkt_status"].tolist() == [EINVAL, OK]
    for name in ("len_above_max_len", "len_above_stride"):
        c, before = cs[name]
        o = c.model(before)
        assert o["pkt_status"].tolist() == [EINVAL, OK] and o["pkt_first"].tolist() == [F.NONE32, 0], name
    c, before = cs["F257"]
    o = c.model(before)
    bad = [f for f in range(257) if f % 5 == 2]
    assert np.flatnonzero(o["pkt_status"] == EINVAL).tolist() == bad and o["n_reports"][0] == 257 - len(bad)
    good = np.flatnonzero(o["pkt_status"] == OK)
    assert o["pkt_first"][good].tolist() == list(range(len(good))) and (o["pkt_count"][good] == 1).all()
    c, before = cs["one_packet_6553"]
    o = c.model(before)
    assert o["n_reports"][0] == 6553 and o["pkt_count"][0] == 6553
    c, before = cs["append_crosses_N_max"]
    o = c.model(before)
    assert (o["n_reports"][0], o["n_left"][0]) == (12, 4) and o["pkt_first"].tolist() == [8, 11, 13]
    assert np.array_equal(o["reports"][:8], before["reports"][:8])
    for name in ("append_base_at_N_max", "append_base_above_N_max"):
        c, before = cs[name]
        o = c.model(before)
        assert np.array_equal(o["reports"], before["reports"]) and (o["n_reports"][0], o["n_left"][0]) == (12, 8)
    c, before = cs["stale_length_without_append"]
    assert c.model(before)["pkt_first"].tolist() == [0, 3, 5]
    c, before = cs["F_0"]
    o = c.model(before)
    assert o["n_reports"][0] == 0 and np.array_equal(o["pkt_status"], before["pkt_status"])
    # values pass here and are judged by the credit update
    c, before = cs["values_pass"]
    o = c.model(before)
    assert o["reports"][:5].tolist() == [(F.ID_LIMIT, 2, 0), (F.U64MAX, 0, 0), (77, 5, 0), (78, 0xFFFF, 0),
                                         (0x0123456789ABCDEF, 1, 0)]
    win = np.zeros(3, np.uint64)
    cc = C.CreditCall(4, 1, 1, 16, win, np.zeros(3), np.zeros(3), o["reports"], int(o["n_reports"][0]), c.N_max)
    assert cc.statuses()[0] == [EINVAL, EINVAL, EINVAL, EINVAL, C.ENOTREADY]


def test_the_closed_model():
    cs = F.closed_cases()
    k = 4
    c, before = cs["no_eclosed"]
    o = c.model(before)
    assert o["n_reports"][0] == 0 and np.array_equal(o["reports"], before["reports"])
    c, before = cs["five_frames_one_generation"]
    o = c.model(before)
    assert o["n_reports"][0] == 1 and o["reports"][0].tolist() == (int(c.frame_id[0]), k, 0)
    c, before = cs["window_contradicts"]
    o = c.model(before)
    assert c.flags().tolist() == [0, 0, 0, 0, 1] and o["n_reports"][0] == 1
    c, before = cs["eclosed_on_id_2_62"]
    assert c.flags().tolist() == [0, 1, 0, 0, 0]
    for G in (3, 7):
        c, before = cs[f"last_id_G{G}"]
        o = c.model(before)
        assert o["n_reports"][0] == 1 and o["reports"][0].tolist() == (F.ID_LIMIT - 1, k, 0)
    c, before = cs["G_src_1"]
    o = c.model(before)
    assert o["n_reports"][0] == 1 and o["reports"][0].tolist() == (int(c.frame_id[0]), 256, 0)
    c, before = cs["shuffled"]
    o = c.model(before)
    n = int(o["n_reports"][0])
    ids = o["reports"]["id"][:n].astype(np.uint64)
    assert 20 < n < c.G_src and (np.diff((ids % np.uint64(c.G_src)).astype(np.int64)) > 0).all()
    c, before = cs["append_overflow"]
    o = c.model(before)
    assert (o["n_reports"][0], o["n_left"][0]) == (8, 1) and np.array_equal(o["reports"][:6], before["reports"][:6])
    c, before = cs["n_frames_mid"]
    assert c.model(before)["n_reports"][0] == 2


# ---------------------------------------------------------------------------
# the loop
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def loops(oracle):
    num, den, delay, mask = CHOSEN
    return {(m, rr): F.fb_loop(oracle, num, den, delay, m, rr) for m in (mask, None) for rr in (True, False)}


def repaired(loops):
    """The generations whose closing report was lost, of which a frame then arrived as QF_ECLOSED, and whose
    re-report brought the relay's peer to k."""
    w = loops[(F.MASK_LOOP, True)][2]
    return sorted(g for g in w["lost_close"] if g in w["eclosed_after"] and g in w["rereported"]
                  and w["peer"].get(g) == E.K_LOOP)


def test_the_chosen_run_loses_closing_reports_and_the_re_report_repairs_them(loops):
    assert (F.NUM_LOOP, F.DEN_LOOP) in ((1, 1), (3, 2), (2, 1)) and F.DELAY_LOOP in (1, 2)
    w, o = loops[(F.MASK_LOOP, True)][2], loops[(F.MASK_LOOP, False)][2]
    assert len(w["lost_close"]) >= 1
    gens = repaired(loops)
    assert len(gens) >= 2
    # without the re-report the relay never learns that they are done
    assert all(o["peer"].get(g, 0) < E.K_LOOP for g in gens)
    assert not o["rereported"]
    for key in loops:
        assert loops[key][2]["max_left"] == 0, key


@pytest.mark.parametrize("rr", [True, False])
@pytest.mark.parametrize("masked", [True, False])
def test_every_generation_is_delivered_once_within_the_cap(loops, masked, rr):
    spec, polls, stats = loops[(F.MASK_LOOP if masked else None, rr)]
    assert sorted(stats["delivered"]) == ALL          # (the loop itself asserts that none is delivered twice)
    assert stats["max_sent"] <= C.CAP_LOOP
    for p in polls:
        assert (p["q2"]["sent"] <= C.CAP_LOOP).all() and (p["credit_out"]["credit"] <= C.CAP_LOOP).all()
    assert masked == any(p["fb_drops"] for p in polls)


def test_frames_spent(loops):
    w, o = loops[(F.MASK_LOOP, True)][2], loops[(F.MASK_LOOP, False)][2]
    # no more frames with the re-report than without.  (Not fewer under this mask, nor under any of the masks
    # (a p + b j) % m == c with m <= 7 at the ratios and delays that deliver all twelve generations: the relay's
    # budget of a generation, at most ceil(3 k / 2) frames, is spent within the poll after the one that closes it,
    # which is when the re-report arrives.)
    assert w["frames"] <= o["frames"]
    assert (w["frames"], o["frames"]) == FRAMES_MASKED
    # with no feedback packet dropped nothing arrives as QF_ECLOSED unreported: the relay emits the same frames
    a, b = loops[(None, True)], loops[(None, False)]
    assert len(a[1]) == len(b[1])
    for pa, pb in zip(a[1], b[1]):
        for key in pa["q2"]:
            assert np.array_equal(pa["q2"][key], pb["q2"][key]), key


FRAMES_MASKED = (72, 72)   # the relay's frames with and without the re-report


def test_the_feedback_calls_of_the_loop(loops):
    spec, polls, stats = loops[(F.MASK_LOOP, True)]
    most = 0
    for p in polls:
        fo, out = p["pack_out"], p["closed_out"]
        n = int(out["n_reports"][0])
        assert int(fo["n_pkts"][0]) == -(-n // F.PER_LOOP) and fo["n_skipped"][0] == 0 and fo["n_left"][0] == 0
        most = max(most, n)
        assert len(set(out["reports"]["id"][:n].tolist())) == n        # a generation is reported once per poll
        po = p["parse_out"]
        assert (po["pkt_status"][: p["parse_call"].n_pkts] != F.FILL32).all()
    # (four slots give a poll three records at the most: one full packet of max_len 33.  Records that span
    # packets are the case tables' business.)
    assert most == F.PER_LOOP


def test_the_python_mirror():
    import ctypes
    import re
    from pathlib import Path

    from quicfuscate_amd import _lib, fec

    assert ctypes.sizeof(_lib.ReportWireShape) == 24
    assert [f[0] for f in _lib.ReportWireShape._fields_] == ["k", "max_len", "F_max", "flags", "stride"]
    hdr = (Path(__file__).resolve().parents[1] / "include" / "qf_fec.h").read_text()
    for name in ("qf_report_frame_capacity", "qf_frame_reports_dev", "qf_parse_report_frames_dev", "qf_report_closed_dev"):
        args = re.search(name + r"\(([^;]*)\);", hdr).group(1).split(",")
        assert len(args) == len(_lib._SIGS[name][1]), name
    assert callable(fec.frame_reports) and callable(fec.parse_report_frames) and callable(fec.report_closed)
