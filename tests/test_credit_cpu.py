"""Properties of tests/credit_ref.py, the models of qf_rank_report_sel_dev and
qf_credit_update_dev, and of the lossy loop under them: what the device test
then holds the library to.  CPU only; nothing here needs a library symbol."""
import numpy as np
import pytest

from tests import credit_ref as C
from tests import emit_ref as E

OK, EINVAL, ENOTREADY, ESTALE = C.OK, C.EINVAL, C.ENOTREADY, C.ESTALE
ALL = list(range(E.GENS_LOOP))


@pytest.fixture(scope="module")
def loops(oracle):
    """(num, den, reports) -> the loop, each run once."""
    return {key: C.lossy_loop(oracle, *key) for key in ((1, 1, False), (1, 1, True), (3, 2, False), (3, 2, True))}


# ---------------------------------------------------------------------------
# the loop
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("key", [(1, 1, True), (3, 2, False), (3, 2, True)])
def test_every_generation_is_delivered_once(loops, key):
    spec, polls, stats = loops[key]
    assert sorted(stats["delivered"]) == ALL          # (the loop itself asserts that none is delivered twice)
    # the mask takes one frame in five of every generation's frames
    n_drops = sum(len(p["drops"]) for p in polls)
    assert n_drops == sum(sum(C.dropped2(g, i) for i in range(n)) for g, n in stats["emitted"].items())
    assert n_drops >= E.GENS_LOOP // 2


def test_todays_budget_does_not_survive_the_mask(loops):
    spec, polls, stats = loops[(1, 1, False)]
    assert len(stats["delivered"]) < E.GENS_LOOP
    # ... and it is today's budget: every generation sends exactly its rank
    assert all(n == E.K_LOOP for n in stats["emitted"].values()) and stats["frames"] == E.GENS_LOOP * E.K_LOOP
    for p in polls:
        assert np.array_equal(p["credit_out"]["credit"], np.minimum(p["credit_call"].rank, E.K_LOOP))


def test_frames_spent(loops):
    frames = {key: loops[key][2]["frames"] for key in loops}
    # reports cost fewer frames than blind redundancy, and stop finished generations early
    assert frames[(1, 1, False)] < frames[(1, 1, True)] < frames[(3, 2, True)] < frames[(3, 2, False)]
    assert frames[(3, 2, False)] == E.GENS_LOOP * C.ceil_rho(E.K_LOOP, 3, 2)


@pytest.mark.parametrize("key", [(1, 1, False), (1, 1, True), (3, 2, False), (3, 2, True)])
def test_bounds(loops, key):
    spec, polls, stats = loops[key]
    assert stats["max_sent"] <= C.CAP_LOOP
    for p in polls:
        assert (p["q2"]["sent"] <= C.CAP_LOOP).all() and (p["credit_out"]["credit"] <= C.CAP_LOOP).all()
    # a generation whose peer reported k emits nothing afterwards
    assert not stats["after_k"]
    if key[2]:
        assert len(stats["satisfied"]) >= E.GENS_LOOP // 2
    # the loop came to rest by itself, with empty polls behind the schedule
    assert len(polls) > len(E.SCHED) or not key[2]
    assert not polls[-1]["listed"]


def test_the_reports_of_the_loop(loops):
    spec, polls, stats = loops[(1, 1, True)]
    kinds = set()
    for p in polls:
        ra, rb = p["report_calls"]
        oa, ob = p["report_out"]
        n_a, n = int(oa["n_reports"][0]), int(ob["n_reports"][0])
        assert n_a == len(p["done"]) and int(ob["n_left"][0]) == 0
        assert (ob["reports"]["rank"][:n_a] == E.K_LOOP).all()                 # closed: k, though the rank is zeroed
        assert ((ob["reports"]["rank"][n_a:n] >= 1) & (ob["reports"]["rank"][n_a:n] < E.K_LOOP)).all()
        assert len(set(ob["reports"]["id"][:n].tolist())) == n
        kinds |= {"done"} if n_a else set()
        kinds |= {"short"} if n > n_a else set()
    assert kinds == {"done", "short"}
    # a short report made the relay send again
    assert any((p["credit_out"]["credit"] > np.minimum(p["credit_call"].rank, E.K_LOOP)).any() for p in polls)


# ---------------------------------------------------------------------------
# the models on hand-written inputs
# ---------------------------------------------------------------------------
def test_without_redundancy_and_reports_the_credit_is_the_rank():
    rng = np.random.default_rng(1)
    for k, cap in ((4, 16), (64, 40), (256, 1 << 20)):
        c, before = C.make_credit(130, k, 7, 7, cap, 0, 300 + k)
        before = c.blank()                                     # a first call: no state, no previous credit
        o = c.model(before)
        want = np.where(c.win == 0, 0, np.minimum(np.minimum(c.rank, k), cap))
        assert np.array_equal(o["credit"], want) and (c.rank > k).any() and (c.win == 0).any()
        assert (o["state"]["peer"] == 0).all() and np.array_equal(o["state"]["owner"] != 0, c.win != 0)
    assert rng is not None


def test_the_sequences():
    q = C.credit_sequences()
    o = C.run_sequence(q["restart"])
    assert o[0]["credit"].tolist() == [6, 6, 3, 0] and o[0]["state"]["peer"].tolist() == [0, 3, 0, 0]
    assert o[1]["credit"].tolist() == [6, 2, 3, 0] and o[1]["state"]["peer"].tolist() == [0, 0, 0, 0]
    o = C.run_sequence(q["repeat"])
    # twice in one call: once; in the next call: again; no report: nothing more; rank k: sent; a lower report: still k
    assert [x["credit"][2] for x in o] == [5, 7, 7, 7, 7]
    assert [x["state"]["peer"][2] for x in o] == [1, 1, 1, 4, 4]
    assert o[0]["status"].tolist() == [OK, OK]
    o = C.run_sequence(q["closed_then_empty"])
    assert o[0]["credit"][0] == 3 and o[0]["status"].tolist() == [OK]
    assert o[1]["credit"][0] == 0 and o[1]["status"].tolist() == [ENOTREADY] and o[1]["state"][0].tolist() == (0, 0, 0)
    o = C.run_sequence(q["cap"])
    assert o[0]["credit"].tolist() == [9, 9, 9, 0] and o[1]["credit"].tolist() == [7, 7, 7, 0]


def test_statuses_and_the_maximum():
    cs = C.credit_cases()
    c, before = cs["id_edges"]
    o = c.model(before)
    assert o["status"].tolist() == [OK, EINVAL, EINVAL, EINVAL]
    s = (C.ID_LIMIT - 1) % c.G
    assert o["state"][s].tolist() == (C.ID_LIMIT, 2, 0) and o["credit"][s] == 3    # max(3, 1 + (3 - 2))
    c, before = cs["one_slot_many_waves"]
    o = c.model(before)
    assert o["state"]["peer"].tolist() == [0, 57, 0, 0, 0] and o["credit"].tolist() == [0, 60, 0, 0, 0]
    c, before = cs["n_reports_mid"]
    o = c.model(before)
    assert (o["status"][17:] == -858993460).all() and (o["status"][:17] != -858993460).all()
    c, before = cs["no_status"]
    assert np.array_equal(c.model(before)["status"], before["status"])
    seen = set()
    for name, (c, before) in cs.items():
        seen |= set(c.statuses()[0])
        o = c.model(before)
        assert (o["credit"][c.win == 0] == 0).all(), name
        sat = o["state"]["peer"] >= c.k
        assert np.array_equal(o["credit"][sat], c.sent[sat]), name
        assert (o["credit"][~sat] <= c.cap).all(), name
    assert seen == {OK, EINVAL, ENOTREADY, ESTALE}


def test_the_report_model():
    cs = C.report_cases()
    c, before, _ = cs["overflow"]
    o = c.model(before)
    assert (o["n_reports"][0], o["n_left"][0]) == (12, 8)
    for name, (n, left) in dict(base0=(20, 0), base_mid=(27, 0), base_fits=(30, 0), base_full=(30, 20),
                                base_above=(30, 20)).items():
        c, before, _ = cs[f"append_{name}"]
        o = c.model(before)
        base = min(int(before["n_reports"][0]), c.N_max)
        assert (o["n_reports"][0], o["n_left"][0]) == (n, left), name
        assert np.array_equal(o["reports"][:base], before["reports"][:base])
        assert np.array_equal(o["reports"][n:], before["reports"][n:])
    c, before, _ = cs["n_max65"]
    o = c.model(before)
    kinds = set()
    for j in range(c.n_max):
        s, rec = int(c.sel[j]), o["reports"][j].tolist()
        if s >= c.G_src or c.win[s] == 0:
            assert rec == (C.U64MAX, 0, 0)
            kinds.add("hole")
        elif int(c.win[s]) & C.CLOSED:
            assert rec == (C.held(c.win[s]) - 1, c.k, 0)
            kinds.add("closed")
        else:
            assert rec == (int(c.win[s]) - 1, min(int(c.rank[s]), c.k), 0)
            kinds.add("clamped" if c.rank[s] > c.k else "open")
    assert kinds == {"hole", "closed", "open", "clamped"}
    c, before, _ = cs["n_sel_0"]
    o = c.model(before)
    assert o["n_reports"][0] == 0 and np.array_equal(o["reports"], before["reports"])


def test_the_python_mirror():
    import ctypes
    import re
    from pathlib import Path

    from quicfuscate_amd import _lib, fec

    assert ctypes.sizeof(_lib.CreditShape) == 24
    assert [f[0] for f in _lib.CreditShape._fields_] == ["k", "num", "den", "cap", "flags", "reserved"]
    assert np.dtype(_lib.RANK_REPORT_DTYPE) == C.REPORT and fec.QF_REPORT_APPEND == 1
    hdr = (Path(__file__).resolve().parents[1] / "include" / "qf_fec.h").read_text()
    for name in ("qf_rank_report_sel_dev", "qf_credit_update_dev"):
        args = re.search(name + r"\(([^;]*)\);", hdr).group(1).split(",")
        assert len(args) == len(_lib._SIGS[name][1]), name
    assert callable(fec.rank_report_sel) and callable(fec.credit_update)
