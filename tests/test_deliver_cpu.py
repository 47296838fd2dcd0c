"""tests/deliver_ref.py pinned by hand-written cases, and the streaming loop
with the deliver steps under the models alone: every (wire generation, source)
pair some decode determines leaves exactly once, with the source's bytes,
across deadline flushes, displacement and completion.  CPU only."""
import numpy as np
import pytest

from tests import deliver_ref as R

OK, EINVAL, ENOTREADY = R.OK, R.EINVAL, R.ENOTREADY
U, S, D, E = R.UNKNOWN, R.STORED, R.RECOVERED, R.EARLIER


def _one(k=4, e_max=2, L=20, mr=6, **kw):
    return R.simple_shape(k, e_max, L, mr, **kw)


def test_a_generation_leaves_in_source_order_with_its_lengths():
    rng = np.random.default_rng(1)
    sh = _one()
    c = R.synth(rng, sh, [dict(stored={0: (3, 20), 2: (0, 7)}, D=[3]), dict(stored={1: (5, 16)}, D=[], status=ENOTREADY)])
    o = c.model()
    assert o["status"].tolist() == [OK, OK] and o["n_out"].tolist() == [3, 1] and o["n_known"].tolist() == [3, 1]
    assert o["out_len"].tolist() == [20, 0, 7, 20, 0, 16, 0, 0]
    assert o["out_state"].tolist() == [S, U, S, D, U, S, U, U]
    out = o["out"].reshape(2, sh.out_gs)
    rs = sh.out_rs
    # source 2: 7 bytes, zero to the end of its unit, nothing behind it
    got = out[0, 2 * rs: 3 * rs]
    at = int(c.row_off[0, 0])
    assert np.array_equal(got[:7], c.src[at: at + 7]) and not got[7:16].any() and (got[16:] == R.FILL).all()
    # source 3 from rec row 0: L bytes, zero to the end of the second unit
    got = out[0, 3 * rs: 4 * rs]
    assert np.array_equal(got[:20], c.dec["rec"][:20]) and not got[20:32].any()
    # source 1 of generation 0 is unknown: no byte of its row is written
    assert (out[0, rs: 2 * rs] == R.FILL).all() and (out[0, 4 * rs:] == R.FILL).all()
    assert [i for i, _ in o["packets"][0]] == [0, 2, 3] and o["delivered"] is None


def test_every_status():
    rng = np.random.default_rng(2)
    sh = _one()
    specs = [dict(stored={0: (0, 5)}, D=[1], status=OK), dict(stored={0: (0, 5)}, status=ENOTREADY),
             dict(stored={0: (0, 5)}, status=EINVAL), dict(stored={0: (0, 5)}, status=-4), dict(stored={0: (0, 5)}, status=7)]
    o = R.synth(rng, sh, specs).model()
    assert o["status"].tolist() == [OK, OK, ENOTREADY, ENOTREADY, ENOTREADY]
    assert o["n_out"].tolist() == [2, 1, 0, 0, 0] and not o["out_len"][8:].any() and not o["out_state"][8:].any()
    assert (o["out"][2 * sh.out_gs:] == R.FILL).all()
    # the listed form: an invalid entry is QF_EINVAL whatever the decode said, an unused one QF_ENOTREADY
    c = R.synth(rng, sh, specs[:2], G_src=2)
    dec = R.synth(rng, sh, [specs[1], specs[0], specs[0], specs[0]]).dec
    c4 = R.Call(sh, 4, c.src, c.row_off, c.row_len, dec, sel=[1, 0, 2, 0], n_sel=3, G_src=2)
    o = c4.model()
    assert o["status"].tolist() == [OK, OK, EINVAL, ENOTREADY] and o["n_out"].tolist() == [1, 2, 0, 0]
    at = 1 * sh.src_gs + int(c.row_off[1, 0])
    assert np.array_equal(o["out"][:5], c.src[at: at + 5])
    assert R.Call(sh, 4, c.src, c.row_off, c.row_len, dec, sel=[1, 0, 2, 0], G_src=2).model()["status"][3] == OK


@pytest.mark.parametrize("what", R.INCONSISTENT)
def test_each_inconsistency(what):
    assert R.inconsistent_call("none").model()["status"].tolist() == [OK] * 3
    c = R.inconsistent_call(what)
    sh = c.sh
    o = c.model()
    assert o["status"].tolist() == [OK, EINVAL, OK] and o["n_out"].tolist() == [4, 0, 4]
    assert not o["out_len"][5:10].any() and not o["out_state"][5:10].any() and o["n_known"][1] == 0
    assert (o["out"][sh.out_gs: 2 * sh.out_gs] == R.FILL).all() and not o["delivered"][1].any()
    assert o["delivered"][0].tolist() == [6, 0b11011, 0, 0, 0]


def test_the_state_makes_a_source_leave_once():
    rng = np.random.default_rng(4)
    sh = _one()
    c = R.synth(rng, sh, [dict(stored={0: (0, 20), 1: (1, 9)}, status=ENOTREADY)])
    c.delivered, c.ids = np.zeros((1, R.WORDS), np.uint64), np.array([41], np.uint64)
    first = c.model()
    assert first["n_out"][0] == 2 and first["delivered"][0].tolist() == [42, 0b0011, 0, 0, 0]
    # the same inputs again: nothing leaves, nothing is written to out or the state
    again = c.model(delivered=first["delivered"])
    assert again["n_out"][0] == 0 and again["n_known"][0] == 2 and again["status"][0] == OK
    assert again["out_state"].tolist() == [E, E, U, U] and not again["out_len"].any()
    assert (again["out"] == R.FILL).all() and np.array_equal(again["delivered"], first["delivered"])
    # more rows arrive: only the new sources leave
    more = R.synth(np.random.default_rng(4), sh, [dict(stored={0: (0, 20), 1: (1, 9), 3: (2, 4)}, D=[2])])
    more.delivered, more.ids = first["delivered"], c.ids
    o = more.model()
    assert o["out_state"].tolist() == [E, E, D, S] and o["n_out"][0] == 2 and o["n_known"][0] == 4
    assert o["delivered"][0].tolist() == [42, 0b1111, 0, 0, 0]
    # a changed id restarts the mask
    more.ids = np.array([45], np.uint64)
    o = more.model()
    assert o["out_state"].tolist() == [S, S, D, S] and o["delivered"][0].tolist() == [46, 0b1111, 0, 0, 0]
    # ... but not when nothing is known: the state stays the old generation's
    none = R.synth(rng, sh, [dict(status=ENOTREADY)])
    none.delivered, none.ids = first["delivered"], np.array([45], np.uint64)
    o = none.model()
    assert o["n_out"][0] == 0 and o["n_known"][0] == 0 and np.array_equal(o["delivered"], first["delivered"])


def test_ids_null_and_bad_ids():
    rng = np.random.default_rng(5)
    sh = _one()
    c = R.synth(rng, sh, [dict(stored={2: (0, 1)}, D=[0])] * 3)
    # without ids the tag is neither read nor written
    c.delivered = np.zeros((3, R.WORDS), np.uint64)
    c.delivered[:, 0] = 99
    c.delivered[1, 1] = 0b0100
    o = c.model()
    assert o["n_out"].tolist() == [2, 1, 2] and o["out_state"][4:8].tolist() == [D, U, E, U]
    assert o["delivered"].tolist() == [[99, 0b0101, 0, 0, 0]] * 3
    # UINT64_MAX (no generation) and ids at and above 2^62
    c.ids = np.array([(1 << 64) - 1, 1 << 62, (1 << 62) - 1], np.uint64)
    o = c.model()
    assert o["status"].tolist() == [EINVAL, EINVAL, OK] and o["delivered"][2].tolist() == [1 << 62, 0b0101, 0, 0, 0]
    assert np.array_equal(o["delivered"][:2], c.delivered[:2])
    # without a state the ids are not looked at and every known source is new
    c.delivered = None
    assert c.model()["status"].tolist() == [OK] * 3 and c.model()["n_out"].tolist() == [2] * 3


def test_rows_of_length_zero_k_1_and_wide_masks():
    rng = np.random.default_rng(6)
    sh = R.simple_shape(1, 1, 33, 2)
    c = R.synth(rng, sh, [dict(stored={0: (1, 0)}), dict(D=[0]), dict(status=ENOTREADY)])
    o = c.model()
    assert o["status"].tolist() == [OK] * 3 and o["n_out"].tolist() == [1, 1, 0]
    assert o["out_len"].tolist() == [0, 33, 0] and o["out_state"].tolist() == [S, D, U]
    assert (o["out"][: sh.out_gs] == R.FILL).all()                     # a packet of length 0 writes nothing
    assert not o["out"][sh.out_gs + 33: sh.out_gs + 48].any()
    # k = 200: the four mask words
    sh = R.simple_shape(200, 8, 5, 200)
    spec = dict(stored={i: (199 - i, 5) for i in (0, 63, 64, 127, 128, 199)}, D=[191, 192], status=ENOTREADY)
    c = R.synth(rng, sh, [spec])
    c.delivered, c.ids = np.zeros((1, R.WORDS), np.uint64), np.array([0], np.uint64)
    o = c.model()
    assert o["delivered"][0].tolist() == [1, 1 | 1 << 63, 1 | 1 << 63, 1 | 1 << 63, 1 | 1 << 7]


def test_the_loop_delivers_every_determined_source_once():
    src, stream, polls, last, stats = R.loop_model()
    R.check_exactly_once(src, stats["left"], stats["determined"])
    R.check_loop_stats(stats)
    # every generation with a surviving frame had something determined, and a complete one all of it
    assert sorted(stats["determined"]) == [g for g in range(R.GENS_LOOP) if stream[g]]
    whole = [g for g, known in stats["determined"].items() if len(known) == R.K_LOOP]
    assert len(whole) >= stats["completed"]
    # the state words name the generation that last left through a slot
    state = last.flush.res["delivered"]
    assert all(int(w[0]) == 0 or R.BASE_LOOP <= int(w[0]) - 1 < R.BASE_LOOP + R.GENS_LOOP for w in state)
