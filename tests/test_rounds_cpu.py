"""The sized cases of test_gpu_rounds.py, checked without a GPU: at 256 CUs
every case wraps its loop into a third, partly filled round (or crosses its
workspace chunk with a ragged second chunk), has the payload-pass geometry it
claims, and fits the device memory it states."""
import pytest

from tests import rounds_ref as rr

NUM_CUS = 256


@pytest.mark.parametrize("name", sorted(rr.CASES))
def test_case_meets_its_round_or_chunk_condition(name):
    c = rr.CASES[name]
    G = c.G(NUM_CUS)
    assert c.ok(NUM_CUS), (name, G)
    if c.chunk:
        assert G > c.chunk and G % c.chunk != 0
        assert c.parts(NUM_CUS) == 2
    else:
        items, rnd = c.items(G), c.rnd(NUM_CUS)
        assert 4 * items >= 9 * rnd and items % rnd != 0, (name, G, items, rnd)
        assert c.parts(NUM_CUS) >= 3
        # the smallest such G: one generation fewer misses the condition
        assert G == c.at_least or not rr.wraps(c.items(G - 1), rnd)
    # a smaller device only adds rounds
    for n in (64, 128, 304):
        assert c.ok(n), (name, n)


@pytest.mark.parametrize("name", sorted(rr.CASES))
def test_case_geometry_and_memory(name):
    c = rr.CASES[name]
    if c.ipg:
        assert rr.cmb_geometry(c.L)[2] == c.ipg
        assert (min(c.k, c.r) + 15) // 16 == c.passes
    mem = c.memory(NUM_CUS)
    assert mem <= c.mem_limit, (name, mem / rr.GIB)
    # only the cases that say so go past 1 GiB
    assert c.mem_limit == rr.GIB or mem > rr.GIB, name
    assert all(0 < e <= min(c.k, c.r) for e in c.own_e)


def test_payload_pass_geometry_of_the_long_rows():
    # L = 2,100: a partial last unit, two items per generation (the magic
    # division by ipg), Q no multiple of 64 (a partly filled second item)
    assert rr.cmb_geometry(2100) == (132, 66, 2)
    assert 2100 % 16 and 66 % 64
    assert rr.cmb_geometry(96) == (6, 3, 1)
    assert rr.cmb_round(NUM_CUS) == 2048
    assert rr.CASES["cmb_one_pass"].G(NUM_CUS) == 2304
    assert rr.CASES["cmb_min_q"].G(NUM_CUS) == 4608
    # the 24-output launch runs ceil(e_max / 24) = 3 passes at e_max = 64 and
    # the third serves the generations with 49 to 64 erasures of their own
    assert {e for e in rr.CASES["cmb_pm24"].own_e if e > 48} == {49, 55, 64}


def test_chunk_lengths():
    # 2^30 / (148 * 1,280) = 5,667.97: the division truncates
    assert rr.enc_chunk(128, 20, 1200) == 5667 and not rr.synw_rows(1200)
    assert rr.enc_chunk(196, 59, 2040) == 8886 and rr.synw_rows(2040)
    # (196, 59) with 9,000-byte rows: the figure of the decode's own comment
    assert rr.enc_chunk(196, 59, 9000) == 2002


def test_capped_grid_rounds():
    assert rr.gen_round(NUM_CUS, 1) == 1024
    # (160, 48): three coset passes and a producer-only wave share a block
    n = rr.spec_of("N", 160, 48)
    assert n is not None and n.waves == 4
    assert rr.merged_round(NUM_CUS, 1, n.waves) == 256
    z = rr.spec_of("Z", 160, 48)
    assert z is not None and 4 // z.waves == 1
    assert rr.occ_round(NUM_CUS) == 8192
    assert rr.prepare_round(4, True) == 512 and rr.prepare_round(4, False) == 16
    G = rr.tiled_G(rr.prepare_round(4, True), 251, at_least=2048)
    assert G >= 2048 and G % 251 and rr.wraps(G, 512)


def test_kernel_names_come_from_the_spec_table():
    names = {rr.cmb_kernel(e_max=16, jump=1), rr.cmb_kernel(e_max=16, jump=0),
             rr.cmb_kernel(e_max=20, wide=1, jump=1), rr.cmb_kernel(e_max=20, wide=1, jump=0),
             rr.cmb_kernel(e_max=40, jump=1, xcd=0), rr.cmb_kernel(e_max=40, jump=0, xcd=0),
             rr.cmb_kernel(e_max=40, jump=1, xcd=1), rr.cmb_kernel(e_max=40, jump=0, xcd=1),
             rr.cmb_kernel(e_max=64, pm24=1)}
    assert None not in names and len(names) == 9
    assert rr.cmb_kernel(e_max=20, wide=0) == rr.cmb_kernel(e_max=40)           # two 16-output passes, pass-major
    assert rr.cmb_kernel(e_max=64, pm24=0) == rr.cmb_kernel(e_max=40)
    assert rr.cmb_kernel(e_max=48, pm24=1) == rr.cmb_kernel(e_max=48, pm24=0)   # the rule: e_max 49 to 64 only
    assert rr.cmb_kernel(e_max=64, pm24=1).startswith("qf_combine_bs_r24_pm_j")
    for k, r in ((128, 20), (128, 39), (160, 48), (196, 59)):
        z, y = rr.synw_kernel(k, r, shared=1), rr.synw_kernel(k, r, shared=0)
        assert z and y and z != y, (k, r)
    assert rr.kernel("g", 32, 5).endswith("_sl") and rr.kernel("g", 64, 10) is None
