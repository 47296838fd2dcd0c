"""Public options that no other GPU test sets, at small shapes against the
CPU oracle: every value of encode_pd x encode_v on the general encode
(k_combine_uniform<R, V, PD>) and every value of decode_pd on the general
payload pass (k_combine_slots<PD>).  Each case also asserts, through the
context's kernel timing, that the instantiation the option selects is the one
that ran, so an option that turned into a no-op fails here."""
import re

import numpy as np
import pytest

from tests.test_gpu_decode import _path, check, make_batch, run_decode
from tests.test_gpu_encode import _r16, run_encode

pytestmark = pytest.mark.gpu


def _profiled(qf, fn):
    ctx = qf.default_context()
    ctx.sync()
    ctx.profile(True)
    try:
        out = fn()
        return out, set(ctx.kernel_times())
    finally:
        ctx.profile(False)


@pytest.mark.parametrize("k,r,L,G", [(7, 5, 33, 11), (63, 16, 1201, 7), (64, 40, 100, 3), (200, 56, 48, 1),
                                     (96, 15, 9000, 2)])
@pytest.mark.parametrize("V", [1, 2])
@pytest.mark.parametrize("pd", [1, 2, 3])
def test_encode_prefetch_depth_and_units_per_lane(qf, oracle, gpu_ctx, k, r, L, G, V, pd):
    """encode_pd in {1, 2, 3} x encode_v in {1, 2} with bitsliced = 0: odd k
    and r with a tail unit, k % 4 = 3 with L % 16 = 1, passes of 16 repairs,
    k + r = 256, a jumbo row.  Every repair byte equals the oracle's and the
    bytes past L are untouched."""
    qf.set_default_options(bitsliced=0, encode_small=0, encode_v=V, encode_pd=pd)
    rng = np.random.default_rng(k * 1000 + r * 10 + L + 7)
    rs = _r16(L) + (16 if k % 2 else 0)
    gs = k * rs + 32
    rrs = _r16(L) + 16
    rgs = r * rrs + 48
    src = rng.integers(0, 256, G * gs, dtype=np.uint8)
    rep, names = _profiled(qf, lambda: run_encode(qf, src, k, r, L, G, rs, gs, rrs, rgs))
    # qf_api.hip encode: a pass of 9 to 16 repairs runs one unit per lane, and
    # two units per lane hold at most two row pairs in flight
    v_eff = 1 if r >= 9 else V
    pd_eff = min(pd, 2 if v_eff == 2 else 3)
    tags = set()
    for n in names:
        m = re.fullmatch(r"k_combine_uniform<(\d+),(\d+),(\d+)>", n)
        assert m, names
        tags.add((int(m.group(2)), int(m.group(3))))
    assert tags == {(v_eff, pd_eff)}, (names, v_eff, pd_eff)
    for g in range(G):
        rows = np.stack([src[g * gs + i * rs: g * gs + i * rs + L] for i in range(k)])
        want = oracle.encode(rows, r)
        for j in range(r):
            off = g * rgs + j * rrs
            assert (rep[off: off + L] == want[j]).all(), (g, j)
            assert (rep[off + L: off + rrs] == 0xA5).all(), "bytes past L written"
        assert (rep[g * rgs + r * rrs: (g + 1) * rgs] == 0xA5).all()


@pytest.mark.parametrize("k,r,L,G,erase", [(64, 16, 1200, 40, None), (33, 7, 37, 25, None), (40, 40, 80, 12, 33),
                                           (128, 39, 1000, 6, None)])
@pytest.mark.parametrize("path", ["syn", "general"])
@pytest.mark.parametrize("pd", [1, 2, 3])
def test_decode_prefetch_depth(qf, oracle, gpu_ctx, k, r, L, G, erase, path, pd):
    """decode_pd in {1, 2, 3}: k_combine_slots<PD> (combine_bs = 0,
    combine_split = 0) behind the syndrome kernels and behind the general
    Gauss-Jordan, one to three passes of 16 outputs, bit-exact."""
    _path(None, path)
    qf.set_default_options(combine_bs=0, combine_split=0, decode_pd=pd)
    rng = np.random.default_rng(k * 17 + r + L)
    max_rows = k + r
    kw = {} if erase is None else {"erase": erase}
    src, gens = make_batch(oracle, rng, k, r, L, G, max_rows, **kw)
    out, names = _profiled(qf, lambda: run_decode(qf, k, r, L, G, max_rows, gens, False))
    payload = {n for n in names if n.startswith("k_combine_slots") or n.startswith("qf_combine_bs")}
    assert payload == {f"k_combine_slots<{pd}>"}, names
    check(oracle, k, L, src, gens, out, False)
