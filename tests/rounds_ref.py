"""Sizes for the tests of the persistent loops and workspace chunks
(test_gpu_rounds.py, checked without a GPU by test_rounds_cpu.py).

Most launches cap their grid and stride over their items.  A test reaches the
stride step, the index arithmetic past the first round and the ragged last
round only when the batch holds more items than one grid round covers.  This
module holds, per launch family, the items one round covers as a function of
the CU count (each function written from the launch code it cites), the items
a batch of G generations makes, and the smallest G that runs the loop a third,
partly filled time.  It also names the generated kernels by their table
letter, from build_lib.kernel_specs()."""
from __future__ import annotations

import dataclasses
import functools
from typing import Callable, Optional

GIB = 1 << 30
# launches that multiply the CU count by a runtime occupancy: the bound of 8
# blocks of 256 threads (32 waves) per CU; a case sized for it wraps for every
# smaller occupancy too
OCC_BOUND = 8


def r16(x: int) -> int:
    return (x + 15) // 16 * 16


def units(L: int) -> int:
    return (L + 15) // 16


def padded_units(L: int) -> int:
    """qf_bs.hip:234 bs_padded_units: the zero-tail lane space of a row."""
    return (units(L) + 7) // 8 * 8


# ---------------------------------------------------------------------------
# items of a batch
# ---------------------------------------------------------------------------
def cmb_geometry(L: int) -> tuple[int, int, int]:
    """qf_bs.hip:465 cmb_launch ("Lu = ..., Q = ..., ipg = ..."): units, lane-chunks
    and items per generation of the bit-sliced payload pass."""
    Lu = units(L)
    Q = (Lu + 1) // 2
    return Lu, Q, (Q + 63) // 64


def cmb_items(L: int, G: int) -> int:
    """qf_bs.hip:467 cmb_launch: n_items = G * ipg."""
    return G * cmb_geometry(L)[2]


def enc_items(L: int, G: int) -> int:
    """qf_bs.hip:161 launch(): n_items = ceil(G * Lv / 128), Lv the padded units
    (zero-tail encode, bs_launch, :250; the synw passes, synw_launch, :310)."""
    return (G * padded_units(L) + 127) // 128


def decc_items(L: int, G: int) -> int:
    """qf_bs.hip:154, :161 launch(), chunked: Lv = ceil(Lu / 2), n_items = ceil(G * Lv / 64)."""
    return (G * ((units(L) + 1) // 2) + 63) // 64


def unit_waves(L: int, G: int, V: int = 1) -> int:
    """qf_kernels.hip:1483 launch_slots_p, :1440 launch_uniform_rvp and
    qf_relay.hip:228 launch_combine_rows_at: waves = ceil(G * Lu / (64 V))."""
    return (G * units(L) + 64 * V - 1) // (64 * V)


# ---------------------------------------------------------------------------
# items one grid round covers
# ---------------------------------------------------------------------------
def cmb_round(num_cus: int) -> int:
    """qf_bs.hip:474 cmb_launch: blocks capped at 2 * num_cus; :485 the item
    stride (kernarg word 29) is blocks * 4 waves."""
    return 2 * num_cus * 4


def gen_round(num_cus: int, per_cu: int) -> int:
    """qf_bs.hip:173 launch(): QF_OPT_ENC/DEC_BLOCKS_PER_CU caps the grid at
    per_cu * num_cus 4-wave blocks; :191 item stride a[14] = blocks * 4."""
    return per_cu * num_cus * 4


def merged_round(num_cus: int, per_cu: int, waves: int) -> int:
    """qf_bs.hip:173 launch(), merged kernels ('M' / 'N' / 'Z'): a block is one
    item, cap = per_cu * num_cus * (4 / waves); :191 item stride a[14] = blocks."""
    return per_cu * num_cus * (4 // waves)


def occ_round(num_cus: int, occ: int = OCC_BOUND) -> int:
    """qf_kernels.hip:1485 launch_slots_p, :1442 launch_uniform_rvp,
    qf_relay.hip:213 launch_combine_rows_at: cap = num_cus * occupancy blocks of 4 waves."""
    return num_cus * occ * 4


def prepare_round(grid: int, lanes: bool) -> int:
    """qf_kernels.hip:1606-1620 launch_decode_prepare_cauchy with grid_cap (split-phase
    decode, QF_OPT_PREPARE_GRID): `grid` blocks of kPrepLanes = 128 generations
    (k_decode_prepare_lu_lanes) or of kPrepWaves = 4 (k_decode_prepare_lu)."""
    return grid * (128 if lanes else 4)


def wraps(items: int, rnd: int) -> bool:
    """The round condition: at least 2.25 rounds, the last one partly filled."""
    return 4 * items >= 9 * rnd and items % rnd != 0


def gens_for(items_of: Callable[[int], int], rnd: int, *, at_least: int = 1, avoid: int = 0) -> int:
    """The smallest G >= at_least whose items meet the round condition (and, for
    tiled batches, that is no multiple of the base length `avoid`)."""
    G = at_least
    while not wraps(items_of(G), rnd) or (avoid and G % avoid == 0):
        G += 1
    return G


# ---------------------------------------------------------------------------
# workspace chunks of the r > 16 decode
# ---------------------------------------------------------------------------
def synw_rows(L: int) -> bool:
    """qf_api.hip:663 decode_cauchy_enc: rows of >= 128 padded units read through
    the slot map (no gather)."""
    return 16 * padded_units(L) >= 16 * 128


def enc_chunk(k: int, r: int, L: int, synw: Optional[bool] = None) -> int:
    """qf_api.hip:665 decode_cauchy_enc: chunk = 2^30 / (((synw ? 0 : k) + r) * Lp)."""
    synw = synw_rows(L) if synw is None else synw
    return GIB // (((0 if synw else k) + r) * 16 * padded_units(L))


# ---------------------------------------------------------------------------
# kernel names by table letter (build_lib._bs_kernels)
# ---------------------------------------------------------------------------
def _letter(spec) -> str:
    from quicfuscate_amd import bs_codegen as bs
    from quicfuscate_amd import build_lib

    if isinstance(spec, bs.MergedSpec):
        if spec.mode == "synw":
            return ("Z" if spec.passes[0].xchg else "Y") if spec.fft else "X"
        return "N" if spec.fft else "M"
    if getattr(spec, "sliding", False):
        return "g"
    if spec.chunked:
        return "C" if spec.fft else "k" if spec.ksplit > 1 else "c"
    if spec.fft:
        return "E"
    if spec.mode == "enc" and spec.ksplit > 1:
        return "f"
    return {"enc": "e", "syn": "s", "dec": "d", "synw": "w", "cmb": build_lib._cmb_mode(spec)}[spec.mode]


@functools.lru_cache(maxsize=None)
def _table() -> tuple:
    from quicfuscate_amd import build_lib

    return tuple((_letter(s), s.k, s.rt, s.j0, s) for s in build_lib.kernel_specs())


def spec_of(letter: str, k: int, r: int):
    """The first-pass spec of table letter `letter` for (k, r); None if not built.
    Payload-pass kernels: k = 0 and r = outputs per pass (16 or 24)."""
    for lt, sk, srt, j0, s in _table():
        if lt == letter and sk == k and srt == r and j0 == 0:
            return s
    return None


def kernel(letter: str, k: int, r: int) -> Optional[str]:
    s = spec_of(letter, k, r)
    return s.name if s else None


def cmb_kernel(*, e_max: int, jump: int = 1, xcd: int = 0, wide: int = 1, pm24: int = 1) -> str:
    """The payload kernel qf_bs.hip cmb_entry picks for a launch over
    e_max = min(k, r) outputs (pass-major launches: e_max <= 64)."""
    passes = (e_max + 15) // 16
    if passes == 4 and pm24 and jump:                       # cmb_pm24_ok
        return kernel("W", 0, 24)
    if passes == 2 and e_max <= 24 and wide:                # cmb_wide_ok
        return kernel("j" if jump else "m", 0, 24)
    if passes == 1:
        return kernel("j" if jump else "m", 0, 16)
    if xcd and passes <= 4:
        return kernel("V" if jump else "Q", 0, 16)
    return kernel("J" if jump else "P", 0, 16)


def synw_kernel(k: int, r: int, *, shared: int = 1, fft: int = 1, merged: int = 1) -> str:
    """The syndrome kernel qf_bs.hip synw_launch picks."""
    if merged and fft and shared and spec_of("Z", k, r):
        return kernel("Z", k, r)
    if merged and fft and spec_of("Y", k, r):
        return kernel("Y", k, r)
    if merged and spec_of("X", k, r):
        return kernel("X", k, r)
    return kernel("w", k, r)


# ---------------------------------------------------------------------------
# the sized cases
# ---------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Case:
    """One sized case.  items(G) / rnd(num_cus): the loop it must wrap (round
    cases) or chunk > 0 (chunk cases: G fixed, G > chunk, G % chunk != 0).
    own_e: the generations' own erasure counts, dealt round-robin after a
    seeded shuffle.  rec_copies: recovered-row buffers alive at once (variants
    are compared with each other).  mem_limit: the device memory the case
    states for itself."""
    name: str
    k: int
    r: int
    L: int
    own_e: tuple
    items: Optional[Callable[[int], int]] = None
    rnd: Optional[Callable[[int], int]] = None
    chunk: int = 0
    fixed_G: int = 0
    at_least: int = 1
    avoid: int = 0
    ipg: int = 0            # claimed items per generation of the payload pass (0: not a payload case)
    passes: int = 0         # claimed 16-output record passes, ceil(min(k, r) / 16)
    rec_copies: int = 2
    rep_copies: int = 1
    mem_limit: int = GIB

    def G(self, num_cus: int) -> int:
        if self.fixed_G:
            return self.fixed_G
        return gens_for(self.items, self.rnd(num_cus), at_least=self.at_least, avoid=self.avoid)

    def ok(self, num_cus: int) -> bool:
        G = self.G(num_cus)
        if self.chunk:
            return G > self.chunk and G % self.chunk != 0
        return wraps(self.items(G), self.rnd(num_cus))

    def parts(self, num_cus: int) -> int:
        """Grid rounds (or workspace chunks) the batch spans."""
        G = self.G(num_cus)
        if self.chunk:
            return -(-G // self.chunk)
        return -(-self.items(G) // self.rnd(num_cus))

    def rep_row(self) -> int:
        return 16 * padded_units(self.L)

    def memory(self, num_cus: int) -> int:
        """Peak device bytes of the round trip: rows (sources, then repairs in
        the erased slots), the erased sources set aside (packed), the index
        arrays, and the larger of the repairs (freed before the decode) and
        the recovered rows (pattern up to the row stride)."""
        G = self.G(num_cus)
        k, r, L = self.k, self.r, self.L
        e_hi, e_sum = max(self.own_e), sum(self.own_e) * G // len(self.own_e) + len(self.own_e) * max(self.own_e)
        rows = G * k * r16(L)
        rep = G * r * self.rep_row()
        saved = e_sum * r16(L)
        rec = self.rec_copies * G * e_hi * (r16(L) + 16)
        idx = G * (2 * k + self.rec_copies * (2 * min(k, r) + 8))
        return rows + saved + max(self.rep_copies * rep, rec) + idx


def _cmb(L):
    return lambda G: cmb_items(L, G)


CASES = {c.name: c for c in [
    # A. the bit-sliced payload pass past two rounds (L = 2,100: Lu 132, Q 66, ipg 2)
    Case("cmb_one_pass", 64, 16, 2100, (12,), _cmb(2100), cmb_round, ipg=2, passes=1),
    Case("cmb_wide", 40, 20, 2100, (17,), _cmb(2100), cmb_round, ipg=2, passes=2),
    # four variants compared pairwise through the first: two buffers at a time
    Case("cmb_pass_major", 80, 40, 2100, (5, 20, 40), _cmb(2100), cmb_round, ipg=2, passes=3),
    # 100 sources + 64 repairs + up to 64 recovered rows of 2,100 bytes for
    # 2,304 generations: 0.49 GB of rows + 0.63 GB of recovered rows (two
    # variants at a time) + 0.2 GB set aside
    Case("cmb_pm24", 100, 64, 2100, (3, 30, 48, 49, 55, 64), _cmb(2100), cmb_round, ipg=2, passes=4,
         mem_limit=GIB * 3 // 2),
    # Q = 3 < 64: one mostly idle item per generation, item index = generation index
    Case("cmb_min_q", 64, 16, 96, (12,), _cmb(96), cmb_round, ipg=1, passes=1),
    # B. generated kernels on a grid capped at one block per CU
    Case("enc_capped", 64, 16, 1200, (13,), lambda G: enc_items(1200, G), lambda n: gen_round(n, 1)),
    Case("dec_capped", 64, 16, 1200, (13,), lambda G: decc_items(1200, G), lambda n: gen_round(n, 1)),
    # merged C5 encode 'N' of (160, 48): 3 coset passes + a producer wave = 4 waves, one item per block
    Case("c5_enc_capped", 160, 48, 2048, (3, 20, 48), lambda G: enc_items(2048, G),
         lambda n: merged_round(n, 1, 4), rec_copies=1),
    # ... and its decode: the pass-major syndrome kernels ('X' / 'Y': 4-wave
    # blocks) need 2.25 * 4 * num_cus items of one generation each; 160 rows
    # of 2,048 bytes for 2,304 generations are 0.76 GB by themselves
    Case("c5_dec_capped", 160, 48, 2048, (3, 20, 48), lambda G: enc_items(2048, G),
         lambda n: gen_round(n, 1), mem_limit=GIB * 3 // 2),
    # k_combine_uniform<16, 1, PD> / k_combine_slots<PD>: num_cus * occupancy blocks
    # (sized for the occupancy bound: 15,728 generations, whose repairs exist
    # twice, from the general and from the bit-sliced encode: 2 x 0.32 GB)
    Case("slots_uniform", 16, 16, 1200, (16, 9, 1), lambda G: unit_waves(1200, G), occ_round, rec_copies=1,
         rep_copies=2, mem_limit=GIB * 9 // 8),
    # C. the second workspace chunk of the r > 16 decode
    # gather path: 5,700 x 128 rows of 1,200 bytes = 0.88 GB of rows
    Case("chunk_gather", 128, 20, 1200, (20,), chunk=enc_chunk(128, 20, 1200), fixed_G=5700, rec_copies=1,
         mem_limit=GIB * 5 // 4),
    # synw path: 8,900 x 196 rows of 2,048 bytes = 3.6 GB of rows, 1.1 GB of
    # repairs, 1.1 GB of recovered rows, 0.6 GB set aside
    Case("chunk_synw", 196, 59, 2040, (3, 20, 40, 59), chunk=enc_chunk(196, 59, 2040), fixed_G=8900,
         rec_copies=1, mem_limit=GIB * 11 // 2),
]}


def tiled_G(rnd: int, base: int, *, at_least: int = 1) -> int:
    """G of a tiled batch over `base` generations whose items are the
    generations themselves (the acceptance pass)."""
    return gens_for(lambda G: G, rnd, at_least=at_least, avoid=base)
