"""Reference of qf_frame_reports_dev, qf_parse_report_frames_dev and
qf_report_closed_dev -- TEST INFRASTRUCTURE ONLY.

The three calls restated in plain numpy from the rules written in
include/qf_fec.h above them (ids on Python ints).  Nothing here touches the
library under test.

PackCall / ParseCall / ClosedCall: the inputs of one call and model(), which
              returns every output buffer whole, as the call leaves it when it
              starts from `before` (default: every byte 0xCC).  `nulls` names the
              nullable outputs the call is given as NULL: they stay as they were.
pack_cases, parse_cases, closed_cases: the named calls of the device test and
              of the host-emulation test.
fb_loop:      credit_ref.lossy_loop with the back channel as bytes: the
              receiver's two report lists, the re-report appended, the pack; a
              drop mask on the feedback packets and a delay of whole polls; the
              relay's parse in front of its credit update."""
from __future__ import annotations

import functools

import numpy as np

from tests import credit_ref as C
from tests import emit_ref as E

OK, EINVAL, ENOTREADY, ECLOSED = 0, -1, -3, -9
FILL, FILL32 = C.FILL, C.FILL32
U64MAX, ID_LIMIT, CLOSED = C.U64MAX, C.ID_LIMIT, C.CLOSED
REPORT = C.REPORT
NONE32 = 0xFFFFFFFF
KIND = 0x02
ENTRY = 10
poisoned, records = C.poisoned, C.records


def capacity(max_len: int) -> int:
    return (max_len - 3) // ENTRY if 13 <= max_len <= 65535 else 0


def sendable(rec, k: int) -> bool:
    return int(rec["id"]) < ID_LIMIT and int(rec["rank"]) <= k and int(rec["reserved"]) == 0


def packet(entries) -> bytes:
    """[(id, rank), ...] -> the bytes of one feedback packet."""
    out = bytes([KIND]) + len(entries).to_bytes(2, "big")
    for x, r in entries:
        out += int(x).to_bytes(8, "big") + int(r).to_bytes(2, "big")
    return out


def _keep(o: dict, before: dict, nulls) -> dict:
    for key in nulls:
        o[key] = before[key].copy()
    return o


# ---------------------------------------------------------------------------
# qf_frame_reports_dev
# ---------------------------------------------------------------------------
class PackCall:
    def __init__(self, k, max_len, F_max, stride, reports, n_reports=None, N_max=None, nulls=()):
        self.k, self.max_len, self.F_max, self.stride = k, max_len, F_max, stride
        self.reports = np.asarray(reports, REPORT)
        self.N_max = len(self.reports) if N_max is None else N_max
        self.n_reports, self.nulls = n_reports, tuple(nulls)
        self.per = capacity(max_len)

    def blank(self) -> dict:
        one = lambda: np.full(1, FILL32, np.uint32)   # noqa: E731
        return dict(pkts=np.full(self.F_max * self.stride, FILL, np.uint8), pkt_len=np.full(self.F_max, FILL32, np.uint32),
                    n_pkts=one(), n_left=one(), n_skipped=one())

    def sent(self):
        """-> N, the sendable records among the first N as [(id, rank)]."""
        N = self.N_max if self.n_reports is None else min(int(self.n_reports), self.N_max)
        return N, [(int(r["id"]), int(r["rank"])) for r in self.reports[:N] if sendable(r, self.k)]

    def model(self, before: dict | None = None) -> dict:
        before = before or self.blank()
        o = {key: v.copy() for key, v in before.items()}
        N, ent = self.sent()
        S, per = len(ent), self.per
        P = min(-(-S // per), self.F_max)
        for p in range(P):
            raw = packet(ent[p * per: (p + 1) * per])
            o["pkts"][p * self.stride: p * self.stride + len(raw)] = np.frombuffer(raw, np.uint8)
            o["pkt_len"][p] = len(raw)
        o["n_pkts"][0] = P
        o["n_left"][0] = S - min(S, self.F_max * per)
        o["n_skipped"][0] = N - S
        return _keep(o, before, self.nulls)


def _mixed(n: int, k: int, seed: int, hole_every: int = 0):
    """n records with distinct ids above 2^40 and ranks 0..k; every hole_every-th one is a hole."""
    rng = np.random.default_rng(seed)
    rows = [((1 << 40) + 977 * i + int(rng.integers(0, 900)), int(rng.integers(0, k + 1)), 0) for i in range(n)]
    if hole_every:
        for i in range(hole_every - 1, n, hole_every):
            rows[i] = (U64MAX, 0, 0)
    return records(rows)


def pack_cases() -> dict:
    """name -> call (each starts from blank())."""
    c = {}
    k = 4
    good = _mixed(12, k, 1)
    c["n_reports_0"] = PackCall(k, 33, 4, 48, good, n_reports=0)
    c["all_holes"] = PackCall(k, 33, 4, 48, records([(U64MAX, 0, 0)] * 5), n_reports=5)
    bad = good[:7].copy()
    bad[1], bad[3], bad[5] = (ID_LIMIT, 1, 0), (7, k + 1, 0), (9, 1, 1)
    c["non_sendable_between"] = PackCall(k, 33, 4, 48, bad, n_reports=7)
    per, F = 3, 2
    for name, S in (("S_per", per), ("S_per_plus_1", per + 1), ("S_full", F * per), ("S_full_plus_1", F * per + 1)):
        c[name] = PackCall(k, 33, F, 48, good[:S], n_reports=S)
    for N in (257, 513):                       # the prefix across blocks, with scattered holes
        c[f"N{N}"] = PackCall(k, 53, 128, 64, _mixed(N, k, N, hole_every=7 if N == 257 else 3), n_reports=N)
    c["n_reports_null"] = PackCall(k, 33, 4, 48, good[:9])
    c["n_reports_above_N_max"] = PackCall(k, 33, 4, 48, good[:9], n_reports=1000)
    c["no_n_left"] = PackCall(k, 33, 2, 48, good[:9], n_reports=9, nulls=("n_left",))
    c["no_n_skipped"] = PackCall(k, 33, 4, 48, bad, n_reports=7, nulls=("n_skipped",))
    for max_len, stride in ((13, 16), (22, 32), (23, 32), (1200, 1200)):
        per = capacity(max_len)
        c[f"max_len{max_len}"] = PackCall(k, max_len, 3, stride, _mixed(2 * per + 1, k, max_len), n_reports=2 * per + 1)
    c["max_len65535"] = PackCall(k, 65535, 2, 65536, _mixed(6554, k, 65535), n_reports=6554)
    c["stride_above_max_len"] = PackCall(k, 33, 3, 80, good[:8], n_reports=8)
    c["k256_rank256"] = PackCall(256, 33, 2, 48, records([(5, 256, 0), (6, 255, 0), (7, 257, 0), (8, 1, 0)]))
    c["id_bytes_differ"] = PackCall(k, 33, 1, 48, records([(0x0123456789ABCDEF, 3, 0), (ID_LIMIT - 1, 4, 0)]))
    return c


# ---------------------------------------------------------------------------
# qf_parse_report_frames_dev
# ---------------------------------------------------------------------------
class ParseCall:
    def __init__(self, k, max_len, F_max, stride, pkts, pkt_len, N_max, n_pkts=None, append=False, nulls=()):
        self.k, self.max_len, self.F_max, self.stride, self.N_max = k, max_len, F_max, stride, N_max
        self.pkts = np.asarray(pkts, np.uint8).reshape(-1)
        self.pkt_len = np.asarray(pkt_len, np.uint32)
        assert len(self.pkts) == F_max * stride and len(self.pkt_len) == F_max
        self.n_pkts, self.append, self.nulls = n_pkts, append, tuple(nulls)

    def blank(self, n_reports: int = FILL32) -> dict:
        return dict(reports=poisoned(self.N_max, REPORT), n_reports=np.array([n_reports], np.uint32),
                    n_left=np.full(1, FILL32, np.uint32), pkt_status=np.full(self.F_max, FILL32, np.uint32).view(np.int32),
                    pkt_first=np.full(self.F_max, FILL32, np.uint32), pkt_count=np.full(self.F_max, FILL32, np.uint32))

    def entries(self, f: int):
        """The entries of packet f as [(id, rank)], None for one that is not QF_OK."""
        ln = int(self.pkt_len[f])
        if ln < 3 or ln > min(self.max_len, self.stride):
            return None
        raw = self.pkts[f * self.stride: f * self.stride + ln].tobytes()
        c = int.from_bytes(raw[1:3], "big")
        if raw[0] != KIND or c < 1 or ln != 3 + ENTRY * c:
            return None
        return [(int.from_bytes(raw[3 + ENTRY * e: 11 + ENTRY * e], "big"),
                 int.from_bytes(raw[11 + ENTRY * e: 13 + ENTRY * e], "big")) for e in range(c)]

    def model(self, before: dict | None = None) -> dict:
        before = before or self.blank()
        o = {key: v.copy() for key, v in before.items()}
        F = self.F_max if self.n_pkts is None else min(int(self.n_pkts), self.F_max)
        base = min(int(o["n_reports"][0]), self.N_max) if self.append else 0
        at = base
        for f in range(F):
            ent = self.entries(f)
            if ent is None:
                o["pkt_status"][f], o["pkt_first"][f], o["pkt_count"][f] = EINVAL, NONE32, 0
                continue
            o["pkt_status"][f], o["pkt_first"][f], o["pkt_count"][f] = OK, min(at, NONE32 - 1), len(ent)
            for e, (x, r) in enumerate(ent):
                if at + e < self.N_max:
                    o["reports"][at + e] = (x, r, 0)
            at += len(ent)
        o["n_reports"][0] = min(at, self.N_max)
        o["n_left"][0] = min(at - min(at, self.N_max), NONE32)
        return _keep(o, before, self.nulls)


def slots(F_max: int, stride: int, raws, lens=None):
    """Packets (bytes) into poisoned slots -> pkts, pkt_len; lens overrides the lengths."""
    pkts = np.full(F_max * stride, FILL, np.uint8)
    pkt_len = np.full(F_max, FILL32, np.uint32)
    for f, raw in enumerate(raws):
        n = min(len(raw), stride)
        pkts[f * stride: f * stride + n] = np.frombuffer(raw[:n], np.uint8)
        pkt_len[f] = len(raw)
    if lens is not None:
        pkt_len[: len(lens)] = lens
    return pkts, pkt_len


def _entries(n: int, seed: int, k: int = 4):
    return [(int(r["id"]), int(r["rank"])) for r in _mixed(n, k, seed)]


def parse_cases() -> dict:
    """name -> (call, the buffers it starts from)."""
    c = {}
    k = 4

    def add(name, call, n_reports=FILL32):
        c[name] = (call, call.blank(n_reports))

    two, three = packet(_entries(2, 11)), packet(_entries(3, 12))
    add("F_0", ParseCall(k, 33, 3, 48, *slots(3, 48, [two, three]), 16, n_pkts=0))
    # the lengths: 0 (a dropped packet), 2, 3 (c = 2 in the header), 12, 14, and 3 + 10 c - 1, + 1
    raws = [two, two, two, two, two, two, two, three, three, two]
    lens = [0, 2, 3, 12, 14, 22, 24, 32, 34, 23]
    add("lengths", ParseCall(k, 53, 10, 64, *slots(10, 64, raws, lens), 16, n_pkts=10))
    zero = bytes([KIND, 0, 0])
    add("c_0_len_3", ParseCall(k, 33, 2, 48, *slots(2, 48, [zero, two]), 16, n_pkts=2))
    # a count that disagrees with the length: c = 3 in 23 bytes, c = 1 in 23 bytes, c = 0x0102 (the high byte is read)
    wrong = [bytes([KIND, 0, 3]) + two[3:], bytes([KIND, 0, 1]) + two[3:], bytes([KIND, 1, 2]) + two[3:], two]
    add("c_disagrees", ParseCall(k, 33, 4, 48, *slots(4, 48, wrong), 16, n_pkts=4))
    add("byte_0", ParseCall(k, 33, 3, 48, *slots(3, 48, [bytes([0]) + two[1:], bytes([1]) + two[1:], two]), 16, n_pkts=3))
    add("len_above_max_len", ParseCall(k, 23, 2, 48, *slots(2, 48, [three, two]), 16, n_pkts=2))
    # a length beyond its slot (stride >= max_len, so beyond max_len too): nothing of the next slot is read
    five = packet(_entries(5, 13))
    add("len_above_stride", ParseCall(k, 48, 2, 48, *slots(2, 48, [five, two]), 16, n_pkts=2))
    # 257 one-entry packets, every fifth bad in turn: empty, wrong kind, c = 2
    raws, ent = [], _entries(257, 14)
    for f in range(257):
        raw = packet(ent[f: f + 1])
        if f % 5 == 2:
            raw = (b"", bytes([1]) + raw[1:], bytes([KIND, 0, 2]) + raw[3:])[(f // 5) % 3]
        raws.append(raw)
    add("F257", ParseCall(k, 13, 257, 16, *slots(257, 16, raws), 300, n_pkts=257))
    add("one_packet_6553", ParseCall(k, 65535, 1, 65536, *slots(1, 65536, [packet(_entries(6553, 15))]), 6553, n_pkts=1))
    pk = [packet(_entries(3, 16)), packet(_entries(2, 17)), packet(_entries(3, 18))]
    add("append_base0", ParseCall(k, 33, 3, 48, *slots(3, 48, pk), 12, n_pkts=3, append=True), 0)
    add("append_crosses_N_max", ParseCall(k, 33, 3, 48, *slots(3, 48, pk), 12, n_pkts=3, append=True), 8)   # 8 + 3 + (1 of 2)
    add("append_base_at_N_max", ParseCall(k, 33, 3, 48, *slots(3, 48, pk), 12, n_pkts=3, append=True), 12)
    add("append_base_above_N_max", ParseCall(k, 33, 3, 48, *slots(3, 48, pk), 12, n_pkts=3, append=True), 1000)
    add("stale_length_without_append", ParseCall(k, 33, 3, 48, *slots(3, 48, pk), 12, n_pkts=3), 5)
    add("overflow", ParseCall(k, 33, 3, 48, *slots(3, 48, pk), 5, n_pkts=3))
    add("n_pkts_null", ParseCall(k, 33, 3, 48, *slots(3, 48, pk), 12))
    add("n_pkts_above_F_max", ParseCall(k, 33, 3, 48, *slots(3, 48, pk), 12, n_pkts=1000))
    for key in ("pkt_status", "pkt_first", "pkt_count", "n_left"):
        add(f"no_{key}", ParseCall(k, 33, 3, 48, *slots(3, 48, [pk[0], b"", pk[2]]), 12, n_pkts=3, nulls=(key,)))
    # values are not judged: an id >= 2^62, UINT64_MAX and a rank > k go through
    odd = [packet([(ID_LIMIT, 2), (U64MAX, 0), (77, k + 1)]), packet([(78, 0xFFFF), (0x0123456789ABCDEF, 1)])]
    add("values_pass", ParseCall(k, 33, 2, 48, *slots(2, 48, odd), 8, n_pkts=2))
    return c


# ---------------------------------------------------------------------------
# qf_report_closed_dev
# ---------------------------------------------------------------------------
class ClosedCall:
    def __init__(self, k, win, frame_id, frame_status, N_max, n_frames=None, append=False, nulls=()):
        self.k, self.N_max, self.n_frames, self.append, self.nulls = k, N_max, n_frames, append, tuple(nulls)
        self.win = np.asarray(win, np.uint64)
        self.frame_id = np.asarray(frame_id, np.uint64)
        self.frame_status = np.asarray(frame_status, np.int32)
        self.G_src, self.F_max = len(self.win), len(self.frame_id)
        assert len(self.frame_status) == self.F_max

    def blank(self, n_reports: int = FILL32) -> dict:
        return dict(reports=poisoned(self.N_max, REPORT), n_reports=np.array([n_reports], np.uint32),
                    n_left=np.full(1, FILL32, np.uint32))

    def flags(self) -> np.ndarray:
        """What k_closed_mark leaves in its zeroed workspace: 1 for a marked slot."""
        M = self.F_max if self.n_frames is None else min(int(self.n_frames), self.F_max)
        out = np.zeros(self.G_src, np.uint32)
        for f in range(M):
            x = int(self.frame_id[f])
            if int(self.frame_status[f]) != ECLOSED or x >= ID_LIMIT:
                continue
            s = x % self.G_src
            if int(self.win[s]) == (x + 1) | CLOSED:
                out[s] = 1
        return out

    def model(self, before: dict | None = None) -> dict:
        before = before or self.blank()
        o = {key: v.copy() for key, v in before.items()}
        marked = np.flatnonzero(self.flags())
        base = min(int(o["n_reports"][0]), self.N_max) if self.append else 0
        for j, s in enumerate(marked):
            if base + j < self.N_max:
                o["reports"][base + j] = (C.held(self.win[s]) - 1, self.k, 0)
        end = base + len(marked)
        o["n_reports"][0] = min(end, self.N_max)
        o["n_left"][0] = end - min(end, self.N_max)
        return _keep(o, before, self.nulls)


def closed_cases() -> dict:
    """name -> (call, the buffers it starts from)."""
    c = {}
    k, G = 4, 5
    base = ((1 << 40) // G + 1) * G

    def add(name, call, n_reports=FILL32):
        c[name] = (call, call.blank(n_reports))

    closed = np.array([(base + s + 1) | CLOSED for s in range(G)], np.uint64)
    add("no_eclosed", ClosedCall(k, closed, [base, base + 1, base + 2], [OK, -8, EINVAL], 8, n_frames=3))
    add("five_frames_one_generation", ClosedCall(k, closed, [base + 2] * 5 + [base + 9], [ECLOSED] * 5 + [OK], 8, n_frames=6))
    # statuses the window contradicts: an open entry, another id in the slot (older and newer), an empty slot
    win = closed.copy()
    win[0], win[3] = base + 1, 0
    add("window_contradicts", ClosedCall(k, win, [base, base + G + 1, base - G + 2, base + 3, base + 4], [ECLOSED] * 5, 8,
                                         n_frames=5))
    add("eclosed_on_id_2_62", ClosedCall(k, closed, [ID_LIMIT, U64MAX, base + 1], [ECLOSED] * 3, 8, n_frames=3))
    for G2 in (3, 7):
        w = np.zeros(G2, np.uint64)
        w[(ID_LIMIT - 1) % G2] = ID_LIMIT | CLOSED
        add(f"last_id_G{G2}", ClosedCall(k, w, [ID_LIMIT - 1, ID_LIMIT - 1 - G2], [ECLOSED] * 2, 4, n_frames=2))
    add("G_src_1", ClosedCall(256, [(base + 1) | CLOSED], [base, base + 1, base], [ECLOSED, ECLOSED, OK], 4, n_frames=3))
    # ascending slot order from shuffled frames, over several blocks of frames
    G3 = 130
    b3 = ((1 << 40) // G3 + 1) * G3
    rng = np.random.default_rng(31)
    w = np.array([(b3 + s + 1) | (CLOSED if s % 3 else 0) for s in range(G3)], np.uint64)
    fid = b3 + rng.permutation(np.repeat(np.arange(G3), 5))[:600].astype(np.uint64)
    fst = np.where(rng.random(600) < 0.4, ECLOSED, OK).astype(np.int32)
    add("shuffled", ClosedCall(64, w, fid, fst, 140, n_frames=600))
    add("append_mid", ClosedCall(k, closed, [base + 4, base + 1], [ECLOSED] * 2, 8, n_frames=2, append=True), 3)
    add("append_overflow", ClosedCall(k, closed, [base + 4, base + 1, base + 3], [ECLOSED] * 3, 8, n_frames=3, append=True), 6)
    add("append_base_above", ClosedCall(k, closed, [base + 4], [ECLOSED], 8, n_frames=1, append=True), 1000)
    add("stale_length_without_append", ClosedCall(k, closed, [base + 4], [ECLOSED], 8, n_frames=1), 5)
    add("n_frames_null", ClosedCall(k, closed, [base + 4, base, base + 2], [ECLOSED, OK, ECLOSED], 8))
    add("n_frames_above_F_max", ClosedCall(k, closed, [base + 4, base], [ECLOSED] * 2, 8, n_frames=1000))
    add("n_frames_mid", ClosedCall(k, closed, [base + 4, base, base + 2], [ECLOSED] * 3, 8, n_frames=2))
    add("no_n_left", ClosedCall(k, closed, [base + 4, base], [ECLOSED] * 2, 1, n_frames=2, nulls=("n_left",)))
    return c


# ---------------------------------------------------------------------------
# the loop: credit_ref.lossy_loop with the back channel as bytes
# ---------------------------------------------------------------------------
MAX_LEN_LOOP, STRIDE_LOOP = 33, 48                 # per = 3: a poll's reports span several packets
PER_LOOP = capacity(MAX_LEN_LOOP)
N_REPORTS = 3 * E.G_LOOP                           # the completed list, the list of open generations, the re-reports
F_LOOP = -(-N_REPORTS // PER_LOOP)                 # ... all fit: n_left is 0 throughout
MAX_POLLS = len(E.SCHED) + 24
# The chosen run (tests/test_fbwire_cpu.py asserts what it was chosen for): the redundancy ratio, the
# polls a feedback packet takes back, and the back channel's drop mask.
NUM_LOOP, DEN_LOOP, DELAY_LOOP = 3, 2, 1
MASK_LOOP = (1, 1, 3, 1)


def dropped_fb(mask, p: int, j: int) -> bool:
    """The drop mask of the back channel: packet j of the receiver's poll p.  mask None: nothing is dropped."""
    if mask is None:
        return False
    a, b, m, c = mask
    return (a * p + b * j) % m == c


def fb_loop(oracle, num: int, den: int, delay: int, mask, rereport: bool, seed: int = E.SEED_LOOP):
    """-> spec, the per-poll records, the statistics the tests assert on."""
    from tests import partial_ref as P
    from tests import window_ref as WR

    spec = E.LoopSpec()
    k, G, M = E.K_LOOP, E.G_LOOP, E.M_RELAY
    relay, rx = E.Node(), E.Node()
    state, credit = np.zeros(G, C.STATE), np.full(G, FILL32, np.uint32)
    nothing = dict(pkts=np.full(F_LOOP * STRIDE_LOOP, FILL, np.uint8), pkt_len=np.full(F_LOOP, FILL32, np.uint32),
                   n_pkts=np.zeros(1, np.uint32))
    line = [nothing] * delay                       # the feedback packets under way, oldest first
    polls, emitted, delivered, peer = [], {}, {}, {}
    lost_close, eclosed_after, rereported = set(), set(), set()
    max_sent = max_left = 0
    for p in range(MAX_POLLS):
        gens = E.SCHED[p] if p < len(E.SCHED) else []
        rec = dict(gens=gens)
        a, b = spec.source_calls(gens)
        q1 = b.model(a.model())
        q1["frame_len"][spec.drop_list(gens)] = 0
        rec["q1"] = q1
        relay.ingest(q1, E.N_SRC)
        # the relay: the feedback packets that arrive now to records, records and ranks to credit
        arrived = line.pop(0)
        pc = ParseCall(k, MAX_LEN_LOOP, F_LOOP, STRIDE_LOOP, arrived["pkts"], arrived["pkt_len"], N_REPORTS,
                       n_pkts=int(arrived["n_pkts"][0]))
        po = pc.model()
        max_left = max(max_left, int(po["n_left"][0]))
        rank = relay.rank()
        cc = C.CreditCall(k, num, den, C.CAP_LOOP, relay.win, rank, relay.sent.copy(), po["reports"],
                          int(po["n_reports"][0]), N_REPORTS)
        co = cc.model(cc.blank(state, credit))
        state, credit = co["state"], co["credit"]
        for s in range(G):
            if int(state[s]["owner"]):
                peer[int(state[s]["owner"]) - 1 - E.BASE_LOOP] = int(state[s]["peer"])
        listed = [s for s in range(G) if credit[s] >= 1 and credit[s] > relay.sent[s]]
        sel = np.full(G, FILL32, np.uint32)
        sel[: len(listed)] = listed
        mix = oracle.fill_splitmix(G * M * k, C.poll_seed(p, seed)).reshape(G, M, k)
        rows = np.full((G, M, spec.rs), E.FILL, np.uint8)
        vec = np.zeros((G, M, k), np.uint8)
        rl = np.zeros((G, M), np.uint32)
        st = np.full(G, ENOTREADY, np.int32)
        for j, s in enumerate(listed):
            n = len(relay.vec[s])
            vec[j] = P.encode_rows(mix[j, :, :n], np.stack(relay.vec[s]))
            rows[j, :, :E.L_LOOP] = P.encode_rows(mix[j, :, :n], np.stack(relay.pay[s]))
            rl[j], st[j] = E.L_LOOP, OK
        _, ids = WR.window_sel(relay.win, sel, len(listed), G, G, False)
        c = spec.relay_call(sel, len(listed), rows.reshape(-1), vec, rl, st, ids, credit.copy(), relay.sent.copy())
        q2 = c.model()
        relay.sent = q2["sent"].copy()
        max_sent = max(max_sent, int(relay.sent.max()))
        drops = []
        for f in range(int(q2["n_frames"][0])):
            g = int(q2["frame_id"][f]) - E.BASE_LOOP
            if C.dropped2(g, emitted.get(g, 0)):
                drops.append(f)
            emitted[g] = emitted.get(g, 0) + 1
        wire = {key: v.copy() for key, v in q2.items()}
        wire["frame_len"][drops] = 0
        rec.update(parse_call=pc, parse_out=po, credit_call=cc, credit_out=co, call=c, q2=q2, drops=drops)
        # the receiver: ingest, the complete generations leave and close, the two report lists, the
        # re-report of the closed generations that frames of this poll belong to, the pack
        w = rx.ingest(wire, E.N_RELAY)
        done = [s for s in range(G) if len(rx.vec[s]) == k]
        for s in done:
            g = WR.held(rx.win[s]) - E.BASE_LOOP
            assert g not in delivered
            got = np.stack(rx.pay[s])
            assert np.array_equal(got, P.encode_rows(np.stack(rx.vec[s]), spec.src[g])), "a row is not its vector x the sources"
            delivered[g] = p
            rx.reset(s)
        rx.win, _ = WR.window_sel(rx.win, done, len(done), G, G, True)
        ra, oa, rb, ob = C.receiver_reports(rx.win, rx.rank(), done)
        ra.N_max = rb.N_max = N_REPORTS
        oa = ra.model(ra.blank())
        ob = rb.model(oa)
        n_frames = int(wire["n_frames"][0])
        for f in range(n_frames):
            if int(w.frame_status[f]) == ECLOSED:
                eclosed_after.add(int(wire["frame_id"][f]) - E.BASE_LOOP)
        out, rc = ob, None
        if rereport:
            rc = ClosedCall(k, rx.win, wire["frame_id"], w.frame_status, N_REPORTS, n_frames=n_frames, append=True)
            out = rc.model(ob)
            rereported |= {int(x) - E.BASE_LOOP for x in out["reports"]["id"][int(ob["n_reports"][0]): int(out["n_reports"][0])]}
        max_left = max(max_left, int(oa["n_left"][0]), int(ob["n_left"][0]), int(out["n_left"][0]))
        fc = PackCall(k, MAX_LEN_LOOP, F_LOOP, STRIDE_LOOP, out["reports"], int(out["n_reports"][0]), N_REPORTS)
        fo = fc.model()
        max_left = max(max_left, int(fo["n_left"][0]))
        # the back channel: a dropped packet arrives with length 0
        n_pkts = int(fo["n_pkts"][0])
        fb_drops = [j for j in range(n_pkts) if dropped_fb(mask, p, j)]
        closing = {int(WR.held(rx.win[s])) for s in done}
        probe = ParseCall(k, MAX_LEN_LOOP, F_LOOP, STRIDE_LOOP, fo["pkts"], fo["pkt_len"], N_REPORTS, n_pkts=n_pkts)
        for j in fb_drops:
            lost_close |= {x - E.BASE_LOOP for x, r in probe.entries(j) if r == k and x in closing}
        back = dict(pkts=fo["pkts"].copy(), pkt_len=fo["pkt_len"].copy(), n_pkts=fo["n_pkts"].copy())
        back["pkt_len"][fb_drops] = 0
        line.append(back)
        rec.update(done=done, report_calls=(ra, rb), report_out=(oa, ob), closed_call=rc, closed_out=out, pack_call=fc,
                   pack_out=fo, fb_drops=fb_drops, frame_status=w.frame_status.copy())
        polls.append(rec)
        if p >= len(E.SCHED) - 1 and not listed and not any(int(x["n_pkts"][0]) for x in line):
            break
    else:
        raise AssertionError("the loop does not come to rest")
    return spec, polls, dict(emitted=emitted, delivered=delivered, max_sent=max_sent, frames=sum(emitted.values()),
                             peer=peer, lost_close=lost_close, eclosed_after=eclosed_after, rereported=rereported,
                             max_left=max_left)


@functools.lru_cache(maxsize=None)
def loop_cached(num, den, delay, mask, rereport):
    from tests import oracle_py

    return fb_loop(oracle_py, num, den, delay, mask, rereport)
