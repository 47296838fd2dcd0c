"""Python mirror of QuicFuscate's `quicfuscate::fec` API on the MI355X library.

Names, argument meaning and error behaviour follow the reference
(src/fec/{gf_tables,decoder,encoder}.rs) so that the parity tests read like
the reference's own tests (tests/fec.rs, src/fec/mod.rs).  Every payload
operation runs on the GPU through libqf_fec.so; there is no CPU fallback.

Reference panics become exceptions: gf_inv(0) and Cauchy rows with
k + r > 256 raise QfError(QF_ERANGE).
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional

from . import _lib as L
from ._lib import QfError, check

# Objects still alive when the interpreter exits are not freed through the
# library: the process is ending, and the HIP runtime may already be torn
# down by then (a late hipFree / hipEventSynchronize can crash the exit).
_SHUTDOWN = False


def _mark_shutdown() -> None:
    global _SHUTDOWN
    _SHUTDOWN = True


import atexit as _atexit  # noqa: E402

_atexit.register(_mark_shutdown)

__all__ = [
    "QfError", "Context", "default_context", "init_gf_tables", "gf_mul", "gf_mul_table",
    "gf_mul_add", "gf_inv", "gf_mul_slice", "cauchy_coefficients", "MemoryPool", "Packet",
    "Encoder", "Decoder", "encode_batch", "decode_batch", "recode_batch", "Recoder",
    "frame_payload_offset", "frame_rows", "parse_frames_coded", "parse_frame_headers", "recode_frames",
    "gf16_mul", "gf16_inv", "cauchy16_coefficients", "encode16_batch", "decode16_batch", "Encoder16", "Decoder16",
]


# ---------------------------------------------------------------------------
# GF(2^8) helpers (gf_tables.rs)
# ---------------------------------------------------------------------------
def init_gf_tables() -> None:
    """gf_tables.rs:392 init_gf_tables (idempotent)."""
    check(L._lib().qf_gf256_init())


def gf_mul(a: int, b: int) -> int:
    """gf_tables.rs:283 gf_mul; identical to gf_mul_table for every pair."""
    return int(L._lib().qf_gf256_mul(a & 0xFF, b & 0xFF))


gf_mul_table = gf_mul  # gf_tables.rs:47 (the semantic contract)


def gf_mul_add(a: int, b: int, c: int) -> int:
    """gf_tables.rs:327 gf_mul_add = gf_mul(a, b) ^ c."""
    return int(L._lib().qf_gf256_mul_add(a & 0xFF, b & 0xFF, c & 0xFF))


def gf_inv(a: int) -> int:
    """gf_tables.rs:304 gf_inv; the reference panics for 0, this raises."""
    out = ctypes.c_uint8(0)
    check(L._lib().qf_gf256_inv(a & 0xFF, ctypes.byref(out)), "gf_inv")
    return int(out.value)


def cauchy_coefficients(k: int, r: int) -> bytes:
    """decoder.rs:280-298 for repairs 0..r-1, row-major r x k."""
    buf = (ctypes.c_uint8 * max(1, k * r))()
    check(L._lib().qf_cauchy_coeffs(k, r, buf), "cauchy")
    return bytes(buf)[: k * r]


def gf_rank(vectors, k: int) -> tuple[int, list[int]]:
    """qf_gf256_rank (host, no device): `vectors` holds n vectors of k bytes
    in arrival order (bytes-like, or anything bytes() accepts row by row, such
    as an n x k uint8 array).  Returns (rank, flags): flags[s] = 1 iff vector
    s is not in the GF(2^8) span of the vectors before it."""
    raw = vectors.tobytes() if hasattr(vectors, "tobytes") else bytes(vectors)
    if k <= 0 or len(raw) % k:
        raise ValueError(f"gf_rank: {len(raw)} bytes are no whole number of vectors of k = {k} bytes")
    n = len(raw) // k
    buf = (ctypes.c_uint8 * max(1, len(raw))).from_buffer_copy(raw.ljust(max(1, len(raw)), b"\0"))
    flags = (ctypes.c_uint8 * max(1, n))()
    rank = ctypes.c_uint32(0)
    check(L._lib().qf_gf256_rank(k, n, buf, flags, ctypes.byref(rank)), "gf_rank")
    return int(rank.value), list(flags)[:n]


# ---------------------------------------------------------------------------
# Device context
# ---------------------------------------------------------------------------
QF_STREAM_NULL = 1   # qf_fec.h: the device's null stream


class Context:
    """A qf_ctx bound to a device and a HIP stream (default: torch's current)."""

    def __init__(self, device: Optional[int] = None, stream: Optional[int] = None):
        import torch

        if not torch.cuda.is_available():
            raise QfError(L.QF_EDEVICE, "no HIP device visible")
        self.device = torch.cuda.current_device() if device is None else int(device)
        if stream is None:
            stream = torch.cuda.current_stream(self.device).cuda_stream
        if not stream:
            # torch's default stream is the null stream: QF_STREAM_NULL binds
            # the library to it, so its work is ordered with torch's (a NULL
            # stream makes qf_ctx_create allocate its own non-blocking stream,
            # which a torch fill / randint on the default stream does not wait for)
            stream = QF_STREAM_NULL
        h = ctypes.c_void_p()
        check(L._lib().qf_ctx_create(self.device, ctypes.c_void_p(stream), ctypes.byref(h)), "ctx")
        self.handle = h

    def set_stream(self, stream: int) -> None:
        check(L._lib().qf_ctx_set_stream(self.handle, ctypes.c_void_p(stream)))

    def set_option(self, name: str, value: int) -> None:
        """qf_ctx_set_option: a kernel-path option of this context
        (L.OPTIONS: "fft_kernels", "decode_path", ...; include/qf_fec.h)."""
        check(L._lib().qf_ctx_set_option(self.handle, L.OPTIONS[name], int(value)), f"option {name}")

    def option(self, name: str) -> int:
        v = ctypes.c_int64()
        check(L._lib().qf_ctx_get_option(self.handle, L.OPTIONS[name], ctypes.byref(v)), f"option {name}")
        return v.value

    def options(self) -> dict:
        return {n: self.option(n) for n in L.OPTIONS}

    def set_payload_wait(self, event) -> None:
        """qf_ctx_set_payload_wait: the next decode_batch runs its acceptance
        pass at once and its payload pass after `event` (a torch.cuda.Event
        that has been recorded, or a raw hipEvent_t handle; None clears)."""
        h = event if (event is None or isinstance(event, int)) else event.cuda_event
        check(L._lib().qf_ctx_set_payload_wait(self.handle, ctypes.c_void_p(h)), "payload_wait")

    def set_payload_stream(self, stream) -> None:
        """qf_ctx_set_payload_stream: the next decode_batch keeps its
        acceptance pass on this context's stream and runs its payload pass on
        `stream` (a torch.cuda.Stream or a raw hipStream_t; torch's default
        stream maps to the null stream; None clears)."""
        if stream is None:
            h = None
        else:
            h = stream if isinstance(stream, int) else stream.cuda_stream
            h = h or QF_STREAM_NULL
        check(L._lib().qf_ctx_set_payload_stream(self.handle, ctypes.c_void_p(h)), "payload_stream")

    def sync(self) -> None:
        check(L._lib().qf_sync(self.handle), "sync")

    def profile(self, on: bool) -> None:
        """Start (clearing totals) or stop per-kernel event timing."""
        check(L._lib().qf_ctx_profile(self.handle, 1 if on else 0), "profile")

    def kernel_times(self) -> dict:
        """{kernel name: (launches, total ms)} accumulated while profiling."""
        out = {}
        i = 0
        lib = L._lib()
        while True:
            name, n, ms = ctypes.c_char_p(), ctypes.c_uint32(), ctypes.c_double()
            s = lib.qf_ctx_profile_read(self.handle, i, ctypes.byref(name), ctypes.byref(n), ctypes.byref(ms))
            if s == L.QF_EINVAL:
                return out
            check(s, "profile_read")
            out[name.value.decode()] = (n.value, ms.value)
            i += 1

    def close(self) -> None:
        if getattr(self, "handle", None):
            L._lib().qf_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):  # pragma: no cover - best effort
        if _SHUTDOWN:
            return
        try:
            self.close()
        except Exception:
            pass


_DEFAULT: Optional[Context] = None


_DEFAULT_OPTS: dict = {}


def default_context() -> Context:
    global _DEFAULT, _DEFAULT_OPTS
    if _DEFAULT is None:
        _DEFAULT = Context()
        _DEFAULT_OPTS = _DEFAULT.options()
    return _DEFAULT


def set_default_options(**opts) -> None:
    """Kernel-path options (QF_OPT_*) on the default context, e.g.
    set_default_options(encode_small=0, decode_path=1)."""
    ctx = default_context()
    for n, v in opts.items():
        ctx.set_option(n, v)


def reset_default_options() -> None:
    """The default context's options back to those it was created with."""
    if _DEFAULT is not None and _DEFAULT.handle:
        for n, v in _DEFAULT_OPTS.items():
            _DEFAULT.set_option(n, v)


def _ptr(t) -> int:
    return int(t.data_ptr())


def _need(t, nbytes: int, what: str) -> None:
    """A buffer the library will read or write must hold nbytes (the C ABI
    takes bare pointers: an undersized tensor would be overrun on the device)."""
    if t is None or nbytes <= 0 or not hasattr(t, "numel"):
        return
    have = int(t.numel()) * int(t.element_size())
    if have < nbytes:
        raise ValueError(f"{what}: {have} bytes, the call needs {nbytes}")


def _opt(t) -> Optional[int]:
    """The device pointer of an optional tensor (None: NULL)."""
    return _ptr(t) if t is not None else None


def _need_rows(G: int, max_rows: int, k: int, row_off, row_len, row_index, row_coeffs, n_rows) -> None:
    """_need for the arrays that describe the max_rows slots of each of G
    generations (each where it is given)."""
    _need(row_off, 4 * G * max_rows, "row_off")
    _need(row_len, 4 * G * max_rows, "row_len")
    _need(row_index, 2 * G * max_rows, "row_index")
    _need(row_coeffs, G * max_rows * k, "row_coeffs")
    _need(n_rows, 4 * G, "n_rows")


def _span(G: int, gen_stride: int, rows: int, row_stride: int, L: int) -> int:
    """Bytes from the first byte of generation 0 to the end of the last row."""
    return 0 if G == 0 or rows == 0 else (G - 1) * gen_stride + (rows - 1) * row_stride + L


def gf_mul_slice(a: bytes, b: bytes, ctx: Optional[Context] = None) -> bytes:
    """gf_tables.rs:255 gf_mul_slice: element-wise a[i]*b[i], on the device."""
    import torch

    if len(a) != len(b):
        raise ValueError("gf_mul_slice: length mismatch (reference asserts)")
    ctx = ctx or default_context()
    n = len(a)
    if n == 0:
        return b""
    da = torch.frombuffer(bytearray(a), dtype=torch.uint8).to(f"cuda:{ctx.device}")
    db = torch.frombuffer(bytearray(b), dtype=torch.uint8).to(f"cuda:{ctx.device}")
    out = torch.empty_like(da)
    torch.cuda.current_stream(ctx.device).synchronize()
    check(L._lib().qf_gf256_mul_slice_dev(ctx.handle, _ptr(da), _ptr(db), _ptr(out), n), "mul_slice")
    ctx.sync()
    return bytes(out.cpu().numpy().tobytes())


# ---------------------------------------------------------------------------
# Batched device API (torch uint8 tensors on the context's device)
# ---------------------------------------------------------------------------
def encode_batch(src, rep, k: int, r: int, Lb: int, *, src_row_stride: int, src_gen_stride: int,
                 rep_row_stride: int, rep_gen_stride: int, G: int,
                 coeff: Optional[bytes] = None, ctx: Optional[Context] = None,
                 zero_tail: bool = False) -> None:
    """qf_encode_batch: repairs of G generations (decoder.rs:172-275).
    zero_tail: QF_ENCODE_ZERO_TAIL (the library may zero [L, round_up(L, 128))
    of each repair row)."""
    _need(src, _span(G, src_gen_stride, k, src_row_stride, Lb), "src")
    _need(rep, _span(G, rep_gen_stride, r, rep_row_stride, Lb), "rep")
    ctx = ctx or default_context()
    sh = L.EncodeShape(k, r, Lb, 1 if zero_tail else 0, src_row_stride, src_gen_stride, rep_row_stride,
                       rep_gen_stride)
    cbuf = None
    if coeff is not None:
        if len(coeff) != k * r:
            raise ValueError("coeff must be r*k bytes")
        cbuf = (ctypes.c_uint8 * len(coeff)).from_buffer_copy(coeff)
    check(L._lib().qf_encode_batch(ctx.handle, ctypes.byref(sh), G, _ptr(src), _ptr(rep),
                                    ctypes.cast(cbuf, ctypes.c_void_p) if cbuf is not None else None),
          "encode_batch")


def pack_gen_descs(descs):
    """A ctypes qf_gen_desc array from dicts / tuples: build it once and pass it
    to encode_batch_desc on every call (a per-call rebuild of thousands of
    descriptors costs milliseconds of host time)."""
    arr = (L.GenDesc * max(1, len(descs)))()
    for i, d in enumerate(descs):
        arr[i] = L.GenDesc(**d) if isinstance(d, dict) else L.GenDesc(*d)
    arr.qf_n = len(descs)
    return arr


def pack_dec_descs(descs):
    """A ctypes qf_dec_desc array (see pack_gen_descs)."""
    arr = (L.DecDesc * max(1, len(descs)))()
    for i, d in enumerate(descs):
        arr[i] = L.DecDesc(**d) if isinstance(d, dict) else L.DecDesc(*d)
    arr.qf_n = len(descs)
    return arr


def encode_batch_desc(src, rep, descs, ctx: Optional[Context] = None) -> None:
    """qf_encode_batch_desc: one call over generations of different (k, r, L)
    at arbitrary offsets.  descs: sequence of dicts or tuples
    (k, r, L, flags, src_offset, src_row_stride, rep_offset, rep_row_stride)."""
    ctx = ctx or default_context()
    arr = descs if isinstance(descs, ctypes.Array) else pack_gen_descs(descs)
    check(L._lib().qf_encode_batch_desc(ctx.handle, arr, getattr(arr, "qf_n", len(arr)), _ptr(src), _ptr(rep)), "encode_batch_desc")


def decode_batch_desc(rows, row_index, rec, rec_index, n_rec, status, descs, ctx: Optional[Context] = None) -> None:
    """qf_decode_batch_desc: descs are dicts / tuples of qf_dec_desc (k, r, L,
    n_rows, rows_offset, row_stride, row_index_offset, rec_offset,
    rec_row_stride, rec_index_offset); n_rec / status: one entry per descriptor."""
    ctx = ctx or default_context()
    arr = descs if isinstance(descs, ctypes.Array) else pack_dec_descs(descs)
    check(L._lib().qf_decode_batch_desc(ctx.handle, arr, getattr(arr, "qf_n", len(arr)), _ptr(rows), _ptr(row_index),
                                         _ptr(rec) if rec is not None else None,
                                         _ptr(rec_index) if rec_index is not None else None, _ptr(n_rec),
                                         _ptr(status)), "decode_batch_desc")


def encode_batch_host(src, rep, k: int, r: int, Lb: int, *, src_row_stride: int, rep_row_stride: int, G: int,
                      coeff: Optional[bytes] = None, ctx: Optional[Context] = None) -> None:
    """qf_encode_batch_host: encode_batch with src / rep in host memory (torch
    CPU tensors, pinned recommended; dense generations); synchronous.  The
    send side of core.rs:252-317, starting from UDP datagrams in host memory."""
    ctx = ctx or default_context()
    sh = L.EncodeShape(k, r, Lb, 0, src_row_stride, k * src_row_stride, rep_row_stride, r * rep_row_stride)
    cbuf = None
    if coeff is not None:
        if len(coeff) != k * r:
            raise ValueError("coeff must be r*k bytes")
        cbuf = (ctypes.c_uint8 * len(coeff)).from_buffer_copy(coeff)
    check(L._lib().qf_encode_batch_host(ctx.handle, ctypes.byref(sh), G, _ptr(src), _ptr(rep),
                                         ctypes.cast(cbuf, ctypes.c_void_p) if cbuf is not None else None),
          "encode_batch_host")


def decode_batch_host(rows, row_index, rec, rec_index, n_rec, status, k: int, r: int, Lb: int, *,
                      max_rows: int, row_stride: int, rows_gen_stride: int, rec_row_stride: int,
                      rec_gen_stride: int, G: int, n_rows=None, row_coeffs=None,
                      ctx: Optional[Context] = None) -> None:
    """qf_decode_batch_host: decode_batch with every buffer in host memory
    (torch CPU tensors, pinned recommended); synchronous."""
    ctx = ctx or default_context()
    sh = L.DecodeShape(k, r, Lb, max_rows, row_stride, rows_gen_stride, rec_row_stride, rec_gen_stride)
    check(L._lib().qf_decode_batch_host(
        ctx.handle, ctypes.byref(sh), G, _ptr(rows), _ptr(row_index),
        _ptr(n_rows) if n_rows is not None else None,
        _ptr(row_coeffs) if row_coeffs is not None else None,
        _ptr(rec) if rec is not None else None, _ptr(rec_index) if rec_index is not None else None,
        _ptr(n_rec), _ptr(status)), "decode_batch_host")


def decode_batch(rows, row_index, rec, rec_index, n_rec, status, k: int, r: int, Lb: int, *,
                 max_rows: int, row_stride: int, rows_gen_stride: int, rec_row_stride: int,
                 rec_gen_stride: int, G: int, n_rows=None, row_coeffs=None,
                 ctx: Optional[Context] = None) -> None:
    """qf_decode_batch: recover erased rows of G generations (decoder.rs:658-791)."""
    em = min(k, r)
    _need(rows, _span(G, rows_gen_stride, max_rows, row_stride, Lb), "rows")
    _need(row_index, 2 * G * max_rows, "row_index")
    _need(rec_index, 2 * G * em, "rec_index (min(k, r) entries per generation)")
    _need(n_rec, 4 * G, "n_rec")
    _need(status, 4 * G, "status")
    if n_rows is not None:
        _need(n_rows, 4 * G, "n_rows")
    ctx = ctx or default_context()
    sh = L.DecodeShape(k, r, Lb, max_rows, row_stride, rows_gen_stride, rec_row_stride, rec_gen_stride)
    check(L._lib().qf_decode_batch(
        ctx.handle, ctypes.byref(sh), G, _ptr(rows), _ptr(row_index),
        _ptr(n_rows) if n_rows is not None else None,
        _ptr(row_coeffs) if row_coeffs is not None else None,
        _ptr(rec) if rec is not None else None, _ptr(rec_index) if rec_index is not None else None,
        _ptr(n_rec), _ptr(status)), "decode_batch")


def recode_batch(rows, row_index, out, out_coeffs, status, k: int, m: int, Lb: int, *, r: int = 0,
                 max_rows: int, row_stride: int, rows_gen_stride: int, out_row_stride: int,
                 out_gen_stride: int, G: int, n_rows=None, row_coeffs=None, mix=None, seed: int = 0,
                 ctx: Optional[Context] = None) -> None:
    """qf_recode_batch: m fresh linear combinations of the rows a relay holds
    of each of G generations, with their coefficient vectors over the k
    sources (out_coeffs: [G, m, k] bytes).  Inputs as decode_batch; mix:
    optional [G, m, max_rows] bytes, else the splitmix64 stream of `seed`."""
    _need(rows, _span(G, rows_gen_stride, max_rows, row_stride, Lb), "rows")
    _need(row_index, 2 * G * max_rows, "row_index")
    _need(out, _span(G, out_gen_stride, m, out_row_stride, Lb), "out")
    _need(out_coeffs, G * m * k, "out_coeffs (m vectors of k bytes per generation)")
    _need(status, 4 * G, "status")
    if n_rows is not None:
        _need(n_rows, 4 * G, "n_rows")
    if row_coeffs is not None:
        _need(row_coeffs, G * max_rows * k, "row_coeffs")
    if mix is not None:
        _need(mix, G * m * max_rows, "mix")
    ctx = ctx or default_context()
    sh = L.RecodeShape(k, r, Lb, max_rows, m, 0, row_stride, rows_gen_stride, out_row_stride, out_gen_stride)
    check(L._lib().qf_recode_batch(
        ctx.handle, ctypes.byref(sh), G, _ptr(rows), _ptr(row_index),
        _ptr(n_rows) if n_rows is not None else None,
        _ptr(row_coeffs) if row_coeffs is not None else None,
        _ptr(mix) if mix is not None else None, int(seed) & 0xFFFFFFFFFFFFFFFF,
        _ptr(out), _ptr(out_coeffs), _ptr(status)), "recode_batch")


def rank_batch(row_index, rank, status, k: int, *, r: int = 0, max_rows: int, G: int, n_rows=None,
               row_coeffs=None, innovative=None, ctx: Optional[Context] = None) -> None:
    """qf_rank_batch: the rank of what each of G generations holds and,
    optionally, which slots are innovative (innovative: [G, max_rows] bytes,
    1 iff the slot's vector is not in the span of the slots before it).
    Indices, n_rows and row_coeffs as decode_batch; no payload is read."""
    _need_rows(G, max_rows, k, None, None, row_index, row_coeffs, n_rows)
    _need(rank, 4 * G, "rank")
    _need(status, 4 * G, "status")
    _need(innovative, G * max_rows, "innovative")
    ctx = ctx or default_context()
    sh = L.RankShape(k, r, max_rows, 0)
    check(L._lib().qf_rank_batch(
        ctx.handle, ctypes.byref(sh), G, _ptr(row_index),
        _opt(n_rows),
        _opt(row_coeffs),
        _opt(innovative),
        _ptr(rank), _ptr(status)), "rank_batch")


def decode_innovative_batch(rows, row_index, rec, rec_index, n_rec, status, k: int, r: int, Lb: int, *,
                            max_rows: int, row_stride: int, rows_gen_stride: int, rec_row_stride: int,
                            rec_gen_stride: int, G: int, n_rows=None, row_coeffs=None, rank=None,
                            innovative=None, ctx: Optional[Context] = None) -> None:
    """qf_decode_innovative_batch: decode_batch over the innovative slots only
    (a row is accepted iff it raises the rank of the rows before it), for
    recoded traffic whose first k rows may be dependent.  rank ([G] u32) and
    innovative ([G, max_rows] bytes) are optional outputs, as rank_batch's."""
    em = min(k, r)
    _need(rows, _span(G, rows_gen_stride, max_rows, row_stride, Lb), "rows")
    _need_rows(G, max_rows, k, None, None, row_index, row_coeffs, n_rows)
    _need(rec, _span(G, rec_gen_stride, em, rec_row_stride, Lb), "rec")
    _need(rec_index, 2 * G * em, "rec_index (min(k, r) entries per generation)")
    _need(n_rec, 4 * G, "n_rec")
    _need(status, 4 * G, "status")
    _need(rank, 4 * G, "rank")
    _need(innovative, G * max_rows, "innovative")
    ctx = ctx or default_context()
    sh = L.DecodeShape(k, r, Lb, max_rows, row_stride, rows_gen_stride, rec_row_stride, rec_gen_stride)
    check(L._lib().qf_decode_innovative_batch(
        ctx.handle, ctypes.byref(sh), G, _ptr(rows), _ptr(row_index),
        _opt(n_rows),
        _opt(row_coeffs),
        _opt(rec), _opt(rec_index),
        _ptr(n_rec), _ptr(status),
        _opt(rank),
        _opt(innovative)), "decode_innovative_batch")


def frame_payload_offset(k: int) -> int:
    """qf_frame_payload_offset: byte P = round_up(3 + k, 16) of a frame slot at
    which every payload sits in the payload-aligned layout (0 for k outside
    1..256).  Host only."""
    return int(L._lib().qf_frame_payload_offset(int(k) & 0xFFFFFFFF))


def frame_rows(rows, frames, frame_len, k: int, Lb: int, *, r: int = 0, max_rows: int, row_stride: int = 0,
               rows_gen_stride: int = 0, frame_stride: int, G: int, row_index=None, n_rows=None, row_coeffs=None,
               row_len=None, frame_off=None, in_place: bool = False, ctx: Optional[Context] = None) -> None:
    """qf_frame_rows_dev: rows with index and vector -> frames in the
    payload-aligned layout (frame f = g*max_rows + s at frames + f*frame_stride,
    its bytes at [frame_off[f], frame_off[f] + frame_len[f])).  Inputs as
    recode_batch; row_index None: every row coded (the recoder's output with
    row_coeffs = its out_coeffs).  in_place: the payloads already sit at byte
    frame_payload_offset(k) of their slots, rows may be None and only the
    headers are written."""
    P = frame_payload_offset(k)
    if not in_place:
        _need(rows, _span(G, rows_gen_stride, max_rows, row_stride, Lb), "rows")
    _need(frames, _span(G * max_rows, frame_stride, 1, 0, P + Lb), "frames")
    _need(frame_len, 4 * G * max_rows, "frame_len")
    _need(frame_off, 4 * G * max_rows, "frame_off")
    _need_rows(G, max_rows, k, None, row_len, row_index, row_coeffs, n_rows)
    ctx = ctx or default_context()
    sh = L.FrameRowsShape(k, r, Lb, max_rows, L.QF_FRAME_IN_PLACE if in_place else 0, 0, row_stride, rows_gen_stride,
                          frame_stride)
    check(L._lib().qf_frame_rows_dev(
        ctx.handle, ctypes.byref(sh), G, _ptr(rows) if (rows is not None and not in_place) else None,
        _opt(row_index),
        _opt(n_rows),
        _opt(row_coeffs),
        _opt(row_len),
        _ptr(frames), _ptr(frame_len),
        _opt(frame_off)), "frame_rows")


def parse_frames_coded(frames, frame_len, ids, rows, row_index, n_rows, frame_status, row_coeffs, k: int, Lb: int, *,
                       max_rows: int, frame_stride: int, row_stride: int, rows_gen_stride: int, G: int,
                       n_frames=None, frame_off=None, row_len=None, ctx: Optional[Context] = None) -> None:
    """qf_parse_frames_coded_dev: received frames -> rows, row_index, n_rows and
    row_coeffs ([G, max_rows, k] bytes: the frame's vector, or the unit vector
    of a systematic frame), the inputs of recode_batch, rank_batch and
    decode_innovative_batch.  Any coefficient vector of length k is accepted.
    frame_off: where each frame starts inside its slot (frame_rows' output);
    row_len: optional output, the payload bytes before zero padding."""
    _need(frames, G * max_rows * frame_stride, "frames")
    _need(frame_len, 4 * G * max_rows, "frame_len")
    _need(ids, 8 * G * max_rows, "ids")
    _need(rows, _span(G, rows_gen_stride, max_rows, row_stride, Lb), "rows")
    _need_rows(G, max_rows, k, None, row_len, row_index, row_coeffs, n_rows)
    _need(frame_status, 4 * G * max_rows, "frame_status")
    _need(n_frames, 4 * G, "n_frames")
    _need(frame_off, 4 * G * max_rows, "frame_off")
    ctx = ctx or default_context()
    check(L._lib().qf_parse_frames_coded_dev(
        ctx.handle, k, Lb, G, max_rows, _ptr(frames), frame_stride, _ptr(frame_len),
        _opt(frame_off), _ptr(ids),
        _opt(n_frames),
        _ptr(rows), row_stride, rows_gen_stride, _ptr(row_index), _ptr(n_rows), _ptr(row_coeffs),
        _opt(row_len), _ptr(frame_status)), "parse_frames_coded")


def parse_frame_headers(frames, frame_len, ids, row_index, n_rows, frame_status, row_coeffs, row_len, row_off,
                        k: int, Lb: int, *, max_rows: int, frame_stride: int, G: int, n_frames=None,
                        frame_off=None, ctx: Optional[Context] = None) -> None:
    """qf_parse_frame_headers_dev: parse_frames_coded that reads the headers
    only.  The payloads stay in their slots; compacted row c of generation g is
    the row_len[g, c] bytes at byte row_off[g, c] of the generation's frame
    region (frames + g*max_rows*frame_stride), the input of recode_frames.  A
    frame whose payload does not start at a multiple of 16 in its slot is
    QF_EINVAL."""
    _need(frames, G * max_rows * frame_stride, "frames")
    _need(frame_len, 4 * G * max_rows, "frame_len")
    _need(ids, 8 * G * max_rows, "ids")
    _need_rows(G, max_rows, k, row_off, row_len, row_index, row_coeffs, n_rows)
    _need(frame_status, 4 * G * max_rows, "frame_status")
    _need(n_frames, 4 * G, "n_frames")
    _need(frame_off, 4 * G * max_rows, "frame_off")
    ctx = ctx or default_context()
    check(L._lib().qf_parse_frame_headers_dev(
        ctx.handle, k, Lb, G, max_rows, _ptr(frames), frame_stride, _ptr(frame_len),
        _opt(frame_off), _ptr(ids),
        _opt(n_frames),
        _ptr(row_index), _ptr(n_rows), _ptr(row_coeffs), _ptr(row_len), _ptr(row_off), _ptr(frame_status)),
        "parse_frame_headers")


def recode_frames(src, row_off, row_len, row_index, row_coeffs, out, out_coeffs, status, k: int, m: int, Lb: int, *,
                  max_rows: int, src_gen_stride: int, out_row_stride: int, out_gen_stride: int, G: int,
                  n_rows=None, mix=None, seed: int = 0, out_len=None, ctx: Optional[Context] = None) -> None:
    """qf_recode_frames_dev: recode_batch (r = 0) over rows that lie where they
    were received: row c of generation g is the row_len[g, c] bytes at
    src + g*src_gen_stride + row_off[g, c], zero padded to Lb (what
    parse_frame_headers leaves, with src = the frames and src_gen_stride =
    max_rows * frame_stride).  out_len: optional [G, m] u32, the longest row
    length of each generation (frame_rows' row_len for the recoded rows)."""
    _need(src, G * src_gen_stride, "src")
    _need_rows(G, max_rows, k, row_off, row_len, row_index, row_coeffs, n_rows)
    _need(out, _span(G, out_gen_stride, m, out_row_stride, Lb), "out")
    _need(out_coeffs, G * m * k, "out_coeffs (m vectors of k bytes per generation)")
    _need(status, 4 * G, "status")
    _need(mix, G * m * max_rows, "mix")
    _need(out_len, 4 * G * m, "out_len")
    ctx = ctx or default_context()
    sh = L.RecodeFramesShape(k, Lb, max_rows, m, 0, 0, src_gen_stride, out_row_stride, out_gen_stride)
    check(L._lib().qf_recode_frames_dev(
        ctx.handle, ctypes.byref(sh), G, _ptr(src), _ptr(row_off), _ptr(row_len), _ptr(row_index),
        _opt(n_rows), _ptr(row_coeffs),
        _opt(mix), int(seed) & 0xFFFFFFFFFFFFFFFF,
        _ptr(out), _ptr(out_coeffs), _opt(out_len), _ptr(status)),
        "recode_frames")


def decode_frames(src, row_off, row_len, row_index, row_coeffs, rec, rec_index, n_rec, status, k: int, r: int,
                  Lb: int, *, max_rows: int, src_gen_stride: int, rec_row_stride: int, rec_gen_stride: int, G: int,
                  n_rows=None, rank=None, innovative=None, src_slot=None, ctx: Optional[Context] = None,
                  _call: str = "decode_frames") -> None:
    """qf_decode_frames_dev: decode_innovative_batch over rows that lie where
    they were received (rows as recode_frames': what parse_frame_headers
    leaves, with src = the frames and src_gen_stride = max_rows *
    frame_stride).  rec, rec_index, n_rec, status, rank and innovative as
    decode_innovative_batch's.  src_slot: optional [G, k] u16, for a QF_OK
    generation the slot of the accepted systematic row of each source, 0xFFFF
    for a recovered one (found in rec through rec_index)."""
    em = min(k, r)
    _need(src, G * src_gen_stride, "src")
    _need_rows(G, max_rows, k, row_off, row_len, row_index, row_coeffs, n_rows)
    _need(rec, _span(G, rec_gen_stride, em, rec_row_stride, Lb), "rec")
    _need(rec_index, 2 * G * em, "rec_index (min(k, r) entries per generation)")
    _need(n_rec, 4 * G, "n_rec")
    _need(status, 4 * G, "status")
    _need(rank, 4 * G, "rank")
    _need(innovative, G * max_rows, "innovative")
    _need(src_slot, 2 * G * k, "src_slot")
    ctx = ctx or default_context()
    sh = L.DecodeFramesShape(k, r, Lb, max_rows, 0, 0, src_gen_stride, rec_row_stride, rec_gen_stride)
    check(getattr(L._lib(), f"qf_{_call}_dev")(
        ctx.handle, ctypes.byref(sh), G, _ptr(src), _ptr(row_off), _ptr(row_len), _ptr(row_index),
        _opt(n_rows), _ptr(row_coeffs),
        _opt(rec), _opt(rec_index),
        _ptr(n_rec), _ptr(status),
        _opt(rank),
        _opt(innovative),
        _opt(src_slot)), _call)


def decode_partial_frames(src, row_off, row_len, row_index, row_coeffs, rec, rec_index, n_rec, status, k: int, r: int,
                          Lb: int, **kw) -> None:
    """qf_decode_partial_frames_dev: decode_frames' arguments and outputs, for
    generations of any rank.  n_rec / rec_index / rec: the sources without an
    accepted systematic row that the accepted rows determine (all of them at
    rank k, where every output equals decode_frames'); status QF_ENOTREADY
    below rank k, with those outputs and src_slot valid."""
    decode_frames(src, row_off, row_len, row_index, row_coeffs, rec, rec_index, n_rec, status, k, r, Lb,
                  _call="decode_partial_frames", **kw)


def rank_state_bytes(k: int) -> int:
    """qf_rank_state_bytes: bytes of one generation's rank state (a multiple of
    16; 0 for k outside 1..256).  Host only."""
    return int(L._lib().qf_rank_state_bytes(int(k) & 0xFFFFFFFF))


def rank_update_batch(row_index, state, rank, status, k: int, *, r: int = 0, max_rows: int, G: int, n_rows=None,
                      row_coeffs=None, innovative=None, ctx: Optional[Context] = None) -> None:
    """qf_rank_update_batch: rank_batch that resumes from and writes back a
    per-generation rank state (state: G * rank_state_bytes(k) bytes, 16-byte
    aligned, all zero = nothing received).  The flags of successive calls,
    concatenated, and the last rank are those of one rank_batch over all the
    slots.  A generation without a slot in the call is not written."""
    _need_rows(G, max_rows, k, None, None, row_index, row_coeffs, n_rows)
    _need(state, G * rank_state_bytes(k), "state (rank_state_bytes(k) per generation)")
    _need(rank, 4 * G, "rank")
    _need(status, 4 * G, "status")
    _need(innovative, G * max_rows, "innovative")
    ctx = ctx or default_context()
    sh = L.RankShape(k, r, max_rows, 0)
    check(L._lib().qf_rank_update_batch(
        ctx.handle, ctypes.byref(sh), G, _ptr(row_index),
        _opt(n_rows),
        _opt(row_coeffs),
        _ptr(state),
        _opt(innovative),
        _ptr(rank), _ptr(status)), "rank_update_batch")


def store_append(src, row_off, row_len, row_index, row_coeffs, store, store_off, store_len, store_index,
                 store_coeffs, store_n, status, k: int, Lb: int, *, max_rows: int, cap: int, src_gen_stride: int,
                 store_row_stride: int, store_gen_stride: int, G: int, n_rows=None, take=None,
                 ctx: Optional[Context] = None) -> None:
    """qf_store_append_dev: the taken rows (take: [G, max_rows] bytes, None =
    all; rank_update_batch's innovative) of what parse_frame_headers leaves are
    appended to each generation's row store behind its store_n rows.  The five
    store arrays with max_rows = cap and src_gen_stride = store_gen_stride are
    the inputs of decode_frames and (cap <= 255) recode_frames."""
    _need(src, G * src_gen_stride, "src")
    _need_rows(G, max_rows, k, row_off, row_len, row_index, row_coeffs, n_rows)
    _need(store, _span(G, store_gen_stride, cap, store_row_stride, (Lb + 15) // 16 * 16), "store")
    _need(store_off, 4 * G * cap, "store_off")
    _need(store_len, 4 * G * cap, "store_len")
    _need(store_index, 2 * G * cap, "store_index")
    _need(store_coeffs, G * cap * k, "store_coeffs")
    _need(store_n, 4 * G, "store_n")
    _need(status, 4 * G, "status")
    _need(take, G * max_rows, "take")
    ctx = ctx or default_context()
    sh = L.StoreShape(k, Lb, max_rows, cap, 0, 0, src_gen_stride, store_row_stride, store_gen_stride)
    check(L._lib().qf_store_append_dev(
        ctx.handle, ctypes.byref(sh), G, _ptr(src), _ptr(row_off), _ptr(row_len), _ptr(row_index),
        _opt(n_rows), _ptr(row_coeffs),
        _opt(take),
        _ptr(store), _ptr(store_off), _ptr(store_len), _ptr(store_index), _ptr(store_coeffs), _ptr(store_n),
        _ptr(status)), "store_append")


QF_SELECT_MARK = L.QF_SELECT_MARK


def gen_select(rank, sel, n_sel, *, G: int, min_rank: int, n_max: int, seen=None, mark: bool = False, n_match=None,
               ctx: Optional[Context] = None) -> None:
    """qf_gen_select_dev: the first n_max generations g of 0..G-1 with rank[g]
    >= min_rank and (seen is None or rank[g] > seen[g]) go to sel[0..] in
    ascending order, their number to n_sel[0] and the number of all matches to
    n_match[0].  mark: seen[g] = rank[g] for the selected generations."""
    _need(sel, 4 * n_max, "sel")
    _need(n_sel, 4, "n_sel")
    if G:
        _need(rank, 4 * G, "rank")
    _need(seen, 4 * G, "seen")
    _need(n_match, 4, "n_match")
    ctx = ctx or default_context()
    check(L._lib().qf_gen_select_dev(
        ctx.handle, G, _opt(rank), _opt(seen),
        min_rank, QF_SELECT_MARK if mark else 0, n_max, _ptr(sel), _ptr(n_sel),
        _opt(n_match)), "gen_select")


def _gen_sel(sel, n_sel, n_max: int, G_src: int) -> "L.GenSel":
    _need(sel, 4 * n_max, "sel")
    _need(n_sel, 4, "n_sel")
    return L.GenSel(_ptr(sel), _opt(n_sel), n_max, G_src)


def decode_frames_sel(sel, n_sel, src, row_off, row_len, row_index, row_coeffs, rec, rec_index, n_rec, status,
                      k: int, r: int, Lb: int, *, n_max: int, G_src: int, max_rows: int, src_gen_stride: int,
                      rec_row_stride: int, rec_gen_stride: int, n_rows=None, rank=None, innovative=None,
                      src_slot=None, ctx: Optional[Context] = None, _call: str = "decode_frames_sel") -> None:
    """qf_decode_frames_sel_dev: decode_frames over the generations sel[0 ..
    min(n_sel[0], n_max)) (n_sel None: n_max) of source arrays that hold G_src
    generations.  Every output is compact: entry j of rec, rec_index, n_rec,
    status, rank, innovative and src_slot belongs to generation sel[j]."""
    em = min(k, r)
    G = n_max
    _need(src, G_src * src_gen_stride, "src")
    _need_rows(G_src, max_rows, k, row_off, row_len, row_index, row_coeffs, n_rows)
    _need(rec, _span(G, rec_gen_stride, em, rec_row_stride, Lb), "rec")
    _need(rec_index, 2 * G * em, "rec_index (min(k, r) entries per list entry)")
    _need(n_rec, 4 * G, "n_rec")
    _need(status, 4 * G, "status")
    _need(rank, 4 * G, "rank")
    _need(innovative, G * max_rows, "innovative")
    _need(src_slot, 2 * G * k, "src_slot")
    gs = _gen_sel(sel, n_sel, n_max, G_src)
    ctx = ctx or default_context()
    sh = L.DecodeFramesShape(k, r, Lb, max_rows, 0, 0, src_gen_stride, rec_row_stride, rec_gen_stride)
    check(getattr(L._lib(), f"qf_{_call}_dev")(
        ctx.handle, ctypes.byref(sh), ctypes.byref(gs), _ptr(src), _ptr(row_off), _ptr(row_len), _ptr(row_index),
        _opt(n_rows), _ptr(row_coeffs),
        _opt(rec), _opt(rec_index),
        _ptr(n_rec), _ptr(status),
        _opt(rank),
        _opt(innovative),
        _opt(src_slot)), _call)


def decode_partial_frames_sel(sel, n_sel, src, row_off, row_len, row_index, row_coeffs, rec, rec_index, n_rec,
                              status, k: int, r: int, Lb: int, **kw) -> None:
    """qf_decode_partial_frames_sel_dev: decode_partial_frames over a list, with
    decode_frames_sel's arguments and compact outputs (the evict list of
    gen_window before the resets, or gen_select with min_rank 1 for a flush)."""
    decode_frames_sel(sel, n_sel, src, row_off, row_len, row_index, row_coeffs, rec, rec_index, n_rec, status, k, r,
                      Lb, _call="decode_partial_frames_sel", **kw)


def recode_frames_sel(sel, n_sel, src, row_off, row_len, row_index, row_coeffs, out, out_coeffs, status, k: int,
                      m: int, Lb: int, *, n_max: int, G_src: int, max_rows: int, src_gen_stride: int,
                      out_row_stride: int, out_gen_stride: int, n_rows=None, mix=None, seed: int = 0, out_len=None,
                      ctx: Optional[Context] = None) -> None:
    """qf_recode_frames_sel_dev: recode_frames over a list (as
    decode_frames_sel).  out, out_coeffs, out_len, status and mix (or the
    seeded stream) are indexed by the list position.  An unused entry gets
    QF_ENOTREADY, out_len 0 and zero out_coeffs; its payload rows are not
    written."""
    G = n_max
    _need(src, G_src * src_gen_stride, "src")
    _need_rows(G_src, max_rows, k, row_off, row_len, row_index, row_coeffs, n_rows)
    _need(out, _span(G, out_gen_stride, m, out_row_stride, Lb), "out")
    _need(out_coeffs, G * m * k, "out_coeffs (m vectors of k bytes per list entry)")
    _need(status, 4 * G, "status")
    _need(mix, G * m * max_rows, "mix")
    _need(out_len, 4 * G * m, "out_len")
    gs = _gen_sel(sel, n_sel, n_max, G_src)
    ctx = ctx or default_context()
    sh = L.RecodeFramesShape(k, Lb, max_rows, m, 0, 0, src_gen_stride, out_row_stride, out_gen_stride)
    check(L._lib().qf_recode_frames_sel_dev(
        ctx.handle, ctypes.byref(sh), ctypes.byref(gs), _ptr(src), _ptr(row_off), _ptr(row_len), _ptr(row_index),
        _opt(n_rows), _ptr(row_coeffs),
        _opt(mix), int(seed) & 0xFFFFFFFFFFFFFFFF,
        _ptr(out), _ptr(out_coeffs), _opt(out_len), _ptr(status)),
        "recode_frames_sel")


def stream_reset(sel, n_sel, k: int, *, n_max: int, G_src: int, state=None, store_n=None, seen=None,
                 ctx: Optional[Context] = None) -> None:
    """qf_stream_reset_dev: zeroes the rank state (rank_state_bytes(k) bytes),
    store_n and seen of the listed generations, each where it is given."""
    _need(state, G_src * rank_state_bytes(k), "state (rank_state_bytes(k) per generation)")
    _need(store_n, 4 * G_src, "store_n")
    _need(seen, 4 * G_src, "seen")
    gs = _gen_sel(sel, n_sel, n_max, G_src)
    ctx = ctx or default_context()
    check(L._lib().qf_stream_reset_dev(
        ctx.handle, k, ctypes.byref(gs), _opt(state),
        _opt(store_n), _opt(seen)), "stream_reset")


def parse_poll_headers(frames, frame_len, ids, frame_gen, sel, n_sel, row_index, n_rows, row_coeffs, row_len, row_off,
                       entry_status, frame_status, k: int, Lb: int, *, max_rows: int, frame_stride: int, N_max: int,
                       G_src: int, n_max: int, n_frames=None, frame_off=None, n_match=None,
                       ctx: Optional[Context] = None) -> None:
    """qf_parse_poll_headers_dev: a flat poll (N_max frame slots in arrival
    order, frame_gen[f] the generation tag of frame f, n_frames[0] the frames
    to look at) grouped by generation and parsed where the frames lie.  sel /
    n_sel / n_match receive the touched generations as gen_select's list; the
    row arrays are indexed by the list position ([n_max, max_rows]) and are
    what parse_frame_headers leaves for the entry's frames in arrival order,
    with row_off relative to frames.  entry_status: [n_max]; frame_status:
    [N_max]."""
    _need(frames, N_max * frame_stride, "frames")
    _need(frame_len, 4 * N_max, "frame_len")
    _need(ids, 8 * N_max, "ids")
    _need(frame_gen, 4 * N_max, "frame_gen")
    _need(frame_off, 4 * N_max, "frame_off")
    _need(n_frames, 4, "n_frames")
    _need(sel, 4 * n_max, "sel")
    _need(n_sel, 4, "n_sel")
    _need(n_match, 4, "n_match")
    _need_rows(n_max, max_rows, k, row_off, row_len, row_index, row_coeffs, n_rows)
    _need(entry_status, 4 * n_max, "entry_status")
    _need(frame_status, 4 * N_max, "frame_status")
    ctx = ctx or default_context()
    check(L._lib().qf_parse_poll_headers_dev(
        ctx.handle, k, Lb, max_rows, _ptr(frames), frame_stride, N_max, _ptr(frame_len),
        _opt(frame_off), _ptr(ids), _ptr(frame_gen),
        _opt(n_frames), G_src, n_max, _ptr(sel), _ptr(n_sel),
        _opt(n_match),
        _ptr(row_index), _ptr(n_rows), _ptr(row_coeffs), _ptr(row_len), _ptr(row_off), _ptr(entry_status),
        _ptr(frame_status)), "parse_poll_headers")


def rank_update_sel_batch(sel, n_sel, row_index, state, status, k: int, *, r: int = 0, max_rows: int, n_max: int,
                          G_src: int, n_rows=None, row_coeffs=None, innovative=None, rank_sel=None, rank=None,
                          ctx: Optional[Context] = None) -> None:
    """qf_rank_update_sel_batch: rank_update_batch over a list.  The slots
    (row_index, n_rows, row_coeffs) and innovative, status and rank_sel are
    indexed by the list position; state (G_src * rank_state_bytes(k) bytes) and
    rank ([G_src], only the listed entries' are written) by sel[j]."""
    _need_rows(n_max, max_rows, k, None, None, row_index, row_coeffs, n_rows)
    _need(state, G_src * rank_state_bytes(k), "state (rank_state_bytes(k) per generation)")
    _need(status, 4 * n_max, "status")
    _need(innovative, n_max * max_rows, "innovative")
    _need(rank_sel, 4 * n_max, "rank_sel")
    _need(rank, 4 * G_src, "rank")
    gs = _gen_sel(sel, n_sel, n_max, G_src)
    ctx = ctx or default_context()
    sh = L.RankShape(k, r, max_rows, 0)
    check(L._lib().qf_rank_update_sel_batch(
        ctx.handle, ctypes.byref(sh), ctypes.byref(gs), _ptr(row_index),
        _opt(n_rows),
        _opt(row_coeffs),
        _ptr(state),
        _opt(innovative),
        _opt(rank_sel),
        _opt(rank),
        _ptr(status)), "rank_update_sel_batch")


def store_append_sel(sel, n_sel, src, row_off, row_len, row_index, row_coeffs, store, store_off, store_len,
                     store_index, store_coeffs, store_n, status, k: int, Lb: int, *, max_rows: int, cap: int,
                     src_bytes: int, store_row_stride: int, store_gen_stride: int, n_max: int, G_src: int,
                     n_rows=None, take=None, ctx: Optional[Context] = None) -> None:
    """qf_store_append_sel_dev: store_append over a list.  The rows (row_off
    relative to src, the flat poll's frames of src_bytes bytes), take and
    status are indexed by the list position; the five store arrays and store_n
    hold G_src generations and are indexed by sel[j]."""
    _need(src, src_bytes, "src")
    _need_rows(n_max, max_rows, k, row_off, row_len, row_index, row_coeffs, n_rows)
    _need(store, _span(G_src, store_gen_stride, cap, store_row_stride, (Lb + 15) // 16 * 16), "store")
    _need(store_off, 4 * G_src * cap, "store_off")
    _need(store_len, 4 * G_src * cap, "store_len")
    _need(store_index, 2 * G_src * cap, "store_index")
    _need(store_coeffs, G_src * cap * k, "store_coeffs")
    _need(store_n, 4 * G_src, "store_n")
    _need(status, 4 * n_max, "status")
    _need(take, n_max * max_rows, "take")
    gs = _gen_sel(sel, n_sel, n_max, G_src)
    ctx = ctx or default_context()
    sh = L.StoreShape(k, Lb, max_rows, cap, 0, 0, src_bytes, store_row_stride, store_gen_stride)
    check(L._lib().qf_store_append_sel_dev(
        ctx.handle, ctypes.byref(sh), ctypes.byref(gs), _ptr(src), _ptr(row_off), _ptr(row_len), _ptr(row_index),
        _opt(n_rows), _ptr(row_coeffs),
        _opt(take),
        _ptr(store), _ptr(store_off), _ptr(store_len), _ptr(store_index), _ptr(store_coeffs), _ptr(store_n),
        _ptr(status)), "store_append_sel")


QF_WINDOW_CLOSE = L.QF_WINDOW_CLOSE
QF_GEN_NONE = L.QF_GEN_NONE


def gen_window(frame_id, win, frame_gen, frame_status, evict_sel, n_evict, *, G_src: int, N_max: int,
               n_evict_max: int, n_frames=None, evict_id=None, ctx: Optional[Context] = None) -> None:
    """qf_gen_window_dev: the step in front of parse_poll_headers.  frame_id
    [N_max] u64 wire generation ids, n_frames[0] the frames to look at; win
    [G_src] u64, the window (0: empty, else id + 1 with bit 63 the closed
    flag), updated to the newest id per slot.  frame_gen [N_max] receives the
    ingest's tags (the slot, or QF_GEN_NONE) and frame_status [N_max] QF_OK /
    QF_ESTALE / QF_ECLOSED / QF_EINVAL; evict_sel [n_evict_max], n_evict[0] and
    evict_id [n_evict_max] u64 the evicted open slots, ascending, and the ids
    they held: stream_reset's list."""
    _need(frame_id, 8 * N_max, "frame_id")
    _need(n_frames, 4, "n_frames")
    _need(win, 8 * G_src, "win")
    _need(frame_gen, 4 * N_max, "frame_gen")
    _need(frame_status, 4 * N_max, "frame_status")
    _need(evict_sel, 4 * n_evict_max, "evict_sel")
    _need(n_evict, 4, "n_evict")
    _need(evict_id, 8 * n_evict_max, "evict_id")
    ctx = ctx or default_context()
    check(L._lib().qf_gen_window_dev(
        ctx.handle, G_src, N_max, _opt(frame_id), _opt(n_frames), _ptr(win), 0, _opt(frame_gen), _opt(frame_status),
        n_evict_max, _ptr(evict_sel), _ptr(n_evict), _opt(evict_id)), "gen_window")


def gen_window_sel(sel, n_sel, win, *, n_max: int, G_src: int, ids=None, close: bool = False,
                   ctx: Optional[Context] = None) -> None:
    """qf_gen_window_sel_dev: ids [n_max] u64 receives the wire id each listed
    slot holds (UINT64_MAX for invalid, unused and empty entries); close sets
    the closed flag of the listed non-empty entries of win [G_src] u64."""
    _need(win, 8 * G_src, "win")
    _need(ids, 8 * n_max, "ids")
    gs = _gen_sel(sel, n_sel, n_max, G_src)
    ctx = ctx or default_context()
    check(L._lib().qf_gen_window_sel_dev(
        ctx.handle, ctypes.byref(gs), _ptr(win), QF_WINDOW_CLOSE if close else 0, _opt(ids)), "gen_window_sel")


QF_DELIVERED_WORDS = L.QF_DELIVERED_WORDS
QF_SRC_UNKNOWN, QF_SRC_STORED, QF_SRC_RECOVERED, QF_SRC_EARLIER = (L.QF_SRC_UNKNOWN, L.QF_SRC_STORED,
                                                                   L.QF_SRC_RECOVERED, L.QF_SRC_EARLIER)


def _need_deliver(G: int, k: int, em: int, Lb: int, rec, rec_index, n_rec, dec_status, src_slot, ids, out, out_len,
                  out_state, n_out, n_known, status, rec_row_stride: int, rec_gen_stride: int, out_row_stride: int,
                  out_gen_stride: int) -> None:
    """_need for the arguments of deliver_frames that are indexed by the
    generation (dense) or by the list position (listed)."""
    _need(rec, _span(G, rec_gen_stride, em, rec_row_stride, (Lb + 15) // 16 * 16), "rec (read in whole 16-byte units)")
    _need(rec_index, 2 * G * em, "rec_index (e_max entries per generation)")
    _need(n_rec, 4 * G, "n_rec")
    _need(dec_status, 4 * G, "dec_status")
    _need(src_slot, 2 * G * k, "src_slot")
    _need(ids, 8 * G, "ids")
    _need(out, _span(G, out_gen_stride, k, out_row_stride, (Lb + 15) // 16 * 16), "out")
    _need(out_len, 4 * G * k, "out_len")
    _need(out_state, G * k, "out_state")
    _need(n_out, 4 * G, "n_out")
    _need(n_known, 4 * G, "n_known")
    _need(status, 4 * G, "status")


def deliver_frames(src, row_off, row_len, rec, rec_index, n_rec, dec_status, src_slot, out, out_len, out_state, n_out,
                   status, k: int, e_max: int, Lb: int, *, max_rows: int, src_gen_stride: int, rec_row_stride: int,
                   rec_gen_stride: int, out_row_stride: int, out_gen_stride: int, G: int, ids=None, delivered=None,
                   n_known=None, ctx: Optional[Context] = None) -> None:
    """qf_deliver_frames_dev: the outputs of decode_frames / decode_partial_frames
    (rec, rec_index, n_rec, their status as dec_status, src_slot; e_max their
    min(k, r)) and the rows they read (src, row_off, row_len) to packets in
    source order: source i of generation g at out + g*out_gen_stride +
    i*out_row_stride, out_len [G, k] u32 its length and out_state [G, k] u8 one
    of QF_SRC_*.  delivered: optional [G, QF_DELIVERED_WORDS] u64 state, zeroed
    once, with which a source of a wire generation (ids [G] u64) leaves once
    across calls; n_out [G] the packets this call wrote, n_known [G] (optional)
    those known so far."""
    _need(src, G * src_gen_stride, "src")
    _need_rows(G, max_rows, k, row_off, row_len, None, None, None)
    _need(delivered, 8 * QF_DELIVERED_WORDS * G, "delivered (QF_DELIVERED_WORDS u64 per generation)")
    _need_deliver(G, k, e_max, Lb, rec, rec_index, n_rec, dec_status, src_slot, ids, out, out_len, out_state, n_out,
                  n_known, status, rec_row_stride, rec_gen_stride, out_row_stride, out_gen_stride)
    ctx = ctx or default_context()
    sh = L.DeliverShape(k, e_max, Lb, max_rows, 0, 0, src_gen_stride, rec_row_stride, rec_gen_stride, out_row_stride,
                        out_gen_stride)
    check(L._lib().qf_deliver_frames_dev(
        ctx.handle, ctypes.byref(sh), G, _opt(src), _opt(row_off), _opt(row_len), _opt(rec), _opt(rec_index),
        _opt(n_rec), _opt(dec_status), _opt(src_slot), _opt(ids), _opt(delivered), _opt(out), _opt(out_len),
        _opt(out_state), _opt(n_out), _opt(n_known), _opt(status)), "deliver_frames")


def deliver_frames_sel(sel, n_sel, src, row_off, row_len, rec, rec_index, n_rec, dec_status, src_slot, out, out_len,
                       out_state, n_out, status, k: int, e_max: int, Lb: int, *, n_max: int, G_src: int,
                       max_rows: int, src_gen_stride: int, rec_row_stride: int, rec_gen_stride: int,
                       out_row_stride: int, out_gen_stride: int, ids=None, delivered=None, n_known=None,
                       ctx: Optional[Context] = None) -> None:
    """qf_deliver_frames_sel_dev: deliver_frames over a list.  src, row_off,
    row_len and delivered hold G_src generations and are indexed by sel[j];
    everything else is indexed by the list position, as decode_frames_sel and
    decode_partial_frames_sel leave their outputs and gen_window_sel /
    gen_window's evict_id the ids."""
    _need(src, G_src * src_gen_stride, "src")
    _need_rows(G_src, max_rows, k, row_off, row_len, None, None, None)
    _need(delivered, 8 * QF_DELIVERED_WORDS * G_src, "delivered (QF_DELIVERED_WORDS u64 per generation)")
    _need_deliver(n_max, k, e_max, Lb, rec, rec_index, n_rec, dec_status, src_slot, ids, out, out_len, out_state,
                  n_out, n_known, status, rec_row_stride, rec_gen_stride, out_row_stride, out_gen_stride)
    gs = _gen_sel(sel, n_sel, n_max, G_src)
    ctx = ctx or default_context()
    sh = L.DeliverShape(k, e_max, Lb, max_rows, 0, 0, src_gen_stride, rec_row_stride, rec_gen_stride, out_row_stride,
                        out_gen_stride)
    check(L._lib().qf_deliver_frames_sel_dev(
        ctx.handle, ctypes.byref(sh), ctypes.byref(gs), _opt(src), _opt(row_off), _opt(row_len), _opt(rec),
        _opt(rec_index), _opt(n_rec), _opt(dec_status), _opt(src_slot), _opt(ids), _opt(delivered), _opt(out),
        _opt(out_len), _opt(out_state), _opt(n_out), _opt(n_known), _opt(status)), "deliver_frames_sel")


QF_EMIT_APPEND = L.QF_EMIT_APPEND


def emit_frames_sel(sel, n_sel, rows, ids, frames, frame_len, frame_off, frame_id, frame_pkt, n_frames, entry_first,
                    entry_count, entry_status, k: int, Lb: int, *, n_max: int, G_src: int, max_rows: int, N_max: int,
                    row_stride: int, rows_gen_stride: int, frame_stride: int, row_index=None, n_rows=None,
                    row_coeffs=None, row_len=None, in_status=None, rank=None, sent=None, n_left=None,
                    append: bool = False, ctx: Optional[Context] = None) -> None:
    """qf_emit_frames_sel_dev: the compact rows of a list (rows, row_index,
    n_rows, row_coeffs, row_len and in_status by list position, as
    recode_frames_sel leaves them; ids [n_max] u64 as gen_window_sel writes
    them) appended to a flat queue of N_max frame slots: frames, frame_len,
    frame_off [N_max] u32, frame_id and frame_pkt [N_max] u64, n_frames [1],
    which are the flat poll gen_window and parse_poll_headers read.  rank and
    sent ([G_src] u32, both or neither) are the budget: an entry emits at most
    rank[sel[j]] - sent[sel[j]] frames and sent grows by what it emitted.
    entry_first, entry_count and entry_status [n_max] say where each entry's
    frames went; n_left [1] (optional) counts the wanted frames that did not
    fit.  append: start at n_frames[0] instead of 0."""
    P = frame_payload_offset(k)
    _need(rows, _span(n_max, rows_gen_stride, max_rows, row_stride, (Lb + 15) // 16 * 16),
          "rows (read in whole 16-byte units)")
    _need_rows(n_max, max_rows, k, None, row_len, row_index, row_coeffs, n_rows)
    _need(in_status, 4 * n_max, "in_status")
    _need(ids, 8 * n_max, "ids")
    _need(rank, 4 * G_src, "rank")
    _need(sent, 4 * G_src, "sent")
    _need(frames, _span(N_max, frame_stride, 1, 0, P + Lb), "frames")
    _need(frame_len, 4 * N_max, "frame_len")
    _need(frame_off, 4 * N_max, "frame_off")
    _need(frame_id, 8 * N_max, "frame_id")
    _need(frame_pkt, 8 * N_max, "frame_pkt")
    _need(n_frames, 4, "n_frames")
    _need(n_left, 4, "n_left")
    _need(entry_first, 4 * n_max, "entry_first")
    _need(entry_count, 4 * n_max, "entry_count")
    _need(entry_status, 4 * n_max, "entry_status")
    gs = _gen_sel(sel, n_sel, n_max, G_src)
    ctx = ctx or default_context()
    sh = L.EmitShape(k, Lb, max_rows, N_max, QF_EMIT_APPEND if append else 0, 0, row_stride, rows_gen_stride,
                     frame_stride)
    check(L._lib().qf_emit_frames_sel_dev(
        ctx.handle, ctypes.byref(sh), ctypes.byref(gs), _opt(rows), _opt(row_index), _opt(n_rows), _opt(row_coeffs),
        _opt(row_len), _opt(in_status), _opt(ids), _opt(rank), _opt(sent), _opt(frames), _opt(frame_len),
        _opt(frame_off), _opt(frame_id), _opt(frame_pkt), _opt(n_frames), _opt(n_left), _opt(entry_first),
        _opt(entry_count), _opt(entry_status)), "emit_frames_sel")


QF_REPORT_APPEND = L.QF_REPORT_APPEND
RANK_REPORT_DTYPE = L.RANK_REPORT_DTYPE


def rank_report_sel(sel, n_sel, win, rank, reports, n_reports, k: int, *, n_max: int, G_src: int, N_max: int,
                    n_left=None, append: bool = False, ctx: Optional[Context] = None) -> None:
    """qf_rank_report_sel_dev: what this node holds of the listed slots as
    16-byte records (RANK_REPORT_DTYPE) in reports [N_max]: the id of win
    [G_src] u64 and min(rank [G_src], k), k for a closed entry, and the hole
    {UINT64_MAX, 0, 0} for an empty entry or a slot >= G_src.  n_reports [1]
    receives the new length, n_left [1] (optional) the records that did not
    fit.  append: start at n_reports[0] instead of 0."""
    _need(win, 8 * G_src, "win")
    _need(rank, 4 * G_src, "rank")
    _need(reports, 16 * N_max, "reports (16 bytes per record)")
    _need(n_reports, 4, "n_reports")
    _need(n_left, 4, "n_left")
    gs = _gen_sel(sel, n_sel, n_max, G_src)
    ctx = ctx or default_context()
    check(L._lib().qf_rank_report_sel_dev(
        ctx.handle, k, ctypes.byref(gs), _opt(win), _opt(rank), N_max, QF_REPORT_APPEND if append else 0,
        _opt(reports), _opt(n_reports), _opt(n_left)), "rank_report_sel")


def report_frame_capacity(max_len: int) -> int:
    """qf_report_frame_capacity: the entries of a feedback packet of at most max_len bytes (0: no such packet)."""
    return int(L._lib().qf_report_frame_capacity(max_len))


def frame_reports(reports, n_reports, pkts, pkt_len, n_pkts, k: int, *, N_max: int, max_len: int, F_max: int,
                  stride: int, n_left=None, n_skipped=None, ctx: Optional[Context] = None) -> None:
    """qf_frame_reports_dev: the sendable records (id < 2^62, rank <= k,
    reserved 0) among the first n_reports[0] (optional: N_max) of reports
    [N_max], in order, as feedback packets "0x02 | c BE u16 | c x {id BE u64,
    rank BE u16}" of at most max_len bytes in the F_max slots of stride bytes of
    pkts.  pkt_len [F_max] and n_pkts [1] receive the packets' lengths and their
    number, n_left [1] (optional) the sendable records that did not fit,
    n_skipped [1] (optional) the records that are not sendable."""
    _need(reports, 16 * N_max, "reports (16 bytes per record)")
    _need(n_reports, 4, "n_reports")
    _need(pkts, F_max * stride, "pkts")
    _need(pkt_len, 4 * F_max, "pkt_len")
    _need(n_pkts, 4, "n_pkts")
    _need(n_left, 4, "n_left")
    _need(n_skipped, 4, "n_skipped")
    ctx = ctx or default_context()
    sh = L.ReportWireShape(k, max_len, F_max, 0, stride)
    check(L._lib().qf_frame_reports_dev(
        ctx.handle, ctypes.byref(sh), N_max, _opt(reports), _opt(n_reports), _opt(pkts), _opt(pkt_len), _opt(n_pkts),
        _opt(n_left), _opt(n_skipped)), "frame_reports")


def parse_report_frames(pkts, pkt_len, n_pkts, reports, n_reports, k: int, *, N_max: int, max_len: int, F_max: int,
                        stride: int, n_left=None, pkt_status=None, pkt_first=None, pkt_count=None,
                        append: bool = False, ctx: Optional[Context] = None) -> None:
    """qf_parse_report_frames_dev: the entries of the well-formed packets among
    the first n_pkts[0] (optional: F_max) slots of pkts, in packet and entry
    order, as records in reports [N_max] from 0 (append: from n_reports[0]);
    n_reports [1] receives the new length, n_left [1] (optional) the records
    that did not fit.  pkt_status / pkt_first / pkt_count [F_max] (optional)
    receive QF_OK / QF_EINVAL, the position of a packet's first record
    (0xFFFFFFFF: none) and its entries.  Entry values are not judged here:
    credit_update decides."""
    _need(pkts, F_max * stride, "pkts")
    _need(pkt_len, 4 * F_max, "pkt_len")
    _need(n_pkts, 4, "n_pkts")
    _need(reports, 16 * N_max, "reports (16 bytes per record)")
    _need(n_reports, 4, "n_reports")
    _need(n_left, 4, "n_left")
    _need(pkt_status, 4 * F_max, "pkt_status")
    _need(pkt_first, 4 * F_max, "pkt_first")
    _need(pkt_count, 4 * F_max, "pkt_count")
    ctx = ctx or default_context()
    sh = L.ReportWireShape(k, max_len, F_max, QF_REPORT_APPEND if append else 0, stride)
    check(L._lib().qf_parse_report_frames_dev(
        ctx.handle, ctypes.byref(sh), _opt(pkts), _opt(pkt_len), _opt(n_pkts), N_max, _opt(reports), _opt(n_reports),
        _opt(n_left), _opt(pkt_status), _opt(pkt_first), _opt(pkt_count)), "parse_report_frames")


def report_closed(frame_id, frame_status, n_frames, win, reports, n_reports, k: int, *, G_src: int, F_max: int,
                  N_max: int, n_left=None, append: bool = False, ctx: Optional[Context] = None) -> None:
    """qf_report_closed_dev: one record {id, k, 0} per window slot whose closed
    generation a QF_ECLOSED frame of this poll belongs to (frame_id [F_max] u64
    and frame_status [F_max] i32 of gen_window, n_frames [1] optional: F_max), in
    ascending slot order, in reports [N_max] from 0 (append: from n_reports[0]).
    n_reports [1] receives the new length, n_left [1] (optional) the records
    that did not fit."""
    _need(frame_id, 8 * F_max, "frame_id")
    _need(frame_status, 4 * F_max, "frame_status")
    _need(n_frames, 4, "n_frames")
    _need(win, 8 * G_src, "win")
    _need(reports, 16 * N_max, "reports (16 bytes per record)")
    _need(n_reports, 4, "n_reports")
    _need(n_left, 4, "n_left")
    ctx = ctx or default_context()
    check(L._lib().qf_report_closed_dev(
        ctx.handle, k, G_src, F_max, _opt(frame_id), _opt(frame_status), _opt(n_frames), _opt(win), N_max,
        QF_REPORT_APPEND if append else 0, _opt(reports), _opt(n_reports), _opt(n_left)), "report_closed")


def credit_update(win, rank, sent, fb_state, credit, k: int, *, G: int, num: int = 1, den: int = 1, cap: int,
                  N_max: int = 0, reports=None, n_reports=None, report_status=None,
                  ctx: Optional[Context] = None) -> None:
    """qf_credit_update_dev: credit [G] u32, the budget gen_select and
    emit_frames_sel take as rank beside sent, from the local rank [G], the ratio
    num / den, the cap and the peer's reports ([N_max] records, n_reports [1]
    optional: N_max).  fb_state [G * 16] bytes, zeroed once, remembers per slot
    the generation and the highest rank reported for it; win [G] u64 is the
    node's window.  report_status [N_max] i32 (optional) receives QF_OK /
    QF_ESTALE / QF_ENOTREADY / QF_EINVAL per report."""
    _need(win, 8 * G, "win")
    _need(rank, 4 * G, "rank")
    _need(sent, 4 * G, "sent")
    _need(fb_state, 16 * G, "fb_state (16 bytes per slot)")
    _need(credit, 4 * G, "credit")
    _need(reports, 16 * N_max, "reports (16 bytes per record)")
    _need(n_reports, 4, "n_reports")
    _need(report_status, 4 * N_max, "report_status")
    ctx = ctx or default_context()
    sh = L.CreditShape(k, num, den, cap, 0, 0)
    check(L._lib().qf_credit_update_dev(
        ctx.handle, ctypes.byref(sh), G, _opt(win), _opt(rank), _opt(sent), N_max, _opt(reports), _opt(n_reports),
        _opt(fb_state), _opt(credit), _opt(report_status)), "credit_update")


# ---------------------------------------------------------------------------
# Packet / MemoryPool / Encoder / Decoder (encoder.rs, decoder.rs, optimize.rs)
# ---------------------------------------------------------------------------
class MemoryPool:
    """Stand-in for optimize.rs:417 MemoryPool: hands out zeroed blocks.

    The reference pool is a host allocator; payloads handed to the GPU path
    are copied into HBM by the encoder/decoder, so this only fixes the block
    size (the maximum packet length)."""

    def __init__(self, capacity: int, block_size: int):
        self.capacity = capacity
        self.block_size = block_size

    def alloc(self) -> bytearray:
        return bytearray(self.block_size)


@dataclass
class Packet:
    """encoder.rs:4-12."""
    id: int
    data: Optional[bytearray]
    len: int
    is_systematic: bool
    coefficients: Optional[bytes] = None
    coeff_len: int = 0

    def clone(self) -> "Packet":
        return Packet(self.id, bytearray(self.data) if self.data is not None else None, self.len,
                      self.is_systematic, self.coefficients, self.coeff_len)

    clone_for_encoder = clone  # encoder.rs:156 (deep copy)

    def payload(self) -> bytes:
        return bytes(self.data[: self.len]) if self.data is not None else b""

    def to_raw(self) -> bytes:
        """encoder.rs:124-152."""
        lib = L._lib()
        cap = self.len + 3 + self.coeff_len
        out = (ctypes.c_uint8 * max(1, cap))()
        n = ctypes.c_uint32(0)
        pay = (ctypes.c_uint8 * max(1, self.len)).from_buffer_copy(self.payload().ljust(max(1, self.len), b"\0"))
        co = None
        if self.coefficients is not None:
            co = (ctypes.c_uint8 * max(1, self.coeff_len)).from_buffer_copy(
                bytes(self.coefficients[: self.coeff_len]).ljust(max(1, self.coeff_len), b"\0"))
        check(lib.qf_packet_to_raw(1 if self.is_systematic else 0,
                                   ctypes.cast(co, ctypes.c_void_p) if co is not None else None,
                                   self.coeff_len, pay, self.len, out, cap, ctypes.byref(n)), "to_raw")
        return bytes(out)[: n.value]

    @staticmethod
    def from_raw(pid: int, raw: bytes, pool: Optional[MemoryPool] = None) -> "Packet":
        """encoder.rs:18-68."""
        lib = L._lib()
        buf = (ctypes.c_uint8 * max(1, len(raw))).from_buffer_copy(raw if raw else b"\0")
        sys_ = ctypes.c_int(0)
        cptr, pptr = ctypes.c_void_p(), ctypes.c_void_p()
        clen, plen = ctypes.c_uint32(0), ctypes.c_uint32(0)
        check(lib.qf_packet_from_raw(buf, len(raw), ctypes.byref(sys_), ctypes.byref(cptr),
                                     ctypes.byref(clen), ctypes.byref(pptr), ctypes.byref(plen)),
              "from_raw")
        base = ctypes.addressof(buf)
        coeffs = None
        if cptr.value:
            off = cptr.value - base
            coeffs = bytes(raw[off: off + clen.value])
        off = pptr.value - base
        payload = bytearray(raw[off: off + plen.value])
        if pool is not None:
            if len(payload) > pool.block_size:   # "Buffer from pool is too small" (encoder.rs:52-56)
                raise QfError(L.QF_ETOOSMALL, "from_raw: pool buffer too small")
            block = pool.alloc()
            block[: len(payload)] = payload
            payload = block
        return Packet(pid, payload, plen.value, bool(sys_.value), coeffs, clen.value)

    @staticmethod
    def from_block(pid: int, block: bytearray, length: int) -> "Packet":
        """encoder.rs:72-121: parse a received frame held in a pool block of
        `length` valid bytes; the payload is moved to the front of the same
        block (qf_packet_from_block)."""
        lib = L._lib()
        buf = (ctypes.c_uint8 * max(1, len(block))).from_buffer(block) if len(block) else (ctypes.c_uint8 * 1)()
        sys_ = ctypes.c_int(0)
        coeffs = (ctypes.c_uint8 * max(1, len(block)))()
        clen, plen = ctypes.c_uint32(0), ctypes.c_uint32(0)
        check(lib.qf_packet_from_block(buf, len(block), length, ctypes.byref(sys_), coeffs, len(block),
                                       ctypes.byref(clen), ctypes.byref(plen)), "from_block")
        co = bytes(coeffs)[: clen.value] if not sys_.value else None
        return Packet(pid, block, plen.value, bool(sys_.value), co, clen.value)


class Encoder:
    """decoder.rs:155-299 Encoder (GF(2^8), Cauchy coefficients)."""

    def __init__(self, k: int, n: int, max_len: int = 4096, ctx: Optional[Context] = None):
        self.k, self.n = k, n
        self.ctx = ctx or default_context()
        h = ctypes.c_void_p()
        check(L._lib().qf_encoder_new(self.ctx.handle, k, n, max_len, ctypes.byref(h)), "Encoder::new")
        self.handle = h
        self.max_len = max_len

    def add_source_packet(self, packet: Packet) -> None:
        data = packet.payload()
        buf = (ctypes.c_uint8 * max(1, len(data))).from_buffer_copy(data.ljust(max(1, len(data)), b"\0"))
        check(L._lib().qf_encoder_add_source_packet(self.handle, packet.id, buf, len(data)),
              "add_source_packet")

    def generate_repair_packet(self, repair_packet_index: int, pool: Optional[MemoryPool] = None) -> Optional[Packet]:
        """Returns None while the window holds fewer than k packets."""
        out = (ctypes.c_uint8 * self.max_len)()
        coeffs = (ctypes.c_uint8 * self.k)()
        n = ctypes.c_uint32(0)
        pid = ctypes.c_uint64(0)
        s = L._lib().qf_encoder_generate_repair_packet(self.handle, repair_packet_index, out, self.max_len,
                                                       ctypes.byref(n), coeffs, ctypes.byref(pid))
        if s == L.QF_ENOTREADY:
            return None
        check(s, "generate_repair_packet")
        block = pool.alloc() if pool is not None else bytearray(max(n.value, 1))
        block[: n.value] = bytes(out)[: n.value]
        return Packet(pid.value, block, n.value, False, bytes(coeffs), self.k)

    def generate_repairs(self, first: int, count: int) -> list[Packet]:
        """All repairs first..first+count-1 of the window in one launch."""
        stride = (self.max_len + 15) // 16 * 16
        out = (ctypes.c_uint8 * (stride * count))()
        coeffs = (ctypes.c_uint8 * (self.k * count))()
        lens = (ctypes.c_uint32 * count)()
        ids = (ctypes.c_uint64 * count)()
        s = L._lib().qf_encoder_generate_repairs(self.handle, first, count, out, stride, lens, coeffs, ids)
        if s == L.QF_ENOTREADY:
            return []
        check(s, "generate_repairs")
        raw = bytes(out)
        cb = bytes(coeffs)
        return [Packet(ids[q], bytearray(raw[q * stride: q * stride + lens[q]]), lens[q], False,
                       cb[q * self.k: (q + 1) * self.k], self.k) for q in range(count)]

    def __del__(self):  # pragma: no cover
        if _SHUTDOWN:
            return
        try:
            L._lib().qf_encoder_free(self.handle)
        except Exception:
            pass


class Decoder:
    """decoder.rs:658-791 Decoder (first k rows win, systematic id % k).
    k <= 256 decodes by Gauss-Jordan / the Cauchy kernels, k > 256 by the
    Wiedemann strategy (decoder.rs:660-664, 794-975), as Decoder::new picks.
    innovative_only=True (no reference counterpart, k <= 256): a packet is
    taken only if it raises the rank of the packets taken before it, so
    recoded traffic with dependent packets decodes once its rank reaches k."""

    def __init__(self, k: int, pool: Optional[MemoryPool] = None, max_len: int = 4096,
                 ctx: Optional[Context] = None, innovative_only: bool = False):
        self.k = k
        self.ctx = ctx or default_context()
        self.max_len = pool.block_size if pool is not None else max_len
        h = ctypes.c_void_p()
        check(L._lib().qf_decoder_new(self.ctx.handle, k, self.max_len, ctypes.byref(h)), "Decoder::new")
        self.handle = h
        self.innovative_only = bool(innovative_only)
        if innovative_only:
            check(L._lib().qf_decoder_set_innovative(self.handle, 1), "Decoder: innovative_only")

    @property
    def rank(self) -> int:
        """Rank of the packets accepted so far (qf_decoder_rank)."""
        return check(L._lib().qf_decoder_rank(self.handle), "Decoder.rank")

    @property
    def is_decoded(self) -> bool:
        return bool(check(L._lib().qf_decoder_is_decoded(self.handle)))

    @property
    def strategy(self) -> str:
        """decoder.rs:520-524 DecodingStrategy chosen by Decoder::new."""
        s = check(L._lib().qf_decoder_strategy(self.handle))
        return "Wiedemann" if s == 1 else "GaussianElimination"

    @property
    def solve_attempts(self) -> int:
        """Projections the last Wiedemann solve tried (1..8; 9 = exact
        elimination decided; 0: none yet / k <= 256)."""
        return check(L._lib().qf_decoder_solve_attempts(self.handle))

    def add_packet(self, packet: Packet) -> bool:
        """Returns is_decoded; raises for a repair packet without coefficients."""
        data = packet.payload()
        buf = (ctypes.c_uint8 * max(1, len(data))).from_buffer_copy(data.ljust(max(1, len(data)), b"\0"))
        co = None
        if packet.coefficients is not None:
            cb = bytes(packet.coefficients[: packet.coeff_len])
            co = (ctypes.c_uint8 * max(1, len(cb))).from_buffer_copy(cb.ljust(max(1, len(cb)), b"\0"))
        elif not packet.is_systematic:
            raise QfError(L.QF_EINVAL, "Repair packet missing coefficients.")
        s = L._lib().qf_decoder_add_packet(self.handle, packet.id, 1 if packet.is_systematic else 0, buf,
                                           len(data), ctypes.cast(co, ctypes.c_void_p) if co is not None else None,
                                           packet.coeff_len)
        return bool(check(s, "add_packet"))

    def get_decoded_packets(self) -> list[Packet]:
        stride = (self.max_len + 15) // 16 * 16
        out = (ctypes.c_uint8 * (stride * self.k))()
        lens = (ctypes.c_uint32 * self.k)()
        ids = (ctypes.c_uint64 * self.k)()
        cnt = ctypes.c_uint32(0)
        check(L._lib().qf_decoder_get_decoded_packets(self.handle, out, stride, lens, ids, ctypes.byref(cnt)),
              "get_decoded_packets")
        raw = bytes(out)
        res = []
        for i in range(cnt.value):
            block = bytearray(self.max_len)
            block[: lens[i]] = raw[i * stride: i * stride + lens[i]]
            res.append(Packet(ids[i], block, lens[i], True))
        return res

    def __del__(self):  # pragma: no cover
        if _SHUTDOWN:
            return
        try:
            L._lib().qf_decoder_free(self.handle)
        except Exception:
            pass


class Recoder:
    """A relay's view of one generation (no reference counterpart): it keeps
    the packets it receives, systematic or coded, in a device buffer and emits
    fresh linear combinations of them through recode_batch (G = 1).  Every
    recoded packet carries its coefficient vector over the k sources, so an
    unmodified Decoder takes it as a repair packet.  No CPU fallback."""

    def __init__(self, k: int, max_len: int, capacity: int, ctx: Optional[Context] = None):
        import torch

        if not (1 <= k <= 255 and 1 <= capacity <= 255 and max_len >= 1):
            raise QfError(L.QF_EINVAL, "Recoder: k, capacity in 1..255, max_len >= 1")
        self.k, self.max_len, self.capacity = k, max_len, capacity
        self.ctx = ctx or default_context()
        self.stride = (max_len + 15) // 16 * 16
        dev = f"cuda:{self.ctx.device}"
        self._rows = torch.zeros(capacity * self.stride, dtype=torch.uint8, device=dev)
        self._index = torch.zeros(capacity, dtype=torch.int16, device=dev)
        self._coeffs = torch.zeros(capacity * k, dtype=torch.uint8, device=dev)
        self.count = 0
        self._len = 0   # longest payload held: the length of the recoded packets

    def add_packet(self, packet: Packet) -> None:
        """Stores a systematic packet (column id % k, decoder.rs:684) or a
        coded one (its k coefficient bytes); shorter payloads count as zero
        padded, as in the encoder's window."""
        import torch

        if self.count >= self.capacity:
            raise QfError(L.QF_ETOOSMALL, "Recoder: capacity reached")
        data = packet.payload()
        if len(data) > self.max_len:
            raise QfError(L.QF_EINVAL, "Recoder: packet longer than max_len")
        s = self.count
        if packet.is_systematic:
            index = packet.id % self.k
        else:
            if packet.coefficients is None or packet.coeff_len != self.k:
                raise QfError(L.QF_EINVAL, "Repair packet missing coefficients.")
            index = self.k
            co = torch.frombuffer(bytearray(packet.coefficients[: self.k]), dtype=torch.uint8)
            self._coeffs[s * self.k: (s + 1) * self.k].copy_(co)
        row = torch.frombuffer(bytearray(data.ljust(self.stride, b"\0")), dtype=torch.uint8)
        self._rows[s * self.stride: (s + 1) * self.stride].copy_(row)
        self._index[s: s + 1].fill_(index)
        self.count += 1
        self._len = max(self._len, len(data))

    def rank(self) -> int:
        """Rank of the rows held (rank_batch, G = 1): how many of them a
        receiver can use, and the most independent packets recode can emit."""
        import torch

        if self.count == 0:
            return 0
        dev = self._rows.device
        rank = torch.empty(1, dtype=torch.int32, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        n_rows = torch.full((1,), self.count, dtype=torch.int32, device=dev)
        torch.cuda.current_stream(self.ctx.device).synchronize()
        rank_batch(self._index, rank, status, self.k, max_rows=self.capacity, G=1, n_rows=n_rows,
                   row_coeffs=self._coeffs, ctx=self.ctx)
        self.ctx.sync()
        check(int(status.cpu()[0]), "Recoder.rank")
        return int(rank.cpu()[0])

    def recode(self, count: int, seed: int, first_id: int = 0) -> list:
        """`count` (1..64) recoded packets of the rows held, ids first_id ..;
        an empty list while nothing is held.  Non-systematic packets with
        coefficients (coeff_len = k)."""
        import torch

        if self.count == 0 or self._len == 0:
            return []
        dev = self._rows.device
        k, stride = self.k, self.stride
        out = torch.empty(count * stride, dtype=torch.uint8, device=dev)
        oc = torch.empty(count * k, dtype=torch.uint8, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        n_rows = torch.full((1,), self.count, dtype=torch.int32, device=dev)
        torch.cuda.current_stream(self.ctx.device).synchronize()
        recode_batch(self._rows, self._index, out, oc, status, k, count, self._len, max_rows=self.capacity,
                     row_stride=stride, rows_gen_stride=self.capacity * stride, out_row_stride=stride,
                     out_gen_stride=count * stride, G=1, n_rows=n_rows, row_coeffs=self._coeffs, seed=seed,
                     ctx=self.ctx)
        self.ctx.sync()
        check(int(status.cpu()[0]), "Recoder.recode")
        raw, cb = out.cpu().numpy().tobytes(), oc.cpu().numpy().tobytes()
        return [Packet(first_id + j, bytearray(raw[j * stride: j * stride + self._len]), self._len, False,
                       cb[j * k: (j + 1) * k], k) for j in range(count)]


# ---------------------------------------------------------------------------
# GF(2^16) Extreme mode (gf_tables.rs:331-380, decoder.rs:10-88, 536-656)
# ---------------------------------------------------------------------------
def gf16_mul(a: int, b: int) -> int:
    """gf_tables.rs:333 gf16_mul with the reduction it intends."""
    return int(L._lib().qf_gf16_mul(a & 0xFFFF, b & 0xFFFF))


def gf16_inv(a: int) -> int:
    """gf_tables.rs:370 gf16_inv; raises for 0."""
    out = ctypes.c_uint16(0)
    check(L._lib().qf_gf16_inv(a & 0xFFFF, ctypes.byref(out)), "gf16_inv")
    return int(out.value)


def cauchy16_coefficients(k: int, r: int) -> list[list[int]]:
    """decoder.rs:77-80 for repairs 0..r-1."""
    buf = (ctypes.c_uint16 * max(1, k * r))()
    check(L._lib().qf_cauchy16_coeffs(k, r, buf), "cauchy16")
    return [list(buf[j * k: (j + 1) * k]) for j in range(r)]


def encode16_batch(src, rep, k: int, r: int, Lb: int, *, src_row_stride: int, src_gen_stride: int,
                   rep_row_stride: int, rep_gen_stride: int, G: int, coeff=None,
                   ctx: Optional[Context] = None) -> None:
    """qf_encode16_batch: GF(2^16) repairs of G generations (Encoder16,
    decoder.rs:33-75).  coeff: optional r x k u16 rows (default Cauchy)."""
    ctx = ctx or default_context()
    sh = L.EncodeShape(k, r, Lb, 0, src_row_stride, src_gen_stride, rep_row_stride, rep_gen_stride)
    cbuf = None
    if coeff is not None:
        flat = [int(v) for row in coeff for v in row]
        if len(flat) != k * r:
            raise ValueError("coeff must be r x k")
        cbuf = (ctypes.c_uint16 * len(flat))(*flat)
    check(L._lib().qf_encode16_batch(ctx.handle, ctypes.byref(sh), G, _ptr(src), _ptr(rep),
                                      ctypes.cast(cbuf, ctypes.c_void_p) if cbuf is not None else None),
          "encode16_batch")


def decode16_batch(rows, row_index, rec, rec_index, n_rec, status, k: int, r: int, Lb: int, *,
                   max_rows: int, row_stride: int, rows_gen_stride: int, rec_row_stride: int,
                   rec_gen_stride: int, G: int, n_rows=None, row_coeffs=None,
                   ctx: Optional[Context] = None) -> None:
    """qf_decode16_batch: Decoder16 (decoder.rs:563-656) over G generations;
    row_coeffs: optional u16 tensor [G, max_rows, k]."""
    ctx = ctx or default_context()
    sh = L.DecodeShape(k, r, Lb, max_rows, row_stride, rows_gen_stride, rec_row_stride, rec_gen_stride)
    check(L._lib().qf_decode16_batch(
        ctx.handle, ctypes.byref(sh), G, _ptr(rows), _ptr(row_index),
        _ptr(n_rows) if n_rows is not None else None,
        _ptr(row_coeffs) if row_coeffs is not None else None,
        _ptr(rec) if rec is not None else None, _ptr(rec_index) if rec_index is not None else None,
        _ptr(n_rec), _ptr(status)), "decode16_batch")


class Encoder16:
    """decoder.rs:10-88 Encoder16 over qf_encoder16_*: sliding window of k
    packets; repair j carries the Cauchy row y = k + j as a big-endian u16
    coefficient block of 2k bytes."""

    def __init__(self, k: int, n: int, max_len: int = 4096, ctx: Optional[Context] = None):
        self.k, self.n, self.max_len = k, n, max_len
        self.ctx = ctx or default_context()
        h = ctypes.c_void_p()
        check(L._lib().qf_encoder16_new(self.ctx.handle, k, n, max_len, ctypes.byref(h)), "Encoder16::new")
        self.handle = h

    def add_source_packet(self, packet: Packet) -> None:
        data = packet.payload()
        buf = (ctypes.c_uint8 * max(1, len(data))).from_buffer_copy(data.ljust(max(1, len(data)), b"\0"))
        check(L._lib().qf_encoder16_add_source_packet(self.handle, packet.id, buf, len(data)), "add_source_packet")

    def generate_repair_packet(self, repair_packet_index: int, pool: Optional[MemoryPool] = None) -> Optional[Packet]:
        out = (ctypes.c_uint8 * self.max_len)()
        coeffs = (ctypes.c_uint8 * (2 * self.k))()
        n = ctypes.c_uint32(0)
        pid = ctypes.c_uint64(0)
        s = L._lib().qf_encoder16_generate_repair_packet(self.handle, repair_packet_index, out, self.max_len,
                                                         ctypes.byref(n), coeffs, ctypes.byref(pid))
        if s == L.QF_ENOTREADY:
            return None
        check(s, "generate_repair_packet")
        block = pool.alloc() if pool is not None else bytearray(max(n.value, 1))
        block[: n.value] = bytes(out)[: n.value]
        return Packet(pid.value, block, n.value, False, bytes(coeffs), 2 * self.k)

    def generate_repairs(self, first: int, count: int) -> list[Packet]:
        stride = (self.max_len + 15) // 16 * 16
        out = (ctypes.c_uint8 * (stride * count))()
        coeffs = (ctypes.c_uint8 * (2 * self.k * count))()
        lens = (ctypes.c_uint32 * count)()
        ids = (ctypes.c_uint64 * count)()
        s = L._lib().qf_encoder16_generate_repairs(self.handle, first, count, out, stride, lens, coeffs, ids)
        if s == L.QF_ENOTREADY:
            return []
        check(s, "generate_repairs")
        raw, cb, kb = bytes(out), bytes(coeffs), 2 * self.k
        return [Packet(ids[q], bytearray(raw[q * stride: q * stride + lens[q]]), lens[q], False,
                       cb[q * kb: (q + 1) * kb], kb) for q in range(count)]

    def __del__(self):  # pragma: no cover
        if _SHUTDOWN:
            return
        try:
            L._lib().qf_encoder16_free(self.handle)
        except Exception:
            pass


class Decoder16:
    """decoder.rs:536-656 Decoder16 over qf_decoder16_*: the first k packets
    (systematic column id % k, repair rows from their big-endian u16
    coefficient blocks), no duplicate filtering.  Systematic payloads are
    carried (F4-style fix) and decoding runs once k rows are present, whatever
    the last row's kind; get_decoded_packets returns the whole generation."""

    def __init__(self, k: int, pool: Optional[MemoryPool] = None, max_len: int = 4096,
                 ctx: Optional[Context] = None):
        self.k = k
        self.ctx = ctx or default_context()
        self.max_len = pool.block_size if pool is not None else max_len
        h = ctypes.c_void_p()
        check(L._lib().qf_decoder16_new(self.ctx.handle, k, self.max_len, ctypes.byref(h)), "Decoder16::new")
        self.handle = h

    @property
    def is_decoded(self) -> bool:
        return bool(check(L._lib().qf_decoder16_is_decoded(self.handle)))

    def add_packet(self, packet: Packet) -> bool:
        data = packet.payload()
        buf = (ctypes.c_uint8 * max(1, len(data))).from_buffer_copy(data.ljust(max(1, len(data)), b"\0"))
        co = None
        if packet.coefficients is not None:
            cb = bytes(packet.coefficients[: packet.coeff_len])
            co = (ctypes.c_uint8 * max(1, len(cb))).from_buffer_copy(cb.ljust(max(1, len(cb)), b"\0"))
        elif not packet.is_systematic:
            raise QfError(L.QF_EINVAL, "missing coeffs")
        s = L._lib().qf_decoder16_add_packet(self.handle, packet.id, 1 if packet.is_systematic else 0, buf,
                                             len(data), ctypes.cast(co, ctypes.c_void_p) if co is not None else None,
                                             packet.coeff_len)
        return bool(check(s, "add_packet"))

    def get_decoded_packets(self) -> list[Packet]:
        stride = (self.max_len + 15) // 16 * 16
        out = (ctypes.c_uint8 * (stride * self.k))()
        lens = (ctypes.c_uint32 * self.k)()
        ids = (ctypes.c_uint64 * self.k)()
        cnt = ctypes.c_uint32(0)
        check(L._lib().qf_decoder16_get_decoded_packets(self.handle, out, stride, lens, ids, ctypes.byref(cnt)),
              "get_decoded_packets")
        raw = bytes(out)
        return [Packet(ids[i], bytearray(raw[i * stride: i * stride + lens[i]]), lens[i], True)
                for i in range(cnt.value)]

    def __del__(self):  # pragma: no cover
        if _SHUTDOWN:
            return
        try:
            L._lib().qf_decoder16_free(self.handle)
        except Exception:
            pass


# ---------------------------------------------------------------------------
# Adaptive FEC driver (adaptive.rs:11-631) over qf_adaptive_*
# ---------------------------------------------------------------------------
import enum
from collections import deque as _deque
from dataclasses import dataclass as _dataclass, field as _field


class FecMode(enum.IntEnum):
    """adaptive.rs:13-21 (with FromStr aliases, 23-37)."""
    Zero = 0
    Light = 1
    Normal = 2
    Medium = 3
    Strong = 4
    Extreme = 5

    @classmethod
    def parse(cls, s: str) -> "FecMode":
        names = {"0": 0, "zero": 0, "1": 1, "light": 1, "leicht": 1, "2": 2, "normal": 2,
                 "3": 3, "medium": 3, "mittel": 3, "4": 4, "strong": 4, "stark": 4, "5": 5, "extreme": 5}
        try:
            return cls(names[s.lower()])
        except KeyError:
            raise ValueError(f"unknown FEC mode {s!r}") from None


def default_windows() -> dict:
    """FecConfig::default_windows (adaptive.rs:352-362)."""
    return {FecMode.Zero: 0, FecMode.Light: 16, FecMode.Normal: 64, FecMode.Medium: 128,
            FecMode.Strong: 512, FecMode.Extreme: 1024}


@_dataclass
class PidConfig:
    kp: float = 1.2
    ki: float = 0.5
    kd: float = 0.1


@_dataclass
class FecConfig:
    """adaptive.rs:338-349, defaults 435-452."""
    lambda_: float = 0.1
    burst_window: int = 20
    hysteresis: float = 0.02
    pid: PidConfig = _field(default_factory=PidConfig)
    initial_mode: FecMode = FecMode.Zero
    kalman_enabled: bool = False
    kalman_q: float = 0.001
    kalman_r: float = 0.01
    window_sizes: dict = _field(default_factory=default_windows)
    max_len: int = 1500

    def to_c(self) -> "L.FecConfig":
        c = L.FecConfig()
        c.lambda_, c.burst_window, c.hysteresis = self.lambda_, self.burst_window, self.hysteresis
        c.kp, c.ki, c.kd = self.pid.kp, self.pid.ki, self.pid.kd
        c.initial_mode = int(self.initial_mode)
        c.kalman_enabled = 1 if self.kalman_enabled else 0
        c.kalman_q, c.kalman_r = self.kalman_q, self.kalman_r
        for m in FecMode:
            c.window_sizes[int(m)] = int(self.window_sizes.get(m, default_windows()[m]))
        c.max_len = self.max_len
        return c

    def validate(self) -> None:
        """FecConfig::validate (adaptive.rs:455-471)."""
        c = self.to_c()
        check(L._lib().qf_fec_config_validate(ctypes.byref(c)), "FecConfig.validate")


class ModeManager:
    """The static parts of adaptive.rs:102-153."""
    CROSS_FADE_LEN = 32
    ALPHA_K = 0.5

    @staticmethod
    def params_for(mode: FecMode, window: int) -> tuple[int, int]:
        k, n = ctypes.c_uint32(), ctypes.c_uint32()
        check(L._lib().qf_mode_params_for(int(mode), window, ctypes.byref(k), ctypes.byref(n)))
        return k.value, n.value

    @staticmethod
    def window_range(mode: FecMode) -> tuple[int, int]:
        lo, hi = ctypes.c_uint32(), ctypes.c_uint32()
        check(L._lib().qf_mode_window_range(int(mode), ctypes.byref(lo), ctypes.byref(hi)))
        return lo.value, hi.value

    @staticmethod
    def overhead_ratio(mode: FecMode) -> float:
        return L._lib().qf_mode_overhead_ratio(int(mode))


class AdaptiveFec:
    """adaptive.rs:326-631.  `ctx=None` with `codec=False` runs the controller
    alone (no GPU); `now` arguments inject the monotonic clock in seconds."""

    def __init__(self, config: FecConfig, pool: Optional[MemoryPool] = None, *, ctx: Optional[Context] = None,
                 codec: bool = True, now: Optional[float] = None):
        self._lib = L._lib()
        self.config = config
        self.pool = pool
        self.ctx = (ctx or default_context()) if codec else None
        h = ctypes.c_void_p()
        c = config.to_c()
        cptr = self.ctx.handle if self.ctx is not None else None
        if now is None:
            check(self._lib.qf_adaptive_new(cptr, ctypes.byref(c), ctypes.byref(h)), "AdaptiveFec.new")
        else:
            check(self._lib.qf_adaptive_new_at(cptr, ctypes.byref(c), float(now), ctypes.byref(h)),
                  "AdaptiveFec.new")
        self.handle = h

    def state(self) -> dict:
        mode, window, k, n = ctypes.c_int32(), ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        tr, left, est = ctypes.c_int32(), ctypes.c_uint32(), ctypes.c_float()
        check(self._lib.qf_adaptive_state(self.handle, ctypes.byref(mode), ctypes.byref(window), ctypes.byref(k),
                                          ctypes.byref(n), ctypes.byref(tr), ctypes.byref(left), ctypes.byref(est)))
        return {"mode": FecMode(mode.value), "window": window.value, "k": k.value, "n": n.value,
                "transitioning": bool(tr.value), "transition_left": left.value, "estimated_loss": est.value}

    def current_mode(self) -> FecMode:
        return self.state()["mode"]

    def is_transitioning(self) -> bool:
        return self.state()["transitioning"]

    def report_loss(self, lost: int, total: int, now: Optional[float] = None) -> None:
        if now is None:
            check(self._lib.qf_adaptive_report_loss(self.handle, lost, total), "report_loss")
        else:
            check(self._lib.qf_adaptive_report_loss_at(self.handle, lost, total, float(now)), "report_loss")

    def on_send(self, pkt: Packet, outgoing_queue) -> int:
        """Pushes the systematic packet and its repairs onto outgoing_queue.
        Returns the status (QF_ERANGE when the field has no code for the
        configuration -- GF(2^8) with k + r > 256, where the reference panics)."""
        cap = self._lib.qf_adaptive_max_send_packets(self.handle)
        stride = max(self.config.max_len, 1)
        st = self.state()
        kmax = max(256, 2 * st["k"])  # coefficient bytes: k (GF(2^8)) or 2k (GF(2^16), Extreme)
        key = (cap, stride, kmax)
        if getattr(self, "_send_bufs", (None,))[0] != key:   # reused across calls
            self._send_bufs = (key, (ctypes.c_uint8 * (cap * stride))(), (ctypes.c_uint8 * (cap * kmax))(),
                               (L.PacketDesc * cap)())
        _, data, co, desc = self._send_bufs
        n = ctypes.c_uint32()
        pay = pkt.payload()
        buf = (ctypes.c_uint8 * max(1, len(pay))).from_buffer_copy(pay.ljust(max(1, len(pay)), b"\0"))
        s = self._lib.qf_adaptive_on_send(self.handle, pkt.id, buf, len(pay), data, stride, co, kmax, desc, cap,
                                          ctypes.byref(n))
        if s not in (L.QF_OK, L.QF_ERANGE):
            check(s, "on_send")
        mv_d, mv_c = memoryview(data), memoryview(co)
        for i in range(n.value):
            d = desc[i]
            payload = bytearray(mv_d[i * stride: i * stride + d.len])
            coeffs = bytes(mv_c[i * kmax: i * kmax + d.coeff_len]) if not d.is_systematic else None
            outgoing_queue.append(Packet(d.id, payload, d.len, bool(d.is_systematic), coeffs, d.coeff_len))
        return s

    def on_receive(self, pkt: Packet) -> list:
        st = self.state()
        cap = max(1, st["k"] + 1024)
        stride = max(self.config.max_len, 1)
        key = (cap, stride)
        if getattr(self, "_recv_bufs", (None,))[0] != key:   # reused across calls
            self._recv_bufs = (key, (ctypes.c_uint8 * (cap * stride))(), (L.PacketDesc * cap)())
        _, data, desc = self._recv_bufs
        n = ctypes.c_uint32()
        pay = pkt.payload()
        buf = (ctypes.c_uint8 * max(1, len(pay))).from_buffer_copy(pay.ljust(max(1, len(pay)), b"\0"))
        co = None
        if pkt.coefficients is not None:
            co = (ctypes.c_uint8 * max(1, pkt.coeff_len)).from_buffer_copy(
                bytes(pkt.coefficients[: pkt.coeff_len]).ljust(max(1, pkt.coeff_len), b"\0"))
        s = self._lib.qf_adaptive_on_receive(self.handle, pkt.id, 1 if pkt.is_systematic else 0, buf, len(pay),
                                             ctypes.cast(co, ctypes.c_void_p) if co is not None else None,
                                             pkt.coeff_len, data, stride, desc, cap, ctypes.byref(n))
        if s == L.QF_EINVAL and not pkt.is_systematic and pkt.coefficients is None:
            raise QfError(s, "Repair packet missing coefficients.")
        check(s, "on_receive")
        mv = memoryview(data)
        return [Packet(desc[i].id, bytearray(mv[i * stride: i * stride + desc[i].len]), desc[i].len, True)
                for i in range(n.value)]

    def close(self) -> None:
        if getattr(self, "handle", None):
            self._lib.qf_adaptive_free(self.handle)
            self.handle = None

    def __del__(self):  # pragma: no cover
        if _SHUTDOWN:
            return
        try:
            self.close()
        except Exception:
            pass


def on_send_batch(fecs, packets, queues=None):
    """AdaptiveFec.on_send for many connections in one call
    (qf_adaptive_on_send_batch): fecs[m] sends packets[m] (a connection may
    appear more than once; its packets are taken in order).  Appends each
    connection's outgoing packets to queues[m] (new lists when None) and
    returns (queues, statuses) -- the same packets and statuses as calling
    fecs[m].on_send(packets[m], queues[m]) for m in order."""
    M = len(fecs)
    if len(packets) != M:
        raise ValueError("one packet per connection")
    queues = [[] for _ in range(M)] if queues is None else queues
    if M == 0:
        return queues, []
    lib = L._lib()
    cap = sum(lib.qf_adaptive_max_send_packets(f.handle) for f in fecs)
    stride = max(max(f.config.max_len for f in fecs), 1)
    kmax = max(256, max(2 * f.state()["k"] for f in fecs))
    conns = (ctypes.c_void_p * M)(*[f.handle for f in fecs])
    ids = (ctypes.c_uint64 * M)(*[p.id for p in packets])
    pays = [p.payload() for p in packets]
    bufs = [(ctypes.c_uint8 * max(1, len(b))).from_buffer_copy(b.ljust(max(1, len(b)), b"\0")) for b in pays]
    data = (ctypes.c_void_p * M)(*[ctypes.addressof(b) for b in bufs])
    lens = (ctypes.c_uint32 * M)(*[len(b) for b in pays])
    out = (ctypes.c_uint8 * (cap * stride))()
    co = (ctypes.c_uint8 * (cap * kmax))()
    desc = (L.PacketDesc * cap)()
    n_out = (ctypes.c_uint32 * M)()
    st = (ctypes.c_int32 * M)()
    check(lib.qf_adaptive_on_send_batch(conns, M, ids, data, lens, out, stride, co, kmax, desc, cap, n_out, st),
          "on_send_batch")
    mv_d, mv_c = memoryview(out), memoryview(co)
    pos = 0
    for m in range(M):
        for i in range(pos, pos + n_out[m]):
            d = desc[i]
            payload = bytearray(mv_d[i * stride: i * stride + d.len])
            coeffs = bytes(mv_c[i * kmax: i * kmax + d.coeff_len]) if not d.is_systematic else None
            queues[m].append(Packet(d.id, payload, d.len, bool(d.is_systematic), coeffs, d.coeff_len))
        pos += n_out[m]
    return queues, list(st)


def on_receive_batch(fecs, packets):
    """AdaptiveFec.on_receive for many connections in one call
    (qf_adaptive_on_receive_batch): fecs[m] receives packets[m].  Returns
    (recovered, statuses): recovered[m] is the list on_receive would return
    (empty on a per-packet error, whose status is in statuses[m])."""
    M = len(fecs)
    if len(packets) != M:
        raise ValueError("one packet per connection")
    if M == 0:
        return [], []
    lib = L._lib()
    cap = max(1, sum(f.state()["k"] + 1024 for f in fecs))
    stride = max(max(f.config.max_len for f in fecs), 1)
    conns = (ctypes.c_void_p * M)(*[f.handle for f in fecs])
    ids = (ctypes.c_uint64 * M)(*[p.id for p in packets])
    sysf = (ctypes.c_int32 * M)(*[1 if p.is_systematic else 0 for p in packets])
    pays = [p.payload() for p in packets]
    bufs = [(ctypes.c_uint8 * max(1, len(b))).from_buffer_copy(b.ljust(max(1, len(b)), b"\0")) for b in pays]
    data = (ctypes.c_void_p * M)(*[ctypes.addressof(b) for b in bufs])
    lens = (ctypes.c_uint32 * M)(*[len(b) for b in pays])
    cbufs = [None if p.coefficients is None else (ctypes.c_uint8 * max(1, p.coeff_len)).from_buffer_copy(
        bytes(p.coefficients[: p.coeff_len]).ljust(max(1, p.coeff_len), b"\0")) for p in packets]
    co = (ctypes.c_void_p * M)(*[None if c is None else ctypes.addressof(c) for c in cbufs])
    cl = (ctypes.c_uint32 * M)(*[p.coeff_len if p.coefficients is not None else 0 for p in packets])
    out = (ctypes.c_uint8 * (cap * stride))()
    desc = (L.PacketDesc * cap)()
    n_out = (ctypes.c_uint32 * M)()
    st = (ctypes.c_int32 * M)()
    check(lib.qf_adaptive_on_receive_batch(conns, M, ids, sysf, data, lens, co, cl, out, stride, desc, cap, n_out,
                                           st), "on_receive_batch")
    mv = memoryview(out)
    res, pos = [], 0
    for m in range(M):
        res.append([Packet(desc[i].id, bytearray(mv[i * stride: i * stride + desc[i].len]), desc[i].len, True)
                    for i in range(pos, pos + n_out[m])])
        pos += n_out[m]
    return res, list(st)
