"""PCM output stage: audio at the caller's sample rate, as f32 or s16.

Host side, importable without a GPU: `plan()` (the filter, fp64 in numpy, stored fp32 phase-major) and `ready()` (the
streaming emission rule).  Device side: `PcmResampler`, the stateful, chunk-invariant polyphase resampler of
csrc/resample.hip (qt_resample) -- one launch per push for all rows, host counters only, no read-back.

Definition (x = a row's input, n samples at in_rate; h = the fp32 taps): for m in [0, ceil(n*up/down))
    y[m] = sum_k x[k] * h[m*down - k*up + half]      over the k whose tap index lies in [0, 2*half],
x outside [0, n) zero.  h is scipy.signal.resample_poly's default filter (firwin(2*half+1, 1/q, kaiser 5.0) * up),
so y is resample_poly(x, up, down) up to rounding.
"""
from __future__ import annotations

from dataclasses import dataclass
from fractions import Fraction
from functools import lru_cache

import numpy as np

IN_RATE = 24000
MAX_Q = 160
FORMATS = ("f32", "s16")


@dataclass(frozen=True)
class Plan:
    sample_rate: int
    in_rate: int
    up: int
    down: int
    half: int
    taps: int           # taps per output = columns of `table`
    h: np.ndarray       # fp32 [2*half + 1]: these values define the resampler
    table: np.ndarray   # fp32 [up][taps], phase-major: table[p][j] = h[p + j*up], 0 past the filter's end

    def out_len(self, n: int) -> int:
        return -(-n * self.up // self.down)

    def ready(self, n_total: int, flush: bool = False) -> int:
        return ready(self, n_total, flush)


@lru_cache(maxsize=None)
def plan(sample_rate, in_rate=IN_RATE) -> Plan:
    if isinstance(sample_rate, bool) or int(sample_rate) != sample_rate or int(in_rate) != in_rate:
        raise ValueError(f"sample rates must be integers, got {sample_rate!r} from {in_rate!r}")
    sample_rate, in_rate = int(sample_rate), int(in_rate)
    if sample_rate <= 0 or in_rate <= 0:
        raise ValueError(f"sample rates must be positive, got {sample_rate} from {in_rate}")
    fr = Fraction(sample_rate, in_rate)
    up, down = fr.numerator, fr.denominator
    q = max(up, down)
    if q > MAX_Q:
        raise ValueError(f"sample_rate {sample_rate} from {in_rate} Hz is the ratio {up}/{down}: ratios above "
                         f"{MAX_Q} are not served (8000, 12000, 16000, 22050, 32000, 44100 and 48000 are)")
    return Plan(sample_rate, in_rate, up, down, *filter_taps(up, down))


def filter_taps(up: int, down: int):
    """(half, taps, h, table) of the ratio up/down in lowest terms: the filter every stage that resamples shares
    (the pitch stage of prosody.py builds its per-request filters here too)."""
    q = max(up, down)
    half = 10 * q
    j = np.arange(2 * half + 1, dtype=np.float64)
    h = np.kaiser(2 * half + 1, 5.0) * np.sinc((j - half) / q)
    if q == 1:  # sinc at the other integers is zero, not numpy's 4e-17: the single tap 1.0, an exact conversion
        h = (j == half).astype(np.float64)
    h = (h / h.sum() * up).astype(np.float32)
    taps = -(-(2 * half + 1) // up)
    table = np.zeros(up * taps, np.float32)
    table[:2 * half + 1] = h                      # [taps][up] ...
    table = np.ascontiguousarray(table.reshape(taps, up).T)  # ... -> [up][taps]
    h.setflags(write=False)
    table.setflags(write=False)
    return half, taps, h, table


def ready(p: Plan, n_total: int, flush: bool = False) -> int:
    """Outputs that exist after n_total input samples: those whose inputs all lie below n_total; at flush the missing
    future is zero and every output of the signal exists."""
    top = -(-n_total * p.up // p.down)
    if flush:
        return top
    return max(0, min((n_total * p.up - 1 - p.half) // p.down + 1, top))


def output_format(sample_rate, pcm_format, in_rate=IN_RATE):
    """Validate a caller's (sample_rate, pcm_format); None when it is the default output (in_rate, f32), which runs
    no resampler, else (Plan, pcm_format)."""
    if pcm_format not in FORMATS:
        raise ValueError(f"pcm_format must be one of {FORMATS}, got {pcm_format!r}")
    if sample_rate is None:
        sample_rate = in_rate
    p = plan(sample_rate, in_rate)
    if p.up == p.down and pcm_format == "f32":
        return None
    return p, pcm_format


_TABLES = {}


def _device_table(p: Plan, device):
    """The plan's taps on `device`, uploaded once (read-only: every resampler of that format shares them)."""
    import torch
    key = (p.sample_rate, p.in_rate, str(device))
    if key not in _TABLES:
        _TABLES[key] = torch.from_numpy(p.table.copy()).to(device)
    return _TABLES[key]


def check_push(stage, src, offsets, lengths, flush, standin, *more):
    """What the push() of every stateful stage checks first (PcmResampler, tempo.PcmTempo, prosody.PcmProsody; `stage`
    has rows, device and flushed).  flush: one bool per row, or one for all; more: the stage's further per-row lists;
    src None: a call that only flushes, which takes no samples and reads `standin`, a tensor of the stage's.  Returns
    (src, flush as a list of bools, [(offset, length)] per row)."""
    import torch
    B = stage.rows
    if isinstance(flush, bool):
        flush = [flush] * B
    if any(len(v) != B for v in (offsets, lengths, flush) + more):
        raise ValueError(f"push() takes one entry per row in each of its lists ({B} rows)")
    if src is None:
        if any(lengths):
            raise ValueError("push(None, ...) takes no samples")
        src = standin
    if src.dtype != torch.float32 or src.device != stage.device or src.dim() not in (1, 2) or \
            (src.numel() and src.stride(-1) != 1):
        raise ValueError("push() takes an fp32 tensor on the stage's device, 1-D or [rows, L], unit stride")
    if src.dim() == 2 and src.shape[0] != B:
        raise ValueError(f"push() takes [rows, L] with rows = {B}, got {tuple(src.shape)}")
    span, spans = src.shape[-1], []
    for b in range(B):
        o, n = int(offsets[b]), int(lengths[b])
        if n < 0 or o < 0 or (n and o + n > span):
            raise ValueError(f"row {b}: samples [{o}, {o + n}) lie outside the source's {span}")
        if n and stage.flushed[b]:
            raise ValueError(f"row {b} was flushed: reset() it before its next signal")
        spans.append((o, n))
    return src, [bool(f) for f in flush], spans


def push_views(src, spans, out, counts):
    """Where a push reads and writes: per row (address of its first source sample, or None where it takes none;
    address of its first output in `out`, or None where it gets none), and the rows' views of `out`, back to back."""
    base, esz = src.data_ptr(), out.element_size()
    stride = src.stride(0) if src.dim() == 2 else 0
    ptrs, outs, at = [], [], 0
    for b, ((o, n), c) in enumerate(zip(spans, counts)):
        ptrs.append((base + 4 * (b * stride + o) if n else None, out.data_ptr() + esz * at if c else None))
        outs.append(out[at:at + c])
        at += c
    return ptrs, outs


class PcmResampler:
    """`rows` independent streams through one device resampler.

    push(src, offsets, lengths, flush) takes row b's next lengths[b] samples from src (fp32 device tensor: [rows, L]
    with offsets into each row, or 1-D with absolute offsets) and returns, per row, the outputs that became ready
    (`ready()`), as fresh tensors.  Whatever the chunking, a row's outputs concatenate to the same bits.  A flushing
    row emits the rest of its signal and must be reset() before it takes another."""

    def __init__(self, rows, sample_rate, pcm_format="f32", in_rate=IN_RATE, device="cuda", start_pos=0):
        import torch
        if pcm_format not in FORMATS:
            raise ValueError(f"pcm_format must be one of {FORMATS}, got {pcm_format!r}")
        self.plan = p = plan(sample_rate, in_rate)
        if int(rows) < 1:
            raise ValueError(f"rows must be at least 1, got {rows}")
        if start_pos < 0 or start_pos % p.down:
            raise ValueError(f"start_pos must be a non-negative multiple of down = {p.down}, got {start_pos}")
        self.rows, self.pcm_format, self.device = int(rows), pcm_format, torch.device(device)
        self.dtype = torch.int16 if pcm_format == "s16" else torch.float32
        self.H = p.taps
        self.table = _device_table(p, self.device)
        self.device = self.table.device  # with its index: "cuda" -> "cuda:0"
        self.hist = torch.zeros(2, self.rows, self.H, dtype=torch.float32, device=self.device)
        self.start_pos = int(start_pos)
        self.pos = [self.start_pos] * self.rows                        # input samples taken
        self.m0 = [self.start_pos // p.down * p.up] * self.rows        # outputs handed out
        self.par = [0] * self.rows                                     # which half of hist holds the row's history
        self.fresh = [True] * self.rows                                # no history yet: zeros
        self.flushed = [False] * self.rows

    def reset(self, row):
        """Row `row` starts a new signal (host counters only: its history counts as zeros)."""
        self.pos[row], self.m0[row] = self.start_pos, self.start_pos // self.plan.down * self.plan.up
        self.fresh[row], self.flushed[row] = True, False

    def emitted(self, row):
        return self.m0[row] - self.start_pos // self.plan.down * self.plan.up

    def push(self, src, offsets, lengths, flush):
        import torch
        from . import kernels as K
        p = self.plan
        src, flush, spans = check_push(self, src, offsets, lengths, flush, self.table.view(-1))
        counts = [max(0, ready(p, self.pos[b] + n - self.start_pos, flush[b]) - self.emitted(b))
                  for b, (_, n) in enumerate(spans)]
        out = torch.empty(sum(counts), dtype=self.dtype, device=self.device)
        ptrs, outs = push_views(src, spans, out, counts)
        table = []
        for b, (_, n) in enumerate(spans):
            hin = None if self.fresh[b] else self.hist[self.par[b], b].data_ptr()
            table.append((*ptrs[b], hin, self.hist[self.par[b] ^ 1, b].data_ptr(), self.pos[b], self.m0[b], n,
                          counts[b], int(flush[b])))
        K.resample(self.table, p.up, p.down, p.half, p.taps, self.H, self.pcm_format, table)
        for b, (_, n) in enumerate(spans):
            if n:
                self.pos[b] += n
                self.par[b] ^= 1
                self.fresh[b] = False
            self.m0[b] += counts[b]
            self.flushed[b] = self.flushed[b] or flush[b]
        return outs

    def one_shot(self, x, lengths=None):
        """A whole signal (1-D -> one tensor) or a batch of them ([B, L], row b's first lengths[b] samples -> a list),
        through a state of its own: this resampler's streams are not touched."""
        single = x.dim() == 1
        x2 = x[None] if single else x
        n = x2.shape[0]
        t = PcmResampler.__new__(PcmResampler)
        t.__dict__.update(self.__dict__)
        t.rows, t.hist = n, self.hist.new_zeros(2, n, self.H)
        t.pos, t.m0 = [self.start_pos] * n, [self.start_pos // self.plan.down * self.plan.up] * n
        t.par, t.fresh, t.flushed = [0] * n, [True] * n, [False] * n
        outs = t.push(x2.float().contiguous(), [0] * n, [x2.shape[1]] * n if lengths is None else list(lengths), True)
        return outs[0] if single else outs
