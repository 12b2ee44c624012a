"""Speaking-rate stage: a request's audio time-stretched by `speed`, 0.5x to 2x, pitch kept.

Host side, in numpy, importable without a GPU: the definition -- `a()`, `out_len()`, `need()`, `ready()` (the streaming
emission rule), `stretch()` (the reference) and `speed_steps()` (validation of a caller's `speed`).  Device side:
`PcmTempo`, the stateful, chunk-invariant stage of csrc/tempo.hip (qt_tempo) -- one launch per push for all rows, host
counters only, no read-back.  It sits between the codec's PCM and the resampler (`PcmOutput` chains the two, with the
pitch and volume stage of prosody.py, DESIGN §22, between them where a request asks for it).

Definition: WSOLA with an integer-exact search.  x = a row's input (24 kHz fp32, n samples, zero outside [0, n)),
S = round(100 * speed) in [50, 200], a(j) = (j * HS * S) // 100.  The output has out_len(n) = ceil(100 n / S) samples,
in blocks of HS = 240; the last block is cut to out_len.
    block 0:  y[0:HS) = x[0:HS), seg_0 = 0
    block j:  t = seg_{j-1} + HS (where the previous segment would continue);  q = int(rint(clamp(x, -1, 1) * 32767));
              d in [-128, 128) minimises sum_{i < L} |q[a(j) + d + i] - q[t + i]|  (L = 480; candidates with
              a(j) + d < 0 are excluded; ties go to the smallest |d|, then to the negative one);  seg_j = a(j) + d;
              y[j * HS + i] = W0[i] * x[seg_j + i] + W1[i] * x[t + i]  in fp32, W0 a raised-cosine ramp, W1 = 1 - W0.
A row with S = 100 is a verbatim copy.  The sums are integers below 2^25, so every correct implementation picks the same
d.  The candidate range covers one pitch period down to about 94 Hz (24000 / 256); lower voices get a partial search.
"""
from __future__ import annotations

import math

import numpy as np

HS = 240          # output block, 10 ms
L = 480           # similarity length
D_LO, D_HI = -128, 128   # candidates d in [D_LO, D_HI)
HIST = 1024       # input samples of history a row keeps (state)
S_MIN, S_MAX = 50, 200
IN_RATE = 24000

_i = np.arange(HS, dtype=np.float64)
W0 = (0.5 - 0.5 * np.cos(np.pi * (_i + 0.5) / HS)).astype(np.float32)
W1 = (np.float32(1.0) - W0).astype(np.float32)
W0.setflags(write=False)
W1.setflags(write=False)


def a(j: int, S: int) -> int:
    """Nominal input position of block j."""
    return (j * HS * S) // 100


def out_len(n: int, S: int) -> int:
    return -(-100 * n // S)


def need(j: int, S: int) -> int:
    """Input samples that must exist before block j is computed.  Block 0 waits for HS samples, and for as many as
    make out_len reach HS (so that what a stream has handed out never exceeds out_len of its input so far: at
    S > 100 a signal of HS samples is shorter than one block).  Block j >= 1 reads its candidates up to
    a(j) + 127 + L and the continuation t + L, with t = seg_{j-1} + HS <= a(j-1) + 127 + HS: a bound that does not
    need the device's seg, so the host never reads anything back."""
    if j == 0:
        return max(HS, (HS - 1) * S // 100 + 1)
    return max(a(j, S) + D_HI - 1, a(j - 1, S) + D_HI - 1 + HS) + L


def low(j: int, S: int) -> int:
    """The first input sample block j can read (may be negative: zeros)."""
    if j == 0:
        return 0
    return min(a(j, S), a(j - 1, S) + HS) + D_LO


def blocks_ready(S: int, n_total: int, flush: bool = False) -> int:
    """Blocks that exist after n_total input samples (at flush: all of the signal's, the missing future zeros)."""
    if flush:
        return -(-out_len(n_total, S) // HS)
    # a(j) <= n_total - 847 puts every read of block j below n_total: start there, then step by the rule
    j = max(0, (n_total - (D_HI - 1 + HS + L)) * 100 // (HS * S))
    while need(j, S) <= n_total:
        j += 1
    return j


def ready(S: int, n_total: int, flush: bool = False) -> int:
    """Output samples that exist after n_total input samples."""
    if S == 100:
        return n_total
    if flush:
        return out_len(n_total, S)
    return blocks_ready(S, n_total) * HS


def history(S: int, n_total: int) -> int:
    """Input samples before n_total that the first pending block can still read."""
    if S == 100:
        return 0
    return max(0, n_total - max(0, low(blocks_ready(S, n_total), S)))


def check_steps(S) -> int:
    if isinstance(S, bool) or int(S) != S or not S_MIN <= int(S) <= S_MAX:
        raise ValueError(f"speed step must be an integer in [{S_MIN}, {S_MAX}] (hundredths), got {S!r}")
    return int(S)


def numbers(v, n, name, lo, hi, default, span=None):
    """Validate a caller's per-request value `name` -- a number, or one per request -- and return n floats in
    [lo, hi], `default` where an entry is None.  span: how the messages write the range."""
    span = span or f"[{lo:g}, {hi:g}]"
    if isinstance(v, (list, tuple, np.ndarray)):
        vals = list(v)
        if len(vals) != n:
            raise ValueError(f"{name} has {len(vals)} entries for {n} requests")
    else:
        vals = [v] * n
    out = []
    for x in vals:
        if x is None:
            x = default
        if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, float, np.integer, np.floating)):
            raise ValueError(f"{name} must be a number in {span}, got {x!r}")
        x = float(x)
        if not math.isfinite(x) or not lo <= x <= hi:
            raise ValueError(f"{name} must be a finite number in {span}, got {x!r}")
        out.append(x)
    return out


def speed_steps(speed, n):
    """Validate a caller's `speed` -- a number, or one per request -- and return one S = round(100 * speed) per
    request, or None when every entry is 1.0 (no stage is built then)."""
    out = [int(round(100 * v)) for v in numbers(speed, n, "speed", 0.5, 2.0, 1.0, "[0.5, 2.0]")]
    if all(s == 100 for s in out):
        return None
    return out


def quantise(x):
    """q of the definition: int32."""
    x = np.asarray(x, np.float32)
    return np.rint(np.clip(x, np.float32(-1), np.float32(1)) * np.float32(32767)).astype(np.int32)


def stretch(x, S, detail=False):
    """The reference: x (1-D fp32) at speed step S -> y fp32 [out_len].  detail=True: (y, seg, y64, bound) with
    seg[j] the chosen segment starts, y64 the overlap-add in fp64 at those segments and bound[m] =
    3 * 2^-24 * (|W0 a| + |W1 b|), the fp32 evaluation's error bound per sample."""
    S = check_steps(S)
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    n = x.shape[0]
    if S == 100:
        y = x.copy()
        return (y, [], y.astype(np.float64), np.zeros(n)) if detail else y
    n_out = out_len(n, S)
    nb = -(-n_out // HS)
    lo_pad = -D_LO
    top = (a(nb - 1, S) if nb else 0) + D_HI + HS + L + 1
    xp = np.zeros(lo_pad + max(top, n) + L, np.float32)
    xp[lo_pad:lo_pad + n] = x
    qp = quantise(xp)
    y = np.zeros(nb * HS, np.float32)
    y64 = np.zeros(nb * HS, np.float64)
    bound = np.zeros(nb * HS, np.float64)
    segs = []
    w0, w1 = W0.astype(np.float64), W1.astype(np.float64)
    win = np.lib.stride_tricks.sliding_window_view
    for j in range(nb):
        if j == 0:
            segs.append(0)
            y[:HS] = xp[lo_pad:lo_pad + HS]
            y64[:HS] = y[:HS]
            continue
        t = segs[-1] + HS
        aj = a(j, S)
        ref = qp[lo_pad + t:lo_pad + t + L]
        cand = win(qp[lo_pad + aj + D_LO:lo_pad + aj + D_HI - 1 + L], L)   # [256, L]
        score = np.abs(cand - ref[None]).sum(1, dtype=np.int64)
        d = np.arange(D_LO, D_HI)
        key = score * 512 + np.abs(d) * 2 + (d >= 0)
        key[aj + d < 0] = np.iinfo(np.int64).max
        dj = int(d[int(np.argmin(key))])
        seg = aj + dj
        segs.append(seg)
        xa = xp[lo_pad + seg:lo_pad + seg + HS]
        xb = xp[lo_pad + t:lo_pad + t + HS]
        y[j * HS:(j + 1) * HS] = W0 * xa + W1 * xb
        pa, pb = w0 * xa.astype(np.float64), w1 * xb.astype(np.float64)
        y64[j * HS:(j + 1) * HS] = pa + pb
        bound[j * HS:(j + 1) * HS] = 3 * 2.0 ** -24 * (np.abs(pa) + np.abs(pb))
    if detail:
        return y[:n_out], segs, y64[:n_out], bound[:n_out]
    return y[:n_out]


_WINDOWS = {}


def _device_window(device):
    """W0 | W1 on `device`, uploaded once (read-only)."""
    import torch
    key = str(device)
    if key not in _WINDOWS:
        _WINDOWS[key] = torch.from_numpy(np.concatenate([W0, W1])).to(device)
    return _WINDOWS[key]


class PcmTempo:
    """`rows` independent streams through the device time-stretch stage.

    push(src, offsets, lengths, flush, steps) takes row b's next lengths[b] samples from src (fp32 device tensor:
    [rows, L] with offsets into each row, or 1-D with absolute offsets) at speed step steps[b] and returns, per row,
    the outputs that became ready (`ready()`), as views of one fresh fp32 buffer (`self.last` after the call).  Whatever
    the chunking, a row's outputs concatenate to the same bits.  A row keeps its step from its first push to its
    reset(); a flushing row emits the rest of its signal and must be reset() before it takes another."""

    STATE_I64 = HIST // 2 + 1  # a row's state: HIST fp32 of history, then seg as int64

    def __init__(self, rows, device="cuda", start_block=0):
        import torch
        if int(rows) < 1:
            raise ValueError(f"rows must be at least 1, got {rows}")
        if isinstance(start_block, bool) or int(start_block) != start_block or start_block < 0 or start_block % 5:
            raise ValueError(f"start_block must be a non-negative multiple of 5, got {start_block!r}")
        self.rows, self.start_block = int(rows), int(start_block)
        self.window = _device_window(torch.device(device))
        self.device = self.window.device  # with its index: "cuda" -> "cuda:0"
        self.state = torch.zeros(2, self.rows, self.STATE_I64, dtype=torch.int64, device=self.device)
        self.step = [None] * self.rows      # S of the row's signal, fixed by its first push
        self.taken = [0] * self.rows        # input samples taken
        self.given = [0] * self.rows        # output samples handed out
        self.par = [0] * self.rows          # which half of state holds the row's state
        self.fresh = [True] * self.rows     # no state yet
        self.flushed = [False] * self.rows
        self.last = None

    def reset(self, row):
        """Row `row` starts a new signal (host counters only)."""
        self.step[row], self.taken[row], self.given[row] = None, 0, 0
        self.fresh[row], self.flushed[row] = True, False

    def emitted(self, row):
        return self.given[row]

    def push(self, src, offsets, lengths, flush, steps):
        import torch
        from . import kernels as K
        from .resample import check_push, push_views
        B = self.rows
        if isinstance(steps, int):
            steps = [steps] * B
        src, flush, spans = check_push(self, src, offsets, lengths, flush, self.window, steps)
        counts, S = [], [0] * B
        for b, (_, n) in enumerate(spans):
            S[b] = check_steps(steps[b])
            if self.step[b] is not None and S[b] != self.step[b]:
                raise ValueError(f"row {b} runs at step {self.step[b]}: reset() it before it changes to {steps[b]}")
            counts.append(max(0, ready(S[b], self.taken[b] + n, flush[b]) - self.given[b]))
        out = torch.empty(sum(counts), dtype=torch.float32, device=self.device)
        ptrs, outs = push_views(src, spans, out, counts)
        table = []
        sb = self.STATE_I64 * 8
        for b, (_, n) in enumerate(spans):
            a0 = a(self.start_block, S[b])
            st_in = None if self.fresh[b] else self.state.data_ptr() + sb * (self.par[b] * B + b)
            st_out = self.state.data_ptr() + sb * ((self.par[b] ^ 1) * B + b)
            table.append((*ptrs[b], st_in, st_out, a0 + self.taken[b], self.start_block + self.given[b] // HS,
                          self.start_block, n, counts[b], S[b], int(flush[b])))
        K.tempo(self.window, table)
        for b, (_, n) in enumerate(spans):
            if n or counts[b] or flush[b]:
                self.step[b] = S[b]
            if n:
                self.taken[b] += n
                if S[b] != 100:  # (a copying row keeps no state)
                    self.par[b] ^= 1
                    self.fresh[b] = False
            self.given[b] += counts[b]
            self.flushed[b] = self.flushed[b] or flush[b]
        self.last = out
        return outs

    def one_shot(self, x, S):
        """A whole signal (1-D fp32 device tensor) at speed step S, through a state of its own: this stage's streams
        are not touched."""
        t = PcmTempo(1, self.device, self.start_block)
        return t.push(x.float().contiguous().reshape(-1), [0], [x.numel()], True, [S])[0]


class PcmOutput:
    """The output side of a stream with a speaking rate, a pitch or a gain: PcmTempo, then (where a request asks for
    a pitch or a gain) prosody.PcmProsody, then (for another sample rate or format) the PcmResampler,
    behind the interface the routes use for the resampler alone -- rows, reset(row), push(src, offsets, lengths, flush).  At
    most three launches per push for all rows; every stage's counts are its host rule's, so its output feeds the next
    as a 1-D source without a synchronisation."""

    def __init__(self, rows, steps, fmt, device, rs=None):
        """steps: per row its (S, T, db) -- speed step, tempo step and gain (prosody.steps) -- or None: every row at
        (100, 100, 0.0); the pitch stage is built with the first row that has T != S or a gain.  fmt:
        resample.output_format()'s (Plan, pcm_format) or None; rs: a PcmResampler of that format to go on with (its
        rows keep their state) instead of a new one."""
        from .resample import PcmResampler
        self.rows = int(rows)
        self.tempo = PcmTempo(rows, device)
        if rs is None and fmt is not None:
            rs = PcmResampler(rows, fmt[0].sample_rate, fmt[1], fmt[0].in_rate, device)
        self.rs = rs
        self.steps = [100] * self.rows    # S: what the output's length follows
        self.tsteps = [100] * self.rows   # the steps the tempo stage runs at: T of prosody.py, S without a pitch
        self.pro = None
        for b, st in enumerate(steps or ()):
            self._step(b, st)

    def _step(self, row, step):
        S, T, db = step
        self.steps[row], self.tsteps[row] = check_steps(S), check_steps(T)
        if self.pro is None:
            if T == S and db == 0:
                return
            from .prosody import PcmProsody
            # (rows under way are copied from here on: a row at T == S and 0 dB passes what it takes)
            self.pro = PcmProsody(self.rows, self.tempo.device)
        self.pro.reset(row, T, S, db)

    def reset(self, row, step=(100, 100, 0.0)):
        self.tempo.reset(row)
        if self.rs is not None:
            self.rs.reset(row)
        self._step(row, step)

    def push(self, src, offsets, lengths, flush):
        if isinstance(flush, bool):
            flush = [flush] * self.rows
        outs = self.tempo.push(src, offsets, lengths, flush, self.tsteps)
        last = self.tempo.last
        if self.pro is not None:
            # a request of N samples yields out_len(N, S) whatever its pitch: the cut at flush
            caps = [out_len(self.tempo.taken[b], self.steps[b]) if flush[b] else None for b in range(self.rows)]
            outs = self.pro.push(last, *self._spans(outs), flush, caps)
            last = self.pro.last
        if self.rs is None:
            return outs
        return self.rs.push(last, *self._spans(outs), flush)

    @staticmethod
    def _spans(outs):
        offs, at = [], 0
        for o in outs:
            offs.append(at)
            at += o.numel()
        return offs, [o.numel() for o in outs]
