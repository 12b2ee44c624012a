"""Pitch and volume stage: a request's audio shifted by `pitch` semitones and scaled by `volume_gain_db`,
with a look-ahead peak limiter on the rows whose gain is positive.

Host side, in numpy, importable without a GPU: the definition -- `steps()` (validation and quantisation of a caller's
speed / pitch / volume_gain_db), `plan()` (the per-request filter), `ready()` (the streaming emission rule), `limit()`
and `apply()` (the reference).  Device side: `PcmProsody`, the stateful, chunk-invariant stage of csrc/prosody.hip
(qt_prosody) -- one launch per push for all rows, each row with its own ratio, host counters only, no read-back.  It
sits between the tempo stage and the resampler (`tempo.PcmOutput` chains the three).

Pitch is resampling pitch: the tempo stage runs the request at step T = floor(S / 2^(pitch/12) + 0.5) instead of
S = round(100 * speed), and this stage resamples its output by U/D = T/S (lowest terms).  The duration is the one at
`speed`, the realised pitch ratio is exactly S/T (`realised_cents`), and formants move with the pitch.

Definition (x = a row's input, n samples; h = plan(T, S).h; g = fp32(10^(db/20))): for m in [0, ceil(n*U/D))
    acc[m] = sum_k x[k] * h[m*D - k*U + half]    over the k whose tap index lies in [0, 2*half], x zero outside,
             fp32, fmaf over k ascending (U == D: acc = x)
    v[m]   = g * acc[m]                          a separate fp32 multiply
and on a limited row (db > 0), with LA = 128, all of it exact:
    r[m]   = 1 / |v[m]| where |v[m]| > 1 (correctly rounded fp32), else 1
    rq[m]  = floor(r[m] * 2^24), 2^24 outside the signal
    mn[m]  = min(rq[m .. m+LA-1]);   sm[m] = sum(mn[m-LA+1 .. m]) <= 2^31
    s[m]   = min(fp32(sm[m]) * 2^-31, r[m]);   y[m] = v[m] * s[m]
Every window of sm[m] holds rq[m], so s <= r and |y| <= 1.0 exactly; an idle limiter has s = 1.0 and y = v bit for bit.
The output is cut to `cap` samples (the caller's ceil(100 N / S)); the limiter runs over the uncut signal.
"""
from __future__ import annotations

import math
from collections import OrderedDict
from dataclasses import dataclass
from fractions import Fraction
from functools import lru_cache

import numpy as np

from . import resample as _rs
from . import tempo as _tempo

LA = 128            # limiter look-ahead window
HIST = 1152         # input samples of history a row keeps (state): 254 outputs back at D/U = 4, and the taps
MAX_Q = 200
PITCH_MIN, PITCH_MAX = -12.0, 12.0
DB_MIN, DB_MAX = -96.0, 16.0
TABLE_CACHE = 64    # device tables kept, least recently used out first
ONE = 1 << 24


@dataclass(frozen=True)
class Plan:
    T: int
    S: int
    up: int
    down: int
    half: int
    taps: int           # taps per output = columns of `table`
    h: np.ndarray       # fp32 [2*half + 1]
    table: np.ndarray   # fp32 [up][taps], phase-major

    def out_len(self, n: int) -> int:
        return -(-n * self.up // self.down)


@lru_cache(maxsize=None)
def _ratio_plan(up, down):
    return _rs.filter_taps(up, down)


def plan(T, S) -> Plan:
    """The filter that resamples the tempo stage's output at step T back to the duration at step S: U/D = T/S."""
    T, S = _tempo.check_steps(T), _tempo.check_steps(S)
    fr = Fraction(T, S)
    return Plan(T, S, fr.numerator, fr.denominator, *_ratio_plan(fr.numerator, fr.denominator))


def gain(db) -> np.float32:
    return np.float32(10.0 ** (float(db) / 20.0))


def realised_cents(S, T) -> float:
    """The pitch a request at speed step S gets when its tempo step is T."""
    return 1200.0 * math.log2(S / T)


def tempo_step(S, pitch) -> int:
    """T of the definition; ValueError when it leaves the tempo stage's range."""
    T = int(math.floor(S / 2.0 ** (pitch / 12.0) + 0.5))
    if not _tempo.S_MIN <= T <= _tempo.S_MAX:
        raise ValueError(f"speed divided by the pitch ratio must lie in [0.5, 2.0]: speed {S / 100:g} at pitch "
                         f"{pitch:g} semitones needs the tempo step {T / 100:g}")
    return T


def steps(speed, pitch, volume_gain_db, n):
    """Validate a caller's speed, pitch (semitones) and volume_gain_db -- each a number, or one per request -- and
    return one (S, T, db) per request: S = round(100 * speed), T the tempo step, db the gain.  None when every
    request is at 1.0 / 0 / 0 (no stage is built then)."""
    S = _tempo.speed_steps(1.0 if speed is None else speed, n) or [100] * n
    p = _tempo.numbers(pitch, n, "pitch", PITCH_MIN, PITCH_MAX, 0.0)
    db = _tempo.numbers(volume_gain_db, n, "volume_gain_db", DB_MIN, DB_MAX, 0.0)
    out = [(s, tempo_step(s, pi), d) for s, pi, d in zip(S, p, db)]
    if all(o == (100, 100, 0.0) for o in out):
        return None
    return out


def ready(p: Plan, limited: bool, n_total: int, flush: bool = False, cap=None) -> int:
    """Output samples that exist after n_total input samples: resample.ready's count at U/D (a row with U == D needs
    x[m] alone for y[m]: n_total), less LA - 1 on a limited row; at flush the natural length, cut to cap."""
    if flush:
        top = p.out_len(n_total)
        return top if cap is None else min(top, int(cap))
    base = n_total if p.up == p.down else _rs.ready(p, n_total)
    return max(0, base - (LA - 1 if limited else 0))


def limit(v):
    """The limiter of the definition on a whole signal v (fp32)."""
    v = np.ascontiguousarray(v, np.float32)
    n = v.shape[0]
    if n == 0:
        return v.copy()
    av = np.abs(v)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(av > np.float32(1), np.float32(1) / av, np.float32(1)).astype(np.float32)
    rq = np.full(n + 2 * (LA - 1), ONE, np.int64)
    rq[LA - 1:LA - 1 + n] = np.floor(r.astype(np.float64) * ONE).astype(np.int64)
    win = np.lib.stride_tricks.sliding_window_view
    mn = win(rq, LA).min(-1)             # mn[i] <-> m = i - (LA - 1), for m in [-(LA-1), n)
    sm = win(mn, LA).sum(-1)             # sm[m] = sum mn[m-LA+1 .. m], m in [0, n)
    s = np.minimum(sm.astype(np.float32) * np.float32(2.0 ** -31), r)
    return (v * s).astype(np.float32)


def _resample32(x, p: Plan):
    """acc of the definition: fp32, fmaf over k ascending (each fmaf as one fp64 multiply-add rounded to fp32; the
    product is exact in fp64, so this is the device's value except where the second rounding falls on a tie)."""
    n = x.shape[0]
    M = p.out_len(n)
    c = np.arange(M, dtype=np.int64) * p.down + p.half
    k_hi = c // p.up
    row = p.table[(c - k_hi * p.up)]     # [M, taps]
    acc = np.zeros(M, np.float32)
    xz = np.concatenate([x, np.zeros(1, np.float32)]).astype(np.float64)
    for j in range(p.taps - 1, -1, -1):
        k = k_hi - j
        xk = xz[np.where((k >= 0) & (k < n), k, n)]
        acc = (xk * row[:, j].astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
    return acc


def apply(x, T, S, db, cap=None):
    """The reference, one-shot: x (1-D fp32, the tempo stage's output at step T) -> y fp32, cut to cap."""
    p = plan(T, S)
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    g = gain(db)
    acc = x if p.up == p.down else _resample32(x, p)
    v = (g * acc).astype(np.float32)
    y = limit(v) if db > 0 else v
    return y.copy() if cap is None else y[:int(cap)].copy()


_TABLES = OrderedDict()


def _device_table(p: Plan, device):
    """The plan's taps on `device` (read-only), from a cache of the TABLE_CACHE ratios used last.  A row keeps a
    reference to its table, so a table that leaves the cache lives on while a row still runs at it."""
    import torch
    key = (p.up, p.down, str(device))
    t = _TABLES.pop(key, None)
    if t is None:
        t = torch.from_numpy(p.table.copy()).to(device)
    _TABLES[key] = t
    while len(_TABLES) > TABLE_CACHE:
        _TABLES.popitem(last=False)
    return t


class PcmProsody:
    """`rows` independent streams through the device pitch and volume stage.

    reset(row, T, S, db) sets a row's ratio and gain; push(src, offsets, lengths, flush, cap) takes row b's next
    lengths[b] samples from src (fp32 device tensor: [rows, L] with offsets into each row, or 1-D with absolute
    offsets) and returns, per row, the outputs that became ready (`ready()`), as views of one fresh fp32 buffer
    (`self.last` after the call).  Whatever the chunking, a row's outputs concatenate to the same bits.  A flushing row
    emits the rest of its signal, cut to cap[b] samples in all, and must be reset() before it takes another.
    start_period: the rows' signals start at input position start_period * D (output start_period * U)."""

    def __init__(self, rows, device="cuda", start_period=0):
        import torch
        if int(rows) < 1:
            raise ValueError(f"rows must be at least 1, got {rows}")
        if isinstance(start_period, bool) or int(start_period) != start_period or start_period < 0:
            raise ValueError(f"start_period must be a non-negative integer, got {start_period!r}")
        self.rows, self.start_period = int(rows), int(start_period)
        self.state = torch.zeros(2, self.rows, HIST, dtype=torch.float32, device=device)
        self.device = self.state.device  # with its index: "cuda" -> "cuda:0"
        unit = plan(100, 100)
        self.plan = [unit] * self.rows
        self.table = [_device_table(unit, self.device)] * self.rows
        self.db = [0.0] * self.rows
        self.taken = [0] * self.rows        # input samples taken
        self.given = [0] * self.rows        # output samples handed out
        self.par = [0] * self.rows          # which half of state holds the row's history
        self.fresh = [True] * self.rows     # no history yet: zeros
        self.flushed = [False] * self.rows
        self.last = None

    def reset(self, row, T=None, S=None, db=None):
        """Row `row` starts a new signal (host counters only), at the ratio T/S and the gain db where given."""
        if (T is None) != (S is None):
            raise ValueError("reset() takes T and S together")
        if T is not None:
            self.plan[row] = plan(T, S)
            self.table[row] = _device_table(self.plan[row], self.device)
        if db is not None:
            self.db[row] = _tempo.numbers(db, 1, "volume_gain_db", DB_MIN, DB_MAX, 0.0)[0]
        self.taken[row], self.given[row] = 0, 0
        self.fresh[row], self.flushed[row] = True, False

    def emitted(self, row):
        return self.given[row]

    def push(self, src, offsets, lengths, flush, cap=None):
        import torch
        from . import kernels as K
        if cap is None:
            cap = [None] * self.rows
        src, flush, spans = _rs.check_push(self, src, offsets, lengths, flush, self.state[0, 0], cap)
        counts = []
        for b, (_, n) in enumerate(spans):
            if cap[b] is not None and int(cap[b]) < 0:
                raise ValueError(f"row {b}: cap must not be negative, got {cap[b]}")
            counts.append(max(0, ready(self.plan[b], self.db[b] > 0, self.taken[b] + n, flush[b], cap[b])
                              - self.given[b]))
        out = torch.empty(sum(counts), dtype=torch.float32, device=self.device)
        ptrs, outs = _rs.push_views(src, spans, out, counts)
        table = []
        for b, (_, n) in enumerate(spans):
            p = self.plan[b]
            st_in = None if self.fresh[b] else self.state[self.par[b], b].data_ptr()
            st_out = self.state[self.par[b] ^ 1, b].data_ptr()
            pos0, m_start = self.start_period * p.down, self.start_period * p.up
            table.append((*ptrs[b], st_in, st_out, self.table[b].data_ptr(), pos0 + self.taken[b],
                          m_start + self.given[b], pos0, -1 if cap[b] is None else int(cap[b]), n, counts[b], p.up,
                          p.down, p.half, p.taps, float(gain(self.db[b])), int(self.db[b] > 0), int(flush[b])))
        K.prosody(table)
        for b, (_, n) in enumerate(spans):
            if n:
                self.taken[b] += n
                self.par[b] ^= 1
                self.fresh[b] = False
            self.given[b] += counts[b]
            self.flushed[b] = self.flushed[b] or flush[b]
        self.last = out
        return outs

    def one_shot(self, x, T, S, db, cap=None):
        """A whole signal (1-D fp32 device tensor) at the ratio T/S and the gain db, through a state of its own: this
        stage's streams are not touched."""
        t = PcmProsody(1, self.device, self.start_period)
        t.reset(0, T, S, db)
        return t.push(x.float().contiguous().reshape(-1), [0], [x.numel()], True, [cap])[0]
