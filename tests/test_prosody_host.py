"""Pitch and volume stage, host side (qwen_tts/prosody.py): validation and quantisation of `pitch` and
`volume_gain_db`, the per-request filter, the emission rule, the length rule and the numpy limiter.  No GPU."""
import math
from fractions import Fraction

import numpy as np
import pytest

import resample_refs as RR
from qwen_tts import prosody as P
from qwen_tts import resample as RS

RATIOS = ((50, 100), (200, 100), (94, 100), (101, 199), (50, 200))  # T, S: 1/2, 2/1, 47/50, 101/199, 1/4


def test_validation_and_broadcast():
    assert P.steps(None, None, None, 3) is None
    assert P.steps(1.0, 0, 0.0, 2) is None
    assert P.steps([1.0, 1], [0, 0.0], [0, -0.0], 2) is None
    assert P.steps(1.25, None, None, 2) == [(125, 125, 0.0)] * 2
    assert P.steps(None, [0, 12, -12], 6, 3) == [(100, 100, 6.0), (100, 50, 6.0), (100, 200, 6.0)]
    assert P.steps(None, np.float32(3), np.int64(-6), 1) == [(100, 84, -6.0)]
    bad = (float("nan"), float("inf"), True, False, "high", [0, 1], [0, True, 0])
    for v in bad + (12.01, -12.01):
        with pytest.raises(ValueError):
            P.steps(None, v, None, 3)
    for v in bad + (16.01, -96.01):
        with pytest.raises(ValueError):
            P.steps(None, None, v, 3)
    with pytest.raises(ValueError):
        P.steps(None, [], None, 1)
    with pytest.raises(ValueError):
        P.steps(2.5, 3, None, 1)  # speed is still checked


def test_pitch_zero_keeps_the_speed_step():
    for S in range(50, 201):
        assert P.tempo_step(S, 0) == S and P.tempo_step(S, 0.0) == S
        assert P.steps(S / 100, 0, 0, 1) == (None if S == 100 else [(S, S, 0.0)])


def test_tempo_step_out_of_range():
    for speed, pitch in ((0.5, 1), (2.0, -1), (0.6, 6), (1.9, -3)):
        with pytest.raises(ValueError, match=r"speed divided by the pitch ratio must lie in \[0.5, 2.0\]"):
            P.steps(speed, pitch, None, 1)
    assert P.steps(1.0, 12, None, 1) == [(100, 50, 0.0)] and P.steps(1.0, -12, None, 1) == [(100, 200, 0.0)]


def test_realised_pitch_and_plan_bounds():
    """Every (S, pitch in 5-cent steps) whose T is in range: the realised pitch is within 17.5 cents of the request;
    every ratio's filter fits the kernel's limits."""
    worst, ratios = 0.0, set()
    for S in range(50, 201):
        for c in range(-1200, 1201, 5):
            T = int(math.floor(S / 2.0 ** (c / 1200) + 0.5))
            if not 50 <= T <= 200:
                continue
            worst = max(worst, abs(P.realised_cents(S, T) - c))
            ratios.add(Fraction(T, S))
    assert worst <= 17.5, worst
    for S in range(50, 201):
        for T in range(50, 201):
            ratios.add(Fraction(T, S))
    assert len(ratios) == 16655
    for fr in ratios:
        U, D = fr.numerator, fr.denominator
        q = max(U, D)
        taps = -(-(20 * q + 1) // U)
        assert q <= P.MAX_Q and taps <= 81 and U * taps <= 4200
        # a limited tile's input span (510 outputs) and the history a limited row reaches back (254 outputs + taps)
        assert -(-509 * D // U) + taps <= 2128
        assert 254 * D // U + taps + 2 <= P.HIST


def test_filter_is_the_resamplers():
    p = P.plan(100, 150)
    q = RS.plan(16000)
    assert (p.up, p.down, p.half, p.taps) == (2, 3, q.half, q.taps)
    assert p.h.dtype == np.float32 and np.array_equal(p.h.view(np.int32), q.h.view(np.int32))
    assert np.array_equal(p.table.view(np.int32), q.table.view(np.int32))
    unit = P.plan(137, 137)
    assert (unit.up, unit.down) == (1, 1) and unit.h[unit.half] == 1.0 and np.count_nonzero(unit.h) == 1


@pytest.mark.parametrize("T,S", RATIOS)
def test_ready_is_the_brute_force_count(T, S):
    p = P.plan(T, S)
    top = 700
    last = RR.last_needed(p, p.out_len(top) + 1)
    for n in list(range(0, 260)) + [top - 1, top]:
        want = RR.brute_ready(p, n, last)
        assert P.ready(p, False, n) == want, n
        assert P.ready(p, True, n) == max(0, want - 127), n
        assert P.ready(p, False, n, flush=True) == P.ready(p, True, n, flush=True) == p.out_len(n)
        assert P.ready(p, True, n, flush=True, cap=5) == min(5, p.out_len(n))


def test_unit_ratio_holds_nothing_back():
    p = P.plan(80, 80)
    assert P.ready(p, False, 777) == 777 and P.ready(p, True, 777) == 650 and P.ready(p, True, 100) == 0


def test_natural_length_exceeds_the_cap_by_at_most_4():
    worst = 0
    for S in range(50, 201):
        for T in range(50, 201):
            fr = Fraction(T, S)
            U, D = fr.numerator, fr.denominator
            for N in list(range(0, 40)) + [1365, 1366, 5999, 6000, 24001, 100003]:
                cap = -(-100 * N // S)
                nat = -(-(-(-100 * N // T)) * U // D)
                assert nat >= cap, (S, T, N)
                worst = max(worst, nat - cap)
    assert worst <= 4, worst


def _square(n, period=300):
    return np.where((np.arange(n) // (period // 2)) % 2 == 0, 1.0, -1.0).astype(np.float32)


def _limiter_properties(x, db):
    g = P.gain(db)
    v = (g * x).astype(np.float32)
    y = P.apply(x, 100, 100, db)
    assert y.dtype == np.float32 and y.shape == v.shape
    assert np.abs(y).max() <= 1.0
    over = np.abs(v) > 1.0
    assert over.any()
    near = np.convolve(over.astype(np.int64), np.ones(2 * P.LA - 1, np.int64), "same") > 0  # +-127 around a peak
    assert (~near).any() or db == 6
    assert np.array_equal(y[~near].view(np.int32), v[~near].view(np.int32))
    return y, v, near


def test_limiter_on_noise_and_on_a_square_wave():
    rng = np.random.default_rng(5)
    x = (rng.standard_normal(6000) * 0.3).astype(np.float32)
    x[2000:3000] *= 0.01  # a stretch the limiter leaves alone
    y, v, near = _limiter_properties(x, 16)
    assert (~near).sum() >= 700
    y, v, near = _limiter_properties(_square(3000), 6)
    # a +-1 square wave at +6 dB is over everywhere: the limiter settles at exactly 1 / g
    assert near.all() and np.abs(y[200:-200]).max() <= 1.0 and np.abs(y[200:-200]).min() > 0.99


def test_idle_limiter_and_plain_gain_are_exact():
    rng = np.random.default_rng(6)
    x = (rng.standard_normal(1000) * 0.05).astype(np.float32)
    for db in (6.0, 0.0, -6.0):
        want = (P.gain(db) * x).astype(np.float32)
        assert np.array_equal(P.apply(x, 100, 100, db).view(np.int32), want.view(np.int32))
    assert np.array_equal(P.apply(x, 93, 93, 0).view(np.int32), x.view(np.int32))
    assert P.apply(x, 94, 100, 0, cap=7).shape == (7,)


def test_reference_resampler_matches_fp64():
    """apply()'s fp32 sum against the fp64 sum of the same taps: each of the `taps` fmaf and the gain's multiply
    rounds once, by at most 2^-24 of a partial sum that sum |x h| bounds -- (taps + 1) * 2^-24 * g * sum |x h|."""
    import torch
    rng = np.random.default_rng(8)
    x = (rng.standard_normal(777) * 0.3).astype(np.float32)
    for T, S in RATIOS:
        p = P.plan(T, S)
        got = P.apply(x, T, S, -6.0).astype(np.float64)
        ref = float(P.gain(-6.0)) * RR.resample(torch.from_numpy(x), p).numpy()
        scale = float(P.gain(-6.0)) * RR.resample_scale(torch.from_numpy(x), p).numpy()
        assert got.shape == ref.shape == (p.out_len(777),)
        assert (np.abs(got - ref) <= (p.taps + 1) * 2.0 ** -24 * scale).all(), (T, S)


def test_abi_refuses_a_wrong_row_table():
    """qt_prosody checks every row against the emission rule before it launches: a count that is not the rule's, a
    filter that is not the ratio's, a state buffer used as both input and output, a start that is no multiple of down
    or a continuing row without state is refused (no GPU needed: nothing is launched)."""
    import ctypes
    from qwen_tts import _hip
    lib = _hip.load_library()
    p = P.plan(94, 100)  # 47/50

    def call(count, n=1365, pos=0, m0=0, pos0=0, cap=-1, up=p.up, down=p.down, half=p.half, taps=p.taps, lim=0,
             flush=0, sin=None, sout=8192, table=1024, src=256, out=512):
        row = _hip.ProsodyRow(src, out, sin, sout, table, pos, m0, pos0, cap, n, count, up, down, half, taps, 1.0, lim,
                              flush, 0)
        a = _hip.ProsodyArgs(1, 0, ctypes.pointer(row))
        return lib.qt_prosody(ctypes.byref(a), None)

    right = P.ready(p, False, 1365)
    for wrong in (right + 1, right - 1, right - 127, p.out_len(1365)):
        assert call(wrong) == -1
    assert call(right, lim=1) == -1 and call(right - 127 + 1, lim=1) == -1
    assert call(p.out_len(1365), flush=1, cap=100) == -1 and call(99, flush=1, cap=100) == -1
    assert call(right, sin=8192) == -1                      # state_in == state_out
    assert call(right, table=None) == -1 and call(right, src=258) == -1
    assert call(right, pos0=25, pos=25, m0=0) == -1         # a start that is no multiple of down
    assert call(P.ready(p, False, 2000) - right, n=635, pos=1365, m0=right) == -1  # continues without its state
    assert call(P.ready(p, False, 40000), n=38635, pos=1365, m0=0, sin=16384) == -1  # behind the history
    assert call(right, half=p.half + 1) == -2 and call(right, taps=p.taps + 1) == -2
    assert call(right, up=2, down=2) == -2 and call(right, up=1, down=201, half=2010, taps=4021) == -2
    assert call(right, up=1, down=8, half=80, taps=161) == -2   # a ratio whose tile does not fit
