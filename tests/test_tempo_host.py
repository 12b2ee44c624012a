"""Speaking-rate stage, host side (qwen_tts/tempo.py): `speed_steps`, the emission rule and the numpy
reference.  No GPU."""
import numpy as np
import pytest

from qwen_tts import tempo as T

SPEEDS = (50, 80, 93, 125, 200)


def test_speed_steps_validation_and_broadcast():
    assert T.speed_steps(1.0, 3) is None
    assert T.speed_steps([1.0, 1, 1.0], 3) is None
    assert T.speed_steps(None, 2) is None
    assert T.speed_steps(1.25, 2) == [125, 125]
    assert T.speed_steps([1.0, 0.8, 1.5, 2.0, 0.5], 5) == [100, 80, 150, 200, 50]
    assert T.speed_steps(np.float32(0.93), 1) == [93]
    assert T.speed_steps(2, 1) == [200]
    for bad in (float("nan"), float("inf"), True, False, 0.49, 2.01, -1.0, "fast", [1.0, 1.25], [1.0, True, 1.0]):
        with pytest.raises(ValueError):
            T.speed_steps(bad, 3)
    with pytest.raises(ValueError):
        T.speed_steps([], 1)


def _needs(S, top):
    out, j = [], 0
    while True:
        v = T.HS if j == 0 else max(T.a(j, S) + 127, T.a(j - 1, S) + 127 + T.HS) + T.L
        while j == 0 and T.out_len(v, S) < T.HS:  # block 0 also waits until out_len reaches one block
            v += 1
        if v > top:
            return np.array(out)
        out.append(v)
        j += 1


def test_ready_history_and_monotonicity_brute_force():
    N = 6000
    n = np.arange(N + 1)
    worst = 0
    for S in range(50, 201):
        got = np.array([T.ready(S, int(k)) for k in n])
        if S == 100:
            assert (got == n).all()
            continue
        needs = _needs(S, N)
        want = np.searchsorted(needs, n, side="right") * T.HS  # block j exists once need(j) <= n_total
        assert (got == want).all(), S
        assert (np.diff(got) >= 0).all(), S
        # never more than the whole signal's output, so a flush after any prefix only adds samples
        assert (got <= np.array([T.out_len(int(k), S) for k in n])).all(), S
        # history: everything from the first pending block's lowest read up to n_total
        blocks = got // T.HS
        lowest = np.array([max(0, T.low(int(j), S)) for j in range(int(blocks.max()) + 2)])
        hist = np.maximum(0, n - lowest[blocks])
        assert all(T.history(S, int(k)) == hist[k] for k in n[::97]), S
        worst = max(worst, int(hist.max()))
        assert hist.max() <= T.HIST, (S, int(hist.max()))
    assert worst <= 1024
    for S in SPEEDS:
        for k in (0, 1, 239, 240, 479, 1365, 5999):
            assert T.history(S, k) == max(0, k - max(0, T.low(T.blocks_ready(S, k), S)))


def test_first_packet_blocks():
    assert [T.blocks_ready(S, 1365) for S in (50, 80, 125, 200)] == [6, 4, 3, 2]


def test_out_len():
    for S in SPEEDS + (100,):
        for n in (0, 1, 239, 240, 1365, 5000, 7321):
            assert T.out_len(n, S) == int(np.ceil(100 * n / S))
            x = np.zeros(n, np.float32)
            assert T.stretch(x, S).shape == (T.out_len(n, S),)
            assert T.ready(S, n, flush=True) == T.out_len(n, S)


def test_period_120_signal_stays_periodic():
    """A signal of exact period 120 comes out as the same periodic signal, phase-continuous: every candidate window a
    multiple of 120 from the continuation scores 0, so seg_j = t (mod 120) and both overlap-add terms are the same
    sample -- W0 x + W1 x, within 3 * 2^-24 * 0.5 of x for |x| <= 0.5."""
    rng = np.random.default_rng(7)
    p = (rng.standard_normal(120) * 0.15).clip(-0.5, 0.5).astype(np.float32)
    x = np.tile(p, 60)  # 7200 samples
    for S in SPEEDS:
        y, seg, _, _ = T.stretch(x, S, detail=True)
        full = (min(len(y), T.out_len(len(x) - 1500, S)) // T.HS) * T.HS  # blocks that read no zeros past the end
        assert full >= 5 * T.HS
        assert all((s - j * T.HS) % 120 == 0 for j, s in enumerate(seg[:full // T.HS]))
        want = p[np.arange(full) % 120]
        assert np.abs(y[:full].astype(np.float64) - want).max() <= 3 * 2.0 ** -24 * 0.5, S


def test_speed_one_copies():
    x = np.random.default_rng(1).standard_normal(1000).astype(np.float32)
    y = T.stretch(x, 100)
    assert y.dtype == np.float32 and np.array_equal(y, x)
    assert T.ready(100, 777) == 777 and T.history(100, 777) == 0


def test_abi_refuses_a_wrong_row_table():
    """qt_tempo checks every row against the emission rule before it launches: a count that is not the rule's, a
    state buffer used as both input and output, a start block that is no multiple of 5 or a continuing row without
    state is QT_ERR_ARG (no GPU needed: nothing is launched)."""
    import ctypes
    from qwen_tts import _hip
    lib = _hip.load_library()

    def call(count, n=1365, S=80, sin=None, sout=4096, pos=0, j0=0, block0=0, flush=0):
        row = _hip.TempoRow(256, 512, sin, sout, pos, j0, block0, n, count, S, flush)
        a = _hip.TempoArgs(1, 0, 1024, ctypes.pointer(row))
        return lib.qt_tempo(ctypes.byref(a), None)

    right = T.ready(80, 1365)
    for wrong in (right + 240, right - 240, right + 1, T.out_len(1365, 80)):
        assert call(wrong) == -1
    assert call(1365) == -1 and call(right, S=100) == -1      # a copying row hands out what it takes
    assert call(right, S=49) == -1 and call(right, S=201) == -1
    assert call(right, block0=3, j0=3, pos=T.a(3, 80)) == -1
    assert call(right, sin=4096) == -1                        # state_in == state_out
    assert call(T.ready(80, 2000) - right, n=635, pos=1365, j0=right // T.HS) == -1  # continues without its state
    assert call(T.ready(80, 2000), n=635, pos=1365, j0=0, sin=8192) == -1  # blocks the history no longer reaches


def test_reference_error_stays_inside_its_bound():
    rng = np.random.default_rng(3)
    x = (rng.standard_normal(5000) * 0.2).astype(np.float32)
    for S in SPEEDS:
        y, seg, y64, bound = T.stretch(x, S, detail=True)
        assert (np.abs(y - y64) <= bound).all()
        assert seg[0] == 0 and all(-128 <= s - T.a(j, S) < 128 for j, s in enumerate(seg))
