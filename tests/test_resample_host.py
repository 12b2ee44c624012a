"""CPU-only: the PCM output stage's host side (qwen_tts/resample.py) -- the filter plan, the streaming emission rule
and the fp64 reference formula of tests/resample_refs.py that the GPU tests judge the kernel by."""
import numpy as np
import pytest
import torch

import resample_refs as RR
import small_kernel_refs as R
from qwen_tts import resample as RS


@pytest.mark.parametrize("rate", RR.RATES)
def test_plan(rate):
    p = RS.plan(rate)
    up, down, length, taps = RR.EXPECT[rate]
    assert (p.up, p.down, len(p.h), p.taps) == (up, down, length, taps)
    assert p.half == 10 * max(up, down) and length == 2 * p.half + 1
    assert p.h.dtype == np.float32 and p.table.dtype == np.float32 and p.table.shape == (up, taps)
    h = p.h.astype(np.float64)
    assert abs(h.sum() - up) <= 4 * length * 2.0 ** -24 * np.abs(h).max()  # fp32 rounding of `length` taps
    assert np.array_equal(p.h, p.h[::-1])
    # phase-major: table[r][j] = h[r + j*up], zero past the filter's end
    for r in range(up):
        col = p.h[r::up]
        assert np.array_equal(p.table[r, :len(col)], col) and not p.table[r, len(col):].any()


@pytest.mark.parametrize("rate", RR.RATES)
def test_plan_is_scipys_default_filter(rate):
    sig = pytest.importorskip("scipy.signal")
    p = RS.plan(rate)
    ref = sig.firwin(2 * p.half + 1, 1.0 / max(p.up, p.down), window=("kaiser", 5.0)) * p.up
    # the stored taps are the fp32 rounding (half an ulp, 2^-24 relative) of a filter equal to scipy's to fp64 rounding
    assert np.all(np.abs(p.h - ref) <= 2.0 ** -24 * np.abs(ref) + 1e-14)


@pytest.mark.parametrize("rate", RR.RATES)
def test_emission_rule(rate):
    p = RS.plan(rate)
    last = RR.last_needed(p, p.out_len(400))
    prev = 0
    for n in range(401):
        r = RS.ready(p, n)
        assert r == RR.brute_ready(p, n, last), n
        assert RS.ready(p, n, flush=True) == -(-n * p.up // p.down)
        assert prev <= r <= RS.ready(p, n, flush=True)
        prev = r
    assert RS.ready(p, 1365) == RR.FIRST_PACKET[rate]
    # held back: at most 10 * max(1, down/up) input samples' worth of outputs
    assert all(RS.ready(p, n, True) - RS.ready(p, n) <= -(-10 * max(p.up, p.down) // p.down) + 1 for n in range(401))


@pytest.mark.parametrize("rate", RR.RATES)
def test_ready_outputs_do_not_depend_on_the_future(rate):
    p = RS.plan(rate)
    g = torch.Generator().manual_seed(rate)
    x = torch.randn(1500, generator=g, dtype=torch.float64)
    full = RR.resample(x, p)
    for n in (1, 7, 31, 1365, 1366):
        cut = RR.resample(x[:n], p)
        r = RS.ready(p, n)
        assert torch.equal(cut[:r], full[:r]), n


@pytest.mark.parametrize("rate", RR.RATES)
def test_reference_formula_is_resample_poly(rate):
    """The fp64 reference against scipy.signal.resample_poly run on the same taps (the fp32 table widened), 3,285
    random samples (resample_poly multiplies a given filter by `up`, so it gets h / up).  Both are fp64 sums of the
    same <= 61 products in different orders: the bound is small_kernel_refs.fp32_tolerance's margin (2) times the
    2e-15 measured when the definition was written, of each output's sum of |products| (here: 4.1e-16 .. 6.5e-16)."""
    sig = pytest.importorskip("scipy.signal")
    p = RS.plan(rate)
    g = torch.Generator().manual_seed(1000 + rate)
    x = torch.randn(3285, generator=g, dtype=torch.float64)
    ref = RR.resample(x, p)
    sp = torch.from_numpy(sig.resample_poly(x.numpy(), p.up, p.down, window=p.h.astype(np.float64) / p.up))
    assert sp.shape == ref.shape == (p.out_len(3285),)
    err = float(R.scaled_error(sp, ref, RR.resample_scale(x, p)))
    print(f"{rate}: reference vs resample_poly {err:.3g} of sum|x h|")
    assert err <= 2.0 * 2e-15
    # and with scipy's own (fp64) default filter the difference is the fp32 rounding of the taps
    sp0 = torch.from_numpy(sig.resample_poly(x.numpy(), p.up, p.down))
    assert float(R.scaled_error(sp0, ref, RR.resample_scale(x, p))) <= 2.0 ** -24


def test_refusals():
    for bad in (11025, 0, -8000):
        with pytest.raises(ValueError):
            RS.plan(bad)
    with pytest.raises(ValueError, match="147/320"):
        RS.plan(11025)
    with pytest.raises(ValueError, match="pcm_format"):
        RS.output_format(16000, "s24")
    with pytest.raises(ValueError):
        RS.output_format(11025, "s16")
    assert RS.output_format(None, "f32") is None and RS.output_format(24000, "f32") is None
    p, fmt = RS.output_format(None, "s16")
    assert (p.up, p.down, fmt) == (1, 1, "s16") and p.h[p.half] == 1.0 and np.count_nonzero(p.h) == 1


def test_abi_refuses_a_wrong_row_table():
    """qt_resample checks every row against the emission rule before it launches: a count that is not the rule's, or
    a history buffer used as both input and output, is QT_ERR_ARG (no GPU needed: nothing is launched)."""
    import ctypes
    from qwen_tts import _hip
    L = _hip.load_library()
    p = RS.plan(16000)

    def call(count, n=100, hin=64, hout=128, pos=0, m0=0, flush=0):
        rows = (_hip.ResampleRow * 1)()
        rows[0].src, rows[0].out, rows[0].hist_in, rows[0].hist_out = 256, 512, hin, hout
        rows[0].pos, rows[0].m0, rows[0].n, rows[0].count, rows[0].flush = pos, m0, n, count, flush
        a = _hip.ResampleArgs(p.up, p.down, p.half, p.taps, p.taps, _hip.PCM_F32, 1, 0, 1024, rows)
        return L.qt_resample(ctypes.byref(a), None)

    assert call(RS.ready(p, 100) + 1) == -1
    assert call(RS.ready(p, 100, True)) == -1
    assert call(RS.ready(p, 100), hin=128) == -1
    early = RS.ready(p, 1000) - 40  # outputs the history no longer reaches
    assert call(RS.ready(p, 1100) - early, pos=1000, m0=early) == -1
