"""GPU units of the PCM output stage (csrc/resample.hip, qt_resample) through qwen_tts.PcmResampler, on seeded
randn * 0.3 inputs of at most 6,000 samples per row, at the seven rates served from 24 kHz.

* Against fp64 (tests/resample_refs.py, the definition on the fp32 taps widened): every element within
  small_kernel_refs.judge_fp32 -- twice the error of the same formula in plain torch fp32, at least 4 ulp -- of the
  output's sum_k |x[k] h[..]|.  Rows of 3285, 61 and 1 samples in one launch.
* Chunk invariance: one shot, sample by sample, and ragged chunks with an empty one and a separate flush give the
  same bits and, after every call, the emission rule's count.
* Ragged rows in one launch (idle / flushing / continuing), sentinels (7.0) around every slot of a test-owned output
  buffer, reset of a row; 64-bit positions; the s16 conversion with the clamp exercised.

measured on the MI355X (kernel vs fp64 / torch-fp32 vs fp64, of sum |x h|, the 3285-sample row of each rate):
  8000   2.2e-7 / 9.8e-8  (worst ratio, 2.3: 61 taps summed in sequence against torch's tree; inside the 4-ulp floor)
  12000  2.8e-7 / 1.4e-7      16000  2.4e-7 / 1.6e-7      22050  2.9e-7 / 1.7e-7      32000  2.6e-7 / 1.9e-7
  44100  3.2e-7 / 2.3e-7  (worst pair)                    48000  2.5e-7 / 1.7e-7
the 61- and 1-sample rows: 6.4e-9 .. 1.9e-7 / 6.4e-9 .. 1.6e-7.
"""
import pytest
import torch

import resample_refs as RR
import small_kernel_refs as R

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
S = R.SENTINEL


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _rs(rows, rate, fmt="f32", **kw):
    from qwen_tts import PcmResampler
    return PcmResampler(rows, rate, fmt, device=_dev(), **kw)


def _signal(n, seed):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed), dtype=F32) * 0.3


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _feed(rs, x, chunks, row=0):
    """Row `row` of rs takes x in `chunks` (lengths; the rest of the rows idle), then a flush of its own.  Returns the
    concatenated output after checking every call's count against the emission rule."""
    B, dev, p = rs.rows, rs.device, rs.plan
    xd, at, got, outs = x.to(dev), 0, 0, []
    for n in list(chunks) + [None]:
        flush = n is None
        n = 0 if flush else n
        lengths, offs = [0] * B, [0] * B
        lengths[row], offs[row] = n, at
        o = rs.push(xd, offs, lengths, [flush and b == row for b in range(B)])
        at += n
        assert all(o[b].numel() == 0 for b in range(B) if b != row)
        assert o[row].numel() == p.ready(at, flush) - got, (at, flush)
        got += o[row].numel()
        outs.append(o[row])
    assert at == x.numel() and got == p.out_len(x.numel())
    return torch.cat(outs)


@pytest.mark.parametrize("rate", RR.RATES)
def test_against_fp64(rate):
    lens = [3285, 61, 1]
    rs = _rs(3, rate)
    x = torch.zeros(3, max(lens), dtype=F32)
    for b, n in enumerate(lens):
        x[b, :n] = _signal(n, 10 * rate + b)
    outs = rs.push(x.to(rs.device), [0, 0, 0], lens, True)
    for b, n in enumerate(lens):
        ref = RR.resample(x[b, :n], rs.plan)
        assert outs[b].dtype == F32 and outs[b].shape == ref.shape == (rs.plan.out_len(n),)
        ok, ek, et = R.judge_fp32(outs[b].cpu(), RR.resample(x[b, :n], rs.plan, F32), ref,
                                  RR.resample_scale(x[b, :n], rs.plan))
        print(f"resample {rate} n={n}: kernel vs fp64 {ek:.3g}, torch-fp32 vs fp64 {et:.3g}")
        assert ok, (rate, n, ek, et)


@pytest.mark.parametrize("rate", RR.RATES)
def test_chunk_invariance(rate):
    n = 6000
    x = _signal(n, rate + 1)
    one = _feed(_rs(1, rate), x, [n])
    assert _same_bits(one, _rs(1, rate).one_shot(x.to(_dev())))
    by_sample = _feed(_rs(1, rate), x, [1] * 70 + [n - 70])
    ragged = _feed(_rs(1, rate), x, [1365, 1920, 3, 0, 61, n - 1365 - 1920 - 3 - 61])
    assert _same_bits(one, by_sample) and _same_bits(one, ragged)


@pytest.mark.parametrize("rate", [8000, 44100])
def test_ragged_rows_in_one_launch(rate):
    """Second call: row 0 idles (length 0, no flush), row 1 flushes, row 2 continues -- once through push(), once through
    the ABI on a twin into a sentinel-filled buffer the test owns."""
    from qwen_tts import kernels as K
    dev = _dev()
    a, t = _rs(3, rate), _rs(3, rate)
    p = a.plan
    x = torch.stack([_signal(900, rate + 10 + b) for b in range(3)]).to(dev)
    first = a.push(x, [0, 0, 0], [500, 400, 300], False)
    t.push(x, [0, 0, 0], [500, 400, 300], False)
    offs, lens, flush = [500, 400, 300], [0, 100, 600], [False, True, False]
    second = a.push(x, offs, lens, flush)
    assert second[0].numel() == 0 and (a.pos, a.m0) == ([500, 500, 900], [p.ready(500), p.out_len(500), p.ready(900)])
    for b, n in enumerate([500, 500, 900]):
        xb = x[b, :n].cpu()  # what is ready does not depend on the future: the head of the taken samples' output
        got = torch.cat([first[b], second[b]])
        c = got.numel()
        assert c == (p.out_len(n) if flush[b] else p.ready(n))
        ok, ek, et = R.judge_fp32(got.cpu(), RR.resample(xb, p, F32)[:c], RR.resample(xb, p)[:c],
                                  RR.resample_scale(xb, p)[:c])
        assert ok, (rate, b, ek, et)
    # the twin, through the ABI: slots 5 apart in a sentinel buffer
    hist0, state0 = t.hist.clone(), (list(t.pos), list(t.m0), list(t.par))
    counts = [s.numel() for s in second]
    buf = torch.full((sum(counts) + 20,), S, dtype=F32, device=dev)
    slot, rows = [5, 10, 15 + counts[1]], []
    for b in range(3):
        rows.append((x[b, offs[b]:].data_ptr() if lens[b] else None, buf[slot[b]:].data_ptr() if counts[b] else None,
                     t.hist[t.par[b], b].data_ptr(), t.hist[t.par[b] ^ 1, b].data_ptr(), t.pos[b], t.m0[b], lens[b],
                     counts[b], int(flush[b])))
    K.resample(t.table, p.up, p.down, p.half, p.taps, t.H, "f32", rows)
    keep = torch.ones_like(buf, dtype=torch.bool)
    for b in range(3):
        assert _same_bits(buf[slot[b]:slot[b] + counts[b]], second[b])
        keep[slot[b]:slot[b] + counts[b]] = False
    assert bool((buf[keep] == S).all())
    assert torch.equal(t.hist[:, 0], hist0[:, 0]) and (t.pos, t.m0, t.par) == state0  # the idle row's state
    assert torch.equal(t.hist[t.par[1], 1], hist0[t.par[1], 1])                       # histories read are not written
    # a reset row equals a fresh resampler
    a.reset(1)
    y = _signal(700, rate + 20)
    assert _same_bits(_feed(a, y, [333, 367], row=1), _feed(_rs(1, rate), y, [700]))


@pytest.mark.parametrize("rate", [8000, 22050, 48000])
def test_64_bit_positions(rate):
    x = _signal(3000, rate + 2)
    zero = _rs(1, rate)
    far = _rs(1, rate, start_pos=zero.plan.down * 2 ** 31)
    assert far.m0[0] == zero.plan.up * 2 ** 31 and far.pos[0] * far.plan.up >= 2 ** 31
    assert _same_bits(_feed(zero, x, [1365, 1635]), _feed(far, x, [1365, 1635]))


@pytest.mark.parametrize("rate", [8000, 48000])
def test_s16(rate):
    n = 4800
    x = torch.where(torch.arange(n) % 48 < 24, 1.0, -1.0).to(F32)
    f = _feed(_rs(1, rate, "f32"), x, [1365, 1920, n - 3285])
    s = _feed(_rs(1, rate, "s16"), x, [1365, 1920, n - 3285])
    assert float(f.abs().max()) > 1.0  # the filter's overshoot: the clamp is exercised
    assert s.dtype == torch.int16 and torch.equal(s.cpu(), RR.s16(f.cpu()))
    assert int(s.max()) == 32767 and int(s.min()) == -32767


def test_s16_at_the_input_rate_is_the_exact_conversion():
    x = _signal(5000, 77) * 4  # some samples beyond +-1
    s = _feed(_rs(1, 24000, "s16"), x, [1365, 1920, 1715])
    assert torch.equal(s.cpu(), RR.s16(x)) and float(x.abs().max()) > 1.0
    assert _same_bits(_feed(_rs(1, 24000, "f32"), x, [5000]), x.to(_dev()))
