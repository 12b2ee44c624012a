"""GPU units of the speaking-rate stage (csrc/tempo.hip, qt_tempo) through qwen_tts.tempo.PcmTempo.

* Against the numpy reference (qwen_tts.tempo.stretch): rows of 5000, 7321 and 1 samples in one launch -- a pitch glide
  in noise, speech-like noise bursts, one sample -- at S = 50, 80, 93, 125, 200.  Every output sample lies within
  3 * 2^-24 * (|W0 a| + |W1 b|) of the fp64 overlap-add at the reference's own d: the search is integer-exact, so no
  sample is left out for being near a tie, and a wrong d misses the bound by orders of magnitude.
* Chunk invariance: one shot, ragged chunks with an empty one and a separate flush, and a 2000-sample signal fed sample
  by sample give the same bits and, after every call, the emission rule's count.
* start_block = 5 * 2^31 gives the bits of position 0; an S = 100 row beside stretched rows is its input, never held
  back; a row table with a wrong count is QT_ERR_ARG and writes nothing.

measured on the MI355X (worst |error| / bound over every sample, the 5000- / 7321-sample rows): S = 50 0.58 / 0.58,
80 0.56 / 0.58, 93 0.61 / 0.58, 125 0.53 / 0.60, 200 0.55 / 0.51; max |error| 9.9e-8.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F32 = torch.float32
SPEEDS = (50, 80, 93, 125, 200)
LENS = (5000, 7321, 1)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _tempo(rows, **kw):
    from qwen_tts.tempo import PcmTempo
    return PcmTempo(rows, device=_dev(), **kw)


def _glide(n, seed):
    """noise plus a pitch glide from 90 to 320 Hz with two harmonics"""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64) / 24000
    f = 90 + (320 - 90) * t / max(float(t[-1]), 1e-9)
    ph = 2 * np.pi * torch.cumsum(f, 0) / 24000
    x = 0.3 * torch.sin(ph) + 0.15 * torch.sin(2 * ph) + 0.08 * torch.sin(3 * ph)
    return (x + 0.05 * torch.randn(n, generator=g, dtype=torch.float64)).to(F32)


def _bursts(n, seed):
    g = torch.Generator().manual_seed(seed)
    env = (torch.sin(torch.arange(n, dtype=F32) * (2 * np.pi / 1700)) > 0).to(F32)
    return torch.randn(n, generator=g, dtype=F32) * 0.4 * env  # (the clamp at +-1 is exercised)


_SIG = {}


def _signals():
    if not _SIG:
        _SIG["x"] = [_glide(LENS[0], 1), _bursts(LENS[1], 2), torch.tensor([0.25], dtype=F32)]
    return _SIG["x"]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("S", SPEEDS)
def test_against_numpy_reference(S):
    from qwen_tts import tempo as T
    xs = _signals()
    tp = _tempo(3)
    x = torch.zeros(3, max(LENS), dtype=F32)
    for b, v in enumerate(xs):
        x[b, :v.numel()] = v
    outs = tp.push(x.to(tp.device), [0, 0, 0], list(LENS), True, [S] * 3)
    for b, v in enumerate(xs):
        _, seg, y64, bound = T.stretch(v.numpy(), S, detail=True)
        got = outs[b].cpu().numpy().astype(np.float64)
        assert got.shape == y64.shape == (T.out_len(LENS[b], S),)
        err = np.abs(got - y64)
        worst = float((err / np.maximum(bound, 1e-300)).max()) if bound.any() else 0.0
        print(f"S={S} row {b}: {got.size} samples, {len(seg)} blocks, max err {err.max():.3g}, "
              f"worst err / bound {worst:.3g}")
        assert (err <= bound).all(), (S, b, int(np.argmax(err - bound)))


def _feed(tp, x, chunks, S, row=0):
    """Row `row` of tp takes x in `chunks` (lengths; the other rows idle), then a flush of its own; every call's count
    is checked against the emission rule."""
    from qwen_tts import tempo as T
    B, xd, at, got, outs = tp.rows, x.to(tp.device), 0, 0, []
    for n in list(chunks) + [None]:
        flush = n is None
        n = 0 if flush else n
        lengths, offs = [0] * B, [0] * B
        lengths[row], offs[row] = n, at
        o = tp.push(xd, offs, lengths, [flush and b == row for b in range(B)], [S] * B)
        at += n
        assert all(o[b].numel() == 0 for b in range(B) if b != row)
        assert o[row].numel() == T.ready(S, at, flush) - got, (at, flush)
        got += o[row].numel()
        outs.append(o[row])
    assert at == x.numel() and got == T.out_len(x.numel(), S)
    return torch.cat(outs)


@pytest.mark.parametrize("S", SPEEDS)
def test_chunk_invariance(S):
    x = _signals()[0]
    tp = _tempo(2)
    whole = tp.one_shot(x.to(tp.device), S)
    ragged = _feed(tp, x, [1, 238, 1, 0, 1365, 7, 1920, 1468], S, row=1)
    assert _same_bits(whole, ragged)
    tp.reset(1)
    again = _feed(tp, x, [5000], S, row=1)  # a reset row starts over
    assert _same_bits(whole, again)


def test_sample_by_sample():
    x = _signals()[1][:2000].clone()
    for S in (80, 200):
        tp = _tempo(1)
        whole = tp.one_shot(x.to(tp.device), S)
        assert _same_bits(whole, _feed(tp, x, [1] * 2000, S))


def test_large_start_block():
    x = _signals()[0]
    for S in (93, 200):
        base = _tempo(1)
        far = _tempo(1, start_block=5 * 2 ** 31)
        want = _feed(base, x, [1365, 1920, 1715], S)
        got = _feed(far, x, [1365, 1920, 1715], S)
        assert _same_bits(want, got)
    with pytest.raises(ValueError, match="multiple of 5"):
        _tempo(1, start_block=3)


def test_speed_one_row_beside_stretched_rows():
    xs = _signals()
    tp = _tempo(3)
    n = 4000
    x = torch.stack([xs[0][:n], xs[1][:n], xs[1][1000:1000 + n]]).to(tp.device)
    steps = [125, 100, 50]
    got, at = [], 0
    for c in (1365, 1, 0, 1920, 714):
        o = tp.push(x, [at] * 3, [c] * 3, False, steps)
        at += c
        assert o[1].numel() == c  # never held back
        got.append(o[1])
    o = tp.push(None, [0] * 3, [0] * 3, True, steps)
    assert at == n and o[1].numel() == 0
    assert _same_bits(torch.cat(got), x[1])
    assert o[0].numel() > 0 and o[2].numel() > 0  # the stretched rows did hold samples back


def test_row_table_validation():
    from qwen_tts import _hip, tempo as T
    dev = _dev()
    tp = _tempo(1)
    x = _signals()[0][:1365].to(dev)
    right = T.ready(80, 1365)
    out = torch.full((right + 480,), 7.0, dtype=F32, device=dev)
    state = torch.zeros(_hip.TEMPO_STATE_BYTES // 8, dtype=torch.int64, device=dev)
    for count in (right - 240, right + 240, right - 1, 0):
        row = _hip.TempoRow(x.data_ptr(), out.data_ptr(), None, state.data_ptr(), 0, 0, 0, 1365, count, 80, 0)
        args = _hip.TempoArgs(1, 0, tp.window.data_ptr(), ctypes.pointer(row))
        assert _hip.lib().qt_tempo(ctypes.byref(args), _hip.stream()) == -1  # QT_ERR_ARG
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and not bool(state.any())
    # the rule's count runs, and writes exactly that many samples
    row = _hip.TempoRow(x.data_ptr(), out.data_ptr(), None, state.data_ptr(), 0, 0, 0, 1365, right, 80, 0)
    args = _hip.TempoArgs(1, 0, tp.window.data_ptr(), ctypes.pointer(row))
    assert _hip.lib().qt_tempo(ctypes.byref(args), _hip.stream()) == 0
    torch.cuda.synchronize()
    assert bool((out[right:] == 7.0).all()) and _same_bits(out[:right], tp.one_shot(x, 80)[:right])
