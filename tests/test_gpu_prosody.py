"""GPU units of the pitch and volume stage (csrc/prosody.hip, qt_prosody) through qwen_tts.prosody.PcmProsody, on
seeded randn * 0.3 inputs of at most 6,000 samples per row.

* Against fp64 (g * tests/resample_refs.py's definition on the fp32 taps widened): rows of 3285, 61 and 1 samples with
  three different ratios in one launch, over 1/2, 2/1, 47/50, 199/200, 101/199, 1/4 and 4/1, at 0 dB and -6 dB, limiter
  off.  Every element within small_kernel_refs.judge_fp32 -- twice the error of the same formula in plain torch fp32,
  at least 4 ulp -- of g * sum_k |x[k] h[..]|.
* Chunk invariance at 47/50 limited, 101/199 unlimited and 1/1 limited: one shot, sample by sample, ragged chunks with
  an empty one and a separate flush, and one_shot() give the same bits and, after every call, the emission rule's count.
* Limiter: 1/1 rows are the numpy definition bit for bit; a resampled limited row is the numpy limiter applied to the
  output of its twin with the limited flag cleared (through the ABI); max |y| <= 1.0.
* Ragged rows in one launch (idle / flushing / continuing) with sentinels (7.0) around every slot of a test-owned
  buffer, reset with a change of ratio, 64-bit positions, 17 rows (two launches), the cap at flush, verbatim rows.

measured on the MI355X (kernel vs fp64 / torch-fp32 vs fp64, of g * sum |x h|, the 3285-sample row of each ratio):
  1/2    2.0e-7 / 1.2e-7      2/1      2.1e-7 / 2.1e-7      47/50  2.5e-7 / 1.8e-7      199/200  2.7e-7 / 2.3e-7
  101/199  2.6e-7 / 1.2e-7  (worst ratio, 2.2: up to 80 taps summed in sequence against torch's tree; inside the 4-ulp
  floor)                     1/4      2.2e-7 / 1.2e-7      4/1    2.4e-7 / 1.9e-7
the 61- and 1-sample rows: 2.6e-11 .. 2.4e-7 / 2.6e-11 .. 1.5e-7.
"""
import numpy as np
import pytest
import torch

import resample_refs as RR
import small_kernel_refs as R

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
SENT = R.SENTINEL
# (T, S): 1/2, 2/1, 47/50, 199/200, 101/199, 1/4, 4/1
RATIOS = [(50, 100), (200, 100), (94, 100), (199, 200), (101, 199), (50, 200), (200, 50)]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _stage(rows, settings=None, **kw):
    """A PcmProsody of `rows` rows, row b at settings[b] = (T, S, db)"""
    from qwen_tts.prosody import PcmProsody
    pp = PcmProsody(rows, device=_dev(), **kw)
    for b, s in enumerate(settings or ()):
        pp.reset(b, *s)
    return pp


def _signal(n, seed):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed), dtype=F32) * 0.3


def _square(n, period=300):
    return torch.where((torch.arange(n) // (period // 2)) % 2 == 0, 1.0, -1.0).to(F32)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _same_as_numpy(t, a):
    return t.dtype == F32 and tuple(t.shape) == a.shape and np.array_equal(t.cpu().numpy().view(np.int32),
                                                                            a.view(np.int32))


def _feed(pp, x, chunks, row=0, cap=None):
    """Row `row` of pp takes x in `chunks` (lengths; the rest of the rows idle), then a flush of its own.  Returns the
    concatenated output after checking every call's count against the emission rule."""
    from qwen_tts import prosody as P
    B, p, lim = pp.rows, pp.plan[row], pp.db[row] > 0
    xd, at, got, outs = x.to(pp.device), 0, 0, []
    for n in list(chunks) + [None]:
        flush = n is None
        n = 0 if flush else n
        lengths, offs, caps = [0] * B, [0] * B, [None] * B
        lengths[row], offs[row], caps[row] = n, at, cap
        o = pp.push(xd, offs, lengths, [flush and b == row for b in range(B)], caps)
        at += n
        assert all(o[b].numel() == 0 for b in range(B) if b != row)
        assert o[row].numel() == P.ready(p, lim, at, flush, cap) - got, (at, flush)
        got += o[row].numel()
        outs.append(o[row])
    assert at == x.numel() and got == (p.out_len(at) if cap is None else min(cap, p.out_len(at)))
    return torch.cat(outs)


def _abi_rows(t, src, offs, lens, flush, counts, outs, limited=None):
    """The row table PcmProsody.push would build for stage t, with the outputs at the pointers `outs` and, where
    given, the limited flags of `limited` instead of the rows' own."""
    from qwen_tts import prosody as P
    rows = []
    for b in range(t.rows):
        p = t.plan[b]
        pos0, m_start = t.start_period * p.down, t.start_period * p.up
        lim = t.db[b] > 0 if limited is None else limited[b]
        rows.append((src[b, offs[b]:].data_ptr() if lens[b] else None, outs[b] if counts[b] else None,
                     None if t.fresh[b] else t.state[t.par[b], b].data_ptr(), t.state[t.par[b] ^ 1, b].data_ptr(),
                     t.table[b].data_ptr(), pos0 + t.taken[b], m_start + t.given[b], pos0, -1, lens[b], counts[b],
                     p.up, p.down, p.half, p.taps, float(P.gain(t.db[b])), int(lim), int(flush[b])))
    return rows


@pytest.mark.parametrize("first", range(len(RATIOS)))
def test_against_fp64(first):
    from qwen_tts import prosody as P
    lens = [3285, 61, 1]
    sets = [RATIOS[(first + b) % len(RATIOS)] + ((0.0, -6.0, 0.0)[b] if first % 2 == 0 else (-6.0, 0.0, -6.0)[b],)
            for b in range(3)]
    pp = _stage(3, sets)
    x = torch.zeros(3, max(lens), dtype=F32)
    for b, n in enumerate(lens):
        x[b, :n] = _signal(n, 100 * first + b)
    outs = pp.push(x.to(pp.device), [0, 0, 0], lens, True)
    for b, n in enumerate(lens):
        p, g = pp.plan[b], P.gain(sets[b][2])
        ref = float(g) * RR.resample(x[b, :n], p)
        assert outs[b].dtype == F32 and outs[b].shape == ref.shape == (p.out_len(n),)
        ok, ek, et = R.judge_fp32(outs[b].cpu(), torch.tensor(g) * RR.resample(x[b, :n], p, F32), ref,
                                  float(g) * RR.resample_scale(x[b, :n], p))
        print(f"prosody {p.up}/{p.down} {sets[b][2]:+g} dB n={n}: kernel vs fp64 {ek:.3g}, torch-fp32 vs fp64 {et:.3g}")
        assert ok, (sets[b], n, ek, et)


@pytest.mark.parametrize("T,S,db", [(94, 100, 6.0), (101, 199, 0.0), (100, 100, 6.0)])
def test_chunk_invariance(T, S, db):
    n = 6000
    x = _signal(n, T + S)
    sets = [(T, S, db)]
    one = _feed(_stage(1, sets), x, [n])
    assert _same_bits(one, _stage(2).one_shot(x.to(_dev()), T, S, db))
    by_sample = _feed(_stage(1, sets), x, [1] * 70 + [n - 70])
    ragged = _feed(_stage(1, sets), x, [1365, 1920, 3, 0, 61, n - 1365 - 1920 - 3 - 61])
    assert _same_bits(one, by_sample) and _same_bits(one, ragged)
    if db > 0:
        assert float((x * 2).abs().max()) > 1.0 and float(one.abs().max()) <= 1.0  # the limiter worked


@pytest.mark.parametrize("db,square", [(12.0, False), (6.0, True)])
def test_unit_ratio_limiter_is_the_numpy_definition(db, square):
    from qwen_tts import prosody as P
    n = 3000
    x = _square(n) if square else _signal(n, 31)
    want = P.apply(x.numpy(), 100, 100, db)
    got = _feed(_stage(1, [(100, 100, db)]), x, [1365, 1, 1634])
    assert _same_as_numpy(got, want)
    assert float(got.abs().max()) <= 1.0 and float(P.gain(db)) * float(x.abs().max()) > 1.0


@pytest.mark.parametrize("T,S", [(94, 100), (50, 200), (200, 100)])
def test_resampled_limiter_is_numpy_on_the_unlimited_twin(T, S):
    from qwen_tts import kernels as K
    from qwen_tts import prosody as P
    n, db = 2500, 9.0
    x = _signal(n, 7 * T + S)
    got = _feed(_stage(1, [(T, S, db)]), x, [1365, 1135])
    t = _stage(1, [(T, S, db)])  # the twin: the same row with the limited flag cleared
    c = t.plan[0].out_len(n)
    v = torch.full((c + 10,), SENT, dtype=F32, device=t.device)
    xd = x.to(t.device)[None]
    K.prosody(_abi_rows(t, xd, [0], [n], [True], [c], [v[5:].data_ptr()], limited=[False]))
    v = v.cpu()
    assert (v[:5] == SENT).all() and (v[5 + c:] == SENT).all()
    v = v[5:5 + c].numpy()
    assert np.abs(v).max() > 1.0
    assert _same_as_numpy(got, P.limit(v))
    assert float(got.abs().max()) <= 1.0


def test_ragged_rows_in_one_launch():
    """Second call: row 0 idles (length 0, no flush), row 1 flushes, row 2 continues -- once through push(), once through
    the ABI on a twin into a sentinel-filled buffer the test owns.  Three ratios, the flushing row limited."""
    from qwen_tts import kernels as K
    from qwen_tts import prosody as P
    dev = _dev()
    sets = [(50, 200, 0.0), (94, 100, 6.0), (200, 100, -6.0)]
    a, t = _stage(3, sets), _stage(3, sets)
    x = torch.stack([_signal(900, 40 + b) for b in range(3)]).to(dev)
    first = a.push(x, [0, 0, 0], [500, 400, 300], False)
    t.push(x, [0, 0, 0], [500, 400, 300], False)
    offs, lens, flush = [0, 400, 300], [0, 100, 600], [False, True, False]
    second = a.push(x, offs, lens, flush)
    assert second[0].numel() == 0 and a.taken == [500, 500, 900]
    for b, n in enumerate([500, 500, 900]):
        want = a.one_shot(x[b, :n], *sets[b])  # what is ready does not depend on the future: the head of it
        got = torch.cat([first[b], second[b]])
        assert got.numel() == P.ready(a.plan[b], sets[b][2] > 0, n, flush[b])
        assert _same_bits(got, want[:got.numel()]), b
    state0 = t.state.clone()
    counts = [s.numel() for s in second]
    buf = torch.full((sum(counts) + 20,), SENT, dtype=F32, device=dev)
    slot = [5, 10, 15 + counts[1]]
    K.prosody(_abi_rows(t, x, offs, lens, flush, counts, [buf[s:].data_ptr() for s in slot]))
    keep = torch.ones(buf.numel(), dtype=torch.bool)
    for b in range(3):
        assert _same_bits(buf[slot[b]:slot[b] + counts[b]], second[b]), b
        keep[slot[b]:slot[b] + counts[b]] = False
    assert (buf.cpu()[keep] == SENT).all()
    # the idle row's state is untouched; the others wrote the half they do not read
    assert torch.equal(t.state[:, 0], state0[:, 0])
    for b in (1, 2):
        assert torch.equal(t.state[t.par[b], b], state0[t.par[b], b])
        assert not torch.equal(t.state[t.par[b] ^ 1, b], state0[t.par[b] ^ 1, b])
    # a reset row equals a fresh stage, at its old ratio and at a new one
    y = _signal(700, 60)
    a.reset(1)
    assert _same_bits(_feed(a, y, [333, 367], row=1), _feed(_stage(1, [sets[1]]), y, [700]))
    a.reset(1, 101, 199, 3.0)
    assert _same_bits(_feed(a, y, [333, 367], row=1), _feed(_stage(1, [(101, 199, 3.0)]), y, [700]))


@pytest.mark.parametrize("T,S,db", [(94, 100, 6.0), (50, 200, 0.0), (200, 100, 0.0)])
def test_64_bit_positions(T, S, db):
    x = _signal(3000, T + 2)
    zero = _stage(1, [(T, S, db)])
    far = _stage(1, [(T, S, db)], start_period=2 ** 31)
    assert far.start_period * far.plan[0].down * far.plan[0].up >= 2 ** 31
    assert _same_bits(_feed(zero, x, [1365, 1635]), _feed(far, x, [1365, 1635]))


def test_17_rows_take_two_launches():
    sets = [RATIOS[b % len(RATIOS)] + ((0.0, 6.0, -6.0)[b % 3],) for b in range(17)]
    pp = _stage(17, sets)
    lens = [300 + 17 * b for b in range(17)]
    x = torch.stack([_signal(600, 80 + b) for b in range(17)]).to(pp.device)
    outs = pp.push(x, [0] * 17, lens, True)
    for b in range(17):
        assert _same_bits(outs[b], pp.one_shot(x[b, :lens[b]], *sets[b])), b


@pytest.mark.parametrize("db", [0.0, 6.0])
def test_cap_cuts_at_flush(db):
    n = 2000
    x = _signal(n, 90)
    whole = _feed(_stage(1, [(94, 100, db)]), x, [n])
    cap = whole.numel() - 3
    cut = _feed(_stage(1, [(94, 100, db)]), x, [1365, 635], cap=cap)
    assert cut.numel() == cap and _same_bits(cut, whole[:cap])
    assert _same_bits(_stage(1).one_shot(x.to(_dev()), 94, 100, db, cap=cap), cut)


def test_default_rows_are_verbatim_copies():
    """pitch 0 / 0 dB rows beside non-default neighbours: their input, -0.0 and all, never held back"""
    pp = _stage(3, [(94, 100, 6.0), (100, 100, 0.0), (125, 125, 0.0)])
    x = torch.stack([_signal(1000, 95 + b) for b in range(3)])
    x[1, 3], x[2, 0] = -0.0, -0.0
    xd = x.to(pp.device)
    a = pp.push(xd, [0, 0, 0], [400, 400, 1], False)
    b = pp.push(xd, [400, 400, 1], [600, 600, 999], True)
    assert a[1].numel() == 400 and a[2].numel() == 1
    for r in (1, 2):
        assert _same_bits(torch.cat([a[r], b[r]]), xd[r])
    assert _same_bits(torch.cat([a[0], b[0]]), pp.one_shot(xd[0], 94, 100, 6.0))
