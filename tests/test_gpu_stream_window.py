"""GPU units of the per-row stream kernels (csrc/stream.hip) through qwen_tts.kernels, against the plain restatement
of tests/stream_window_ref.py.  Both kernels only move data (and count), so every result is bit-exact, fp32 and bf16.

Every launch's row table mixes the four row states: idle (nrow 0), partial, full, and a beginning row with its head.
H covers no history (a masked copy), one row (the transposed convs), a k=7 conv and the largest (k=7, dilation 9);
n x rows_per_frame covers windows shorter than, equal to and longer than the history, one to many blocks per batch
row; C covers less than a wave of 16-byte groups per row, a count that straddles waves and one that straddles blocks.
All buffers carry a sentinel row (or batch row) behind their end, which must survive."""
import pytest
import torch

import stream_window_ref as R

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
S = 7.0


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# (rows of x, rows per frame, nrow of the partial row): n * rows_per_frame in {1, 4, 33}, and 150 rows
WINDOWS = [(1, 1, 0), (4, 1, 3), (4, 2, 1), (33, 33, 0), (33, 3, 7), (150, 15, 6)]


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("head", [0, 8, 200])
@pytest.mark.parametrize("C", [8, 96, 1032])
@pytest.mark.parametrize("L,rpf,part", WINDOWS)
@pytest.mark.parametrize("H", [0, 1, 6, 54])
def test_stream_window(H, L, rpf, part, C, head, dtype):
    from qwen_tts import kernels as Kn
    dev = _dev()
    B, full = 3, L // rpf
    g = torch.Generator().manual_seed(H * 1000 + L * 10 + C + head)
    hist = torch.randn(B, H, C, generator=g).to(dtype)
    x = torch.randn(B, L, C, generator=g).to(dtype)
    # two launches, so that every batch row is once idle / partial / full and once beginning
    for nrow, begin in (([0, part, full], [0, 0, 1]), ([full, 0, part], [1, 0, 0]), ([part, full, 0], [0, 1, 1])):
        want_xin, want_hist = R.stream_window(hist, x, nrow, begin, rpf, head)
        d_hist = torch.full((B + 1, H, C), S, dtype=dtype, device=dev)
        d_hist[:B] = hist.to(dev)
        d_x = x.to(dev)
        d_xin = torch.full((B + 1, H + L, C), S, dtype=dtype, device=dev)
        rows = torch.tensor([nrow, begin], dtype=torch.int32, device=dev)
        Kn.stream_window(d_hist if H else None, d_x, d_xin, B, H, L, C, rpf, head, rows)
        torch.cuda.synchronize()
        assert _same_bits(d_xin[:B].cpu(), want_xin), (nrow, begin)
        assert _same_bits(d_hist[:B].cpu(), want_hist), (nrow, begin)
        assert bool((d_xin[B] == S).all()) and bool((d_hist[B] == S).all())
        assert _same_bits(d_x.cpu(), x)
        hist = want_hist  # the next launch continues from this state


def test_stream_window_rejects_bad_shapes():
    from qwen_tts import kernels as Kn
    dev = _dev()
    rows = torch.zeros(2, 1, dtype=torch.int32, device=dev)
    x = torch.zeros(1, 4, 6, device=dev)
    with pytest.raises(RuntimeError):  # a channel row that is no multiple of 16 bytes
        Kn.stream_window(torch.zeros(1, 2, 6, device=dev), x, torch.zeros(1, 6, 6, device=dev), 1, 2, 4, 6, 1, 0, rows)


@pytest.mark.parametrize("n", [1, 7])
def test_stream_rows(n):
    from qwen_tts import kernels as Kn
    dev = _dev()
    B, cap = 5, 20
    nf = torch.tensor([3, 11, cap - n, 6, 0], dtype=torch.int32)
    # continuing with a partial count, a beginning row over an old clock, a row ending exactly at capacity, an idle
    # row, a beginning row with no frames (a reset)
    nrow, begin = [max(n - 2, 0), n, n, 0, 0], [0, 1, 0, 0, 1]
    pos, row_len, new = R.stream_rows(nf, nrow, begin, n)
    assert int(new[2]) == cap
    d_nf = torch.full((B + 1,), 7, dtype=torch.int32, device=dev)
    d_nf[:B] = nf.to(dev)
    d_pos = torch.full((B + 1, n), 7, dtype=torch.int32, device=dev)
    d_len = torch.full((B + 1, n), 7, dtype=torch.int32, device=dev)
    rows = torch.tensor([nrow, begin], dtype=torch.int32, device=dev)
    for _ in range(2):  # twice: the clock carries over
        Kn.stream_rows(d_nf, rows, B, n, d_pos, d_len)
        torch.cuda.synchronize()
        assert torch.equal(d_pos[:B].cpu(), pos) and torch.equal(d_len[:B].cpu(), row_len)
        assert torch.equal(d_nf[:B].cpu(), new)
        assert int(d_nf[B]) == 7 and bool((d_pos[B] == 7).all()) and bool((d_len[B] == 7).all())
        pos, row_len, new = R.stream_rows(new, nrow, begin, n)
