"""GPU unit of qt_kv_prefix (csrc/kv_prefix.hip) through qwen_tts.kernels, against torch slicing.  The kernel only
moves data, so every result is bit-exact, fp32 and bf16.

Geometry: 2 layers, Hkv = 2, D = 64, B = 3, Lmax = 48.  One launch carries four jobs: N = 1 at offset 0, N = 33 at
offset 5 (a segment that is no multiple of a block's 16 KiB, nor of a wave), N = 7 ending exactly at Lmax, and N = 0.
Batch row 2 belongs to no job.  The session cache is filled with a sentinel first, and every byte outside the jobs'
spans -- other heads' neighbours, other batch rows -- must survive."""
import pytest
import torch

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
NL, HKV, D, B, LMAX = 2, 2, 64, 3, 48
S = 7.0
# (batch row, first position, N)
SPANS = [(0, 0, 1), (1, 5, 33), (1, LMAX - 7, 7), (0, 9, 0)]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _kv(dtype, dev, fill=None, seed=0):
    g = torch.Generator().manual_seed(seed)
    mk = (lambda: torch.randn(B, HKV, LMAX, D, generator=g).to(dtype).to(dev)) if fill is None else \
        (lambda: torch.full((B, HKV, LMAX, D), fill, dtype=dtype, device=dev))
    return [mk() for _ in range(NL)], [mk() for _ in range(NL)]


def _blocks(dtype, dev, fill=None, seed=1):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _, _, n in SPANS:
        out.append(torch.randn(2, NL, HKV, n, D, generator=g).to(dtype).to(dev) if fill is None else
                   torch.full((2, NL, HKV, n, D), fill, dtype=dtype, device=dev))
    return out


def _layers(kv):
    return list(kv[0]) + list(kv[1])   # kl = K layers, then V layers: the entry block's first two axes, flattened


def _launch(kv, blocks, direction, spans=SPANS):
    from qwen_tts import kernels as Kn
    Kn.kv_prefix([(blk, row, pos, n, direction) for blk, (row, pos, n) in zip(blocks, spans)],
                 Kn.kv_layer_table(kv), kv)
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_adopt_writes_the_spans_and_nothing_else(dtype):
    from qwen_tts import _hip
    dev = _dev()
    kv, blocks = _kv(dtype, dev, fill=S), _blocks(dtype, dev)
    want = [t.clone() for t in _layers(kv)]
    for blk, (row, pos, n) in zip(blocks, SPANS):
        for kl, w in enumerate(want):
            w[row, :, pos:pos + n] = blk.view(2 * NL, HKV, n, D)[kl]
    keep = [b.clone() for b in blocks]
    _launch(kv, blocks, _hip.KV_ADOPT)
    for kl, (got, w) in enumerate(zip(_layers(kv), want)):
        assert _same_bits(got, w), kl
        assert bool((got[2] == S).all())                 # the batch row of no job
        assert bool((got[0, :, 1:] == S).all())          # behind the one-position span
        assert bool((got[1, :, :5] == S).all()) and bool((got[1, :, 38:LMAX - 7] == S).all())
    for b, k in zip(blocks, keep):
        assert _same_bits(b, k)                          # the source side is only read


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_export_reads_the_spans(dtype):
    from qwen_tts import _hip
    dev = _dev()
    kv, blocks = _kv(dtype, dev), _blocks(dtype, dev, fill=S)
    keep = [t.clone() for t in _layers(kv)]
    _launch(kv, blocks, _hip.KV_EXPORT)
    for blk, (row, pos, n) in zip(blocks, SPANS):
        want = torch.stack([t[row, :, pos:pos + n] for t in keep]).view(2, NL, HKV, n, D)
        assert _same_bits(blk, want), (row, pos, n)
    for got, k in zip(_layers(kv), keep):
        assert _same_bits(got, k)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_export_then_adopt_elsewhere_reproduces_the_bytes(dtype):
    from qwen_tts import _hip
    dev = _dev()
    kv, blocks = _kv(dtype, dev), _blocks(dtype, dev, fill=S)
    _launch(kv, blocks, _hip.KV_EXPORT)
    other = _kv(dtype, dev, fill=S)
    moved = [(2, 3, 1), (0, 15, 33), (2, 11, 7), (1, 0, 0)]   # other rows, other offsets
    _launch(other, blocks, _hip.KV_ADOPT, moved)
    for (row, pos, n), (row2, pos2, _) in zip(SPANS, moved):
        for src, dst in zip(_layers(kv), _layers(other)):
            assert _same_bits(dst[row2, :, pos2:pos2 + n], src[row, :, pos:pos + n])
    # one launch may carry both directions: adopt into row 2 what the same launch does not export from it
    from qwen_tts import kernels as Kn
    fresh = torch.full((2, NL, HKV, 7, D), S, dtype=dtype, device=dev)
    Kn.kv_prefix([(blocks[1], 2, 0, 33, _hip.KV_ADOPT), (fresh, 1, LMAX - 7, 7, _hip.KV_EXPORT)],
                 Kn.kv_layer_table(kv), kv)
    torch.cuda.synchronize()
    assert _same_bits(fresh, blocks[2])
    for t in _layers(kv):
        assert _same_bits(t[2, :, 0:33], t[1, :, 5:38])


def test_bad_jobs_launch_nothing():
    from qwen_tts import _hip, kernels as Kn
    dev = _dev()
    kv = _kv(F32, dev, fill=S)
    layers = Kn.kv_layer_table(kv)
    blk = torch.zeros(2, NL, HKV, 7, D, device=dev)
    good = (torch.zeros(2, NL, HKV, 1, D, device=dev), 0, 0, 1, _hip.KV_ADOPT)
    for bad in ((blk, 1, LMAX - 6, 7, _hip.KV_ADOPT),     # one position past Lmax
                (blk, 1, -1, 7, _hip.KV_ADOPT), (blk, B, 0, 7, _hip.KV_ADOPT), (blk, -1, 0, 7, _hip.KV_ADOPT)):
        with pytest.raises(RuntimeError, match="SHAPE|shape"):
            Kn.kv_prefix([good, bad], layers, kv)        # the good job in front is not launched either
    with pytest.raises(RuntimeError, match="ARG|arg"):
        Kn.kv_prefix([good, (None, 1, 0, 7, _hip.KV_ADOPT)], layers, kv)
    with pytest.raises(RuntimeError, match="ARG|arg"):
        Kn.kv_prefix([(blk, 1, 0, 7, 2)], layers, kv)    # no such direction
    with pytest.raises(ValueError):
        Kn.kv_prefix([(blk, 1, 0, 6, _hip.KV_ADOPT)], layers, kv)   # the block holds 7 positions
    Kn.kv_prefix([(None, 1, 0, 0, _hip.KV_ADOPT)], layers, kv)      # N = 0 needs no block
    torch.cuda.synchronize()
    for t in _layers(kv):
        assert bool((t == S).all())
