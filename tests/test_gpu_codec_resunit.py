"""qt_codec_resunit (one launch per codec residual unit, C = 96 / 192) against the two qt_gemm implicit-GEMM calls it
replaces: bit equality, argument rejects, and CodecDecoder.decode with the fused route on against off."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

# one row; a window that is mostly padding; both sides of the tile edge (64 rows for C = 192, 128 for C = 96); several
# tiles with a ragged tail
LENGTHS = (1, 20, 63, 64, 65, 127, 128, 129, 300)
PAD = 8                                # sentinel rows on either side of x_out (8 rows keep it 16-byte aligned)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _unit(Kn, C, dil, dev, seed):
    """Seeded weights, biases and snake tables of one C -> C residual unit (k = 7 dilated conv, k = 1 conv)."""
    g = torch.Generator().manual_seed(seed)
    w1, b1 = torch.randn(C, C, 7, generator=g) * 0.05, torch.randn(C, generator=g) * 0.1
    w2, b2 = torch.randn(C, C, 1, generator=g) * 0.1, torch.randn(C, generator=g) * 0.1
    sn = [torch.exp(0.3 * torch.randn(C, generator=g)).to(dev).contiguous() for _ in range(4)]
    c1 = Kn.tile_conv(w1.to(dev), b1.to(dev), torch.bfloat16, dil)
    c2 = Kn.tile_conv(w2.to(dev), b2.to(dev), torch.bfloat16)
    return c1, (sn[0], sn[1]), c2, (sn[2], sn[3]), g


def _two_calls(Kn, _hip, x, B, L, C, dil, c1, s1, c2, s2):
    """The route the fused launch replaces: conv1 into a scratch, conv2 + residual in place, both on igemm_k.
    qt_gemm keeps convs of 16 rows or fewer off igemm_k, so for B * L <= 16 the B items are followed by filler items
    (igemm_k's tiles never span batch items) up to 17 rows or more, and the first B items are the reference."""
    Br = max(B, -(-17 // L))
    xr = x if Br == B else torch.cat([x, torch.ones((Br - B) * L, C, dtype=x.dtype, device=x.device)])
    bb = torch.empty_like(xr)
    out = xr.clone()
    k1 = dict(conv=(L, L, -6 * dil, dil), snake=s1, splitk=1)
    k2 = dict(conv=(L, L, 0, 1), snake=s2, epi=_hip.EPI_ADD, splitk=1)
    assert _hip.ROUTE_NAMES[Kn.gemm_route(xr, c1, bb, Br * L, C, C, **k1).route] == "IGEMM"
    assert _hip.ROUTE_NAMES[Kn.gemm_route(bb, c2, out, Br * L, C, C, **k2).route] == "IGEMM"
    Kn.gemm(xr, c1, bb, Br * L, C, C, **k1)
    Kn.gemm(bb, c2, out, Br * L, C, C, **k2)
    return out[:B * L].clone()


@pytest.mark.parametrize("dil", [1, 3, 9])
@pytest.mark.parametrize("C", [96, 192])
def test_resunit_equals_two_igemm_calls(C, dil):
    """Bit equality with gemm(c1, snake=s1) -> scratch -> gemm(c2, snake=s2, EPI_ADD) for B = 2 and every length of
    LENGTHS; x_in is left alone, nothing outside x_out's B * L rows is written, and a second run gives the same bits."""
    from qwen_tts import kernels as Kn, _hip
    dev = _dev()
    Kn.gemm_workspace(dev)
    c1, s1, c2, s2, g = _unit(Kn, C, dil, dev, 1000 * C + dil)
    B = 2
    for L in LENGTHS:
        x = torch.randn(B * L, C, generator=g).to(dev, torch.bfloat16)
        x0 = x.clone()
        ref = _two_calls(Kn, _hip, x, B, L, C, dil, c1, s1, c2, s2)
        assert torch.equal(x, x0)
        runs = []
        for _ in range(2):
            big = torch.full((B * L + 2 * PAD, C), -7.5, dtype=torch.bfloat16, device=dev)
            out = big[PAD:PAD + B * L]
            assert Kn.codec_resunit_supported(x, out, B, L, C, c1, s1, c2, s2)
            Kn.codec_resunit(x, out, B, L, C, c1, s1, c2, s2)
            torch.cuda.synchronize()
            assert torch.equal(out, ref), (C, dil, L, int((out != ref).sum()))
            assert bool((big[:PAD] == -7.5).all()) and bool((big[PAD + B * L:] == -7.5).all()), (C, dil, L)
            runs.append(out.clone())
        assert torch.equal(runs[0], runs[1])
        assert torch.equal(x, x0), (C, dil, L)


def test_resunit_rejects():
    """C = 64, C = 100, fp32 activations, dil = 27 (window past the staged reach) and x_out aliasing x_in: the entry
    returns its shape / dtype / argument code, qt_codec_resunit_supported is false, and nothing is launched (x_out
    keeps its sentinel)."""
    from qwen_tts import kernels as Kn, _hip
    dev = _dev()
    B, L = 2, 40
    SHAPE, DTYPE, ARG = -2, -3, -1
    assert (_hip.ERRORS[ARG], _hip.ERRORS[SHAPE], _hip.ERRORS[DTYPE]) == ("bad argument", "bad shape", "unsupported dtype")
    cases = [(64, 1, torch.bfloat16, False, SHAPE), (100, 1, torch.bfloat16, False, SHAPE),
             (96, 1, torch.float32, False, DTYPE), (96, 27, torch.bfloat16, False, SHAPE),
             (96, 3, torch.bfloat16, True, ARG)]
    for C, dil, dt, alias, want in cases:
        c1, s1, c2, s2, g = _unit(Kn, C, dil, dev, C + dil)
        x = torch.randn(B * L, C, generator=g).to(dev, dt)
        x0 = x.clone()
        out = x if alias else torch.full((B * L, C), -7.5, dtype=dt, device=dev)
        a = Kn._codec_resunit_args(x, out, B, L, C, c1, s1, c2, s2)
        assert _hip.lib().qt_codec_resunit_supported(ctypes.byref(a)) == 0, (C, dil, dt, alias)
        assert not Kn.codec_resunit_supported(x, out, B, L, C, c1, s1, c2, s2)
        assert _hip.lib().qt_codec_resunit(ctypes.byref(a), _hip.stream()) == want, (C, dil, dt, alias)
        torch.cuda.synchronize()
        assert torch.equal(x, x0)
        if not alias:
            assert bool((out == -7.5).all())
    # the same unit with a buffer of its own runs
    c1, s1, c2, s2, g = _unit(Kn, 96, 3, dev, 99)
    x = torch.randn(B * L, 96, generator=g).to(dev, torch.bfloat16)
    assert Kn.codec_resunit_supported(x, torch.empty_like(x), B, L, 96, c1, s1, c2, s2)


def test_decoder_fused_units_equal_two_call_route(monkeypatch):
    """CodecDecoder.decode at the full-dims preset (synthetic weights, B = 2, lengths 3 and 2) with fuse_units on
    equals the same with it off, bit for bit, and the on side went through qt_codec_resunit."""
    from oracle import codec_param_specs, load_preset, synth_state_dict
    from qwen_tts import kernels as Kn
    from qwen_tts.codec import CodecDecoder
    dev = _dev()
    _, ccfg = load_preset("1.7b-customvoice")
    W = {k: torch.from_numpy(v) for k, v in synth_state_dict(codec_param_specs(ccfg), threads=16).items()}
    dec = CodecDecoder(ccfg, W, dtype="bf16", device=str(dev))
    assert dec.fuse_units
    g = torch.Generator().manual_seed(5)
    codes = torch.randint(1, 2048, (2, 3, 16), generator=g)
    codes[1, 2] = 0  # second row: length 2
    calls = []
    real = Kn.codec_resunit

    def counted(x_in, x_out, B, L, C, *a, **kw):
        calls.append((C, L))
        return real(x_in, x_out, B, L, C, *a, **kw)

    monkeypatch.setattr(Kn, "codec_resunit", counted)
    on = dec.decode(codes.to(dev))
    n_on = len(calls)
    assert n_on and {c for c, _ in calls} <= {96, 192}
    dec.fuse_units = False
    off = dec.decode(codes.to(dev))
    assert len(calls) == n_on  # the off side never enters the fused kernel
    assert [w.shape[0] for w in on] == [3 * 1920 - 555, 2 * 1920] == [w.shape[0] for w in off]
    for a, b in zip(on, off):
        assert torch.equal(a, b)
    off_dec = CodecDecoder(ccfg, W, dtype="bf16", device=str(dev), fuse_units=False)
    for a, b in zip(on, off_dec.decode(codes.to(dev))):
        assert torch.equal(a, b)
    assert len(calls) == n_on
