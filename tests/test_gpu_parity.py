"""GPU parity: the HIP path (through the C ABI) against the oracle and the reference golden vectors.

Tolerances: codebook indices bit-exact (fp32 parity mode, greedy); PCM |diff| <= 2e-4 abs in fp32 mode,
and in bf16 mode a relative L2 error <= 5e-2 (bf16 weights + activations vs the fp32 reference).
Kernel unit tests compare against plain torch fp32 on the same seeded inputs.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _route(Kn, *args, **kw):
    """(route name, plan) of the Kn.gemm call with these arguments: qt_gemm_route, nothing is launched"""
    from qwen_tts import _hip
    info = Kn.gemm_route(*args, **kw)
    return _hip.ROUTE_NAMES[info.route], info


# ------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("M,N,K", [(1, 64, 64), (8, 256, 512), (16, 96, 160), (37, 128, 96), (130, 48, 64)])
def test_gemm_linear(dtype, M, N, K):
    from qwen_tts import kernels as Kn
    dev = _dev()
    g = torch.Generator(device="cpu").manual_seed(M * 1000 + N)
    W = torch.randn(N, K, generator=g) * 0.1
    A = torch.randn(M, K, generator=g)
    b = torch.randn(N, generator=g) * 0.1
    gamma = 1 + 0.1 * torch.randn(K, generator=g)
    t = Kn.tile_linear(W.to(dev), dtype, b.to(dev))
    out = torch.zeros(M, N, device=dev)
    # a gamma vector keeps the call off the GEMV / tiled GEMMs: the gemm_wt fallbacks (1 x 8 to 16 rows, 4 x 4 above 32)
    assert _route(Kn, A.to(dev), t, out, M, K, N, gamma=gamma.to(dev), eps=1e-6)[0] == ("WT_1x8" if M <= 16 else "WT_4x4")
    Kn.gemm(A.to(dev), t, out, M, K, N, gamma=gamma.to(dev), eps=1e-6)
    Wr = W.to(dtype).float()
    h = A * torch.rsqrt(A.pow(2).mean(-1, keepdim=True) + 1e-6) * gamma
    if dtype == torch.bfloat16:
        h = (A * gamma).to(dtype).float() * torch.rsqrt(A.pow(2).mean(-1, keepdim=True) + 1e-6)
    ref = h @ Wr.T + b
    tol = 1e-4 if dtype == torch.float32 else 2e-2
    torch.testing.assert_close(out.cpu(), ref, atol=tol, rtol=tol)
    # RMSNorm gamma folded into W at load time (the engine's form; decode GEMV fast path for M <= 16)
    tf = Kn.tile_linear(W.to(dev), dtype, b.to(dev), gamma=gamma.to(dev))
    out2 = torch.zeros(M, N, device=dev)
    Kn.gemm(A.to(dev), tf, out2, M, K, N, rms=True, eps=1e-6)
    Wf = (W * gamma).to(dtype).float()
    Aa = A.to(dtype).float() if dtype == torch.bfloat16 else A
    ref2 = (Aa @ Wf.T) * torch.rsqrt(A.pow(2).mean(-1, keepdim=True) + 1e-6) + b
    torch.testing.assert_close(out2.cpu(), ref2, atol=tol, rtol=tol)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("M,N,K", [(8, 1024, 3072), (3, 176, 1024), (16, 64, 512), (8, 6144, 1024), (5, 4400, 2048)])
def test_gemv_splitk_deterministic(dtype, M, N, K):
    """Decode GEMV split-K (last-arriving block reduces partials in split order): matches the unsplit
    kernel to fp32 rounding, is bitwise reproducible, and keeps RMSNorm / bias / residual epilogues."""
    from qwen_tts import kernels as Kn, _hip
    dev = _dev()
    Kn.gemm_workspace(dev)
    g = torch.Generator().manual_seed(N + K)
    W = torch.randn(N, K, generator=g) * 0.05
    A = torch.randn(M, K, generator=g).to(dev)
    b = (torch.randn(N, generator=g) * 0.1).to(dev)
    t = Kn.tile_linear(W.to(dev), dtype, b)
    x0 = torch.randn(M, N, generator=g).to(dev)
    outs = {}
    # the plan: bf16 weights run 5+ rows of <= 128 column tiles as row groups (4 groups to 64 tiles, else 2) without
    # split-K; otherwise K splits by the forced factor (at most 16 and half the k tiles), and on its own only over
    # deep K (more than 4 k tiles per wave) on < 256 column tiles, by 2
    ntl, ktl = (N + 15) // 16, K // Kn.KT_OF[dtype]
    rg = (4 if ntl <= 64 else 2 if ntl <= 128 else 1) if dtype == torch.bfloat16 and M > 4 else 1
    wpb = 16 if ktl >= 48 else 8 if ktl >= 16 else 4
    auto = 2 if -(-ktl // wpb) > 4 and ntl < 256 else 1
    splits = set()
    for sk in (1, 2, 3, 4, 8, 0):
        for rms in (False, True):
            o = x0.clone()
            name, plan = _route(Kn, A, t, o, M, K, N, rms=rms, eps=1e-6, epi=_hip.EPI_ADD, splitk=sk)
            want_ks = 1 if rg > 1 else max(1, min(sk if sk else auto, 16, ktl // 2))
            assert (name, plan.mr, plan.ks, plan.ws_split) == ("GEMV", -(-M // rg), want_ks, int(want_ks > 1))
            splits.add(plan.ks)
            Kn.gemm(A, t, o, M, K, N, rms=rms, eps=1e-6, epi=_hip.EPI_ADD, splitk=sk)
            o2 = x0.clone()
            Kn.gemm(A, t, o2, M, K, N, rms=rms, eps=1e-6, epi=_hip.EPI_ADD, splitk=sk)
            assert torch.equal(o, o2), f"split-K {sk} not reproducible"
            outs[(sk, rms)] = o.cpu()
    Wr = W.to(dtype).float()
    Aa = A.cpu().to(dtype).float() if dtype == torch.bfloat16 else A.cpu()
    for rms in (False, True):
        ref = Aa @ Wr.T
        if rms:
            ref = ref * torch.rsqrt(A.cpu().pow(2).mean(-1, keepdim=True) + 1e-6)
        ref = x0.cpu() + ref + b.cpu()
        for sk in (1, 2, 3, 4, 8, 0):
            torch.testing.assert_close(outs[(sk, rms)], ref, atol=2e-4, rtol=2e-4)
            torch.testing.assert_close(outs[(sk, rms)], outs[(1, rms)], atol=2e-5, rtol=2e-5)
    assert splits == ({1} if rg > 1 else {1, 2, 3, 4, 8})  # (row-group shapes never split: see the plan above)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("H,I,sk", [(128, 192, 0), (256, 3072, 0), (256, 3072, 2)])
def test_gemm_swiglu_and_residual(dtype, H, I, sk):
    """SwiGLU epilogue (gate/up interleaved tiles, wide grid) + residual down-proj (auto / forced split-K)."""
    from qwen_tts import kernels as Kn, _hip
    dev = _dev()
    g = torch.Generator().manual_seed(3)
    M = 8
    gate, up, down = (torch.randn(I, H, generator=g) * 0.05, torch.randn(I, H, generator=g) * 0.05,
                      torch.randn(H, I, generator=g) * 0.05)
    x = torch.randn(M, H, generator=g)
    tgu, td = Kn.tile_swiglu(gate.to(dev), up.to(dev), dtype), Kn.tile_linear(down.to(dev), dtype)
    h = torch.zeros(M, I, device=dev)
    Kn.gemm(x.to(dev), tgu, h, M, H, I, epi=_hip.EPI_SWIGLU, splitk=sk)
    xr = x.to(dev).clone()
    Kn.gemm(h, td, xr, M, I, H, epi=_hip.EPI_ADD, splitk=sk)
    c = lambda w: w.to(dtype).float()  # noqa: E731
    xa = x.to(dtype).float() if dtype == torch.bfloat16 else x
    hr = torch.nn.functional.silu(xa @ c(gate).T) * (xa @ c(up).T)
    ha = hr.to(dtype).float() if dtype == torch.bfloat16 else hr
    ref = x + ha @ c(down).T
    tol = 1e-4 if dtype == torch.float32 else 3e-2
    torch.testing.assert_close(h.cpu(), hr, atol=tol, rtol=tol)
    torch.testing.assert_close(xr.cpu(), ref, atol=tol, rtol=tol)


@pytest.mark.parametrize("cin,cout,k,dil", [(32, 48, 3, 1), (64, 16, 7, 3), (24, 40, 1, 1), (96, 1, 7, 1)])
def test_gemm_causal_conv(cin, cout, k, dil):
    from qwen_tts import kernels as Kn
    dev = _dev()
    g = torch.Generator().manual_seed(cin + cout)
    B, T = 2, 37
    w, b = torch.randn(cout, cin, k, generator=g) * 0.1, torch.randn(cout, generator=g) * 0.1
    x = torch.randn(B, cin, T, generator=g)
    ref = torch.nn.functional.conv1d(torch.nn.functional.pad(x, ((k - 1) * dil, 0)), w, b, dilation=dil)
    t = Kn.tile_conv(w.to(dev), b.to(dev), torch.float32, dil)
    xl = x.permute(0, 2, 1).contiguous().to(dev)
    out = torch.zeros(B * T, cout, device=dev)
    # one output channel: conv_n1_k; the other fp32-weight convs of 74 rows: the 4 x 4 gemm_wt fallback
    assert _route(Kn, xl, t, out, B * T, cin, cout, conv=(T, T, -(k - 1) * dil, dil))[0] == \
        ("CONV_N1" if cout == 1 else "WT_4x4")
    Kn.gemm(xl, t, out, B * T, cin, cout, conv=(T, T, -(k - 1) * dil, dil))
    torch.testing.assert_close(out.view(B, T, cout).permute(0, 2, 1).cpu(), ref, atol=1e-4, rtol=1e-4)


@pytest.mark.parametrize("cin,cout,s", [(32, 16, 2), (64, 32, 5), (16, 8, 3)])
def test_gemm_transposed_conv(cin, cout, s):
    from qwen_tts import kernels as Kn
    dev = _dev()
    g = torch.Generator().manual_seed(s)
    B, T = 2, 11
    x = torch.randn(B, cin, T, generator=g)
    for k in (s, 2 * s):
        w, b = torch.randn(cin, cout, k, generator=g) * 0.1, torch.randn(cout, generator=g) * 0.1
        y = torch.nn.functional.conv_transpose1d(x, w, b, stride=s)
        pad = k - s
        ref = y[..., pad:y.shape[-1] - pad]
        t = Kn.tile_transconv(w.to(dev), b.to(dev), torch.float32, s)
        tout = T if k == s else T - 1
        out = torch.zeros(B * tout * s, cout, device=dev)
        xl = x.permute(0, 2, 1).contiguous().to(dev)
        assert _route(Kn, xl, t, out, B * tout, cin, s * cout, conv=(T, tout, 0, 1))[0] == "WT_2x8"  # 20 / 22 rows, fp32
        Kn.gemm(xl, t, out, B * tout, cin, s * cout, conv=(T, tout, 0, 1))
        torch.testing.assert_close(out.view(B, tout * s, cout).permute(0, 2, 1).cpu(), ref, atol=1e-4, rtol=1e-4)


def _bf(t):
    return t.to(torch.bfloat16).float()


def _snake_ref(x, al, ib):  # channels on dim 1 (NCT), same fp32 formula as the kernels
    return x + ib[None, :, None] * torch.sin(x * al[None, :, None]) ** 2


@pytest.mark.parametrize("cin,cout,k,dil,T", [(64, 96, 7, 9, 300), (96, 64, 7, 1, 129), (32, 48, 1, 1, 257),
                                             (64, 768, 7, 3, 140), (160, 32, 7, 9, 64)])
@pytest.mark.parametrize("snake", [False, True])
def test_igemm_conv_bf16(cin, cout, k, dil, T, snake):
    """LDS-tiled implicit-GEMM conv (bf16 weights/activations, several 128-row tiles per batch item, ragged
    tail, window up to 182 rows) with optional fused SnakeBeta, against torch conv1d on the same roundings."""
    from qwen_tts import kernels as Kn, _hip
    dev = _dev()
    g = torch.Generator().manual_seed(cin * 7 + cout + k + dil)
    B = 3
    w, b = torch.randn(cout, cin, k, generator=g) * 0.05, torch.randn(cout, generator=g) * 0.1
    x = _bf(torch.randn(B, cin, T, generator=g))
    al, ib = torch.exp(0.3 * torch.randn(cin, generator=g)), torch.exp(-0.3 * torch.randn(cin, generator=g))
    xin = _bf(_snake_ref(x, al, ib)) if snake else x
    ref = torch.nn.functional.conv1d(torch.nn.functional.pad(xin, ((k - 1) * dil, 0)), _bf(w), b, dilation=dil)
    res = torch.randn(B, cout, T, generator=g)
    t = Kn.tile_conv(w.to(dev), b.to(dev), torch.bfloat16, dil)
    xl = x.permute(0, 2, 1).contiguous().to(dev, torch.bfloat16)
    Kn.gemm_workspace(dev)
    for sk in (1, 0):  # splitk=1: the implicit GEMM; 0: windows of <= 1024 rows as im2col + the linear GEMMs
        out = res.permute(0, 2, 1).contiguous().reshape(B * T, cout).to(dev)
        kw = dict(conv=(T, T, -(k - 1) * dil, dil), epi=_hip.EPI_ADD,
                  snake=(al.to(dev), ib.to(dev)) if snake else None, splitk=sk)
        assert _route(Kn, xl, t, out, B * T, cin, cout, **kw)[0] == ("IGEMM" if sk == 1 or B * T > 1024 else "IM2COL")
        Kn.gemm(xl, t, out, B * T, cin, cout, **kw)
        got = out.view(B, T, cout).permute(0, 2, 1).cpu()
        torch.testing.assert_close(got, ref + res, atol=2e-3, rtol=2e-3)


@pytest.mark.parametrize("cin,cout,k,dil,T,B,elu", [(1024, 1536, 7, 1, 6, 8, False), (192, 96, 7, 9, 30, 2, False),
                                                   (64, 40, 3, 3, 17, 3, True), (96, 64, 1, 1, 40, 4, False)])
@pytest.mark.parametrize("snake", [False, True])
def test_short_window_conv_im2col(cin, cout, k, dil, T, B, elu, snake):
    """Short conv windows (<= 256 rows: a streamed codec window's early stages) go through im2col + the linear GEMMs:
    same result as the implicit-GEMM path (splitk=1 keeps igemm_k) and as torch conv1d on the same bf16 operands."""
    from qwen_tts import kernels as Kn, _hip
    dev = _dev()
    Kn.gemm_workspace(dev)
    g = torch.Generator().manual_seed(cin + cout + k + T)
    w, b = torch.randn(cout, cin, k, generator=g) * 0.03, torch.randn(cout, generator=g) * 0.1
    x = _bf(torch.randn(B, cin, T, generator=g))
    al, ib = torch.exp(0.3 * torch.randn(cin, generator=g)), torch.exp(-0.3 * torch.randn(cin, generator=g))
    xin = torch.nn.functional.elu(x) if elu else x
    xin = _bf(_snake_ref(xin, al, ib)) if snake else _bf(xin)
    ref = torch.nn.functional.conv1d(torch.nn.functional.pad(xin, ((k - 1) * dil, 0)), _bf(w), b, dilation=dil)
    t = Kn.tile_conv(w.to(dev), b.to(dev), torch.bfloat16, dil)
    xl = x.permute(0, 2, 1).contiguous().to(dev, torch.bfloat16)
    outs = []
    for sk in (0, 1):
        out = torch.zeros(B * T, cout, device=dev)
        kw = dict(conv=(T, T, -(k - 1) * dil, dil), splitk=sk, snake=(al.to(dev), ib.to(dev)) if snake else None,
                  a_act=_hip.AACT_ELU if elu else _hip.AACT_NONE)
        name, plan = _route(Kn, xl, t, out, B * T, cin, cout, **kw)
        assert name == ("IGEMM" if sk else "IM2COL")
        if not sk:  # the 48-row window of 1536 x 7168 weights on the split-K prefill GEMM, the others on the GEMV
            assert _hip.ROUTE_NAMES[plan.inner] == ("PF2" if cout == 1536 else "GEMV")
        Kn.gemm(xl, t, out, B * T, cin, cout, **kw)
        outs.append(out.view(B, T, cout).permute(0, 2, 1).cpu())
    torch.testing.assert_close(outs[0], ref, atol=3e-3, rtol=3e-3)
    torch.testing.assert_close(outs[0], outs[1], atol=1e-4, rtol=1e-4)


@pytest.mark.parametrize("s,T", [pytest.param(2, 150, id="2"), pytest.param(5, 150, id="5"), pytest.param(8, 150, id="8"),
                                 (2, 514), (5, 514), (8, 514)])
def test_igemm_transposed_conv_bf16(s, T):
    """2-tap transposed conv on igemm_k.  The 298 rows of T = 150 stay on it only while no workspace has been allocated
    in the process (with one, they are a short window: im2col + gemm_pf2_k); the 1026 rows of T = 514 always do."""
    from qwen_tts import kernels as Kn
    dev = _dev()
    g = torch.Generator().manual_seed(s + 100)
    B, cin, cout = 2, 64, 48
    x = _bf(torch.randn(B, cin, T, generator=g))
    w, b = torch.randn(cin, cout, 2 * s, generator=g) * 0.05, torch.randn(cout, generator=g) * 0.1
    y = torch.nn.functional.conv_transpose1d(x, _bf(w), b, stride=s)
    ref = y[..., s:y.shape[-1] - s]
    t = Kn.tile_transconv(w.to(dev), b.to(dev), torch.bfloat16, s)
    out = torch.zeros(B * (T - 1) * s, cout, device=dev)
    xl = x.permute(0, 2, 1).contiguous().to(dev, torch.bfloat16)
    short = T == 150 and Kn.active_workspace(dev) is not None
    assert _route(Kn, xl, t, out, B * (T - 1), cin, s * cout, conv=(T, T - 1, 0, 1))[0] == ("IM2COL" if short else "IGEMM")
    Kn.gemm(xl, t, out, B * (T - 1), cin, s * cout, conv=(T, T - 1, 0, 1))
    torch.testing.assert_close(out.view(B, (T - 1) * s, cout).permute(0, 2, 1).cpu(), ref, atol=2e-3, rtol=2e-3)


@pytest.mark.parametrize("M,H,I", [(128, 256, 384), (300, 256, 384), (700, 288, 400), (1100, 512, 1024)])
def test_igemm_linear_rms_swiglu_bf16(M, H, I):
    """Large-M linears on the tiled paths (ragged row / column / k tiles): folded-gamma RMSNorm rows + SwiGLU epilogue on
    fp32 A (igemm_k), residual add on bf16 A (gemm_pf2_k; gemm_pf_k, 128 x 128 / 128 x 64 tiles, where K % 64 != 0:
    the 700-row case).  The 128-row case is below both: its 768- and 256-column outputs run the row-group GEMV."""
    from qwen_tts import kernels as Kn, _hip
    dev = _dev()
    g = torch.Generator().manual_seed(M)
    x = torch.randn(M, H, generator=g)
    gamma = 1 + 0.1 * torch.randn(H, generator=g)
    gate, up = torch.randn(I, H, generator=g) * 0.05, torch.randn(I, H, generator=g) * 0.05
    tgu = Kn.tile_swiglu(gate.to(dev), up.to(dev), torch.bfloat16, gamma=gamma.to(dev))
    h = torch.zeros(M, I, device=dev)
    assert _route(Kn, x.to(dev), tgu, h, M, H, I, rms=True, eps=1e-6, epi=_hip.EPI_SWIGLU)[0] == \
        ("GEMV" if M == 128 else "IGEMM")
    Kn.gemm(x.to(dev), tgu, h, M, H, I, rms=True, eps=1e-6, epi=_hip.EPI_SWIGLU)
    rs = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + 1e-6)
    xa = _bf(x)
    hg = (xa @ _bf(gate * gamma).T) * rs
    hu = (xa @ _bf(up * gamma).T) * rs
    torch.testing.assert_close(h.cpu(), torch.nn.functional.silu(hg) * hu, atol=2e-3, rtol=2e-3)
    down = torch.randn(H, I, generator=g) * 0.05
    td = Kn.tile_linear(down.to(dev), torch.bfloat16)
    hb = h.to(torch.bfloat16)
    xr = x.to(dev).clone()
    assert _route(Kn, hb, td, xr, M, I, H, epi=_hip.EPI_ADD)[0] == ("GEMV" if M == 128 else "PF" if I % 64 else "PF2")
    Kn.gemm(hb, td, xr, M, I, H, epi=_hip.EPI_ADD)
    torch.testing.assert_close(xr.cpu(), x + _bf(hb.cpu().float()) @ _bf(down).T, atol=2e-3, rtol=2e-3)


@pytest.mark.parametrize("M,N,K,mode", [
    (2900, 3072, 512, "swiglu"), (2900, 3072, 512, "rms"), (650, 11856, 512, "swiglu"),   # cfg 9: 256 x 160 ping-pong
    (680, 12288, 2048, "swiglu"), (700, 11000, 512, "add"),
    (520, 8192, 1024, "rms"), (520, 8192, 1024, "add"), (1100, 4096, 512, "rms"),          # cfg 4: 256 x 128, 8 waves
    (300, 1000, 640, "add"), (300, 1008, 640, "swiglu"), (131, 2048, 6144, "add_plain"),   # cfg 11: 64 x 96, 4 waves
    (680, 2048, 2048, "add_noshadow"),
    (1000, 2048, 512, "add"), (1000, 2056, 512, "add_noshadow"),                           # cfg 3: 128 x 64
    (1300, 2048, 1024, "add"), (1300, 2048, 1024, "add_plain"), (1300, 2056, 1024, "add_noshadow"),  # cfg 21:
    (680, 4096, 2048, "rms"), (333, 6160, 1024, "swiglu"), (1300, 2048, 512, "add"),       #   128 x 128 ping-pong
    (1536, 8192, 1024, "swiglu"), (1700, 8190, 1024, "rms"), (2900, 4096, 1024, "add_noshadow"),  # cfg 23: 256 x 256
    # ping-pong with 1..3 K stages (the two groups' prologue / stagger / drain with fewer stages than LDS slots)
    (300, 4096, 64, "rms"), (680, 4096, 192, "add"), (700, 12288, 64, "swiglu"), (700, 12288, 192, "swiglu"),
    (1600, 8192, 128, "rms"), (3000, 8192, 192, "add_noshadow")])
def test_prefill_gemm_pf2_bf16(M, N, K, mode):
    """Deep-pipelined prefill GEMM (gemm_pf2_k: LDS-DMA operands, NS stages in flight) on bf16 A, every tile
    configuration the shape rule picks (gemm_pf2.hip pf2_pick: 256 x 256, 256 x 160 and 128 x 128 ping-pong -- two staggered
    groups of 4 waves --, 256 x 128 / 8 waves, 64 x 96 / 4 waves, 128 x 64 / 4 waves), interior and ragged row /
    column tiles, every epilogue form: RMSNorm rows from the bf16 A values (plain store), SwiGLU, residual add with
    bias (generic form), without bias with / without the bf16 shadow (out2) -- vs torch fp32 on the same bf16-rounded
    operands."""
    from qwen_tts import kernels as Kn, _hip
    dev = _dev()
    g = torch.Generator().manual_seed(M + N + K)
    A = torch.randn(M, K, generator=g).to(torch.bfloat16)
    Af = A.float()
    rs = torch.rsqrt(Af.pow(2).mean(-1, keepdim=True) + 1e-6)
    if mode == "swiglu":
        I = N // 2
        gate, up = torch.randn(I, K, generator=g) * 0.05, torch.randn(I, K, generator=g) * 0.05
        gamma = 1 + 0.1 * torch.randn(K, generator=g)
        t = Kn.tile_swiglu(gate.to(dev), up.to(dev), torch.bfloat16, gamma=gamma.to(dev))
        out = torch.zeros(M, I, device=dev, dtype=torch.bfloat16)
        assert _route(Kn, A.to(dev), t, out, M, K, I, rms=True, eps=1e-6, epi=_hip.EPI_SWIGLU)[0] == "PF2"
        Kn.gemm(A.to(dev), t, out, M, K, I, rms=True, eps=1e-6, epi=_hip.EPI_SWIGLU)
        ref = torch.nn.functional.silu((Af @ _bf(gate * gamma).T) * rs) * ((Af @ _bf(up * gamma).T) * rs)
        torch.testing.assert_close(out.float().cpu(), ref, atol=1e-2, rtol=1e-2)
        return
    W = torch.randn(N, K, generator=g) * 0.05
    if mode == "rms":
        gamma = 1 + 0.1 * torch.randn(K, generator=g)
        t = Kn.tile_linear(W.to(dev), torch.bfloat16, gamma=gamma.to(dev))
        out = torch.zeros(M, N, device=dev)
        assert _route(Kn, A.to(dev), t, out, M, K, N, rms=True, eps=1e-6)[0] == "PF2"
        Kn.gemm(A.to(dev), t, out, M, K, N, rms=True, eps=1e-6)
        ref = (Af @ _bf(W * gamma).T) * rs
        torch.testing.assert_close(out.cpu(), ref, atol=2e-3, rtol=2e-3)
        return
    b = torch.randn(N, generator=g) * 0.1 if mode == "add" else None
    t = Kn.tile_linear(W.to(dev), torch.bfloat16, None if b is None else b.to(dev))
    x0 = torch.randn(M, N, generator=g)
    out = x0.to(dev).clone()
    o16 = None if mode == "add_noshadow" else torch.zeros(M, N, device=dev, dtype=torch.bfloat16)
    assert _route(Kn, A.to(dev), t, out, M, K, N, epi=_hip.EPI_ADD, out2=o16)[0] == "PF2"
    Kn.gemm(A.to(dev), t, out, M, K, N, epi=_hip.EPI_ADD, out2=o16)
    ref = x0 + Af @ _bf(W).T + (0 if b is None else b)
    torch.testing.assert_close(out.cpu(), ref, atol=2e-3, rtol=2e-3)
    if o16 is not None:
        torch.testing.assert_close(o16.float().cpu(), _bf(out.cpu()), atol=0, rtol=0)


@pytest.mark.parametrize("M,N,K,mode", [(200, 2048, 6144, "add"), (200, 2048, 2048, "add_shadow"),
                                        (300, 1024, 3072, "rms"), (256, 1000, 2048, "add"), (700, 2048, 6144, "add"),
                                        (680, 2048, 6144, "add_shadow"), (680, 1040, 3072, "rms"),
                                        (400, 2048, 4096, "add"), (700, 2048, 4160, "add")])
def test_prefill_gemm_pf2_splitk(M, N, K, mode):
    """gemm_pf2_k split-K (narrow outputs whose tiles leave most CUs idle: K split over up to 4 blocks per tile of
    the 4-wave kernels, over 2 per 128 x 128 ping-pong tile from 256 rows (cfg 22); the last split to arrive sums every
    split's record in split order): matches the unsplit kernel (splitk=1) to fp32 rounding and torch fp32, is bitwise
    reproducible, keeps the RMS rows / residual / bf16 shadow epilogues."""
    from qwen_tts import kernels as Kn, _hip
    dev = _dev()
    Kn.gemm_workspace(dev)
    g = torch.Generator().manual_seed(M + N + K + 1)
    A = torch.randn(M, K, generator=g).to(torch.bfloat16)
    Af = A.float()
    W = torch.randn(N, K, generator=g) * 0.05
    if mode == "rms":
        gamma = 1 + 0.1 * torch.randn(K, generator=g)
        t = Kn.tile_linear(W.to(dev), torch.bfloat16, gamma=gamma.to(dev))
        ref = (Af @ _bf(W * gamma).T) * torch.rsqrt(Af.pow(2).mean(-1, keepdim=True) + 1e-6)
        outs = []
        for sk in (0, 0, 1):
            o = torch.zeros(M, N, device=dev)
            name, plan = _route(Kn, A.to(dev), t, o, M, K, N, rms=True, eps=1e-6, splitk=sk)
            assert name == "PF2" and (plan.pf2_ks > 1) == (sk == 0) == bool(plan.ws_split)
            Kn.gemm(A.to(dev), t, o, M, K, N, rms=True, eps=1e-6, splitk=sk)
            outs.append((o.cpu(), None))
    else:
        t = Kn.tile_linear(W.to(dev), torch.bfloat16)
        x0 = torch.randn(M, N, generator=g)
        ref = x0 + Af @ _bf(W).T
        outs = []
        for sk in (0, 0, 1):
            o = x0.to(dev).clone()
            o16 = torch.zeros(M, N, device=dev, dtype=torch.bfloat16) if mode == "add_shadow" else None
            name, plan = _route(Kn, A.to(dev), t, o, M, K, N, epi=_hip.EPI_ADD, out2=o16, splitk=sk)
            assert name == "PF2" and (plan.pf2_ks > 1) == (sk == 0) == bool(plan.ws_split)
            Kn.gemm(A.to(dev), t, o, M, K, N, epi=_hip.EPI_ADD, out2=o16, splitk=sk)
            outs.append((o.cpu(), None if o16 is None else o16.cpu()))
    torch.testing.assert_close(outs[0][0], ref, atol=2e-3, rtol=2e-3)
    assert torch.equal(outs[0][0], outs[1][0]), "split-K not reproducible"
    torch.testing.assert_close(outs[0][0], outs[2][0], atol=2e-5, rtol=2e-5)
    if outs[0][1] is not None:
        assert torch.equal(outs[0][1].float(), _bf(outs[0][0]))


@pytest.mark.parametrize("M", [17, 40, 80, 131, 200, 256])
@pytest.mark.parametrize("N,K,mode", [(2048, 2048, "add"), (1000, 640, "add_noshadow"), (4096, 512, "swiglu"),
                                      (4096, 1024, "rms"), (1024, 3072, "add_plain"), (12288, 512, "swiglu")])
def test_skinny_gemm_bf16(M, N, K, mode):
    """17..256-row GEMMs on bf16 A through qt_gemm's skinny routing (gemm_sk_k: every row in one block per 16-column
    tile, waves split K; the row-group GEMV; gemm_pf2_k below its old row floor): RMSNorm rows, SwiGLU, residual add
    with bias / without, with / without the bf16 shadow, ragged row fragments and columns -- vs torch fp32 on the same
    bf16-rounded operands; on gemm_sk_k and the row-group GEMV every row's bits are independent of M (a request
    prefilled alone == inside a batch)."""
    from qwen_tts import kernels as Kn, _hip
    dev = _dev()
    g = torch.Generator().manual_seed(M * 7 + N + K)
    A = torch.randn(M, K, generator=g).to(torch.bfloat16)
    Af = A.float()
    rs = torch.rsqrt(Af.pow(2).mean(-1, keepdim=True) + 1e-6)
    Ad = A.to(dev)
    if mode == "swiglu":
        I = N // 2
        gate, up = torch.randn(I, K, generator=g) * 0.05, torch.randn(I, K, generator=g) * 0.05
        gamma = 1 + 0.1 * torch.randn(K, generator=g)
        t = Kn.tile_swiglu(gate.to(dev), up.to(dev), torch.bfloat16, gamma=gamma.to(dev))
        call = lambda f, m: f(Ad, t, outs[m], abs(m), K, I, rms=True, eps=1e-6, epi=_hip.EPI_SWIGLU)  # noqa: E731
        outs = {m: torch.zeros(abs(m), I, device=dev, dtype=torch.bfloat16) for m in (M, -17)}
        ref = torch.nn.functional.silu((Af @ _bf(gate * gamma).T) * rs) * ((Af @ _bf(up * gamma).T) * rs)
        tol = 1e-2
    elif mode == "rms":
        W = torch.randn(N, K, generator=g) * 0.05
        gamma = 1 + 0.1 * torch.randn(K, generator=g)
        t = Kn.tile_linear(W.to(dev), torch.bfloat16, gamma=gamma.to(dev))
        outs = {m: torch.zeros(abs(m), N, device=dev) for m in (M, -17)}
        call = lambda f, m: f(Ad, t, outs[m], abs(m), K, N, rms=True, eps=1e-6)  # noqa: E731
        ref = (Af @ _bf(W * gamma).T) * rs
        tol = 2e-3
    else:
        W = torch.randn(N, K, generator=g) * 0.05
        b = torch.randn(N, generator=g) * 0.1 if mode == "add" else None
        t = Kn.tile_linear(W.to(dev), torch.bfloat16, None if b is None else b.to(dev))
        x0 = torch.randn(M, N, generator=g)
        outs = {m: x0[:abs(m)].to(dev).clone() for m in (M, -17)}
        o16 = {m: (None if mode == "add_noshadow" else torch.zeros(abs(m), N, device=dev, dtype=torch.bfloat16))
               for m in (M, -17)}
        call = lambda f, m: f(Ad, t, outs[m], abs(m), K, N, epi=_hip.EPI_ADD, out2=o16[m])  # noqa: E731
        ref = x0 + Af @ _bf(W).T + (0 if b is None else b)
        tol = 2e-3
    # qt_gemm's 17..256-row rule (gemm_route.h): gemm_sk_k / row-group GEMV rows do not depend on M
    nw = N

    def route(m):
        if nw >= 4096:
            return "sk" if m <= 48 and nw * K <= (8 << 20) else "pf2"
        return "gemv" if m * nw * K <= (400 << 20) else "pf2"
    for m in (M, -17):  # the first 17 rows alone (key -17)
        assert _hip.ROUTE_NAMES[call(Kn.gemm_route, m).route] == route(abs(m)).upper()
        call(Kn.gemm, m)
    got = outs[M].float().cpu()
    torch.testing.assert_close(got, ref, atol=tol, rtol=tol)
    if route(M) == route(17) != "pf2":
        assert torch.equal(outs[-17].float().cpu(), got[:17]), "row results depend on M"
    if mode in ("add", "add_plain"):
        torch.testing.assert_close(o16[M].float().cpu(), _bf(outs[M].cpu()), atol=0, rtol=0)


@pytest.mark.parametrize("D,hq,hkv,window", [(128, 16, 8, 0), (16, 4, 2, 0), (64, 4, 4, 5)])
def test_qkv_post_and_attention(D, hq, hkv, window):
    from qwen_tts import kernels as Kn
    from oracle.talker import apply_rope, rmsnorm, rope_cos_sin
    dev = _dev()
    g = torch.Generator().manual_seed(D + hq)
    B, L = 3, 23
    qkv = torch.randn(B * L, (hq + 2 * hkv) * D, generator=g)
    qn, kn = 1 + 0.1 * torch.randn(D, generator=g), 1 + 0.1 * torch.randn(D, generator=g)
    pos = torch.arange(L).repeat(B)
    starts = torch.tensor([0, 4, 9])
    cos, sin = Kn.rope_tables(D, 1e6, 64, dev)
    rb = torch.arange(B).repeat_interleave(L)
    kc = torch.zeros(B, hkv, L, D, device=dev)
    vc = torch.zeros_like(kc)
    q = torch.zeros(B * L, hq * D, device=dev)
    i32 = lambda t: t.to(dev, torch.int32)  # noqa: E731
    use_norm = window == 0
    Kn.qkv_post(qkv.to(dev), B * L, hq, hkv, D, qn.to(dev) if use_norm else None, kn.to(dev) if use_norm else None,
                1e-6, cos, sin, i32(pos), i32(rb), i32(pos), q, kc, vc, L)
    row_start = starts.repeat_interleave(L)
    row_len = torch.maximum(pos + 1, row_start + 1)
    att = torch.zeros(B * L, hq * D, device=dev)
    Kn.attention(q, B * L, hq, hkv, D, kc, vc, L, i32(rb), i32(row_start), i32(row_len), att, L, window=window)
    # torch reference
    x = qkv.view(B, L, hq + 2 * hkv, D)
    qr, kr, vr = x[:, :, :hq], x[:, :, hq:hq + hkv], x[:, :, hq + hkv:]
    if use_norm:
        qr, kr = rmsnorm(qr, qn, 1e-6), rmsnorm(kr, kn, 1e-6)
    c, s = rope_cos_sin(torch.arange(L)[None].expand(B, L), D, 1e6)
    qr, kr = apply_rope(qr.transpose(1, 2), c, s), apply_rope(kr.transpose(1, 2), c, s)
    torch.testing.assert_close(kc.cpu(), kr, atol=1e-5, rtol=1e-5)
    kr, vr = kr.repeat_interleave(hq // hkv, 1), vr.transpose(1, 2).repeat_interleave(hq // hkv, 1)
    sc = qr @ kr.transpose(2, 3) * D ** -0.5
    kv = torch.arange(L)
    allowed = kv[None, :] <= torch.arange(L)[:, None]
    allowed = allowed[None] & (kv[None, None, :] >= starts[:, None, None])
    if window:
        allowed = allowed & (kv[None, None, :] > torch.arange(L)[None, :, None] - window)
    allowed = allowed | (kv[None, None, :] == torch.maximum(torch.arange(L)[None, :, None], starts[:, None, None]))
    sc = sc.masked_fill(~allowed[:, None], float("-inf"))
    ref = (sc.softmax(-1) @ vr).transpose(1, 2).reshape(B * L, hq * D)
    torch.testing.assert_close(att.cpu(), ref, atol=2e-5, rtol=2e-5)


@pytest.mark.parametrize("D,hq,hkv,L", [(128, 16, 8, 300), (128, 16, 8, 129), (128, 16, 8, 520), (128, 16, 8, 17), (16, 4, 2, 9),
                                        (128, 16, 8, 2100)])
@pytest.mark.parametrize("kvdt", [torch.float32, torch.bfloat16])
def test_decode_attention_matches_two_kernel_path(D, hq, hkv, L, kvdt):
    """Fused qt_decode_attention == qt_qkv_post + qt_attention on the same cache (decode rows)."""
    from qwen_tts import kernels as Kn
    dev = _dev()
    g = torch.Generator().manual_seed(L + D)
    B = 4
    qkv = torch.randn(B, (hq + 2 * hkv) * D, generator=g).to(dev)
    qn, kn = (1 + 0.1 * torch.randn(D, generator=g)).to(dev), (1 + 0.1 * torch.randn(D, generator=g)).to(dev)
    kc = torch.randn(B, hkv, L + 3, D, generator=g).to(dev, kvdt)
    vc = torch.randn(B, hkv, L + 3, D, generator=g).to(dev, kvdt)
    kc2, vc2 = kc.clone(), vc.clone()
    cos, sin = Kn.rope_tables(D, 1e6, L + 64, dev)
    i32 = lambda t: torch.as_tensor(t, dtype=torch.int32, device=dev)  # noqa: E731
    pos, kvpos = i32([L - 1 + 5, L - 1, L - 1 + 2, L - 1]), i32([L - 1] * B)
    rb, start = i32(range(B)), i32([0, 3, 0, L - 1])
    q = torch.zeros(B, hq * D, device=dev)
    a1 = torch.zeros(B, hq * D, device=dev)
    Kn.qkv_post(qkv, B, hq, hkv, D, qn, kn, 1e-6, cos, sin, pos, rb, kvpos, q, kc, vc, L + 3)
    Kn.attention(q, B, hq, hkv, D, kc, vc, L + 3, rb, start, kvpos + 1, a1, L)
    a2 = torch.zeros(B, hq * D, device=dev)
    Kn.decode_attention(qkv, B, hq, hkv, D, qn, kn, 1e-6, cos, sin, pos, rb, kvpos, start, kc2, vc2, L + 3, a2)
    ktol = 2e-6 if kvdt == torch.float32 else 1e-2  # fp contraction / one bf16 ulp
    torch.testing.assert_close(kc2.float(), kc.float(), atol=ktol, rtol=ktol)
    torch.testing.assert_close(vc2.float(), vc.float(), atol=0, rtol=0)
    tol = 2e-5 if kvdt == torch.float32 else 2e-3
    torch.testing.assert_close(a2, a1, atol=tol, rtol=tol)
    # bf16 output = RNE rounding of the fp32 output (what the o_proj MFMA would apply)
    a3 = torch.zeros(B, hq * D, device=dev, dtype=torch.bfloat16)
    kc3, vc3 = kc2.clone(), vc2.clone()
    Kn.decode_attention(qkv, B, hq, hkv, D, qn, kn, 1e-6, cos, sin, pos, rb, kvpos, start, kc3, vc3, L + 3, a3)
    torch.testing.assert_close(a3, a2.to(torch.bfloat16), atol=0, rtol=0)
    # static positions as a launch constant (code-predictor steps) == the same positions through device arrays
    same, zero = i32([L - 1] * B), i32([0] * B)
    kc4, vc4, kc5, vc5 = kc.clone(), vc.clone(), kc.clone(), vc.clone()
    a4 = torch.zeros(B, hq * D, device=dev)
    a5 = torch.zeros(B, hq * D, device=dev)
    Kn.decode_attention(qkv, B, hq, hkv, D, qn, kn, 1e-6, cos, sin, same, rb, same, zero, kc4, vc4, L + 3, a4)
    Kn.decode_attention(qkv, B, hq, hkv, D, qn, kn, 1e-6, cos, sin, same, rb, same, zero, kc5, vc5, L + 3, a5,
                        const_pos=L - 1)
    assert torch.equal(a4, a5) and torch.equal(kc4, kc5) and torch.equal(vc4, vc5)
    # split-KV (nsplit blocks per (row, kv head), deterministic merge) == single block, bitwise reproducible (2100 keys:
    # several ping-pong chunks per split)
    for ns in (2, 3, 8):
        ws = torch.zeros(Kn.decode_attn_ws_bytes(B, hq, hkv, D, ns), dtype=torch.uint8, device=dev)
        outs = []
        for _ in range(2):
            kc6, vc6 = kc.clone(), vc.clone()
            a6 = torch.zeros(B, hq * D, device=dev)
            Kn.decode_attention(qkv, B, hq, hkv, D, qn, kn, 1e-6, cos, sin, pos, rb, kvpos, start, kc6, vc6, L + 3, a6,
                                nsplit=ns, ws=ws)
            outs.append(a6)
            assert torch.equal(kc6, kc2) and torch.equal(vc6, vc2)
        assert torch.equal(outs[0], outs[1])
        torch.testing.assert_close(outs[0], a2, atol=tol, rtol=tol)


@pytest.mark.parametrize("D,hq,hkv,L,N,B", [(128, 16, 8, 17, 1024, 8), (128, 16, 8, 3, 1024, 16), (128, 8, 4, 40, 200, 3),
                                            (16, 8, 2, 9, 32, 5), (64, 4, 4, 64, 96, 1), (128, 16, 4, 20, 256, 4),
                                            (128, 16, 8, 16, 1024, 8), (128, 16, 8, 1, 1024, 3)])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_decode_attn_oproj_matches_two_kernel_path(D, hq, hkv, L, N, B, dt):
    """qt_decode_attn_oproj (attention fused into o_proj + residual, head partials summed in-block) == qt_decode_attention
    followed by the o_proj GEMV with residual add; same cache writes; bitwise reproducible; const_pos == arrays."""
    from qwen_tts import kernels as Kn, _hip
    if dt == torch.float32 and (hq // hkv) * D // 16 > 16:
        pytest.skip("fp32 o_proj K slice of one kv head > 16 k tiles: rejected by design (QT_ERR_SHAPE)")
    dev = _dev()
    g = torch.Generator().manual_seed(L * 7 + D + N)
    qkv = torch.randn(B, (hq + 2 * hkv) * D, generator=g).to(dev)
    qn, kn = (1 + 0.1 * torch.randn(D, generator=g)).to(dev), (1 + 0.1 * torch.randn(D, generator=g)).to(dev)
    Lmax = L + 2
    kc = torch.randn(B, hkv, Lmax, D, generator=g).to(dev, dt)
    vc = torch.randn(B, hkv, Lmax, D, generator=g).to(dev, dt)
    Wo = torch.randn(N, hq * D, generator=g) * 0.05
    wo = Kn.tile_linear(Wo.to(dev), dt)
    x0 = torch.randn(B, N, generator=g).to(dev)
    cos, sin = Kn.rope_tables(D, 1e6, Lmax + 8, dev)
    i32 = lambda t: torch.as_tensor(t, dtype=torch.int32, device=dev)  # noqa: E731
    pos = i32([L - 1] * B)
    rb, zero = i32(range(B)), i32([0] * B)
    # two-kernel reference
    kc1, vc1 = kc.clone(), vc.clone()
    att = torch.zeros(B, hq * D, device=dev, dtype=dt)
    Kn.decode_attention(qkv, B, hq, hkv, D, qn, kn, 1e-6, cos, sin, pos, rb, pos, zero, kc1, vc1, Lmax, att)
    x1 = x0.clone()
    Kn.gemm(att, wo, x1, B, hq * D, N, epi=_hip.EPI_ADD, splitk=1)
    outs = []
    for _ in range(2):
        kc2, vc2 = kc.clone(), vc.clone()
        x2 = x0.clone()
        Kn.decode_attn_oproj(qkv, B, hq, hkv, D, qn, kn, 1e-6, cos, sin, kc2, vc2, Lmax, wo, x2, const_pos=L - 1)
        ktol = 2e-6 if dt == torch.float32 else 1e-2  # fp contraction of the k RMSNorm + RoPE / one bf16 ulp
        torch.testing.assert_close(kc2.float(), kc1.float(), atol=ktol, rtol=ktol)
        assert torch.equal(vc2, vc1)
        outs.append(x2)
    assert torch.equal(outs[0], outs[1])
    tol = 1e-4 if dt == torch.float32 else 2e-2
    torch.testing.assert_close(outs[0], x1, atol=tol, rtol=tol)
    # the same positions through device arrays (rope_pos / kv_pos / row_start) give the same bits
    kc3, vc3 = kc.clone(), vc.clone()
    x3 = x0.clone()
    Kn.decode_attn_oproj(qkv, B, hq, hkv, D, qn, kn, 1e-6, cos, sin, kc3, vc3, Lmax, wo, x3,
                         rope_pos=pos, kv_pos=pos, row_start=zero)
    assert torch.equal(x3, outs[0]) and torch.equal(kc3, kc2)
    # ragged key ranges (row_start > 0) through the arrays path vs the two-kernel path
    start = i32([(b * 3) % max(L - 1, 1) for b in range(B)])
    kc4, vc4, kc5, vc5 = kc.clone(), vc.clone(), kc.clone(), vc.clone()
    att4 = torch.zeros(B, hq * D, device=dev, dtype=dt)
    Kn.decode_attention(qkv, B, hq, hkv, D, qn, kn, 1e-6, cos, sin, pos, rb, pos, start, kc4, vc4, Lmax, att4)
    x4 = x0.clone()
    Kn.gemm(att4, wo, x4, B, hq * D, N, epi=_hip.EPI_ADD, splitk=1)
    x5 = x0.clone()
    Kn.decode_attn_oproj(qkv, B, hq, hkv, D, qn, kn, 1e-6, cos, sin, kc5, vc5, Lmax, wo, x5,
                         rope_pos=pos, kv_pos=pos, row_start=start)
    torch.testing.assert_close(x5, x4, atol=tol, rtol=tol)
    # head-split form (a workspace given; bf16, D = 128, Hq = 2 Hkv, <= 8 rows, N % 256 == 0, <= 16 cached keys):
    # same results within the tolerance, bitwise reproducible over repeated launches on one workspace (the sequence
    # tags advance), same cache writes, the error flag clear; the x16 shadow = bf16(x)
    if dt == torch.bfloat16 and D == 128 and hq == 2 * hkv and B <= 8 and N % 256 == 0 and L - 1 <= 16:
        ws = torch.zeros(Kn.attn_oproj_ws_bytes(N, hkv), dtype=torch.uint8, device=dev)
        hs = []
        for _ in range(3):
            kc6, vc6 = kc.clone(), vc.clone()
            x6 = x0.clone()
            x16 = torch.zeros(B, N, dtype=torch.bfloat16, device=dev)
            Kn.decode_attn_oproj(qkv, B, hq, hkv, D, qn, kn, 1e-6, cos, sin, kc6, vc6, Lmax, wo, x6, const_pos=L - 1,
                                 x16=x16, ws=ws)
            assert torch.equal(kc6, kc2) and torch.equal(vc6, vc2)
            assert torch.equal(x16, x6.to(torch.bfloat16))
            hs.append(x6)
        assert torch.equal(hs[0], hs[1]) and torch.equal(hs[0], hs[2])
        torch.testing.assert_close(hs[0], x1, atol=tol, rtol=tol)
        assert int(ws[:4].view(torch.int32).item()) == 0


def test_attn_oproj_head_split_tags_across_row_counts():
    """The head-split fused attention + o_proj on ONE workspace across launches with changing row counts (8, 3, 1, 8)
    and key counts: every launch equals the (column group, row) form within bf16 tolerance and the hand-off sequence
    tags stay consistent (no stale granule is taken, no poll gives up)."""
    from qwen_tts import kernels as Kn
    dev = _dev()
    D, hq, hkv, N = 128, 16, 8, 1024
    g = torch.Generator().manual_seed(77)
    Lmax = 18
    qn, kn = (1 + 0.1 * torch.randn(D, generator=g)).to(dev), (1 + 0.1 * torch.randn(D, generator=g)).to(dev)
    wo = Kn.tile_linear((torch.randn(N, hq * D, generator=g) * 0.05).to(dev), torch.bfloat16)
    cos, sin = Kn.rope_tables(D, 1e6, Lmax + 8, dev)
    ws = torch.zeros(Kn.attn_oproj_ws_bytes(N, hkv), dtype=torch.uint8, device=dev)
    for B, pos in ((8, 3), (3, 16), (1, 0), (8, 9), (5, 12), (8, 16)):
        qkv = torch.randn(B, (hq + 2 * hkv) * D, generator=g).to(dev)
        kc = torch.randn(B, hkv, Lmax, D, generator=g).to(dev, torch.bfloat16)
        vc = torch.randn(B, hkv, Lmax, D, generator=g).to(dev, torch.bfloat16)
        x0 = torch.randn(B, N, generator=g).to(dev)
        xa, xb = x0.clone(), x0.clone()
        kca, vca, kcb, vcb = kc.clone(), vc.clone(), kc.clone(), vc.clone()
        Kn.decode_attn_oproj(qkv, B, hq, hkv, D, qn, kn, 1e-6, cos, sin, kca, vca, Lmax, wo, xa, const_pos=pos)
        Kn.decode_attn_oproj(qkv, B, hq, hkv, D, qn, kn, 1e-6, cos, sin, kcb, vcb, Lmax, wo, xb, const_pos=pos, ws=ws)
        torch.testing.assert_close(xb, xa, atol=2e-2, rtol=2e-2)
        assert torch.equal(kca, kcb) and torch.equal(vca, vcb)
    assert int(ws[:4].view(torch.int32).item()) == 0


def test_attn_oproj_head_split_needs_a_head_per_row():
    """The head-split form sums output row r in the block of kv head r: with more rows than kv heads a launch given a
    workspace takes the (column group, row) form (before this check, rows >= Hkv were never written)."""
    from qwen_tts import kernels as Kn
    dev = _dev()
    D, hq, hkv, N, B, Lmax, pos = 128, 8, 4, 1024, 8, 18, 5
    g = torch.Generator().manual_seed(5)
    qn, kn = (1 + 0.1 * torch.randn(D, generator=g)).to(dev), (1 + 0.1 * torch.randn(D, generator=g)).to(dev)
    wo = Kn.tile_linear((torch.randn(N, hq * D, generator=g) * 0.05).to(dev), torch.bfloat16)
    cos, sin = Kn.rope_tables(D, 1e6, Lmax + 8, dev)
    qkv = torch.randn(B, (hq + 2 * hkv) * D, generator=g).to(dev)
    kc = torch.randn(B, hkv, Lmax, D, generator=g).to(dev, torch.bfloat16)
    vc = torch.randn(B, hkv, Lmax, D, generator=g).to(dev, torch.bfloat16)
    x0 = torch.randn(B, N, generator=g).to(dev)
    ws = torch.zeros(Kn.attn_oproj_ws_bytes(N, hkv), dtype=torch.uint8, device=dev)
    xa, xb = x0.clone(), x0.clone()
    Kn.decode_attn_oproj(qkv, B, hq, hkv, D, qn, kn, 1e-6, cos, sin, kc.clone(), vc.clone(), Lmax, wo, xa, const_pos=pos)
    Kn.decode_attn_oproj(qkv, B, hq, hkv, D, qn, kn, 1e-6, cos, sin, kc.clone(), vc.clone(), Lmax, wo, xb, const_pos=pos,
                         ws=ws)
    assert torch.equal(xa, xb)  # both took the (column group, row) form
    assert int(ws[:4].view(torch.int32).item()) == 0


@pytest.mark.parametrize("D,hq,hkv", [(128, 16, 8), (16, 4, 2), (64, 4, 4)])
@pytest.mark.parametrize("kvdt", [torch.float32, torch.bfloat16])
def test_small_prefill_attention_matches_two_kernel_path(D, hq, hkv, kvdt):
    """Fused 2-token prefill (code-predictor per-frame prefill) == qt_qkv_post + qt_attention."""
    from qwen_tts import kernels as Kn
    dev = _dev()
    g = torch.Generator().manual_seed(D + hq)
    B, T, Lmax = 5, 2, 18
    R = B * T
    qkv = torch.randn(R, (hq + 2 * hkv) * D, generator=g).to(dev)
    qn, kn = (1 + 0.1 * torch.randn(D, generator=g)).to(dev), (1 + 0.1 * torch.randn(D, generator=g)).to(dev)
    cos, sin = Kn.rope_tables(D, 1e6, 64, dev)
    i32 = lambda t: torch.as_tensor(t, dtype=torch.int32, device=dev)  # noqa: E731
    pos = i32([t for _ in range(B) for t in range(T)])
    rb = i32([b for b in range(B) for _ in range(T)])
    kc1 = torch.zeros(B, hkv, Lmax, D, device=dev, dtype=kvdt)
    vc1 = torch.zeros_like(kc1)
    q = torch.zeros(R, hq * D, device=dev)
    a1 = torch.zeros(R, hq * D, device=dev)
    Kn.qkv_post(qkv, R, hq, hkv, D, qn, kn, 1e-6, cos, sin, pos, rb, pos, q, kc1, vc1, Lmax)
    Kn.attention(q, R, hq, hkv, D, kc1, vc1, Lmax, rb, i32([0] * R), pos + 1, a1, T)
    kc2, vc2 = torch.zeros_like(kc1), torch.zeros_like(vc1)
    a2 = torch.zeros(R, hq * D, device=dev)
    Kn.small_prefill_attention(qkv, R, T, hq, hkv, D, qn, kn, 1e-6, cos, sin, kc2, vc2, Lmax, a2)
    ktol = 2e-6 if kvdt == torch.float32 else 1e-2
    torch.testing.assert_close(kc2.float(), kc1.float(), atol=ktol, rtol=ktol)
    torch.testing.assert_close(vc2.float(), vc1.float(), atol=0, rtol=0)
    torch.testing.assert_close(a2, a1, atol=2e-5, rtol=2e-5)


def test_sample_greedy_processors():
    from qwen_tts import kernels as Kn
    from oracle.talker import process_logits
    dev = _dev()
    g = torch.Generator().manual_seed(5)
    B, V, eos = 4, 3072, 2150
    logits = torch.randn(B, V, generator=g)
    logits[0, 2150] = 50.0  # eos wins if not masked
    logits[1, 7] = logits[1, 9] = 40.0  # tie -> lowest index
    hist = torch.randint(0, 2048, (B, 5), generator=g)
    hist[2, 0] = int(torch.argmax(logits[2, :2048]))  # penalised winner
    seen = torch.zeros(B, V, dtype=torch.uint8)
    seen.scatter_(1, hist, 1)
    supp = [i for i in range(V - 1024, V) if i != eos]
    for ngen in (1, 5):
        ref = torch.argmax(process_logits(logits, hist, ngen, eos, supp, 1.05), -1)
        tok = torch.zeros(B, dtype=torch.int32, device=dev)
        sd = seen.to(dev)
        Kn.sample(logits.to(dev), B, V, V, tok, seen=sd, rep_penalty=1.05,
                  n_generated=torch.tensor([ngen], dtype=torch.int32, device=dev), min_new_tokens=2, eos_id=eos,
                  suppress=(V - 1024, V, eos))
        assert tok.cpu().long().tolist() == ref.tolist()


@pytest.mark.parametrize("V,scale,ties", [(2048, 0.7, False), (2048, 3.0, False), (3072, 1.0, True), (2048, 40.0, False),
                                          (2048, 0.02, False)])
def test_sample_histogram_topk_matches_per_wave_path(V, scale, ties):
    """The histogram top-k path (default) and the per-wave candidate path (algo=1) keep the same top-k set and draw
    the same Philox-keyed Gumbel-max token, for spreads inside the histogram (0.7, 3 units), beyond it (40: falls
    through) and flat rows (0.02: the boundary bin overflows, falls through).  With many ties (scores on a 0.25 grid)
    the per-wave path can overflow its candidate lists and draw by inverse CDF instead (another use of the Philox
    stream), so there both paths are only checked to draw from the kept set (every score >= the k-th largest)."""
    from qwen_tts import kernels as Kn
    dev = _dev()
    g = torch.Generator().manual_seed(11)
    R = 16
    logits = torch.randn(R, V, generator=g) * scale
    if ties:
        logits = (logits * 4).round() / 4  # many equal scores, also at the k-th
    lg = logits.to(dev)
    for k in (1, 20, 50, 64):
        for seed in range(6):
            toks = []
            for algo in (0, 1):
                tok = torch.zeros(R, dtype=torch.int32, device=dev)
                Kn.sample(lg, R, V, V, tok, do_sample=True, top_k=k, temperature=0.9, seed=seed, algo=algo)
                toks.append(tok.cpu())
            if not ties:
                assert torch.equal(toks[0], toks[1]), (k, seed)
            kth = logits.topk(k, -1).values[:, -1:]
            for t in toks:
                assert bool((logits.gather(1, t.long()[:, None]) >= kth).all()), (k, seed)


def test_sample_next_step_rows():
    """The sampler's next-step outputs: the chosen token's table row (fp32), its bf16 copy (the residual shadow)
    and the second table's row (the code predictor's precomputed layer-0 q/k/v), each at its own row stride."""
    from qwen_tts import kernels as Kn
    dev = _dev()
    g = torch.Generator().manual_seed(3)
    R, V, D, D2 = 8, 2048, 1024, 4096
    logits = torch.randn(R, V, generator=g).to(dev)
    tab = torch.randn(V, D, generator=g).to(dev)
    tab2 = torch.randn(V, D2, generator=g).to(dev)
    out = torch.zeros(R, D + 8, device=dev)
    out16 = torch.zeros(R, D + 16, dtype=torch.bfloat16, device=dev)
    out2 = torch.zeros(R, D2 + 4, device=dev)
    tok = torch.zeros(R, dtype=torch.int32, device=dev)
    Kn.sample(logits, R, V, V, tok, emb=(tab, out, D + 8), emb16=(out16, D + 16), emb2=(tab2, out2, D2 + 4))
    t = tok.long()
    assert torch.equal(t, logits.argmax(-1))
    torch.testing.assert_close(out[:, :D], tab[t], atol=0, rtol=0)
    torch.testing.assert_close(out16[:, :D], tab[t].to(torch.bfloat16), atol=0, rtol=0)
    torch.testing.assert_close(out2[:, :D2], tab2[t], atol=0, rtol=0)
    assert not out[:, D:].any() and not out16[:, D:].float().any() and not out2[:, D2:].any()


def test_sample_distribution_topk():
    """Sampling parity is distribution-level (RNG streams differ by device): frequencies vs probabilities."""
    from qwen_tts import kernels as Kn
    dev = _dev()
    V, R = 64, 2048
    logits = torch.linspace(-2, 2, V)[None].expand(R, V).contiguous()
    tok = torch.zeros(R, dtype=torch.int32, device=dev)
    Kn.sample(logits.to(dev), R, V, V, tok, do_sample=True, top_k=8, top_p=1.0, temperature=0.9, seed=11,
              step=torch.zeros(1, dtype=torch.int32, device=dev), substep=0)
    t = tok.cpu().long()
    assert t.min() >= V - 8
    p = torch.softmax(logits[0, V - 8:] / 0.9, -1)
    freq = torch.bincount(t - (V - 8), minlength=8).float() / R
    assert (freq - p).abs().max() < 0.05


@pytest.mark.parametrize("V,k,ties", [(3072, 50, False), (2048, 50, True), (3072, 300, False), (200, 7, True)])
def test_sample_topk_support_large_vocab(V, k, ties):
    """Exact k-th-largest threshold on realistic vocabularies (block search + LDS compaction + wave finish):
    every draw lies in {scores >= k-th largest} (ties kept, TopKLogitsWarper), and the top token is drawn
    at about its renormalised probability."""
    from qwen_tts import kernels as Kn
    dev = _dev()
    R = 512
    g = torch.Generator().manual_seed(V + k)
    logits = torch.randn(R, V, generator=g) * 2
    if ties:  # a block of equal scores straddling the threshold
        kth = torch.topk(logits, k, -1).values[:, -1:]
        idx = torch.randint(0, V, (R, 40), generator=g)
        logits.scatter_(1, idx, kth.expand(R, 40))
    thr = torch.topk(logits, k, -1).values[:, -1:]
    tok = torch.zeros(R, dtype=torch.int32, device=dev)
    Kn.sample(logits.to(dev), R, V, V, tok, do_sample=True, top_k=k, top_p=1.0, temperature=1.0, seed=5,
              step=torch.zeros(1, dtype=torch.int32, device=dev), substep=0)
    t = tok.cpu().long()
    picked = logits.gather(1, t[:, None])
    assert bool((picked >= thr).all())
    # same row repeated: frequency of the argmax token vs its kept-set softmax probability
    row = logits[:1].expand(4096, V).contiguous()
    tok2 = torch.zeros(4096, dtype=torch.int32, device=dev)
    Kn.sample(row.to(dev), 4096, V, V, tok2, do_sample=True, top_k=k, top_p=1.0, temperature=1.0, seed=9,
              step=torch.zeros(1, dtype=torch.int32, device=dev), substep=1)
    kept = torch.where(logits[0] >= thr[0], logits[0], torch.tensor(-float("inf")))
    pr = torch.softmax(kept, -1)
    top = int(torch.argmax(logits[0]))
    assert abs((tok2.cpu().long() == top).float().mean().item() - pr[top].item()) < 0.03


@pytest.mark.parametrize("V,k", [(2048, 50), (3072, 64), (1024, 1)])
def test_sample_fast_topk_distribution(V, k):
    """k <= 64 path (per-wave candidates + Gumbel-max in one wave): every kept token is drawn at its renormalised
    softmax probability (chi-square-like bound over the whole kept set, same row repeated)."""
    from qwen_tts import kernels as Kn
    dev = _dev()
    R = 8192
    g = torch.Generator().manual_seed(V * 7 + k)
    row = torch.randn(1, V, generator=g) * 1.5
    thr = torch.topk(row, k, -1).values[:, -1:]
    pr = torch.softmax(torch.where(row >= thr, row / 0.9, torch.tensor(-float("inf"))), -1)[0]
    tok = torch.zeros(R, dtype=torch.int32, device=dev)
    Kn.sample(row.expand(R, V).contiguous().to(dev), R, V, V, tok, do_sample=True, top_k=k, top_p=1.0,
              temperature=0.9, seed=21, step=torch.full((1,), 3, dtype=torch.int32, device=dev), substep=2)
    t = tok.cpu().long()
    assert bool((row[0, t] >= thr[0]).all())
    freq = torch.bincount(t, minlength=V).float() / R
    sd = (pr * (1 - pr) / R).sqrt()
    assert bool(((freq - pr).abs() <= 5 * sd + 1e-3).all())


@pytest.mark.parametrize("V,k,p,ngen", [(3072, 50, 1.0, 1), (3072, 50, 1.0, 5), (2048, 50, 1.0, 5), (3072, 50, 0.8, 5),
                                       (2048, 0, 0.9, 5)])
def test_sample_full_processor_chain_distribution(V, k, p, ngen):
    """Sampled mode through the whole HF-4.57 chain the bench and the wrapper defaults use (M:2044-2066): repetition
    penalty 1.05 on the generated history (`seen`), min_new_tokens = 2 (EOS masked while n_generated < 2), the
    suppress range [V - 1024, V) minus EOS (talker vocab), then temperature 0.9 -> top-k -> top-p -> softmax -> draw.
    Frequencies of one row repeated R times vs oracle.process_logits -> oracle.warp_probs (5-sigma bound per token);
    the penalised history sits at the top of the row (it moves the top-k boundary), a suppressed token and EOS carry
    the largest logits (never drawn / masked below min_new_tokens)."""
    from qwen_tts import kernels as Kn
    from oracle.talker import process_logits, warp_probs
    dev = _dev()
    R, eos = 16384, V - 1024 + 102
    g = torch.Generator().manual_seed(V + k + ngen)
    row = torch.randn(1, V, generator=g) * 1.5
    top = torch.topk(row, 8, -1).indices[0]
    hist = torch.cat([top[:5], torch.randint(0, V - 1024, (7,), generator=g)])[None]  # penalised history
    row[0, V - 1024 + 5] = 9.0   # suppressed: never drawn
    row[0, eos] = float(row.max()) + 0.5  # EOS: masked while n_generated < min_new_tokens
    supp = [i for i in range(V - 1024, V) if i != eos] if V == 3072 else []
    scores = process_logits(row, hist, ngen, eos, supp, 1.05)
    pr = warp_probs(scores, 0.9, k, p)[0]
    seen = torch.zeros(R, V, dtype=torch.uint8)
    seen[:, hist[0]] = 1
    tok = torch.zeros(R, dtype=torch.int32, device=dev)
    Kn.sample(row.expand(R, V).contiguous().to(dev), R, V, V, tok, seen=seen.to(dev), rep_penalty=1.05,
              n_generated=torch.tensor([ngen], dtype=torch.int32, device=dev), min_new_tokens=2, eos_id=eos,
              suppress=(V - 1024, V, eos) if supp else (0, 0, -1), do_sample=True, top_k=k, top_p=p, temperature=0.9,
              seed=31 + ngen, step=torch.full((1,), 4, dtype=torch.int32, device=dev), substep=1)
    t = tok.cpu().long()
    assert bool((pr[t] > 0).all()), "drew a token outside the processed + warped support"
    freq = torch.bincount(t, minlength=V).float() / R
    sd = (pr * (1 - pr) / R).sqrt()
    assert bool(((freq - pr).abs() <= 5 * sd + 1e-3).all()), float(((freq - pr).abs() - 5 * sd).max())
    if ngen < 2:
        assert not bool((t == eos).any())
    else:
        assert pr[eos] > 0.01 and abs(freq[eos] - pr[eos]) <= 5 * sd[eos] + 1e-3


def test_sample_fast_topk_fallbacks():
    """Shapes the fast path hands back to the block search or must mask: a wave with > 64 tied keys (all scores
    equal: uniform over the whole row, ties kept), and fewer finite scores than k (-inf never drawn)."""
    from qwen_tts import kernels as Kn
    dev = _dev()
    V, R = 2048, 8192
    tok = torch.zeros(R, dtype=torch.int32, device=dev)
    Kn.sample(torch.zeros(R, V, device=dev), R, V, V, tok, do_sample=True, top_k=50, top_p=1.0, temperature=1.0,
              seed=2, step=torch.zeros(1, dtype=torch.int32, device=dev), substep=0)
    t = tok.cpu().long()
    assert t.min() >= 0 and t.max() < V
    assert len(set(t.tolist())) > V // 2  # ties kept: the draw spreads over the row
    logits = torch.full((R, V), -float("inf"))
    fin = torch.tensor([5, 300, 301, 1000, 2047])
    logits[:, fin] = torch.tensor([0.0, 1.0, -1.0, 0.5, 2.0])
    Kn.sample(logits.to(dev), R, V, V, tok, do_sample=True, top_k=50, top_p=1.0, temperature=1.0,
              seed=3, step=torch.zeros(1, dtype=torch.int32, device=dev), substep=0)
    t = tok.cpu().long()
    assert set(t.tolist()) <= set(fin.tolist())
    pr = torch.softmax(torch.tensor([0.0, 1.0, -1.0, 0.5, 2.0]), -1)
    freq = torch.tensor([(t == int(f)).float().mean().item() for f in fin])
    assert (freq - pr).abs().max() < 0.02


def test_sample_top_p_support():
    """TopP keeps the smallest top set whose mass reaches top_p (TopPLogitsWarper semantics)."""
    from qwen_tts import kernels as Kn
    dev = _dev()
    V, R = 16, 1024
    logits = torch.log(torch.tensor([0.4, 0.3, 0.15, 0.1] + [0.05 / 12] * 12))[None].expand(R, V).contiguous()
    tok = torch.zeros(R, dtype=torch.int32, device=dev)
    Kn.sample(logits.to(dev), R, V, V, tok, do_sample=True, top_k=0, top_p=0.65, temperature=1.0, seed=3,
              step=torch.zeros(1, dtype=torch.int32, device=dev), substep=0)
    t = tok.cpu().long()
    assert set(t.tolist()) == {0, 1}  # 0.4 < 0.65 <= 0.4 + 0.3
    assert abs((t == 0).float().mean().item() - 0.4 / 0.7) < 0.06


@pytest.mark.parametrize("V", [2048, 3072, 4096])
def test_sample_top_p_large_vocab(V):
    """TopP on full-size vocabularies (every per-thread register width): draws stay inside the nucleus."""
    from qwen_tts import kernels as Kn
    dev = _dev()
    R = 256
    g = torch.Generator().manual_seed(V)
    logits = torch.randn(R, V, generator=g) * 3
    tok = torch.zeros(R, dtype=torch.int32, device=dev)
    Kn.sample(logits.to(dev), R, V, V, tok, do_sample=True, top_k=0, top_p=0.8, temperature=1.0, seed=4,
              step=torch.zeros(1, dtype=torch.int32, device=dev), substep=0)
    p = torch.softmax(logits, -1)
    sp, idx = p.sort(-1, descending=True)
    keep = (sp.cumsum(-1) - sp) < 0.8  # TopPLogitsWarper: smallest prefix reaching top_p
    t = tok.cpu().long()
    for r in range(R):
        assert int(t[r]) in set(idx[r][keep[r]].tolist())


@pytest.mark.parametrize("V,k,p", [(2048, 100, 1.0), (3072, 0, 0.9), (2048, 300, 0.95)])
def test_sample_draw_at_total_stays_in_kept_set(V, k, p):
    """Slow path (top_k > 64 or top_p < 1): a draw u that rounds to the total mass (forced via debug_u = 1.0) is
    claimed by the last thread holding mass -- the last kept token in category order -- never token 0 or a token
    outside the kept set, also when the block's last thread holds no mass."""
    from qwen_tts import kernels as Kn
    dev = _dev()
    R = 16
    g = torch.Generator().manual_seed(V + k)
    logits = torch.randn(R, V, generator=g) * 2
    logits[:, 0] = -30.0  # token 0 is never in the kept set
    logits[:, 255::256] = -40.0  # thread 255's tokens: outside the kept set (that thread holds no mass)
    tok = torch.zeros(R, dtype=torch.int32, device=dev)
    Kn.sample(logits.to(dev), R, V, V, tok, do_sample=True, top_k=k, top_p=p, temperature=1.0, seed=1,
              step=torch.zeros(1, dtype=torch.int32, device=dev), substep=0, debug_u=1.0)
    t = tok.cpu().long()
    for r in range(R):
        row = logits[r]
        kept = torch.ones(V, dtype=torch.bool)
        if 0 < k < V:
            kept &= row >= torch.topk(row, k).values[-1]
        if p < 1.0:
            pr = torch.softmax(torch.where(kept, row, torch.tensor(-float("inf"))), -1)
            sp, idx = pr.sort(descending=True)
            keep = (sp.cumsum(-1) - sp) < p
            kept &= torch.zeros(V, dtype=torch.bool).scatter(0, idx[keep], True)
        # category order of the inverse CDF: thread-major (token v lives on thread v % 256, slot v // 256)
        order = sorted(range(V), key=lambda v: (v % 256, v // 256))
        last = [v for v in order if kept[v]][-1]
        assert int(t[r]) != 0 and bool(kept[t[r]]), (r, int(t[r]))
        assert int(t[r]) == last, (r, int(t[r]), last)


# ------------------------------------------------------------------------------------------ end-to-end talker
@pytest.fixture(scope="module")
def tiny_models():
    from oracle import load_preset, synth_state_dict, talker_param_specs
    from qwen_tts.model import TTSModel
    _dev()
    out = {}
    for p in ("tiny-customvoice", "tiny-voicedesign"):
        cfg, _ = load_preset(p)
        W = {k: torch.from_numpy(v) for k, v in synth_state_dict(talker_param_specs(cfg)).items()}
        out[p] = (cfg, W, TTSModel(cfg, W, dtype="fp32"))
    return out


def _run_case(model, key, case, idx, cfg, use_graph=True):
    from cases import gen_kwargs, make_inputs
    ids, ins, vcp, ref_ids = make_inputs(case, idx, cfg["talker_config"]["hidden_size"])
    return model.generate(input_ids=ids, instruct_ids=ins, ref_ids=ref_ids, voice_clone_prompt=vcp,
                          languages=case["languages"], speakers=case["speakers"],
                          non_streaming_mode=case["non_streaming_mode"], use_graph=use_graph, seed=case.get("seed"),
                          **gen_kwargs(case))


@pytest.mark.parametrize("use_graph", [True, False])
def test_talker_greedy_codes_bit_exact(tiny_models, use_graph):
    from cases import talker_cases
    z = np.load(os.path.join(GOLD, "tiny_talker.npz"))
    cases = talker_cases()
    for idx, (key, case) in enumerate(cases.items()):
        if case.get("do_sample"):
            continue
        preset = "tiny-voicedesign" if key.startswith("vd_") else "tiny-customvoice"
        cfg, _, model = tiny_models[preset]
        codes, hid = _run_case(model, key, case, idx, cfg, use_graph)
        assert len(codes) == int(z[f"{key}/n"]), key
        for j, c in enumerate(codes):
            np.testing.assert_array_equal(c.numpy(), z[f"{key}/codes{j}"], err_msg=key)
            np.testing.assert_allclose(hid[j].numpy(), z[f"{key}/hidden{j}"], atol=2e-4, rtol=2e-4, err_msg=key)


def test_talker_split_kv_by_length_bit_exact(tiny_models, monkeypatch):
    """The talker decode attention's length-bucketed split-KV (talker.attn_nsplit: one frame graph per split factor,
    picked by the host's bound on the longest row's keys) with thresholds lowered so every frame of the golden
    cases runs split 2, 3, 4 or 8 and the graph switches mid-decode: codes equal the reference fixtures bit for
    bit (fp32), graph and eager."""
    from cases import talker_cases
    from qwen_tts import talker as T
    from qwen_tts.model import TTSModel
    monkeypatch.setattr(T, "ATTN_SPLIT", [(12, 2), (24, 3), (40, 4), (1 << 30, 8)])
    z = np.load(os.path.join(GOLD, "tiny_talker.npz"))
    cases = talker_cases()
    switched = 0
    for use_graph in (True, False):
        for idx, (key, case) in enumerate(cases.items()):
            if case.get("do_sample") or key.startswith("vd_"):
                continue
            cfg, W, _ = tiny_models["tiny-customvoice"]
            model = TTSModel(cfg, W, dtype="fp32")
            codes, _ = _run_case(model, key, case, idx, cfg, use_graph)
            for j, c in enumerate(codes):
                np.testing.assert_array_equal(c.numpy(), z[f"{key}/codes{j}"], err_msg=key)
            if use_graph:
                switched += max(len(s.graphs) for s in model.engine.all_sessions()) >= 2
    assert switched >= 3  # the split factor changed mid-decode (a second graph captured) in most cases


def test_checkpoint_directory_drop_in(tiny_models, tmp_path):
    """A checkpoint directory in the reference's on-disk layout (config.json, generation_config.json,
    model.safetensors keyed by the reference state_dict names, speech_tokenizer/{config.json,
    model.safetensors}) loads through Qwen3TTSModel.from_pretrained and reproduces the golden codes; a
    directory without weights is an error (no silent synthetic fallback outside the packaged presets)."""
    import shutil
    from safetensors.torch import save_file
    from cases import talker_cases
    from oracle import codec_param_specs, load_preset, synth_state_dict
    from qwen_tts import Qwen3TTSModel
    from qwen_tts.weights import resolve_path
    cfg, W, _ = tiny_models["tiny-customvoice"]
    src = resolve_path("synthetic:tiny-customvoice")
    for f in ("config.json", "generation_config.json"):
        shutil.copy(os.path.join(src, f), tmp_path / f)
    save_file({k: v.contiguous() for k, v in W.items()}, str(tmp_path / "model.safetensors"))
    (tmp_path / "speech_tokenizer").mkdir()
    shutil.copy(os.path.join(src, "speech_tokenizer", "config.json"), tmp_path / "speech_tokenizer" / "config.json")
    _, ccfg = load_preset("tiny-customvoice")
    CW = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synth_state_dict(codec_param_specs(ccfg)).items()}
    save_file(CW, str(tmp_path / "speech_tokenizer" / "model.safetensors"))
    from cases import write_test_tokenizer
    write_test_tokenizer(tmp_path)  # a real checkpoint dir carries its BPE files (no hash stand-in outside presets)
    tts = Qwen3TTSModel.from_pretrained(str(tmp_path), dtype=torch.float32)
    z = np.load(os.path.join(GOLD, "tiny_talker.npz"))
    cases = talker_cases()
    key = "cv_b2_stream_dialect"
    codes, _ = _run_case(tts.model, key, cases[key], list(cases).index(key), cfg)
    for j, c in enumerate(codes):
        np.testing.assert_array_equal(c.numpy(), z[f"{key}/codes{j}"])
    wavs, sr = tts.model.speech_tokenizer.decode([{"audio_codes": c} for c in codes])
    assert sr == 24000 and all(w.shape[0] > 0 for w in wavs)
    (tmp_path / "model.safetensors").unlink()
    with pytest.raises(FileNotFoundError):
        Qwen3TTSModel.from_pretrained(str(tmp_path), dtype=torch.float32)


def test_talker_eos_ragged_bit_exact(tiny_models):
    from cases import talker_cases
    from qwen_tts.model import TTSModel
    z = np.load(os.path.join(GOLD, "tiny_talker.npz"))
    cfg, W, _ = tiny_models["tiny-customvoice"]
    W = dict(W)
    head = W["talker.codec_head.weight"].clone()
    head[cfg["talker_config"]["codec_eos_token_id"]] = head[int(z["eos_b2/donor"])]
    W["talker.codec_head.weight"] = head
    model = TTSModel(cfg, W, dtype="fp32")
    cases = talker_cases()
    key = "cv_b2_stream_dialect"
    codes, _ = _run_case(model, key, dict(cases[key], max_new_tokens=24), list(cases).index(key), cfg)
    for j, c in enumerate(codes):
        np.testing.assert_array_equal(c.numpy(), z[f"eos_b2/codes{j}"])


@pytest.mark.parametrize("ctx,eos,frames", [(None, False, 30), (None, True, 24), (None, False, 331), (1000, False, 30),
                                            (1000, True, 24), (2, True, 24), (1000, False, 331)])
def test_stream_matches_one_shot(tiny_models, ctx, eos, frames):
    """stream(): per utterance the PCM chunks concatenate to exactly the one-shot generate+decode length
    (EOS-ragged batch and > 300-frame chunk restarts included); with the stateful incremental decoder (ctx None,
    the default) or a left context covering each reference chunk they equal the one-shot PCM; the first chunk
    (no left context needed) always does."""
    from cases import gen_kwargs, make_inputs, talker_cases
    from oracle import codec_param_specs, load_preset, synth_state_dict
    from qwen_tts import Qwen3TTSTokenizer
    from qwen_tts.model import TTSModel
    _dev()
    cfg, W, _ = tiny_models["tiny-customvoice"]
    W = dict(W)
    if eos:
        z = np.load(os.path.join(GOLD, "tiny_talker.npz"))
        head = W["talker.codec_head.weight"].clone()
        head[cfg["talker_config"]["codec_eos_token_id"]] = head[int(z["eos_b2/donor"])]
        W["talker.codec_head.weight"] = head
    model = TTSModel(cfg, W, dtype="fp32")
    _, ccfg = load_preset("tiny-customvoice")
    CW = {k: torch.from_numpy(v) for k, v in synth_state_dict(codec_param_specs(ccfg)).items()}
    tok = Qwen3TTSTokenizer.from_pretrained("synthetic:tiny-customvoice/speech_tokenizer", dtype="fp32", weights=CW)
    model.load_speech_tokenizer(tok)
    key = "cv_b2_stream_dialect"
    case = dict(talker_cases()[key], max_new_tokens=frames)
    ids, ins, vcp, ref_ids = make_inputs(case, list(talker_cases()).index(key), cfg["talker_config"]["hidden_size"])
    kw = dict(input_ids=ids, instruct_ids=ins, ref_ids=ref_ids, voice_clone_prompt=vcp, languages=case["languages"],
              speakers=case["speakers"], non_streaming_mode=case["non_streaming_mode"], **gen_kwargs(case))
    codes, _ = model.generate(**kw)
    wavs, _ = tok.decode([{"audio_codes": c} for c in codes])
    if eos:
        assert len({c.shape[0] for c in codes}) > 1  # ragged: rows stop at different frames
    chunks = {}
    for b, pcm, last in model.stream(first_chunk_frames=3, chunk_frames=5, left_context=ctx, **kw):
        chunks.setdefault(b, []).append(pcm.cpu().numpy())
    assert sorted(chunks) == list(range(len(codes)))
    for b, w in enumerate(wavs):
        got = np.concatenate(chunks[b])
        assert got.shape == w.shape, (b, got.shape, w.shape)
        first = chunks[b][0]
        np.testing.assert_allclose(first, w[:first.shape[0]], atol=2e-4, rtol=0)
        if ctx is None or ctx >= 1000:
            np.testing.assert_allclose(got, w, atol=2e-4, rtol=0)


def test_stream_chunk_schedule_grows(tiny_models):
    """stream() chunks double from first_chunk_frames up to chunk_frames (1, 2, 4, 8, 8, ... frames of 1920
    samples; the first one is short by the 555 samples that wait for the next frame), so the audio of each chunk
    outlasts the generation of the next."""
    from cases import gen_kwargs, make_inputs, talker_cases
    from oracle import codec_param_specs, load_preset, synth_state_dict
    from qwen_tts import Qwen3TTSTokenizer
    from qwen_tts.model import TTSModel
    _dev()
    cfg, W, _ = tiny_models["tiny-customvoice"]
    model = TTSModel(cfg, W, dtype="fp32")
    _, ccfg = load_preset("tiny-customvoice")
    CW = {k: torch.from_numpy(v) for k, v in synth_state_dict(codec_param_specs(ccfg)).items()}
    model.load_speech_tokenizer(Qwen3TTSTokenizer.from_pretrained("synthetic:tiny-customvoice/speech_tokenizer",
                                                                  dtype="fp32", weights=CW))
    key = "cv_b2_stream_dialect"
    case = dict(talker_cases()[key], max_new_tokens=41)
    ids, ins, vcp, ref_ids = make_inputs(case, list(talker_cases()).index(key), cfg["talker_config"]["hidden_size"])
    kw = dict(input_ids=ids, instruct_ids=ins, ref_ids=ref_ids, voice_clone_prompt=vcp, languages=case["languages"],
              speakers=case["speakers"], non_streaming_mode=case["non_streaming_mode"], **gen_kwargs(case))
    kw["ignore_eos"] = True
    sizes = [pcm.numel() for b, pcm, last in model.stream(first_chunk_frames=1, chunk_frames=8, **kw) if b == 0]
    assert sizes[:5] == [1920 * 1 - 555, 1920 * 2, 1920 * 4, 1920 * 8, 1920 * 8], sizes
    # a hand-off give-up during frame 0 (a session flag word set on the stream right behind the first frame) fails the
    # request before the early one-frame first chunk's PCM is handed out (that chunk skips the EOS scan)
    import qwen_tts.talker as T
    flag = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    orig = T.TalkerEngine._run_frame
    ran = []

    def run_frame(self, s, keys, use_graph=True, part="all"):
        orig(self, s, keys, use_graph, part)
        if not ran:
            flag.fill_(1)
        ran.append(part)
    import pytest as _pt
    mp = _pt.MonkeyPatch()
    try:
        mp.setattr(T, "_flag_words", lambda s: [flag])
        mp.setattr(T.TalkerEngine, "_run_frame", run_frame)
        got = []
        with _pt.raises(RuntimeError, match="hand-off timed out"):
            for item in model.stream(first_chunk_frames=1, chunk_frames=8, **kw):
                got.append(item)
        assert ran[0] == "cp" and not got, (ran, len(got))
        assert int(flag.item()) == 0  # cleared for the session's next request
    finally:
        mp.undo()


def test_prefill_graph_replay_matches_eager(tiny_models):
    """A repeated prompt length gets a captured talker prefill (second call captures, third replays): greedy codes
    and hidden states of all three calls are identical, in fp32 and bf16."""
    from cases import talker_cases
    from qwen_tts.model import TTSModel
    cfg, W, _ = tiny_models["tiny-customvoice"]
    for dt in ("fp32", "bf16"):
        model = TTSModel(cfg, W, dtype=dt)
        case = dict(talker_cases()["cv_b3_auto_nospk"], max_new_tokens=12)
        outs = [_run_case(model, "cv_b3_auto_nospk", case, 2, cfg) for _ in range(3)]
        sess = model.engine.all_sessions()
        assert any(pre["graph"] is not None for s in sess for pre in s.prefill.values())
        for codes, hid in outs[1:]:
            assert all(torch.equal(a, b) for a, b in zip(codes, outs[0][0]))
            assert all(torch.equal(a, b) for a, b in zip(hid, outs[0][1]))


def test_sampling_fresh_seed_per_call_reuses_session(tiny_models):
    """Sampling draws a fresh Philox key per generate() call (like the reference's torch.multinomial): two calls
    give different codes, torch.manual_seed reproduces a call, an explicit seed reproduces itself -- and every
    call replays the same Session and captured graph (the seed is a device word, not part of the session key)."""
    from cases import talker_cases
    from qwen_tts.model import TTSModel
    cfg, W, _ = tiny_models["tiny-customvoice"]
    model = TTSModel(cfg, W, dtype="fp32")
    case = dict(talker_cases()["cv_b3_auto_nospk"], do_sample=True, subtalker_dosample=True, max_new_tokens=20)
    a, _ = _run_case(model, "cv_b3_auto_nospk", case, 2, cfg)
    sess = model.engine.all_sessions()
    assert len(sess) == 1 and not sess[0].busy
    graph = sess[0].graph
    b, _ = _run_case(model, "cv_b3_auto_nospk", case, 2, cfg)
    assert any(not torch.equal(x, y) for x, y in zip(a, b)), "two unseeded calls drew the same codes"
    torch.manual_seed(123)
    c, _ = _run_case(model, "cv_b3_auto_nospk", case, 2, cfg)
    torch.manual_seed(123)
    d, _ = _run_case(model, "cv_b3_auto_nospk", case, 2, cfg)
    assert all(torch.equal(x, y) for x, y in zip(c, d))
    e, _ = _run_case(model, "cv_b3_auto_nospk", dict(case, seed=77), 2, cfg)
    f, _ = _run_case(model, "cv_b3_auto_nospk", dict(case, seed=77), 2, cfg)
    assert all(torch.equal(x, y) for x, y in zip(e, f))
    assert model.engine.all_sessions() == sess and sess[0].graph is graph  # no re-allocation, no re-capture


def test_interleaved_streams_do_not_share_state(tiny_models):
    """Two stream() generators of the same shape, advanced alternately (a server interleaving requests): each
    gets a session of its own, and each one's PCM equals its one-shot generate() + decode()."""
    from cases import gen_kwargs, make_inputs, talker_cases
    from oracle import codec_param_specs, load_preset, synth_state_dict
    from qwen_tts import Qwen3TTSTokenizer
    from qwen_tts.model import TTSModel
    cfg, W, _ = tiny_models["tiny-customvoice"]
    model = TTSModel(cfg, W, dtype="fp32")
    _, ccfg = load_preset("tiny-customvoice")
    CW = {k: torch.from_numpy(v) for k, v in synth_state_dict(codec_param_specs(ccfg)).items()}
    tok = Qwen3TTSTokenizer.from_pretrained("synthetic:tiny-customvoice/speech_tokenizer", dtype="fp32", weights=CW)
    model.load_speech_tokenizer(tok)
    key = "cv_b2_stream_dialect"
    case = dict(talker_cases()[key], max_new_tokens=30)
    kws, refs = [], []
    for idx, spk in ((3, ["eric", "ryan"]), (11, ["ryan", "eric"])):  # different requests of one batch shape
        ids, ins, vcp, ref_ids = make_inputs(case, idx, cfg["talker_config"]["hidden_size"])
        kw = dict(input_ids=ids, instruct_ids=ins, ref_ids=ref_ids, voice_clone_prompt=vcp,
                  languages=case["languages"], speakers=spk,
                  non_streaming_mode=case["non_streaming_mode"], **gen_kwargs(case))
        codes, _ = model.generate(**kw)
        refs.append(tok.decode([{"audio_codes": c} for c in codes])[0])
        kws.append(kw)
    assert not np.array_equal(refs[0][0], refs[1][0])
    gens = [model.stream(first_chunk_frames=3, chunk_frames=4, **kw) for kw in kws]
    chunks = [{}, {}]
    live = [True, True]
    while any(live):
        for i, gnr in enumerate(gens):
            if live[i]:
                try:
                    b, pcm, last = next(gnr)
                    chunks[i].setdefault(b, []).append(pcm.cpu().numpy())
                except StopIteration:
                    live[i] = False
    assert len(model.engine.all_sessions()) >= 2 and not any(s.busy for s in model.engine.all_sessions())
    for i in range(2):
        for b, w in enumerate(refs[i]):
            np.testing.assert_allclose(np.concatenate(chunks[i][b]), w, atol=2e-4, rtol=0, err_msg=f"stream {i} row {b}")


def test_talker_bf16_runs_and_tracks_fp32(tiny_models):
    from cases import talker_cases
    from qwen_tts.model import TTSModel
    cfg, W, m32 = tiny_models["tiny-customvoice"]
    m16 = TTSModel(cfg, W, dtype="bf16")
    case = talker_cases()["cv_b1_nonstream"]
    c32, _ = _run_case(m32, "cv_b1_nonstream", case, 0, cfg)
    c16, _ = _run_case(m16, "cv_b1_nonstream", case, 0, cfg)
    assert c16[0].shape == c32[0].shape
    assert (c16[0][:2, 0] == c32[0][:2, 0]).all()  # the first tokens agree; later frames may drift in bf16


def test_bf16_decode_shortcuts_track_the_plain_path(tiny_models, monkeypatch):
    """bf16 decode shortcuts -- the bf16 residual shadow read by the RMS-normalised GEMVs (talker.X16) and the code
    predictor's layer-0 q/k/v gathered from precomputed tables (talker.QKV0_TAB) -- change only roundings (RMS sums
    from the bf16-rounded activations the MFMA reads anyway; another GEMM's summation order for the tables): greedy
    codes and per-frame hidden states stay with the plain bf16 path."""
    from cases import talker_cases
    from qwen_tts import talker as T
    from qwen_tts.model import TTSModel
    cfg, W, _ = tiny_models["tiny-customvoice"]
    case = talker_cases()["cv_b2_stream_dialect"]
    idx = list(talker_cases()).index("cv_b2_stream_dialect")
    runs = {}
    for x16, tab in ((False, False), (True, False), (True, True)):
        monkeypatch.setattr(T, "X16", x16)
        monkeypatch.setattr(T, "QKV0_TAB", tab)
        m = TTSModel(cfg, W, dtype="bf16")
        assert (m.engine.cp_qkv_tabs is not None) == tab
        runs[(x16, tab)] = _run_case(m, "cv_b2_stream_dialect", case, idx, cfg)
    c0, h0 = runs[(False, False)]
    for key in ((True, False), (True, True)):
        c, h = runs[key]
        for a, b, ha, hb in zip(c, c0, h, h0):
            n = min(a.shape[0], b.shape[0])
            assert n >= 4
            assert torch.equal(a[:4], b[:4]), key  # greedy codes of the first frames agree exactly
            # (later frames may follow a flipped near-tie of the tiny model's flat logits into another continuation)
            assert (a[:n] == b[:n]).float().mean() >= 0.5, key
            rel = (ha[:4] - hb[:4]).norm() / hb[:4].norm()
            assert rel < 3e-2, (key, float(rel))


# ------------------------------------------------------------------------------------------ codec
@pytest.mark.parametrize("preset,dtype", [("tiny-customvoice", "fp32"), ("1.7b-customvoice", "fp32"),
                                          ("1.7b-customvoice", "bf16")])
def test_codec_stream_matches_forward(preset, dtype):
    """codec.CodecStream (stateful incremental decode) fed in ragged pieces (1 frame, a few, many;
    past the 72-frame attention window) gives forward()'s PCM for every prefix it has produced: 1920 n - 555 samples
    after n frames.  Parity vs forward() (itself pinned to the reference by test_codec_decode_matches_reference)."""
    from oracle import codec_param_specs, load_preset, synth_state_dict
    from qwen_tts.codec import CodecDecoder
    dev = _dev()
    _, ccfg = load_preset(preset)
    W = {k: torch.from_numpy(v) for k, v in synth_state_dict(codec_param_specs(ccfg)).items()}
    dec = CodecDecoder(ccfg, W, dtype=dtype, device=str(dev))
    g = torch.Generator().manual_seed(5)
    B, T = 2, 90
    codes = torch.randint(1, dec.tables.shape[1], (B, T, dec.tables.shape[0]), generator=g).to(dev, torch.int32)
    codes[1, 70:] = 0  # a row that ended early: zero padding, as in a ragged batch decode
    ref = dec.forward(codes)
    # three streams in a row on the decoder's pooled state slot: the first feeds eagerly, the second captures each
    # feed shape into a graph, the third replays them -- all three equal forward()
    pcms = []
    for rep in range(3):
        cs = dec.stream(B, T)
        fed = 0
        for n in (1, 3, 1, 8, 40, 37):
            ns = cs.feed(codes[:, fed:fed + n])
            fed += n
            assert ns == 1920 * fed - 555
            got, exp = cs.pcm[:, :ns], ref[:, :ns]
            if dtype == "fp32":
                torch.testing.assert_close(got, exp, atol=2e-5, rtol=0)
            else:
                rel = float((got - exp).norm() / exp.norm())
                assert rel < 2e-2, (fed, rel)
        assert fed == T
        with pytest.raises(ValueError):
            cs.feed(codes[:, :1])
        pcms.append(cs.pcm[:, :ns].clone())
        if rep == 2:
            assert len(cs.slot.graphs) == 6
        cs.close()
    assert torch.equal(pcms[1], pcms[2])  # captured replay == the eager feed it was captured from


def test_codec_forward_rope_growth_keeps_captured_tables():
    """A forward() of more than 512 frames grows the decoder's RoPE tables; the outgoing tables stay alive in
    dec._old_rope, because the feed graphs captured before hold their pointers: a stream on the same pooled slot
    replays them afterwards to the same bits, still within the fp32 bound of forward()."""
    from oracle import codec_param_specs, load_preset, synth_state_dict
    from qwen_tts.codec import CodecDecoder
    dev = _dev()
    _, ccfg = load_preset("tiny-customvoice")
    W = {k: torch.from_numpy(v) for k, v in synth_state_dict(codec_param_specs(ccfg)).items()}
    dec = CodecDecoder(ccfg, W, dtype="fp32", device=str(dev))
    g = torch.Generator().manual_seed(17)
    codes = torch.randint(1, dec.tables.shape[1], (1, 520, dec.tables.shape[0]), generator=g).to(dev, torch.int32)

    def run():
        cs = dec.stream(1, 8)
        slot = cs.slot
        for f in (0, 2, 4):
            ns = cs.feed(codes[:, f:f + 2])
        pcm = cs.pcm[:, :ns].clone()
        cs.close()
        return slot, pcm

    # the first stream feeds eagerly and captures the continuing feed, the second captures the first feed, the third
    # replays all three
    for _ in range(3):
        slot, before = run()
    assert sorted(slot.graphs) == [(2, False), (2, True)]
    old = (dec.cos, dec.sin)
    assert old[0].shape[0] == 512 and not dec._old_rope
    dec.forward(codes)
    assert dec.cos.shape[0] >= 520 and dec.cos is not old[0]
    assert any(c is old[0] and s is old[1] for c, s in dec._old_rope)
    slot2, after = run()
    assert slot2 is slot and sorted(slot.graphs) == [(2, False), (2, True)]
    assert torch.equal(after, before)
    assert after.shape[1] == 1920 * 6 - 555
    torch.testing.assert_close(after, dec.forward(codes[:, :6])[:, :after.shape[1]], atol=2e-5, rtol=0)


@pytest.mark.parametrize("fname,preset", [("codec_tiny.npz", "tiny-customvoice"), ("codec_full.npz", "1.7b-customvoice"),
                                           ("codec_full_chunks.npz", "1.7b-customvoice")])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_codec_decode_matches_reference(fname, preset, dtype):
    """Qwen3TTSTokenizer.decode vs the reference's decode (Z:259-365, K:992-1022) on the same codes: single, ragged
    batches, and at full dims T = 300 (one chunk), 325 and 700 (300/25 chunk restarts, K:885-895) plus a ragged pair
    whose long row restarts while the short one is zero padding."""
    from oracle import codec_param_specs, load_preset, synth_state_dict
    from qwen_tts import Qwen3TTSTokenizer
    _dev()
    z = np.load(os.path.join(GOLD, fname))
    _, ccfg = load_preset(preset)
    W = {k: torch.from_numpy(v) for k, v in synth_state_dict(codec_param_specs(ccfg)).items()}
    tok = Qwen3TTSTokenizer.from_pretrained(f"synthetic:{preset}/speech_tokenizer", dtype=dtype, weights=W)
    for key in sorted({k.split("/")[0] for k in z.files}):
        n = len([k for k in z.files if k.startswith(key + "/codes")])
        codes = [z[f"{key}/codes{j}"].astype(np.int64) for j in range(n)]
        wavs, sr = tok.decode([{"audio_codes": c} for c in codes])
        assert sr == 24000
        for j, w in enumerate(wavs):
            assert w.shape[0] == int(z[f"{key}/len{j}"]), key
            ref = z[f"{key}/wav{j}"] if f"{key}/wav{j}" in z.files else None
            got = w if ref is not None else w[::int(z[f"{key}/stride"]) if f"{key}/stride" in z.files else 7]
            ref = ref if ref is not None else z[f"{key}/wav{j}_stride"]
            if dtype == "fp32":
                np.testing.assert_allclose(got, ref, atol=2e-4, rtol=0, err_msg=key)
            else:
                rel = np.linalg.norm(got - ref) / np.linalg.norm(ref)
                assert rel < 5e-2, (key, rel)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_codec_stream_chunk_restarts_full_dims(dtype):
    """The streaming codec's chunk handling at full dims (what stream() does per reference chunk: a fresh stateful
    decoder per 300-frame chunk, primed with the chunk's 25 context frames, fed in pieces, its 555-sample tail
    dropped at the chunk end) reproduces the reference's chunked decode of 325 and 700 frames (codec_full_chunks.npz,
    from the reference's own decode): fp32 within 2e-4, bf16 rel-L2 < 5e-2."""
    from oracle import codec_param_specs, load_preset, synth_state_dict
    from qwen_tts.codec import CodecDecoder
    dev = _dev()
    z = np.load(os.path.join(GOLD, "codec_full_chunks.npz"))
    _, ccfg = load_preset("1.7b-customvoice")
    W = {k: torch.from_numpy(v) for k, v in synth_state_dict(codec_param_specs(ccfg), threads=16).items()}
    dec = CodecDecoder(ccfg, W, dtype=dtype, device=str(dev))
    up = dec.total_upsample
    for key in ("t325", "t700"):
        codes = torch.from_numpy(z[f"{key}/codes0"].astype(np.int32))[None].to(dev)
        T = codes.shape[1]
        outs, k = [], 0
        while k * 300 < T:
            base = k * 300 - (25 if k * 300 - 25 > 0 else 0)
            end = min((k + 1) * 300, T)
            cs = dec.stream(1, 325)
            fed = base
            for n in (1, 7, 40, 300):  # ragged feeds
                n = min(n, end - fed)
                if n > 0:
                    cs.feed(codes[:, fed:fed + n])
                    fed += n
            assert fed == end and cs.ns == up * (end - base) - 555
            outs.append(cs.pcm[0, (k * 300 - base) * up:cs.ns].clone())
            cs.close()
            k += 1
        w = torch.cat(outs)[:int(z[f"{key}/len0"])].cpu().numpy()
        assert w.shape[0] == int(z[f"{key}/len0"])
        stride = int(z[f"{key}/stride"])
        got, ref = w[::stride], z[f"{key}/wav0_stride"]
        if dtype == "fp32":
            np.testing.assert_allclose(got, ref, atol=2e-4, rtol=0, err_msg=key)
            np.testing.assert_allclose((w.astype(np.float64) ** 2).sum(), z[f"{key}/wav0_sum"][1], rtol=1e-3)
        else:
            assert np.linalg.norm(got - ref) / np.linalg.norm(ref) < 5e-2, key


def _serve_case():
    return dict(texts=[7, 3, 10, 5, 12, 4], languages=["auto", "english", "japanese", "chinese", "english", "auto"],
                speakers=["vivian", None, "dylan", "eric", "ryan", ""], non_streaming_mode=False, max_new_tokens=40)


@pytest.mark.parametrize("dtype,sample", [("fp32", False), ("fp32", True), ("bf16", True)])
def test_continuous_batching_matches_one_shot(tiny_models, dtype, sample):
    """generate(max_batch=k) decodes 6 requests through k batch rows, refilling a row as soon as its request ends
    (TalkerEngine.serve); every request's codes and hidden states equal the one-shot batched call's
    (EOS-ragged lengths, per-request Philox streams when sampling)."""
    from cases import make_inputs
    from qwen_tts.model import TTSModel
    z = np.load(os.path.join(GOLD, "tiny_talker.npz"))
    cfg, W, _ = tiny_models["tiny-customvoice"]
    W = dict(W)
    head = W["talker.codec_head.weight"].clone()
    head[cfg["talker_config"]["codec_eos_token_id"]] = head[int(z["eos_b2/donor"])]
    W["talker.codec_head.weight"] = head
    model = TTSModel(cfg, W, dtype=dtype)
    case = _serve_case()
    ids, _, _, _ = make_inputs(case, 11, cfg["talker_config"]["hidden_size"])
    kw = dict(input_ids=ids, languages=case["languages"], speakers=case["speakers"], non_streaming_mode=False,
              max_new_tokens=case["max_new_tokens"], do_sample=sample, subtalker_dosample=sample, seed=7)
    ref, ref_h = model.generate(**kw)
    assert len({c.shape[0] for c in ref}) > 1  # EOS-ragged
    for mb in (1, 2, 4):
        codes, hid = model.generate(**kw, max_batch=mb)
        assert len(codes) == len(ref)
        for i, (a, b) in enumerate(zip(codes, ref)):
            np.testing.assert_array_equal(a.numpy(), b.numpy(), err_msg=f"max_batch={mb} request {i}")
            np.testing.assert_allclose(hid[i].numpy(), ref_h[i].numpy(), atol=1e-5, rtol=1e-5)


def test_advance_rows_caps_each_row():
    from qwen_tts import kernels as K
    dev = _dev()
    B = 5
    c = torch.arange(5 * B, dtype=torch.int32, device=dev)  # field 0 = [0, 1, 2, 3, 4]
    ref = c.clone().view(5, B)
    K.advance_rows(c, B, 5, 3)
    ref[:, :3] += 1  # rows with frame index < 3 advance every field; rows 3, 4 stay
    torch.testing.assert_close(c.view(5, B), ref)


@pytest.mark.parametrize("frames,both", [(30, False), (331, False), (30, True)])
def test_stream_voice_clone_matches_wrapper(tiny_models, frames, both):
    """stream() with a voice-clone prompt (row 0 ICL with 7 reference code frames, row 1 x-vector only): per row the
    chunks concatenate to generate_voice_clone's decode of cat(ref_code, codes) (W:263-274) from the
    reference/generated boundary on, including a > 300-frame sequence whose reference chunk restart falls inside the
    generated part."""
    from cases import gen_kwargs, make_inputs, talker_cases
    from oracle import codec_param_specs, load_preset, synth_state_dict
    from qwen_tts import Qwen3TTSTokenizer
    _dev()
    cfg, W, model = tiny_models["tiny-customvoice"]
    _, ccfg = load_preset("tiny-customvoice")
    CW = {k: torch.from_numpy(v) for k, v in synth_state_dict(codec_param_specs(ccfg)).items()}
    tok = Qwen3TTSTokenizer.from_pretrained("synthetic:tiny-customvoice/speech_tokenizer", dtype="fp32", weights=CW)
    model.load_speech_tokenizer(tok)
    key = "icl_b2"
    case = dict(talker_cases()[key], max_new_tokens=frames)
    if both:  # every row ICL (7 and 4 reference frames): the common reference prefix is pre-decoded on a side stream
        case["icl"] = [(5, 7, True, False), (12, 4, True, False)]
    ids, ins, vcp, ref_ids = make_inputs(case, list(talker_cases()).index(key), cfg["talker_config"]["hidden_size"])
    kw = dict(input_ids=ids, instruct_ids=ins, ref_ids=ref_ids, voice_clone_prompt=vcp, languages=case["languages"],
              speakers=case["speakers"], non_streaming_mode=case["non_streaming_mode"], **gen_kwargs(case))
    codes, _ = model.generate(**kw)
    refs = vcp["ref_code"]
    dec = [torch.cat([refs[i].long(), c], 0) if refs[i] is not None else c for i, c in enumerate(codes)]
    wavs, _ = tok.decode([{"audio_codes": c} for c in dec])
    chunks = {}
    for b, pcm, last in model.stream(first_chunk_frames=2, chunk_frames=8, **kw):
        chunks.setdefault(b, []).append(pcm.cpu().numpy())
    up = model.speech_tokenizer.model.total_upsample
    for b, w in enumerate(wavs):
        R = 0 if refs[b] is None else int(refs[b].shape[0])
        cut = int(R / dec[b].shape[0] * w.shape[0]) if R else 0
        # the wrapper's proportional cut lands floor(555 R / T) samples before the reference/generated boundary (its
        # decoded length lacks the last frame's 555 lookahead samples) -- a point that moves with the final length
        # T; the stream starts at the boundary itself, so it equals the wrapper's PCM without those samples
        assert 0 <= up * R - cut <= 555, (cut, up * R)
        want = w[up * R:]
        got = np.concatenate(chunks[b])
        assert got.shape == want.shape, (b, got.shape, want.shape)
        np.testing.assert_allclose(got, want, atol=2e-4, rtol=0)


def test_stream_voice_clone_bad_request_releases_codec_slot(tiny_models):
    """stream() starts the reference-frame codec decode (a pooled CodecStream slot) before the prompt assembly; a
    request the assembly rejects (unknown language -> NotImplementedError, as the reference) must hand the slot back,
    so repeated bad requests do not grow the pool."""
    from cases import gen_kwargs, make_inputs, talker_cases
    from oracle import codec_param_specs, load_preset, synth_state_dict
    from qwen_tts import Qwen3TTSTokenizer
    _dev()
    cfg, W, model = tiny_models["tiny-customvoice"]
    _, ccfg = load_preset("tiny-customvoice")
    CW = {k: torch.from_numpy(v) for k, v in synth_state_dict(codec_param_specs(ccfg)).items()}
    tok = Qwen3TTSTokenizer.from_pretrained("synthetic:tiny-customvoice/speech_tokenizer", dtype="fp32", weights=CW)
    model.load_speech_tokenizer(tok)
    key = "icl_b2"
    case = dict(talker_cases()[key], max_new_tokens=6)
    case["icl"] = [(5, 7, True, False), (12, 4, True, False)]
    ids, ins, vcp, ref_ids = make_inputs(case, list(talker_cases()).index(key), cfg["talker_config"]["hidden_size"])
    kw = dict(input_ids=ids, instruct_ids=ins, ref_ids=ref_ids, voice_clone_prompt=vcp, speakers=case["speakers"],
              non_streaming_mode=case["non_streaming_mode"], **gen_kwargs(case))
    dec = model.speech_tokenizer.model
    for _ in range(3):
        with pytest.raises(NotImplementedError):
            next(iter(model.stream(languages=["klingon"] * len(ids), **kw)))
    torch.cuda.synchronize()
    slots = [sl for pool in dec._slots.values() for sl in pool]
    assert slots and not any(sl.busy for sl in slots)
    assert len(slots) == 1  # the one slot was reused by every attempt
    out = list(model.stream(languages=case["languages"], **kw))  # and a good request still streams
    assert out and out[-1][2]


def test_prefill_buffers_lru_bounded(tiny_models):
    """Static prefill buffers are kept for the PREFILL_CACHE most recently used prompt lengths only (LRU): a server
    seeing many distinct prompt lengths does not grow HBM without bound, and evicted / re-created lengths still
    decode exactly as before."""
    import gc
    from cases import talker_cases
    from qwen_tts import talker as T
    from qwen_tts.model import TTSModel
    cfg, W, _ = tiny_models["tiny-customvoice"]
    model = TTSModel(cfg, W, dtype="fp32")
    case = dict(talker_cases()["cv_b1_nonstream"], max_new_tokens=6)
    first, mem = {}, []
    for rep in range(2):
        for n in range(3, 13):  # 10 distinct prompt lengths, each twice (the second use captures a prefill graph)
            for _ in range(2):
                c, _ = _run_case(model, "cv_b1_nonstream", dict(case, texts=[n]), 0, cfg)
                if rep == 0 and n not in first:
                    first[n] = c
                else:
                    assert all(torch.equal(a, b) for a, b in zip(c, first[n])), n
            torch.cuda.synchronize()
            # unreachable cycles left by earlier tests (a dropped model's buffers) die whenever the collector next
            # runs, which may be between two of these readings: collect first, so only reachable memory is counted
            gc.collect()
            mem.append(torch.cuda.memory_allocated())
        for s in model.engine.all_sessions():
            assert len(s.prefill) <= T.PREFILL_CACHE
    # the second pass over the same lengths ends with the same PREFILL_CACHE lengths held: the same memory (a growing
    # cache would hold all ten lengths by now)
    assert mem[-1] == mem[len(mem) // 2 - 1], mem


def test_rope_growth_keeps_captured_graphs_valid(tiny_models):
    """Growing the talker's RoPE tables (a session with a longer K/V capacity) must not free the tables that graphs
    captured by pooled sessions still read: B=1, then the tables grow (old memory reused by new allocations), then
    the same B=1 request replays its captured frame graph -- identical codes."""
    from cases import talker_cases
    from qwen_tts.model import TTSModel
    cfg, W, _ = tiny_models["tiny-customvoice"]
    model = TTSModel(cfg, W, dtype="fp32")
    case = dict(talker_cases()["cv_b1_nonstream"], max_new_tokens=20)
    a, _ = _run_case(model, "cv_b1_nonstream", case, 0, cfg)
    t = model.engine.talker
    old = t.cos.data_ptr()
    t.ensure_rope(t.cos.shape[0] * 3, model.engine.dev)
    assert t.cos.data_ptr() != old
    torch.cuda.empty_cache()
    junk = [torch.full((1 << 20,), 7.0, device="cuda") for _ in range(16)]  # would land on freed tables
    b, _ = _run_case(model, "cv_b1_nonstream", case, 0, cfg)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    del junk


def test_codec_feed_graph_uses_slot_workspace():
    """A feed captured on a pooled stream slot while the caller had a temporary split-K workspace active (the
    voice-clone side-stream feed) must not bind that temporary: every feed of a slot uses the slot's own workspace,
    so later replays stay correct after the temporary is freed (B=1 -> skinny GEMVs use split-K)."""
    from oracle import codec_param_specs, load_preset, synth_state_dict
    from qwen_tts import kernels as Kn
    from qwen_tts.codec import CodecDecoder
    dev = _dev()
    _, ccfg = load_preset("tiny-customvoice")
    W = {k: torch.from_numpy(v) for k, v in synth_state_dict(codec_param_specs(ccfg)).items()}
    dec = CodecDecoder(ccfg, W, dtype="fp32", device=str(dev))
    g = torch.Generator().manual_seed(9)
    codes = torch.randint(1, dec.tables.shape[1], (1, 12, dec.tables.shape[0]), generator=g).to(dev, torch.int32)
    ref = dec.forward(codes)
    for rep in range(4):
        with Kn.use_workspace(Kn.new_workspace(dev)):
            cs = dec.stream(1, 12)
            cs.feed(codes[:, :4])
            cs.feed(codes[:, 4:12])
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        junk = [torch.full((1 << 20,), 3, dtype=torch.int32, device=dev) for _ in range(8)]  # reuse freed memory
        torch.testing.assert_close(cs.pcm[:, :cs.ns], ref[:, :cs.ns], atol=2e-5, rtol=0)
        assert rep < 2 or len(cs.slot.graphs) == 2
        cs.close()
        del junk
