"""One codec residual unit at the one-shot decode's shapes: the two igemm_k launches against qt_codec_resunit.
    python tools/codec_unit_bench.py [B] [T]      (B utterances x T frames; default 8 x 256)
Prints, per block (C = 192, C = 96) and dilation, the time of each route (mean of 5 after 2 warm-ups, device events),
its TFLOP/s and its GB/s (pair: 5 activation tensors; fused: 2 + the halo rows), and whether the outputs are equal.
With the probe library (QWEN3TTS_AMD_LIB=.../libqwen3tts_amd_probe.so) QT_CU_MI = 1 / 2 / 4 forces the fused
kernel's rows per block / 64 (C = 96: 1 or 4 instead of 2; C = 192: 2 instead of 1)."""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "qwen3-tts_amd"))
from qwen_tts import _hip, kernels as K  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 8
T = int(sys.argv[2]) if len(sys.argv) > 2 else 256
dev = torch.device("cuda:0")
K.gemm_workspace(dev)


def timed(fn, n=5):
    for _ in range(2):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(n):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / n


L = T * 4  # the two 2x upsampling stages
lens = {}
for r, c in ((8, 768), (5, 384), (4, 192), (3, 96)):
    L = (L - 1) * r
    lens[c] = L
g = torch.Generator().manual_seed(0)
knob = _hip.lib_knob("QT_CU_MI", 0)
print(f"codec residual unit, B={B} T={T}")
for C in (192, 96):
    L = lens[C]
    mi = {96: {1: 1, 4: 4}, 192: {2: 2, 4: 2}}[C].get(knob, 2 if C == 96 else 1)  # the library's choice
    x = torch.randn(B * L, C, generator=g).to(dev, torch.bfloat16)
    for dil in (1, 3, 9):
        w1, b1 = torch.randn(C, C, 7, generator=g) * 0.05, torch.randn(C, generator=g) * 0.1
        w2, b2 = torch.randn(C, C, 1, generator=g) * 0.1, torch.randn(C, generator=g) * 0.1
        sn = [torch.exp(0.3 * torch.randn(C, generator=g)).to(dev) for _ in range(4)]
        c1 = K.tile_conv(w1.to(dev), b1.to(dev), torch.bfloat16, dil)
        c2 = K.tile_conv(w2.to(dev), b2.to(dev), torch.bfloat16)
        bb, ref, out = torch.empty_like(x), x.clone(), torch.empty_like(x)

        def pair():
            K.gemm(x, c1, bb, B * L, C, C, conv=(L, L, -6 * dil, dil), snake=(sn[0], sn[1]))
            K.gemm(bb, c2, ref, B * L, C, C, conv=(L, L, 0, 1), snake=(sn[2], sn[3]), epi=_hip.EPI_ADD)

        def fused():
            K.codec_resunit(x, out, B, L, C, c1, (sn[0], sn[1]), c2, (sn[2], sn[3]))

        ref.copy_(x)
        pair()
        fused()
        same = torch.equal(ref, out)
        tp, tf = timed(pair), timed(fused)
        flop = 2.0 * B * L * C * C * 8
        tensor = B * L * C * 2
        halo = tensor * 6 * dil / (64 * mi)
        print(f"C={C:3d} dil={dil} rows={B * L} tile={64 * mi}: pair {tp:.3f} ms ({flop / tp / 1e9:.0f} TFLOP/s, {5 * tensor / tp / 1e6:.0f} GB/s)"
              f"  fused {tf:.3f} ms ({flop / tf / 1e9:.0f} TFLOP/s, {(2 * tensor + halo) / tf / 1e6:.0f} GB/s)"
              f"  x{tp / tf:.2f}  equal={same}", flush=True)
