"""qt_tempo at the shapes the serving routes give it, for a rocprofv3 kernel trace.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o run -- python tools/tempo_bench.py --step 125
    python tools/tempo_bench.py --step 125            # without a profiler: device-event time per call

--mode report (default): `--rows` rows take `--frames` frames (1920 samples each) per call, steady state, `--calls`
calls after `--warmup`.  --mode first: every call is a fresh row's first packet, 1365 samples (each row is reset before
it).  Prints one JSON line: the shape, the blocks computed per call and the mean device time per call.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "qwen3-tts_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", type=int, default=125, help="speed in hundredths, 50..200")
    ap.add_argument("--mode", default="report", choices=["report", "first"])
    ap.add_argument("--rows", type=int, default=8)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    from qwen_tts import tempo as T
    dev = torch.device("cuda:0")
    n = 1365 if a.mode == "first" else 1920 * a.frames
    g = torch.Generator().manual_seed(5)
    t = torch.arange(n * 4, dtype=torch.float32) / 24000
    x = (0.3 * torch.sin(2 * torch.pi * 140 * t) + 0.1 * torch.randn(n * 4, generator=g)).to(dev)
    x = torch.stack([x[b * 37:b * 37 + n] for b in range(a.rows)]).contiguous()
    tp = T.PcmTempo(a.rows, dev)
    steps = [a.step] * a.rows
    blocks = 0
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for c in range(a.warmup + a.calls):
        if c == a.warmup:
            torch.cuda.synchronize()
            ev[0].record()
            blocks = 0
        if a.mode == "first":
            for b in range(a.rows):
                tp.reset(b)
        outs = tp.push(x, [0] * a.rows, [n] * a.rows, False, steps)
        blocks += sum(o.numel() for o in outs) // T.HS
    ev[1].record()
    torch.cuda.synchronize()
    print(json.dumps({"tool": "tempo_bench", "mode": a.mode, "step": a.step, "rows": a.rows, "samples_per_row": n,
                      "blocks_per_call": round(blocks / a.calls, 2),
                      "ms_per_call_with_host": round(ev[0].elapsed_time(ev[1]) / a.calls, 4)}), flush=True)


if __name__ == "__main__":
    main()
