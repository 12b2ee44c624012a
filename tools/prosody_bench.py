"""qt_prosody at the shapes the serving routes give it, for a rocprofv3 kernel trace.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o run -- python tools/prosody_bench.py --ratio 47/50
    python tools/prosody_bench.py --ratio 47/50 --db 6     # without a profiler: device-event time per call

--ratio U/D: the row's ratio T/S (every T and S in 50..200 is served; the tool takes T = U * k, S = D * k).  --db: the
gain; above 0 the rows are limited.  --mode report (default): `--rows` rows take `--frames` frames (1920 samples each)
per call, steady state, `--calls` calls after `--warmup`.  --mode first: every call is a fresh row's first packet, 1365
samples (each row is reset before it).  Prints one JSON line: the shape, the samples written per call and the mean
device time per call.
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
    ap.add_argument("--ratio", default="47/50", help="U/D = T/S in lowest terms")
    ap.add_argument("--db", type=float, default=0.0, help="gain in dB; above 0 the rows are limited")
    ap.add_argument("--mode", default="report", choices=["report", "first"])
    ap.add_argument("--rows", type=int, default=8)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    from qwen_tts import prosody as P
    U, D = (int(v) for v in a.ratio.split("/"))
    k = -(-50 // min(U, D))
    T, S = U * k, D * k
    dev = torch.device("cuda:0")
    n = 1365 if a.mode == "first" else 1920 * a.frames
    g = torch.Generator().manual_seed(5)
    t = torch.arange(n * 4, dtype=torch.float32) / 24000
    x = (0.3 * torch.sin(2 * torch.pi * 140 * t) + 0.1 * torch.randn(n * 4, generator=g)).to(dev)
    x = torch.stack([x[b * 37:b * 37 + n] for b in range(a.rows)]).contiguous()
    pp = P.PcmProsody(a.rows, dev)
    for b in range(a.rows):
        pp.reset(b, T, S, a.db)
    written = 0
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for c in range(a.warmup + a.calls):
        if c == a.warmup:
            torch.cuda.synchronize()
            ev[0].record()
            written = 0
        if a.mode == "first":
            for b in range(a.rows):
                pp.reset(b)
        outs = pp.push(x, [0] * a.rows, [n] * a.rows, False)
        written += sum(o.numel() for o in outs)
    ev[1].record()
    torch.cuda.synchronize()
    print(json.dumps({"tool": "prosody_bench", "mode": a.mode, "T": T, "S": S, "ratio": f"{pp.plan[0].up}/{pp.plan[0].down}",
                      "taps": pp.plan[0].taps, "db": a.db, "limited": a.db > 0, "rows": a.rows, "samples_per_row": n,
                      "samples_written_per_call": round(written / a.calls, 1),
                      "ms_per_call_with_host": round(ev[0].elapsed_time(ev[1]) / a.calls, 4)}), flush=True)


if __name__ == "__main__":
    main()
