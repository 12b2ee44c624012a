"""stream(text_feed=...) against stream() at the bench configuration: 1.7B CustomVoice, synthetic weights,
bf16, 200-token texts, streaming text, 256 frames, sampling, B = 1 and B = 8.  Same ids, same process, the two paths
alternated, three runs each after one warm-up each:

  first packet   feed: from the submit of a head holding the first text token alone (nothing pushed yet) to the first
                 chunk complete on the device; stream(): from the call with the whole text to the same point
  frames/s       feed: every text token pushed and the rows closed before the first next(); stream(): the whole text
  append         one append replay (copy of ids + slots, fc1, fc2, qt_trail_append) with 1 and with 16 useful tokens:
                 host time per call and device time per call (events around 100 calls)

    python tools/text_feed_bench.py [--out profiles/text_feed_vs_stream.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "qwen3-tts_amd"))
import bench  # noqa: E402

SPK = ["vivian", "ryan", "serena", "aiden", "eric", "dylan", "sohee", "ono_anna"]
F = 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    from qwen_tts import Qwen3TTSModel, TextFeed
    cfg, W, CW = bench.make_weights("1.7b-customvoice", dev, 1, 0)
    tts = Qwen3TTSModel.from_pretrained("synthetic:1.7b-customvoice", device_map=str(dev), dtype=torch.bfloat16,
                                        weights=W, codec_weights=CW)
    model = tts.model
    gen = dict(max_new_tokens=F + 1, do_sample=True, top_k=50, top_p=1.0, temperature=0.9, subtalker_dosample=True,
               subtalker_top_k=50, subtalker_top_p=1.0, subtalker_temperature=0.9, repetition_penalty=1.05,
               ignore_eos=True, seed=7)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def consume(it, after_first=None):
        """(first packet ms, whole stream ms, samples) of a (row, pcm, last) stream started now"""
        t0 = time.perf_counter()
        first, n = None, 0
        for b, pcm, last in it:
            if first is None:
                torch.cuda.synchronize()
                first = (time.perf_counter() - t0) * 1e3
                if after_first is not None:
                    after_first()
            n += pcm.numel()
        torch.cuda.synchronize()
        return first, (time.perf_counter() - t0) * 1e3, n

    held = []
    eng = model.engine
    release = eng.release

    def rel(sessions):
        held[:] = sessions
        release(sessions)
    eng.release = rel

    for B in (1, 8):
        ids = [bench.synth_ids(200, i) for i in range(B)]
        rows = [i[0].tolist() for i in ids]
        kw = dict(languages=["english"] * B, speakers=SPK[:B], non_streaming_mode=False, **gen)

        def whole():
            return consume(model.stream(input_ids=ids, **kw))

        def fed(ahead):
            feed = TextFeed(rows=B, timeout=5.0)

            def rest():
                for b, r in enumerate(rows):
                    feed.push(r[4:-5], row=b)
                    feed.close(row=b)
            if ahead:
                rest()
            return consume(model.stream(input_ids=[torch.tensor([r[:4]]) for r in rows], text_feed=feed, **kw),
                           None if ahead else rest)

        whole(), fed(True), fed(False)  # warm-up: sessions, graphs, codec slots
        rs, ra, rl = [], [], []
        for _ in range(a.runs):
            rs.append(whole())
            ra.append(fed(True))
            rl.append(fed(False))
        fps = lambda r: [F / (x[1] / 1e3) for x in r]  # noqa: E731
        med = lambda v: float(np.median(v))  # noqa: E731

        def row(name, v, unit):
            return f"  {name:<44s} median {med(v):8.2f} {unit}   runs {' '.join(f'{x:.2f}' for x in v)}"
        say(f"B = {B}, {F} frames, 200-token texts ({a.runs} alternated runs each)")
        say(row("stream(): first packet", [x[0] for x in rs], "ms"))
        say(row("feed, first token only: first packet", [x[0] for x in rl], "ms"))
        say(row("feed, all text ahead: first packet", [x[0] for x in ra], "ms"))
        say(row("stream(): frames/s", fps(rs), "f/s"))
        say(row("feed, all text ahead: frames/s", fps(ra), "f/s"))
        say(row("feed, text after the first packet: frames/s", fps(rl), "f/s"))
        s_fp, s_fs = [x[0] for x in rs], fps(rs)
        say(f"  stream() spread: first packet {max(s_fp) - min(s_fp):.2f} ms, frames/s {max(s_fs) - min(s_fs):.2f}; "
            f"feed - stream(): first packet {med([x[0] for x in rl]) - med(s_fp):+.2f} ms, "
            f"frames/s {med(fps(ra)) - med(s_fs):+.2f}")
        # (bf16: the whole-text call projects its text through another GEMM route, so its sampled codes, and with
        # them the count of zero cb0 the length rule drops, may differ from the feed's; the two feed runs must agree)
        say(f"  samples: stream() {rs[0][2]}, feed ahead {ra[0][2]}, feed after the first packet {rl[0][2]}")
        assert ra[0][2] == rl[0][2], "the two feed deliveries produced different sample counts"
        # one append replay on the (idle) session of the last feed run
        s = held[0]
        for useful in (1, 16):
            items = [(j % B, j // B, rows[j % B][4 + j // B]) for j in range(useful)]
            for _ in range(5):
                eng.append_text(s, items)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            n = 100
            t0 = time.perf_counter()
            e0.record()
            for _ in range(n):
                eng.append_text(s, items)
            e1.record()
            host = (time.perf_counter() - t0) / n * 1e6
            torch.cuda.synchronize()
            say(f"  append replay, {useful:2d} useful tokens: host {host:6.1f} us per call, device "
                f"{e0.elapsed_time(e1) * 1e3 / n:6.1f} us per call")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
