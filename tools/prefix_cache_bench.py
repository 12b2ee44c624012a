"""First packet of stream() with and without the prefix cache: 1.7B VoiceDesign, synthetic weights, bf16,
B = 1 and B = 8 rows of 200-token texts that share one 60-token instruction, streaming text (the prefill holds the
instruction, the role ids, the codec prefix and the first text token), sampling.

Per batch size the cached and the uncached call alternate within every repetition; the cache is filled by the warm-up,
so every measured cached call hits for all its rows.  Prints one JSON line per (B, cached) with the first-packet p50 /
p90 (host time from the call to the first chunk being complete) and, for the cached calls, the device time between two
events around TalkerEngine._prefill_cached (adopt + suffix prefill + first token).

    python tools/prefix_cache_bench.py [--reps 20] [--batches 1,8] [--frames 9]
    python tools/prefix_cache_bench.py --profile    # a few cached B = 1 calls only, for a kernel trace
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "qwen3-tts_amd"))
import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--frames", type=int, default=9)
    ap.add_argument("--text", type=int, default=200)
    ap.add_argument("--instruct", type=int, default=60)
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    from qwen_tts import PrefixCache, Qwen3TTSModel
    _, W, CW = bench.make_weights("1.7b-voicedesign", dev, 1, 0)
    tts = Qwen3TTSModel.from_pretrained("synthetic:1.7b-voicedesign", device_map=str(dev), dtype=torch.bfloat16,
                                        weights=W, codec_weights=CW)
    del W, CW
    m, eng = tts.model, tts.model.engine
    g = np.random.default_rng([5, 97])
    ins = torch.tensor([[151644, 872, 198] + g.integers(1000, 150000, a.instruct - 5).tolist() + [151645, 198]],
                       dtype=torch.long)
    gen = dict(max_new_tokens=a.frames + 1, do_sample=True, top_k=50, top_p=1.0, temperature=0.9,
               subtalker_dosample=True, subtalker_top_k=50, subtalker_top_p=1.0, subtalker_temperature=0.9,
               repetition_penalty=1.05, ignore_eos=True)
    cache = PrefixCache()
    spans = []  # (start, end) events around the cached prefills of the current call
    inner = eng._prefill_cached

    def timed(*args, **kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        inner(*args, **kw)
        e1.record()
        spans.append((e0, e1))
    eng._prefill_cached = timed

    def run(B, cached, seed):
        ids = [bench.synth_ids(a.text, i) for i in range(B)]
        spans.clear()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        first = None
        for b, pcm, last in m.stream(input_ids=ids, instruct_ids=[ins] * B, languages=["english"] * B,
                                     non_streaming_mode=False, seed=seed, first_chunk_frames=1, chunk_frames=8,
                                     prefix_cache=cache if cached else None, **gen):
            if first is None:
                torch.cuda.current_stream().synchronize()
                first = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
        return first, [e0.elapsed_time(e1) for e0, e1 in spans]

    if a.profile:
        for r in range(6):
            run(1, True, r)
        print(json.dumps({"profile": "6 cached B = 1 calls", "cache": cache.stats}), flush=True)
        return
    for B in [int(x) for x in a.batches.split(",") if x]:
        for cached in (False, True):  # warm-up: sessions, graphs (the prefill graph from its second use), the entry
            for r in range(3):
                run(B, cached, r)
        res = {False: ([], []), True: ([], [])}
        before = cache.stats
        for r in range(a.reps):
            for cached in (False, True):
                first, dev_ms = run(B, cached, 10 + r)
                res[cached][0].append(first)
                res[cached][1].extend(dev_ms)
        for cached in (False, True):
            fp, dm = res[cached]
            line = {"B": B, "prefix_cache": cached, "text": a.text, "instruct": a.instruct, "reps": a.reps,
                    "first_packet_p50_ms": round(float(np.percentile(fp, 50)), 3),
                    "first_packet_p90_ms": round(float(np.percentile(fp, 90)), 3)}
            if cached:
                line.update(cached_prefill_device_p50_ms=round(float(np.percentile(dm, 50)), 3),
                            hits=cache.stats["hits"] - before["hits"], misses=cache.stats["misses"] - before["misses"])
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
