"""Voice-clone (ICL) requests through serve_stream() with a VoiceCache: 1.7B-Base dims, synthetic
weights, bf16.  64 requests over K = 4 voices with R-frame references (38 = a 3 s clip, 125 = 10 s) through 8 rows,
streaming text, sampling, ignore_eos + a per-request frame cap.  Four schedules alternate within every repetition:

* warmed: a VoiceCache filled by warm() before the run -- every request hits;
* cold:   a fresh VoiceCache per run -- the first request of each voice builds its entry (K misses);
* none:   VoiceCache(max_bytes=0) -- every request decodes its reference on the warm-up stream;
* xvec:   the same texts as x-vector-only requests without a cache: the route of the parent commit, and the yardstick
          for "a hit costs nothing".

One JSON line per (R, schedule): audio-s/s over the generated audio, and the time from a request's prefill being
queued to its first chunk being complete (p50 / p90).  Then the adopt launch on its own: device time between two
events around RowCodecStream.adopt_rows for 1 and for 8 rows, and the bytes it reads + writes over that time (the
block was just written or read, so this is the cache-resident rate, as it is in serving right after a build).

    python tools/voice_clone_serve_bench.py [--requests 64] [--voices 4] [--slots 8] [--refs 38,125] [--reps 3]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "qwen3-tts_amd"))
sys.path.insert(0, REPO)

from bench import make_weights  # noqa: E402


def workload(n, voices, R, H, seed=4):
    """n requests (text ids, voice index, frames) and K voices (reference codes [R, 16], x-vector, reference text)"""
    g = np.random.default_rng([seed, 101])
    wrap = lambda body: torch.tensor([[151644, 77091, 198] + body + [151645, 198]], dtype=torch.long)  # noqa: E731
    vs = [(torch.tensor(g.integers(1, 2048, (R, 16)), dtype=torch.long),
           torch.tensor(0.02 * g.standard_normal(H), dtype=torch.float32),
           wrap(g.integers(1000, 150000, 40).tolist())) for _ in range(voices)]
    reqs = []
    for i in range(n):
        t, f = int(g.integers(40, 121)), int(g.integers(32, 97))
        body = g.integers(1000, 150000, t).tolist()
        ids = torch.tensor([[151644, 77091, 198] + body + [151645, 198, 151644, 77091, 198]], dtype=torch.long)
        reqs.append((ids, int(g.integers(0, voices)), f))
    return reqs, vs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="1.7b-base")
    ap.add_argument("--requests", type=int, default=64)
    ap.add_argument("--voices", type=int, default=4)
    ap.add_argument("--slots", type=int, default=8)
    ap.add_argument("--refs", default="38,125")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--chunk-frames", type=int, default=8)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    from qwen_tts import Qwen3TTSModel, VoiceCache
    _, W, CW = make_weights(a.preset, dev, 1, 0)
    tts = Qwen3TTSModel.from_pretrained(f"synthetic:{a.preset}", device_map=str(dev), dtype=torch.bfloat16,
                                        weights=W, codec_weights=CW)
    del W, CW
    m, eng = tts.model, tts.model.engine
    dec = m.speech_tokenizer.model
    H = m.tc["hidden_size"]
    gen = dict(do_sample=True, top_k=50, top_p=1.0, temperature=0.9, subtalker_dosample=True, subtalker_top_k=50,
               subtalker_top_p=1.0, subtalker_temperature=0.9, repetition_penalty=1.05, ignore_eos=True)
    for R in [int(x) for x in a.refs.split(",") if x]:
        reqs, vs = workload(a.requests, a.voices, R, H)
        F = [f for _, _, f in reqs]
        audio_s = 0.08 * sum(F)
        N = len(reqs)

        def vcp(icl):
            return dict(ref_code=[vs[v][0] if icl else None for _, v, _ in reqs],
                        ref_spk_embedding=[vs[v][1] for _, v, _ in reqs], x_vector_only_mode=[not icl] * N,
                        icl_mode=[icl] * N)
        warmed = VoiceCache()
        warmed.warm(m, vcp(True))
        caches = {"warmed": lambda: warmed, "cold": VoiceCache, "none": lambda: VoiceCache(max_bytes=0),
                  "xvec": lambda: None}

        def run(name, seed):
            cache = caches[name]()
            icl = name != "xvec"
            lat, got = {}, [0] * N
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i, pcm, last in m.serve_stream(input_ids=[r[0] for r in reqs],
                                               ref_ids=[vs[v][2] for _, v, _ in reqs] if icl else None,
                                               voice_clone_prompt=vcp(icl), languages=["english"] * N,
                                               non_streaming_mode=False, max_new_tokens=max(F) + 1, seed=seed,
                                               frame_caps=F, max_batch=a.slots, first_chunk_frames=1,
                                               chunk_frames=a.chunk_frames, voice_cache=cache, **gen):
                if i not in lat:  # the chunk is usable once the stream has produced it
                    torch.cuda.current_stream().synchronize()
                    lat[i] = (time.perf_counter() - eng.serve_queued[i]) * 1e3
                got[i] += pcm.numel()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert all(0 < x <= 1920 * f for x, f in zip(got, F)), got
            return dt, [lat[i] for i in range(N)], None if cache is None else cache.stats

        res = {k: ([], [], None) for k in caches}
        for k in caches:  # warm-up: sessions, frame graphs, codec slots and their feed graphs
            run(k, 1)
            run(k, 2)
        for r in range(a.reps):
            for k in caches:
                before = None if k != "warmed" else warmed.stats
                dt, lats, st = run(k, 10 + r)
                res[k][0].append(dt)
                res[k][1].extend(lats)
                if k == "warmed":
                    st = {x: st[x] - before[x] for x in ("hits", "misses")}
                res[k] = (res[k][0], res[k][1], st)
        for k, (ts, lats, st) in res.items():
            dt = float(np.median(ts))
            print(json.dumps({"schedule": k, "ref_frames": R, "requests": N, "voices": a.voices, "slots": a.slots,
                              "chunk_frames": a.chunk_frames, "audio_s": round(audio_s, 2), "wall_s": round(dt, 4),
                              "audio_s_per_s": round(audio_s / dt, 2),
                              "audio_s_per_s_runs": [round(audio_s / t, 2) for t in ts],
                              "first_chunk_p50_ms": round(float(np.percentile(lats, 50)), 2),
                              "first_chunk_p90_ms": round(float(np.percentile(lats, 90)), 2),
                              "cache_last_run": st}), flush=True)

        # the adopt launch alone
        entry = warmed._entries[warmed.keys()[0]]
        rs = dec.row_stream(a.slots, 325, a.chunk_frames)
        try:
            tab = rs._state_table()
            hist = sum(h[0].numel() * h.element_size() for h in tab.keep[0])
            kv = 2 * len(dec.layers) * dec.kvh * min(entry.R, dec.d["sliding_window"]) * dec.hd * 4
            for rows in (1, a.slots):
                pairs = [(b, entry.snapshot) for b in range(rows)]
                for _ in range(5):
                    rs.adopt_rows(pairs)
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                iters = 200
                ev[0].record()
                for _ in range(iters):
                    rs.adopt_rows(pairs)
                ev[1].record()
                torch.cuda.synchronize()
                ms = ev[0].elapsed_time(ev[1]) / iters
                moved = 2 * rows * (hist + kv + 4)
                print(json.dumps({"adopt_rows": rows, "ref_frames": R, "block_bytes": tab.block_bytes,
                                  "bytes_read_and_written": moved, "launch_ms": round(ms, 4),
                                  "GB_per_s": round(moved / (ms * 1e-3) / 1e9, 1),
                                  "note": "200 back-to-back launches between two events: includes the launch gap"}),
                      flush=True)
        finally:
            rs.close()


if __name__ == "__main__":
    main()
