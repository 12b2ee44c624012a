"""Live serving measured against serve_stream in one process.

1. throughput: `--requests` whole-text requests, all submitted ahead, through `--slots` rows -- TTSModel.serve_live
   against TTSModel.serve_stream on the same list (tools/serve_bench.py's workload without instructions: text ~
   U[40, 300] tokens, F ~ U[64, 320] frames fixed by ignore_eos + a per-request cap, sampling), alternating within
   every repetition.  serve_stream starts its first `slots` requests with one batched prefill, serve_live with
   `slots` single-request prefills.
2. held replay: the same frame replayed plainly and with one of the rows held (TalkerEngine._run_frame_held: a save
   launch in front, a restore launch behind), in alternating blocks, device time per replay from events.
3. first chunk of a request that arrives mid-run: `slots - 1` long requests keep the batch busy; short requests are
   submitted one after the other from the consumer loop, and the time from submit() to the request's first chunk being
   complete (stream synchronised) is taken.

Prints one JSON line per measurement.

    python tools/live_bench.py [--preset 1.7b-customvoice] [--requests 64] [--slots 8] [--reps 3]
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


def workload(n, seed=4):
    g = np.random.default_rng([seed, 99])
    reqs = []
    for _ in range(n):
        t, f = int(g.integers(40, 301)), int(g.integers(64, 321))
        body = g.integers(1000, 150000, t).tolist()
        reqs.append(([151644, 77091, 198] + body + [151645, 198, 151644, 77091, 198], f))
    return reqs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="1.7b-customvoice")
    ap.add_argument("--requests", type=int, default=64)
    ap.add_argument("--slots", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--chunk-frames", type=int, default=8)
    ap.add_argument("--held-frames", type=int, default=50, help="replays per block of the held-replay measurement")
    ap.add_argument("--arrivals", type=int, default=9)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    from qwen_tts import Qwen3TTSModel, RequestQueue
    from qwen_tts import kernels as K
    from qwen_tts.talker import GenParams
    _, W, CW = make_weights(a.preset, dev, 1, 0)
    tts = Qwen3TTSModel.from_pretrained(f"synthetic:{a.preset}", device_map=str(dev), dtype=torch.bfloat16,
                                        weights=W, codec_weights=CW)
    del W, CW
    m, eng = tts.model, tts.model.engine
    reqs = workload(a.requests)
    F = [f for _, f in reqs]
    audio_s = 0.08 * sum(F)
    gen = dict(do_sample=True, top_k=50, top_p=1.0, temperature=0.9, subtalker_dosample=True, subtalker_top_k=50,
               subtalker_top_p=1.0, subtalker_temperature=0.9, repetition_penalty=1.05)
    max_prompt = (max(len(ids) for ids, _ in reqs) + 16 + 63) // 64 * 64

    def expect(got):  # every frame's 1920 samples but each reference chunk's last 555 (fewer only where a cb0 is 0)
        assert all(0 < g <= 1920 * f - 555 * -(-f // 300) for g, f in zip(got, F)), got

    def stream(seed):
        got = [0] * len(reqs)
        for i, pcm, last in m.serve_stream(input_ids=[torch.tensor([ids]) for ids, _ in reqs],
                                           languages=["english"] * len(reqs), speakers=["vivian"] * len(reqs),
                                           non_streaming_mode=True, max_new_tokens=max(F) + 1, seed=seed,
                                           frame_caps=F, max_batch=a.slots, first_chunk_frames=1,
                                           chunk_frames=a.chunk_frames, ignore_eos=True, **gen):
            got[i] += pcm.numel()
        expect(got)

    def live(seed):
        q = RequestQueue(timeout=5.0)
        for ids, f in reqs:
            q.submit(ids, language="english", speaker="vivian", non_streaming_mode=True, frame_cap=f, **gen)
        q.close()
        got = [0] * len(reqs)
        for i, pcm, last in m.serve_live(q, max_batch=a.slots, max_prompt=max_prompt, max_new_tokens=max(F) + 1,
                                         seed=seed, first_chunk_frames=1, chunk_frames=a.chunk_frames,
                                         ignore_eos=True):
            got[i] += pcm.numel()
        expect(got)
        assert not q.rejected and not q.timed_out

    runs = {"serve_stream": stream, "serve_live": live}
    ts, replays = {k: [] for k in runs}, {}
    for fn in runs.values():
        fn(1)  # warmup: sessions, graph captures, codec slots
    for r in range(a.reps):
        for name, fn in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(10 + r)
            torch.cuda.synchronize()
            ts[name].append(time.perf_counter() - t0)
            replays[name] = eng.serve_stats["frames"]
    for name in runs:
        rate = [audio_s / t for t in ts[name]]
        print(json.dumps({"measure": "throughput", "schedule": name, "preset": a.preset, "slots": a.slots,
                          "requests": a.requests, "frames_replayed": replays[name], "audio_s": round(audio_s, 2),
                          "audio_s_per_s_median": round(float(np.median(rate)), 2),
                          "audio_s_per_s_runs": [round(x, 2) for x in rate]}), flush=True)

    # ---- 2. a held replay against a plain one
    B, n = a.slots, a.held_frames
    ids = [torch.tensor([reqs[i][0]]) for i in range(B)]
    emb, mask, trail, pad = m.build_prompts(ids, ["english"] * B, ["vivian"] * B, None, True)
    gp = GenParams(max_new_tokens=8 * n + 8, ignore_eos=True, seed=3, **gen)
    s = eng.session(B, emb.shape[1], gp.max_new_tokens - 1, gp)
    try:
        with K.use_workspace(s.ws):
            eng._prefill(s, emb, mask, trail, pad, 3)
        s.hiddens[:, 0].copy_(s.past_hidden)
        P, f = emb.shape[1], 0
        for hold in (0, 1 << 3):  # warm both paths (graph capture, the region table)
            eng._run_frame_held(s, P + f + 1, hold)
            f += 1
        # plain, held, plain, ..., plain: the rows' caches grow from block to block, so a held block is compared with
        # the mean of the plain blocks on either side of it
        us = []
        for blk in range(7):
            hold = (0, 1 << 3)[blk % 2]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                eng._run_frame_held(s, P + f + 1, hold)
                f += 1
            e1.record()
            e1.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3 / n)
    finally:
        eng.release([s])
    extra = [us[i] - (us[i - 1] + us[i + 1]) / 2 for i in (1, 3, 5)]
    print(json.dumps({"measure": "held_replay", "rows": B, "held_rows": 1, "replays_per_block": n,
                      "plain_us_per_replay": [round(x, 1) for x in us[0::2]],
                      "held_us_per_replay": [round(x, 1) for x in us[1::2]],
                      "extra_us_vs_neighbouring_plain_blocks": [round(x, 1) for x in extra],
                      "extra_us_median": round(float(np.median(extra)), 1),
                      "stash_row_bytes": s.held.row_bytes}), flush=True)

    # ---- 3. first chunk of a request that arrives while the batch is busy
    q = RequestQueue(timeout=5.0)
    for i in range(B - 1):
        q.submit(reqs[i][0], language="english", speaker="vivian", non_streaming_mode=True, frame_cap=320, **gen)
    sent, lat, left = {}, [], [a.arrivals]

    def arrive():
        if left[0] == 0:
            q.close()
            return
        left[0] -= 1
        j = B - 1 + len(sent)
        t0 = time.perf_counter()
        sent[q.submit(reqs[j % len(reqs)][0], language="english", speaker="vivian", non_streaming_mode=True,
                      frame_cap=24, **gen)] = t0
    started = False
    for i, pcm, last in m.serve_live(q, max_batch=B, max_prompt=max_prompt, max_new_tokens=321, seed=5,
                                     first_chunk_frames=1, chunk_frames=a.chunk_frames, ignore_eos=True):
        if not started:  # the batch is running: the first arrival
            started = True
            arrive()
        if i in sent and sent[i] is not None:
            torch.cuda.current_stream().synchronize()
            lat.append((time.perf_counter() - sent[i]) * 1e3)
            sent[i] = None
        if i in sent and last:
            arrive()
    print(json.dumps({"measure": "first_chunk_mid_run", "busy_rows": B - 1, "arrivals": len(lat),
                      "submit_to_first_chunk_ms": [round(x, 2) for x in lat],
                      "p50_ms": round(float(np.percentile(lat[1:], 50)), 2),
                      "note": "p50 over the arrivals after the first"}), flush=True)


if __name__ == "__main__":
    main()
