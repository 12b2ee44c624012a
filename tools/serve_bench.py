"""Continuous batching vs padded one-shot batches on BASELINE.json configs[3]'s per-GPU work.

configs[3] = Qwen3-TTS-12Hz-1.7B VoiceDesign, 64 mixed-length requests data-parallel over 8 GPUs (SURVEY §8d:
text ~ U[40, 300] tokens, instruct ~ U[10, 60] tokens, F ~ U[64, 320] frames; non_streaming_mode=True, the
voice-design wrapper's default; sampling with the wrapper defaults).  Per request the frame count is fixed
(ignore_eos + a per-request cap), so both schedules generate the same audio:

* padded: the reference's schedule -- the requests in batches of `--slots`, each batch decoded until its longest
  request ends (finished rows emit EOS padding), M:2272-2292;
* serve: TalkerEngine.serve through `--slots` batch rows, a row refilled as soon as its request ends.

Both include prompt assembly and the codec decode of every request.  Prints one JSON line per schedule.

--stream adds a third schedule, TTSModel.serve_stream on the same list: the rows are refilled as in
`serve`, and every request's audio leaves in chunks while it decodes.  Its line also gives, per request, the time
from the moment its prefill was queued to its first chunk being complete on the host's side of the stream (p50, p90).

--sample-rate / --pcm select the stream's output format (resampled and converted on the device); the
defaults are the codec's own 24 kHz fp32.  --ab 16000:s16,48000:f32 runs those formats beside the selected one in the
same process, alternating within every repetition, one line each; --only-stream skips the first two schedules.

--voices K draws every request's instruction from K distinct ones (a voice product's traffic; 0, the default, gives
every request its own).  --prefix-cache runs the stream schedule with and without a qwen_tts.PrefixCache in
the same process, alternating within every repetition, one line each; the cache lives for the whole process, so the
measured runs are warm (their hits and misses are in the line).  --streaming-text puts only the first text token into
the prefill (non_streaming_mode=False) instead of the wrapper's default.  --speed 1.25 runs the stream
schedule with and without that speaking rate in the same process, alternating within every repetition, one line each.
--pitch 3 and / or --volume-gain-db 6 do the same with that pitch and gain (together with --speed: all of
them on against all of them off).

    python tools/serve_bench.py [--requests 8] [--slots 8] [--extra-slots 16,32] [--stream]
        [--sample-rate 16000 --pcm s16] [--ab 16000:s16,48000:f32] [--only-stream]
        [--voices 8] [--prefix-cache] [--streaming-text] [--speed 1.25] [--pitch 3] [--volume-gain-db 6]
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


def workload(n, seed=4, voices=0):
    """n requests (text ids, instruct ids, frames).  voices = K > 0: K instructions ~ U[10, 60] tokens are drawn first
    (a generator of their own, so texts and frame counts are those of the default workload) and every request picks
    one of them at random."""
    g = np.random.default_rng([seed, 99])
    gv = np.random.default_rng([seed, 98])
    wrap = lambda body: torch.tensor([[151644, 872, 198] + body + [151645, 198]], dtype=torch.long)  # noqa: E731
    vs = [wrap(gv.integers(1000, 150000, int(gv.integers(10, 61))).tolist()) for _ in range(voices)]
    reqs = []
    for i in range(n):
        t, k, f = int(g.integers(40, 301)), int(g.integers(10, 61)), int(g.integers(64, 321))
        body = g.integers(1000, 150000, t).tolist()
        ids = torch.tensor([[151644, 77091, 198] + body + [151645, 198, 151644, 77091, 198]], dtype=torch.long)
        ins = wrap(g.integers(1000, 150000, k).tolist())
        reqs.append((ids, vs[int(gv.integers(0, voices))] if voices else ins, f))
    return reqs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="1.7b-voicedesign")
    ap.add_argument("--requests", type=int, default=8)
    ap.add_argument("--slots", type=int, default=8)
    ap.add_argument("--extra-slots", default="")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--stream", action="store_true", help="also run the list through serve_stream")
    ap.add_argument("--chunk-frames", type=int, default=8)
    ap.add_argument("--sample-rate", type=int, default=None, help="output rate of the stream schedule (default 24000)")
    ap.add_argument("--pcm", default="f32", choices=["f32", "s16"], help="sample format of the stream schedule")
    ap.add_argument("--ab", default="", help="more rate:format pairs for the stream schedule, run alternately")
    ap.add_argument("--only-stream", action="store_true", help="skip the padded and serve schedules")
    ap.add_argument("--voices", type=int, default=0, help="draw the instructions from this many distinct ones")
    ap.add_argument("--prefix-cache", action="store_true", help="stream schedule with and without a PrefixCache")
    ap.add_argument("--streaming-text", action="store_true", help="non_streaming_mode=False (default True)")
    ap.add_argument("--speed", type=float, default=None, help="stream schedule with and without this speaking rate")
    ap.add_argument("--pitch", type=float, default=None, help="... and with and without this pitch in semitones")
    ap.add_argument("--volume-gain-db", type=float, default=None, help="... and with and without this gain in dB")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    from qwen_tts import PrefixCache, Qwen3TTSModel
    from qwen_tts.talker import GenParams
    _, W, CW = make_weights(a.preset, dev, 1, 0)
    tts = Qwen3TTSModel.from_pretrained(f"synthetic:{a.preset}", device_map=str(dev), dtype=torch.bfloat16,
                                        weights=W, codec_weights=CW)
    del W, CW
    m, eng = tts.model, tts.model.engine
    reqs = workload(a.requests, voices=a.voices)
    nsm = not a.streaming_text
    cache = PrefixCache() if a.prefix_cache else None
    F = [f for _, _, f in reqs]
    audio_s = 0.08 * sum(F)
    # F = max_new_tokens - 1 frames, as in bench.py; every row runs with ignore_eos so its length is exact
    gen = dict(do_sample=True, top_k=50, top_p=1.0, temperature=0.9, subtalker_dosample=True, subtalker_top_k=50,
               subtalker_top_p=1.0, subtalker_temperature=0.9, repetition_penalty=1.05, ignore_eos=True)

    def prompts(sel):
        return m.build_prompts([reqs[i][0] for i in sel], ["english"] * len(sel), None, [reqs[i][1] for i in sel],
                               nsm)

    def padded(slots, seed):
        codes = [None] * len(reqs)
        for b0 in range(0, len(reqs), slots):
            sel = list(range(b0, min(b0 + slots, len(reqs))))
            emb, mask, trail, pad = prompts(sel)
            gp = GenParams(max_new_tokens=max(F[i] for i in sel) + 1, seed=seed, **gen)
            out, _ = eng.generate_from_embeds(emb, mask, trail, pad, gp)
            for j, i in enumerate(sel):
                codes[i] = out[j][:F[i]]
        return codes

    def serve(slots, seed):
        emb, mask, trail, pad = prompts(list(range(len(reqs))))
        P = emb.shape[1]
        n_real = mask.sum(-1).tolist()
        rq = [(emb[i, P - int(n_real[i]):], trail[i], F[i]) for i in range(len(reqs))]
        gp = GenParams(max_new_tokens=max(F) + 1, seed=seed, **gen)
        codes = [None] * len(reqs)
        for i, c, _ in eng.serve(rq, pad, gp, slots=slots):
            codes[i] = c
        return codes

    first_ms = []

    formats = [(a.sample_rate, a.pcm)] + [(int(x.split(":")[0]), x.split(":")[1]) for x in a.ab.split(",") if x]

    # (format, with the prefix cache, (speaking rate, pitch, gain) or None) of every stream run
    ab = a.speed is not None or a.pitch is not None or a.volume_gain_db is not None
    variants = [(fmt, c, sp) for fmt in formats for c in ((False, True) if a.prefix_cache else (False,))
                for sp in ((None, (a.speed, a.pitch, a.volume_gain_db)) if ab else (None,))]

    def stream(slots, seed, var=variants[0]):
        """serve_stream: returns the samples received per request; first-chunk latencies go to first_ms"""
        fmt, cached, speed = var
        got, lat = [0] * len(reqs), {}
        out = {} if fmt == (None, "f32") else dict(sample_rate=fmt[0], pcm_format=fmt[1])
        if cached:
            out["prefix_cache"] = cache
        if speed is not None:
            out.update({k: v for k, v in zip(("speed", "pitch", "volume_gain_db"), speed) if v is not None})
        it = m.serve_stream(input_ids=[r[0] for r in reqs], instruct_ids=[r[1] for r in reqs],
                            languages=["english"] * len(reqs), non_streaming_mode=nsm, max_new_tokens=max(F) + 1,
                            seed=seed, frame_caps=F, max_batch=slots, first_chunk_frames=1,
                            chunk_frames=a.chunk_frames, **gen, **out)
        for i, pcm, last in it:
            if i not in lat:  # the chunk is usable once the stream has produced it
                torch.cuda.current_stream().synchronize()
                lat[i] = (time.perf_counter() - eng.serve_queued[i]) * 1e3
            got[i] += pcm.numel()
        first_ms[:] = [lat[i] for i in range(len(reqs))]
        return got

    def run_stream(slots):
        """{(format, cached): (wall times, first-chunk latencies, [hits, misses] of the measured runs)}; the variants
        alternate within every repetition"""
        res = {var: ([], [], [0, 0]) for var in variants}
        for var in variants:
            stream(slots, 1, var)  # warmup (graph captures, sessions, codec slot; fills the prefix cache)
        for r in range(a.reps):
            for var in variants:
                fmt = var[0]
                before = cache.stats if var[1] else None
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got = stream(slots, 10 + r, var)
                torch.cuda.synchronize()
                res[var][0].append(time.perf_counter() - t0)
                res[var][1].extend(first_ms)
                if var[1]:
                    res[var][2][0] += cache.stats["hits"] - before["hits"]
                    res[var][2][1] += cache.stats["misses"] - before["misses"]
                # every frame's 1920 samples but each reference chunk's last 555 (fewer only where a cb0 is 0), at
                # the output rate
                rate = 24000 if fmt[0] is None else fmt[0]
                S = 100 if var[2] is None or var[2][0] is None else int(round(100 * var[2][0]))
                assert all(0 < g <= -(-(-(-100 * (1920 * f - 555 * -(-f // 300)) // S)) * rate // 24000)
                           for g, f in zip(got, F)), got
        return res

    def run(fn, slots):
        fn(slots, 1)  # warmup (graph capture, sessions)
        ts = []
        for r in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            codes = fn(slots, 10 + r)
            assert [c.shape[0] for c in codes] == F, [c.shape[0] for c in codes]
            wavs, sr = m.speech_tokenizer.decode([{"audio_codes": c} for c in codes])
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return ts

    slot_list = [a.slots] + [int(x) for x in a.extra_slots.split(",") if x]
    for name, fn in (() if a.only_stream else (("padded", padded), ("serve", serve))):
        for slots in slot_list:
            if name == "padded" and slots != a.slots:
                continue
            ts = run(fn, slots)
            dt = float(np.median(ts))
            st = getattr(eng, "serve_stats", {}) if name == "serve" else {}
            print(json.dumps({"schedule": name, "slots": slots, "requests": a.requests, "frames": F,
                              "frames_replayed": st.get("frames"), "frames_min": -(-sum(F) // slots),
                              "audio_s": round(audio_s, 2), "wall_s": round(dt, 4),
                              "audio_s_per_s": round(audio_s / dt, 2),
                              "audio_s_per_s_runs": [round(audio_s / t, 2) for t in ts],
                              "workload": f"{a.preset} configs[3] shard, text U[40,300], instruct U[10,60], "
                                          "F U[64,320], sampling, ignore_eos + per-request cap, + codec decode"}),
                  flush=True)
    if a.stream:
        for slots, ((fmt, cached, speed), (ts, lats, hm)) in ((s, kv) for s in slot_list for kv in run_stream(s).items()):
            dt = float(np.median(ts))
            pc = {} if not a.prefix_cache else {"prefix_cache": cached}
            if a.speed is not None:
                pc["speed"] = 1.0 if speed is None else speed[0]
            if a.pitch is not None:
                pc["pitch"] = 0.0 if speed is None else speed[1]
            if a.volume_gain_db is not None:
                pc["volume_gain_db"] = 0.0 if speed is None else speed[2]
            if cached:
                pc.update(hits=hm[0], misses=hm[1], cache=cache.stats)
            st = getattr(eng, "serve_stats", {})
            print(json.dumps({"schedule": "serve_stream", "slots": slots, "requests": a.requests,
                              "sample_rate": 24000 if fmt[0] is None else fmt[0], "pcm": fmt[1], **pc,
                              "voices": a.voices, "non_streaming_mode": nsm,
                              "chunk_frames": a.chunk_frames, "frames_replayed": st.get("frames"),
                              "frames_min": -(-sum(F) // slots), "audio_s": round(audio_s, 2),
                              "wall_s": round(dt, 4), "audio_s_per_s": round(audio_s / dt, 2),
                              "audio_s_per_s_runs": [round(audio_s / t, 2) for t in ts],
                              "first_chunk_p50_ms": round(float(np.percentile(lats, 50)), 2),
                              "first_chunk_p90_ms": round(float(np.percentile(lats, 90)), 2),
                              "first_chunk_first_batch_p50_ms": round(float(np.percentile(
                                  [x for r in range(a.reps) for x in lats[r * len(reqs):r * len(reqs) + slots]], 50)), 2),
                              "workload": "as above, audio streamed per request (first chunk 1 frame)"}),
                  flush=True)


if __name__ == "__main__":
    main()
