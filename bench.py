"""Benchmark: Qwen3-TTS-12Hz-1.7B CustomVoice, batch 8 x 200-token prompts, streaming-text decode
(BASELINE.json configs[2]) on the MI355X HIP path.

    python bench.py [--gpus N --steps K --warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1 bench.py --gpus N ...

A plain run sets up, warms up, times the K steps and prints the result line (value, ms_per_step).  `--full` adds every
other figure, each measured in runs of its own after the timed steps: batch 1, first-packet latencies, the kernel
table and rooflines (`--roofline 0` leaves them out) and the CPU baseline (`--cpu-baseline 0` leaves it out).
`--dump-outputs DIR` writes what the last timed step returned to its caller, per utterance i of the batch:
DIR/codes_<i>.npy (frames x code groups) and DIR/pcm_<i>.npy (24 kHz PCM), float32 (`r<rank>_` in front with more
than one rank).  Weights, token ids and the sampling seed of every step are fixed, so two runs with the same arguments
see the same inputs.

`--gpus N` (N > 1) without a launcher starts the N ranks itself (torch.distributed.run in a child process, before
this process makes any GPU call); under a launcher WORLD_SIZE must equal N.  Ranks talk over RCCL ("nccl").

One step = prefill + 256 AR frames (talker + 15-step code predictor per frame, HIP-graph replay) +
12 Hz codec decode of all 8 utterances to 24 kHz PCM.  Weak scaling: every rank serves its own batch of
8 independent utterances (data parallel, no collective on the data path; RCCL only broadcasts the
weights at init).  Weights are seeded synthetic at the ASSUMED 1.7B dims (no checkpoint offline).
value = sum over ranks of generated audio seconds / max-over-ranks wall time of the K timed steps.
Prints ONE JSON line on rank 0.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(REPO, "qwen3-tts_amd"))
sys.path.insert(0, REPO)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec (MI355X_MICROARCH.md)
# Infinity Cache (256 MiB die-level L3): no spec rate in the guide; its measured read rate from a 38 MB table gathered
# chip-wide (MI355X_MICROARCH.md, "Indexed rows: gather into LDS": 8.6 TB/s) is the second bound of kernels whose bytes
# stay resident there between two uses (the code predictor's 157 MB of layer weights, re-read by the 15 forwards of a
# frame with ~161 MB touched in between)
IC_RATE_GBS = 8600.0
MFMA_BF16_PEAK_TFS = 2500.0  # MI355X dense bf16 MFMA peak (no sparsity), MI355X_MICROARCH.md


def synth_ids(n, seed):
    g = np.random.default_rng([1234, seed])
    body = g.integers(1000, 150000, n).tolist()
    return torch.tensor([[151644, 77091, 198] + body + [151645, 198, 151644, 77091, 198]], dtype=torch.long)


def make_weights(preset, dev, world, rank):
    from qwen_tts.weights import codec_specs, read_json, resolve_path, synthetic, talker_specs
    d = resolve_path(f"synthetic:{preset}")
    cfg = read_json(os.path.join(d, "config.json"))
    ccfg = read_json(os.path.join(d, "speech_tokenizer", "config.json"))
    specs_t, specs_c = talker_specs(cfg), codec_specs(ccfg)
    if world > 1:  # rank 0 generates, RCCL broadcast over xGMI (the only collective of the design)
        from qwen_tts.dp import broadcast_weights
        W = synthetic(specs_t, dev) if rank == 0 else {n: torch.empty(s, device=dev) for n, s in specs_t}
        CW = synthetic(specs_c, dev) if rank == 0 else {n: torch.empty(s, device=dev) for n, s in specs_c}
        broadcast_weights(W)
        broadcast_weights(CW)
    else:
        W, CW = synthetic(specs_t, dev), synthetic(specs_c, dev)
    return cfg, W, CW


def _graph_us(run, dev, reps=10):
    """Capture run() into a HIP graph on a side stream, replay it `reps` times between HIP events recorded on that
    stream; returns microseconds per replay (the per-launch dispatch gaps of the graph included)."""
    st = torch.cuda.Stream(device=dev)
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        run()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            run()
        g.replay()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(reps):
            g.replay()
        e1.record(st)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def frame_bytes(cfg, B, L_talker):
    """Algorithmic HBM bytes of one AR frame for B rows at talker cache length L_talker: every
    talker weight once (28 layers + codec_head), per code-predictor forward (the 2-token prefill + 14 decode steps =
    15) the 5 layers + that step's lm_head, small_to_mtp once, the talker K/V of every row (28 x 2 x Hkv x D x 2 x L)
    and the code predictor's K/V (keys 2..16 over the 15 forwards)."""
    t, c = cfg["talker_config"], cfg["talker_config"]["code_predictor_config"]

    def layer_params(d):
        H, I, hq, hkv, D = d["hidden_size"], d["intermediate_size"], d["num_attention_heads"], d["num_key_value_heads"], \
            d["head_dim"]
        return H * (hq + 2 * hkv) * D + hq * D * H + 3 * H * I
    w_t = t["num_hidden_layers"] * layer_params(t) + t["vocab_size"] * t["hidden_size"]
    w_cp = c["num_hidden_layers"] * layer_params(c) + c["vocab_size"] * c["hidden_size"]
    # the 14 decode steps never read layer 0's q/k/v weights: their rows come from the precomputed table (bf16 mode)
    qkv0 = c["hidden_size"] * (c["num_attention_heads"] + 2 * c["num_key_value_heads"]) * c["head_dim"]
    s2m = t["hidden_size"] * c["hidden_size"] if t["hidden_size"] != c["hidden_size"] else 0
    kv_t = t["num_hidden_layers"] * 2 * t["num_key_value_heads"] * t["head_dim"] * 2 * L_talker
    kv_cp = sum(c["num_hidden_layers"] * 2 * c["num_key_value_heads"] * c["head_dim"] * 2 * j for j in range(2, 17))
    return 2 * (w_t + 15 * w_cp - 14 * qkv0 + s2m) + B * (kv_t + kv_cp)


def _gemv_entry(name, kernel, n_frame, Ws, M, K, N, a_dtype, o_dtype, dev, rms=False, epi=None, reps=10,
                extra_bytes=0):
    """One decode GEMV shape timed live: a HIP graph of one launch per weight in Ws (the model's distinct per-layer
    weights, as in a frame), replayed `reps` times between HIP events on the capture stream.  Algorithmic bytes per
    launch = weight tiles + M x K activations + M x N outputs (x2 + the bf16 shadow for a residual add)."""
    from qwen_tts import _hip, kernels as Kn
    A = torch.randn(M, K, device=dev).to(a_dtype)
    out = torch.randn(M, N, device=dev).to(o_dtype)
    x16 = torch.empty(M, N, dtype=torch.bfloat16, device=dev) if epi == _hip.EPI_ADD else None
    e = _hip.EPI_STORE if epi is None else epi
    N_out = N // 2 if e == _hip.EPI_SWIGLU else N
    if e == _hip.EPI_SWIGLU:
        out = torch.empty(M, N_out, dtype=o_dtype, device=dev)

    def run():
        for W in Ws:
            Kn.gemm(A, W, out, M, K, N_out, rms=rms, eps=1e-6, epi=e, out2=x16)
    us = _graph_us(run, dev, reps) / len(Ws)
    w_bytes = Ws[0].w.numel() * Ws[0].w.element_size()
    o_el = torch.tensor([], dtype=o_dtype).element_size()
    a_el = torch.tensor([], dtype=a_dtype).element_size()
    byt = w_bytes + M * K * a_el + M * N_out * o_el * (2 if e == _hip.EPI_ADD else 1) + (M * N_out * 2 if x16 is not None
                                                                                       else 0) + extra_bytes
    return dict(name=name, kernel=kernel, bound="hbm", launches_per_frame=n_frame, avg_us=us, bytes=byt)


def attn_oproj_entry(tts, B, pos=9, reps=20, n_frame=None):
    """Code-predictor fused attention + o_proj + residual (attn_oproj_k) at cache position `pos` (the mean over the 14
    decode steps), 5 launches over the 5 layers' distinct o_proj weights per replay.  Algorithmic bytes per launch =
    o_proj weights + K/V of (pos + 1) keys + the q/k/v rows read + the residual read and written (fp32 + bf16)."""
    from qwen_tts import kernels as Kn
    eng = tts.model.engine
    c, dev = eng.cp, eng.dev
    kc = [torch.randn(B, c.Hkv, 18, c.D, device=dev).to(eng.kv_dtype) for _ in c.layers]
    vc = [torch.randn(B, c.Hkv, 18, c.D, device=dev).to(eng.kv_dtype) for _ in c.layers]
    qkv = torch.randn(B, c.qkv_w, device=dev)
    x = torch.randn(B, c.H, device=dev)
    x16 = x.to(torch.bfloat16) if eng.wdt == torch.bfloat16 else None
    # the form the engine runs: head-split when its code-predictor scratch carries the hand-off workspace
    ss = [s for s in eng.all_sessions() if s.cp.sc.get("ao_ws") is not None]
    ws = torch.zeros_like(ss[0].cp.sc["ao_ws"]) if ss else None

    def run():
        for i, L in enumerate(c.layers):
            Kn.decode_attn_oproj(qkv, B, c.Hq, c.Hkv, c.D, L.q_norm, L.k_norm, c.eps, c.cos, c.sin, kc[i], vc[i], 18,
                                 L.o, x, const_pos=pos, x16=x16, ws=ws)
    us = _graph_us(run, dev, reps) / len(c.layers)
    L0 = c.layers[0]
    byt = (L0.o.w.numel() * L0.o.w.element_size() + B * c.Hkv * (pos + 1) * c.D * 2 * kc[0].element_size()
           + B * c.qkv_w * 4 + B * c.H * (4 + 4 + (2 if x16 is not None else 0)))
    kname = "attn_oproj_hs_k (head-split" if ws is not None else "attn_oproj_k ("
    return dict(name="cp_attn_oproj", kernel=f"{kname} code-predictor attention + o_proj + residual, {pos + 1} keys)",
                bound="hbm", launches_per_frame=5 * (eng.G - 2) if n_frame is None else n_frame, avg_us=us, bytes=byt,
                pmc_tag="attn_oproj_hs" if ws is not None else "attn_oproj")


def cp_step_entry(tts, B, Lmax=18, reps=20):
    """The code-predictor step engine (cp_step_k: 5 layers + lm_head[g] in one persistent launch), the 14 decode steps
    of a frame (cache positions 2..15, lm_head 1..14) captured in one graph.  Algorithmic bytes per launch = what the
    kernel reads and writes: the weights of layers 1-4 and layer 0's o_proj / gate-up / down (layer 0's q/k/v rows
    come from the table, its q/k/v weights are never read) + lm_head[g] + the K/V rows read (pos keys per layer) and
    the new key written + the x and layer-0 q/k/v input rows + the logits written (+ the previous logits read by the
    fused token choice)."""
    from qwen_tts import kernels as Kn
    eng = tts.model.engine
    c, dev = eng.cp, eng.dev
    kc = [torch.randn(B, c.Hkv, Lmax, c.D, device=dev).to(eng.kv_dtype) for _ in c.layers]
    vc = [torch.randn(B, c.Hkv, Lmax, c.D, device=dev).to(eng.kv_dtype) for _ in c.layers]
    qkv = torch.randn(B, c.qkv_w, device=dev)
    x = torch.randn(B, c.H, device=dev)
    logits = torch.empty(B, eng.Vc, device=dev)
    ws = torch.zeros(Kn.cp_step_ws_bytes(), dtype=torch.uint8, device=dev)
    steps = list(range(1, eng.G - 1))
    from qwen_tts.talker import CP_FUSE_SAMPLE
    fuse = CP_FUSE_SAMPLE and eng.cp_in_tabs is not None and eng.cp_qkv_tabs is not None
    if fuse:  # each launch first makes the previous step's token choice (qt_cp_step_sampled), as in a frame
        logits.normal_()
        i32 = lambda v: torch.full((B,), v, dtype=torch.int32, device=dev)  # noqa: E731
        tok, stp, prow = i32(0), i32(0), torch.arange(B, dtype=torch.int32, device=dev)
        seed = torch.tensor([7], dtype=torch.int64, device=dev)
        codes = torch.zeros(B, 4 * eng.G, dtype=torch.int32, device=dev)
        sas = [Kn.sample(logits, B, eng.Vc, eng.Vc, tok, do_sample=True, top_k=50, top_p=1.0, temperature=0.9,
                         seed_ptr=seed, step=stp, substep=g, codes=codes, codes_ld=4 * eng.G, codes_w=eng.G,
                         codes_col=g, ctr_stride=1, philox_row=prow, emb=(eng.cp_in_tabs[g - 1], x, c.H),
                         emb2=(eng.cp_qkv_tabs[g - 1], qkv, c.qkv_w), launch=False) for g in steps]

    def run():
        for i, g in enumerate(steps):
            Kn.cp_step(c.layers, eng.lm_heads[g], x, qkv, B, kc, vc, Lmax, g + 1, c.cos, c.sin, c.eps, logits, ws,
                       sample=sas[i] if fuse else None)
    us = _graph_us(run, dev, reps) / len(steps)
    assert int(ws[:4].view(torch.int32).item()) == 0, "cp_step hand-off flag set during the kernel-table run"
    nb = lambda W: W.w.numel() * W.w.element_size()  # noqa: E731  (tiled bf16 weights, no padding at these dims)
    wb = sum(nb(L.o) + nb(L.gu) + nb(L.down) + (nb(L.qkv) if i > 0 else 0) for i, L in enumerate(c.layers))
    lm = nb(eng.lm_heads[1])
    el = kc[0].element_size()
    kv = sum(len(c.layers) * B * c.Hkv * c.D * el * (2 * (g + 1) + 2) for g in steps) / len(steps)
    # x + layer-0 q/k/v input rows (the chosen tokens' table rows when fused) and the logits written
    byt = int(wb + lm + kv + B * (c.H + c.qkv_w + eng.Vc) * 4)
    if fuse:  # + the previous step's logits rows read by the token choice
        byt += B * eng.Vc * 4
    return dict(name="cp_step", kernel="cp_step_k (code-predictor step engine: 5 layers + lm_head in one launch, "
                "keys 2..15" + (", the previous step's token choice first" if fuse else "") + ")", bound="hbm",
                launches_per_frame=len(steps), avg_us=us, bytes=byt, pmc_tag="cp_step", ic_resident=True)


def cp_prefill_entry(tts, B, Lmax=18, reps=20):
    """The code predictor's 2-token prefill through the step engine (cp_step_k<1, 1>: 2B token rows, every layer +
    lm_head[0]), one launch per frame.  Algorithmic bytes per launch = the 5 layers' weights + lm_head[0] + the K/V rows
    written (positions 0, 1) + x and the logits."""
    from qwen_tts import kernels as Kn
    eng = tts.model.engine
    c, dev = eng.cp, eng.dev
    kc = [torch.zeros(B, c.Hkv, Lmax, c.D, device=dev, dtype=eng.kv_dtype) for _ in c.layers]
    vc = [torch.zeros(B, c.Hkv, Lmax, c.D, device=dev, dtype=eng.kv_dtype) for _ in c.layers]
    x = torch.randn(2 * B, c.H, device=dev)
    logits = torch.empty(B, eng.Vc, device=dev)
    ws = torch.zeros(Kn.cp_step_ws_bytes(), dtype=torch.uint8, device=dev)

    def run():
        for _ in range(4):
            Kn.cp_prefill(c.layers, eng.lm_heads[0], x, B, kc, vc, Lmax, c.cos, c.sin, c.eps, logits, ws)
    us = _graph_us(run, dev, reps) / 4
    assert int(ws[:4].view(torch.int32).item()) == 0, "cp_prefill hand-off flag set during the kernel-table run"
    L0 = c.layers[0]
    wb = sum(W.w.numel() * W.w.element_size() for W in (L0.qkv, L0.o, L0.gu, L0.down)) * len(c.layers)
    lm = eng.lm_heads[0].w.numel() * eng.lm_heads[0].w.element_size()
    kv = len(c.layers) * B * c.Hkv * c.D * kc[0].element_size() * 4
    byt = int(wb + lm + kv + B * (2 * c.H + eng.Vc) * 4)
    return dict(name="cp_prefill", kernel="cp_step_k<1, 1> (code-predictor 2-token prefill through the step engine)",
                bound="hbm", launches_per_frame=1, avg_us=us, bytes=byt, ic_resident=True)


def talker_tail_entry(tts, B, reps=5):
    """The talker decode-layer tail engine (talker_tail_k: o_proj, gate/up, down, next q/k/v in one launch), 28
    launches over the talker's distinct per-layer weights captured in one graph (every launch streams its weights from
    HBM, as in a frame).  Algorithmic bytes per launch = the four matrices' bf16 weights + the attention rows in + x
    read and written (fp32) + the q/k/v rows out."""
    from qwen_tts import kernels as Kn
    eng = tts.model.engine
    t, dev = eng.talker, eng.dev
    att = torch.randn(B, t.Hq * t.D, device=dev).to(torch.bfloat16)
    x = torch.randn(B, t.H, device=dev)
    qkv = torch.empty(B, t.qkv_w, device=dev)
    ws = torch.zeros(Kn.talker_tail_ws_bytes(), dtype=torch.uint8, device=dev)
    nl = t.n_layers

    def run():
        for i in range(nl):
            Kn.talker_tail(att, x, B, t.layers[i], t.layers[i + 1] if i + 1 < nl else t.layers[0], qkv, t.eps, ws)
    us = _graph_us(run, dev, reps) / nl
    assert int(ws[:4].view(torch.int32).item()) == 0, "talker tail hand-off flag set during the kernel-table run"
    L0 = t.layers[0]
    wb = sum(W.w.numel() * W.w.element_size() for W in (L0.o, L0.gu, L0.down, L0.qkv))
    byt = int(wb + B * t.Hq * t.D * 2 + B * t.H * 8 + B * t.qkv_w * 4)
    return dict(name="talker_tail", kernel="talker_tail_k (talker o_proj + gate/up + down + next q/k/v in one launch, "
                "LDS weight ring)", bound="hbm", launches_per_frame=nl, avg_us=us, bytes=byt, pmc_tag="talker_tail")


def decode_kernel_table(tts, B, L_mean):
    """Every decode kernel of a frame timed live at its production shape (B rows, bf16): per-launch time x launches per
    frame gives each kernel's share of the frame; `roofline` in the JSON line is the entry with the largest share.
    Launch counts per frame: talker 28 layers; code predictor 5 layers x (the 2-token prefill + 14 decode steps), its
    layer-0 q/k/v of the decode steps comes from the sampler's table gather (bf16 mode)."""
    from qwen_tts import _hip
    eng = tts.model.engine
    t, c, dev = eng.talker, eng.cp, eng.dev
    bf = torch.bfloat16
    G = eng.G
    n_cp = G - 1  # CP forwards per frame: the 2-token prefill + 14 decode steps
    # with the step engine (qt_cp_step) the 14 decode steps are one launch each; the launch chain runs the prefill only
    engine = any(s.cp.ce_ws is not None for s in eng.all_sessions())
    # with the talker tail engine the o_proj / gate-up / down GEMVs are gone and q/k/v runs for layer 0 only
    tail = any(s.sc_t.get("tt_ws") is not None for s in eng.all_sessions())
    n_tg = 0 if tail else t.n_layers
    n_dec = 0 if engine else n_cp - 1  # decode-step forwards on the launch chain
    from qwen_tts.talker import CP_PREFILL
    n_pre = 0 if engine and CP_PREFILL else 1  # the 2-token prefill on the launch chain (else qt_cp_prefill)
    tab = [
        _gemv_entry("talker_gateup", "gemv_wt (talker MLP gate/up + SwiGLU, RMS folded)", n_tg,
                    [L.gu for L in t.layers], B, t.H, 2 * t.I, bf, bf, dev, rms=True, epi=_hip.EPI_SWIGLU),
        _gemv_entry("talker_down", "gemv_wt (talker MLP down + residual)", n_tg, [L.down for L in t.layers], B,
                    t.I, t.H, bf, torch.float32, dev, epi=_hip.EPI_ADD),
        _gemv_entry("talker_qkv", "gemv_wt (talker q/k/v, RMS folded)", 1 if tail else t.n_layers, [L.qkv for L in t.layers], B, t.H,
                    t.qkv_w, bf, torch.float32, dev, rms=True),
        _gemv_entry("talker_o", "gemv_wt (talker o_proj + residual)", n_tg, [L.o for L in t.layers], B,
                    t.Hq * t.D, t.H, bf, torch.float32, dev, epi=_hip.EPI_ADD),
        _gemv_entry("cp_gateup", "gemv_wt (code-predictor gate/up + SwiGLU)", c.n_layers * (n_pre + n_dec),
                    [L.gu for L in c.layers], B, c.H, 2 * c.I, bf, bf, dev, rms=True, epi=_hip.EPI_SWIGLU),
        _gemv_entry("cp_down", "gemv_wt (code-predictor down + residual)", c.n_layers * (n_pre + n_dec),
                    [L.down for L in c.layers],
                    B, c.I, c.H, bf, torch.float32, dev, epi=_hip.EPI_ADD),
        _gemv_entry("cp_qkv", "gemv_wt (code-predictor q/k/v, layers 1-4 of decode steps + prefill)",
                    (c.n_layers - 1) * n_dec + c.n_layers * n_pre, [L.qkv for L in c.layers], B, c.H, c.qkv_w, bf,
                    torch.float32, dev, rms=True),
        _gemv_entry("cp_lm_head", "gemv_wt (code-predictor lm_head, final norm folded)", n_pre + n_dec, eng.lm_heads, B, c.H,
                    eng.Vc, bf, torch.float32, dev, rms=True),
        attn_oproj_entry(tts, B, n_frame=c.n_layers * (n_pre + n_dec)),
    ]
    if engine:
        tab.append(cp_step_entry(tts, B))
        if not n_pre:
            tab.append(cp_prefill_entry(tts, B))
    if tail:
        tab.append(talker_tail_entry(tts, B))
    ra = attention_roofline(tts, B, L_mean)
    tab.append(dict(name="talker_attention", kernel=f"attn_decode_k (talker decode attention, {L_mean} keys)",
                    bound="hbm", launches_per_frame=t.n_layers, avg_us=ra["avg_us"], bytes=ra["bytes"]))
    for e in tab:
        e["gbs"] = e["bytes"] / (e["avg_us"] * 1e-6) / 1e9
        e["frac"] = e["gbs"] / HBM_PEAK_GBS
        e["us_per_frame"] = e["avg_us"] * e["launches_per_frame"]
    return tab


def _pmc_traffic(tag):
    """HBM traffic per launch of a kernel from the committed rocprofv3 PMC profile (profiles/*_pmc_<tag>.json) whose
    build id (content digest of the kernel sources) matches this library's; else the newest, labelled as such.
    Counters cannot be read inside this process."""
    from qwen_tts import _hip
    pdir = os.path.join(REPO, "profiles")
    pmcs = [f for f in sorted(os.listdir(pdir), reverse=True) if f.endswith(f"_pmc_{tag}.json")]
    for f in pmcs:
        j = json.load(open(os.path.join(pdir, f)))
        if j.get("build_id") == _hip.BUILD_ID:
            return j.get("hbm_bytes_per_launch"), f"profiles/{f} (this build, {j['build_id']})", \
                j.get("l2_to_cu_read_bytes_64B_req")
    if pmcs:
        j = json.load(open(os.path.join(pdir, pmcs[0])))
        return j.get("hbm_bytes_per_launch"), (f"profiles/{pmcs[0]} (earlier build {j.get('build_id')}, not this "
                                               f"library's {_hip.BUILD_ID})"), j.get("l2_to_cu_read_bytes_64B_req")
    return None, None, None


PMC_TAG = {"talker_gateup": "gateup", "cp_attn_oproj": "attn_oproj", "cp_step": "cp_step", "talker_tail": "talker_tail"}


def _rocprof_avg(tag):
    """Average kernel duration (us, begin -> end) of a kernel in the rocprofv3 --kernel-trace --stats run of this bench
    command committed for this library's build (profiles/*_rocprof_<tag>.json, reduced from the stats CSV by
    tools/rocprof_kernel_avg.py).  The bench's own per-launch time is a graph replay of dependent launches divided by
    the launches, so it also holds the dispatch gap between them; the two are reported side by side."""
    from qwen_tts import _hip
    pdir = os.path.join(REPO, "profiles")
    for f in sorted(os.listdir(pdir), reverse=True):
        if f.endswith(f"_rocprof_{tag}.json"):
            j = json.load(open(os.path.join(pdir, f)))
            if j.get("build_id") == _hip.BUILD_ID:
                return j.get("avg_us"), f"profiles/{f} (this build, {j['build_id']}, {j.get('calls')} launches)"
    return None, None


def whole_frame_roofline(tts, cfg, B, reps=32):
    """The captured per-frame graph (15 code-predictor steps + the talker step + token choices) of the bench's own
    session replayed `reps` times at its final cache length: algorithmic bytes per frame / time per frame."""
    eng = tts.model.engine
    ss = [s for s in eng.all_sessions() if s.B == B and s.graph is not None and s.force is None]
    if not ss:
        return None
    s = max(ss, key=lambda x: int(x.meta["kv_pos"].max().item()))
    L = int(s.meta["kv_pos"].max().item()) + 1
    st = torch.cuda.Stream(device=eng.dev)
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        s.graph.replay()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(reps):
            s.graph.replay()
        e1.record(st)
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / reps
    byt = frame_bytes(cfg, B, L)
    return dict(avg_us=us, bytes=byt, gbs=byt / (us * 1e-6) / 1e9, keys=L)


def prefill_mfma(tts, M=680, reps=3):
    """Prefill linears on gemm_pf_k at M rows (M = 680: four ~170-token voice-clone prompts, configs[4]): per replay
    the 28 talker layers' q/k/v (RMS), o_proj (+ residual, bf16 shadow), gate/up (RMS, SwiGLU) and down (+ residual)
    GEMMs on their distinct weights, as _Stack.forward issues them for a prefill.  flops = 2 M sum(N K)."""
    from qwen_tts import _hip, kernels as Kn
    eng = tts.model.engine
    t, dev = eng.talker, eng.dev
    x = torch.randn(M, t.H, device=dev)
    x16 = x.to(torch.bfloat16)
    qkv = torch.empty(M, t.qkv_w, device=dev)
    att = torch.randn(M, t.Hq * t.D, device=dev).to(eng.wdt)
    h = torch.empty(M, t.I, dtype=eng.wdt, device=dev)

    def run():
        for L in t.layers:
            Kn.gemm(x16, L.qkv, qkv, M, t.H, t.qkv_w, rms=True, eps=t.eps)
            Kn.gemm(att, L.o, x, M, t.Hq * t.D, t.H, epi=_hip.EPI_ADD, out2=x16)
            Kn.gemm(x16, L.gu, h, M, t.H, t.I, rms=True, eps=t.eps, epi=_hip.EPI_SWIGLU)
            Kn.gemm(h, L.down, x, M, t.I, t.H, epi=_hip.EPI_ADD, out2=x16)
    us = _graph_us(run, dev, reps)
    nk = t.H * t.qkv_w + t.Hq * t.D * t.H + t.H * 2 * t.I + t.I * t.H
    flops = 2.0 * M * nk * len(t.layers)
    return dict(us_per_layer=us / len(t.layers), tflops=flops / (us * 1e-6) / 1e12, M=M)


def attention_roofline(tts, B, L, reps=10):
    """North-star secondary roofline: the talker decode attention (q/k norm + RoPE + KV append + GQA attention,
    attn_decode_k) at cache length L, 28 launches over distinct per-layer caches (as in a frame) in a HIP graph.
    Algorithmic bytes per launch = the K and V rows read: B x Hkv x L x D x 2 x sizeof(bf16)."""
    from qwen_tts import kernels as Kn
    eng = tts.model.engine
    t = eng.talker
    dev = eng.dev
    nl = len(t.layers)
    kc = [torch.randn(B, t.Hkv, L + 1, t.D, device=dev).to(eng.kv_dtype) for _ in range(nl)]
    vc = [torch.randn(B, t.Hkv, L + 1, t.D, device=dev).to(eng.kv_dtype) for _ in range(nl)]
    qkv = torch.randn(B, (t.Hq + 2 * t.Hkv) * t.D, device=dev)
    att = torch.empty(B, t.Hq * t.D, dtype=eng.wdt, device=dev)
    pos = torch.full((B,), L - 1, dtype=torch.int32, device=dev)
    rb = torch.arange(B, dtype=torch.int32, device=dev)
    zero = torch.zeros(B, dtype=torch.int32, device=dev)
    t.ensure_rope(L + 4, dev)
    L0 = t.layers[0]

    def run():
        for i in range(nl):
            Kn.decode_attention(qkv, B, t.Hq, t.Hkv, t.D, L0.q_norm, L0.k_norm, t.eps, t.cos, t.sin, pos, rb, pos,
                                zero, kc[i], vc[i], L + 1, att)
    st = torch.cuda.Stream(device=dev)
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        run()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            run()
        g.replay()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(reps):
            g.replay()
        e1.record(st)
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / (reps * nl)
    byt = B * t.Hkv * L * t.D * 2 * kc[0].element_size()
    return dict(avg_us=us, bytes=byt, gbs=byt / (us * 1e-6) / 1e9, keys=L)


def eng_wdt_bf16(tts):
    return tts.model.engine.wdt == torch.bfloat16


def cpu_baseline(B, prompt, frames, threads, preset="1.7b-customvoice"):
    """Oracle (CPU fp32 restatement of the reference) on a bounded sample of the same workload, with the GPU run's own
    seeded weights (qwen_tts.weights.synthetic on the CPU; the oracle's two extra codec input projections, which the
    HIP path folds away, are seeded separately).  Cross-checked against the reference itself on this workload by
    tests/golden/cpu_baseline_xval.py (profiles/*_cpu_baseline_xval.json, attached as `xval`)."""
    from oracle import CodecOracle, TalkerOracle, build_prompts, codec_param_specs, generate, load_preset
    from oracle.talker import talker_param_specs
    from qwen_tts.weights import synthetic
    torch.set_num_threads(threads)
    cfg, ccfg = load_preset(preset)
    cpu = torch.device("cpu")
    W = synthetic(talker_param_specs(cfg), cpu)
    cspecs = codec_param_specs(ccfg)
    CW = synthetic([(n, s) for n, s in cspecs if not n.endswith("input_proj.weight")], cpu)
    g = torch.Generator().manual_seed(0)
    CW.update({n: 0.02 * torch.randn(s, generator=g) for n, s in cspecs if n not in CW})
    o, co = TalkerOracle(cfg, W), CodecOracle(ccfg, CW)
    ids = [synth_ids(prompt, i) for i in range(B)]
    spk = ["vivian", "ryan", "serena", "aiden", "eric", "dylan", "sohee", "ono_anna"][:B]
    t0 = time.time()
    with torch.no_grad():
        emb, mask, trail, pad = build_prompts(o, ids, ["english"] * B, (spk * 8)[:B], None, False)
        res = generate(o, emb, mask, trail, pad, max_new_tokens=frames + 1, do_sample=True, ignore_eos=True)
        codes = torch.stack(res.codes)
        wav = co.decode(codes)
    dt = time.time() - t0
    audio = sum(w.shape[0] for w in wav) / 24000.0
    xval = None
    pdir = os.path.join(REPO, "profiles")
    xs = sorted(f for f in os.listdir(pdir) if f.endswith("_cpu_baseline_xval.json"))
    if xs:
        j = json.load(open(os.path.join(pdir, xs[-1])))
        xval = {"oracle_over_reference": round(j["oracle_over_reference"], 4), "threads": j["threads"],
                "within_10pct": j["within_10pct"], "source": f"profiles/{xs[-1]} (container host, same workload shape)"}
    return dict(value=audio / dt, unit="audio-seconds/sec", cores=threads, threads=threads,
                host_cpu_count=os.cpu_count(), kind="port", xval=xval,
                sample=f"oracle fp32, 1.7B dims, the GPU run's seeded weights, B={B} x {prompt}-token prompts, {frames} "
                       f"sampled frames + codec, {dt:.1f}s, torch.set_num_threads({threads})")


def _free_port() -> int:
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def self_launch(gpus: int) -> int:
    """`bench.py --gpus N` (N > 1) run without a torch.distributed launcher around it: start the N ranks ourselves, one
    process per GPU, as `python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1 bench.py ...` in a
    CHILD process, and return its exit code.  This process never touches the GPU (no HIP call before or after: a
    process that has initialised the GPU must not be replaced by another), and the ranks print the one JSON line."""
    import subprocess
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={gpus}",
           "--master-addr", "127.0.0.1", f"--master-port={_free_port()}", os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, QT_BENCH_LAUNCHER="self")
    return subprocess.call(cmd, env=env)


def init_ranks(a):
    """Rank environment of this process: (world, rank, local, backend, dist module or None, device).  Under a launcher
    the world size must equal --gpus (the driver's 1 -> 8 scaling run passes both; a mismatch would report one GPU's
    work as N GPUs').  QT_BENCH_BACKEND=gloo + QT_BENCH_SAME_DEVICE=1 rehearse the N > 1 path on one GPU;
    QT_BENCH_DRYRUN=1 (CPU tests of this launcher) runs no model and no GPU at all."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != a.gpus:
        raise SystemExit(f"bench.py: --gpus {a.gpus} but WORLD_SIZE={world} ranks were launched")
    backend = os.environ.get("QT_BENCH_BACKEND", "nccl")  # nccl == RCCL over xGMI on ROCm
    dry = os.environ.get("QT_BENCH_DRYRUN") == "1"
    if dry:
        backend = "gloo"
        dev = torch.device("cpu")
    else:
        if os.environ.get("QT_BENCH_SAME_DEVICE") == "1":
            local = 0
        torch.cuda.set_device(local)
        dev = torch.device(f"cuda:{local}")
    dist = None
    if world > 1:
        import torch.distributed as dist
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)
        assert dist.get_world_size() == a.gpus, (dist.get_world_size(), a.gpus)
    return world, rank, local, backend, dist, dev


def gather_rank_rates(dist, audio, dt):
    """Per-rank audio-seconds/sec (rank order) -- reported beside the whole-job value."""
    if dist is None:
        return [audio / dt]
    objs = [None] * dist.get_world_size()
    dist.all_gather_object(objs, (audio, dt))
    return [a_ / d_ for a_, d_ in objs]


def main_dryrun(a, world, rank, dist, dev, backend):
    """CPU rehearsal of the launcher, barriers and reductions (QT_BENCH_DRYRUN=1): every step "generates" B x frames
    of audio in a fixed sleep.  Same JSON keys as the real line; never used for a reported number."""
    B = a.batch
    audio_per_step = B * a.frames * 1920 / 24000.0

    def barrier():
        if dist is not None:
            dist.barrier()
    for _ in range(a.warmup):
        time.sleep(0.01)
    barrier()
    t0 = time.perf_counter()
    audio = 0.0
    for _ in range(a.steps):
        time.sleep(0.02)
        audio += audio_per_step
    barrier()
    dt = time.perf_counter() - t0
    per_rank = gather_rank_rates(dist, audio, dt)
    if dist is not None:
        from qwen_tts.dp import reduce_timing
        dt, audio = reduce_timing(dt, audio, device=dev)
    if rank == 0:
        print(json.dumps({"metric": "dryrun", "value": round(audio / dt, 3), "unit": "audio-seconds/sec",
                          "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "dist_backend": backend if world > 1
                          else None, "rccl_ranks": world if backend == "nccl" and world > 1 else 0,
                          "per_rank_value": [round(v, 3) for v in per_rank], "audio_seconds": audio,
                          "launcher": os.environ.get("QT_BENCH_LAUNCHER", "external" if world > 1 else None)}),
              flush=True)
    if dist is not None:
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--prompt-tokens", type=int, default=200)
    ap.add_argument("--preset", default="1.7b-customvoice")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--cpu-baseline", type=int, default=1)
    ap.add_argument("--cpu-frames", type=int, default=24)
    ap.add_argument("--cpu-threads", type=int, default=8)
    ap.add_argument("--roofline", type=int, default=1)
    ap.add_argument("--workload", default="cv8", choices=["cv8", "vd64"],
                    help="cv8: configs[2] (default, weak scaling: 8 x 200-token CustomVoice utterances per GPU); vd64: "
                         "configs[3] (strong scaling: 64 mixed-length VoiceDesign requests LPT-sharded over the ranks)")
    ap.add_argument("--slots", type=int, default=64, help="vd64: continuously refilled batch rows per GPU")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also measure batch 1, first-packet latencies, the kernel table and "
                         "rooflines (--roofline) and the CPU baseline (--cpu-baseline); a plain run prints the headline "
                         "figures only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's codes and PCM of every utterance to DIR/<name>.npy (float32)")
    a = ap.parse_args()
    if a.dump_outputs and a.workload != "cv8":
        ap.error("--dump-outputs is implemented for the default workload (cv8)")
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(a.gpus))  # before any GPU call: the N ranks run in child processes
    world, rank, local, backend, dist, dev = init_ranks(a)
    if os.environ.get("QT_BENCH_DRYRUN") == "1":
        return main_dryrun(a, world, rank, dist, dev, backend)
    if a.workload == "vd64":
        return main_vd64(a, world, rank, dist, dev, backend)

    from qwen_tts import Qwen3TTSModel
    cfg, W, CW = make_weights(a.preset, dev, world, rank)
    tts = Qwen3TTSModel.from_pretrained(f"synthetic:{a.preset}", device_map=str(dev),
                                        dtype=torch.bfloat16 if a.dtype == "bf16" else torch.float32,
                                        weights=W, codec_weights=CW)
    del W, CW
    torch.cuda.empty_cache()
    B = a.batch
    ids = [synth_ids(a.prompt_tokens, rank * 1000 + i) for i in range(B)]
    spk = (["vivian", "ryan", "serena", "aiden", "eric", "dylan", "sohee", "ono_anna"] * 8)[:B]
    langs = ["english"] * B
    gen = dict(max_new_tokens=a.frames + 1, do_sample=True, top_k=50, top_p=1.0, temperature=0.9,
               subtalker_dosample=True, subtalker_top_k=50, subtalker_top_p=1.0, subtalker_temperature=0.9,
               repetition_penalty=1.05, ignore_eos=True)

    def step(seed, n=B):
        t0 = time.perf_counter()
        codes, _ = tts.model.generate(input_ids=ids[:n], languages=langs[:n], speakers=spk[:n], non_streaming_mode=False,
                                      seed=seed, **gen)
        wavs, sr = tts.model.speech_tokenizer.decode([{"audio_codes": c} for c in codes])
        last["codes"], last["wavs"] = codes, wavs  # what the caller receives (kept for --dump-outputs)
        return sum(w.shape[0] for w in wavs) / sr, time.perf_counter() - t0

    last = {}

    for i in range(a.warmup):
        step(100 + i)

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    barrier()
    t0 = time.perf_counter()
    audio, lat = 0.0, []
    for i in range(a.steps):
        s_audio, s_t = step(i)
        audio += s_audio
        lat.append(s_t)
    barrier()
    dt = time.perf_counter() - t0
    per_rank = gather_rank_rates(dist, audio, dt)
    if dist is not None:
        from qwen_tts.dp import reduce_timing
        dt, audio = reduce_timing(dt, audio, device=dev)
    value = audio / dt
    if a.dump_outputs and a.steps > 0:
        dump_outputs(a.dump_outputs, last["codes"], last["wavs"], world, rank)
    if rank == 0:
        per_utt_rtf = value / (B * world)
        from qwen_tts import _hip
        out = {"metric": "audio-seconds/sec (RTF) + p50 first-packet latency, 1.7B @ batch 1/8, 1->8 GPU",
               "value": round(value, 3), "unit": "audio-seconds/sec", "n_gpus": world, "steps": a.steps,
               "warmup": a.warmup, "ms_per_step": round(1e3 * dt / a.steps, 2), "higher_is_better": True,
               "scaling": "weak", "vs_baseline": None, "dtype": a.dtype, "data": "synthetic (seeded weights + token ids)",
               "config": {"workload": f"Qwen3-TTS-12Hz-{a.preset} B={B}/GPU x {a.prompt_tokens}-token prompts, "
                                      f"streaming text, {a.frames} frames + codec decode",
                          "global_batch": B * world, "seq_len": a.prompt_tokens, "frames": a.frames,
                          "parallelism": f"dp{world}"},
               "rtf_per_utterance": round(per_utt_rtf, 2),
               "full_batch_latency_p50_ms": round(1e3 * float(np.median(lat)), 1), "full": a.full,
               "build_id": _hip.BUILD_ID, "dist_backend": backend if world > 1 else None,
               "rccl_ranks": world if backend == "nccl" and world > 1 else 0,
               "per_rank_value": [round(v, 3) for v in per_rank],
               "launcher": os.environ.get("QT_BENCH_LAUNCHER", "external" if world > 1 else None)}
    if a.full:
        extra = full_figures(a, tts, cfg, step, ids, spk, langs, gen, B, world, rank)
        if rank == 0:
            out.update(extra)
    if rank == 0:
        print(json.dumps(out), flush=True)
    if dist is not None:
        dist.destroy_process_group()


def dump_outputs(d, codes, wavs, world, rank):
    """--dump-outputs: the codes and PCM the last timed step returned, one float32 .npy per utterance (codec codes are
    small integers, exact in float32); B = 8 x 256 frames is ~16 MB."""
    os.makedirs(d, exist_ok=True)
    pre = f"r{rank}_" if world > 1 else ""
    for i, (c, w) in enumerate(zip(codes, wavs)):
        np.save(os.path.join(d, f"{pre}codes_{i}.npy"), torch.as_tensor(c).cpu().numpy().astype(np.float32))
        np.save(os.path.join(d, f"{pre}pcm_{i}.npy"), np.asarray(w, dtype=np.float32))


def full_figures(a, tts, cfg, step, ids, spk, langs, gen, B, world, rank):
    """--full: everything the result line holds beyond the headline figures, measured after the timed steps in runs of
    their own (every rank takes the first-packet samples, as its own batch's; rank 0 does the rest).  Returns the extra
    keys of the JSON line."""
    # talker cache length at the end of a timed step (prompt + frames), before other shapes reuse the sessions
    L_end = max(int(ss.meta["kv_pos"].max().item()) for ss in tts.model.engine.all_sessions() if ss.B == B)
    fr = whole_frame_roofline(tts, cfg, B) if a.roofline and rank == 0 else None
    # batch 1 (the metric's "1.7B @ batch 1"): one utterance of the same shape per GPU, 1 warm-up + `steps` timed
    b1 = None
    if rank == 0 and B > 1:
        step(200, 1)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        au1 = sum(step(300 + i, 1)[0] for i in range(a.steps))
        torch.cuda.synchronize()
        d1 = time.perf_counter() - t1
        b1 = {"value": round(au1 / d1, 3), "unit": "audio-seconds/sec", "rtf": round(au1 / d1, 2),
              "ms_per_step": round(1e3 * d1 / a.steps, 2),
              "workload": f"1 utterance x {a.prompt_tokens}-token prompt, {a.frames} frames + codec, 1 GPU"}
    # first packet (SURVEY §8 metric): request submit -> first PCM chunk delivered by stream(), on this rank's batch
    # of B and on a single utterance
    def first_packet(n):
        t0 = time.perf_counter()
        for _ in tts.model.stream(input_ids=ids[:n], languages=langs[:n], speakers=spk[:n], non_streaming_mode=False,
                                  seed=7, **gen):
            break
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    fp = {}
    for n in (B, 1):
        # two warm-ups (the second call of a prompt length captures its prefill / codec-feed graphs), then the median
        # of 9 (3 samples moved the p50 by up to 0.6 ms between boxes)
        first_packet(n)
        first_packet(n)
        fp[n] = 1e3 * float(np.median([first_packet(n) for _ in range(9)]))
    roof = table = frame_roof = pf_roof = gateup = None
    if a.roofline and rank == 0 and eng_wdt_bf16(tts):
        # decode attention at the run's mean cache length (prompt + half the frames)
        L_mean = max(L_end - a.frames // 2, 1)
        tab = decode_kernel_table(tts, B, L_mean)
        frame_us = fr["avg_us"] if fr is not None else None

        def as_roof(e):
            tag = e.get("pmc_tag", PMC_TAG.get(e["name"]))
            traffic, tsrc, l2cu = _pmc_traffic(tag) if tag else (None, None, None)
            rp_us, rp_src = _rocprof_avg(tag) if tag else (None, None)
            ach_rp = None if not rp_us else e["bytes"] / (rp_us * 1e-6) / 1e9
            r = {"bound": e["bound"], "kernel": e["kernel"], "achieved": round(e["gbs"], 1), "peak": HBM_PEAK_GBS,
                 "unit": "GB/s", "frac": round(e["frac"], 4), "traffic": traffic, "traffic_source": tsrc,
                 "traffic_over_bytes": None if not traffic else round(traffic / e["bytes"], 3),
                 "l2_to_cu_over_bytes": None if not l2cu else round(l2cu / e["bytes"], 3),
                 "avg_launch_us": round(e["avg_us"], 2), "bytes_per_launch": int(e["bytes"]),
                 "launches_per_frame": e["launches_per_frame"], "us_per_frame": round(e["us_per_frame"], 1),
                 "frame_share": None if frame_us is None else round(e["us_per_frame"] / frame_us, 4),
                 "rocprof_avg_us": rp_us, "rocprof_source": rp_src,
                 "achieved_at_rocprof_avg": None if ach_rp is None else round(ach_rp, 1),
                 "frac_at_rocprof_avg": None if ach_rp is None else round(ach_rp / HBM_PEAK_GBS, 4),
                 "timing_note": "avg_launch_us: a graph of the frame's launches replayed between HIP events on their "
                                "stream, divided by the launches (each dependent launch's dispatch gap included); "
                                "rocprof_avg_us: the kernel's own begin -> end in rocprofv3 --kernel-trace"}
            if e.get("ic_resident"):  # second bound: the weights are re-read from the Infinity Cache within a frame
                r["second_bound"] = {"bound": "infinity_cache", "achieved": round(e["gbs"], 1), "peak": IC_RATE_GBS,
                                     "unit": "GB/s", "frac": round(e["gbs"] / IC_RATE_GBS, 4),
                                     "frac_at_rocprof_avg": None if ach_rp is None else round(ach_rp / IC_RATE_GBS, 4),
                                     "peak_source": "MI355X_MICROARCH.md: measured chip-wide read rate from a 38 MB "
                                                    "table in the Infinity Cache (no spec figure)"}
            return r
        # the dominant decode kernel = the largest measured time per frame (launch time x launches per frame)
        dom = max(tab, key=lambda e: e["us_per_frame"])
        roof = dict(as_roof(dom), selected_by="largest measured time per frame among the decode kernels (kernel_table)")
        gateup = as_roof(next(e for e in tab if e["name"] == "talker_gateup"))
        table = {e["name"]: {"avg_launch_us": round(e["avg_us"], 2), "launches_per_frame": e["launches_per_frame"],
                             "us_per_frame": round(e["us_per_frame"], 1), "bytes_per_launch": int(e["bytes"]),
                             "frac": round(e["frac"], 4)} for e in tab}
        if fr is not None:
            frame_roof = {"bound": "hbm", "what": f"whole AR frame (15 CP steps + talker step), B={B}, "
                                                  f"{fr['keys']} talker keys, captured frame graph replayed",
                          "achieved": round(fr["gbs"], 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                          "frac": round(fr["gbs"] / HBM_PEAK_GBS, 4), "us_per_frame": round(fr["avg_us"], 1),
                          "bytes_per_frame": int(fr["bytes"]),
                          "kernel_table_us": round(sum(e["us_per_frame"] for e in tab), 1)}
        pf = prefill_mfma(tts)
        pf_roof = {"bound": "mfma", "kernel": f"gemm_pf2_k (talker prefill linears, M={pf['M']} rows, 28 layers)",
                   "achieved": round(pf["tflops"], 1), "peak": MFMA_BF16_PEAK_TFS, "unit": "TFLOP/s",
                   "frac": round(pf["tflops"] / MFMA_BF16_PEAK_TFS, 4), "us_per_layer": round(pf["us_per_layer"], 1)}
    cpu = None
    if a.cpu_baseline and rank == 0 and world == 1:
        # 8 threads: the reference's own published CPU figure and the cross-check use 8 (the box's CPU
        # share is 16, os.cpu_count() reports the whole host)
        cpu = cpu_baseline(B, a.prompt_tokens, a.cpu_frames, a.cpu_threads, a.preset)
    return {"batch1": b1, "first_packet_p50_ms": round(fp[B], 1), "first_packet_p50_ms_b1": round(fp[1], 1),
            "roofline": roof, "frame_roofline": frame_roof, "kernel_table": table, "gateup_roofline": gateup,
            "prefill_mfma": pf_roof, "cpu_baseline": cpu}


def vd64_requests(n=64, seed=4321):
    """configs[3]: 64 VoiceDesign requests, text ~ U[40, 300] tokens, instruct ~ U[10, 60] tokens,
    F ~ U[64, 320] frames, the same list on every rank."""
    g = np.random.default_rng(seed)
    texts = g.integers(40, 301, n)
    ins = g.integers(10, 61, n)
    frames = g.integers(64, 321, n)
    ids = [synth_ids(int(t), 5000 + i) for i, t in enumerate(texts)]
    ins_ids = []
    for i, k in enumerate(ins):
        gi = np.random.default_rng([seed, i, 11])
        ins_ids.append(torch.tensor([[151644, 872, 198] + gi.integers(1000, 150000, int(k)).tolist() + [151645, 198]],
                                    dtype=torch.long))
    langs = (["english", "chinese", "japanese", "korean"] * (n // 4 + 1))[:n]
    return ids, ins_ids, langs, [int(f) for f in frames]


def main_vd64(a, world, rank, dist, dev, backend):
    """configs[3]: one step = all 64 requests generated (sampling, exact frame counts) and decoded to PCM.  Each rank
    decodes its longest-first share (qwen_tts.dp.dp_generate: continuous batching through --slots rows, its own PCM);
    value = total audio seconds of the 64 / max-over-ranks wall time (strong scaling)."""
    from qwen_tts import Qwen3TTSModel, _hip
    from qwen_tts.dp import dp_generate
    preset = "1.7b-voicedesign"
    cfg, W, CW = make_weights(preset, dev, world, rank)
    tts = Qwen3TTSModel.from_pretrained(f"synthetic:{preset}", device_map=str(dev),
                                        dtype=torch.bfloat16 if a.dtype == "bf16" else torch.float32,
                                        weights=W, codec_weights=CW)
    del W, CW
    torch.cuda.empty_cache()
    ids, ins_ids, langs, frames = vd64_requests()
    gen = dict(max_new_tokens=max(frames) + 1, do_sample=True, top_k=50, top_p=1.0, temperature=0.9,
               subtalker_dosample=True, subtalker_top_k=50, subtalker_top_p=1.0, subtalker_temperature=0.9,
               repetition_penalty=1.05, ignore_eos=True, non_streaming_mode=True)

    def step(seed):
        t0 = time.perf_counter()
        mine = dp_generate(tts.model, ids, langs, None, ins_ids, frames=frames, slots=a.slots, gather=False,
                           decode=True, seed=seed, **gen)
        torch.cuda.synchronize()
        audio = sum(w.shape[0] for _, w in mine.values()) / 24000.0
        return audio, time.perf_counter() - t0

    for i in range(a.warmup):
        step(100 + i)

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()
    barrier()
    t0 = time.perf_counter()
    audio = 0.0
    for i in range(a.steps):
        audio += step(i)[0]
    barrier()
    dt = time.perf_counter() - t0
    per_rank = gather_rank_rates(dist, audio, dt)
    if dist is not None:
        from qwen_tts.dp import reduce_timing
        dt, audio = reduce_timing(dt, audio, device=dev)
    if rank == 0:
        value = audio / dt
        out = {"metric": "audio-seconds/sec (RTF) + p50 first-packet latency, 1.7B @ batch 1/8, 1->8 GPU",
               "value": round(value, 3), "unit": "audio-seconds/sec", "n_gpus": world, "steps": a.steps,
               "warmup": a.warmup, "ms_per_step": round(1e3 * dt / a.steps, 2), "higher_is_better": True,
               "scaling": "strong", "vs_baseline": None, "dtype": a.dtype,
               "data": "synthetic (seeded weights + token ids)",
               "config": {"workload": "configs[3]: Qwen3-TTS-12Hz-1.7B VoiceDesign, 64 requests (text U[40,300], "
                                      "instruct U[10,60] tokens, F U[64,320] frames, sampling) LPT-sharded over the "
                                      f"ranks, {a.slots} refilled rows per GPU, + codec decode",
                          "global_batch": 64, "frames_total": int(sum(frames)), "parallelism": f"dp{world}"},
               "build_id": _hip.BUILD_ID, "dist_backend": backend if world > 1 else None,
               "rccl_ranks": world if backend == "nccl" and world > 1 else 0,
               "per_rank_value": [round(v, 3) for v in per_rank],
               "launcher": os.environ.get("QT_BENCH_LAUNCHER", "external" if world > 1 else None)}
        print(json.dumps(out), flush=True)
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
