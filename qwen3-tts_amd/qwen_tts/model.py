"""`Qwen3TTSForConditionalGeneration` equivalent on the MI355X engine (inner generate() contract).

Prompt assembly follows qwen_tts/core/models/modeling_qwen3_tts.py (M) :1968-2269 exactly; every
embedding / text-projection product runs through the HIP kernels (gather + fused MFMA GEMMs), the
sequence layout (cat / left-pad) is torch plumbing on device tensors.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch

from . import kernels as K
from .prefix import PrefixCache, PrefixPlan
from .resample import PcmResampler, output_format
from .prosody import steps as prosody_steps
from .tempo import PcmOutput
from .talker import MIN_NEW_TOKENS, GenParams, HandoffWatch, TalkerEngine
from .voice import VoiceCache, boundary_skip, check_codes, feed_span, joint_walk, plan_feed


class _Runs:
    """Runs of text ids / codec ids collected for one batched text_projection + one codec-embedding gather."""

    def __init__(self):
        self.ids = {"t": [], "c": []}
        self.out = {}

    def _add(self, kind, ids):
        ids = [int(x) for x in (ids.reshape(-1).tolist() if isinstance(ids, torch.Tensor) else ids)]
        s = len(self.ids[kind])
        self.ids[kind].extend(ids)
        return kind, s, len(ids)

    def text(self, ids):
        return self._add("t", ids)

    def codec(self, ids):
        return self._add("c", ids)

    def run(self, e):
        if self.ids["t"]:
            self.out["t"] = e.text_proj(self.ids["t"])
        if self.ids["c"]:
            self.out["c"] = e.codec_embed(self.ids["c"])

    def get(self, h):
        kind, s, n = h
        return self.out[kind][s:s + n][None]


class TTSModel:
    def __init__(self, config: dict, weights: Dict[str, torch.Tensor], dtype="bf16", device="cuda",
                 generate_config: Optional[dict] = None):
        self.config = config
        self.tc = config["talker_config"]
        self.engine = TalkerEngine(config, weights, dtype=dtype, device=device)
        self.device = self.engine.dev
        self.tts_model_type = config.get("tts_model_type")
        self.tts_model_size = config.get("tts_model_size")
        self.tokenizer_type = config.get("tokenizer_type")
        self.generate_config = generate_config or {}
        self.speech_tokenizer = None
        self.supported_speakers = list((self.tc.get("spk_id") or {}).keys())
        self.supported_languages = ["auto"] + [k for k in (self.tc.get("codec_language_id") or {}) if "dialect" not in k]
        self.speaker_encoder_sample_rate = config.get("speaker_encoder_config", {}).get("sample_rate", 24000)
        self.speaker_encoder = None
        if self.tts_model_type == "base" and "speaker_encoder.fc.weight" in weights:  # M:1821-1824
            from .speaker import SpeakerEncoder
            self.speaker_encoder = SpeakerEncoder(config, weights, dtype=dtype, device=self.device)

    @torch.inference_mode()
    def extract_speaker_embedding(self, audio, sr):
        """M:1940-1954: 24 kHz mono float32 waveform -> x-vector [enc_dim] (device, fp32)."""
        assert sr == 24000, "Only support 24kHz audio"
        if self.speaker_encoder is None:
            raise ValueError("no speaker encoder loaded (tts_model_type != 'base', or its weights are absent)")
        with torch.cuda.device(self.device):
            return self.speaker_encoder.embed(audio)

    @torch.inference_mode()
    def extract_speaker_embeddings(self, audios, sr):
        """extract_speaker_embedding of several clips at once (equal-length clips share one ECAPA pass):
        [n][enc_dim] (device, fp32)."""
        assert sr == 24000, "Only support 24kHz audio"
        if self.speaker_encoder is None:
            raise ValueError("no speaker encoder loaded (tts_model_type != 'base', or its weights are absent)")
        with torch.cuda.device(self.device):
            return self.speaker_encoder.embed_many(audios)

    def get_supported_speakers(self):
        return self.supported_speakers

    def get_supported_languages(self):
        return self.supported_languages

    def load_speech_tokenizer(self, tok):
        self.speech_tokenizer = tok

    # -------------------------------------------------------------------------------- G1 / G2
    def _icl_prompt(self, text_id, ref_id, ref_code, pad_e, eos_e, non_streaming_mode):
        """generate_icl_prompt (M:1968-2019)."""
        e, t = self.engine, self.tc
        text = torch.cat([e.text_proj(torch.cat([ref_id, text_id], -1))[None], eos_e], 1)
        ref_code = ref_code.to(self.device)
        parts = [e.codec_embed(ref_code[:, 0])]
        for i in range(1, t["num_code_groups"]):
            parts.append(e.cp_embed(i - 1, ref_code[:, i]))
        codec = torch.stack(parts, 1).sum(1)[None]
        codec = torch.cat([e.codec_embed([t["codec_bos_id"]])[None], codec], 1)
        tl, cl = text.shape[1], codec.shape[1]
        if non_streaming_mode:
            x = text + e.codec_embed([t["codec_pad_id"]] * tl)[None]
            return torch.cat([x, codec + pad_e], 1), pad_e
        if tl > cl:
            return text[:, :cl] + codec, text[:, cl:]
        text = torch.cat([text] + [pad_e] * (cl - tl), 1)
        return text + codec, pad_e

    def build_prompts(self, input_ids, languages, speakers=None, instruct_ids=None, non_streaming_mode=False,
                      voice_clone_prompt=None, ref_ids=None, open_text=False, lens_out=None):
        """(embeds [B,P,H] fp32, mask [B,P], trailing [B,T,H], tts_pad [1,1,H]) -- M:2068-2269.
        open_text (streaming-text input; not in the reference): the ids are a request's head -- the three
        role ids and the text known so far, no template suffix -- so every id after the fourth goes to the trailing
        rows and no end-of-text position follows them (the text is not complete; stream(text_feed=...) appends it).
        Two passes: the rows' text-id and codec-id runs are collected on the host first, then projected in one
        text_projection and one codec-embedding gather for the whole batch (one host->device copy each instead of
        a few per row: the per-row calls were host-bound, ~3.3 ms at B=8), and each row is assembled from slices.
        lens_out: a list that receives every row's prompt length (the prefix-cache path needs them on the host and
        would otherwise synchronise on the mask)."""
        e, t, cfg = self.engine, self.tc, self.config
        B = len(input_ids)
        if open_text and non_streaming_mode:
            raise ValueError("open_text prompts are streaming-text prompts: non_streaming_mode=True puts the whole "
                             "text into the prefill")
        runs = _Runs()
        spk_embeds = None
        if voice_clone_prompt is not None:
            spk_embeds = [torch.as_tensor(x).to(self.device).float() for x in voice_clone_prompt["ref_spk_embedding"]]
        h_ins = [None] * B
        if instruct_ids is not None:
            for i, ins in enumerate(instruct_ids):
                if ins is not None:
                    h_ins[i] = runs.text(ins)
        if speakers is None:
            speakers = [None] * B
        h_special = runs.text([cfg["tts_bos_token_id"], cfg["tts_eos_token_id"], cfg["tts_pad_token_id"]])
        plans = []
        for i, (ids, lang, spk) in enumerate(zip(input_ids, languages, speakers)):
            ids = torch.as_tensor(ids).reshape(-1).tolist()
            pl = {"ids": ids}
            spk_e = None
            if spk_embeds is None:
                if spk == "" or spk is None:
                    pass
                else:
                    if spk.lower() not in t["spk_id"]:
                        raise NotImplementedError(f"Speaker {spk} not implemented")
                    pl["spk_code"] = runs.codec([t["spk_id"][spk.lower()]])
            else:
                use = voice_clone_prompt["x_vector_only_mode"][i] or voice_clone_prompt["icl_mode"][i]
                spk_e = spk_embeds[i] if use else None
            pl["spk_vec"] = spk_e
            assert lang is not None
            if lang.lower() == "auto":
                lang_id = None
            else:
                if lang.lower() not in t["codec_language_id"]:
                    raise NotImplementedError(f"Language {lang} not implemented")
                lang_id = t["codec_language_id"][lang.lower()]
            if lang.lower() in ["chinese", "auto"] and spk != "" and spk is not None and \
                    t["spk_is_dialect"][spk.lower()] is not False:
                lang_id = t["codec_language_id"][t["spk_is_dialect"][spk.lower()]]
            if lang_id is None:
                pre = [t["codec_nothink_id"], t["codec_think_bos_id"], t["codec_think_eos_id"]]
            else:
                pre = [t["codec_think_id"], t["codec_think_bos_id"], lang_id, t["codec_think_eos_id"]]
            pl["c0"] = runs.codec(pre)
            pl["c1"] = runs.codec([t["codec_pad_id"], t["codec_bos_id"]])
            pl["role"] = runs.text(ids[:3])
            pl["icl"] = (voice_clone_prompt is not None and voice_clone_prompt["ref_code"] is not None
                         and voice_clone_prompt["icl_mode"][i])
            if not pl["icl"]:
                pl["first"] = runs.text(ids[3:4])
                if non_streaming_mode:
                    n = len(ids[3:-5])
                    pl["txt"] = runs.text(ids[3:-5])
                    pl["txt_pad"] = runs.codec([t["codec_pad_id"]] * (n + 1))
                    pl["end_bos"] = runs.codec([t["codec_bos_id"]])
                else:
                    pl["trail"] = runs.text(ids[4:] if open_text else ids[4:-5])
            plans.append(pl)
        runs.run(e)
        if not any(pl["icl"] for pl in plans):
            return self._assemble_indexed(runs, plans, h_ins, h_special, non_streaming_mode, open_text, lens_out)
        special = runs.get(h_special)[0]
        bos_e, eos_e, pad_e = special[0].view(1, 1, -1), special[1].view(1, 1, -1), special[2].view(1, 1, -1)
        per: List[list] = [[] if h_ins[i] is None else [runs.get(h_ins[i])] for i in range(B)]
        trailing = []
        for i, pl in enumerate(plans):
            c0, c1 = runs.get(pl["c0"]), runs.get(pl["c1"])
            spk_e = runs.get(pl["spk_code"]) if "spk_code" in pl else pl["spk_vec"]
            codec_in = torch.cat([c0, c1], 1) if spk_e is None else torch.cat([c0, spk_e.view(1, 1, -1), c1], 1)
            role = runs.get(pl["role"])
            body = torch.cat([pad_e.expand(-1, codec_in.shape[1] - 2, -1), bos_e], 1) + codec_in[:, :-1]
            emb = torch.cat([role, body], 1)
            if pl["icl"]:
                ids = torch.as_tensor(pl["ids"]).reshape(1, -1)
                ref = torch.as_tensor(ref_ids[i]).reshape(1, -1)
                icl_e, trail = self._icl_prompt(ids[:, 3:-5], ref[:, 3:-2],
                                                torch.as_tensor(voice_clone_prompt["ref_code"][i]), pad_e, eos_e,
                                                non_streaming_mode)
                emb = torch.cat([emb, icl_e], 1)
            else:
                emb = torch.cat([emb, runs.get(pl["first"]) + codec_in[:, -1:]], 1)
                if non_streaming_mode:
                    emb = emb[:, :-1]
                    txt = torch.cat([runs.get(pl["txt"]), eos_e], 1) + runs.get(pl["txt_pad"])
                    emb = torch.cat([emb, txt, pad_e + runs.get(pl["end_bos"])], 1)
                    trail = pad_e
                else:
                    trail = torch.cat([runs.get(pl["trail"]), pad_e if open_text else eos_e], 1)
            per[i].append(emb)
            trailing.append(trail)
        seqs = [torch.cat(p, 1)[0] for p in per]
        if lens_out is not None:
            lens_out[:] = [int(s.shape[0]) for s in seqs]
        P = max(s.shape[0] for s in seqs)
        H = seqs[0].shape[1]
        embeds = torch.zeros(B, P, H, device=self.device)
        mask = torch.zeros(B, P, dtype=torch.long, device=self.device)
        for i, s in enumerate(seqs):
            embeds[i, P - s.shape[0]:] = s
            mask[i, P - s.shape[0]:] = 1
        T = max(tr.shape[1] for tr in trailing)
        trail = pad_e.reshape(1, 1, H).expand(B, T, H).clone()
        for i, tr in enumerate(trailing):
            trail[i, :tr.shape[1]] = tr[0]
        return embeds, mask, trail, pad_e

    def _assemble_indexed(self, runs, plans, h_ins, h_special, non_streaming_mode, open_text=False, lens_out=None):
        """build_prompts' assembly for non-ICL rows as one gather: every prompt / trailing position is the sum of at
        most two rows of [text projections; codec embeddings; x-vectors; zero row], so the host writes a [positions,
        2] index table and three GPU ops build the whole batch (the per-row slicing / cat / add chain was ~120
        host-bound launches at B = 8).  Same two fp32 operands per position as that chain, so the same bits."""
        B = len(plans)
        out_t, out_c = runs.out.get("t"), runs.out.get("c")
        NT = 0 if out_t is None else out_t.shape[0]
        NC = 0 if out_c is None else out_c.shape[0]
        vecs = [pl["spk_vec"] for pl in plans if pl["spk_vec"] is not None]
        Z = NT + NC + len(vecs)  # the zero row

        def t(h, j=0):
            return h[1] + j

        def c(h, j=0):
            return NT + h[1] + j
        sp = h_special
        bos, eos, pad = t(sp, 0), t(sp, 1), t(sp, 2)
        seqs, trails, v = [], [], 0
        for i, pl in enumerate(plans):
            pos = [] if h_ins[i] is None else [(t(h_ins[i], j), Z) for j in range(h_ins[i][2])]
            pos += [(t(pl["role"], j), Z) for j in range(3)]
            ci = [c(pl["c0"], j) for j in range(pl["c0"][2])]
            if "spk_code" in pl:
                ci.append(c(pl["spk_code"]))
            elif pl["spk_vec"] is not None:
                ci.append(NT + NC + v)
                v += 1
            ci += [c(pl["c1"], j) for j in range(2)]
            pos += [(pad if k < len(ci) - 2 else bos, ci[k]) for k in range(len(ci) - 1)]
            if non_streaming_mode:
                n = pl["txt"][2]
                pos += [(t(pl["txt"], j) if j < n else eos, c(pl["txt_pad"], j)) for j in range(n + 1)]
                pos.append((pad, c(pl["end_bos"])))
                trails.append([(pad, Z)])
            else:
                if pl["first"][2]:  # (a prompt without a first text token has no such position, as in the chain)
                    pos.append((t(pl["first"]), ci[-1]))
                # (open text: no end-of-text position yet; a pad one keeps the row non-empty)
                trails.append([(t(pl["trail"], j), Z) for j in range(pl["trail"][2])] +
                              [(pad if open_text else eos, Z)])
            seqs.append(pos)
        if lens_out is not None:
            lens_out[:] = [len(s) for s in seqs]
        P, T = max(len(s) for s in seqs), max(len(tr) for tr in trails)
        idx = [[(Z, Z)] * (P - len(s)) + s for s in seqs] + [tr + [(pad, Z)] * (T - len(tr)) for tr in trails]
        H = (out_t if out_t is not None else out_c).shape[1]
        parts = [x for x in (out_t, out_c) if x is not None] + [x.reshape(1, H) for x in vecs] + \
            [torch.zeros(1, H, device=self.device)]
        table = torch.cat(parts, 0)
        ix = torch.tensor([p for row in idx for p in row], dtype=torch.long).pin_memory().to(self.device,
                                                                                             non_blocking=True)
        rows = table[ix.view(-1)].view(-1, 2, H).sum(1)
        embeds = rows[:B * P].view(B, P, H)
        trail = rows[B * P:].view(B, T, H)
        mask = torch.tensor([[0] * (P - len(s)) + [1] * len(s) for s in seqs], dtype=torch.long).pin_memory().to(
            self.device, non_blocking=True)
        pad_e = table[pad].view(1, 1, H)
        return embeds, mask, trail, pad_e

    # -------------------------------------------------------------------------------- prefix cache
    def _prefix_bind(self, prefix_cache):
        """Check a call's prefix_cache= before anything is allocated; returns the list that build_prompts fills with
        the prompt lengths (None without a cache)."""
        if prefix_cache is None:
            return None
        if not isinstance(prefix_cache, PrefixCache):
            raise ValueError(f"prefix_cache must be a qwen_tts.PrefixCache, got {type(prefix_cache).__name__}")
        prefix_cache.bind(self.engine)
        return []

    @staticmethod
    def _prefix_plan(prefix_cache, instruct_ids, voice_clone_prompt, lens):
        """The engine's view of a call's cache use: request i's key is its instruction's ids.  Requests without an
        instruction, and every request of a voice-clone call (ICL or x-vector prompts), do not take part."""
        if prefix_cache is None:
            return None
        keys = [None] * len(lens)
        if instruct_ids is not None and voice_clone_prompt is None:
            keys = [None if ins is None else (PrefixCache.key(ins) or None) for ins in instruct_ids]
        if all(k is None for k in keys):
            return None  # nobody takes part: the call runs exactly the code it runs without a cache
        return PrefixPlan(prefix_cache, keys, lens)

    # -------------------------------------------------------------------------------- voice cache
    def _voice_bind(self, voice_cache):
        """Check a call's voice_cache= before anything is allocated, and bind it to the codec decoder."""
        if voice_cache is None:
            return None
        if not isinstance(voice_cache, VoiceCache):
            raise ValueError(f"voice_cache must be a qwen_tts.VoiceCache, got {type(voice_cache).__name__}")
        if self.speech_tokenizer is None:
            raise ValueError("voice_cache needs the speech tokenizer: load_speech_tokenizer() first")
        voice_cache.bind(self.speech_tokenizer.model)
        return voice_cache

    # -------------------------------------------------------------------------------- generate
    @torch.no_grad()
    def generate(self, input_ids=None, instruct_ids=None, ref_ids=None, voice_clone_prompt=None, languages=None,
                 speakers=None, non_streaming_mode=False, max_new_tokens=4096, do_sample=True, top_k=50, top_p=1.0,
                 temperature=0.9, subtalker_dosample=True, subtalker_top_k=50, subtalker_top_p=1.0,
                 subtalker_temperature=0.9, eos_token_id=None, repetition_penalty=1.05, ignore_eos=False, seed=None,
                 use_graph=True, max_batch=None, philox_ids=None, frame_caps=None, prefix_cache=None, **kwargs):
        """Same contract as Qwen3TTSForConditionalGeneration.generate (M:2022-2292):
        returns (list of [F_i,16] int64 codes, list of [F_i,H] last hidden states).

        philox_ids (not in the reference): the sampling stream id of each request (default its index in this call);
        the data-parallel runner (qwen_tts.dp.dp_generate) passes global request indices.  frame_caps (not in the
        reference): per-request frame limits below max_new_tokens - 1 (decoded through serve()).

        max_batch (not in the reference): with more requests than max_batch, decode them by continuous batching
        through max_batch batch rows (TalkerEngine.serve: a row is refilled with the next request as soon as its
        request ends).  Per request the result is that of the one-shot batched call (same Philox stream per request
        index; per-row arithmetic does not depend on the batch's other rows).

        Per-request sampling parameters (not in the reference): do_sample, top_k, top_p, temperature, the four
        subtalker_* values, repetition_penalty and seed each take a list with one entry per request (GenParams);
        request i then gets the codes of the same call made with its values as scalars.

        prefix_cache (not in the reference): a qwen_tts.PrefixCache.  A request whose instruction is in
        the cache adopts the instruction's talker K/V and prefills only the positions behind it; the first request
        that misses stores it.  None (default): every prefill computes the whole prompt."""
        lens = self._prefix_bind(prefix_cache)
        emb, mask, trail, pad = self.build_prompts(input_ids, languages, speakers, instruct_ids, non_streaming_mode,
                                                   voice_clone_prompt, ref_ids, lens_out=lens)
        plan = self._prefix_plan(prefix_cache, instruct_ids, voice_clone_prompt, lens)
        gp = GenParams(max_new_tokens, do_sample, top_k, top_p, temperature, subtalker_dosample, subtalker_top_k,
                       subtalker_top_p, subtalker_temperature, eos_token_id, repetition_penalty, ignore_eos, seed)
        B, P = emb.shape[0], emb.shape[1]
        gp.check_rows(B)
        if (max_batch is not None and B > int(max_batch)) or frame_caps is not None:
            n_real = mask.sum(-1).tolist()
            reqs = [(emb[i, P - int(n_real[i]):], trail[i], None if frame_caps is None else frame_caps[i])
                    for i in range(B)]
            max_batch = B if max_batch is None else max_batch
            codes, hid = [None] * B, [None] * B
            for i, c, h in self.engine.serve(reqs, pad, gp, slots=int(max_batch), use_graph=use_graph,
                                             philox_ids=philox_ids, prefix=plan):
                codes[i], hid[i] = c, h
            return codes, hid
        return self.engine.generate_from_embeds(emb, mask, trail, pad, gp, use_graph=use_graph, philox_ids=philox_ids,
                                                prefix=plan)

    @torch.no_grad()
    def teacher_forced(self, ref_codes, input_ids=None, instruct_ids=None, ref_ids=None, voice_clone_prompt=None,
                       languages=None, speakers=None, non_streaming_mode=False, repetition_penalty=1.05,
                       eos_token_id=None, use_graph=True, **kwargs):
        """Greedy choices of this path at every step of the reference's own code sequence (parity diagnostics; not in
        the reference): the prompt is assembled as generate() does, each talker / code-predictor argmax is recorded
        and then replaced by the reference token of ref_codes (list of [F_b, 16]).  Returns (picks [B, F, 16], hidden
        [B, F, H]) so a bf16 run can be compared with fp32 reference codes position by position."""
        emb, mask, trail, pad = self.build_prompts(input_ids, languages, speakers, instruct_ids, non_streaming_mode,
                                                   voice_clone_prompt, ref_ids)
        gp = GenParams(max_new_tokens=2, do_sample=False, subtalker_dosample=False, eos_token_id=eos_token_id,
                       repetition_penalty=repetition_penalty)
        return self.engine.teacher_forced(emb, mask, trail, pad, gp, ref_codes, use_graph=use_graph)

    # -------------------------------------------------------------------------------- streaming
    REF_CHUNK, REF_CTX = 300, 25  # Qwen3TTSTokenizerV2Decoder.chunked_decode (K:885-895)

    @torch.no_grad()
    def stream(self, input_ids=None, instruct_ids=None, ref_ids=None, voice_clone_prompt=None, languages=None,
               speakers=None, non_streaming_mode=False, max_new_tokens=4096, do_sample=True, top_k=50, top_p=1.0,
               temperature=0.9, subtalker_dosample=True, subtalker_top_k=50, subtalker_top_p=1.0,
               subtalker_temperature=0.9, eos_token_id=None, repetition_penalty=1.05, ignore_eos=False, seed=None,
               first_chunk_frames=1, chunk_frames=48, left_context=None, use_graph=True, max_batch=None,
               text_feed=None, sample_rate=None, pcm_format="f32", prefix_cache=None, voice_cache=None, speed=None,
               pitch=None, volume_gain_db=None, **kwargs):
        """Streaming generation (the reference has none): yields (row, pcm, last) as frames finish.

        Per row the chunks concatenate to the one-shot generate() + decode() PCM (Z:259-365): the reference
        decodes the zero-right-padded batch in 300-frame chunks with 25 frames of left context, dropping the
        last 555 samples of each chunk (no next frame), and keeps 1920 x #nonzero-cb0 samples.  Default
        (left_context=None): one stateful incremental decoder per reference chunk (codec.CodecStream, primed with the
        chunk's 25 context frames) is fed each final frame once and every sample computable so far is emitted (a
        chunk yields 1920 n - 555 samples after its n frames: no lookahead frame is waited for), so every sample is
        computed once and equals the one-shot output up to fp summation order.  An int `left_context` selects the
        stateless form instead (windows [s, e) within a reference chunk, one lookahead frame), re-decoded from
        min(its chunk's start, left_context frames back) -- 325 reproduces the reference, less is approximate (in
        fp32 150 frames -> rel-L2 1e-6, 72 -> 7e-4, 25 -> 2e-2; tools/stream_fidelity.py).  Codes are identical to
        generate().  pcm is a 1-D fp32 device tensor of 24 kHz samples.

        max_batch: with more requests than max_batch, stream them by continuous batching through max_batch batch
        rows (serve_stream(): a row is refilled as soon as its request ends; chunk_frames then defaults to 8).

        text_feed: a qwen_tts.TextFeed with one row per request -- the text arrives while the audio is
        generated.  input_ids[b] is then the request's head: the three role ids and at least one text id, no template
        suffix.  The prefill holds the first text id; later ones, from the head or pushed, are read one per frame, and
        a frame is queued only when every row that is neither closed nor finished has its token.  With
        first_chunk_frames=1 the first packet needs the first text id alone.  After feed.close(b), row b has decoded
        exactly what a whole-text call with role + text + suffix ids decodes in streaming-text mode.  When the text
        runs out, all audio generated so far is yielded, then the loop waits up to feed.timeout seconds and raises
        TextFeedTimeout.  Only the thread running this generator issues GPU work; push / close may come from any.

        sample_rate / pcm_format: pcm at that rate, fp32 or ("s16") int16.  Each row's default sample
        sequence goes through a stateful device resampler (resample.PcmResampler), one launch per codec report for all
        rows, so the chunks concatenate to the resampled whole -- ceil(N * up / down) samples for the default's N --
        bit for bit whatever the chunking.  Outputs that need samples not generated yet (at most 10 * max(1, down / up)
        input samples' worth) follow with the next chunk; last=True flushes, so the last chunk may hold samples where
        the default's is empty.  The stateless left_context form serves the default format only.

        prefix_cache: as in generate() -- with text_feed and with max_batch too.

        voice_cache: a qwen_tts.VoiceCache, used when max_batch routes the call to serve_stream(), which
        then serves voice-clone prompts with reference codes too; the other routes decode the reference themselves.

        speed: the speaking rate, 0.5 to 2.0 in hundredths -- a number, or one per request.  Each row's
        default sample sequence goes through the stateful device time-stretch (tempo.PcmTempo, in front of the
        resampler; one launch per codec report for all rows): the chunks concatenate to PcmTempo.one_shot of the
        default's, ceil(100 N / S) samples, bit for bit whatever the chunking.  The output for the last 25 to 35 ms
        of input is held back for the search and follows with the next chunk; last=True flushes.  A request at 1.0
        keeps the default's bits; with every request at 1.0 (or None) no stage is built.  The stateless left_context
        form does not serve it.

        pitch / volume_gain_db: the pitch in semitones, -12 to 12, and the gain in dB, -96 to 16 -- each a
        number, or one per request.  Pitch is resampling pitch (formants move with it): the tempo stage runs the
        request at T = floor(S / 2^(pitch/12) + 0.5) and prosody.PcmProsody resamples its output by T/S, so the
        duration stays ceil(100 N / S) samples and the realised pitch ratio is S/T (within 17.4 cents of the request).
        A positive gain runs a look-ahead peak limiter: no sample leaves above 1.0, and 127 more samples (under 6 ms)
        are held back.  The chunks concatenate to the one-shot chain of the default's samples bit for bit; a request
        at 0 / 0 keeps the default's bits, and with every request there nothing is built.  speed divided by the pitch
        ratio must lie in [0.5, 2.0].  The stateless left_context form does not serve them."""
        fmt = self._output_format(sample_rate, pcm_format)
        steps = prosody_steps(speed, pitch, volume_gain_db, 0 if input_ids is None else len(input_ids))
        self._voice_bind(voice_cache)
        lens = self._prefix_bind(prefix_cache)
        if fmt is not None and left_context is not None:
            raise NotImplementedError("stream(left_context=...) with sample_rate / pcm_format: use the default "
                                      "stateful stream")
        if steps is not None and left_context is not None:
            raise NotImplementedError("stream(left_context=...) with speed, pitch or volume_gain_db: use the default "
                                      "stateful stream")
        # GenParams' arguments, in its order: it validates them, so each route builds it where it always raised
        sampling = (max_new_tokens, do_sample, top_k, top_p, temperature, subtalker_dosample, subtalker_top_k,
                    subtalker_top_p, subtalker_temperature, eos_token_id, repetition_penalty, ignore_eos, seed)
        if text_feed is not None:
            yield from self._stream_fed(text_feed, input_ids, instruct_ids, voice_clone_prompt, languages, speakers,
                                        non_streaming_mode, left_context, max_batch, first_chunk_frames, chunk_frames,
                                        use_graph, GenParams(*sampling), fmt, prefix_cache, steps)
            return
        if max_batch is not None and input_ids is not None and len(input_ids) > int(max_batch):
            if left_context is not None:
                raise NotImplementedError("stream(left_context=...) with max_batch: use the default stateful stream")
            yield from self.serve_stream(
                input_ids, instruct_ids, ref_ids, voice_clone_prompt, languages, speakers, non_streaming_mode,
                *sampling, max_batch=max_batch, first_chunk_frames=first_chunk_frames,
                chunk_frames=8 if chunk_frames == 48 else chunk_frames, use_graph=use_graph, sample_rate=sample_rate,
                pcm_format=pcm_format, prefix_cache=prefix_cache, voice_cache=voice_cache, speed=speed,
                pitch=pitch, volume_gain_db=volume_gain_db, **kwargs)
            return
        dec = self.speech_tokenizer.model
        refs = voice_clone_prompt.get("ref_code") if voice_clone_prompt is not None else None
        prefix = None if refs is None or all(r is None for r in refs) else list(refs)
        # voice clone: the reference frames every row starts with are known at submit -- their codec decode starts on
        # a side stream before the (host-bound) prompt assembly, so it runs beside it instead of beside the prefill
        started = self._start_ref_decode(dec, prefix, len(prefix)) if prefix is not None and left_context is None \
            else None
        try:
            emb, mask, trail, pad = self.build_prompts(input_ids, languages, speakers, instruct_ids,
                                                       non_streaming_mode, voice_clone_prompt, ref_ids, lens_out=lens)
            plan = self._prefix_plan(prefix_cache, instruct_ids, voice_clone_prompt, lens)
            gp = GenParams(*sampling)
            gp.check_rows(emb.shape[0])
        except BaseException:
            # the side-stream reference decode holds a pooled codec slot: hand it back before the error propagates
            if started is not None:
                torch.cuda.current_stream(self.device).wait_stream(started[1])
                started[2].close()
            raise
        eos = self.engine.tc["codec_eos_token_id"]
        B = emb.shape[0]
        # chunk sizes double from first_chunk_frames up to chunk_frames: each chunk's audio (80 ms per frame) covers
        # the generation of the next one (~3 ms per frame), so playback started at the first packet never starves
        if left_context is None:
            yield from self._stream_stateful(dec, emb, mask, trail, pad, gp, B, eos, first_chunk_frames, chunk_frames,
                                             use_graph, prefix, started, fmt=fmt, plan=plan, steps=steps)
            return
        if prefix is not None:
            raise NotImplementedError("stream(left_context=...) with voice-clone reference codes (ICL): use the "
                                      "default stateful stream")
        up = dec.total_upsample
        RC, RX = self.REF_CHUNK, self.REF_CTX
        emitted = 0                       # windows [0, emitted) decoded for every row
        end = [None] * B                  # frame count of each row once its EOS is seen
        cap = [None] * B                  # one-shot sample count (1920 x #nonzero cb0) once the row has ended
        done = [False] * B
        cum = [0] * B                     # samples emitted per row
        it = self.engine.decode_iter(emb, mask, trail, pad, gp, use_graph=use_graph, every=chunk_frames,
                                     first=first_chunk_frames + 1, grow=True, prefix=plan)
        for sessions, frames, final in it:
            # codes of frames [0, frames) are final; column `frames` holds the next cb0 (EOS of finishing rows)
            codes = torch.cat([s.codes[:, :frames + 1] for s in sessions], 0)  # int32 [B, frames+1, 16], device
            c0 = codes[:, :, 0].cpu()
            if not final and sessions[0].watch is not None:  # (synchronised above) before any audio is handed out
                sessions[0].watch.check()
            for b in range(B):
                if end[b] is None:
                    hit = (c0[b, emitted:] == eos).nonzero()
                    if hit.numel():
                        end[b] = emitted + int(hit[0])
                if final and end[b] is None:
                    end[b] = frames
                if end[b] is not None and cap[b] is None:
                    cap[b] = up * int((c0[b, :end[b]] != 0).sum())
            # the batch's length once known: every row ended (longest row), or generation stopped
            t_end = max(end) if all(x is not None for x in end) else None
            target = t_end if t_end is not None else frames - 1  # else keep frame `frames-1` as lookahead
            while emitted < target:
                k = emitted // RC
                cend = (k + 1) * RC
                e = min(target, cend)
                closed = e == cend or e == t_end  # this reference chunk ends at e
                base = k * RC - (RX if k * RC - RX > 0 else k * RC)
                hi = e if closed else e + 1
                ctx = min(emitted - base, left_context)
                lo = emitted - ctx
                cc = codes[:, lo:hi].clone()
                for b in range(B):  # finished rows continue as the one-shot batch decode's zero padding
                    if end[b] is not None and end[b] < hi:
                        cc[b, max(end[b] - lo, 0):] = 0
                w = dec.forward(cc)
                n = up * (e - emitted) - (555 if closed else 0)
                for b in range(B):
                    if done[b]:
                        continue
                    take = n if cap[b] is None else max(0, min(n, cap[b] - cum[b]))
                    chunk = w[b, ctx * up:ctx * up + take]
                    cum[b] += take
                    last = cap[b] is not None and (cum[b] >= cap[b] or e == t_end)
                    done[b] = last
                    yield b, chunk, last
                emitted = e
            if t_end is not None and emitted >= t_end:
                for b in range(B):  # rows whose output was complete before the last window
                    if not done[b]:
                        done[b] = True
                        yield b, torch.zeros(0, device=codes.device), True
            if all(done):
                break

    def _stream_fed(self, feed, heads, instruct_ids, voice_clone_prompt, languages, speakers, non_streaming_mode,
                    left_context, max_batch, first_chunk_frames, chunk_frames, use_graph, gp, fmt=None,
                    prefix_cache=None, steps=None):
        """stream(text_feed=feed): the combinations it does not serve are refused before anything is allocated."""
        from .feed import TextFeed
        from .talker import TextGate
        refs = voice_clone_prompt.get("ref_code") if voice_clone_prompt is not None else None
        if refs is not None and any(r is not None for r in refs):
            raise NotImplementedError("stream(text_feed=...) with voice-clone reference codes (ICL): the reference "
                                      "text and codes take the text's place in the prefill; use x-vector-only prompts")
        if max_batch is not None:
            raise NotImplementedError("stream(text_feed=...) with max_batch: continuous batching takes whole texts")
        if left_context is not None:
            raise NotImplementedError("stream(text_feed=...) with left_context: use the default stateful stream")
        if non_streaming_mode:
            raise ValueError("stream(text_feed=...) needs non_streaming_mode=False: non-streaming mode puts the whole "
                             "text into the prefill")
        if not isinstance(feed, TextFeed):
            raise ValueError(f"text_feed must be a qwen_tts.TextFeed, got {type(feed).__name__}")
        heads = [torch.as_tensor(h).reshape(-1).tolist() for h in heads]
        B = len(heads)
        if feed.rows != B:
            raise ValueError(f"text_feed has {feed.rows} rows for {B} requests")
        for b, h in enumerate(heads):
            if len(h) < 4:
                raise ValueError(f"request {b}: a head is the three role ids plus at least one text id, got "
                                 f"{len(h)} ids")
        lens = None if prefix_cache is None else []
        emb, mask, trail, pad = self.build_prompts(heads, languages, speakers, instruct_ids, False,
                                                   voice_clone_prompt, None, open_text=True, lens_out=lens)
        plan = self._prefix_plan(prefix_cache, instruct_ids, voice_clone_prompt, lens)
        gp.check_rows(B)
        gate = TextGate(feed, [len(h) - 4 for h in heads], self.config["tts_eos_token_id"])
        yield from self._stream_stateful(self.speech_tokenizer.model, emb, mask, trail, pad, gp, B,
                                         self.engine.tc["codec_eos_token_id"], first_chunk_frames, chunk_frames,
                                         use_graph, gate=gate, fmt=fmt, plan=plan, steps=steps)

    @torch.no_grad()
    def serve_stream(self, input_ids=None, instruct_ids=None, ref_ids=None, voice_clone_prompt=None, languages=None,
                     speakers=None, non_streaming_mode=False, max_new_tokens=4096, do_sample=True, top_k=50,
                     top_p=1.0, temperature=0.9, subtalker_dosample=True, subtalker_top_k=50, subtalker_top_p=1.0,
                     subtalker_temperature=0.9, eos_token_id=None, repetition_penalty=1.05, ignore_eos=False,
                     seed=None, max_batch=8, first_chunk_frames=1, chunk_frames=8, use_graph=True, philox_ids=None,
                     frame_caps=None, sample_rate=None, pcm_format="f32", prefix_cache=None, voice_cache=None,
                     speed=None, pitch=None, volume_gain_db=None, **kwargs):
        """Streaming from the continuously batched route (the reference has neither): the requests are
        decoded through max_batch batch rows as generate(max_batch=...) decodes them, and each request's audio
        leaves as it is generated -- yields (request index, pcm, last).

        Per request the chunks concatenate to Qwen3TTSTokenizer.decode of that request's codes alone (300-frame
        reference chunks with 25 frames of left context, each chunk's last 555 samples dropped, 1920 x #nonzero-cb0
        samples kept), and the codes are generate(max_batch=...)'s.  The talker reports progress every chunk_frames
        frame replays, and first_chunk_frames after a row's refill (TalkerEngine.serve_iter); the new frames of
        every row go through one per-row incremental codec feed (codec.RowCodecStream: a refilled row begins, the
        others continue, idle ones ride along), so a refilled request has a first packet of its own.  A row that
        reaches the end of a reference chunk restarts on the chunk's 25 context frames (their output discarded)
        while the other rows carry on.  The sampling parameters take per-request lists as in generate().  Voice-clone
        prompts that carry reference codes (ICL) are not supported here; x-vector-only prompts are.
        sample_rate / pcm_format: as in stream() -- one resampler launch per codec feed for all slots, a slot's state
        reset when its request changes.  prefix_cache: as in generate() -- the first prefill and every refill use it.
        speed: as in stream(), a number or one per request -- a slot's tempo state is reset, and takes the new
        request's rate, when its request changes.  pitch / volume_gain_db: as in stream(), likewise.

        voice_cache: a qwen_tts.VoiceCache.  With one, prompts whose ref_code[i] is not None (ICL) are
        served too, mixed freely with x-vector-only and plain requests: request i's audio is the decode of
        cat(ref_i, codes_i) from sample 1920 R_i on, up to 1920 x #nonzero-cb0 of both (the rule _stream_stateful
        documents, its up-to-555-sample deviation from the wrapper's proportional cut included).  The row adopts the
        codec state behind the voice's reference frames from the cache (built on a miss on a one-row stream of its
        own), so a request's first chunk is 1920 x first_chunk_frames - 555 samples as for any other request."""
        fmt = self._output_format(sample_rate, pcm_format)
        steps = prosody_steps(speed, pitch, volume_gain_db, 0 if input_ids is None else len(input_ids))
        voice = self._voice_bind(voice_cache)
        refs = voice_clone_prompt.get("ref_code") if voice_clone_prompt is not None else None
        if voice is None and refs is not None and any(r is not None for r in refs):
            raise NotImplementedError("serve_stream() / stream(max_batch=...) with voice-clone reference codes (ICL): "
                                      "use stream() without max_batch, or x-vector-only prompts")
        lens = self._prefix_bind(prefix_cache)
        emb, mask, trail, pad = self.build_prompts(input_ids, languages, speakers, instruct_ids, non_streaming_mode,
                                                   voice_clone_prompt, ref_ids, lens_out=lens)
        plan = self._prefix_plan(prefix_cache, instruct_ids, voice_clone_prompt, lens)
        gp = GenParams(max_new_tokens, do_sample, top_k, top_p, temperature, subtalker_dosample, subtalker_top_k,
                       subtalker_top_p, subtalker_temperature, eos_token_id, repetition_penalty, ignore_eos, seed)
        N, P = emb.shape[0], emb.shape[1]
        gp.check_rows(N)
        n_real = mask.sum(-1).tolist()
        reqs = [(emb[i, P - int(n_real[i]):], trail[i], None if frame_caps is None else frame_caps[i])
                for i in range(N)]
        B = max(1, min(int(max_batch), N))
        first, every = max(1, int(first_chunk_frames)), max(1, int(chunk_frames))
        yield from self._serve_codec(
            self.engine.serve_iter(reqs, pad, gp, slots=B, use_graph=use_graph, every=every, first=first,
                                   philox_ids=philox_ids, prefix=plan), B, first, every, fmt, voice,
            None if refs is None else (lambda i: refs[i]), None if steps is None else steps.__getitem__)

    def _serve_codec(self, reports, B, first, every, fmt, voice=None, ref_of=None, step_of=None):
        """The codec half of serve_stream() and serve_live(): consumes the talker's (session, report) items
        (TalkerEngine.serve_iter / serve_live_iter) and yields (request, pcm, last).  A row without new frames in a
        report -- idle, or held -- rides along.  An item (None, [requests]) names requests that end without audio.
        step_of(request) -> its (S, T, db) (prosody.steps), asked once when the request takes its
        slot; the output stages are built when the first request off the defaults arrives (_slot_output), so a call
        without one runs the default path.

        voice (a VoiceCache): requests with reference codes are served beside the others, ref_of(request)
        -> its reference codes or None.  Request i decodes cat(ref_i, codes_i): its generated frame t sits at joint
        position R_i + t, and the chunk walk (voice.joint_walk), the restarts and the 1920 x #nonzero-cb0 length rule
        (voice.feed_span) run over joint positions; without a voice cache R_i = 0 and they are the plain request's.
        In the first report of its slot the request's voice entry is looked up or built (VoiceCache.get: on a miss
        the reference frames are decoded on a one-row stream of their own, never through this stream's feeds), and
        the row adopts the entry's state -- all rows adopting in that report in one qt_codec_row_state launch.  The
        code window of every feed is then assembled on the device from the joint positions (qt_codec_feed_codes), so
        a restart's 25 context frames come from reference and / or generated frames alike; a call without a voice
        cache gathers it from the session's codes by index."""
        dec = self.speech_tokenizer.model
        up, RC, RX = dec.total_upsample, self.REF_CHUNK, self.REF_CTX
        caps = sorted({first, every})  # feed capacities (one captured codec graph each)
        dev = self.device
        rs = dec.row_stream(B, RX + RC, caps[-1])
        out = None if fmt is None else PcmResampler(B, fmt[0].sample_rate, fmt[1], fmt[0].in_rate, dev)
        req = [-1] * B        # request in each slot, as the codec has seen it
        discard = [0] * B     # samples of the slot's decode still to drop (a restarted chunk's context, the boundary)
        extra = [0] * B       # ... to drop on top of the context's at the request's first begin (R a chunk multiple)
        cum = [0] * B         # sample of the request's whole decode the slot has reached (1920 R at its start)
        nz = [0] * B          # nonzero cb0 among the request's reference and final frames
        Rb = [0] * B          # reference frames of the slot's request
        held = [None] * B     # the slot's voice entry (keeps its reference codes alive while the row reads them)
        if voice is None:
            ref_of = None
            rows_ix = torch.arange(B, device=dev)[:, None]
        else:
            # per-slot reference table of qt_codec_feed_codes: pointers and lengths, re-uploaded when a slot's request
            # changes; the joint positions of a feed go up from pinned memory in stream order
            ref_ptr = torch.zeros(B, dtype=torch.int64, device=dev)
            ref_len = torch.zeros(B, dtype=torch.int32, device=dev)

        def window(codes, rows, n):
            """The feed's code window [B, n, Q]: row b's joint positions rows[b], filler behind them"""
            fill, dt = (0, torch.long) if voice is None else (-1, torch.int32)
            pos = torch.tensor([r + [fill] * (n - len(r)) for r in rows], dtype=dt).pin_memory().to(
                dev, non_blocking=True)
            if voice is None:
                return codes[rows_ix, pos]
            win = torch.empty(B, n, codes.shape[2], dtype=torch.int32, device=dev)
            K.codec_feed_codes(pos, ref_ptr, ref_len, codes, win)
            return win
        try:
            for s, report in reports:
                if s is None:
                    for i in report:
                        if ref_of is not None:
                            ref_of(i)  # (a live loop forgets the request's reference)
                        yield i, self._empty(fmt), True
                    continue
                # per slot: the joint positions to feed, and the positions in that list at which the row (re)starts
                todo, marks, ended = [[] for _ in range(B)], [{} for _ in range(B)], [False] * B
                adopt, changed = [], False
                for b, r in enumerate(report):
                    if r is None:
                        continue
                    i, lo, f, ended[b], nzb = r
                    if req[b] != i:
                        req[b], discard[b], extra[b], cum[b], nz[b], Rb[b], held[b] = i, 0, 0, 0, 0, 0, None
                        out = self._slot_output(out, b, (100, 100, 0.0) if step_of is None else step_of(i), fmt, B)
                        ref = None if ref_of is None else ref_of(i)
                        if ref is not None and len(ref) > 0:
                            e = held[b] = voice.get(dec, ref)
                            Rb[b], nz[b], cum[b] = e.R, e.nz, up * e.R
                            takes, skip = boundary_skip(e.R, RC)
                            if takes:
                                adopt.append((b, e))
                                discard[b] = skip
                            else:
                                extra[b] = skip
                        changed = True
                    nz[b] += nzb
                    # a frame that opens a reference chunk begins the row, after chunk 0 on the 25 context frames
                    todo[b], mk = joint_walk(Rb[b], lo, f, RC, RX)
                    marks[b] = {k: c * up for k, c in mk.items()}
                    if ended[b] and not todo[b]:  # nothing new: the request's audio was complete already
                        yield i, self._flush_row(out, b, fmt), True
                if changed and voice is not None:
                    tab = [[0 if held[b] is None else held[b].ref.data_ptr() for b in range(B)], Rb]
                    ref_ptr.copy_(torch.tensor(tab[0], dtype=torch.int64).pin_memory(), non_blocking=True)
                    ref_len.copy_(torch.tensor(tab[1], dtype=torch.int32).pin_memory(), non_blocking=True)
                if adopt:
                    main = torch.cuda.current_stream(dev)
                    for _, e in adopt:
                        if e.event is not None:
                            main.wait_event(e.event)
                    rs.adopt_rows([(b, e.snapshot) for b, e in adopt])
                at = [0] * B
                while any(at[b] < len(todo[b]) for b in range(B)):
                    nrow, begin = [0] * B, [0] * B
                    for b in range(B):  # (a restart opens a feed of its own)
                        nrow[b], begin[b] = plan_feed(todo[b], marks[b], at[b], caps[-1])
                    n = next(c for c in caps if c >= max(nrow))
                    pcm = rs.feed(window(s.codes, [todo[b][at[b]:at[b] + nrow[b]] for b in range(B)], n), nrow, begin)
                    pend = []  # (slot, first sample, samples, last) of this feed, for the resampler's one launch
                    for b in range(B):
                        if not nrow[b]:
                            continue
                        ctx_s = marks[b][at[b]] if begin[b] else 0
                        at[b] += nrow[b]
                        lo_s, hi_s, last, discard[b], extra[b], cum[b] = feed_span(
                            begin[b], nrow[b], ctx_s, ended[b], at[b] == len(todo[b]), nz[b], discard[b], extra[b],
                            cum[b], up)
                        if hi_s > lo_s or last:
                            if out is not None:
                                pend.append((b, lo_s, hi_s - lo_s, last))
                                continue
                            yield req[b], pcm[b, lo_s:hi_s].clone(), last
                    if pend:
                        yield from self._resampled(out, pcm, pend, req)
        finally:
            rs.close()
            reports.close()

    @torch.no_grad()
    def serve_live(self, queue, max_batch=8, max_prompt=512, max_new_tokens=4096, eos_token_id=None, ignore_eos=False,
                   seed=None, first_chunk_frames=1, chunk_frames=8, use_graph=True, sample_rate=None, pcm_format="f32",
                   prefix_cache=None, voice_cache=None):
        """Live serving (the reference has none): serve_stream() over an open request stream.  `queue` is
        a qwen_tts.RequestQueue; requests are submitted to it while this generator runs, each with its own sampling
        parameters, and decoded through max_batch batch rows as they arrive -- yields (request id, pcm, last).

        A whole-text request gets the codes generate(max_batch=...) gives the request of that index and seed, and the
        audio serve_stream() gives it.  An open-text request (submit(head, open_text=True): the three role ids and at
        least one text id) receives its text through queue.push / close_text while it decodes, as
        stream(text_feed=...) does, and decodes what the whole-text request decodes in streaming-text mode; while its
        next token is missing its row is held and the other rows go on (TalkerEngine._run_frame_held).  It still gets
        a one-frame first packet from its first text id alone.  A request starved for queue.timeout seconds is
        retired with the audio it has (queue.timed_out), as is a cancelled one; one that cannot be served -- a prompt
        longer than max_prompt, voice-clone reference codes (ICL), open_text with non_streaming_mode, an unknown
        speaker or language -- is yielded once as (id, empty, True) with the reason in queue.rejected[id].  None of
        them ends the loop: it ends when the queue is closed and every request is over.

        Only the thread running this generator issues GPU work, prompt assembly included (at admission).  max_prompt:
        the K/V capacity per row in prompt positions.  seed: the call's seed, for requests that name none; request i
        draws Philox stream i.  sample_rate / pcm_format / prefix_cache / voice_cache: as in serve_stream() -- with a
        voice_cache, a request submitted with reference codes (and its reference text: submit(..., ref_ids=...)) is
        served; without one it stays a rejection.  A request's speaking rate, pitch and gain are submit(speed=...,
        pitch=..., volume_gain_db=...)'s."""
        from .live import RequestQueue
        if not isinstance(queue, RequestQueue):
            raise ValueError(f"queue must be a qwen_tts.RequestQueue, got {type(queue).__name__}")
        fmt = self._output_format(sample_rate, pcm_format)
        voice = self._voice_bind(voice_cache)
        live_refs = {}  # request -> its reference codes, from admission until the codec half has taken them
        live_steps = {}  # request -> its (S, T, db) where it is off the defaults (submit(speed=...)), likewise
        self._prefix_bind(prefix_cache)
        B = int(max_batch)
        if not 1 <= B <= 64:
            raise ValueError(f"serve_live takes 1..64 batch rows, got {max_batch}")
        first, every = max(1, int(first_chunk_frames)), max(1, int(chunk_frames))
        cfg = self.config
        one = lambda v: (v,)  # noqa: E731 -- every ROW_FIELD as a list: the session reads per-row tables
        gp = GenParams(max_new_tokens, one(True), one(50), one(1.0), one(0.9), one(True), one(50), one(1.0), one(0.9),
                       eos_token_id, one(1.05), ignore_eos, seed)
        pad = self.engine.text_proj([cfg["tts_pad_token_id"]])

        def prepare(r):
            vcp = r.voice_clone_prompt
            refs = vcp.get("ref_code") if vcp is not None else None
            icl = refs is not None and any(x is not None for x in refs)
            if icl and voice is None:
                raise NotImplementedError("serve_live() with voice-clone reference codes (ICL): use stream(), or "
                                          "x-vector-only prompts")
            if vcp is not None and any(vcp.get("icl_mode") or []) and (not icl or r.ref_ids is None):
                raise ValueError("a voice-clone request in icl_mode needs its reference codes and the reference "
                                 "text's ids: submit(..., voice_clone_prompt=..., ref_ids=...)")
            if icl and r.open_text:
                raise NotImplementedError("open_text with voice-clone reference codes (ICL): the reference text and "
                                          "codes take the text's place in the prefill")
            if r.open_text and r.non_streaming_mode:
                raise ValueError("open_text needs non_streaming_mode=False: non-streaming mode puts the whole text "
                                 "into the prefill")
            if r.open_text and len(r.input_ids) < 4:
                raise ValueError(f"an open-text head is the three role ids plus at least one text id, got "
                                 f"{len(r.input_ids)} ids")
            sp = r.sampling
            rgp = GenParams(max_new_tokens, one(sp["do_sample"]), one(sp["top_k"]), one(sp["top_p"]),
                            one(sp["temperature"]), one(sp["subtalker_dosample"]), one(sp["subtalker_top_k"]),
                            one(sp["subtalker_top_p"]), one(sp["subtalker_temperature"]), eos_token_id,
                            one(sp["repetition_penalty"]), ignore_eos, one(sp["seed"]))
            lens = []
            ins = None if r.instruct_ids is None else [r.instruct_ids]
            emb, _, trail, _ = self.build_prompts([r.input_ids], [r.language or "auto"], [r.speaker], ins,
                                                  r.non_streaming_mode, vcp, [r.ref_ids] if icl else None,
                                                  open_text=r.open_text, lens_out=lens)
            plan = self._prefix_plan(prefix_cache, ins, vcp, lens)
            if icl:
                # (a malformed reference rejects the request here, not in the loop)
                check_codes(self.speech_tokenizer.model, VoiceCache.codes_array(refs[0]))
                live_refs[r.id] = refs[0]
            if r.step != (100, 100, 0.0):
                live_steps[r.id] = r.step
            return emb[0], trail[0], rgp, plan

        yield from self._serve_codec(
            self.engine.serve_live_iter(queue, pad, gp, prepare, slots=B, max_prompt=max_prompt, use_graph=use_graph,
                                        every=every, first=first, text_eos=cfg["tts_eos_token_id"]), B, first, every,
            fmt, voice, lambda i: live_refs.pop(i, None), lambda i: live_steps.pop(i, (100, 100, 0.0)))

    def _output_format(self, sample_rate, pcm_format):
        """The streams' output format, validated before anything is allocated: None = the codec's own (24 kHz fp32,
        no resampler), else (resample.Plan, pcm_format)."""
        tok = self.speech_tokenizer
        return output_format(sample_rate, pcm_format, 24000 if tok is None else tok.get_output_sample_rate())

    def _output_stage(self, B, fmt, steps):
        """The output stage of a stream of B rows: None for the default output, the resampler for another format, and
        with steps (prosody.steps(): one (S, T, db) per row) the tempo stage in front of it, and the prosody stage
        behind that where a row has a pitch or a gain (tempo.PcmOutput)."""
        if steps is not None:
            return PcmOutput(B, steps, fmt, self.device)
        return None if fmt is None else PcmResampler(B, fmt[0].sample_rate, fmt[1], fmt[0].in_rate, self.device)

    def _slot_output(self, out, b, step, fmt, B):
        """Slot b of a serving route's output stage `out` takes a new request at `step`, its (S, T, db) (an entry of
        prosody.steps()): its state is reset.  The first request at another rate than 1.0, or with a pitch or a gain,
        puts the stages in front of what there was (the resampler keeps its state; default rows are copied, so
        requests under way are not disturbed).  Returns the stage."""
        if step != (100, 100, 0.0) and not isinstance(out, PcmOutput):
            out = PcmOutput(B, None, fmt, self.device, rs=out)
        if isinstance(out, PcmOutput):
            out.reset(b, step)
        elif out is not None:
            out.reset(b)
        return out

    def _empty(self, fmt):
        """A chunk without samples, in the output format's dtype."""
        return torch.zeros(0, dtype=torch.int16 if fmt is not None and fmt[1] == "s16" else torch.float32,
                           device=self.device)

    def _flush_row(self, out, b, fmt):
        """The last chunk of a row whose input was complete already: what its output stage still holds back, by a
        push that only flushes that row (nothing without a stage)."""
        if out is None:
            return self._empty(fmt)
        B = out.rows
        return out.push(None, [0] * B, [0] * B, [c == b for c in range(B)])[b]

    @staticmethod
    def _resampled(out, pcm, pend, names=None):
        """One resampler launch for the (row, first sample, samples, last) entries of `pend`, samples taken from
        pcm [B, L]; yields (row or names[row], chunk, last) for the rows that got samples or end."""
        B = out.rows
        offs, lens, flush = [0] * B, [0] * B, [False] * B
        for b, o, n, last in pend:
            offs[b], lens[b], flush[b] = o, n, last
        chunks = out.push(pcm, offs, lens, flush)
        for b, _, _, last in pend:
            if chunks[b].numel() or last:
                yield (b if names is None else names[b]), chunks[b], last

    @staticmethod
    def _stream_window(codes, pre, R, end, lo, hi):
        """Decode positions [lo, hi) of every row's sequence prefix_b + generated_b + zeros, int32 [B, hi-lo, 16]
        (generated frame f of row b sits at position R_b + f; rows past their end are the batch decode's zero
        padding)."""
        B = codes.shape[0]
        if not any(R):
            cc = codes[:, lo:hi].clone()
            for b in range(B):
                if end[b] is not None and end[b] < hi:
                    cc[b, max(end[b] - lo, 0):] = 0
            return cc
        cc = torch.zeros(B, hi - lo, codes.shape[2], dtype=codes.dtype, device=codes.device)
        for b in range(B):
            if R[b] > lo:  # prefix part
                cc[b, :min(R[b], hi) - lo] = pre[b][lo:min(R[b], hi)]
            g0, g1 = max(lo, R[b]) - R[b], hi - R[b]  # generated frames [g0, g1)
            if end[b] is not None:
                g1 = min(g1, end[b])
            if g1 > g0:
                cc[b, g0 + R[b] - lo:g1 + R[b] - lo] = codes[b, g0:g1]
        return cc

    def _start_ref_decode(self, dec, prefix, B):
        """Feed every row's leading reference frames (the first min(R_b, 300) of them) to a fresh incremental decoder
        on a side stream; returns (pre, side stream, decoder, frames fed) for _stream_stateful, or None when some row
        has no reference frames."""
        dev = self.device
        pre = [None if x is None else torch.as_tensor(x).to(dev, torch.int32) for x in prefix]
        if any(x is None or x.shape[0] == 0 for x in pre):
            return None
        main = torch.cuda.current_stream(dev)
        side = K.side_stream(dev)
        side.wait_stream(main)
        with torch.cuda.stream(side):  # (the stream's state slot brings its own split-K workspace)
            cs = dec.stream(B, self.REF_CTX + self.REF_CHUNK)
            fed = min(min(int(x.shape[0]) for x in pre), self.REF_CHUNK)
            cs.feed(torch.stack([x[:fed] for x in pre]))
        return pre, side, cs, fed

    def _stream_stateful(self, dec, emb, mask, trail, pad, gp, B, eos, first_chunk_frames, chunk_frames, use_graph,
                         prefix=None, started=None, gate=None, fmt=None, plan=None, steps=None):
        """stream() on the incremental codec: every final frame is fed once to the decoder of its reference chunk
        and every sample computable from the frames fed so far is emitted -- 1920 n - 555 samples of a chunk after
        its n frames, i.e. no lookahead frame is waited for (the 555 samples that need it follow with the next
        chunk; at a reference chunk's end they are dropped, as the reference's chunked decode drops them).

        prefix[b] (voice clone, ICL mode): the reference codes int [R_b, 16] that generate_voice_clone decodes in
        front of row b's generated codes (W:263-274, `cat(ref_code, codes)` then a proportional cut).  Row b's decode
        sequence is then ref_b + generated + zero padding; the ref frames are known at submit and fed with the first
        chunk, and row b's output starts at sample 1920 R_b of its sequence, the reference/generated boundary.  The
        wrapper's proportional cut int(R_b / T_b * len_b) lands floor(555 R_b / T_b) samples earlier (len_b lacks
        the last frame's 555 lookahead samples), at a point that depends on the final length T_b, which a stream
        does not know when it starts: the streamed PCM is generate_voice_clone's PCM without those leading samples
        (< 555, e.g. 72 for 38 reference frames + 256 generated)."""
        up = dec.total_upsample
        RC, RX = self.REF_CHUNK, self.REF_CTX
        dev = self.device
        if started is not None:
            pre = started[0]
        else:
            pre = [None] * B if prefix is None else [None if x is None else torch.as_tensor(x).to(dev, torch.int32)
                                                      for x in prefix]
        R = [0 if x is None else int(x.shape[0]) for x in pre]
        pre_nz = [0 if x is None else int((x[:, 0] != 0).sum()) for x in pre]
        end = [None] * B                  # generated frame count of each row once its EOS is seen
        cap = [None] * B                  # one-shot sample count (1920 x #nonzero cb0 of its sequence) once ended
        done = [False] * B
        skip = [up * r for r in R]        # samples of row b's sequence before its output starts
        gpos = 0                          # samples of the (shared) decode timeline produced so far
        scanned = 0                       # cb0 columns already searched for EOS
        k, cs, fed, emit_s, ctx_s = 0, None, 0, 0, 0   # reference chunk, its decoder, positions fed, samples emitted
        main, side = torch.cuda.current_stream(dev), None
        out = self._output_stage(B, fmt, steps)
        if started is not None:  # stream() began decoding the reference frames before the prompt assembly
            _, side, cs, fed = started
        elif min(R) > 0:
            # every row starts with reference frames, known at submit: decode them on a side stream while the talker
            # prefills and generates the first frames on this one
            _, side, cs, fed = self._start_ref_decode(dec, pre, B)
        # a one-frame first chunk is handed over as soon as frame 0's codes exist: its codec window is queued before the
        # talker step that starts frame 1 (the first packet does not wait for it)
        it = self.engine.decode_iter(emb, mask, trail, pad, gp, use_graph=use_graph, every=chunk_frames,
                                     first=first_chunk_frames, grow=True, early_first=first_chunk_frames == 1,
                                     gate=gate, prefix=plan)
        try:
            for sessions, frames, final in it:
                if side is not None:
                    main.wait_stream(side)
                    side = None
                # codes of frames [0, frames) are final; column `frames` holds the next cb0 (EOS of finishing rows)
                codes = torch.cat([s.codes[:, :frames + 1] for s in sessions], 0)  # int32 [B, frames+1, 16], device
                # the EOS scan reads cb0 on the host (a sync on the frame just launched); columns [0, frames] hold
                # tokens sampled at n_generated <= frames, and EOS is suppressed below MIN_NEW_TOKENS, so the first
                # chunk skips the scan and its codec feed is queued right behind the frame
                # frames not covered by a watch check yet (the early first chunk skips the scan): checked, behind their
                # codec feed, before the first of their audio is handed out
                unchecked = not (final or frames + 1 > MIN_NEW_TOKENS)
                if not unchecked:
                    c0 = codes[:, :, 0].cpu()
                    for b in range(B):
                        if end[b] is None:
                            hit = (c0[b, scanned:] == eos).nonzero()
                            if hit.numel():
                                end[b] = scanned + int(hit[0])
                        if final and end[b] is None:
                            end[b] = frames
                        if end[b] is not None and cap[b] is None:
                            cap[b] = up * (pre_nz[b] + int((c0[b, :end[b]] != 0).sum()))
                    scanned = frames
                    # the host just synchronised on these frames: a hand-off give-up among them raises before any
                    # of their audio is handed out
                    if sessions[0].watch is not None:
                        sessions[0].watch.check()
                # decode positions (prefix + generated) available for every row; the sequence length once all ended
                t_end = max(R[b] + end[b] for b in range(B)) if all(x is not None for x in end) else None
                avail = t_end if t_end is not None else min(R[b] + frames for b in range(B) if end[b] is None)
                while True:
                    cend = (k + 1) * RC
                    if cs is None:  # reference chunk k: a fresh decoder, primed from its 25 context frames
                        base = k * RC - (RX if k * RC - RX > 0 else k * RC)
                        cs, fed, emit_s, ctx_s = dec.stream(B, RX + RC), base, 0, (k * RC - base) * up
                    hi = min(avail, cend)
                    if hi > fed:
                        cc = self._stream_window(codes, pre, R, end, fed, hi)
                        cs.feed(cc)
                        fed = hi
                    n = max(cs.ns - ctx_s - emit_s, 0)
                    ended = t_end is not None and fed >= t_end
                    pend = []  # (row, first sample, samples, last) of this report, for the resampler's one launch
                    for b in range(B):
                        if done[b] or n == 0:
                            continue
                        lo_s = max(gpos, skip[b])
                        hi_s = gpos + n if cap[b] is None else min(gpos + n, cap[b])
                        last = cap[b] is not None and (gpos + n >= cap[b] or ended)
                        if hi_s <= lo_s and not last:
                            continue
                        o = ctx_s + emit_s + (lo_s - gpos)
                        chunk = cs.pcm[b, o:o + max(hi_s - lo_s, 0)]
                        done[b] = last
                        if out is not None:
                            pend.append((b, o, max(hi_s - lo_s, 0), last))
                            continue
                        if unchecked:  # flags copied behind the feed that produced this PCM: the caller waits on it anyway
                            HandoffWatch(sessions).check()
                            unchecked = False
                        yield b, chunk, last
                    if pend:  # queued directly behind the codec feed, before the hand-off check synchronises
                        chunks = list(self._resampled(out, cs.pcm, pend))
                        if unchecked:
                            HandoffWatch(sessions).check()
                            unchecked = False
                        yield from chunks
                    emit_s += n
                    gpos += n
                    if fed == cend and not ended:  # chunk k complete (its 555-sample tail is dropped): next chunk
                        cs.close()
                        cs, k = None, k + 1
                        continue
                    break
                if t_end is not None and fed >= t_end:
                    for b in range(B):  # rows whose output was complete before the last window
                        if not done[b]:
                            if unchecked:
                                HandoffWatch(sessions).check()
                                unchecked = False
                            done[b] = True
                            yield b, self._flush_row(out, b, fmt), True
                if all(done):
                    break
        finally:
            if cs is not None:
                cs.close()
