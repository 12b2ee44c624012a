"""Drop-in `Qwen3TTSModel` (reference: qwen_tts/inference/qwen3_tts_model.py, `W` below).

Same public surface and semantics: from_pretrained, generate_custom_voice / generate_voice_design /
generate_voice_clone (from reference audio or a prepared voice_clone_prompt), create_voice_clone_prompt,
get_supported_speakers / languages, kwargs
precedence of `_merge_generate_kwargs` (W:287-352), validation errors (W:141-186), wrapper defaults
(max_new_tokens 2048, non_streaming_mode True/True/False) and the 0.6B instruct drop (W:799).
New: `stream()` yields (pcm chunk, sr) per utterance as soon as its codes are decoded.
All compute runs on the MI355X engine (qwen_tts/model.py + qwen_tts/codec.py).
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Tuple, Union

import numpy as np
import torch

from .. import audio as _audio
from .. import kernels as _kernels
from .. import resample as _resample
from .. import prosody as _prosody
from ..live import SAMPLING_DEFAULTS, RequestQueue
from ..model import TTSModel
from ..text import load_processor
from ..speaker import speaker_specs
from ..weights import is_preset_dir, load_safetensors, read_json, resolve_path, synthetic, talker_specs
from .qwen3_tts_tokenizer import Qwen3TTSTokenizer, _dtype_name

AudioLike = Union[str, np.ndarray, Tuple[np.ndarray, int]]
MaybeList = Union[Any, List[Any]]


@dataclass
class VoiceClonePromptItem:
    """W:40-51."""
    ref_code: Optional[torch.Tensor]
    ref_spk_embedding: torch.Tensor
    x_vector_only_mode: bool
    icl_mode: bool
    ref_text: Optional[str] = None


def save_voice_clone_prompt(items: List[VoiceClonePromptItem], path: str) -> None:
    """The reference demo's voice file (qwen_tts/cli/demo.py:514-521): torch.save({"items": [asdict(item)]}),
    tensors moved to the CPU so the file loads anywhere."""
    from dataclasses import asdict
    out = []
    for it in items:
        d = asdict(it)
        for k in ("ref_code", "ref_spk_embedding"):
            if isinstance(d[k], torch.Tensor):
                d[k] = d[k].detach().cpu()
        out.append(d)
    torch.save({"items": out}, path)


def load_voice_clone_prompt(path: str) -> List[VoiceClonePromptItem]:
    """Read a voice file written by save_voice_clone_prompt or the reference demo (demo.py:527-563), with
    torch.load(weights_only=True) like the reference: no code in the file is executed."""
    payload = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(payload, dict) or "items" not in payload:
        raise ValueError("Invalid file format")
    raw = payload["items"]
    if not isinstance(raw, list) or len(raw) == 0:
        raise ValueError("Empty voice items")
    items = []
    for d in raw:
        if not isinstance(d, dict):
            raise ValueError("Invalid item format in file")
        ref_code = d.get("ref_code", None)
        if ref_code is not None and not torch.is_tensor(ref_code):
            ref_code = torch.tensor(ref_code)
        spk = d.get("ref_spk_embedding", None)
        if spk is None:
            raise ValueError("Missing ref_spk_embedding")
        if not torch.is_tensor(spk):
            spk = torch.tensor(spk)
        xv = bool(d.get("x_vector_only_mode", False))
        items.append(VoiceClonePromptItem(ref_code=ref_code, ref_spk_embedding=spk, x_vector_only_mode=xv,
                                          icl_mode=bool(d.get("icl_mode", not xv)), ref_text=d.get("ref_text", None)))
    return items


class _TextRequestQueue(RequestQueue):
    """Qwen3TTSModel.request_queue(): a RequestQueue whose submit() also takes strings."""

    def __init__(self, wrapper: "Qwen3TTSModel", timeout: float):
        super().__init__(timeout)
        self._wrapper, self.processor = wrapper, wrapper.processor

    def submit(self, input_ids=None, *, text=None, instruct=None, language=None, speaker=None, open_text=False,
               non_streaming_mode=None, **kwargs) -> int:
        w = self._wrapper
        if (text is None) == (input_ids is None):
            raise ValueError("submit() takes either text=... or input_ids")
        if text is not None:
            ids, ins, langs, spks = w._custom_voice_inputs(text, speaker, language, instruct)
            if len(ids) != 1:
                raise ValueError("submit() takes one utterance per request")
            input_ids, language, speaker = ids[0], langs[0], spks[0]
            if ins[0] is not None:
                kwargs["instruct_ids"] = ins[0]
            if open_text:  # the head: role ids + the first piece, no template suffix
                input_ids = w._tokenize_texts([f"<|im_start|>assistant\n{text}"])[0]
        if non_streaming_mode is None:
            non_streaming_mode = not open_text
        sampling = {k: kwargs.pop(k, None) for k in SAMPLING_DEFAULTS if k != "seed"}
        merged = w._merge_generate_kwargs(**sampling)
        merged.pop("max_new_tokens")
        return super().submit(input_ids, language=language, speaker=speaker, open_text=open_text,
                              non_streaming_mode=non_streaming_mode, **merged, **kwargs)


class Qwen3TTSModel:
    def __init__(self, model: TTSModel, processor, generate_defaults: Optional[Dict[str, Any]] = None):
        self.model = model
        self.processor = processor
        self.generate_defaults = generate_defaults or {}
        self.device = model.device

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path: str, device_map="cuda:0", dtype=None,
                        attn_implementation=None, weights=None, codec_weights=None, seed: int = 1234,
                        **kwargs) -> "Qwen3TTSModel":
        """W:82-121.  A local checkpoint dir (config.json, generation_config.json, model*.safetensors,
        speech_tokenizer/) or a synthetic preset / hub id (offline: synthetic weights).  `attn_implementation`
        is accepted for API compatibility; attention always runs on the HIP kernel."""
        d = resolve_path(pretrained_model_name_or_path)
        cfg = read_json(os.path.join(d, "config.json"))
        if cfg.get("model_type") != "qwen3_tts":
            raise TypeError(f"expected a qwen3_tts checkpoint, got model_type={cfg.get('model_type')!r}")
        gpath = os.path.join(d, "generation_config.json")
        gen = read_json(gpath) if os.path.exists(gpath) else {}
        dev = torch.device(device_map if isinstance(device_map, str) and device_map.startswith("cuda") else "cuda:0")
        W = weights if weights is not None else load_safetensors(d)
        if not W:
            if not is_preset_dir(d):
                raise FileNotFoundError(f"no model*.safetensors in checkpoint directory {d!r}")
            specs = talker_specs(cfg)
            if cfg.get("tts_model_type") == "base":
                specs = specs + speaker_specs(cfg)
            W = synthetic(specs, dev, seed)
        with torch.cuda.device(dev):
            m = TTSModel(cfg, W, dtype=_dtype_name(dtype), device=dev, generate_config=gen)
        del W
        m.load_speech_tokenizer(Qwen3TTSTokenizer.from_pretrained(os.path.join(d, "speech_tokenizer"), device_map=dev,
                                                                  dtype=dtype, weights=codec_weights, seed=seed))
        return cls(m, load_processor(d), gen)

    # ---------------------------------------------------------------- validation (W:123-186)
    def _supported_languages_set(self):
        v = self.model.get_supported_languages()
        return None if v is None else set(str(x).lower() for x in v)

    def _supported_speakers_set(self):
        v = self.model.get_supported_speakers()
        return None if v is None else set(str(x).lower() for x in v)

    def _validate_languages(self, languages):
        sup = self._supported_languages_set()
        if sup is None:
            return
        bad = [x for x in languages if x is None or str(x).lower() not in sup]
        if bad:
            raise ValueError(f"Unsupported languages: {bad}. Supported: {sorted(sup)}")

    def _validate_speakers(self, speakers):
        sup = self._supported_speakers_set()
        if sup is None:
            return
        bad = [s for s in speakers if s not in (None, "") and str(s).lower() not in sup]
        if bad:
            raise ValueError(f"Unsupported speakers: {bad}. Supported: {sorted(sup)}")

    def _ensure_list(self, x: MaybeList) -> List[Any]:
        return x if isinstance(x, list) else [x]

    def _build_assistant_text(self, text: str) -> str:
        return f"<|im_start|>assistant\n{text}<|im_end|>\n<|im_start|>assistant\n"

    def _build_ref_text(self, text: str) -> str:
        return f"<|im_start|>assistant\n{text}<|im_end|>\n"

    def _build_instruct_text(self, instruct: str) -> str:
        return f"<|im_start|>user\n{instruct}<|im_end|>\n"

    def _tokenize_texts(self, texts: List[str]) -> List[torch.Tensor]:
        out = []
        for t in texts:
            ids = self.processor(text=t, return_tensors="pt", padding=True)["input_ids"]
            out.append(ids.unsqueeze(0) if ids.dim() == 1 else ids)
        return out

    def _merge_generate_kwargs(self, do_sample=None, top_k=None, top_p=None, temperature=None, repetition_penalty=None,
                               subtalker_dosample=None, subtalker_top_k=None, subtalker_top_p=None,
                               subtalker_temperature=None, max_new_tokens=None, n_requests=None,
                               **kwargs) -> Dict[str, Any]:
        """W:287-352: user value > generation_config.json > hard default.  A user value may be a list with one entry
        per request (TTSModel.generate; also `seed`): checked against n_requests, passed through as it is."""
        hard = dict(do_sample=True, top_k=50, top_p=1.0, temperature=0.9, repetition_penalty=1.05,
                    subtalker_dosample=True, subtalker_top_k=50, subtalker_top_p=1.0, subtalker_temperature=0.9,
                    max_new_tokens=2048)

        def pick(name, v):
            if v is not None:
                return v
            if name in self.generate_defaults:
                return self.generate_defaults[name]
            return hard[name]

        merged = dict(kwargs)
        if n_requests is not None:
            given = dict(do_sample=do_sample, top_k=top_k, top_p=top_p, temperature=temperature,
                         repetition_penalty=repetition_penalty, subtalker_dosample=subtalker_dosample,
                         subtalker_top_k=subtalker_top_k, subtalker_top_p=subtalker_top_p,
                         subtalker_temperature=subtalker_temperature, seed=kwargs.get("seed"))
            for name, v in given.items():
                if isinstance(v, (list, tuple)) and len(v) != n_requests:
                    raise ValueError(f"Batch size mismatch: text={n_requests}, {name}={len(v)}")
        merged.update(do_sample=pick("do_sample", do_sample), top_k=pick("top_k", top_k), top_p=pick("top_p", top_p),
                      temperature=pick("temperature", temperature),
                      repetition_penalty=pick("repetition_penalty", repetition_penalty),
                      subtalker_dosample=pick("subtalker_dosample", subtalker_dosample),
                      subtalker_top_k=pick("subtalker_top_k", subtalker_top_k),
                      subtalker_top_p=pick("subtalker_top_p", subtalker_top_p),
                      subtalker_temperature=pick("subtalker_temperature", subtalker_temperature),
                      max_new_tokens=pick("max_new_tokens", max_new_tokens))
        return merged

    def _decode(self, codes_list, sample_rate=None, pcm_format="f32", cut=None, steps=None):
        return self.model.speech_tokenizer.decode([{"audio_codes": c} for c in codes_list], sample_rate, pcm_format,
                                                  _cut=cut, _steps=steps)

    def _output_format(self, sample_rate, pcm_format):
        """Validate the output format before anything runs; returns the rate the caller will get."""
        tok = self.model.speech_tokenizer
        fmt = _resample.output_format(sample_rate, pcm_format, tok.get_output_sample_rate())
        return tok.get_output_sample_rate() if fmt is None else fmt[0].sample_rate

    # ---------------------------------------------------------------- voice clone (W:356-633)
    def create_voice_clone_prompt(self, ref_audio, ref_text=None, x_vector_only_mode=False) -> List[VoiceClonePromptItem]:
        """W:356-458: reference audio -> ref_code (12 Hz tokenizer encode, HIP) + x-vector (mel + ECAPA, HIP)."""
        if self.model.tts_model_type != "base":
            raise ValueError(f"model with \ntokenizer_type: {self.model.tokenizer_type}\n"
                             f"tts_model_size: {self.model.tts_model_size}\n"
                             f"tts_model_type: {self.model.tts_model_type}\n"
                             "does not support create_voice_clone_prompt, Please check Model Card or Readme for more details.")
        ref_audio_list = self._ensure_list(ref_audio)
        ref_text_list = self._ensure_list(ref_text) if isinstance(ref_text, list) else [ref_text] * len(ref_audio_list)
        xvec_list = self._ensure_list(x_vector_only_mode) if isinstance(x_vector_only_mode, list) else \
            [x_vector_only_mode] * len(ref_audio_list)
        if len(ref_text_list) != len(ref_audio_list) or len(xvec_list) != len(ref_audio_list):
            raise ValueError(f"Batch size mismatch: ref_audio={len(ref_audio_list)}, ref_text={len(ref_text_list)}, "
                             f"x_vector_only_mode={len(xvec_list)}")
        normalized = _audio.normalize_pairs(ref_audio_list)
        srs = [sr for _, sr in normalized]
        tok = self.model.speech_tokenizer
        spk_sr = self.model.speaker_encoder_sample_rate
        for i, (rtext, xvec_only) in enumerate(zip(ref_text_list, xvec_list)):
            if not xvec_only and (rtext is None or rtext == ""):
                raise ValueError(f"ref_text is required when x_vector_only_mode=False (ICL mode). Bad index={i}")
        # x-vectors of all clips (W:434 per clip; equal-length clips share one ECAPA pass here) on a side stream with
        # its own split-K workspace, concurrently with the tokenizer encode on this one (the two front ends are
        # independent; ~1.2 and ~3 ms of GPU work for four 3 s clips).  The encode is issued first: its GPU time
        # outlasts its host launch time, so the x-vector launches that follow land beside queued encoder work.
        dev = torch.device(self.model.device)
        main = torch.cuda.current_stream(dev)
        side = _kernels.side_stream(dev)
        side.wait_stream(main)
        if len(set(srs)) == 1:
            ref_codes = tok.encode([w for w, _ in normalized], sr=srs[0]).audio_codes
        else:
            ref_codes = [tok.encode(w, sr=sr).audio_codes[0] for w, sr in normalized]
        if getattr(self, "_side_ws", None) is None:
            self._side_ws = _kernels.new_workspace(dev)
        with torch.cuda.stream(side), _kernels.use_workspace(self._side_ws):
            spks = self.model.extract_speaker_embeddings(
                [_audio.resample(wav, sr, spk_sr) if sr != spk_sr else wav for wav, sr in normalized], sr=spk_sr)
        main.wait_stream(side)
        spks.record_stream(main)
        items = []
        for i, ((wav, sr), code, rtext, xvec_only) in enumerate(zip(normalized, ref_codes, ref_text_list, xvec_list)):
            spk = spks[i]
            items.append(VoiceClonePromptItem(ref_code=None if xvec_only else code, ref_spk_embedding=spk,
                                              x_vector_only_mode=bool(xvec_only), icl_mode=bool(not xvec_only),
                                              ref_text=rtext))
        return items

    def _prompt_items_to_voice_clone_prompt(self, items: List[VoiceClonePromptItem]) -> Dict[str, Any]:
        return dict(ref_code=[it.ref_code for it in items], ref_spk_embedding=[it.ref_spk_embedding for it in items],
                    x_vector_only_mode=[it.x_vector_only_mode for it in items], icl_mode=[it.icl_mode for it in items])

    @torch.no_grad()
    def generate_voice_clone(self, text, language=None, ref_audio=None, ref_text=None, x_vector_only_mode=False,
                             voice_clone_prompt=None, non_streaming_mode=False, sample_rate=None, pcm_format="f32",
                             speed=None, pitch=None, volume_gain_db=None, **kwargs):
        """speed (not in the reference): the speaking rate, 0.5 to 2.0, a number or one per text -- the
        wavs time-stretched on the device (after the reference's cut, before the resampler and the host copy).
        pitch / volume_gain_db (not in the reference): the pitch in semitones, -12 to 12 (resampling
        pitch: formants move with it), and the gain in dB, -96 to 16 (a positive gain is peak-limited at 1.0), a
        number or one per text, applied on the device between the time-stretch and the resampler."""
        self._output_format(sample_rate, pcm_format)
        input_ids, ref_ids, vcp, languages = self._voice_clone_inputs(text, language, ref_audio, ref_text,
                                                                      x_vector_only_mode, voice_clone_prompt)
        steps = _prosody.steps(speed, pitch, volume_gain_db, len(input_ids))
        codes, _ = self.model.generate(input_ids=input_ids, ref_ids=ref_ids, voice_clone_prompt=vcp, languages=languages,
                                       non_streaming_mode=non_streaming_mode,
                                       **self._merge_generate_kwargs(n_requests=len(input_ids), **kwargs))
        refs = vcp.get("ref_code", None)
        dec = [torch.cat([refs[i].cpu().long(), c], 0) if refs is not None and refs[i] is not None else c
               for i, c in enumerate(codes)]
        if steps is not None or \
                _resample.output_format(sample_rate, pcm_format, self.model.speech_tokenizer.get_output_sample_rate()):
            # the same cut, taken on the device in front of the tempo stage and the resampler
            return self._decode(dec, sample_rate, pcm_format,
                                cut=[(int(refs[i].shape[0]), int(d.shape[0])) if refs is not None and refs[i] is not None
                                     else None for i, d in enumerate(dec)], steps=steps)
        wavs, fs = self._decode(dec)
        out = []
        for i, w in enumerate(wavs):
            if refs is not None and refs[i] is not None:
                cut = int(int(refs[i].shape[0]) / max(int(dec[i].shape[0]), 1) * w.shape[0])
                out.append(w[cut:])
            else:
                out.append(w)
        return out, fs

    @torch.no_grad()
    def stream_voice_clone(self, text, language=None, ref_audio=None, ref_text=None, x_vector_only_mode=False,
                           voice_clone_prompt=None, non_streaming_mode=False, first_chunk_frames=1, chunk_frames=48,
                           sample_rate=None, pcm_format="f32", max_batch=None, voice_cache=None, speed=None,
                           pitch=None, volume_gain_db=None, **kwargs):
        """New surface (no reference counterpart, SURVEY.md §8f-1 + 8f-2): streaming voice clone.  Same inputs as
        generate_voice_clone (reference audio is encoded / x-vectored at submit); yields (utterance index, pcm chunk
        np.float32, sample rate, is_last).  Per utterance the chunks concatenate to generate_voice_clone()'s PCM: in
        ICL mode the reference codes are decoded in front of the generated ones and the output starts at their
        boundary -- the wrapper's proportional cut keeps floor(555 R / T) more samples of the reference's tail, a
        length-dependent point a stream cannot know in advance (TTSModel._stream_stateful).  sample_rate /
        pcm_format / speed / pitch / volume_gain_db: as in stream().  max_batch: with more texts than max_batch, stream
        them by continuous batching through max_batch rows (TTSModel.serve_stream); ICL prompts then need voice_cache, a qwen_tts.VoiceCache that
        keeps each voice's codec state across requests (VoiceCache.warm fills it ahead of the first request)."""
        sr = self._output_format(sample_rate, pcm_format)
        input_ids, ref_ids, vcp, languages = self._voice_clone_inputs(text, language, ref_audio, ref_text,
                                                                      x_vector_only_mode, voice_clone_prompt)
        for i, pcm, last in self.model.stream(input_ids=input_ids, ref_ids=ref_ids, voice_clone_prompt=vcp,
                                              languages=languages, non_streaming_mode=non_streaming_mode,
                                              first_chunk_frames=first_chunk_frames, chunk_frames=chunk_frames,
                                              sample_rate=sample_rate, pcm_format=pcm_format, max_batch=max_batch,
                                              voice_cache=voice_cache, speed=speed, pitch=pitch,
                                              volume_gain_db=volume_gain_db,
                                              **self._merge_generate_kwargs(n_requests=len(input_ids), **kwargs)):
            yield i, (pcm if pcm.dtype == torch.int16 else pcm.to(torch.float32)).cpu().numpy(), sr, last

    def _voice_clone_inputs(self, text, language, ref_audio, ref_text, x_vector_only_mode, voice_clone_prompt):
        """W:460-633 input handling of generate_voice_clone: -> (input_ids, ref_ids, voice_clone_prompt dict,
        languages)."""
        if self.model.tts_model_type != "base":
            raise ValueError(f"model with tts_model_type: {self.model.tts_model_type} does not support "
                             "generate_voice_clone, Please check Model Card or Readme for more details.")
        texts = self._ensure_list(text)
        languages = self._ensure_list(language) if isinstance(language, list) else \
            ([language] * len(texts) if language is not None else ["Auto"] * len(texts))
        if len(languages) == 1 and len(texts) > 1:
            languages = languages * len(texts)
        if len(texts) != len(languages):
            raise ValueError(f"Batch size mismatch: text={len(texts)}, language={len(languages)}")
        self._validate_languages(languages)
        if voice_clone_prompt is None:
            if ref_audio is None:
                raise ValueError("Either `voice_clone_prompt` or `ref_audio` must be provided.")
            items = self.create_voice_clone_prompt(ref_audio, ref_text, x_vector_only_mode)
            if len(items) == 1 and len(texts) > 1:  # one reference voice for a batch of texts (W:567-571)
                items = items * len(texts)
            if len(items) != len(texts):
                raise ValueError(f"Batch size mismatch: prompt={len(items)}, text={len(texts)}")
            vcp, ref_texts = self._prompt_items_to_voice_clone_prompt(items), [it.ref_text for it in items]
        elif isinstance(voice_clone_prompt, list):
            items = voice_clone_prompt
            if len(items) == 1 and len(texts) > 1:
                items = items * len(texts)
            if len(items) != len(texts):
                raise ValueError(f"Batch size mismatch: prompt={len(items)}, text={len(texts)}")
            vcp, ref_texts = self._prompt_items_to_voice_clone_prompt(items), [it.ref_text for it in items]
        else:
            vcp, ref_texts = voice_clone_prompt, None
        input_ids = self._tokenize_texts([self._build_assistant_text(t) for t in texts])
        ref_ids = None
        if ref_texts is not None:
            ref_ids = [None if not rt else self._tokenize_texts([self._build_ref_text(rt)])[0] for rt in ref_texts]
        return input_ids, ref_ids, vcp, languages

    # ---------------------------------------------------------------- voice design (W:637-728)
    @torch.no_grad()
    def generate_voice_design(self, text, instruct, language=None, non_streaming_mode=True, sample_rate=None,
                              pcm_format="f32", prefix_cache=None, speed=None, pitch=None, volume_gain_db=None,
                              **kwargs):
        """prefix_cache (not in the reference): a qwen_tts.PrefixCache that keeps each instruction's talker K/V across
        calls (TTSModel.generate).  speed / pitch / volume_gain_db: as in generate_voice_clone."""
        self._output_format(sample_rate, pcm_format)
        if self.model.tts_model_type != "voice_design":
            raise ValueError(f"model with tts_model_type: {self.model.tts_model_type} does not support "
                             "generate_voice_design, Please check Model Card or Readme for more details.")
        texts = self._ensure_list(text)
        languages = self._ensure_list(language) if isinstance(language, list) else \
            ([language] * len(texts) if language is not None else ["Auto"] * len(texts))
        instructs = self._ensure_list(instruct)
        if len(languages) == 1 and len(texts) > 1:
            languages = languages * len(texts)
        if len(instructs) == 1 and len(texts) > 1:
            instructs = instructs * len(texts)
        if not (len(texts) == len(languages) == len(instructs)):
            raise ValueError(f"Batch size mismatch: text={len(texts)}, language={len(languages)}, "
                             f"instruct={len(instructs)}")
        self._validate_languages(languages)
        input_ids = self._tokenize_texts([self._build_assistant_text(t) for t in texts])
        ins_ids = [None if not x else self._tokenize_texts([self._build_instruct_text(x)])[0] for x in instructs]
        steps = _prosody.steps(speed, pitch, volume_gain_db, len(input_ids))
        codes, _ = self.model.generate(input_ids=input_ids, instruct_ids=ins_ids, languages=languages,
                                       non_streaming_mode=non_streaming_mode, prefix_cache=prefix_cache,
                                       **self._merge_generate_kwargs(n_requests=len(input_ids), **kwargs))
        return self._decode(codes, sample_rate, pcm_format, steps=steps)

    # ---------------------------------------------------------------- custom voice (W:732-839)
    def _custom_voice_inputs(self, text, speaker, language, instruct):
        if self.model.tts_model_type != "custom_voice":
            raise ValueError(f"model with tts_model_type: {self.model.tts_model_type} does not support "
                             "generate_custom_voice, Please check Model Card or Readme for more details.")
        texts = self._ensure_list(text)
        languages = self._ensure_list(language) if isinstance(language, list) else \
            ([language] * len(texts) if language is not None else ["Auto"] * len(texts))
        speakers = self._ensure_list(speaker)
        if self.model.tts_model_size in "0b6":  # W:799 (substring test, kept as-is)
            instruct = None
        instructs = self._ensure_list(instruct) if isinstance(instruct, list) else \
            ([instruct] * len(texts) if instruct is not None else [""] * len(texts))
        if len(languages) == 1 and len(texts) > 1:
            languages = languages * len(texts)
        if len(speakers) == 1 and len(texts) > 1:
            speakers = speakers * len(texts)
        if len(instructs) == 1 and len(texts) > 1:
            instructs = instructs * len(texts)
        if not (len(texts) == len(languages) == len(speakers) == len(instructs)):
            raise ValueError(f"Batch size mismatch: text={len(texts)}, language={len(languages)}, "
                             f"speaker={len(speakers)}, instruct={len(instructs)}")
        self._validate_languages(languages)
        self._validate_speakers(speakers)
        input_ids = self._tokenize_texts([self._build_assistant_text(t) for t in texts])
        ins_ids = [None if not x else self._tokenize_texts([self._build_instruct_text(x)])[0] for x in instructs]
        return input_ids, ins_ids, languages, speakers

    @torch.no_grad()
    def generate_custom_voice(self, text, speaker, language=None, instruct=None, non_streaming_mode=True,
                              sample_rate=None, pcm_format="f32", prefix_cache=None, speed=None, pitch=None,
                              volume_gain_db=None, **kwargs):
        """prefix_cache (not in the reference): as in generate_voice_design; the 0.6B models drop the instruction
        (W:799), so their requests leave the cache untouched.  speed / pitch / volume_gain_db: as in
        generate_voice_clone."""
        self._output_format(sample_rate, pcm_format)
        input_ids, ins_ids, languages, speakers = self._custom_voice_inputs(text, speaker, language, instruct)
        steps = _prosody.steps(speed, pitch, volume_gain_db, len(input_ids))
        codes, _ = self.model.generate(input_ids=input_ids, instruct_ids=ins_ids, languages=languages,
                                       speakers=speakers, non_streaming_mode=non_streaming_mode,
                                       prefix_cache=prefix_cache,
                                       **self._merge_generate_kwargs(n_requests=len(input_ids), **kwargs))
        return self._decode(codes, sample_rate, pcm_format, steps=steps)

    @torch.no_grad()
    def stream(self, text, speaker=None, language=None, instruct=None, non_streaming_mode=None,
               first_chunk_frames=1, chunk_frames=48, left_context=None, max_batch=None, text_feed=None,
               sample_rate=None, pcm_format="f32", prefix_cache=None, speed=None, pitch=None, volume_gain_db=None,
               **kwargs):
        """New surface (no reference counterpart): streaming custom-voice generation.
        Yields (utterance index, pcm chunk np.float32, sample rate, is_last) while the batch decodes: the first
        chunk arrives after prefill + `first_chunk_frames` decode frames (1 frame: 1365 samples = 57 ms of audio,
        which outlasts the ~9 ms the next 2-frame chunk takes), later chunks double in size up to `chunk_frames`
        (each chunk's audio outlasts the generation of the next).  Per utterance the
        chunks concatenate to the one-shot generate_custom_voice() length and equal its PCM up to fp summation order
        (a stateful incremental codec decode; codes are identical -- see TTSModel.stream for the chunk rule and the
        stateless `left_context` form).  max_batch: with more utterances than max_batch, they stream through
        max_batch continuously batched rows instead (TTSModel.serve_stream): a row is refilled with the next
        utterance as soon as its own ends, and every utterance has a first chunk of its own.

        text_feed (a qwen_tts.TextFeed, one row per utterance): the text arrives while the audio is
        generated (make it with self.text_feed(rows, timeout), so that push_text works before the first next()).
        `text` then holds each utterance's first piece (at least one token); later pieces come through
        text_feed.push_text(piece, row) -- or push(ids, row) -- from any thread, and text_feed.close(row) ends an
        utterance's text.  Each piece is tokenized on its own, and piece-wise BPE is not the whole sentence's BPE
        (cut at word boundaries); what is guaranteed is stated on ids: after close, an utterance is decoded exactly
        as the whole id sequence would be in streaming-text mode (non_streaming_mode=False, the only mode here).
        non_streaming_mode defaults to True as in generate_custom_voice(), and to False with a text_feed.

        sample_rate / pcm_format: the chunks at that rate (8000 .. 48000) as np.float32 or, with "s16",
        np.int16, resampled on the device by a stateful filter (qwen_tts.PcmResampler): per utterance they concatenate
        to the resampled whole, ceil(N * rate / 24000) samples for the default's N, whatever the chunking; up to
        10 * max(1, 24000 / rate) input samples' worth of output waits for the next chunk (the last one flushes).

        speed: the speaking rate, 0.5 to 2.0, a number or one per utterance -- the chunks time-stretched
        on the device by a stateful stage (qwen_tts.tempo.PcmTempo) in front of the resampler: per utterance they
        concatenate to the stretched whole, ceil(N / speed) samples, whatever the chunking.

        pitch / volume_gain_db: the pitch in semitones, -12 to 12, and the gain in dB, -96 to 16, a number
        or one per utterance, applied by a stateful device stage (qwen_tts.prosody.PcmProsody) between the two.  Pitch
        is resampling pitch (formants move with it; the duration stays that of `speed`, and speed divided by the pitch
        ratio must lie in [0.5, 2.0]); a positive gain is peak-limited, so no sample leaves above 1.0.

        prefix_cache: a qwen_tts.PrefixCache -- an utterance whose instruction is cached skips that part of its
        prefill (TTSModel.generate)."""
        sr = self._output_format(sample_rate, pcm_format)
        if non_streaming_mode is None:
            non_streaming_mode = text_feed is None
        input_ids, ins_ids, languages, speakers = self._custom_voice_inputs(text, speaker, language, instruct)
        if text_feed is not None:  # heads: role ids + the first piece, no template suffix
            input_ids = self._tokenize_texts([f"<|im_start|>assistant\n{t}" for t in self._ensure_list(text)])
            text_feed.processor = self.processor
        for i, pcm, last in self.model.stream(input_ids=input_ids, instruct_ids=ins_ids, languages=languages,
                                              speakers=speakers, non_streaming_mode=non_streaming_mode,
                                              first_chunk_frames=first_chunk_frames, chunk_frames=chunk_frames,
                                              left_context=left_context, max_batch=max_batch, text_feed=text_feed,
                                              sample_rate=sample_rate, pcm_format=pcm_format,
                                              prefix_cache=prefix_cache, speed=speed, pitch=pitch,
                                              volume_gain_db=volume_gain_db,
                                              **self._merge_generate_kwargs(n_requests=len(input_ids), **kwargs)):
            yield i, (pcm if pcm.dtype == torch.int16 else pcm.to(torch.float32)).cpu().numpy(), sr, last

    def text_feed(self, rows: int = 1, timeout: float = 30.0):
        """A qwen_tts.TextFeed for stream(text_feed=...) whose push_text tokenizes with this model's processor (usable
        at once: stream() is a generator and binds the processor of a plain TextFeed only at its first next())."""
        from ..feed import TextFeed
        feed = TextFeed(rows=rows, timeout=timeout)
        feed.processor = self.processor
        return feed

    def request_queue(self, timeout: float = 30.0):
        """A qwen_tts.RequestQueue for serve_live() that also takes strings:
        submit(text=..., instruct=..., language=..., speaker=..., open_text=False, speed=None, pitch=None,
        volume_gain_db=None, **sampling) tokenizes as stream()
        does (with open_text, `text` is the first piece and the rest follows through push_text / close_text), and
        fills the sampling parameters a request leaves out from generation_config.json.  non_streaming_mode defaults
        to True as in generate_custom_voice(), and to False with open_text."""
        return _TextRequestQueue(self, timeout)

    @torch.no_grad()
    def serve_live(self, queue, max_batch=8, max_prompt=512, first_chunk_frames=1, chunk_frames=8, sample_rate=None,
                   pcm_format="f32", prefix_cache=None, max_new_tokens=None, **kwargs):
        """New surface (no reference counterpart): serve the requests of `queue` (self.request_queue()) as they
        arrive, through max_batch continuously batched rows (TTSModel.serve_live).  Yields (request id, pcm chunk
        np.float32 -- np.int16 with pcm_format="s16" --, sample rate, is_last) until the queue is closed and every
        request is over.  kwargs: eos_token_id, ignore_eos, seed, use_graph."""
        sr = self._output_format(sample_rate, pcm_format)
        if self.model.tts_model_type != "custom_voice":
            raise ValueError(f"model with tts_model_type: {self.model.tts_model_type} does not support serve_live")
        mnt = self._merge_generate_kwargs(max_new_tokens=max_new_tokens)["max_new_tokens"]
        for i, pcm, last in self.model.serve_live(queue, max_batch=max_batch, max_prompt=max_prompt,
                                                  max_new_tokens=mnt, first_chunk_frames=first_chunk_frames,
                                                  chunk_frames=chunk_frames, sample_rate=sample_rate,
                                                  pcm_format=pcm_format, prefix_cache=prefix_cache, **kwargs):
            yield i, (pcm if pcm.dtype == torch.int16 else pcm.to(torch.float32)).cpu().numpy(), sr, last

    def get_supported_speakers(self) -> Optional[List[str]]:
        s = self._supported_speakers_set()
        return None if s is None else sorted(s)

    def get_supported_languages(self) -> Optional[List[str]]:
        s = self._supported_languages_set()
        return None if s is None else sorted(s)
