"""The PCM output stage on the streaming routes and the one-shot decode: `sample_rate` / `pcm_format` of
TTSModel.stream / serve_stream / the text_feed route, Qwen3TTSTokenizer.decode and the generate_* wrappers.  Tiny
preset in fp32; the model recipes are those of test_gpu_serve_stream.py.

Per row or request the chunks concatenate to ceil(N * up / down) samples (N = the one-shot decode's length) and agree
with the fp64 resample (tests/resample_refs.py) of the one-shot wav within
    2e-4 * max over phases of sum |h_phase|  +  the unit test's bound (small_kernel_refs.fp32_tolerance),
2e-4 being the project's stream-versus-one-shot bound and the L1 gain how far the filter can amplify that difference;
for s16 that tolerance times 32767, rounded up, plus 1.

measured on the MI355X: stream 16000/f32 max |diff| 4.3e-7 (allowed 3.6e-4), text_feed 48000/f32 5.4e-7 (4.5e-4), every
s16 case at most 1 of int16 (allowed 13).
"""
import math
import os

import numpy as np
import pytest
import torch

import resample_refs as RR
import small_kernel_refs as R

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F32, F64 = torch.float32, torch.float64


def _serve_case():  # the recipe of test_continuous_batching_matches_one_shot
    return dict(texts=[7, 3, 10, 5, 12, 4], languages=["auto", "english", "japanese", "chinese", "english", "auto"],
                speakers=["vivian", None, "dylan", "eric", "ryan", ""], non_streaming_mode=False, max_new_tokens=40)


@pytest.fixture(scope="module")
def models():
    """(config, model whose EOS row is the donor's so that requests end raggedly, plain model, tokenizer)"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from oracle import codec_param_specs, load_preset, synth_state_dict, talker_param_specs
    from qwen_tts import Qwen3TTSTokenizer
    from qwen_tts.model import TTSModel
    cfg, ccfg = load_preset("tiny-customvoice")
    W = {k: torch.from_numpy(v) for k, v in synth_state_dict(talker_param_specs(cfg)).items()}
    CW = {k: torch.from_numpy(v) for k, v in synth_state_dict(codec_param_specs(ccfg)).items()}
    tok = Qwen3TTSTokenizer.from_pretrained("synthetic:tiny-customvoice/speech_tokenizer", dtype="fp32", weights=CW)
    plain = TTSModel(cfg, W, dtype="fp32")
    z = np.load(os.path.join(GOLD, "tiny_talker.npz"))
    We = dict(W)
    head = W["talker.codec_head.weight"].clone()
    head[cfg["talker_config"]["codec_eos_token_id"]] = head[int(z["eos_b2/donor"])]
    We["talker.codec_head.weight"] = head
    ragged = TTSModel(cfg, We, dtype="fp32")
    for m in (plain, ragged):
        m.load_speech_tokenizer(tok)
    return cfg, ragged, plain, tok


def _kw(cfg, n=6, **over):
    from cases import make_inputs
    case = _serve_case()
    ids, _, _, _ = make_inputs(case, 11, cfg["talker_config"]["hidden_size"])
    kw = dict(input_ids=ids[:n], languages=case["languages"][:n], speakers=case["speakers"][:n],
              non_streaming_mode=False, max_new_tokens=case["max_new_tokens"], seed=7, do_sample=False,
              subtalker_dosample=False)
    kw.update(over)
    return kw


_REF = {}


def _reference(model, tok, n, mb):
    """generate()'s codes of the first n requests and their one-shot decode, computed once per key: as one batch for
    stream() (a shorter row's tail is decoded beside the longer rows' frames), each request alone for serve_stream"""
    if (n, mb) not in _REF:
        codes, _ = model.generate(**_kw(model.config, n), max_batch=mb)
        _REF[n, mb] = (codes, tok.decode([{"audio_codes": c} for c in codes])[0] if mb is None else
                       [tok.decode([{"audio_codes": c}])[0][0] for c in codes])
    return _REF[n, mb]


def _collect(stream, n):
    chunks, lasts = {}, {}
    for i, pcm, last in stream:
        assert i not in lasts, (i, "a chunk after last=True")
        chunks.setdefault(i, []).append(pcm.cpu())
        if last:
            lasts[i] = True
    assert sorted(chunks) == list(range(n)) and sorted(lasts) == list(range(n))  # one last=True each, and it came last
    return chunks


def _judge(got, wav, rate, fmt, what):
    """got: the concatenated chunks of one request; wav: its one-shot 24 kHz decode (numpy fp32)"""
    from qwen_tts.resample import plan
    p = plan(rate)
    x = torch.from_numpy(wav)
    ref = RR.resample(x, p)
    assert got.shape == ref.shape == (p.out_len(wav.shape[0]),), (what, got.shape, ref.shape)
    assert got.dtype == (torch.int16 if fmt == "s16" else F32)
    if not ref.numel():
        return
    unit, _ = R.fp32_tolerance(RR.resample(x, p, F32), ref, RR.resample_scale(x, p))
    tol = 2e-4 * RR.l1_gain(p) + unit
    if fmt == "s16":
        d = int((got.to(torch.int64) - RR.s16(ref).to(torch.int64)).abs().max())
        cap = math.ceil(float(tol.max()) * 32767) + 1
        print(f"{what}: {got.numel()} samples, max |diff| {d} of int16, allowed {cap}")
        assert d <= cap, what
    else:
        d = (got.to(F64) - ref).abs()
        print(f"{what}: {got.numel()} samples, max |diff| {float(d.max()):.3g}, allowed {float(tol.min()):.3g}")
        assert bool((d <= tol).all()), what


@pytest.mark.parametrize("rate,fmt", [(16000, "f32"), (8000, "s16")])
def test_stream(models, rate, fmt):
    cfg, model, _, tok = models
    codes, wavs = _reference(model, tok, 2, None)
    chunks = _collect(model.stream(**_kw(cfg, 2), first_chunk_frames=1, chunk_frames=8, sample_rate=rate,
                                   pcm_format=fmt), 2)
    for b in range(2):
        _judge(torch.cat(chunks[b]), wavs[b], rate, fmt, f"stream {rate}/{fmt} row {b}")
    # the first packet is the emission rule's share of the first frame's 1365 samples
    if codes[0].shape[0] > 1:
        assert chunks[0][0].numel() == RR.FIRST_PACKET[rate]


def test_serve_stream(models):
    cfg, model, _, tok = models
    codes, wavs = _reference(model, tok, 6, 2)
    assert len({c.shape[0] for c in codes}) > 1  # EOS-ragged
    chunks = _collect(model.serve_stream(**_kw(cfg), max_batch=2, first_chunk_frames=1, chunk_frames=8,
                                         sample_rate=16000, pcm_format="s16"), 6)
    for i in range(6):
        _judge(torch.cat(chunks[i]), wavs[i], 16000, "s16", f"serve_stream request {i}")
    # and through the public switch of stream()
    chunks = _collect(model.stream(**_kw(cfg), max_batch=2, sample_rate=16000, pcm_format="s16"), 6)
    for i in range(6):
        _judge(torch.cat(chunks[i]), wavs[i], 16000, "s16", f"stream(max_batch=2) request {i}")


def test_text_feed_route(models):
    from cases import text_ids
    from qwen_tts import TextFeed
    cfg, _, model, tok = models
    ids = text_ids(9, 5)[0].tolist()
    kw = dict(languages=["auto"], speakers=[""], non_streaming_mode=False, max_new_tokens=12, do_sample=False,
              subtalker_dosample=False)
    codes, _ = model.generate(input_ids=[torch.tensor([ids])], **kw)
    wav = tok.decode([{"audio_codes": codes[0]}])[0][0]
    feed = TextFeed(rows=1, timeout=5.0)
    feed.push(ids[4:-5], row=0)
    feed.close(row=0)
    chunks = _collect(model.stream(input_ids=[torch.tensor([ids[:4]])], text_feed=feed, sample_rate=48000, **kw), 1)
    _judge(torch.cat(chunks[0]), wav, 48000, "f32", "text_feed 48000/f32")


def test_defaults_are_the_default_path(models):
    cfg, model, _, tok = models
    a = _collect(model.stream(**_kw(cfg, 2), chunk_frames=8), 2)
    b = _collect(model.stream(**_kw(cfg, 2), chunk_frames=8, sample_rate=None, pcm_format="f32"), 2)
    c = _collect(model.stream(**_kw(cfg, 2), chunk_frames=8, sample_rate=24000), 2)
    for r in range(2):
        for other in (b, c):
            assert [(x.dtype, x.shape) for x in a[r]] == [(x.dtype, x.shape) for x in other[r]]


def test_refusals(models):
    cfg, model, _, tok = models
    with pytest.raises(NotImplementedError, match="stateful"):
        next(iter(model.stream(**_kw(cfg, 2), left_context=100, sample_rate=16000)))
    with pytest.raises(ValueError, match="147/320"):
        next(iter(model.stream(**_kw(cfg, 2), sample_rate=11025)))
    with pytest.raises(ValueError, match="pcm_format"):
        next(iter(model.serve_stream(**_kw(cfg, 2), max_batch=1, pcm_format="u8")))
    with pytest.raises(ValueError, match="pcm_format"):
        tok.decode([{"audio_codes": torch.zeros(2, 16, dtype=torch.long)}], pcm_format="u8")
    torch.cuda.synchronize()
    dec = tok.model
    pools = list(dec._slots.values()) + list(getattr(dec, "_row_slots", {}).values())
    assert not any(sl.busy for pool in pools for sl in pool)  # refused before any pooled codec slot was taken


def _one_shot(wavs, rate, fmt):
    from qwen_tts import PcmResampler
    rs = PcmResampler(1, rate, fmt, device="cuda:0")
    return [rs.one_shot(torch.from_numpy(w).cuda()).cpu().numpy() for w in wavs]


def test_tokenizer_decode(models):
    cfg, model, _, tok = models
    codes, _ = _reference(model, tok, 2, None)
    enc = [{"audio_codes": c} for c in codes]
    base, sr0 = tok.decode(enc)
    got, sr = tok.decode(enc, sample_rate=16000, pcm_format="s16")
    assert sr0 == 24000 and sr == 16000 and len(got) == len(base)
    for g, w in zip(got, _one_shot(base, 16000, "s16")):
        assert g.dtype == np.int16 and np.array_equal(g, w)
    got, sr = tok.decode(enc, sample_rate=44100)
    assert sr == 44100
    for g, w, b in zip(got, _one_shot(base, 44100, "f32"), base):
        assert g.dtype == np.float32 and g.shape == (-(-b.shape[0] * 147 // 80),) and np.array_equal(g, w)


def _wrapper(preset):
    """Qwen3TTSModel on the oracle's seeded weights (the recipe of test_gpu_examples.py)"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from oracle import codec_param_specs, load_preset, synth_state_dict, talker_param_specs
    from oracle.encoder import encoder_param_specs
    from oracle.speaker import speaker_param_specs
    from qwen_tts import Qwen3TTSModel
    cfg, ccfg = load_preset(preset)
    Wn = synth_state_dict(talker_param_specs(cfg) + (speaker_param_specs(cfg) if cfg.get("tts_model_type") == "base"
                                                       else []))
    CWn = synth_state_dict(codec_param_specs(ccfg) + encoder_param_specs(ccfg))
    return Qwen3TTSModel.from_pretrained(f"synthetic:{preset}", dtype=torch.float32,
                                         weights={k: torch.from_numpy(v) for k, v in Wn.items()},
                                         codec_weights={k: torch.from_numpy(v) for k, v in CWn.items()})


def test_generate_custom_voice():
    tts = _wrapper("tiny-customvoice")
    kw = dict(text=["She said she would be here by noon.", "No."], language="English", speaker=["Vivian", "Ryan"],
              do_sample=False, subtalker_dosample=False, max_new_tokens=10)
    base, sr0 = tts.generate_custom_voice(**kw)
    got, sr = tts.generate_custom_voice(**kw, sample_rate=16000, pcm_format="s16")
    assert sr0 == 24000 and sr == 16000
    for g, w in zip(got, _one_shot(base, 16000, "s16")):
        assert g.dtype == np.int16 and np.array_equal(g, w)
    with pytest.raises(ValueError, match="pcm_format"):
        tts.generate_custom_voice(**kw, pcm_format="u8")
    # the streaming wrapper hands out numpy chunks in the format, with the requested rate
    n = [0, 0]
    for i, pcm, rate, last in tts.stream(**kw, sample_rate=16000, pcm_format="s16"):
        assert pcm.dtype == np.int16 and rate == 16000
        n[i] += pcm.shape[0]
    assert n == [g.shape[0] for g in got]


def test_voice_clone():
    """ICL mode: the reference codes are decoded in front of the generated ones and cut off before the resampler."""
    from cases import ref_audio
    tts = _wrapper("tiny-base")
    items = tts.create_voice_clone_prompt(ref_audio=(ref_audio(31234, 5), 24000), ref_text="Okay. Yeah. I resent you.")
    kw = dict(text="Good one. Okay, fine.", language="Auto", voice_clone_prompt=items, do_sample=False,
              subtalker_dosample=False, max_new_tokens=10)
    base, _ = tts.generate_voice_clone(**kw)
    got, sr = tts.generate_voice_clone(**kw, sample_rate=16000, pcm_format="s16")
    assert sr == 16000 and len(got) == len(base) == 1
    assert got[0].dtype == np.int16 and np.array_equal(got[0], _one_shot(base, 16000, "s16")[0])
    # streamed: the default stream's samples, resampled (the stream starts at the reference / generated boundary)
    plain = np.concatenate([pcm for _, pcm, _, _ in tts.stream_voice_clone(**kw)])
    chunks = []
    for i, pcm, rate, last in tts.stream_voice_clone(**kw, sample_rate=16000, pcm_format="s16"):
        assert i == 0 and pcm.dtype == np.int16 and rate == 16000
        chunks.append(pcm)
    assert last
    _judge(torch.from_numpy(np.concatenate(chunks)), plain, 16000, "s16", "stream_voice_clone 16000/s16")
