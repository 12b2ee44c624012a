"""The pitch and volume stage on the routes: `pitch` and `volume_gain_db` of TTSModel.stream /
serve_stream / the text_feed route / serve_live (RequestQueue.submit) and the generate_* wrappers.  Tiny preset in
fp32; the model recipes are those of test_gpu_stream_speed.py.

Every stage is chunk-invariant bit for bit, so every check is an equality: a row's or request's chunks concatenate to
the device one-shot chain -- PcmTempo.one_shot at T, PcmProsody.one_shot at T/S and the gain, cut to ceil(100 N / S),
then PcmResampler.one_shot for another format -- of the default stream's concatenation for it, and a request at 0 / 0
keeps the default's bits.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F32 = torch.float32


def _serve_case():  # the recipe of test_continuous_batching_matches_one_shot
    return dict(texts=[7, 3, 10, 5, 12, 4], languages=["auto", "english", "japanese", "chinese", "english", "auto"],
                speakers=["vivian", None, "dylan", "eric", "ryan", ""], non_streaming_mode=False, max_new_tokens=40)


@pytest.fixture(scope="module")
def models():
    """(config, model whose EOS row is the donor's so that requests end raggedly, plain model)"""
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
    return cfg, ragged, plain


def _kw(cfg, n=6, **over):
    from cases import make_inputs
    case = _serve_case()
    ids, _, _, _ = make_inputs(case, 11, cfg["talker_config"]["hidden_size"])
    kw = dict(input_ids=ids[:n], languages=case["languages"][:n], speakers=case["speakers"][:n],
              non_streaming_mode=False, max_new_tokens=case["max_new_tokens"], seed=7, do_sample=False,
              subtalker_dosample=False)
    kw.update(over)
    return kw


def _collect(stream, n):
    chunks, lasts = {}, {}
    for i, pcm, last in stream:
        assert i not in lasts, (i, "a chunk after last=True")
        chunks.setdefault(i, []).append(pcm.clone())
        if last:
            lasts[i] = True
    assert sorted(chunks) == list(range(n)) and sorted(lasts) == list(range(n))  # one last=True each, and it came last
    return {i: torch.cat(c) for i, c in chunks.items()}


def _same_bits(a, b):
    view = torch.int32 if a.dtype == F32 else torch.int16
    return a.dtype == b.dtype and a.shape == b.shape and \
        torch.equal(a.contiguous().view(view), b.contiguous().view(view))


def _chain(x, step, fmt=None):
    """The device one-shot chain of a request's default samples x at step = (S, T, db)"""
    from qwen_tts import PcmResampler, PcmTempo
    from qwen_tts import tempo as T_
    from qwen_tts.prosody import PcmProsody
    S, T, db = step
    y = x if T == 100 else PcmTempo(1, device=x.device).one_shot(x, T)
    if (T, db) != (S, 0.0):
        y = PcmProsody(1, device=x.device).one_shot(y, T, S, db, cap=T_.out_len(x.numel(), S))
    assert y.numel() == T_.out_len(x.numel(), S)
    if fmt is not None:
        y = PcmResampler(1, fmt[0], fmt[1], device=x.device).one_shot(y)
    return y


_DEFAULT = {}


def _default(model, cfg, key):
    """The default streams' concatenations, computed once: "stream" (3 rows, one batch) and "serve" (6 requests
    through 2 rows)."""
    if key not in _DEFAULT:
        if key == "stream":
            _DEFAULT[key] = _collect(model.stream(**_kw(cfg, 3), first_chunk_frames=1, chunk_frames=8), 3)
        else:
            _DEFAULT[key] = _collect(model.serve_stream(**_kw(cfg, 6), max_batch=2, first_chunk_frames=1,
                                                        chunk_frames=8), 6)
    return _DEFAULT[key]


def test_stream_per_request(models):
    from qwen_tts import prosody as P
    from qwen_tts import tempo as T_
    cfg, model, _ = models
    base = _default(model, cfg, "stream")
    assert len({v.numel() for v in base.values()}) > 1  # EOS-ragged
    speed, pitch, db = [1.0, 1.25, 0.8], [0, 3, -4], [0, 6, -6]
    steps = P.steps(speed, pitch, db, 3)
    assert steps == [(100, 100, 0.0), (125, 105, 6.0), (80, 101, -6.0)]
    got = _collect(model.stream(**_kw(cfg, 3), first_chunk_frames=1, chunk_frames=8, speed=speed, pitch=pitch,
                                volume_gain_db=db), 3)
    assert _same_bits(got[0], base[0])  # the request at 0 / 0 keeps the default's bits
    for b in range(3):
        assert got[b].numel() == T_.out_len(base[b].numel(), steps[b][0])
        assert _same_bits(got[b], _chain(base[b], steps[b])), b
    assert float(got[1].abs().max()) <= 1.0
    # and in front of the resampler
    got = _collect(model.stream(**_kw(cfg, 3), first_chunk_frames=1, chunk_frames=8, speed=speed, pitch=pitch,
                                volume_gain_db=db, sample_rate=16000, pcm_format="s16"), 3)
    for b in range(3):
        assert _same_bits(got[b], _chain(base[b], steps[b], (16000, "s16"))), b


def test_serve_stream_slot_reuse(models):
    """6 requests through 2 slots: a slot's state is reset, and takes the new request's ratio and gain"""
    from qwen_tts import prosody as P
    cfg, model, _ = models
    base = _default(model, cfg, "serve")
    assert len({v.numel() for v in base.values()}) > 1
    speed, pitch, db = [1.0, 0.8, 1.0, 1.5, 1.0, 0.7], [0, 5, -12, 0, 12, -2.5], [0, 0, 6, -20, 0, 16]
    steps = P.steps(speed, pitch, db, 6)
    got = _collect(model.serve_stream(**_kw(cfg, 6), max_batch=2, first_chunk_frames=1, chunk_frames=8, speed=speed,
                                      pitch=pitch, volume_gain_db=db), 6)
    for i in range(6):
        assert _same_bits(got[i], _chain(base[i], steps[i])), i
    assert _same_bits(got[0], base[0])
    # and through the public switch of stream(), with speed left out
    got = _collect(model.stream(**_kw(cfg, 6), max_batch=2, pitch=pitch, volume_gain_db=3.0), 6)
    for i, st in enumerate(P.steps(None, pitch, 3.0, 6)):
        assert _same_bits(got[i], _chain(base[i], st)), i


def test_all_defaults_build_no_stage(models, monkeypatch):
    from qwen_tts import PcmResampler
    cfg, model, _ = models
    base = _default(model, cfg, "stream")
    built = []
    stage = model._output_stage
    monkeypatch.setattr(model, "_output_stage", lambda *a: built.append(stage(*a)) or built[-1])
    got = _collect(model.stream(**_kw(cfg, 3), first_chunk_frames=1, chunk_frames=8, speed=[1.0] * 3, pitch=[0, 0.0, 0],
                                volume_gain_db=0), 3)
    assert built == [None]
    for b in range(3):
        assert _same_bits(got[b], base[b])
    _collect(model.stream(**_kw(cfg, 3), first_chunk_frames=1, chunk_frames=8, pitch=0, volume_gain_db=[0, 0, 0],
                          sample_rate=16000), 3)
    assert type(built[1]) is PcmResampler


def test_text_feed_route(models):
    from cases import text_ids
    from qwen_tts import TextFeed
    cfg, _, model = models
    ids = text_ids(9, 5)[0].tolist()
    kw = dict(languages=["auto"], speakers=[""], non_streaming_mode=False, max_new_tokens=12, do_sample=False,
              subtalker_dosample=False)
    out = []
    for over in ({}, dict(pitch=-3, volume_gain_db=4.5, speed=0.93)):
        feed = TextFeed(rows=1, timeout=5.0)
        feed.push(ids[4:-5], row=0)
        feed.close(row=0)
        out.append(_collect(model.stream(input_ids=[torch.tensor([ids[:4]])], text_feed=feed, **over, **kw), 1)[0])
    assert out[0].numel() > 0 and _same_bits(out[1], _chain(out[0], (93, 111, 4.5)))


def test_serve_live_submit(models):
    from qwen_tts import RequestQueue
    from qwen_tts import prosody as P
    cfg, model, _ = models
    kw = _kw(cfg, 3)
    vals = ((1.5, 2, None), (None, None, None), (None, -7, 6))
    out = []
    for use in (False, True):
        q = RequestQueue(timeout=5.0)
        for i in range(3):
            extra = dict(zip(("speed", "pitch", "volume_gain_db"), vals[i])) if use else {}
            q.submit(kw["input_ids"][i], language=kw["languages"][i], speaker=kw["speakers"][i],
                     non_streaming_mode=False, do_sample=False, subtalker_dosample=False, seed=7, **extra)
        q.close()
        out.append(_collect(model.serve_live(q, max_batch=2, max_new_tokens=kw["max_new_tokens"],
                                             first_chunk_frames=1, chunk_frames=8), 3))
    for i, (s, p, d) in enumerate(vals):
        st = (P.steps(s, p, d, 1) or [(100, 100, 0.0)])[0]
        assert out[0][i].numel() > 0 and _same_bits(out[1][i], _chain(out[0][i], st)), i
    for bad in (dict(pitch=13), dict(volume_gain_db=17), dict(pitch=True), dict(speed=0.5, pitch=2)):
        with pytest.raises(ValueError):
            RequestQueue().submit(kw["input_ids"][0], **bad)


def test_refusals(models):
    cfg, model, _ = models
    for over in (dict(pitch=2), dict(volume_gain_db=-3)):
        with pytest.raises(NotImplementedError, match="pitch"):
            next(iter(model.stream(**_kw(cfg, 2), left_context=100, **over)))
    for over in (dict(pitch=12.5), dict(volume_gain_db=float("nan")), dict(volume_gain_db=16.5), dict(pitch="up")):
        with pytest.raises(ValueError):
            next(iter(model.stream(**_kw(cfg, 2), **over)))
    with pytest.raises(ValueError, match=r"speed divided by the pitch ratio must lie in \[0.5, 2.0\]"):
        next(iter(model.stream(**_kw(cfg, 2), speed=1.9, pitch=-2)))
    with pytest.raises(ValueError, match="entries"):
        next(iter(model.serve_stream(**_kw(cfg, 3), max_batch=2, pitch=[1.0, 2.0])))


def _wrapper(preset):
    """Qwen3TTSModel on the oracle's seeded weights (the recipe of test_gpu_stream_format.py)"""
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
    over = dict(speed=[1.25, 1.0], pitch=[4, 0], volume_gain_db=[6, -3])
    base, _ = tts.generate_custom_voice(**kw)
    got, sr = tts.generate_custom_voice(**kw, **over, sample_rate=16000, pcm_format="s16")
    assert sr == 16000 and len(got) == 2
    for b, st in enumerate([(125, 99, 6.0), (100, 100, -3.0)]):
        want = _chain(torch.from_numpy(base[b]).cuda(), st, (16000, "s16")).cpu().numpy()
        assert got[b].dtype == np.int16 and np.array_equal(got[b], want), b
    # the streaming wrapper hands out numpy chunks that add up to the same lengths
    n = [0, 0]
    for i, pcm, rate, last in tts.stream(**kw, **over, sample_rate=16000, pcm_format="s16"):
        assert pcm.dtype == np.int16 and rate == 16000
        n[i] += pcm.shape[0]
    assert n == [g.shape[0] for g in got]
    with pytest.raises(ValueError, match="pitch"):
        tts.generate_custom_voice(**kw, pitch=float("inf"))
    with pytest.raises(TypeError):
        tts.model.speech_tokenizer.decode([], pitch=1)  # the tokenizer's decode does not take them


def test_generate_voice_clone():
    """ICL mode: the chain runs after the cut of the reference's samples; streamed, on the default stream's samples"""
    from cases import ref_audio
    tts = _wrapper("tiny-base")
    items = tts.create_voice_clone_prompt(ref_audio=(ref_audio(31234, 5), 24000), ref_text="Okay. Yeah. I resent you.")
    kw = dict(text="Good one. Okay, fine.", language="Auto", voice_clone_prompt=items, do_sample=False,
              subtalker_dosample=False, max_new_tokens=10)
    over, st = dict(pitch=-5, volume_gain_db=9), (100, 133, 9.0)
    base, _ = tts.generate_voice_clone(**kw)
    got, sr = tts.generate_voice_clone(**kw, **over, sample_rate=16000, pcm_format="s16")
    assert sr == 16000 and len(got) == len(base) == 1
    want = _chain(torch.from_numpy(base[0]).cuda(), st, (16000, "s16")).cpu().numpy()
    assert got[0].dtype == np.int16 and np.array_equal(got[0], want)
    plain = np.concatenate([pcm for _, pcm, _, _ in tts.stream_voice_clone(**kw)])
    chunks = [pcm for _, pcm, _, _ in tts.stream_voice_clone(**kw, **over, sample_rate=16000, pcm_format="s16")]
    want = _chain(torch.from_numpy(plain).cuda(), st, (16000, "s16")).cpu().numpy()
    assert np.array_equal(np.concatenate(chunks), want)
