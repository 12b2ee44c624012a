"""The speaking-rate stage on the routes: `speed` of TTSModel.stream / serve_stream / the text_feed route
/ serve_live (RequestQueue.submit) and the generate_* wrappers.  Tiny preset in fp32; the model recipes are those of
test_gpu_stream_format.py.

The stage is chunk-invariant bit for bit, so every check is an equality: a row's or request's chunks concatenate to
PcmTempo.one_shot of the default stream's concatenation for it (then PcmResampler.one_shot for another format), and a
request at 1.0 keeps the default's bits.
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


def _stretched(x, S):
    from qwen_tts import PcmTempo
    return x if S == 100 else PcmTempo(1, device=x.device).one_shot(x, S)


_DEFAULT = {}


def _default(model, cfg, key):
    """The default streams' concatenations, computed once: "stream" (2 rows, one batch) and "serve" (5 requests
    through 2 rows)."""
    if key not in _DEFAULT:
        if key == "stream":
            _DEFAULT[key] = _collect(model.stream(**_kw(cfg, 2), first_chunk_frames=1, chunk_frames=8), 2)
        else:
            _DEFAULT[key] = _collect(model.serve_stream(**_kw(cfg, 5), max_batch=2, first_chunk_frames=1,
                                                        chunk_frames=8), 5)
    return _DEFAULT[key]


def test_stream(models):
    from qwen_tts import tempo as T
    cfg, model, _ = models
    base = _default(model, cfg, "stream")
    assert base[0].numel() != base[1].numel()  # EOS-ragged
    first = []
    got = {}
    for i, pcm, last in model.stream(**_kw(cfg, 2), first_chunk_frames=1, chunk_frames=8, speed=1.25):
        if i == 0 and not first:
            first.append(pcm.numel())
        got.setdefault(i, []).append(pcm.clone())
    for b in range(2):
        y = torch.cat(got[b])
        assert y.numel() == T.out_len(base[b].numel(), 125)
        assert _same_bits(y, _stretched(base[b], 125)), b
    if base[0].numel() > 1365:  # the first packet is the emission rule's share of the first frame's 1365 samples
        assert first == [T.ready(125, 1365)] == [720]


def test_serve_stream_per_request_speeds(models):
    from qwen_tts import tempo as T
    cfg, model, _ = models
    base = _default(model, cfg, "serve")
    assert len({v.numel() for v in base.values()}) > 1
    speeds = [1.0, 0.8, 1.5, 2.0, 0.5]
    got = _collect(model.serve_stream(**_kw(cfg, 5), max_batch=2, first_chunk_frames=1, chunk_frames=8,
                                      speed=speeds), 5)
    for i, S in enumerate(T.speed_steps(speeds, 5)):
        assert _same_bits(got[i], _stretched(base[i], S)), i
    assert _same_bits(got[0], base[0])  # the request at 1.0 keeps the default's bits
    # and through the public switch of stream()
    got = _collect(model.stream(**_kw(cfg, 5), max_batch=2, speed=speeds), 5)
    for i, S in enumerate(T.speed_steps(speeds, 5)):
        assert _same_bits(got[i], _stretched(base[i], S)), i


def test_speed_then_resampler(models):
    from qwen_tts import PcmResampler
    cfg, model, _ = models
    base = _default(model, cfg, "stream")
    got = _collect(model.stream(**_kw(cfg, 2), first_chunk_frames=1, chunk_frames=8, speed=[0.8, 1.25],
                                sample_rate=16000, pcm_format="s16"), 2)
    rs = PcmResampler(1, 16000, "s16", device="cuda:0")
    for b, S in enumerate((80, 125)):
        assert got[b].dtype == torch.int16
        assert _same_bits(got[b], rs.one_shot(_stretched(base[b], S))), b


def test_all_ones_build_no_stage(models):
    cfg, model, _ = models
    base = _default(model, cfg, "stream")
    got = _collect(model.stream(**_kw(cfg, 2), first_chunk_frames=1, chunk_frames=8, speed=[1.0, 1.0]), 2)
    for b in range(2):
        assert _same_bits(got[b], base[b])


def test_text_feed_route(models):
    from cases import text_ids
    from qwen_tts import TextFeed
    cfg, _, model = models
    ids = text_ids(9, 5)[0].tolist()
    kw = dict(languages=["auto"], speakers=[""], non_streaming_mode=False, max_new_tokens=12, do_sample=False,
              subtalker_dosample=False)
    out = []
    for speed in (None, 0.93):
        feed = TextFeed(rows=1, timeout=5.0)
        feed.push(ids[4:-5], row=0)
        feed.close(row=0)
        out.append(_collect(model.stream(input_ids=[torch.tensor([ids[:4]])], text_feed=feed, speed=speed, **kw), 1)[0])
    assert out[0].numel() > 0 and _same_bits(out[1], _stretched(out[0], 93))


def test_serve_live_submit_speed(models):
    from qwen_tts import RequestQueue
    cfg, model, _ = models
    kw = _kw(cfg, 3)
    out = []
    for speeds in ((None, None, None), (1.5, None, 0.5)):
        q = RequestQueue(timeout=5.0)
        for i in range(3):
            q.submit(kw["input_ids"][i], language=kw["languages"][i], speaker=kw["speakers"][i],
                     non_streaming_mode=False, do_sample=False, subtalker_dosample=False, seed=7, speed=speeds[i])
        q.close()
        out.append(_collect(model.serve_live(q, max_batch=2, max_new_tokens=kw["max_new_tokens"],
                                             first_chunk_frames=1, chunk_frames=8), 3))
    for i, S in enumerate((150, 100, 50)):
        assert out[0][i].numel() > 0 and _same_bits(out[1][i], _stretched(out[0][i], S)), i
    with pytest.raises(ValueError, match="speed"):
        RequestQueue().submit(kw["input_ids"][0], speed=3.0)


def test_refusals(models):
    cfg, model, _ = models
    with pytest.raises(NotImplementedError, match="speed"):
        next(iter(model.stream(**_kw(cfg, 2), left_context=100, speed=1.25)))
    with pytest.raises(ValueError, match="speed"):
        next(iter(model.stream(**_kw(cfg, 2), speed=2.5)))
    with pytest.raises(ValueError, match="entries"):
        next(iter(model.serve_stream(**_kw(cfg, 3), max_batch=2, speed=[1.0, 1.25])))


def test_generate_custom_voice():
    from oracle import codec_param_specs, load_preset, synth_state_dict, talker_param_specs
    from oracle.encoder import encoder_param_specs
    from qwen_tts import Qwen3TTSModel
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    cfg, ccfg = load_preset("tiny-customvoice")
    Wn = synth_state_dict(talker_param_specs(cfg))
    CWn = synth_state_dict(codec_param_specs(ccfg) + encoder_param_specs(ccfg))
    tts = Qwen3TTSModel.from_pretrained("synthetic:tiny-customvoice", dtype=torch.float32,
                                        weights={k: torch.from_numpy(v) for k, v in Wn.items()},
                                        codec_weights={k: torch.from_numpy(v) for k, v in CWn.items()})
    kw = dict(text=["She said she would be here by noon.", "No."], language="English", speaker=["Vivian", "Ryan"],
              do_sample=False, subtalker_dosample=False, max_new_tokens=10)
    base, sr0 = tts.generate_custom_voice(**kw)
    got, sr = tts.generate_custom_voice(**kw, speed=[1.25, 1.0])
    assert sr0 == sr == 24000 and len(got) == 2
    want = _stretched(torch.from_numpy(base[0]).cuda(), 125).cpu().numpy()
    assert got[0].dtype == np.float32 and np.array_equal(got[0], want)
    assert np.array_equal(got[1], base[1])
    # the streaming wrapper hands out numpy chunks that add up to the stretched length
    n = [0, 0]
    for i, pcm, rate, last in tts.stream(**kw, speed=[1.25, 1.0]):
        assert pcm.dtype == np.float32 and rate == 24000
        n[i] += pcm.shape[0]
    assert n == [g.shape[0] for g in got]
    with pytest.raises(ValueError, match="speed"):
        tts.generate_custom_voice(**kw, speed=float("nan"))
