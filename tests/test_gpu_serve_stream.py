"""TTSModel.serve_stream / stream(max_batch=k): streaming from the continuously batched route, tiny
models in fp32.  Per request the chunks concatenate to Qwen3TTSTokenizer.decode of that request's codes alone, within
the bound of test_stream_matches_one_shot (atol 2e-4), and the codes are generate(max_batch=k)'s."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


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


def _kw(cfg, **over):
    from cases import make_inputs
    case = _serve_case()
    ids, _, _, _ = make_inputs(case, 11, cfg["talker_config"]["hidden_size"])
    kw = dict(input_ids=ids, languages=case["languages"], speakers=case["speakers"], non_streaming_mode=False,
              max_new_tokens=case["max_new_tokens"], seed=7)
    kw.update(over)
    return kw


_REF = {}


def _reference(model, tok, name, kw, mb):
    """generate(max_batch=mb)'s codes and the one-shot decode of each request alone (computed once per key)"""
    key = (name, mb)
    if key not in _REF:
        codes, _ = model.generate(**kw, max_batch=mb)
        _REF[key] = (codes, [tok.decode([{"audio_codes": c}])[0][0] for c in codes])
    return _REF[key]


def _check(stream, codes, wavs, what):
    chunks, lasts = {}, {}
    for i, pcm, last in stream:
        assert i not in lasts, (what, i, "a chunk after last=True")
        chunks.setdefault(i, []).append(pcm.cpu().numpy())
        if last:
            lasts[i] = True
    assert sorted(chunks) == list(range(len(codes))), what      # every request index appears
    assert sorted(lasts) == list(range(len(codes))), what       # exactly one last=True each, and it came last
    for i, w in enumerate(wavs):
        got = np.concatenate(chunks[i])
        assert got.shape == w.shape, (what, i, got.shape, w.shape)
        err = float(np.abs(got - w).max()) if w.size else 0.0
        print(f"{what} request {i}: {codes[i].shape[0]} frames, {len(chunks[i])} chunks, max |diff| {err:.3g}")
        np.testing.assert_allclose(got, w, atol=2e-4, rtol=0, err_msg=f"{what} request {i}")
    return chunks


@pytest.mark.parametrize("sample", [False, True])
@pytest.mark.parametrize("mb", [1, 2, 4])
def test_serve_stream_matches_one_shot(models, mb, sample):
    cfg, model, _, tok = models
    kw = _kw(cfg, do_sample=sample, subtalker_dosample=sample)
    name = f"sample={sample}"
    one, _ = _reference(model, tok, name, kw, None)
    assert len({c.shape[0] for c in one}) > 1  # EOS-ragged
    codes, wavs = _reference(model, tok, name, kw, mb)
    for a, b in zip(codes, one):
        np.testing.assert_array_equal(a.numpy(), b.numpy())
    # mb = 2 goes through the public switch of stream(), the others call serve_stream() itself
    it = model.stream(**kw, max_batch=mb, first_chunk_frames=1, chunk_frames=8) if mb == 2 else \
        model.serve_stream(**kw, max_batch=mb, first_chunk_frames=1, chunk_frames=8)
    chunks = _check(it, codes, wavs, f"max_batch={mb} {name}")
    # a request's first packet is its own first frame: 1920 - 555 samples, for refilled requests too
    for i, c in enumerate(codes):
        if c.shape[0] >= 1 and int((c[:, 0] != 0).sum()) == c.shape[0]:
            assert chunks[i][0].shape[0] == 1920 - 555, (i, chunks[i][0].shape)
    assert not any(sl.busy for pool in tok.model._row_slots.values() for sl in pool)


def test_serve_stream_per_request_parameters(models):
    cfg, model, _, tok = models
    kw = _kw(cfg, do_sample=[True, False, True, True, False, True], top_k=[50, 1, 8, 50, 50, 3],
             temperature=[0.9, 1.0, 0.7, 1.2, 0.9, 0.8], top_p=[1.0, 1.0, 0.9, 1.0, 0.8, 1.0],
             subtalker_dosample=[True, False, True, False, True, True], repetition_penalty=[1.05, 1.0, 1.1, 1.05, 1.2, 1.0],
             seed=[7, 8, 9, 10, 11, 12])
    codes, wavs = _reference(model, tok, "per-row", kw, 2)
    _check(model.serve_stream(**kw, max_batch=2, first_chunk_frames=2, chunk_frames=5), codes, wavs, "per-request")


@pytest.mark.parametrize("caps", [None, [331, 40, 331]])
def test_serve_stream_chunk_restarts(models, caps):
    """3 requests of 331 frames through 2 rows: every request crosses the 300-frame reference chunk, so its row
    restarts on the chunk's 25 context frames -- the first two together, the refilled one on its own later.  With
    frame caps (331, 40, 331) the refill comes early, and each long request restarts while the other row is mid-way
    through its own."""
    cfg, _, model, tok = models
    kw = _kw(cfg, do_sample=False, subtalker_dosample=False, max_new_tokens=332)
    for k in ("input_ids", "languages", "speakers"):
        kw[k] = kw[k][:3]
    if caps is not None:
        kw["frame_caps"] = caps
    codes, wavs = _reference(model, tok, f"long{caps}", kw, 2)
    assert [c.shape[0] for c in codes] == (caps or [331] * 3)
    _check(model.serve_stream(**kw, max_batch=2, first_chunk_frames=1, chunk_frames=8), codes, wavs, f"331 {caps}")


def test_serve_stream_rejects_icl_prompts(models):
    from cases import gen_kwargs, make_inputs, talker_cases
    cfg, _, model, tok = models
    key = "icl_b2"
    case = dict(talker_cases()[key], max_new_tokens=6)
    ids, ins, vcp, ref_ids = make_inputs(case, list(talker_cases()).index(key), cfg["talker_config"]["hidden_size"])
    kw = dict(input_ids=ids, instruct_ids=ins, ref_ids=ref_ids, voice_clone_prompt=vcp, speakers=case["speakers"],
              languages=case["languages"], non_streaming_mode=case["non_streaming_mode"], **gen_kwargs(case))
    assert any(r is not None for r in vcp["ref_code"])
    dec = tok.model
    for call in (lambda: model.stream(**kw, max_batch=1), lambda: model.serve_stream(**kw, max_batch=1)):
        with pytest.raises(NotImplementedError, match="ICL"):
            next(iter(call()))
    with pytest.raises(NotImplementedError, match="left_context"):
        next(iter(model.stream(**kw, max_batch=1, left_context=100)))
    torch.cuda.synchronize()
    pools = list(dec._slots.values()) + list(getattr(dec, "_row_slots", {}).values())
    assert not any(sl.busy for pool in pools for sl in pool)  # no pooled codec slot is left taken
