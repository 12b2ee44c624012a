"""Voice-clone (ICL) requests on the continuously batched routes through a VoiceCache: serve_stream(),
stream(max_batch=...) and serve_live() with voice_cache=.  Tiny models in fp32, the recipes of
test_gpu_serve_stream.py.  Per request the codes are generate(max_batch=k)'s (= generate()'s) and the chunks
concatenate to Qwen3TTSTokenizer.decode(cat(ref_i, codes_i))[1920 R_i:] within the project's PCM bound (atol 2e-4),
with exact shapes."""
import math
import os

import numpy as np
import pytest
import torch

import resample_refs as RR
import small_kernel_refs as SR

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
UP, FIRST = 1920, 1920 - 555
ICL = [0, 2, 3, 5]  # the ICL requests of the six; 3 has the voice of 0, 5 that of 2


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


def _six(cfg, **over):
    """icl_b2 of tests/golden/cases.py extended to six requests: ICL R = 7, x-vector-only, ICL R = 4, ICL R = 7 with
    the first one's voice, plain, ICL R = 4 with the third one's voice."""
    from cases import make_inputs, talker_cases
    key = "icl_b2"
    case = dict(talker_cases()[key], texts=[6, 9, 5, 8, 7, 4], languages=["english", "auto", "english", "auto", "english", "auto"],
                icl=[(5, 7, True, False), (12, 4, False, True), (8, 4, True, False), (5, 7, True, False),
                     (6, 3, False, False), (8, 4, True, False)])
    ids, _, vcp, ref_ids = make_inputs(case, list(talker_cases()).index(key), cfg["talker_config"]["hidden_size"])
    for dst, src in ((3, 0), (5, 2)):
        vcp["ref_code"][dst], vcp["ref_spk_embedding"][dst] = vcp["ref_code"][src], vcp["ref_spk_embedding"][src]
        ref_ids[dst] = ref_ids[src]
    assert [None if r is None else r.shape[0] for r in vcp["ref_code"]] == [7, None, 4, 7, None, 4]
    kw = dict(input_ids=ids, ref_ids=ref_ids, voice_clone_prompt=vcp, languages=case["languages"], speakers=None,
              non_streaming_mode=False, max_new_tokens=24, seed=7, do_sample=False, subtalker_dosample=False)
    kw.update(over)
    return kw


_REF = {}


def _expected(tok, refs, codes):
    out = []
    for r, c in zip(refs, codes):
        if r is None:
            out.append(tok.decode([{"audio_codes": c}])[0][0])
        else:
            out.append(tok.decode([{"audio_codes": torch.cat([r.long(), c])}])[0][0][UP * r.shape[0]:])
    return out


def _reference(model, tok, name, kw, mb):
    """generate(max_batch=mb)'s codes and the one-shot decode of cat(ref_i, codes_i) from the boundary on (computed
    once per key)"""
    if (name, mb) not in _REF:
        codes, _ = model.generate(**kw, max_batch=mb)
        _REF[name, mb] = (codes, _expected(tok, kw["voice_clone_prompt"]["ref_code"], codes))
    return _REF[name, mb]


def _collect(stream, n, what):
    chunks, lasts = {}, {}
    for i, pcm, last in stream:
        assert i not in lasts, (what, i, "a chunk after last=True")
        chunks.setdefault(i, []).append(pcm.cpu())
        if last:
            lasts[i] = True
    assert sorted(chunks) == list(range(n)), what      # every request index appears
    assert sorted(lasts) == list(range(n)), what       # exactly one last=True each, and it came last
    return chunks


def _check(chunks, codes, wavs, what):
    for i, w in enumerate(wavs):
        got = torch.cat(chunks[i]).numpy()
        assert got.shape == w.shape, (what, i, got.shape, w.shape)
        err = float(np.abs(got - w).max()) if w.size else 0.0
        print(f"{what} request {i}: {codes[i].shape[0]} frames, {len(chunks[i])} chunks, max |diff| {err:.3g}")
        np.testing.assert_allclose(got, w, atol=2e-4, rtol=0, err_msg=f"{what} request {i}")


def _nothing_held(model, tok):
    torch.cuda.synchronize()
    assert not any(s.busy for s in model.engine.all_sessions())
    dec = tok.model
    pools = list(dec._slots.values()) + list(getattr(dec, "_row_slots", {}).values())
    assert not any(sl.busy for pool in pools for sl in pool)


@pytest.mark.parametrize("sample", [False, True])
@pytest.mark.parametrize("mb", [1, 2, 4])
def test_serve_stream_voice_clone_matches_one_shot(models, mb, sample):
    from qwen_tts import VoiceCache
    cfg, model, _, tok = models
    kw = _six(cfg, do_sample=sample, subtalker_dosample=sample)
    name = f"sample={sample}"
    one, _ = _reference(model, tok, name, kw, None)
    codes, wavs = _reference(model, tok, name, kw, mb)
    for a, b in zip(codes, one):
        np.testing.assert_array_equal(a.numpy(), b.numpy())
    cache = VoiceCache()
    # mb = 2 goes through the public switch of stream(), the others call serve_stream() itself
    call = model.stream if mb == 2 else model.serve_stream
    chunks = _collect(call(**kw, max_batch=mb, first_chunk_frames=1, chunk_frames=8, voice_cache=cache), 6,
                      f"max_batch={mb} {name}")
    _check(chunks, codes, wavs, f"max_batch={mb} {name}")
    for i in ICL:  # a request's first packet is its own first frame, the reference's frames cost it nothing
        c = codes[i]
        if c.shape[0] >= 1 and int((c[:, 0] != 0).sum()) == c.shape[0]:
            assert chunks[i][0].shape[0] == FIRST, (i, chunks[i][0].shape)
    s = cache.stats
    assert (s["misses"], s["hits"], s["stores"], s["entries"]) == (2, 2, 2, 2), s
    _nothing_held(model, tok)


def test_cache_that_keeps_nothing_and_warmed_cache(models):
    from qwen_tts import VoiceCache
    cfg, model, _, tok = models
    kw = _six(cfg)
    codes, wavs = _reference(model, tok, "sample=False", kw, 2)
    run = lambda cache: _collect(model.serve_stream(**kw, max_batch=2, first_chunk_frames=1, chunk_frames=8,  # noqa: E731
                                                    voice_cache=cache), 6, "variants")
    kept = VoiceCache()
    base = run(kept)
    _check(base, codes, wavs, "kept")
    none = VoiceCache(max_bytes=0)
    got = run(none)
    s = none.stats
    assert (s["misses"], s["hits"], s["stores"], s["entries"], s["bytes"]) == (4, 0, 0, 0, 0), s
    for i in range(6):
        assert torch.equal(torch.cat(got[i]), torch.cat(base[i])), f"max_bytes=0: request {i} differs"
    warm = VoiceCache()
    assert warm.warm(model, kw["voice_clone_prompt"]) == 2 and warm.warm(tok, kw["voice_clone_prompt"]) == 0
    assert warm.stats["entries"] == 2 and warm.stats["misses"] == 0
    got = run(warm)
    s = warm.stats
    assert (s["misses"], s["hits"], s["stores"]) == (0, 4, 2), s
    _check(got, codes, wavs, "warmed")
    with pytest.raises(ValueError, match="VoiceCache"):
        next(iter(model.serve_stream(**kw, max_batch=2, voice_cache=object())))
    with pytest.raises(NotImplementedError, match="ICL"):  # without a cache the refusal stands
        next(iter(model.serve_stream(**kw, max_batch=2)))
    _nothing_held(model, tok)


def test_chunk_rule_edges(models):
    """R = 290: the restart 10 frames after adoption takes context frames from the reference and from generated codes;
    R = 300: the first generated frame opens a chunk, nothing is adopted; R = 301: the snapshot was taken after a
    restart.  14 frames each through two rows."""
    from cases import ref_text_ids, text_ids
    from qwen_tts import VoiceCache
    cfg, _, model, tok = models
    H = cfg["talker_config"]["hidden_size"]
    g = np.random.default_rng([5, 17])
    Rs = [290, 300, 301]
    vcp = dict(ref_code=[torch.tensor(g.integers(0, 2048, (R, 16)), dtype=torch.long) for R in Rs],
               ref_spk_embedding=[torch.tensor(0.02 * g.standard_normal(H), dtype=torch.float32) for _ in Rs],
               x_vector_only_mode=[False] * 3, icl_mode=[True] * 3)
    kw = dict(input_ids=[text_ids(6, 900 + j) for j in range(3)], ref_ids=[ref_text_ids(5, 950 + j) for j in range(3)],
              voice_clone_prompt=vcp, languages=["english"] * 3, speakers=None, non_streaming_mode=False,
              max_new_tokens=40, seed=7, do_sample=False, subtalker_dosample=False, frame_caps=[14, 14, 14])
    codes, wavs = _reference(model, tok, "edges", kw, 2)
    assert [c.shape[0] for c in codes] == [14, 14, 14]
    cache = VoiceCache()
    chunks = _collect(model.serve_stream(**kw, max_batch=2, first_chunk_frames=1, chunk_frames=8, voice_cache=cache),
                      3, "edges")
    _check(chunks, codes, wavs, "edges")
    entries = {k[0]: cache._entries[k] for k in cache.keys()}
    assert entries[290].adopts and entries[290].snapshot.p == 290
    assert not entries[300].adopts                            # nothing to adopt: the entry says so
    assert entries[301].adopts and entries[301].snapshot.p == 26   # 25 context frames + frame 300
    _nothing_held(model, tok)


def _judge(got, wav, rate, fmt, what):
    """test_gpu_stream_format's comparison: the fp64 resample of the expected 24 kHz audio, within 2e-4 x the filter's
    L1 gain + the resampler's own bound; for s16 that times 32767, rounded up, plus 1"""
    from qwen_tts.resample import plan
    p = plan(rate)
    x = torch.from_numpy(wav)
    ref = RR.resample(x, p)
    assert got.shape == ref.shape == (p.out_len(wav.shape[0]),), (what, got.shape, ref.shape)
    assert got.dtype == (torch.int16 if fmt == "s16" else torch.float32)
    if not ref.numel():
        return
    unit, _ = SR.fp32_tolerance(RR.resample(x, p, torch.float32), ref, RR.resample_scale(x, p))
    tol = 2e-4 * RR.l1_gain(p) + unit
    d = int((got.to(torch.int64) - RR.s16(ref).to(torch.int64)).abs().max())
    cap = math.ceil(float(tol.max()) * 32767) + 1
    print(f"{what}: {got.numel()} samples, max |diff| {d} of int16, allowed {cap}")
    assert d <= cap, what


def test_16khz_s16(models):
    from qwen_tts import VoiceCache
    cfg, model, _, tok = models
    kw = _six(cfg)
    codes, wavs = _reference(model, tok, "sample=False", kw, 2)
    chunks = _collect(model.serve_stream(**kw, max_batch=2, first_chunk_frames=1, chunk_frames=8, sample_rate=16000,
                                         pcm_format="s16", voice_cache=VoiceCache()), 6, "16k s16")
    for i in range(6):
        _judge(torch.cat(chunks[i]), wavs[i], 16000, "s16", f"16000/s16 request {i}")
    _nothing_held(model, tok)


def test_serve_live_voice_clone(models):
    from qwen_tts import RequestQueue, VoiceCache
    cfg, model, _, tok = models
    kw = _six(cfg)
    vcp = kw["voice_clone_prompt"]
    ss = _collect(model.serve_stream(**kw, max_batch=2, first_chunk_frames=1, chunk_frames=8,
                                     voice_cache=VoiceCache()), 6, "serve_stream")

    def submit(q, j, with_ref=True):
        one = {k: [v[j]] for k, v in vcp.items()}
        if not (one["icl_mode"][0] or one["x_vector_only_mode"][0]):
            return q.submit(kw["input_ids"][j], language=kw["languages"][j], do_sample=False, subtalker_dosample=False)
        return q.submit(kw["input_ids"][j], language=kw["languages"][j], voice_clone_prompt=one,
                        ref_ids=kw["ref_ids"][j] if with_ref and one["icl_mode"][0] else None, do_sample=False,
                        subtalker_dosample=False)
    q = RequestQueue(timeout=5.0)
    assert [submit(q, 0), submit(q, 1)] == [0, 1]
    cache = VoiceCache()
    chunks, lasts, later = {}, {}, False
    for i, pcm, last in model.serve_live(q, max_batch=2, max_prompt=64, max_new_tokens=24, seed=7, first_chunk_frames=1,
                                         chunk_frames=8, voice_cache=cache):
        assert i not in lasts
        chunks.setdefault(i, []).append(pcm.cpu())
        if last:
            lasts[i] = True
        if not later:  # the other four arrive while the loop runs
            later = True
            assert [submit(q, j) for j in range(2, 6)] == [2, 3, 4, 5]
            assert submit(q, 0, with_ref=False) == 6   # icl_mode without the reference text
            q.close()
    assert sorted(lasts) == list(range(7)) and q.timed_out == ()
    assert list(q.rejected) == [6] and isinstance(q.rejected[6], ValueError) and "ref_ids" in str(q.rejected[6])
    assert torch.cat(chunks[6]).numel() == 0
    for i in range(6):
        got, exp = torch.cat(chunks[i]), torch.cat(ss[i])
        assert got.shape == exp.shape, (i, got.shape, exp.shape)
        err = float((got - exp).abs().max()) if exp.numel() else 0.0
        print(f"live request {i}: {got.numel()} samples, max |pcm - serve_stream| {err:.3g}")
        torch.testing.assert_close(got, exp, atol=2e-4, rtol=0)
    s = cache.stats
    assert (s["misses"], s["hits"]) == (2, 2), s
    _nothing_held(model, tok)

    # a loop without a voice cache rejects the ICL request and serves the other
    q = RequestQueue(timeout=5.0)
    assert [submit(q, 0), submit(q, 4)] == [0, 1]
    q.close()
    chunks, lasts = {}, {}
    for i, pcm, last in model.serve_live(q, max_batch=2, max_prompt=64, max_new_tokens=24, seed=7):
        chunks.setdefault(i, []).append(pcm.cpu())
        lasts[i] = lasts.get(i, False) or last
    assert lasts == {0: True, 1: True}
    assert list(q.rejected) == [0] and isinstance(q.rejected[0], NotImplementedError) and "ICL" in str(q.rejected[0])
    assert torch.cat(chunks[0]).numel() == 0 and torch.cat(chunks[1]).numel() > 0
    _nothing_held(model, tok)
