"""Prefix cache end to end: tiny-voicedesign with synthetic weights whose EOS row is the donor's of
test_gpu_serve_stream.py (requests end raggedly), fp32 unless stated.

Six requests carry the instructions A (8 ids) and B (12 ids) and none, with mixed text lengths and languages and
max_new_tokens = 40.  Every test asserts on cache.stats as well as on outputs: generate() swallows unknown keywords,
so equal outputs alone would also pass without the feature.

The tolerance between a cached and an uncached prefill of one request is atol = rtol = 1e-5, the bound
test_continuous_batching_matches_one_shot uses for two prefill row counts of one request (the cached prefill computes
fewer rows, so its linears may take another kernel); PCM is compared at atol 2e-4, the bound of
test_gpu_serve_stream.py."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TEXTS = [7, 3, 10, 5, 12, 4]
LANGS = ["auto", "english", "japanese", "chinese", "english", "auto"]
LISTED = "AABA-B"   # the request list as listed
SPREAD = "ABAA-B"   # the same requests ordered so that, through two slots, no two first uses of a key share a prefill
TOL = dict(atol=1e-5, rtol=1e-5)


def _instruction(name):
    from cases import instruct_ids
    return {"A": instruct_ids(3, 901), "B": instruct_ids(7, 902), "-": None}[name]   # 3 + 5 and 7 + 5 template ids


def _build(preset, dtype, ragged=True):
    from oracle import codec_param_specs, load_preset, synth_state_dict, talker_param_specs
    from qwen_tts import Qwen3TTSTokenizer
    from qwen_tts.model import TTSModel
    cfg, ccfg = load_preset(preset)
    W = {k: torch.from_numpy(v) for k, v in synth_state_dict(talker_param_specs(cfg)).items()}
    if ragged:
        z = np.load(os.path.join(GOLD, "tiny_talker.npz"))
        head = W["talker.codec_head.weight"].clone()
        head[cfg["talker_config"]["codec_eos_token_id"]] = head[int(z["eos_b2/donor"])]
        W["talker.codec_head.weight"] = head
    CW = {k: torch.from_numpy(v) for k, v in synth_state_dict(codec_param_specs(ccfg)).items()}
    tok = Qwen3TTSTokenizer.from_pretrained(f"synthetic:{preset}/speech_tokenizer", dtype="fp32", weights=CW)
    m = TTSModel(cfg, W, dtype=dtype)
    m.load_speech_tokenizer(tok)
    return cfg, m, tok


@pytest.fixture(scope="module")
def vd():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return _build("tiny-voicedesign", "fp32")


def _kw(cfg, pattern=LISTED, rows=None, **over):
    from cases import make_inputs
    rows = list(range(len(pattern))) if rows is None else rows
    ids, _, _, _ = make_inputs(dict(texts=TEXTS), 11, cfg["talker_config"]["hidden_size"])
    kw = dict(input_ids=[ids[i] for i in rows], instruct_ids=[_instruction(pattern[i]) for i in rows],
              languages=[LANGS[i] for i in rows], speakers=None, non_streaming_mode=False, max_new_tokens=40, seed=7)
    kw.update(over)
    return kw


def _cache():
    from qwen_tts import PrefixCache
    return PrefixCache()


def _counts(c):
    s = c.stats
    return s["hits"], s["misses"], s["stores"]


def _same_codes(got, want, what):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(a.numpy(), b.numpy(), err_msg=f"{what} request {i}")


def _close_hidden(got, want, what):
    for i, (a, b) in enumerate(zip(got, want)):
        np.testing.assert_allclose(a.numpy(), b.numpy(), err_msg=f"{what} request {i}", **TOL)


def _slot_prefill(model, kw, i, plan=None, row=0, session=None):
    """Request i of kw through TalkerEngine._prefill_slot into batch row `row` of a 2-row session: the row's K/V over
    the prompt, past_hidden, first-token logits and first token (device clones), and the session."""
    from qwen_tts import kernels as Kn
    from qwen_tts.talker import GenParams
    eng = model.engine
    lens = []
    emb, mask, trail, pad = model.build_prompts([kw["input_ids"][i]], [kw["languages"][i]], None,
                                                [kw["instruct_ids"][i]], False, lens_out=lens)
    P = lens[0]
    assert emb.shape[1] == P
    s = session
    if s is None:
        s = eng.session(2, P, 39, GenParams(max_new_tokens=40, do_sample=False, subtalker_dosample=False))
        s.pad_embed.copy_(pad.reshape(-1).float())
        s.seed.fill_(7)
    with Kn.use_workspace(s.ws):
        eng._prefill_slot(s, row, (emb[0], trail[0]), i, prefix=None if plan is None else plan(P))
    torch.cuda.synchronize()
    out = dict(k=torch.stack([t[row, :, :P] for t in s.kv[0]]).clone(),
               v=torch.stack([t[row, :, :P] for t in s.kv[1]]).clone(), hidden=s.past_hidden[row].clone(),
               logits=s.logits[row].clone(), tok=int(s.tok0[row]), P=P)
    return out, s


def test_adopt_and_suffix_prefill_match_the_full_prefill(vd):
    from qwen_tts.prefix import PrefixCache, PrefixPlan
    cfg, model, _ = vd
    kw = _kw(cfg)
    eng = model.engine
    c = _cache()
    c.bind(eng)
    key = PrefixCache.key(kw["instruct_ids"][0])
    N = len(key)
    assert N == 8
    plan = lambda P: PrefixPlan(c, [key], [P])  # noqa: E731
    full, s = _slot_prefill(model, kw, 0)
    try:
        donor, _ = _slot_prefill(model, kw, 0, plan, row=0, session=s)      # a miss: computes in full and exports
        assert _counts(c) == (0, 1, 1) and c.stats["entries"] == 1
        block = c.lookup(key).block
        t = eng.talker
        assert tuple(block.shape) == (2, t.n_layers, t.Hkv, N, t.D) and block.dtype == eng.kv_dtype
        assert c.stats["bytes"] == block.numel() * block.element_size()
        assert torch.equal(block[0], donor["k"][:, :, :N]) and torch.equal(block[1], donor["v"][:, :, :N])
        for lay in s.kv[0] + s.kv[1]:
            lay[1].fill_(float("nan"))                                      # whatever is not written would show
        got, _ = _slot_prefill(model, kw, 0, plan, row=1, session=s)       # a hit: adopts, computes P - N rows
        assert c.stats["hits"] == 2 and got["P"] - N in s.prefix_prefill    # (one hit is the lookup above)
        # the adopted positions are the donor's export, bit for bit
        assert torch.equal(got["k"][:, :, :N], block[0]) and torch.equal(got["v"][:, :, :N], block[1])
        for name in ("k", "v"):
            err = float((got[name][:, :, N:] - full[name][:, :, N:]).abs().max())
            print(f"suffix {name} max |diff| vs the full prefill: {err:.3g}")
            torch.testing.assert_close(got[name][:, :, N:], full[name][:, :, N:], **TOL)
            torch.testing.assert_close(donor[name], full[name], **TOL)
        for name in ("hidden", "logits"):
            print(f"{name} max |diff| vs the full prefill: {float((got[name] - full[name]).abs().max()):.3g}")
            torch.testing.assert_close(got[name], full[name], **TOL)
        assert got["tok"] == full["tok"] == donor["tok"]
    finally:
        eng.release([s])


@pytest.mark.parametrize("sample", [False, True])
def test_generate_through_two_slots(vd, sample):
    cfg, model, _ = vd
    kw = _kw(cfg, SPREAD, do_sample=sample, subtalker_dosample=sample)
    want, want_h = model.generate(**kw, max_batch=2)
    assert len({c.shape[0] for c in want}) > 1  # EOS-ragged
    c = _cache()
    got, got_h = model.generate(**kw, max_batch=2, prefix_cache=c)
    _same_codes(got, want, f"sample={sample}")
    _close_hidden(got_h, want_h, f"sample={sample}")
    # A and B miss in the first prefill and are stored; the two later A and the later B hit; "-" never asks
    assert _counts(c) == (3, 2, 2), c.stats
    assert c.stats["entries"] == 2 and c.stats["evictions"] == 0


def test_two_first_uses_in_one_prefill_both_compute_in_full(vd):
    """The list as listed starts with A, A in one prefill: both miss (each computes in full), the first one exports."""
    cfg, model, _ = vd
    kw = _kw(cfg, LISTED, do_sample=False, subtalker_dosample=False)
    want, _ = model.generate(**kw, max_batch=2)
    c = _cache()
    got, _ = model.generate(**kw, max_batch=2, prefix_cache=c)
    _same_codes(got, want, "listed order")
    assert _counts(c) == (2, 3, 2), c.stats


def test_one_shot_batch_hits_at_every_padding_offset(vd):
    cfg, model, _ = vd
    rows = [0, 4, 2, 3]  # A, none, B, A
    kw = _kw(cfg, LISTED, rows, non_streaming_mode=True, do_sample=False, subtalker_dosample=False)
    assert [LISTED[i] for i in rows] == ["A", "-", "B", "A"]
    lens = []
    model.build_prompts(kw["input_ids"], kw["languages"], None, kw["instruct_ids"], True, lens_out=lens)
    assert len({max(lens) - lens[i] for i in (0, 2, 3)}) == 3   # three instructed rows, three padding offsets
    want, want_h = model.generate(**kw)
    c = _cache()
    first, _ = model.generate(**kw, prefix_cache=c)
    assert _counts(c) == (0, 3, 2), c.stats      # the two A rows of one call both miss
    second, second_h = model.generate(**kw, prefix_cache=c)
    assert _counts(c) == (3, 3, 2), c.stats
    _same_codes(first, want, "first call")
    _same_codes(second, want, "second call")
    _close_hidden(second_h, want_h, "second call")


def _collect(stream):
    chunks, lasts = {}, set()
    for i, pcm, last in stream:
        assert i not in lasts, (i, "a chunk after last=True")
        chunks.setdefault(i, []).append(pcm.cpu().numpy())
        if last:
            lasts.add(i)
    assert sorted(lasts) == sorted(chunks)
    return chunks


def test_serve_stream(vd):
    cfg, model, tok = vd
    kw = _kw(cfg, LISTED, do_sample=False, subtalker_dosample=False)
    codes, _ = model.generate(**kw, max_batch=2)
    wavs = [tok.decode([{"audio_codes": x}])[0][0] for x in codes]
    plain = _collect(model.serve_stream(**kw, max_batch=2, first_chunk_frames=1, chunk_frames=8))
    c = _cache()
    got = _collect(model.serve_stream(**kw, max_batch=2, first_chunk_frames=1, chunk_frames=8, prefix_cache=c))
    assert sorted(got) == list(range(len(codes)))
    for i, w in enumerate(wavs):
        a, b = np.concatenate(got[i]), np.concatenate(plain[i])
        assert a.shape == b.shape == w.shape, (i, a.shape, b.shape, w.shape)   # the codes are generate(max_batch=2)'s
        print(f"request {i}: {codes[i].shape[0]} frames, max |diff| vs uncached stream "
              f"{float(np.abs(a - b).max()) if a.size else 0.0:.3g}")
        np.testing.assert_allclose(a, b, atol=2e-4, rtol=0, err_msg=f"request {i} vs the uncached stream")
        np.testing.assert_allclose(a, w, atol=2e-4, rtol=0, err_msg=f"request {i} vs decode(generate's codes)")
    assert _counts(c) == (2, 3, 2), c.stats      # hits > 0: the refills of the later A and B
    assert not any(sl.busy for pool in tok.model._row_slots.values() for sl in pool)


def test_stream_second_call_hits(vd):
    cfg, model, _ = vd
    kw = _kw(cfg, LISTED, [0])
    c = _cache()
    first = _collect(model.stream(**kw, first_chunk_frames=1, chunk_frames=8, prefix_cache=c))
    assert _counts(c) == (0, 1, 1)
    second = _collect(model.stream(**kw, first_chunk_frames=1, chunk_frames=8, prefix_cache=c))
    assert _counts(c) == (1, 1, 1)
    a, b = np.concatenate(first[0]), np.concatenate(second[0])
    assert a.shape == b.shape and a.size > 0
    np.testing.assert_allclose(b, a, atol=2e-4, rtol=0)
    assert second[0][0].shape[0] == 1920 - 555


def _entry_bytes(model, n):
    t = model.engine.talker
    return 2 * t.n_layers * t.Hkv * n * t.D * torch.empty(0, dtype=model.engine.kv_dtype).element_size()


def test_eviction_through_one_slot(vd):
    from qwen_tts import PrefixCache
    cfg, model, _ = vd
    kw = _kw(cfg, "ABA", do_sample=False, subtalker_dosample=False)
    want, _ = model.generate(**kw, max_batch=1)
    c = PrefixCache(max_bytes=_entry_bytes(model, 12))   # room for B alone, or for A alone
    got, _ = model.generate(**kw, max_batch=1, prefix_cache=c)
    _same_codes(got, want, "A, B, A")
    s = c.stats
    assert (s["hits"], s["misses"], s["stores"], s["evictions"], s["entries"]) == (0, 3, 3, 2, 1), s
    tiny = PrefixCache(max_bytes=_entry_bytes(model, 8) - 1)   # nothing fits: nothing is stored, nothing breaks
    got, _ = model.generate(**kw, max_batch=1, prefix_cache=tiny)
    _same_codes(got, want, "A, B, A without room")
    s = tiny.stats
    assert (s["hits"], s["misses"], s["stores"], s["entries"], s["bytes"]) == (0, 3, 0, 0, 0), s


def test_eviction_while_the_adopter_is_still_decoding(vd):
    """Two slots, frame counts fixed by frame_caps with ignore_eos.  Slot 0: A for 2 frames (stores A), then A again
    for 30 frames (adopts A).  Slot 1: no instruction for 6 frames, then B for 4 frames, whose store evicts A while
    the adopter has ~24 frames to go.  The adopter's K/V is a copy: its codes are the uncached ones."""
    from qwen_tts import PrefixCache
    cfg, model, _ = vd
    rows = [0, 4, 1, 2]  # A, none, A, B
    caps = [2, 6, 30, 4]
    kw = _kw(cfg, LISTED, rows, do_sample=False, subtalker_dosample=False, ignore_eos=True, frame_caps=caps)
    assert [LISTED[i] for i in rows] == ["A", "-", "A", "B"]
    want, _ = model.generate(**kw, max_batch=2)
    assert [x.shape[0] for x in want] == caps
    c = PrefixCache(max_bytes=_entry_bytes(model, 12))
    got, _ = model.generate(**kw, max_batch=2, prefix_cache=c)
    _same_codes(got, want, "evicted mid-request")
    s = c.stats
    assert (s["hits"], s["misses"], s["stores"], s["evictions"]) == (1, 2, 2, 1), s
    assert c.keys() == [PrefixCache.key(_instruction("B"))]


def test_requests_without_instruction_leave_the_cache_empty():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cases import make_inputs
    cfg, model, _ = _build("tiny-customvoice", "fp32")
    ids, _, _, _ = make_inputs(dict(texts=TEXTS), 11, cfg["talker_config"]["hidden_size"])
    kw = dict(input_ids=ids, languages=LANGS, speakers=["vivian", None, "dylan", "eric", "ryan", ""],
              non_streaming_mode=False, max_new_tokens=40, seed=7)
    c = _cache()
    for extra in (dict(), dict(max_batch=2)):
        want, want_h = model.generate(**kw, **extra)
        got, got_h = model.generate(**kw, **extra, prefix_cache=c)
        for a, b, x, y in zip(got, want, got_h, want_h):
            assert torch.equal(a, b) and torch.equal(x, y)     # the same code ran: the same bits
    assert c.stats == dict(hits=0, misses=0, stores=0, evictions=0, entries=0, bytes=0)
    with pytest.raises(ValueError, match="bound to another engine"):   # bound at its first use, instruction or not
        _build("tiny-customvoice", "fp32")[1].generate(**kw, prefix_cache=c)
    with pytest.raises(ValueError, match="PrefixCache"):
        model.generate(**kw, prefix_cache={})


def test_bf16_cached_prefill_is_as_close_to_fp32_as_the_uncached_one(vd):
    """First-token logits of every request of the two-slot list: the bf16 engine's cached prefill (a hit) and its
    uncached prefill, each against the fp32 engine's logits of the same request, as relative L2 error.  Asserted:
    cached <= 1.25 x uncached (the project's engine-versus-launch-chain rule).  Codes are printed, not asserted: a
    near-tie may resolve differently between two prefill row counts (TalkerEngine.serve)."""
    from qwen_tts.prefix import PrefixCache, PrefixPlan
    cfg, m32, _ = vd
    _, m16, _ = _build("tiny-voicedesign", "bf16")
    kw = _kw(cfg, SPREAD, do_sample=False, subtalker_dosample=False)
    c = _cache()
    c.bind(m16.engine)
    sessions = []
    try:
        for i, name in enumerate(SPREAD):
            if name == "-":
                continue
            key = PrefixCache.key(kw["instruct_ids"][i])
            plan = lambda P: PrefixPlan(c, [key], [P])  # noqa: E731
            ref, s32 = _slot_prefill(m32, kw, i)
            sessions.append((m32, s32))
            unc, s16 = _slot_prefill(m16, kw, i)
            sessions.append((m16, s16))
            if key not in c.keys():
                _slot_prefill(m16, kw, i, plan, session=s16)       # the miss that stores the entry
            hits = c.stats["hits"]
            hit, _ = _slot_prefill(m16, kw, i, plan, row=1, session=s16)
            assert c.stats["hits"] == hits + 1
            rel = lambda x: float((x["logits"].double() - ref["logits"].double()).norm() /  # noqa: E731
                                  ref["logits"].double().norm())
            e_hit, e_unc = rel(hit), rel(unc)
            print(f"request {i} ({name}): cached {e_hit:.3e}  uncached {e_unc:.3e}  ratio {e_hit / e_unc:.3f}  "
                  f"first token fp32 / cached / uncached {ref['tok']} / {hit['tok']} / {unc['tok']}")
            assert e_hit <= 1.25 * e_unc, (i, e_hit, e_unc)
            for m, s in sessions:
                m.engine.release([s])
            sessions = []
        got, _ = m16.generate(**kw, max_batch=2, prefix_cache=c)
        want, _ = m16.generate(**kw, max_batch=2)
        print("bf16 codes, cached vs uncached, equal per request:",
              [bool(a.shape == b.shape and torch.equal(a, b)) for a, b in zip(got, want)])
    finally:
        for m, s in sessions:
            m.engine.release([s])
