"""TTSModel.serve_live(queue): requests that arrive while the engine decodes, text fed per request, held rows
(DESIGN §19).  tiny-customvoice; the fp32 model's EOS row is the donor's (the recipe of test_gpu_text_feed.py), so
requests end raggedly.

1. five whole-text requests submitted ahead, 2 rows, fp32: generate(max_batch=2)'s codes, serve_stream()'s PCM (2e-4);
2. the same requests, the later ones submitted when request 0's first chunk arrives: the same codes;
3. open text all pushed ahead against trickled -- a row gets its next token only when the other request's chunk is
   received, so it starves while the other decodes: bit-equal codes, bf16 and fp32, greedy and sampled; in fp32 they
   are the whole-text streaming-mode request's; rows were held in the trickled delivery only;
4. a request holding only its first text token gets its one-frame first packet while another runs to its end, and
   completes with the whole-text codes once its text has come;
5. timeout retirement, cancel (decoding and queued), rejected requests beside one that completes, nothing left held,
   one 16 kHz s16 run against serve_stream()'s bit for bit, one prefix-cache run with two hits;
6. the wrapper's request_queue() / serve_live() with strings against the model-level requests of their ids.

Every queue has a timeout of at most 5 s and nothing else blocks: a bug ends as a failure, not as a stalled process."""
import contextlib
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIRST = 1920 - 555  # samples of a one-frame first packet
TEXTS = [7, 3, 10, 5, 12]
LANGS = ["auto", "english", "japanese", "chinese", "english"]
SPKS = ["vivian", None, "dylan", "eric", "ryan"]


@pytest.fixture(scope="module")
def models():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from oracle import codec_param_specs, load_preset, synth_state_dict, talker_param_specs
    from qwen_tts import Qwen3TTSTokenizer
    from qwen_tts.model import TTSModel
    cfg, ccfg = load_preset("tiny-customvoice")
    W = {k: torch.from_numpy(v) for k, v in synth_state_dict(talker_param_specs(cfg)).items()}
    CW = {k: torch.from_numpy(v) for k, v in synth_state_dict(codec_param_specs(ccfg)).items()}
    tok = Qwen3TTSTokenizer.from_pretrained("synthetic:tiny-customvoice/speech_tokenizer", dtype="fp32", weights=CW)
    z = np.load(os.path.join(GOLD, "tiny_talker.npz"))
    We = dict(W)
    head = W["talker.codec_head.weight"].clone()
    head[cfg["talker_config"]["codec_eos_token_id"]] = head[int(z["eos_b2/donor"])]
    We["talker.codec_head.weight"] = head
    ms = {"fp32": TTSModel(cfg, We, dtype="fp32"), "bf16": TTSModel(cfg, W, dtype="bf16")}
    for m in ms.values():
        m.load_speech_tokenizer(tok)
    return cfg, ms, tok


def _queue(timeout=5.0):
    from qwen_tts import RequestQueue
    assert timeout <= 5.0
    return RequestQueue(timeout=timeout)


def _ids(n, seed):
    """(whole-text ids with the template suffix, head = 3 role ids + first text id, the other n - 1 text ids)"""
    from cases import text_ids
    ids = text_ids(n, seed)[0].tolist()
    return ids, ids[:4], ids[4:-5]


def _whole():
    return [_ids(n, 1100 + j)[0] for j, n in enumerate(TEXTS)]


def _nothing_held(model, tok):
    torch.cuda.synchronize()
    assert not any(s.busy for s in model.engine.all_sessions())
    dec = tok.model
    pools = list(dec._slots.values()) + list(getattr(dec, "_row_slots", {}).values())
    assert not any(sl.busy for pool in pools for sl in pool)


@contextlib.contextmanager
def _tap(model):
    """request -> the code rows the talker reported for it, in order (read where the codec reads them)"""
    eng, got = model.engine, {}
    orig = eng.serve_live_iter

    def tapped(*a, **k):
        for s, report in orig(*a, **k):
            if s is not None:
                for b, r in enumerate(report):
                    if r is not None:
                        got.setdefault(r[0], []).append(s.codes[b, r[1]:r[2]].cpu().long())
            yield s, report
    eng.serve_live_iter = tapped
    try:
        yield got
    finally:
        del eng.serve_live_iter


class Run:
    """one serve_live() run: chunks and codes per request; on_chunk(run, i, pcm, last) is called after each chunk"""

    def __init__(self, model, queue, on_chunk=None, **kw):
        self.chunks, self.last, self.order = {}, {}, []
        kw.setdefault("seed", 7)
        with _tap(model) as got:
            for i, pcm, last in model.serve_live(queue, **kw):
                assert i not in self.last, (i, "a chunk after last=True")
                self.chunks.setdefault(i, []).append(pcm.cpu().numpy())
                self.order.append((i, int(pcm.shape[0]), bool(last)))
                if last:
                    self.last[i] = True
                if on_chunk is not None:
                    on_chunk(self, i, pcm, last)
        self.codes = {i: torch.cat(c) for i, c in got.items()}
        self.stats = dict(model.engine.serve_stats)

    def pcm(self, i):
        return np.concatenate(self.chunks[i])


def _submit_whole(q, which=range(len(TEXTS)), **kw):
    ids = _whole()
    return [q.submit(ids[j], language=LANGS[j], speaker=SPKS[j], **kw) for j in which]


_REF = {}


def _reference(model, tok, fmt=()):
    """generate(max_batch=2)'s codes of the five requests and serve_stream()'s PCM per request (once per format)"""
    if fmt not in _REF:
        kw = dict(input_ids=[torch.tensor([x]) for x in _whole()], languages=LANGS, speakers=SPKS,
                  non_streaming_mode=False, max_new_tokens=40, seed=7)
        codes, _ = model.generate(**kw, max_batch=2)
        chunks = {}
        for i, pcm, last in model.serve_stream(**kw, max_batch=2, first_chunk_frames=1, chunk_frames=8, **dict(fmt)):
            chunks.setdefault(i, []).append(pcm.cpu().numpy())
        _REF[fmt] = (codes, [np.concatenate(chunks[i]) for i in range(len(TEXTS))])
    return _REF[fmt]


def _same_codes(run, codes, what):
    assert sorted(run.codes) == list(range(len(codes))), what
    assert sorted(run.last) == list(range(len(codes))), what
    for i, c in enumerate(codes):
        assert torch.equal(run.codes[i], c), (what, i, run.codes[i].shape, c.shape)


# ------------------------------------------------------------------------------------------ 1. / 2. whole texts
def test_requests_submitted_ahead_match_generate_and_serve_stream(models):
    cfg, ms, tok = models
    model = ms["fp32"]
    codes, wavs = _reference(model, tok)
    assert len({c.shape[0] for c in codes}) > 1  # EOS-ragged
    q = _queue()
    assert _submit_whole(q) == [0, 1, 2, 3, 4]
    q.close()
    run = Run(model, q, max_batch=2, max_prompt=64, max_new_tokens=40, first_chunk_frames=1, chunk_frames=8)
    _same_codes(run, codes, "ahead")
    for i, w in enumerate(wavs):
        got = run.pcm(i)
        assert got.shape == w.shape, (i, got.shape, w.shape)
        err = float(np.abs(got - w).max()) if w.size else 0.0
        print(f"request {i}: {codes[i].shape[0]} frames, {len(run.chunks[i])} chunks, max |pcm - serve_stream| {err:.3g}")
        np.testing.assert_allclose(got, w, atol=2e-4, rtol=0, err_msg=f"request {i}")
        if codes[i].shape[0] >= 1 and int((codes[i][:, 0] != 0).sum()) == codes[i].shape[0]:
            assert run.chunks[i][0].shape[0] == FIRST, (i, run.chunks[i][0].shape)
    assert run.stats["held"] == 0 and run.stats["admitted"] == 5 and run.stats["retired"] == 5
    assert run.stats["requests"] == 5 and run.stats["slots"] == 2
    assert q.timed_out == () and q.rejected == {}
    _nothing_held(model, tok)


def test_requests_submitted_while_the_loop_runs_get_the_same_codes(models):
    cfg, ms, tok = models
    model = ms["fp32"]
    codes, _ = _reference(model, tok)
    q = _queue()
    _submit_whole(q, [0])
    sent = []

    def later(run, i, pcm, last):
        if not sent:  # request 0's first chunk has arrived: the loop is running
            assert i == 0
            sent.extend(_submit_whole(q, [1, 2, 3, 4]))
            q.close()
    run = Run(model, q, later, max_batch=2, max_prompt=64, max_new_tokens=40, first_chunk_frames=1, chunk_frames=8)
    assert sent == [1, 2, 3, 4]
    _same_codes(run, codes, "submitted later")
    _nothing_held(model, tok)


# ------------------------------------------------------------------------------------------ 3. open text, two deliveries
def _open_pair(model, how, sampling):
    """requests 0 (12 text tokens) and 1 (9) as open text.  "ahead": all text pushed and closed before the loop
    starts.  "trickled": request 0's text is there, request 1 gets one token per chunk received for request 0 and the
    rest when request 0 has ended.  "whole": the same two texts as whole-text requests."""
    parts = [_ids(12, 1200), _ids(9, 1201)]
    q = _queue()
    kw = dict(max_batch=2, max_prompt=64, max_new_tokens=31, first_chunk_frames=1, chunk_frames=2)
    if how == "whole":
        for j, p in enumerate(parts):
            q.submit(p[0], language=LANGS[j], speaker=SPKS[j], **sampling)
        q.close()
        return Run(model, q, **kw)
    for j, p in enumerate(parts):
        assert q.submit(p[1], language=LANGS[j], speaker=SPKS[j], open_text=True, **sampling) == j
    q.push(parts[0][2], 0)
    q.close_text(0)
    if how == "ahead":
        q.push(parts[1][2], 1)
        q.close_text(1)
        q.close()
        return Run(model, q, **kw)
    left = list(parts[1][2])

    def trickle(run, i, pcm, last):
        if i != 0 or not left:
            return
        n = len(left) if last else 1
        q.push(left[:n], 1)
        del left[:n]
        if not left:
            q.close_text(1)
            q.close()
    run = Run(model, q, trickle, **kw)
    assert not left
    return run


@pytest.mark.parametrize("sample", [False, True])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_open_text_trickled_equals_all_ahead(models, dtype, sample):
    cfg, ms, tok = models
    model = ms[dtype]
    sampling = dict(do_sample=sample, subtalker_dosample=sample)
    ahead = _open_pair(model, "ahead", sampling)
    trickled = _open_pair(model, "trickled", sampling)
    for i in (0, 1):
        print(f"{dtype} sample={sample} request {i}: {ahead.codes[i].shape[0]} frames; held row-frames "
              f"{trickled.stats['held']} of {trickled.stats['frames']} replays")
        assert ahead.codes[i].shape[0] >= 1
        assert torch.equal(trickled.codes[i], ahead.codes[i]), (dtype, sample, i)
        assert sorted(ahead.last) == sorted(trickled.last) == [0, 1]
    assert ahead.stats["held"] == 0 and trickled.stats["held"] > 0
    if dtype == "fp32":
        whole = _open_pair(model, "whole", sampling)
        for i in (0, 1):
            assert torch.equal(whole.codes[i], ahead.codes[i]), ("whole text", sample, i)
            a, w = ahead.pcm(i), whole.pcm(i)
            assert a.shape == w.shape
            np.testing.assert_allclose(a, w, atol=2e-4, rtol=0)
    _nothing_held(model, tok)


# ------------------------------------------------------------------------------------------ 4. first token only
def test_first_packet_from_the_first_text_token_while_another_request_runs(models):
    cfg, ms, tok = models
    model = ms["fp32"]
    parts = [_ids(12, 1200), _ids(9, 1201)]
    kw = dict(max_batch=2, max_prompt=64, max_new_tokens=31, first_chunk_frames=1, chunk_frames=2,
              do_sample=False, subtalker_dosample=False)
    run_kw = {k: kw.pop(k) for k in ("max_batch", "max_prompt", "max_new_tokens", "first_chunk_frames", "chunk_frames")}
    q = _queue()
    q.submit(parts[0][0], language=LANGS[0], speaker=SPKS[0], **kw)
    q.submit(parts[1][0], language=LANGS[1], speaker=SPKS[1], **kw)
    q.close()
    whole = Run(model, q, **run_kw)

    q = _queue()
    assert q.submit(parts[0][1], language=LANGS[0], speaker=SPKS[0], open_text=True, **kw) == 0   # head only
    assert q.submit(parts[1][0], language=LANGS[1], speaker=SPKS[1], **kw) == 1
    state = {}

    def on_chunk(run, i, pcm, last):
        if i == 1 and last:   # request 1 ran to its end while request 0 had no text beyond its first token
            state["at_end_of_1"] = [x for x in run.order if x[0] == 0]
            q.push(parts[0][2], 0)
            q.close_text(0)
            q.close()
    run = Run(model, q, on_chunk, **run_kw)
    assert state["at_end_of_1"] == [(0, FIRST, False)]   # exactly its one-frame first packet, nothing more
    assert whole.codes[1].shape[0] > 1
    for i in (0, 1):
        assert torch.equal(run.codes[i], whole.codes[i]), i
        assert run.pcm(i).shape == whole.pcm(i).shape
        np.testing.assert_allclose(run.pcm(i), whole.pcm(i), atol=2e-4, rtol=0)
    assert run.stats["held"] > 0 and sorted(run.last) == [0, 1]
    _nothing_held(model, tok)


# ------------------------------------------------------------------------------------------ 5. failure and output paths
def test_a_starved_request_is_retired_and_the_others_go_on(models):
    cfg, ms, tok = models
    model = ms["fp32"]
    parts = [_ids(12, 1200), _ids(9, 1201)]
    q = _queue(timeout=0.0)   # (returns at once: no test waits for a time limit)
    q.submit(parts[0][1], language=LANGS[0], speaker=SPKS[0], open_text=True, do_sample=False, subtalker_dosample=False)
    q.submit(parts[1][0], language=LANGS[1], speaker=SPKS[1], do_sample=False, subtalker_dosample=False)
    q.close()
    run = Run(model, q, max_batch=2, max_prompt=64, max_new_tokens=31, chunk_frames=2)
    assert q.timed_out == (0,) and q.rejected == {}
    assert [x[1:] for x in run.order if x[0] == 0] == [(FIRST, False), (0, True)]
    assert run.last == {0: True, 1: True} and run.codes[1].shape[0] > 1
    q.push([5], 0)   # a late push for the retired request is dropped, not an error
    _nothing_held(model, tok)


def test_cancel_while_decoding_and_while_queued(models):
    cfg, ms, tok = models
    model = ms["fp32"]
    codes, _ = _reference(model, tok)
    q = _queue()
    _submit_whole(q, [0, 1, 2, 3], do_sample=True)
    q.cancel(3)              # still queued when the loop starts: never started
    q.close()

    def on_chunk(run, i, pcm, last):
        if i == 0 and len(run.chunks[0]) == 1:
            q.cancel(0)      # decoding: retired with what it has
    run = Run(model, q, on_chunk, max_batch=2, max_prompt=64, max_new_tokens=40, chunk_frames=8)
    assert sorted(run.last) == [0, 1, 2, 3]
    assert run.order[0] == (3, 0, True) and 3 not in run.codes
    assert 1 <= run.codes[0].shape[0] <= codes[0].shape[0]
    assert torch.equal(run.codes[0], codes[0][:run.codes[0].shape[0]])
    for i in (1, 2):         # the others are untouched
        assert torch.equal(run.codes[i], codes[i]), i
    assert q.timed_out == () and q.rejected == {}
    assert run.stats["admitted"] == 3 and run.stats["requests"] == 4
    _nothing_held(model, tok)


def test_rejected_requests_do_not_end_the_loop(models):
    cfg, ms, tok = models
    model = ms["fp32"]
    codes, _ = _reference(model, tok)
    ids = _whole()
    q = _queue()
    long_ids = _ids(80, 1300)[0]
    vcp = {"ref_code": [torch.zeros(3, 16, dtype=torch.long)], "ref_spk_embedding": [torch.zeros(8)],
           "x_vector_only_mode": [False], "icl_mode": [True]}
    # (non-streaming mode puts the whole text into the prompt: 88 ids + the codec prefix against max_prompt = 64)
    bad = {q.submit(long_ids, language="english", non_streaming_mode=True): (ValueError, "max_prompt"),
           q.submit(ids[1], language="english", voice_clone_prompt=vcp): (NotImplementedError, "ICL"),
           q.submit(ids[1][:4], language="english", open_text=True, non_streaming_mode=True): (ValueError, "open_text")}
    good = q.submit(ids[3], language=LANGS[3], speaker=SPKS[3])
    bad[q.submit(ids[1], language="english", speaker="nobody")] = (NotImplementedError, "Speaker")
    bad[q.submit(ids[1], language="klingon")] = (NotImplementedError, "Language")
    bad[q.submit(ids[1][:3], language="english", open_text=True)] = (ValueError, "head")
    bad[q.submit(ids[1], language="english", temperature=0.0)] = (ValueError, "temperature")
    q.close()
    assert good == 3
    run = Run(model, q, max_batch=2, max_prompt=64, max_new_tokens=40, chunk_frames=8)
    assert sorted(run.last) == list(range(8))
    rej = q.rejected
    assert sorted(rej) == sorted(bad)
    for i, (kind, word) in bad.items():
        assert isinstance(rej[i], kind) and word in str(rej[i]), (i, rej[i])
        assert [x[1:] for x in run.order if x[0] == i] == [(0, True)], i
    # request 3 here is request 3 of the reference list: same ids, same Philox stream
    assert torch.equal(run.codes[good], codes[3])
    assert run.stats["admitted"] == 1 and run.stats["requests"] == 8
    with pytest.raises(ValueError, match="RequestQueue"):
        next(model.serve_live(object()))
    with pytest.raises(ValueError, match="64"):
        next(model.serve_live(_queue(), max_batch=65))
    _nothing_held(model, tok)


def test_16khz_s16_chunks_concatenate_to_serve_streams(models):
    cfg, ms, tok = models
    model = ms["fp32"]
    fmt = (("sample_rate", 16000), ("pcm_format", "s16"))
    codes, wavs = _reference(model, tok, fmt)
    q = _queue()
    _submit_whole(q)
    q.close()
    run = Run(model, q, max_batch=2, max_prompt=64, max_new_tokens=40, first_chunk_frames=1, chunk_frames=8, **dict(fmt))
    _same_codes(run, codes, "s16")
    for i, w in enumerate(wavs):
        got = run.pcm(i)
        assert got.dtype == np.int16 and w.dtype == np.int16
        assert got.shape == w.shape, (i, got.shape, w.shape)
        print(f"request {i}: {got.shape[0]} samples at 16 kHz, {int((got != w).sum())} differ from serve_stream's")
        assert np.array_equal(got, w), i
    _nothing_held(model, tok)


def test_prefix_cache_hits_in_a_live_run(models):
    from cases import instruct_ids
    from qwen_tts import PrefixCache
    cfg, ms, tok = models
    model = ms["fp32"]
    ins = instruct_ids(7, 902)[0].tolist()
    runs = []
    for cache in (None, PrefixCache()):
        q = _queue()
        for j in range(3):
            q.submit(_whole()[j], language=LANGS[j], speaker=SPKS[j], instruct_ids=ins)
        q.close()
        runs.append(Run(model, q, max_batch=1, max_prompt=64, max_new_tokens=40, chunk_frames=8, prefix_cache=cache))
    s = cache.stats
    assert (s["hits"], s["misses"], s["stores"]) == (2, 1, 1), s
    for i in range(3):
        assert runs[0].codes[i].shape[0] >= 1
        assert torch.equal(runs[1].codes[i], runs[0].codes[i]), i
    _nothing_held(model, tok)


# ------------------------------------------------------------------------------------------ the wrapper
def test_wrapper_takes_strings(models):
    """Qwen3TTSModel.request_queue() + serve_live(): submit(text=...) / push_text are the model-level requests of the
    ids the strings tokenize to."""
    from qwen_tts import Qwen3TTSModel
    from qwen_tts.text import FallbackProcessor
    cfg, ms, tok = models
    tts = Qwen3TTSModel(ms["fp32"], FallbackProcessor())
    greedy = dict(do_sample=False, subtalker_dosample=False)
    pieces = [" world, this is", " text that arrives"]
    q = tts.request_queue(timeout=5.0)
    assert q.submit(text="a whole sentence", speaker="vivian", language="english", **greedy) == 0
    assert q.submit(text="hello", speaker="dylan", language="english", open_text=True, **greedy) == 1
    for p in pieces:
        q.push_text(p, 1)
    q.close_text(1)
    q.close()
    with pytest.raises(ValueError, match="either"):
        q.submit()
    got, last = {}, {}
    for i, pcm, sr, is_last in tts.serve_live(q, max_batch=2, max_prompt=64, max_new_tokens=14, seed=7):
        assert sr == 24000 and isinstance(pcm, np.ndarray) and pcm.dtype == np.float32
        got.setdefault(i, []).append(pcm)
        last[i] = is_last
    assert last == {0: True, 1: True}
    # the same requests by ids, at the model level
    ids = lambda t: tts._tokenize_texts([t])[0][0].tolist()  # noqa: E731
    q2 = _queue()
    q2.submit(ids(tts._build_assistant_text("a whole sentence")), speaker="vivian", language="english",
              non_streaming_mode=True, **greedy)
    q2.submit(ids("<|im_start|>assistant\nhello"), speaker="dylan", language="english", open_text=True, **greedy)
    for p in pieces:
        q2.push(ids(p), 1)
    q2.close_text(1)
    q2.close()
    run = Run(ms["fp32"], q2, max_batch=2, max_prompt=64, max_new_tokens=14)
    for i in (0, 1):
        a, r = np.concatenate(got[i]), run.pcm(i)
        assert a.shape == r.shape and a.shape[0] >= FIRST, (i, a.shape, r.shape)
        np.testing.assert_allclose(a, r, atol=2e-4, rtol=0)
    _nothing_held(ms["fp32"], tok)
