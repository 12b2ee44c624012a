"""TTSModel.stream(text_feed=...): text fed while the audio is generated, tiny-customvoice.

1. how the text is cut into pieces does not matter (codes and trailing rows bit-equal, PCM within 2e-4);
2. the rows the feed writes are engine.text_proj's, bit for bit, for pieces of 1, 5 and 16 ids;
3. a closed feed decodes the utterance of the whole-text call (fp32: equal codes; trailing rows of both paths against
   an fp64 recomputation from the stored operands, printed);
4. the first packet needs the head's one text token; 5. a starved loop hands out all audio that exists, then raises
   and leaves nothing held; 6. rows that all reached end-of-speech end the stream although their text never closed;
7. the combinations that are not served are refused on the first next(); 8. stream() without a feed is untouched;
9. frames are issued and chunks handed out in one literal order, with a feed and without.

Every feed has a timeout of at most 5 s and the one producer thread is joined with a timeout, so a bug ends as a
failure, not as a stalled process; the starvation cases use timeout=0, which returns at once.

measured on the MI355X (case 3, fp32, the 20 trailing rows of B = 3, max |row - fp64| over them; the tiny preset's
rows are of magnitude ~1e-2):
  feed path (16-row decode GEMV)  2.28e-09    whole-text path (one batched projection)  2.28e-09
"""
import contextlib
import os
import threading
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIRST = 1920 - 555  # samples of a one-frame first packet


@pytest.fixture(scope="module")
def models():
    """cfg, weights, {fp32, bf16: plain model; ragged: fp32 model whose EOS row is the donor's (the recipe of
    test_gpu_serve_stream.py), so that rows reach end-of-speech at different frames}, tokenizer"""
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
    ms = {"fp32": TTSModel(cfg, W, dtype="fp32"), "bf16": TTSModel(cfg, W, dtype="bf16"),
          "ragged": TTSModel(cfg, We, dtype="fp32")}
    for m in ms.values():
        m.load_speech_tokenizer(tok)
    return cfg, W, ms, tok


LANGS, SPKS = ["auto", "english", "japanese"], ["", None, "dylan"]  # the cv_b3_auto_nospk recipe


def _ids(n, seed):
    """(head = 3 role ids + first text id, the other n - 1 text ids, the whole-text ids with the template suffix)"""
    from cases import text_ids
    ids = text_ids(n, seed)[0].tolist()
    return ids[:4], ids[4:-5], ids


def _feed(rows, timeout):
    from qwen_tts import TextFeed
    assert timeout <= 5.0
    return TextFeed(rows=rows, timeout=timeout)


@contextlib.contextmanager
def _held(model):
    """the sessions the block's requests decoded in (recorded as the engine releases them)"""
    got, eng = [], model.engine
    orig = eng.release

    def rel(sessions):
        got.extend(sessions)
        orig(sessions)
    eng.release = rel
    try:
        yield got
    finally:
        del eng.release


def _nothing_held(model, tok):
    torch.cuda.synchronize()
    assert not any(s.busy for s in model.engine.all_sessions())
    dec = tok.model
    pools = list(dec._slots.values()) + list(getattr(dec, "_row_slots", {}).values())
    assert not any(sl.busy for pool in pools for sl in pool)


def _row_codes(s, eos):
    """per row: the final frames' codes, int64 [F_b, 16] (cut at the row's end-of-speech token)"""
    codes, step = s.codes.cpu(), s.step.cpu()
    out = []
    for b in range(s.B):
        F = int(step[b])
        hit = (codes[b, :F + 1, 0] == eos).nonzero()
        F = int(hit[0]) if hit.numel() else F
        out.append(codes[b, :F].long())
    return out


class _Collect:
    """chunks per row of a (row, pcm, last) stream; checks that each row's one last=True comes last"""

    def __init__(self, B):
        self.B, self.chunks, self.last = B, [[] for _ in range(B)], [False] * B

    def add(self, b, pcm, last):
        assert not self.last[b], (b, "a chunk after last=True")
        self.chunks[b].append(pcm.cpu().numpy())
        self.last[b] = bool(last)

    def heard(self, b):
        """frames of row b handed out so far (n frames of a reference chunk give 1920 n - 555 samples)"""
        n = sum(c.shape[0] for c in self.chunks[b])
        return (n + 555) // 1920 if n else 0

    def pcm(self, b):
        return np.concatenate(self.chunks[b]) if self.chunks[b] else np.zeros(0, np.float32)

    def complete(self):
        assert all(self.last), self.last


def _stream(model, heads, feed, **kw):
    kw.setdefault("languages", LANGS[:len(heads)])
    kw.setdefault("speakers", SPKS[:len(heads)])
    return model.stream(input_ids=[torch.tensor([h]) for h in heads], non_streaming_mode=False, text_feed=feed, **kw)


# ------------------------------------------------------------------------------------------ 1. pieces do not matter
def _deliver(model, how, heads, tails, **kw):
    """one request whose tails[b] reach row b in the way `how` names; returns (collector, codes, trailing)"""
    B = len(heads)
    feed = _feed(B, 5.0)
    col = _Collect(B)
    eos = model.engine.tc["codec_eos_token_id"]
    th = None
    with _held(model) as held:
        if how == "ahead":       # everything pushed and closed before the first next()
            for b in range(B):
                feed.push(tails[b], row=b)
                feed.close(row=b)
            for b, pcm, last in _stream(model, heads, feed, **kw):
                col.add(b, pcm, last)
        elif how == "by_one":    # one token per push from the consumer loop, two tokens ahead of the frames
            sent = [0] * B

            def more(b):
                while sent[b] < min(col.heard(b) + 2, len(tails[b])):
                    feed.push([tails[b][sent[b]]], row=b)
                    sent[b] += 1
                if sent[b] == len(tails[b]) and not feed.closed(b):
                    feed.close(row=b)
            for b in range(B):
                more(b)
            for b, pcm, last in _stream(model, heads, feed, first_chunk_frames=1, chunk_frames=2, **kw):
                col.add(b, pcm, last)
                more(b)
        elif how == "ragged":    # ragged pieces: an empty one, and one of 19 tokens (two appends)
            cuts = [[2, 0, 19, 1, 100], [0, 3, 100], [1, 1, 0, 4, 100]]
            pieces = []
            for b in range(B):
                ps, at = [], 0
                for c in cuts[b]:
                    ps.append(tails[b][at:at + c])
                    at += c
                assert at >= len(tails[b])
                pieces.append(ps)
            assert any(len(p) == 19 for p in pieces[0]) and any(len(p) == 0 for ps in pieces for p in ps)

            sent = [0] * B

            def nxt(b):  # whole pieces, until the row is two tokens ahead of what was heard
                while pieces[b] and sent[b] < col.heard(b) + 2:
                    sent[b] += len(pieces[b][0])
                    feed.push(pieces[b].pop(0), row=b)
                if not pieces[b] and not feed.closed(b):
                    feed.close(row=b)
            for b in range(B):
                nxt(b)
            for b, pcm, last in _stream(model, heads, feed, first_chunk_frames=1, chunk_frames=4, **kw):
                col.add(b, pcm, last)
                nxt(b)
        elif how == "thread":    # a producer thread with short sleeps
            def producer():
                for at in range(0, max(len(t) for t in tails), 3):
                    for b in range(B):
                        if at < len(tails[b]):
                            feed.push(tails[b][at:at + 3], row=b)
                        if at + 3 >= len(tails[b]) and not feed.closed(b):
                            feed.close(row=b)
                    time.sleep(0.002)
            th = threading.Thread(target=producer)
            th.start()
            try:
                for b, pcm, last in _stream(model, heads, feed, **kw):
                    col.add(b, pcm, last)
            finally:
                th.join(5.0)
            assert not th.is_alive()
        else:
            raise AssertionError(how)
    col.complete()
    assert len(held) == 1
    s = held[0]
    torch.cuda.synchronize()
    return col, _row_codes(s, eos), s.trailing.clone()


@pytest.mark.parametrize("sample", [False, True])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_pieces_do_not_matter(models, dtype, sample):
    cfg, _, ms, tok = models
    model = ms[dtype]
    parts = [_ids(n, 900 + j) for j, n in enumerate([24, 4, 7])]
    heads, tails = [p[0] for p in parts], [p[1] for p in parts]
    kw = dict(max_new_tokens=31, do_sample=sample, subtalker_dosample=sample, seed=7)
    ref = None
    for how in ("ahead", "by_one", "ragged", "thread"):
        col, codes, trailing = _deliver(model, how, heads, tails, **kw)
        if ref is None:
            ref = (col, codes, trailing)
            assert all(c.shape[0] >= 1 for c in codes)
            continue
        for b in range(len(heads)):
            assert torch.equal(codes[b], ref[1][b]), (how, b)
            a, r = col.pcm(b), ref[0].pcm(b)
            assert a.shape == r.shape, (how, b, a.shape, r.shape)
            err = float(np.abs(a - r).max()) if a.size else 0.0
            print(f"{dtype} sample={sample} {how} row {b}: {codes[b].shape[0]} frames, {len(col.chunks[b])} chunks, "
                  f"max |pcm diff| {err:.3g}")
            np.testing.assert_allclose(a, r, atol=2e-4, rtol=0, err_msg=f"{how} row {b}")
        assert torch.equal(trailing.view(torch.int32), ref[2].view(torch.int32)), how
    _nothing_held(model, tok)


# ------------------------------------------------------------------------------------------ 2. the existing projection
@pytest.mark.parametrize("n", [1, 5, 16])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_rows_are_text_proj_rows(models, dtype, n):
    cfg, _, ms, tok = models
    model = ms[dtype]
    head, tail, _ = _ids(n + 1, 40 + n)
    assert len(tail) == n
    feed = _feed(1, 0.0)
    feed.push(tail, row=0)
    feed.close(row=0)
    with _held(model) as held:
        it = _stream(model, [head], feed, max_new_tokens=24, do_sample=False, subtalker_dosample=False)
        b, pcm, last = next(it)       # the feed was drained, and its rows queued, before this first packet
        assert pcm.shape[0] == FIRST and not last
        it.close()
    torch.cuda.synchronize()
    s = held[0]
    got = s.trailing[0, :n + 1].contiguous()
    piece = model.engine.text_proj(tail)  # the piece on its own: the existing n <= 16 branch
    assert torch.equal(got[:n].view(torch.int32), piece.view(torch.int32))
    end = model.engine.text_proj([cfg["tts_eos_token_id"]])
    assert torch.equal(got[n:].view(torch.int32), end.view(torch.int32))
    pad = s.pad_embed.view(1, -1).expand(s.trailing.shape[1] - n - 1, -1)
    assert torch.equal(s.trailing[0, n + 1:], pad)  # positions after the end-of-text one stay pad
    _nothing_held(model, tok)


# ------------------------------------------------------------------------------------------ 3. the whole-text utterance
def _proj64(W, ids):
    g = lambda k: W[k].double()  # noqa: E731
    x = g("talker.model.text_embedding.weight")[torch.as_tensor(ids)]
    h = x @ g("talker.text_projection.linear_fc1.weight").T + g("talker.text_projection.linear_fc1.bias")
    h = h * torch.sigmoid(h)
    return h @ g("talker.text_projection.linear_fc2.weight").T + g("talker.text_projection.linear_fc2.bias")


def test_closed_feed_is_the_whole_text_utterance(models):
    from cases import gen_kwargs, make_inputs, talker_cases
    cfg, W, ms, tok = models
    model = ms["fp32"]
    key = "cv_b3_auto_nospk"
    case = talker_cases()[key]
    ids, _, _, _ = make_inputs(case, list(talker_cases()).index(key), cfg["talker_config"]["hidden_size"])
    kw = gen_kwargs(case)
    want, _ = model.generate(input_ids=ids, languages=case["languages"], speakers=case["speakers"],
                             non_streaming_mode=False, **kw)
    whole = model.build_prompts(ids, case["languages"], case["speakers"], None, False)[2]
    rows = [i[0].tolist() for i in ids]
    feed = _feed(len(rows), 5.0)
    for b, r in enumerate(rows):
        feed.push(r[4:-5], row=b)
        feed.close(row=b)
    col = _Collect(len(rows))
    with _held(model) as held:
        for b, pcm, last in _stream(model, [r[:4] for r in rows], feed, languages=case["languages"],
                                    speakers=case["speakers"], **kw):
            col.add(b, pcm, last)
    col.complete()
    s = held[0]
    got = _row_codes(s, model.engine.tc["codec_eos_token_id"])
    e_feed = e_whole = 0.0
    for b, r in enumerate(rows):
        t = r[4:-5] + [cfg["tts_eos_token_id"]]
        n = min(len(t), case["max_new_tokens"] - 1)
        ref = _proj64(W, t[:n])
        e_feed = max(e_feed, float((s.trailing[b, :n].double().cpu() - ref).abs().max()))
        e_whole = max(e_whole, float((whole[b, :n].double().cpu() - ref).abs().max()))
    print(f"trailing rows vs fp64: feed path max |err| {e_feed:.3g}, whole-text path max |err| {e_whole:.3g}")
    assert np.isfinite(e_feed)
    for b in range(len(rows)):
        assert torch.equal(got[b], want[b]), b
    _nothing_held(model, tok)


# ------------------------------------------------------------------------------------------ 4. / 5. starvation
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_one_token_is_enough_for_the_first_packet(models, dtype):
    from qwen_tts import TextFeedTimeout
    cfg, _, ms, tok = models
    model = ms[dtype]
    B = 3
    heads = [_ids(2, 60 + b)[0] for b in range(B)]
    assert all(len(h) == 4 for h in heads)
    feed = _feed(B, 0.0)
    it = _stream(model, heads, feed, max_new_tokens=24, do_sample=False, subtalker_dosample=False,
                 first_chunk_frames=1)
    got = [next(it) for _ in range(B)]  # the first report: one packet per row
    assert sorted(b for b, _, _ in got) == list(range(B))
    for b, pcm, last in got:
        assert pcm.shape[0] == FIRST and not last, (b, pcm.shape, last)
    with pytest.raises(TextFeedTimeout):
        next(it)
    _nothing_held(model, tok)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_starvation_flushes_then_raises(models, dtype):
    from qwen_tts import TextFeedTimeout
    cfg, _, ms, tok = models
    model = ms[dtype]
    B, m = 3, 5
    parts = [_ids(1 + m, 70 + b) for b in range(B)]
    heads = [p[0] + p[1] for p in parts]  # 3 role ids + 1 + m text ids
    assert all(len(h) == 4 + m for h in heads)
    kw = dict(max_new_tokens=24, do_sample=False, subtalker_dosample=False, first_chunk_frames=1, chunk_frames=48)
    eos = model.engine.tc["codec_eos_token_id"]
    # the closed-feed run of the same heads
    feed = _feed(B, 0.0)
    for b in range(B):
        feed.close(row=b)
    with _held(model) as held:
        for _ in _stream(model, heads, feed, **kw):
            pass
    torch.cuda.synchronize()
    closed = held[0].codes[:, :m].cpu().clone()
    assert all(c.shape[0] > m for c in _row_codes(held[0], eos))
    # the open one
    feed = _feed(B, 0.0)
    col = _Collect(B)
    with _held(model) as held:
        with pytest.raises(TextFeedTimeout):
            for b, pcm, last in _stream(model, heads, feed, **kw):
                col.add(b, pcm, last)
    torch.cuda.synchronize()
    for b in range(B):
        assert not col.last[b]
        assert col.pcm(b).shape[0] == 1920 * m - 555, (b, col.pcm(b).shape)
    assert torch.equal(held[0].codes[:, :m].cpu(), closed)
    _nothing_held(model, tok)


# ------------------------------------------------------------------------------------------ 6. end-of-speech, open feed
def test_end_of_speech_beats_an_open_feed(models):
    cfg, _, ms, tok = models
    model = ms["ragged"]
    B, cap = 3, 47
    parts = [_ids(cap + 2, 80 + b) for b in range(B)]
    heads, tails = [p[0] for p in parts], [p[1] for p in parts]
    kw = dict(max_new_tokens=cap + 1, do_sample=False, subtalker_dosample=False)
    eos = model.engine.tc["codec_eos_token_id"]

    def run(n_text):
        feed = _feed(B, 0.0)
        for b in range(B):
            feed.push(tails[b][:n_text], row=b)  # never closed
        col = _Collect(B)
        with _held(model) as held:
            for b, pcm, last in _stream(model, heads, feed, **kw):
                col.add(b, pcm, last)
        col.complete()
        return col, _row_codes(held[0], eos)

    # with text for every frame, every row ends on its own end-of-speech token, at different frames
    col_a, codes_a = run(cap)
    F = [c.shape[0] for c in codes_a]
    print("frames per row:", F)
    assert max(F) < cap and len(set(F)) > 1, F
    # with just the text the longest row needs, the loop starves afterwards, finds every row finished and ends
    col_b, codes_b = run(max(F))
    for b in range(B):
        assert torch.equal(codes_a[b], codes_b[b]), b
        a, r = col_b.pcm(b), col_a.pcm(b)
        assert a.shape == r.shape, (b, a.shape, r.shape)
        np.testing.assert_allclose(a, r, atol=2e-4, rtol=0, err_msg=f"row {b}")
    _nothing_held(model, tok)


# ------------------------------------------------------------------------------------------ 7. rejections
def test_rejections(models):
    from cases import gen_kwargs, make_inputs, talker_cases
    cfg, _, ms, tok = models
    model = ms["fp32"]
    head = _ids(3, 5)[0]
    kw = dict(languages=["english"], speakers=["vivian"], max_new_tokens=6)
    one = [torch.tensor([head])]

    def first(**over):
        a = dict(input_ids=one, non_streaming_mode=False, text_feed=_feed(1, 0.0), **kw)
        a.update(over)
        return next(iter(model.stream(**a)))

    key = "icl_b2"
    case = dict(talker_cases()[key], max_new_tokens=6)
    ids, ins, vcp, ref_ids = make_inputs(case, list(talker_cases()).index(key), cfg["talker_config"]["hidden_size"])
    assert any(r is not None for r in vcp["ref_code"])
    with pytest.raises(NotImplementedError, match="ICL"):
        first(input_ids=[i[:, :4] for i in ids], ref_ids=ref_ids, voice_clone_prompt=vcp, speakers=case["speakers"],
              languages=case["languages"], text_feed=_feed(2, 0.0))
    with pytest.raises(NotImplementedError, match="max_batch"):
        first(max_batch=1)
    with pytest.raises(NotImplementedError, match="left_context"):
        first(left_context=100)
    with pytest.raises(ValueError, match="non_streaming_mode"):
        first(non_streaming_mode=True)
    with pytest.raises(ValueError, match="rows"):
        first(text_feed=_feed(2, 0.0))
    with pytest.raises(ValueError, match="head"):
        first(input_ids=[torch.tensor([head[:3]])])
    _nothing_held(model, tok)
    # at push (the host test covers the feed alone): after close, and a row out of range, with a live request
    feed = _feed(1, 0.0)
    feed.close(row=0)
    for _ in model.stream(input_ids=one, non_streaming_mode=False, text_feed=feed, **kw):
        pass
    with pytest.raises(ValueError, match="closed"):
        feed.push([1], row=0)
    with pytest.raises(ValueError, match="out of range"):
        feed.push([1], row=1)
    _nothing_held(model, tok)


def test_text_past_the_frame_cap_is_dropped(models):
    cfg, _, ms, tok = models
    model = ms["fp32"]
    head, tail, _ = _ids(30, 6)
    feed = _feed(1, 0.0)
    feed.push(tail, row=0)  # 29 tokens for 5 positions
    feed.close(row=0)
    col = _Collect(1)
    with _held(model) as held:
        for b, pcm, last in _stream(model, [head], feed, max_new_tokens=6, do_sample=False, subtalker_dosample=False):
            col.add(b, pcm, last)
    col.complete()
    torch.cuda.synchronize()
    s = held[0]
    assert s.trailing.shape[1] == 6
    assert torch.equal(s.trailing[0, :5].view(torch.int32), model.engine.text_proj(tail[:5]).view(torch.int32))
    assert torch.equal(s.trailing[0, 5], s.pad_embed)  # no frame reads it: never written
    _nothing_held(model, tok)


# ------------------------------------------------------------------------------------------ 8. the scalar path
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_stream_without_a_feed_is_untouched(models, dtype):
    from cases import make_inputs, talker_cases
    cfg, _, ms, tok = models
    model = ms[dtype]
    case = talker_cases()["cv_b3_auto_nospk"]
    ids, _, _, _ = make_inputs(case, 2, cfg["talker_config"]["hidden_size"])
    kw = dict(input_ids=ids, languages=case["languages"], speakers=case["speakers"], non_streaming_mode=False,
              max_new_tokens=14, do_sample=True, subtalker_dosample=True, seed=11, first_chunk_frames=1,
              chunk_frames=4)

    def plain():
        col = _Collect(3)
        with _held(model) as held:
            for b, pcm, last in model.stream(**kw):
                col.add(b, pcm, last)
        col.complete()
        torch.cuda.synchronize()
        return _row_codes(held[0], model.engine.tc["codec_eos_token_id"]), [col.pcm(b) for b in range(3)]

    before = plain()
    rows = [i[0].tolist() for i in ids]
    feed = _feed(3, 5.0)
    for b, r in enumerate(rows):
        feed.push(r[4:-5], row=b)
        feed.close(row=b)
    for _ in _stream(model, [r[:4] for r in rows], feed, languages=case["languages"], speakers=case["speakers"],
                     max_new_tokens=14, do_sample=True, subtalker_dosample=True, seed=11):
        pass
    after = plain()
    assert all(torch.equal(a, b) and a.shape[0] >= 1 for a, b in zip(before[0], after[0]))
    for a, b in zip(before[1], after[1]):
        assert a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))
    _nothing_held(model, tok)


# ------------------------------------------------------------------------------------------ 9. the order of issue
def _a(lo, hi):
    return [("all", k) for k in range(lo, hi + 1)]


# decode_iter's contract for max_new_tokens=12 (11 frames), chunk_frames=4, growing chunks: the interval starts at
# max(first - 1, 1) = 1 and doubles to 2 and then 4; frame 11 is the cap, so it is handed out by the final yield alone
SCHEDULES = {
    1: [("cp", 1), ("yield", 1), ("talk", 1)] + _a(2, 3) + [("yield", 3)] + _a(4, 7) + [("yield", 7)] + _a(8, 11)
       + [("yield", 11)],
    2: _a(1, 2) + [("yield", 2)] + _a(3, 4) + [("yield", 4)] + _a(5, 8) + [("yield", 8)] + _a(9, 11) + [("yield", 11)],
}


@pytest.mark.parametrize("first", [1, 2])
def test_frame_schedule_is_the_same_with_and_without_a_gate(models, first, monkeypatch):
    """The order in which stream() issues frame replays and hands out chunks, plain and with a feed that holds the
    whole text from the start: ("cp" | "talk" | "all", key bound - prompt length) per _run_frame call, ("yield", frames
    heard so far) per report.  Both equal the literal schedule."""
    import qwen_tts.talker as T
    from cases import make_inputs, talker_cases
    cfg, _, ms, tok = models
    model = ms["fp32"]
    case = talker_cases()["cv_b3_auto_nospk"]
    ids, _, _, _ = make_inputs(case, 2, cfg["talker_config"]["hidden_size"])
    rows = [i[0].tolist() for i in ids]
    kw = dict(languages=case["languages"], speakers=case["speakers"], first_chunk_frames=first, chunk_frames=4,
              max_new_tokens=12, ignore_eos=True, do_sample=False, subtalker_dosample=False)
    trace = []
    orig = T.TalkerEngine._run_frame

    def run_frame(self, s, keys, use_graph=True, part="all"):
        trace.append((part, keys - s.P))
        orig(self, s, keys, use_graph, part)
    monkeypatch.setattr(T.TalkerEngine, "_run_frame", run_frame)

    def run(it):
        del trace[:]
        col = _Collect(3)
        for b, pcm, last in it:
            col.add(b, pcm, last)
            ev = ("yield", col.heard(b))
            if trace[-1] != ev:  # one report hands a chunk to every row
                trace.append(ev)
        col.complete()
        return list(trace)

    plain = run(model.stream(input_ids=ids, non_streaming_mode=False, **kw))
    feed = _feed(3, 5.0)
    for b, r in enumerate(rows):
        feed.push(r[4:-5], row=b)
        feed.close(row=b)
    fed = run(_stream(model, [r[:4] for r in rows], feed, **kw))
    print("plain", plain)
    print("fed  ", fed)
    assert plain == fed
    assert plain == SCHEDULES[first]
    _nothing_held(model, tok)


# ------------------------------------------------------------------------------------------ the wrapper
def test_wrapper_push_text(models):
    """Qwen3TTSModel.stream(text=[first piece], text_feed=feed) with pieces pushed as strings is the model-level
    stream of the ids each piece tokenizes to on its own."""
    from qwen_tts import Qwen3TTSModel
    from qwen_tts.text import FallbackProcessor
    cfg, _, ms, tok = models
    proc = FallbackProcessor()
    tts = Qwen3TTSModel(ms["fp32"], proc)
    pieces = [" world, this is", "", " text that arrives", " in pieces"]
    kw = dict(max_new_tokens=14, do_sample=False, subtalker_dosample=False)
    feed = tts.text_feed(rows=1, timeout=5.0)
    for p in pieces:
        feed.push_text(p, row=0)
    feed.close(row=0)
    got, lasts = [], []
    for i, pcm, sr, last in tts.stream(text=["hello"], speaker=["vivian"], language=["english"], text_feed=feed, **kw):
        assert i == 0 and sr == 24000 and isinstance(pcm, np.ndarray)
        got.append(pcm)
        lasts.append(last)
    assert lasts[-1] and not any(lasts[:-1])
    ids = lambda t: proc(text=t)["input_ids"][0].tolist()  # noqa: E731
    head = ids("<|im_start|>assistant\nhello")
    assert len(head) == 4
    feed = _feed(1, 5.0)
    feed.push([x for p in pieces if p for x in ids(p)], row=0)
    feed.close(row=0)
    col = _Collect(1)
    for b, pcm, last in _stream(ms["fp32"], [head], feed, languages=["english"], speakers=["vivian"], **kw):
        col.add(b, pcm, last)
    col.complete()
    a, r = np.concatenate(got), col.pcm(0)
    assert a.shape == r.shape and a.shape[0] > FIRST
    np.testing.assert_allclose(a, r, atol=2e-4, rtol=0)
    with pytest.raises(ValueError, match="non_streaming_mode"):  # an explicit non-streaming request is refused
        next(iter(tts.stream(text=["hello"], speaker=["vivian"], language=["english"], non_streaming_mode=True,
                             text_feed=tts.text_feed(1, 0.0), **kw)))
    _nothing_held(ms["fp32"], tok)
