"""CPU-only: the host side of live serving -- qwen_tts.RequestQueue, and the slot table of a run whose
requests arrive while it decodes and whose rows can be held out of a replay (talker.LiveSlots), the account of the rows'
trailing text (talker.TextAccount, and TextGate on top of it) and the loop's per-row record (talker.LiveRow)."""
import random
import threading

import pytest


def _queue(timeout=5.0):
    from qwen_tts.live import RequestQueue
    assert timeout <= 5.0
    return RequestQueue(timeout=timeout)


def test_ids_are_consecutive_and_requests_arrive_once_in_order():
    q = _queue()
    assert [q.submit([1, 2, 3, 4 + i]) for i in range(3)] == [0, 1, 2]
    new, text, closed_text, cancelled, closed = q.drain()
    assert [r.id for r in new] == [0, 1, 2] and [r.input_ids[-1] for r in new] == [4, 5, 6]
    assert text == {} and closed_text == [] and cancelled == [] and closed is False
    assert new[0].sampling["temperature"] == 0.9 and new[0].sampling["seed"] is None and not new[0].open_text
    i = q.submit([9, 9, 9, 9], open_text=True, speaker="dylan", language="english", frame_cap=7, do_sample=False, seed=5)
    assert i == 3
    (r,), *_ = q.drain()
    assert (r.id, r.open_text, r.speaker, r.language, r.frame_cap) == (3, True, "dylan", "english", 7)
    assert r.sampling["do_sample"] is False and r.sampling["seed"] == 5 and r.sampling["top_k"] == 50
    assert q.drain()[0] == []
    with pytest.raises(TypeError):
        q.submit([1, 2, 3, 4], temperatur=0.5)
    with pytest.raises(ValueError):
        q.submit([1, 2, 3, 4], frame_cap=0)


def test_a_requests_step_is_the_tuple_of_prosody_steps():
    """speed, pitch and gain reach the loop as prosody.steps()'s (S, T, db), checked at submit"""
    from qwen_tts import prosody as P
    from qwen_tts.live import LiveRequest
    q = _queue()
    vals = ((None, None, None), (1.0, 0, 0.0), (1.25, None, None), (1.5, 2, None), (None, -7, 6), (0.8, 3, -4.5),
            (None, None, 16))
    for s, p, d in vals:
        q.submit([1, 2, 3, 4], speed=s, pitch=p, volume_gain_db=d)
    new = q.drain()[0]
    assert LiveRequest(0, [1]).step == (100, 100, 0.0)
    for r, (s, p, d) in zip(new, vals):
        assert type(r.step) is tuple and r.step == (P.steps(s, p, d, 1) or [(100, 100, 0.0)])[0], r.id
    assert [r.step for r in new[:5]] == [(100, 100, 0.0), (100, 100, 0.0), (125, 125, 0.0), (150, 134, 0.0),
                                         (100, 150, 6.0)]
    for bad in (dict(pitch=13), dict(volume_gain_db=17), dict(pitch=True), dict(speed=0.5, pitch=2), dict(speed=2.5),
                dict(speed=[1.0, 1.0])):
        with pytest.raises(ValueError):
            q.submit([1, 2, 3, 4], **bad)
    assert q.drain()[0] == []  # a refused submit queues nothing and takes no id
    assert q.submit([1, 2, 3, 4]) == len(vals)


def test_push_before_admission_and_no_push_after_close_text():
    import torch
    q = _queue()
    whole, fed = q.submit([1, 2, 3, 4, 5]), q.submit([1, 2, 3, 4], open_text=True)
    q.push([10, 11], fed)          # nobody has drained the request yet, let alone admitted it
    q.push(torch.tensor([[12]]), fed)
    q.push([], fed)
    q.push(13, fed)
    new, text, closed_text, _, _ = q.drain()
    assert [r.id for r in new] == [whole, fed] and text == {fed: [10, 11, 12, 13]} and closed_text == []
    q.push([14], fed)
    q.close_text(fed)
    q.close_text(fed)              # twice is harmless, and reported once
    _, text, closed_text, _, _ = q.drain()
    assert text == {fed: [14]} and closed_text == [fed]
    with pytest.raises(ValueError, match="closed"):
        q.push([15], fed)
    with pytest.raises(ValueError, match="whole text"):
        q.push([15], whole)
    with pytest.raises(ValueError, match="whole text"):
        q.close_text(whole)
    with pytest.raises(ValueError, match="no request"):
        q.push([15], 2)
    assert q.drain()[1] == {}
    with pytest.raises(ValueError, match="processor"):
        q.push_text("hello", fed)


def test_cancel_close_and_the_loops_records():
    q = _queue()
    a, b, c = q.submit([1, 2, 3, 4]), q.submit([1, 2, 3, 4], open_text=True), q.submit([1, 2, 3, 4], open_text=True)
    q.cancel(a)
    q.cancel(a)
    assert q.drain()[3] == [a]
    assert q.closed is False
    q.close()
    q.close()
    assert q.closed is True
    with pytest.raises(ValueError, match="closed"):
        q.submit([1, 2, 3, 4])
    assert q.drain()[4] is True
    q.push([7], b)                                    # text still flows after close()
    assert q.drain()[1] == {b: [7]}
    assert q.timed_out == () and q.rejected == {}
    err = ValueError("too long")
    q.over(a)
    q.over(b, timed_out=True)
    q.over(c, rejected=err)
    assert q.timed_out == (b,) and q.rejected == {c: err}
    q.rejected[99] = err                              # a copy: the record itself is read-only
    assert 99 not in q.rejected
    q.push([8], b)                                    # a request that is over: dropped, no error
    q.close_text(c)
    q.cancel(a)
    assert q.drain()[:4] == ([], {}, [], [])
    with pytest.raises(ValueError):
        _queue(timeout=-1)


def test_wait_sees_what_happened_since_the_last_drain():
    q = _queue()
    assert q.wait(0) is False
    i = q.submit([1, 2, 3, 4], open_text=True)
    assert q.wait(0) is True and q.wait(0) is True    # until it is drained
    q.drain()
    assert q.wait(0) is False and q.wait(0.01) is False
    t = threading.Timer(0.05, lambda: q.push([5], i))
    t.start()
    assert q.wait(5.0) is True
    t.join(5.0)
    assert q.drain()[1] == {i: [5]}


def test_every_push_is_drained_exactly_once_from_two_producer_threads():
    q = _queue()
    reqs = [q.submit([1, 2, 3, 4], open_text=True) for _ in range(2)]
    q.drain()
    N = 2000

    def producer(i):
        for j in range(N):
            q.push([i * N + j], reqs[i])
        q.close_text(reqs[i])
    threads = [threading.Thread(target=producer, args=(i,)) for i in range(2)]
    got, closed_at = {r: [] for r in reqs}, {}
    for t in threads:
        t.start()
    drains = 0
    while len(closed_at) < 2:
        assert q.wait(5.0)
        _, text, closed_text, _, _ = q.drain()
        drains += 1
        for r, ids in text.items():
            assert r not in closed_at, "ids after the request's close_text was reported"
            got[r].extend(ids)
        for r in closed_text:
            closed_at[r] = drains
    for t in threads:
        t.join(5.0)
        assert not t.is_alive()
    assert q.drain()[1] == {}
    for i, r in enumerate(reqs):
        assert got[r] == list(range(i * N, (i + 1) * N))   # all of them, once, in push order


def test_live_slots_against_a_brute_force_count():
    """random arrivals, holds and ends: frames(), capped() and keys() equal a per-row count kept replay by replay"""
    from qwen_tts.talker import LiveSlots, SlotTable
    rng = random.Random(3)
    B, MAXF = 4, 9
    tab = LiveSlots(B, MAXF)
    assert isinstance(tab, SlotTable) and tab.busy() == [] and tab.keys() == 1
    took = [0] * B         # replays the row's request took part in
    plen = [0] * B
    cap = [0] * B
    nxt, total_held = 0, 0
    for step in range(400):
        for b in range(B):
            if tab.req[b] < 0 and rng.random() < 0.3:
                plen[b], c = rng.randrange(1, 40), rng.choice([None, 3, 20])
                cap[b] = MAXF if c is None else min(c, MAXF)
                tab.admit(b, nxt, plen[b], c)
                took[b], nxt = 0, nxt + 1
        busy = tab.busy()
        assert busy == [b for b in range(B) if tab.req[b] >= 0]
        if busy:
            assert tab.keys() == max(plen[b] + took[b] + 1 for b in busy)
        held = [b for b in busy if rng.random() < 0.4]
        for b in held:
            s0 = tab.start[b]
            tab.hold(b)
            assert tab.start[b] == s0 + 1
        tab.frame += 1
        total_held += len(held)
        for b in busy:
            if b not in held:
                took[b] += 1
            assert tab.frames(b) == min(took[b], cap[b])
            assert tab.capped(b) == (took[b] >= cap[b])
        for b in busy:
            if tab.capped(b) or rng.random() < 0.1:
                assert tab.retire(b) == -1 and tab.req[b] == -1
    assert nxt > 20 and total_held > 50 and tab.n == nxt
    with pytest.raises(ValueError):
        b = tab.busy()[0] if tab.busy() else None
        if b is None:
            tab.admit(0, nxt, 5)
            b = 0
        tab.admit(b, nxt + 1, 5)


VOCAB, EOT = 50, 49  # text ids are 0 .. 49; 49 closes a text


@pytest.mark.parametrize("cap", [9, 40])
def test_text_account_against_a_brute_force_model(cap):
    """random pushes, closes, resets, frame advances and writes: n, closed and every list due() returns equal a model
    that keeps, per row, all (pos, id) below the cap and how many of them are written"""
    from qwen_tts.talker import TextAccount
    LOW, AHEAD = TextAccount.LOW, TextAccount.AHEAD
    assert 0 < LOW < AHEAD
    rng = random.Random(cap)
    B = 3
    acct = TextAccount(B, cap)
    assert acct.n == [0] * B and acct.closed == [True] * B and acct.due(lambda b: 0, range(B)) == []
    n, closed, frame = [0] * B, [True] * B, [0] * B
    kept = [[] for _ in range(B)]      # every (pos, id) with pos < cap since the row's last reset
    written = [0] * B                  # how many of them due() has returned
    got = [[] for _ in range(B)]       # what due() returned for the row since its last reset
    seen = dict.fromkeys(("bad", "dropped", "eot", "eot_capped", "reclose", "quiet", "cut", "unlisted"), 0)
    for step in range(800):
        b, what = rng.randrange(B), rng.random()
        if what < 0.04:
            n[b], closed[b], frame[b] = rng.randrange(0, 4), rng.random() < 0.1, 0
            kept[b], written[b], got[b] = [], 0, []
            acct.reset(b, n[b], closed[b])
        elif what < 0.45 and not closed[b]:
            ids = [rng.randrange(VOCAB) for _ in range(rng.randrange(0, 10))]
            bad = rng.choice([-1, VOCAB, VOCAB + 7]) if ids and rng.random() < 0.15 else None
            if bad is not None:
                j = rng.randrange(len(ids))
                ids[j] = bad
            for t in ids[:j] if bad is not None else ids:
                if n[b] < cap:
                    kept[b].append((n[b], t))
                else:
                    seen["dropped"] += 1
                n[b] += 1
            if bad is None:
                acct.push(b, ids, VOCAB)
            else:  # the ids before the bad one count, it and the ones after it do not
                with pytest.raises(ValueError) as e:
                    acct.push(b, ids, VOCAB)
                assert str(e.value) == f"text id {bad} pushed for row {b} is outside the text vocabulary ({VOCAB})"
                seen["bad"] += 1
        elif what < 0.49:
            if closed[b]:
                seen["reclose"] += 1
            elif n[b] < cap:
                kept[b].append((n[b], EOT))  # exactly one end-of-text item, at position n
                seen["eot"] += 1
            else:
                seen["eot_capped"] += 1
            closed[b] = True
            acct.close(b, EOT)
        elif what < 0.7:
            frame[b] = min(frame[b] + rng.randrange(1, 4), cap)
        else:
            rows = sorted(rng.sample(range(B), rng.randrange(1, B + 1)))
            nxt = {r: kept[r][written[r]][0] for r in rows if written[r] < len(kept[r])}
            want = []
            if any(p < frame[r] + LOW for r, p in nxt.items()):
                for r in rows:
                    while written[r] < len(kept[r]) and kept[r][written[r]][0] < frame[r] + AHEAD:
                        want.append((r,) + kept[r][written[r]])
                        written[r] += 1
                seen["cut"] += any(written[r] < len(kept[r]) for r in rows)
            elif nxt:
                seen["quiet"] += 1
            seen["unlisted"] += any(written[r] < len(kept[r]) and kept[r][written[r]][0] < frame[r] + LOW
                                    for r in range(B) if r not in rows)
            items = acct.due(lambda r: frame[r], rows)
            assert items == want, step
            for r, p, t in items:
                assert r in rows and p < min(cap, frame[r] + AHEAD)
                got[r].append((p, t))
        assert acct.n == n and acct.closed == closed, step
        for r in range(B):
            assert got[r] == kept[r][:written[r]] and list(acct.todo[r]) == kept[r][written[r]:], (step, r)
    # (with a cap below AHEAD positions the far limit never binds, and a next position is rarely LOW ahead)
    assert all(v > 0 for k, v in seen.items() if cap > AHEAD or k not in ("cut", "quiet")), seen


def test_text_account_writes_ahead_of_the_frames_and_no_further():
    from qwen_tts.talker import TextAccount
    LOW, AHEAD = TextAccount.LOW, TextAccount.AHEAD
    acct = TextAccount(3, 100)
    for b in range(3):
        acct.reset(b, LOW, False)
        acct.push(b, [b + 1] * 60, VOCAB)            # positions LOW .. LOW + 59
    at = [0, 0, 0]
    rows = [0, 1]
    assert acct.due(at.__getitem__, rows) == []       # every next position is >= frame + LOW
    at[1] = 1                                         # row 1 crosses LOW: both listed rows are written, row 2 is not
    items = acct.due(at.__getitem__, rows)
    assert items == [(0, p, 1) for p in range(LOW, AHEAD)] + [(1, p, 2) for p in range(LOW, AHEAD + 1)]
    assert acct.todo[0][0][0] == AHEAD and acct.todo[1][0][0] == AHEAD + 1 and len(acct.todo[2]) == 60
    assert acct.due(at.__getitem__, rows) == []
    assert acct.due(at.__getitem__, [2]) == []        # row 2 on its own: still LOW ahead
    at[2] = 5
    assert acct.due(at.__getitem__, [2]) == [(2, p, 3) for p in range(LOW, AHEAD + 5)]
    # close: one end-of-text item at position n below the cap, none at or past it, none the second time
    acct = TextAccount(2, 9)
    acct.reset(0, 3, False)
    acct.reset(1, 8, False)
    acct.push(1, [4, 5, 6], VOCAB)                    # position 8 is kept, 9 and 10 are counted and dropped
    assert acct.n == [3, 11] and list(acct.todo[1]) == [(8, 4)]
    acct.close(0, EOT)
    acct.close(1, EOT)
    assert acct.closed == [True, True] and acct.n == [3, 11]
    assert list(acct.todo[0]) == [(3, EOT)] and list(acct.todo[1]) == [(8, 4)]
    acct.close(0, EOT)
    assert acct.due(lambda b: 0, [0, 1]) == [(0, 3, EOT), (1, 8, 4)]
    acct.reset(0, 0, True)                            # a whole-text request: nothing to write, nothing awaited
    assert acct.n[0] == 0 and acct.closed[0] and not acct.todo[0]
    with pytest.raises(ValueError, match=r"text id 50 pushed for request 7 is outside the text vocabulary \(50\)"):
        acct.push(0, [1, 50, 2], VOCAB, "request 7")
    assert acct.n[0] == 1 and list(acct.todo[0]) == [(0, 1)]


class _ScriptedFeed:
    """TextFeed's drain(): what was scripted for this call as (ids per row, rows closed), then nothing"""

    def __init__(self, rows, script):
        self.rows, self.script = rows, list(script)

    def drain(self):
        return self.script.pop(0) if self.script else ([[] for _ in range(self.rows)], [])


class _RecordingEngine:
    class text_emb:
        shape = (VOCAB, 8)

    def __init__(self):
        self.items, self.calls = [], 0

    def append_text(self, s, items, use_graph):
        assert items and s == "session" and use_graph is True  # (an empty list is never passed on)
        self.items += items
        self.calls += 1


def _gate(script, n0=(1, 1), cap=64):
    from qwen_tts.talker import TextGate
    gate, eng = TextGate(_ScriptedFeed(len(n0), script), list(n0), EOT), _RecordingEngine()
    gate.bind(eng, "session", cap, True)
    return gate, eng


def test_text_gate_writes_the_same_items_however_the_text_is_cut():
    from qwen_tts.talker import TextAccount
    text = [[3, 1, 4, 1, 5, 9, 2, 6], [5, 3, 5, 8, 9]]
    want = ([(0, 1 + j, t) for j, t in enumerate(text[0])] + [(0, 9, EOT)]
            + [(1, 1 + j, t) for j, t in enumerate(text[1])] + [(1, 6, EOT)])
    whole, eng_w = _gate([(text, [0, 1])])
    assert whole.ready(0) and not whole.ready(1) and not whole.row_ready(1, 1)   # the heads hold one token each
    whole.poll(0)
    assert eng_w.items == want and eng_w.calls == 1
    cut = ([([[t], []], []) for t in text[0]] + [([[], []], [0])]
           + [([[], [t]], []) for t in text[1]] + [([[], []], [1])])
    pieces, eng_p = _gate(cut)
    for k in range(len(cut)):
        assert pieces.closed == [k > len(text[0]), False]
        assert pieces.row_ready(0, 7) == (k > 6) and pieces.ready(7) is False
        pieces.poll(0)
    assert eng_p.items == want and eng_p.calls == len(cut) - 2   # (positions 8 and 9 waited for row 1's first token)
    for gate in (whole, pieces):
        assert gate.n == [9, 6] and gate.closed == [True, True] and gate.ready(10 ** 6)
        gate.poll(3)                                                          # nothing left: no append
    assert (eng_w.calls, eng_p.calls) == (1, len(cut) - 2)
    # a long text is written as the frames advance, row by row the same tokens whatever the cut
    long = [[(7 * j + b) % EOT for j in range(90)] for b in range(2)]
    runs = []
    for script in ([(long, [])], [([[long[0][j]], [long[1][j]]], []) for j in range(90)]):
        gate, eng = _gate(script + [([[], []], [0, 1])], cap=64)
        for f in range(64):
            gate.poll(f)
            assert all(p < f + TextAccount.AHEAD for _, p, _ in eng.items)
        while gate.feed.script:
            gate.poll(63)
        assert gate.n == [91, 91] and not any(gate.acct.todo)
        runs.append([[it for it in eng.items if it[0] == b] for b in range(2)])
    assert runs[0] == runs[1] == [[(b, 1 + j, t) for j, t in enumerate(long[b][:63])] for b in range(2)]
    # a finished row stops gating; an id outside the vocabulary is refused by poll
    gate, eng = _gate([([[1, VOCAB, 2], []], [])])
    assert not gate.ready(1)
    gate.finished = [True, True]
    assert gate.ready(1) and gate.row_ready(0, 5)
    with pytest.raises(ValueError, match=r"text id 50 pushed for row 0 is outside the text vocabulary \(50\)"):
        gate.poll(0)
    assert gate.n == [2, 1] and eng.items == []


def test_live_row_reset_leaves_a_new_record_but_for_primed():
    import dataclasses
    from qwen_tts.talker import LiveRow
    names = [f.name for f in dataclasses.fields(LiveRow)]
    assert sorted(names) == ["cp_ran", "fresh", "kill", "opened", "primed", "seen", "starved"]
    row = LiveRow(seen=5, fresh=False, cp_ran=True, starved=1.5, kill="timeout", opened=True, primed=True)
    assert all(getattr(row, k) != getattr(LiveRow(), k) for k in names)
    row.reset()
    assert row == LiveRow(primed=True) and row.primed is True
    assert {k: getattr(row, k) for k in names if k != "primed"} == {k: getattr(LiveRow(), k) for k in names
                                                                    if k != "primed"}
    fresh = LiveRow()
    fresh.reset()
    assert fresh == LiveRow() and fresh.primed is False
