"""CPU-only: the host side of live serving -- qwen_tts.RequestQueue, and the slot table of a run whose
requests arrive while it decodes and whose rows can be held out of a replay (talker.LiveSlots)."""
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
