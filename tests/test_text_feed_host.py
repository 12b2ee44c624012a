"""CPU-only: qwen_tts.TextFeed, the host side of stream(text_feed=...) -- per-row order, empty pieces,
the rejections at push, drain() handing everything out exactly once, and the wait that ends on a push or close from a
second thread or at its timeout."""
import threading
import time

import pytest
import torch


def _feed(rows=2, timeout=2.0):
    from qwen_tts.feed import TextFeed
    return TextFeed(rows=rows, timeout=timeout)


def test_public_names():
    import qwen_tts
    from qwen_tts.feed import TextFeed, TextFeedTimeout
    assert qwen_tts.TextFeed is TextFeed and qwen_tts.TextFeedTimeout is TextFeedTimeout
    assert issubclass(TextFeedTimeout, TimeoutError)


def test_per_row_order_and_empty_pieces():
    f = _feed(rows=3)
    f.push([5, 6], row=1)
    f.push([], row=0)                              # an empty piece is accepted
    f.push(torch.tensor([[7, 8, 9]]), row=1)       # tensors of any shape
    f.push(3, row=2)                               # one int
    f.push([4], row=0)
    pieces, closed = f.drain()
    assert pieces == [[4], [5, 6, 7, 8, 9], [3]] and closed == []
    assert all(isinstance(x, int) for p in pieces for x in p)


def test_drain_hands_everything_out_exactly_once():
    f = _feed()
    assert f.drain() == ([[], []], [])
    f.push([1, 2], row=0)
    f.close(row=0)
    assert f.drain() == ([[1, 2], []], [0])        # a close comes with (or after) the row's last ids
    assert f.drain() == ([[], []], [])             # nothing twice, the close included
    f.push([3], row=1)
    f.close(row=1)
    f.close(row=1)                                 # closing twice is harmless
    assert f.drain() == ([[], [3]], [1])
    assert f.drain() == ([[], []], [])
    assert f.closed(0) and f.closed(1)


def test_rejections():
    from qwen_tts.feed import TextFeed
    f = _feed()
    f.close(row=1)
    with pytest.raises(ValueError, match="closed"):
        f.push([1], row=1)
    with pytest.raises(ValueError, match="closed"):
        f.push([], row=1)
    for row in (-1, 2):
        with pytest.raises(ValueError, match="out of range"):
            f.push([1], row=row)
        with pytest.raises(ValueError, match="out of range"):
            f.close(row=row)
    f.push([9], row=0)                             # the other row is unaffected
    assert f.drain() == ([[9], []], [1])
    with pytest.raises(ValueError):
        TextFeed(rows=0)
    with pytest.raises(ValueError):
        TextFeed(rows=1, timeout=-1)
    with pytest.raises(ValueError, match="processor"):
        _feed().push_text("hello")


def test_push_text_tokenizes_each_piece_on_its_own():
    from qwen_tts.text import FallbackProcessor
    f = _feed(rows=1)
    f.processor = proc = FallbackProcessor()
    f.push_text("hello world")
    f.push_text("")
    f.push_text(" again")
    want = proc(text="hello world")["input_ids"][0].tolist() + proc(text=" again")["input_ids"][0].tolist()
    assert f.drain() == ([want], [])


def test_wait_returns_at_once_for_what_is_already_there_and_at_timeout_otherwise():
    f = _feed(timeout=0.05)
    f.push([1], row=0)
    t0 = time.perf_counter()
    assert f.wait() is True                        # pushed before the wait: no waiting
    assert time.perf_counter() - t0 < 0.04
    f.drain()
    t0 = time.perf_counter()
    assert f.wait() is False                       # nothing since the drain: the feed's timeout
    assert 0.04 <= time.perf_counter() - t0 < 1.0
    t0 = time.perf_counter()
    assert f.wait(0) is False                      # timeout 0 never waits
    assert time.perf_counter() - t0 < 0.04


@pytest.mark.parametrize("what", ["push", "close", "empty"])
def test_wait_returns_on_an_event_from_a_second_thread(what):
    f = _feed(timeout=5.0)
    f.drain()
    started = threading.Event()

    def producer():
        started.wait(2.0)
        if what == "close":
            f.close(row=1)
        else:
            f.push([7] if what == "push" else [], row=1)

    th = threading.Thread(target=producer)
    th.start()
    try:
        t0 = time.perf_counter()
        started.set()
        assert f.wait() is True
        assert time.perf_counter() - t0 < 4.0      # the event, not the timeout, ended the wait
    finally:
        th.join(5.0)
    assert not th.is_alive()
    pieces, closed = f.drain()
    assert (pieces, closed) == {"push": ([[], [7]], []), "close": ([[], []], [1]), "empty": ([[], []], [])}[what]
