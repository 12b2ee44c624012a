"""Text that arrives while its audio is generated: the host side of `stream(text_feed=...)`.

A `TextFeed` carries, per batch row, the text ids that were not known when the request was submitted.  It is the only
object of a streamed request that another thread may touch: `push` / `close` take a lock and append to host lists; the
thread that runs the `stream()` generator drains them and is the only one that issues GPU work.
"""
from __future__ import annotations

import threading
from typing import List, Tuple


class TextFeedTimeout(TimeoutError):
    """stream(text_feed=...) ran out of text: some row that is neither closed nor finished had no token for the next
    frame, and none arrived within the feed's `timeout` seconds.  The generator has released its session and codec
    slots when this propagates."""


class TextFeed:
    """Per-row queues of text ids for `TTSModel.stream(text_feed=feed)`.

        feed = TextFeed(rows=B, timeout=30.0)
        feed.push(ids, row=0)     # any number of ids, none included; any thread
        feed.close(row=0)         # this row's text is complete: the end-of-text position follows its last token

    timeout: how long the consumer waits for text when no frame can be queued (0: it never waits)."""

    def __init__(self, rows: int = 1, timeout: float = 30.0):
        if int(rows) < 1:
            raise ValueError(f"TextFeed needs at least one row, got {rows}")
        if timeout is None or not float(timeout) >= 0:
            raise ValueError(f"TextFeed timeout must be >= 0 seconds, got {timeout}")
        self.rows, self.timeout = int(rows), float(timeout)
        self.processor = None  # set by Qwen3TTSModel.stream(text_feed=...): what push_text tokenizes with
        self._cv = threading.Condition()
        self._new: List[List[int]] = [[] for _ in range(self.rows)]  # pushed, not drained yet
        self._closed = [False] * self.rows
        self._close_seen = [False] * self.rows  # the close has been handed out by drain()
        self._events = 0      # pushes + closes so far
        self._drained = 0     # ... as of the last drain()

    def _row(self, row) -> int:
        r = int(row)
        if not 0 <= r < self.rows:
            raise ValueError(f"TextFeed row {row} out of range (the feed has {self.rows} rows)")
        return r

    def push(self, ids, row: int = 0) -> None:
        """Append text ids (a list, a tensor of any shape, or one int) to a row; an empty piece is accepted."""
        r = self._row(row)
        if hasattr(ids, "reshape") and hasattr(ids, "tolist"):
            ids = ids.reshape(-1).tolist()
        elif isinstance(ids, int):
            ids = [ids]
        ids = [int(x) for x in ids]
        with self._cv:
            if self._closed[r]:
                raise ValueError(f"TextFeed row {r} is closed: no push after close")
            self._new[r].extend(ids)
            self._events += 1
            self._cv.notify_all()

    def push_text(self, text: str, row: int = 0) -> None:
        """Tokenize one piece on its own (the model's processor, no special tokens) and push its ids.  Piece-wise BPE
        is not the BPE of the whole sentence: a word cut between two pieces gets other ids than it would in one
        piece, so cut at word boundaries; what stream(text_feed=...) guarantees is stated on ids, not on strings."""
        if self.processor is None:
            raise ValueError("TextFeed.push_text needs the model's processor: pass the feed to "
                             "Qwen3TTSModel.stream(text_feed=feed) first, or push ids")
        r = self._row(row)
        ids = [] if not text else self.processor(text=text, return_tensors="pt", padding=True)["input_ids"]
        self.push(ids, r)

    def close(self, row: int = 0) -> None:
        """This row's text is complete (closing twice is harmless)."""
        r = self._row(row)
        with self._cv:
            if not self._closed[r]:
                self._closed[r] = True
                self._events += 1
                self._cv.notify_all()

    def closed(self, row: int = 0) -> bool:
        with self._cv:
            return self._closed[self._row(row)]

    def drain(self) -> Tuple[List[List[int]], List[int]]:
        """Everything pushed since the last drain, exactly once, without blocking: (ids per row, in push order; rows
        closed since the last drain).  A row's close is reported with or after its last ids."""
        with self._cv:
            out, self._new = self._new, [[] for _ in range(self.rows)]
            closed = [r for r in range(self.rows) if self._closed[r] and not self._close_seen[r]]
            for r in closed:
                self._close_seen[r] = True
            self._drained = self._events
            return out, closed

    def wait(self, timeout: float = None) -> bool:
        """Block until a push or close has happened since the last drain() (True), at most `timeout` seconds
        (default the feed's; 0 never blocks) -- False when none came."""
        t = self.timeout if timeout is None else float(timeout)
        with self._cv:
            if self._events != self._drained:
                return True
            if t <= 0:
                return False
            return self._cv.wait_for(lambda: self._events != self._drained, t)
