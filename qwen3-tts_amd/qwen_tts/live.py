"""Requests that arrive while the engine decodes: the host side of `TTSModel.serve_live(queue)`.

A `RequestQueue` is the only object of a live serving loop that other threads may touch.  `submit`, `push`,
`close_text`, `cancel` and `close` take a lock and append to host lists; the thread that runs the `serve_live()`
generator drains them, assembles the prompts and is the only one that issues GPU work.
"""
from __future__ import annotations

import threading
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

SAMPLING_DEFAULTS = dict(do_sample=True, top_k=50, top_p=1.0, temperature=0.9, subtalker_dosample=True,
                         subtalker_top_k=50, subtalker_top_p=1.0, subtalker_temperature=0.9, repetition_penalty=1.05,
                         seed=None)


def _id_list(ids) -> List[int]:
    if ids is None:
        return []
    if hasattr(ids, "reshape") and hasattr(ids, "tolist"):
        ids = ids.reshape(-1).tolist()
    elif isinstance(ids, int):
        ids = [ids]
    return [int(x) for x in ids]


@dataclass
class LiveRequest:
    """One submitted request, as the serving loop receives it.  `id` is also its Philox stream id."""
    id: int
    input_ids: List[int]
    instruct_ids: Optional[List[int]] = None
    language: Optional[str] = None
    speaker: Optional[str] = None
    voice_clone_prompt: Optional[dict] = None
    non_streaming_mode: bool = False
    open_text: bool = False
    frame_cap: Optional[int] = None
    sampling: dict = field(default_factory=dict)
    ref_ids: Optional[List[int]] = None  # a voice-clone (ICL) request's reference text (serve_live(voice_cache=...))
    step: tuple = (100, 100, 0.0)  # (S, T, db): its speaking rate, tempo step and gain (prosody.steps)


class RequestQueue:
    """The open request stream of `TTSModel.serve_live(queue)`.

        q = RequestQueue(timeout=30.0)
        i = q.submit(ids)                           # a whole text: role ids + text + template suffix; any thread
        j = q.submit(head, open_text=True)          # the three role ids and at least one text id, text to follow
        q.push(more_ids, j); q.close_text(j)        # also before request j has reached a batch row
        q.cancel(i)                                 # the request ends with what has been generated
        q.close()                                   # no more submissions: the loop ends once everything is served

    Ids are consecutive from 0.  timeout: how long an open-text request may go without the text its next frame needs
    before the loop retires it (its id is then in `timed_out`; 0: at once).  `rejected` maps the ids of requests the
    loop could not serve to the exception that says why."""

    def __init__(self, timeout: float = 30.0):
        if timeout is None or not float(timeout) >= 0:
            raise ValueError(f"RequestQueue timeout must be >= 0 seconds, got {timeout}")
        self.timeout = float(timeout)
        self.processor = None  # set by Qwen3TTSModel.request_queue(): what the text wrapper tokenizes with
        self._cv = threading.Condition()
        self._next = 0
        self._closed = False
        self._new: List[LiveRequest] = []            # submitted, not drained yet
        self._text: Dict[int, List[int]] = {}        # request -> ids pushed, not drained yet
        self._open: Dict[int, bool] = {}             # open-text request -> its text is still open (live requests only)
        self._text_closed: List[int] = []            # close_text() calls not drained yet
        self._cancelled: List[int] = []              # cancel() calls not drained yet
        self._live = set()                           # submitted and not over
        self._timed_out: List[int] = []
        self._rejected: Dict[int, BaseException] = {}
        self._events = 0      # submits + pushes + closes + cancels so far
        self._drained = 0     # ... as of the last drain()

    # ------------------------------------------------------------------ producers (any thread)
    def submit(self, input_ids, *, instruct_ids=None, language=None, speaker=None, voice_clone_prompt=None,
               non_streaming_mode=False, open_text=False, frame_cap=None, ref_ids=None, speed=None,
               pitch=None, volume_gain_db=None, **sampling) -> int:
        """Queue a request; returns its id.  **sampling: the per-request sampling parameters of generate() (do_sample,
        top_k, top_p, temperature, the four subtalker_* values, repetition_penalty, seed).  What the loop finds
        unservable when it assembles the prompt (prompt too long, unknown speaker, ...) ends up in `rejected`.
        ref_ids: the reference text's ids of a voice-clone request in ICL mode (its voice_clone_prompt carries
        reference codes), as generate() takes them; the loop serves such a request when it was given a voice_cache.
        speed: the request's speaking rate, 0.5 to 2.0.  pitch / volume_gain_db: its pitch in semitones,
        -12 to 12, and its gain in dB, -96 to 16."""
        from .prosody import steps
        step = (steps(speed, pitch, volume_gain_db, 1) or [LiveRequest.step])[0]
        unknown = set(sampling) - set(SAMPLING_DEFAULTS)
        if unknown:
            raise TypeError(f"submit() got unexpected keyword arguments {sorted(unknown)}")
        if frame_cap is not None and int(frame_cap) < 1:
            raise ValueError(f"frame_cap must be >= 1, got {frame_cap}")
        ids = _id_list(input_ids)
        ins = None if instruct_ids is None else _id_list(instruct_ids)
        ref = None if ref_ids is None else _id_list(ref_ids)
        with self._cv:
            if self._closed:
                raise ValueError("RequestQueue is closed: no submit after close")
            i = self._next
            self._next += 1
            self._new.append(LiveRequest(i, ids, ins, language, speaker, voice_clone_prompt, bool(non_streaming_mode),
                                         bool(open_text), None if frame_cap is None else int(frame_cap),
                                         {**SAMPLING_DEFAULTS, **sampling}, ref, step))
            self._live.add(i)
            if open_text:
                self._open[i] = True
            self._event()
            return i

    def _known(self, request) -> int:
        i = int(request)
        if not 0 <= i < self._next:
            raise ValueError(f"no request {request} (ids 0..{self._next - 1} were issued)")
        return i

    def push(self, ids, request: int) -> None:
        """Append text ids to an open-text request, admitted to a batch row or not; an empty piece is accepted.  A
        push for a request that is over (finished, cancelled, timed out, rejected) is dropped."""
        ids = _id_list(ids)
        with self._cv:
            i = self._known(request)
            if i not in self._live:
                return
            if i not in self._open:
                raise ValueError(f"request {i} was submitted with its whole text (open_text=False)")
            if not self._open[i]:
                raise ValueError(f"request {i}'s text is closed: no push after close_text")
            self._text.setdefault(i, []).extend(ids)
            self._event()

    def push_text(self, text: str, request: int) -> None:
        """Tokenize one piece on its own (the model's processor, no special tokens) and push its ids; cut at word
        boundaries (TextFeed.push_text)."""
        if self.processor is None:
            raise ValueError("RequestQueue.push_text needs the model's processor: take the queue from "
                             "Qwen3TTSModel.request_queue(), or push ids")
        self.push([] if not text else self.processor(text=text, return_tensors="pt", padding=True)["input_ids"],
                  request)

    def close_text(self, request: int) -> None:
        """This request's text is complete (closing twice is harmless)."""
        with self._cv:
            i = self._known(request)
            if i not in self._live:
                return
            if i not in self._open:
                raise ValueError(f"request {i} was submitted with its whole text (open_text=False)")
            if self._open[i]:
                self._open[i] = False
                self._text_closed.append(i)
                self._event()

    def cancel(self, request: int) -> None:
        """End a request: queued, it is never started; decoding, it is retired with the audio generated so far.  Either
        way the loop yields its last chunk with last=True.  Cancelling a request that is over is harmless."""
        with self._cv:
            i = self._known(request)
            if i in self._live and i not in self._cancelled:
                self._cancelled.append(i)
                self._event()

    def close(self) -> None:
        """No more submissions.  The serving loop ends when every request submitted so far is over."""
        with self._cv:
            if not self._closed:
                self._closed = True
                self._event()

    @property
    def closed(self) -> bool:
        with self._cv:
            return self._closed

    @property
    def timed_out(self) -> Tuple[int, ...]:
        """Ids of the requests retired because their text did not arrive within `timeout`, in that order."""
        with self._cv:
            return tuple(self._timed_out)

    @property
    def rejected(self) -> Dict[int, BaseException]:
        """Request id -> the exception that kept the loop from serving it (a copy)."""
        with self._cv:
            return dict(self._rejected)

    def _event(self):
        self._events += 1
        self._cv.notify_all()

    # ------------------------------------------------------------------ the consumer (the serving loop's thread)
    def drain(self):
        """Everything that happened since the last drain, exactly once, without blocking: (new requests in id order,
        {request: ids pushed, in push order}, requests whose text was closed, requests cancelled, closed).  A
        request's close_text is reported with or after its last ids.  `closed` is True only together with, or after,
        the last request: nothing can be submitted behind it."""
        with self._cv:
            out = (self._new, self._text, self._text_closed, self._cancelled, self._closed)
            self._new, self._text, self._text_closed, self._cancelled = [], {}, [], []
            self._drained = self._events
            return out

    def wait(self, timeout: Optional[float] = None) -> bool:
        """Block until something has happened since the last drain() (True), at most `timeout` seconds (default the
        queue's; 0 never blocks) -- False when nothing did."""
        t = self.timeout if timeout is None else float(timeout)
        with self._cv:
            if self._events != self._drained:
                return True
            if t <= 0:
                return False
            return self._cv.wait_for(lambda: self._events != self._drained, t)

    def over(self, request: int, timed_out: bool = False, rejected: Optional[BaseException] = None) -> None:
        """The loop's record that a request has ended: later pushes are dropped, and the reason is kept."""
        with self._cv:
            i = int(request)
            self._live.discard(i)
            self._open.pop(i, None)
            self._text.pop(i, None)
            if timed_out:
                self._timed_out.append(i)
            if rejected is not None:
                self._rejected[i] = rejected
