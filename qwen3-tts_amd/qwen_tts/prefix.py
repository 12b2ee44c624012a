"""Prefix cache: the talker K/V of a voice instruction, kept across requests.

The instruction is always the head of the talker prompt (TTSModel.build_prompts puts its embeddings first, at RoPE
positions 0..N-1) and attention is causal, so the K/V of those N positions depends on the instruction's ids alone.
`PrefixCache` keeps them per instruction; a prefill that finds its instruction adopts the block into its session rows
(qt_kv_prefix) and computes only the positions behind it (TalkerEngine._prefill_cached over `prefix_rows`).

Host bookkeeping only: this module touches no device API, so it imports (and is tested) without a GPU.
"""
from __future__ import annotations

import threading
import weakref
from collections import OrderedDict
from dataclasses import dataclass
from typing import List, Optional

import numpy as np


@dataclass
class PrefixEntry:
    n: int                 # the instruction's length N
    block: object          # device tensor [2 (K, V)][n_layers][Hkv][N][D] in the engine's K/V dtype
    nbytes: int
    event: object = None   # recorded behind the export that filled the block
    stream: object = None  # the stream it was recorded on (and the block was allocated on)


class PrefixCache:
    """Instruction K/V entries keyed by tuple(instruct ids), LRU by bytes.

    A cache binds to the first TalkerEngine that uses it (its weights, K/V dtype and layer geometry): the entries are
    that engine's bytes.  Passing it to another engine raises ValueError.  The bookkeeping takes a lock, so two host
    threads serving on different streams may share one cache; adopted data is a copy, so evicting an entry never
    touches a running request."""

    def __init__(self, max_bytes: int = 256 << 20):
        self.max_bytes = int(max_bytes)
        self._lock = threading.Lock()
        self._entries: "OrderedDict[tuple, PrefixEntry]" = OrderedDict()
        self._bytes = 0
        self._owner = None  # weakref to the engine
        self._sig = None
        self._n = dict(hits=0, misses=0, stores=0, evictions=0)

    @staticmethod
    def key(ids) -> tuple:
        """The entry key of an instruction: its ids as a tuple of ints (list / tuple / tensor / array, any shape)."""
        if hasattr(ids, "reshape") and hasattr(ids, "tolist"):
            ids = ids.reshape(-1).tolist()
        return tuple(int(x) for x in ids)

    def bind(self, engine):
        """Bind to `engine` (first use), or check that it is the engine this cache is bound to."""
        sig = engine.prefix_signature()
        with self._lock:
            if self._owner is None:
                self._owner, self._sig = weakref.ref(engine), sig
                return
            if self._owner() is not engine or self._sig != sig:
                raise ValueError("this PrefixCache is bound to another engine (its entries are that engine's K/V: "
                                 f"weights, dtype and layer geometry {self._sig}); use one cache per model")

    def fits(self, nbytes: int) -> bool:
        return int(nbytes) <= self.max_bytes

    def lookup(self, key: tuple) -> Optional[PrefixEntry]:
        """The entry of `key`, now the most recently used (a hit), or None (a miss)."""
        with self._lock:
            e = self._entries.get(key)
            if e is None:
                self._n["misses"] += 1
                return None
            self._entries.move_to_end(key)
            self._n["hits"] += 1
            return e

    def store(self, key: tuple, n: int, block, nbytes: Optional[int] = None, event=None, stream=None) -> bool:
        """Keep `block` as the entry of `key`, evicting least recently used entries until it fits.  An entry larger
        than max_bytes is not stored; a key that is present already keeps its entry.  True when stored."""
        if nbytes is None:
            nbytes = block.numel() * block.element_size()
        nbytes = int(nbytes)
        with self._lock:
            if nbytes > self.max_bytes or key in self._entries:
                return False
            while self._entries and self._bytes + nbytes > self.max_bytes:
                _, old = self._entries.popitem(last=False)
                self._bytes -= old.nbytes
                self._n["evictions"] += 1
            self._entries[key] = PrefixEntry(int(n), block, nbytes, event, stream)
            self._bytes += nbytes
            self._n["stores"] += 1
            return True

    def clear(self):
        """Drop every entry (the counters stay)."""
        with self._lock:
            self._entries.clear()
            self._bytes = 0

    def keys(self) -> List[tuple]:
        """The keys held, least recently used first."""
        with self._lock:
            return list(self._entries)

    @property
    def stats(self) -> dict:
        with self._lock:
            return dict(self._n, entries=len(self._entries), bytes=self._bytes)


class PrefixPlan:
    """What a call hands to the engine: the cache, and per request its key (None: the request does not take part) and
    its prompt length, both known on the host."""

    def __init__(self, cache: PrefixCache, keys, lens):
        self.cache, self.keys, self.lens = cache, list(keys), [int(x) for x in lens]
        if len(self.keys) != len(self.lens):
            raise ValueError(f"{len(self.keys)} keys for {len(self.lens)} prompt lengths")

    def rows(self, lo: int, hi: int) -> "Optional[PrefixPlan]":
        """The plan of requests [lo, hi), or None when none of them takes part (they are then served by the
        ordinary prefill, exactly as without a cache)."""
        if all(k is None for k in self.keys[lo:hi]):
            return None
        return PrefixPlan(self.cache, self.keys[lo:hi], self.lens[lo:hi])


def prefix_rows(P: int, n_real, C) -> dict:
    """Row arrays of a prefill that computes, for batch row b of a batch left-padded to P, only the positions j in
    [C_b, n_real_b), packed over all batch rows in order (int32 numpy arrays, one element per computed position):

        rope_pos = j    kv_pos = n_pads_b + j    row_len = n_pads_b + j + 1    row_start = n_pads_b    row_batch = b

    with n_pads_b = P - n_real_b: today's values of the same positions (C = 0 computes every real position; B = 1 with
    n_real = P is the slot refill).  Also `count` [B] (computed positions per batch row), `last` [B] (packed index of
    each batch row's last real position, int64) and `src` (index of each computed position in the flattened [B * P]
    batch).  Every batch row computes at least its last position: C_b < n_real_b."""
    n_real = np.asarray(n_real, dtype=np.int64).reshape(-1)
    C = np.asarray(C, dtype=np.int64).reshape(-1)
    if n_real.shape != C.shape:
        raise ValueError(f"{n_real.shape[0]} prompt lengths for {C.shape[0]} cached lengths")
    if (n_real > P).any() or (C < 0).any() or (C >= n_real).any():
        raise ValueError(f"need 0 <= C_b < n_real_b <= P, got P = {P}, n_real = {n_real.tolist()}, C = {C.tolist()}")
    count = n_real - C
    b = np.repeat(np.arange(n_real.shape[0], dtype=np.int64), count)
    first = np.cumsum(count) - count                 # packed index of each batch row's first computed position
    j = np.arange(int(count.sum()), dtype=np.int64) - first[b] + C[b]
    pads = (P - n_real)[b]
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)  # noqa: E731
    return {"rope_pos": i32(j), "kv_pos": i32(pads + j), "row_len": i32(pads + j + 1), "row_start": i32(pads),
            "row_batch": i32(b), "src": i32(b * P + pads + j), "count": i32(count),
            "last": np.ascontiguousarray(first + count - 1, dtype=np.int64)}
