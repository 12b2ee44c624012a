"""CPU-only: the prefix cache's host side (qwen_tts/prefix.py) -- PrefixCache bookkeeping with stub blocks,
and the row table of a prefill over adopted keys as a pure function of (P, n_real, C)."""
import numpy as np
import pytest
import torch

from qwen_tts.prefix import PrefixCache, PrefixPlan, prefix_rows

ROW_ARRAYS = ("rope_pos", "kv_pos", "row_len", "row_start", "row_batch")


class _Engine:
    def __init__(self, sig=("torch.float32", 2, 2, 64)):
        self.sig = sig

    def prefix_signature(self):
        return self.sig


def _stats(c):
    s = c.stats
    return s["hits"], s["misses"], s["stores"], s["evictions"], s["entries"], s["bytes"]


def test_lru_by_bytes_and_counts():
    c = PrefixCache(max_bytes=100)
    assert c.stats == dict(hits=0, misses=0, stores=0, evictions=0, entries=0, bytes=0)
    a, b, d = (1, 2), (3,), (4, 5, 6)
    assert c.lookup(a) is None
    assert c.store(a, 2, "A", nbytes=40) and c.store(b, 1, "B", nbytes=40)
    assert _stats(c) == (0, 1, 2, 0, 2, 80)
    e = c.lookup(a)                      # a is now the most recently used: b goes first
    assert (e.n, e.block, e.nbytes) == (2, "A", 40)
    assert c.store(d, 3, "D", nbytes=50)
    assert c.keys() == [a, d] and c.lookup(b) is None
    assert _stats(c) == (1, 2, 3, 1, 2, 90)
    assert c.store(b, 1, "B2", nbytes=100)   # needs the whole cache: both others go, least recently used first
    assert c.keys() == [b] and _stats(c) == (1, 2, 4, 3, 1, 100)
    assert not c.store(b, 1, "B3", nbytes=10)    # a key that is present keeps its entry
    assert c.lookup(b).block == "B2" and c.stats["stores"] == 4


def test_entry_larger_than_the_cache_is_not_stored():
    c = PrefixCache(max_bytes=64)
    assert c.store((1,), 1, "small", nbytes=64)
    assert not c.fits(65) and not c.store((2,), 1, "big", nbytes=65)
    assert c.keys() == [(1,)] and _stats(c) == (0, 0, 1, 0, 1, 64)   # and it evicted nothing
    t = torch.zeros(2, 2, 2, 3, 4)        # a tensor block is sized from its elements
    assert not c.store((3,), 3, t) and PrefixCache(max_bytes=t.numel() * 4).store((3,), 3, t)


def test_clear():
    c = PrefixCache(max_bytes=100)
    c.store((1,), 1, "x", nbytes=10)
    c.lookup((1,))
    c.clear()
    assert c.keys() == [] and c.lookup((1,)) is None
    assert _stats(c) == (1, 1, 1, 0, 0, 0)
    assert c.store((1,), 1, "y", nbytes=100)


def test_key_equality_on_ids():
    ids = [151644, 872, 198, 7, 151645, 198]
    k = PrefixCache.key(ids)
    assert k == tuple(ids) and all(type(x) is int for x in k)
    assert PrefixCache.key(tuple(ids)) == k
    assert PrefixCache.key(torch.tensor([ids])) == k            # the wrapper's [1, n] tensors
    assert PrefixCache.key(torch.tensor(ids, dtype=torch.int32)) == k
    assert PrefixCache.key(np.asarray(ids)) == k
    assert PrefixCache.key(ids[:-1]) != k
    c = PrefixCache()
    c.store(PrefixCache.key(torch.tensor([ids])), len(ids), "blk", nbytes=1)
    assert c.lookup(PrefixCache.key(ids)).block == "blk"


def test_binding_to_a_second_engine_raises():
    c = PrefixCache()
    e1, e2 = _Engine(), _Engine()
    c.bind(e1)
    c.bind(e1)                            # the same engine again is fine
    with pytest.raises(ValueError, match="bound to another engine"):
        c.bind(e2)                        # same geometry, other weights
    e1.sig = ("torch.bfloat16", 2, 2, 64)
    with pytest.raises(ValueError):
        c.bind(e1)                        # the engine's K/V format is not the entries'
    assert c.stats["entries"] == 0


def test_plan_slices():
    p = PrefixPlan(PrefixCache(), [(1,), None, (2, 3)], [9, 4, 12])
    q = p.rows(1, 3)
    assert q.cache is p.cache and q.keys == [None, (2, 3)] and q.lens == [4, 12]
    assert p.rows(1, 2) is None           # nobody in the slice takes part: the ordinary prefill serves it
    with pytest.raises(ValueError):
        PrefixPlan(PrefixCache(), [None], [1, 2])


def _prefill_tables(mask):
    """The row arrays TalkerEngine._prefill builds for every position of a left-padded batch, restated from `mask`."""
    B, P = mask.shape
    pos = mask.float().cumsum(-1) - 1
    pos = pos.masked_fill(mask == 0, 1)
    n_pads = P - mask.sum(-1)
    return {"rope_pos": pos.reshape(-1).to(torch.int32),
            "kv_pos": torch.arange(P, dtype=torch.int32).repeat(B),
            "row_len": torch.arange(1, P + 1, dtype=torch.int32).repeat(B),
            "row_start": torch.where(mask.bool(), n_pads[:, None], torch.zeros_like(n_pads)[:, None]).reshape(-1)
            .to(torch.int32),
            "row_batch": torch.arange(B, dtype=torch.int32).repeat_interleave(P)}


P, N_REAL = 7, [7, 4, 5]


def test_rows_without_cache_are_todays_rows_at_the_real_positions():
    mask = torch.tensor([[0] * (P - n) + [1] * n for n in N_REAL])
    want = _prefill_tables(mask)
    real = mask.reshape(-1).bool()
    got = prefix_rows(P, N_REAL, [0, 0, 0])
    for k in ROW_ARRAYS:
        assert got[k].dtype == np.int32
        np.testing.assert_array_equal(got[k], want[k][real].numpy(), err_msg=k)
    np.testing.assert_array_equal(got["src"], np.flatnonzero(real.numpy()))
    np.testing.assert_array_equal(got["count"], N_REAL)
    np.testing.assert_array_equal(got["last"], np.cumsum(N_REAL) - 1)


@pytest.mark.parametrize("n", [1, 9])
def test_one_unpadded_row_is_the_slot_refill(n):
    got = prefix_rows(n, [n], [0])
    ar = np.arange(n, dtype=np.int32)     # _prefill_slot's arange tables
    np.testing.assert_array_equal(got["rope_pos"], ar)
    np.testing.assert_array_equal(got["kv_pos"], ar)
    np.testing.assert_array_equal(got["row_len"], ar + 1)
    np.testing.assert_array_equal(got["row_start"], np.zeros(n, np.int32))
    np.testing.assert_array_equal(got["row_batch"], np.zeros(n, np.int32))
    assert got["last"].tolist() == [n - 1] and got["count"].tolist() == [n]


def test_mixed_cached_lengths():
    C = [0, 3, 5 - 1]                     # the last row computes a single position
    got = prefix_rows(P, N_REAL, C)
    assert got["count"].tolist() == [7, 1, 1]
    assert got["row_batch"].tolist() == [0] * 7 + [1, 2]             # packed in batch order
    assert got["rope_pos"].tolist() == [0, 1, 2, 3, 4, 5, 6, 3, 4]   # j
    assert got["kv_pos"].tolist() == [0, 1, 2, 3, 4, 5, 6, 3 + 3, 2 + 4]       # n_pads + j
    assert got["row_len"].tolist() == [1, 2, 3, 4, 5, 6, 7, 7, 7]    # n_pads + j + 1
    assert got["row_start"].tolist() == [0] * 7 + [3, 2]             # n_pads
    assert got["src"].tolist() == [0, 1, 2, 3, 4, 5, 6, 1 * P + 6, 2 * P + 6]
    assert got["last"].tolist() == [6, 7, 8] and got["last"].dtype == np.int64
    # and they are today's values of the same positions
    mask = torch.tensor([[0] * (P - n) + [1] * n for n in N_REAL])
    want = _prefill_tables(mask)
    for k in ROW_ARRAYS:
        np.testing.assert_array_equal(got[k], want[k].numpy()[got["src"]], err_msg=k)


def test_every_row_computes_its_last_position():
    for bad in ([7, 4, 5], [0, 0, 6], [0, -1, 0]):
        with pytest.raises(ValueError):
            prefix_rows(P, N_REAL, bad)
    with pytest.raises(ValueError):
        prefix_rows(6, N_REAL, [0, 0, 0])     # a row longer than the batch
