"""CPU-only: the host side of per-request sampling parameters -- GenParams lists, session keys, the ctypes mirrors of
qt_sample_row / qt_sample_args against the library's own sizeof, and the data-parallel sharding of list values."""
import ctypes
import dataclasses

import pytest
import torch


def test_scalar_genparams_key_is_unchanged():
    """A call with scalar parameters keeps its session key (and with it its kernel arguments and captured graphs)."""
    from qwen_tts.talker import GenParams
    gp = GenParams()
    assert not gp.per_row
    assert gp.key() == (True, 50, 1.0, 0.9, True, 50, 1.0, 0.9, None, 1.05, False)
    gp = GenParams(max_new_tokens=7, do_sample=False, top_k=3, top_p=0.5, temperature=1.5, subtalker_dosample=False,
                   subtalker_top_k=4, subtalker_top_p=0.25, subtalker_temperature=2.0, eos_token_id=11,
                   repetition_penalty=1.5, ignore_eos=True, seed=5)
    assert gp.key() == (False, 3, 0.5, 1.5, False, 4, 0.25, 2.0, 11, 1.5, True)
    assert gp.resolve_seed() == 5
    gp.check_rows(3)  # scalars fit any request count


def test_per_row_genparams_normalise_and_key():
    from qwen_tts.talker import GenParams
    a = GenParams(temperature=[0.3, 1.5, 0.9], top_k=(50, 0, 5), seed=[7, None, 8], eos_token_id=4)
    b = GenParams(do_sample=[True, False, True], repetition_penalty=[1.0, 1.1, 1.2], eos_token_id=4)
    assert a.per_row and b.per_row and a.n_rows == 3
    assert a.key() == b.key() == ("per_row", 4, False)  # the values are not part of the key
    assert a.key() != GenParams(temperature=[0.3], eos_token_id=4, ignore_eos=True).key()
    assert a.key() != GenParams(eos_token_id=4).key()
    hash(a.key())
    a.check_rows(3)
    with pytest.raises(ValueError):
        a.check_rows(2)
    # records: (do_sample, top_k, top_p, temperature, rep_penalty, seed) for the talker, the sub-talker's has penalty 1
    t, c = a.row_records(1, seed=99)
    assert t == (True, 0, 1.0, 1.5, 1.05, 99) and c == (True, 50, 1.0, 0.9, 1.0, 99)  # None -> the call's seed
    assert a.row_records(0, seed=99)[0] == (True, 50, 1.0, 0.3, 1.05, 7)
    assert dataclasses.replace(a, max_new_tokens=3).n_rows == 3
    torch.manual_seed(3)
    x = a.resolve_seed()
    torch.manual_seed(3)
    assert GenParams().resolve_seed() == x  # the call's seed of a list is drawn like a scalar None


@pytest.mark.parametrize("bad", [dict(temperature=[0.9, 0.0]), dict(temperature=[-1.0]), dict(top_p=[1.0, 1.5]),
                                 dict(top_p=[0.0]), dict(top_k=[-1]), dict(repetition_penalty=[0.0]),
                                 dict(subtalker_temperature=[0.0]), dict(subtalker_top_p=[2.0]),
                                 dict(subtalker_top_k=[-3]), dict(temperature=[0.9, 1.0], top_k=[5]),
                                 dict(top_k=[None])])
def test_per_row_genparams_validation(bad):
    from qwen_tts.talker import GenParams
    with pytest.raises(ValueError):
        GenParams(**bad)


def test_ctypes_mirrors_match_the_library():
    from qwen_tts import _hip
    L = _hip.load_library()
    assert ctypes.sizeof(_hip.SampleRow) == L.qt_sample_row_bytes() == 32
    assert ctypes.sizeof(_hip.SampleArgs) == L.qt_sample_args_bytes()
    # `rows` is the last field: a caller built against the struct without it passes NULL by zero-initialising
    name, _ = _hip.SampleArgs._fields_[-1]
    assert name == "rows" and _hip.SampleArgs.rows.offset + 8 == ctypes.sizeof(_hip.SampleArgs)
    assert [f for f, _ in _hip.SampleRow._fields_] == ["temperature", "top_p", "rep_penalty", "top_k", "do_sample",
                                                       "reserved", "seed"]
    assert _hip.SampleRow.seed.offset == 24


class _StubModel:
    speech_tokenizer = None

    def __init__(self):
        self.calls = []

    def generate(self, **kw):
        self.calls.append(kw)
        return [torch.full((1, 16), i) for i in kw["philox_ids"]], None


def test_dp_generate_shards_list_parameters_by_request(monkeypatch):
    from qwen_tts import dp
    ids = [torch.zeros(n, dtype=torch.long) for n in (5, 9, 3, 7, 2)]
    temps = [0.1, 0.2, 0.3, 0.4, 0.5]
    seeds = [10, None, 30, 40, 50]
    shards = dp.shard_longest_first(dp.request_cost(ids, None, None, 16), 2)
    assert sorted(shards[0] + shards[1]) == list(range(5)) and shards[0] and shards[1]
    for rank in (0, 1):
        monkeypatch.setattr(dp.dist, "is_initialized", lambda: True)
        monkeypatch.setattr(dp.dist, "get_world_size", lambda group=None: 2)
        monkeypatch.setattr(dp.dist, "get_rank", lambda group=None, r=rank: r)
        m = _StubModel()
        local = dp.dp_generate(m, ids, ["auto"] * 5, gather=False, max_new_tokens=16, temperature=temps, seed=seeds,
                               top_k=20)
        mine = shards[rank]
        (kw,) = m.calls
        assert kw["philox_ids"] == mine and sorted(local) == mine
        assert kw["temperature"] == [temps[i] for i in mine] and kw["seed"] == [seeds[i] for i in mine]
        assert kw["top_k"] == 20 and len(kw["input_ids"]) == len(mine)
    with pytest.raises(ValueError):
        dp.dp_generate(_StubModel(), ids, ["auto"] * 5, gather=False, temperature=[0.5, 0.6])


def test_wrapper_checks_list_lengths():
    from qwen_tts.inference.qwen3_tts_model import Qwen3TTSModel
    w = Qwen3TTSModel.__new__(Qwen3TTSModel)
    w.generate_defaults = {"temperature": 0.7}
    out = w._merge_generate_kwargs(n_requests=2, temperature=[0.5, 0.6], seed=[1, None], top_k=3)
    assert out["temperature"] == [0.5, 0.6] and out["seed"] == [1, None] and out["top_k"] == 3
    assert w._merge_generate_kwargs(n_requests=2)["temperature"] == 0.7  # file defaults stay scalars
    assert "n_requests" not in out
    with pytest.raises(ValueError):
        w._merge_generate_kwargs(n_requests=2, temperature=[0.5, 0.6, 0.7])
    with pytest.raises(ValueError):
        w._merge_generate_kwargs(n_requests=2, seed=[1])
