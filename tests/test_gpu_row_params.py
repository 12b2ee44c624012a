"""Per-request sampling parameters (qt_sample_args.rows, GenParams lists): every row of a launch / request of a call
reads its own record from a device table.  The contract pinned here: row i under record i gets exactly what it gets
from the same launch / call made with record i's values as scalars -- the kernels and the batch shape are the same,
so this is equality of tokens, not a tolerance."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


# (do_sample, top_k, top_p, temperature, rep_penalty, seed): one sampler path each
RECORDS = [(False, 50, 1.0, 0.9, 1.05, 11),   # greedy: argmax
           (True, 50, 1.0, 0.9, 1.05, 12),    # histogram / per-wave fast path
           (True, 50, 0.8, 0.9, 1.05, 13),    # nucleus sort
           (True, 0, 1.0, 1.3, 1.05, 14),     # inverse CDF over the whole vocabulary
           (True, 200, 1.0, 0.7, 1.05, 15),   # block search
           (True, 1, 1.0, 0.9, 1.3, 16)]      # k = 1 with a stronger repetition penalty
G = 16


def _table(records, dev):
    from qwen_tts import kernels as Kn
    t = Kn.sample_rows_table(len(records), dev)
    Kn.upload_sample_rows(t, 0, records)
    return t


class _SampleState:
    """Inputs of one qt_sample launch over R rows, and a launcher that leaves them unchanged."""

    def __init__(self, V, R, dev, seed=0):
        g = torch.Generator().manual_seed(1000 * V + R + seed)
        self.V, self.R, self.dev = V, R, dev
        self.logits = (torch.randn(R, V, generator=g) * 3).to(dev)
        self.seen = (torch.rand(R, V, generator=g) < 0.1).to(torch.uint8).to(dev)
        self.step = torch.tensor([3, 1, 4, 1, 5, 9][:R], dtype=torch.int32, device=dev)
        self.ngen = torch.full((R,), 5, dtype=torch.int32, device=dev)
        self.prow = torch.arange(10, 10 + R, dtype=torch.int32, device=dev)
        self.eos = -1

    def run(self, r0=0, r1=None, rec=None, rows=None, philox=True):
        """Rows [r0, r1) in one launch, with the scalars of `rec` or the table `rows`: (tok, codes, seen, finished)."""
        from qwen_tts import kernels as Kn
        r1 = self.R if r1 is None else r1
        n = r1 - r0
        tok = torch.full((n,), -1, dtype=torch.int32, device=self.dev)
        codes = torch.full((n, 12 * G), -1, dtype=torch.int32, device=self.dev)
        seen = self.seen[r0:r1].clone()
        fin = torch.zeros(n, dtype=torch.uint8, device=self.dev)
        how = {"rows": rows} if rows is not None else dict(
            do_sample=rec[0], top_k=rec[1], top_p=rec[2], temperature=rec[3], rep_penalty=rec[4], seed=rec[5])
        Kn.sample(self.logits[r0:r1], n, self.V, self.V, tok, seen=seen, n_generated=self.ngen[r0:r1], min_new_tokens=2,
                  eos_id=self.eos, finished=fin, step=self.step[r0:r1], substep=3, codes=codes, codes_ld=12 * G,
                  codes_w=G, codes_col=2, ctr_stride=1, philox_row=self.prow[r0:r1] if philox else None,
                  row_base=10 + r0, **how)
        torch.cuda.synchronize()
        return tok, codes, seen, fin


def _same_row(got, j, ref, i, what):
    for a, b, name in zip(got, ref, ("tok_out", "codes", "seen", "finished")):
        assert torch.equal(a[j], b[i]), f"{what}: {name} differs"


@pytest.mark.parametrize("V", [2048, 3072])
def test_sample_mixed_rows_equal_scalar_launches(V):
    """Six rows, six records (one per sampler path) in one launch against six scalar launches of the same kernel, each
    with one record's values on every row: row j of the mixed launch equals row j of scalar launch j in tok_out, codes,
    seen and finished.  Also a table slice rows[2:5] with the Philox ids offset to match (by philox_row and by
    row_base), which is the addressing a lane of a larger session uses."""
    dev = _dev()
    st = _SampleState(V, 6, dev)
    st.eos = int(st.run(rec=RECORDS[0])[0][0])  # row 0's greedy token: its row sets `finished`
    ref = [st.run(rec=rec) for rec in RECORDS]
    table = _table(RECORDS, dev)
    got = st.run(rows=table)
    print(f"\n  V={V}: mixed {got[0].tolist()}; scalar launches {[r[0].tolist() for r in ref]}")
    for j in range(6):
        _same_row(got, j, ref[j], j, f"row {j}")
    assert int(got[3][0]) == 1  # the greedy row chose eos
    # non-vacuity: on no row do the six parameter sets all lead to the same token, and the records matter -- rows 1-5
    # under their own record differ from the same rows under row 0's (greedy) record somewhere
    for r in range(6):
        assert len({int(ref[j][0][r]) for j in range(6)}) > 1, f"row {r}: every record chose the same token"
    assert any(int(ref[j][0][j]) != int(ref[0][0][j]) for j in range(1, 6))
    for philox in (True, False):
        part = st.run(2, 5, rows=table[2:5], philox=philox)
        for j in range(3):
            _same_row(part, j, ref[2 + j], 2 + j, f"slice row {2 + j} (philox_row {philox})")


@pytest.mark.parametrize("j", [1, 2])
def test_sample_single_row_table(j):
    dev = _dev()
    st = _SampleState(2048, 1, dev, seed=j)
    ref = st.run(rec=RECORDS[j])
    got = st.run(rows=_table([RECORDS[j]], dev))
    _same_row(got, 0, ref, 0, f"R = 1, record {j}")
    # the seed matters on this row (so the equality above shows the record's seed was the key of the draw)
    draws = {int(st.run(rec=RECORDS[j][:5] + (sd,))[0][0]) for sd in (RECORDS[j][5], 91, 92, 93, 94)}
    assert len(draws) > 1, "five seeds drew the same token"


@pytest.mark.parametrize("R", [8, 3])
def test_cp_step_sampled_with_row_table(R):
    """The fused sampler of the code-predictor step engine with a mixed table (greedy, k = 50, k = 200 with p = 0.8,
    k = 0, cycled): qt_sample(rows) followed by qt_cp_step against qt_cp_step_sampled(rows) -- the same tokens and
    codes, bit-identical logits and appended K/V, hand-off flag word 0 (the sampler's barrier count differs per row's
    path and the other waves of its workgroup follow it)."""
    from qwen_tts import kernels as Kn
    from test_gpu_cp_engine import _cp_stack
    dev = _dev()
    st, lm, g = _cp_stack(dev, seed=7)
    if not Kn.cp_step_supported(st.H, st.I, st.Hq, st.Hkv, st.D, st.n_layers, lm.N):
        pytest.skip("qt_cp_step not supported on this device")
    Lmax, V, pos = 18, lm.N, 6
    prev_logits = (torch.randn(R, V, generator=g) * 3).to(dev)
    tab_x = torch.randn(V, st.H, generator=g).to(dev)
    tab_q = torch.randn(V, st.qkv_w, generator=g).to(dev)
    kc = [torch.randn(R, st.Hkv, Lmax, st.D, generator=g).to(dev, torch.bfloat16) for _ in st.layers]
    vc = [torch.randn(R, st.Hkv, Lmax, st.D, generator=g).to(dev, torch.bfloat16) for _ in st.layers]
    step = torch.tensor([3, 1, 4, 1, 5, 9, 2, 6][:R], dtype=torch.int32, device=dev)
    prow = torch.arange(10, 10 + R, dtype=torch.int32, device=dev)
    mix = [(False, 50, 1.0, 0.9, 1.0), (True, 50, 1.0, 0.9, 1.0), (True, 200, 0.8, 0.9, 1.0), (True, 0, 1.0, 1.1, 1.0)]
    records = [mix[r % 4] + (100 + r,) for r in range(R)]
    table = _table(records, dev)

    def run(fused, rows=table, rec=None):
        codes = torch.full((R, 12 * G), -1, dtype=torch.int32, device=dev)
        tok = torch.full((R,), -1, dtype=torch.int32, device=dev)
        x = torch.zeros(R, st.H, device=dev)
        q0 = torch.zeros(R, st.qkv_w, device=dev)
        k2, v2 = [k.clone() for k in kc], [v.clone() for v in vc]
        logits = torch.full((R, V), float("nan"), device=dev)
        ws = torch.zeros(Kn.cp_step_ws_bytes(), dtype=torch.uint8, device=dev)
        how = {"rows": rows} if rec is None else dict(do_sample=rec[0], top_k=rec[1], top_p=rec[2],
                                                      temperature=rec[3], seed=rec[5])
        sa = Kn.sample(prev_logits, R, V, V, tok, step=step, substep=pos, codes=codes, codes_ld=12 * G, codes_w=G,
                       codes_col=pos - 1, codes_step_off=0, ctr_stride=1, philox_row=prow, emb=(tab_x, x, st.H),
                       emb2=(tab_q, q0, st.qkv_w), launch=not fused, **how)
        Kn.cp_step(st.layers, lm, x, q0, R, k2, v2, Lmax, pos, st.cos, st.sin, st.eps, logits, ws,
                   sample=sa if fused else None)
        torch.cuda.synchronize()
        assert int(ws[:4].view(torch.int32).item()) == 0, "hand-off poll gave up"
        return tok, codes, logits, k2, v2

    ref, fus = run(False), run(True)
    print(f"\n  R={R}: tokens {ref[0].tolist()} / {fus[0].tolist()}")
    assert torch.equal(ref[0], fus[0]) and torch.equal(ref[1], fus[1])
    assert torch.equal(ref[2], fus[2])
    for a, b in zip(ref[3] + ref[4], fus[3] + fus[4]):
        assert torch.equal(a, b)
    # the fused sampler read each row's own record: row r equals the fused scalar launch made with record r
    for r, rec in enumerate(records):
        assert int(run(True, rec=rec)[0][r]) == int(fus[0][r]), f"row {r}"
    assert len({int(t) for t in fus[0]}) > 1


# ------------------------------------------------------------------------------------------ end to end, tiny preset
@pytest.fixture(scope="module")
def tiny():
    from oracle import load_preset, synth_state_dict, talker_param_specs
    _dev()
    cfg, _ = load_preset("tiny-customvoice")
    W = {k: torch.from_numpy(v) for k, v in synth_state_dict(talker_param_specs(cfg)).items()}
    return cfg, W


def _eos_donor(cfg, W):
    """Weights whose EOS logit copies a token the tiny model does emit, so requests end at different frames."""
    z = np.load(os.path.join(GOLD, "tiny_talker.npz"))
    W = dict(W)
    head = W["talker.codec_head.weight"].clone()
    head[cfg["talker_config"]["codec_eos_token_id"]] = head[int(z["eos_b2/donor"])]
    W["talker.codec_head.weight"] = head
    return W


def _scalar_of(lists, i):
    return {k: v[i] for k, v in lists.items()}


MIX_A = dict(temperature=[0.3, 1.5, 0.9], top_k=[50, 0, 5], do_sample=[True, True, False],
             subtalker_top_k=[50, 10, 50], repetition_penalty=[1.05, 1.3, 1.0], seed=[7, 8, None])
MIX_B = dict(temperature=[1.2, 0.5, 0.7], top_k=[0, 20, 50], do_sample=[False, True, True],
             subtalker_top_k=[10, 50, 5], repetition_penalty=[1.0, 1.1, 1.2], seed=[None, 3, 4])
CALL_SEED = 9  # torch.manual_seed before a call: the seed of the requests whose entry is None (as for a scalar None)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_generate_per_request_parameters(tiny, dtype):
    """generate() with per-request lists: request i gets the codes (and hidden states) of the scalar call made with
    its values; a second call with another mix replays the same Session and the same captured frame graph."""
    from cases import make_inputs, talker_cases
    from qwen_tts.model import TTSModel
    cfg, W = tiny
    model = TTSModel(cfg, W, dtype=dtype)
    key = "cv_b3_auto_nospk"
    case = talker_cases()[key]
    ids, _, _, _ = make_inputs(case, list(talker_cases()).index(key), cfg["talker_config"]["hidden_size"])
    kw = dict(input_ids=ids, languages=case["languages"], speakers=case["speakers"], non_streaming_mode=False,
              max_new_tokens=20, subtalker_dosample=True)

    def call(**params):
        torch.manual_seed(CALL_SEED)
        return model.generate(**kw, **params)

    got_a = call(**MIX_A)
    sess = model.engine.all_sessions()
    assert len(sess) == 1 and not sess[0].busy
    graph = sess[0].graph
    assert graph is not None
    got_b = call(**MIX_B)
    assert model.engine.all_sessions() == sess and sess[0].graph is graph  # no new session, no re-capture
    refs = []
    for mix, got in ((MIX_A, got_a), (MIX_B, got_b)):
        for i in range(3):
            ref = call(**_scalar_of(mix, i))
            refs.append(ref[0])
            np.testing.assert_array_equal(got[0][i].numpy(), ref[0][i].numpy(), err_msg=f"request {i}")
            np.testing.assert_allclose(got[1][i].numpy(), ref[1][i].numpy(), atol=1e-5, rtol=1e-5)
    # non-vacuity: the scalar reference calls do not all produce the same codes for a row
    assert any(not torch.equal(refs[0][r], refs[j][r]) for j in range(1, 3) for r in range(3))


LISTS6 = dict(do_sample=[True, False, True, True, False, True], subtalker_dosample=[True, False, True, True, False, True],
              temperature=[0.6, 0.9, 1.1, 0.9, 0.9, 1.4], top_k=[50, 50, 0, 10, 50, 200],
              top_p=[1.0, 1.0, 1.0, 0.9, 1.0, 1.0], repetition_penalty=[1.05, 1.05, 1.2, 1.0, 1.05, 1.1],
              seed=[1, None, 3, 4, None, 6])


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_continuous_batching_per_request_parameters(tiny, dtype):
    """Six requests with six parameter sets through 2 and 4 refilled batch rows: per request the codes of the one-shot
    per-row call (a refilled slot decodes with its new request's record, not its predecessor's); the two greedy
    requests also equal a plain scalar greedy call (fp32)."""
    from cases import make_inputs
    from qwen_tts.model import TTSModel
    from test_gpu_parity import _serve_case
    cfg, W = tiny
    model = TTSModel(cfg, _eos_donor(cfg, W), dtype=dtype)
    case = _serve_case()
    ids, _, _, _ = make_inputs(case, 11, cfg["talker_config"]["hidden_size"])
    kw = dict(input_ids=ids, languages=case["languages"], speakers=case["speakers"], non_streaming_mode=False,
              max_new_tokens=case["max_new_tokens"])
    torch.manual_seed(CALL_SEED)
    ref, ref_h = model.generate(**kw, **LISTS6)
    assert len({c.shape[0] for c in ref}) > 1  # EOS-ragged: slots are refilled at different frames
    for mb in (2, 4):
        torch.manual_seed(CALL_SEED)
        codes, hid = model.generate(**kw, **LISTS6, max_batch=mb)
        mine = [x for x in model.engine.all_sessions() if x.B == mb]
        assert len(mine) == 1 and mine[0].rows_t is not None  # every mix of values in one session of mb rows
        for i, (a, b) in enumerate(zip(codes, ref)):
            np.testing.assert_array_equal(a.numpy(), b.numpy(), err_msg=f"max_batch={mb} request {i}")
            np.testing.assert_allclose(hid[i].numpy(), ref_h[i].numpy(), atol=1e-5, rtol=1e-5)
    if dtype == "fp32":
        greedy, _ = model.generate(**kw, do_sample=False, subtalker_dosample=False)
        for i in (1, 4):
            np.testing.assert_array_equal(ref[i].numpy(), greedy[i].numpy(), err_msg=f"greedy request {i}")
        assert any(not torch.equal(ref[i], greedy[i]) for i in (0, 2, 3, 5))


def test_stream_per_request_parameters(tiny):
    """stream() of two requests with their own temperatures: per row the chunks concatenate to generate() with the
    same lists + decode()."""
    from cases import make_inputs, talker_cases
    from oracle import codec_param_specs, load_preset, synth_state_dict
    from qwen_tts import Qwen3TTSTokenizer
    from qwen_tts.model import TTSModel
    cfg, W = tiny
    model = TTSModel(cfg, W, dtype="fp32")
    _, ccfg = load_preset("tiny-customvoice")
    CW = {k: torch.from_numpy(v) for k, v in synth_state_dict(codec_param_specs(ccfg)).items()}
    tok = Qwen3TTSTokenizer.from_pretrained("synthetic:tiny-customvoice/speech_tokenizer", dtype="fp32", weights=CW)
    model.load_speech_tokenizer(tok)
    key = "cv_b2_stream_dialect"
    case = talker_cases()[key]
    ids, ins, vcp, ref_ids = make_inputs(case, list(talker_cases()).index(key), cfg["talker_config"]["hidden_size"])
    kw = dict(input_ids=ids, instruct_ids=ins, ref_ids=ref_ids, voice_clone_prompt=vcp, languages=case["languages"],
              speakers=case["speakers"], non_streaming_mode=case["non_streaming_mode"], max_new_tokens=30,
              do_sample=True, subtalker_dosample=True, temperature=[0.5, 1.2], subtalker_temperature=[1.1, 0.7],
              seed=[5, 6])
    codes, _ = model.generate(**kw)
    same, _ = model.generate(**dict(kw, temperature=0.5, subtalker_temperature=1.1))
    assert torch.equal(codes[0], same[0]) and not torch.equal(codes[1], same[1])  # row 1 decodes at its own values
    wavs, _ = tok.decode([{"audio_codes": c} for c in codes])
    chunks = {}
    for b, pcm, last in model.stream(first_chunk_frames=3, chunk_frames=5, **kw):
        chunks.setdefault(b, []).append(pcm.cpu().numpy())
    assert sorted(chunks) == [0, 1]
    for b, w in enumerate(wavs):
        got = np.concatenate(chunks[b])
        assert got.shape == w.shape, (b, got.shape, w.shape)
        first = chunks[b][0]
        np.testing.assert_allclose(first, w[:first.shape[0]], atol=2e-4, rtol=0)
        np.testing.assert_allclose(got, w, atol=2e-4, rtol=0)


@pytest.mark.parametrize("bad", [dict(top_k=[50, 50, 50]), dict(temperature=[0.9, 0.0]), dict(top_p=[1.0, 1.5]),
                                 dict(temperature=[0.9, 1.0], seed=[1, 2, 3])])
def test_bad_per_request_lists_raise_before_a_session_is_taken(tiny, bad):
    from cases import make_inputs, talker_cases
    from qwen_tts.model import TTSModel
    cfg, W = tiny
    model = TTSModel(cfg, W, dtype="fp32")
    key = "cv_b2_stream_dialect"
    case = talker_cases()[key]
    ids, _, _, _ = make_inputs(case, list(talker_cases()).index(key), cfg["talker_config"]["hidden_size"])
    kw = dict(input_ids=ids, languages=case["languages"], speakers=case["speakers"],
              non_streaming_mode=case["non_streaming_mode"], max_new_tokens=8)
    model.generate(**kw, temperature=[0.8, 0.9])  # a session exists and is idle
    with pytest.raises(ValueError):
        model.generate(**kw, **bad)
    with pytest.raises(ValueError):
        model.generate(**kw, **bad, max_batch=1)
    assert model.engine.all_sessions() and not any(s.busy for s in model.engine.all_sessions())
