"""TalkerEngine._run_frame_held: a row held out of some frame replays decodes what it decodes without.

Engine level.  A batch is prefilled once per run; the reference run replays the plain frame, the other run holds rows
out of replays with _run_frame_held.  After every replay of the held run, a row that has taken part in F replays is
compared with the reference run after F replays, bit for bit: its codes (frames [0, F) and the next cb0), `seen`,
`past_hidden`, its five counters, tok0, `finished`, its cb0 embedding row of cp_x, and hiddens[b, :F + 1].

tiny-customvoice, B = 3, 12 replays: row 0 never held, row 1 at replays {0, 1, 5}, row 2 at {2, 3, 4, 7} -- the first
replay after the prefill, and consecutive holds (saved once, restored after each) -- in fp32 and bf16, greedy and
sampled, with captured graphs, and once issued eagerly.  One case at the 0.6b-customvoice dims in bf16 (the weight
recipe of test_gpu_full.py), B = 2, 8 replays, row 1 held at {0, 1, 4}, captured graphs: the held rows pass through
the code-predictor step engine and the talker tail engine."""
import pytest
import torch

pytestmark = pytest.mark.gpu

HOLDS3 = [set(), {0, 1, 5}, {2, 3, 4, 7}]
FIELDS = ("seen", "past_hidden", "tok0", "finished")


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def tiny():
    _dev()
    from oracle import load_preset, synth_state_dict, talker_param_specs
    from qwen_tts.model import TTSModel
    cfg, _ = load_preset("tiny-customvoice")
    W = {k: torch.from_numpy(v) for k, v in synth_state_dict(talker_param_specs(cfg)).items()}
    return {d: TTSModel(cfg, W, dtype=d) for d in ("fp32", "bf16")}


def _snap(s):
    torch.cuda.synchronize()
    out = {k: getattr(s, k).cpu().clone() for k in FIELDS}
    out["ctr"] = s.ctr.view(5, s.B).cpu().clone()
    out["codes"] = s.codes.cpu().clone()
    out["hiddens"] = s.hiddens.cpu().clone()
    out["cb0_emb"] = s.cp_x[1::2].cpu().clone()
    if s.cp_x16 is not None:
        out["cb0_emb16"] = s.cp_x16[1::2].view(torch.int16).cpu().clone()
    return out


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _run(model, texts, langs, spks, holds, replays, use_graph, sample):
    """snapshots after the prefill and after every replay, and the frames each row had taken part in by then"""
    from cases import text_ids
    from qwen_tts import kernels as K
    from qwen_tts.talker import GenParams, check_handoffs
    eng = model.engine
    ids = [text_ids(n, 300 + j) for j, n in enumerate(texts)]
    emb, mask, trail, pad = model.build_prompts(ids, langs, spks, None, False)
    B, P = emb.shape[0], emb.shape[1]
    gp = GenParams(max_new_tokens=replays + 8, do_sample=sample, subtalker_dosample=sample, ignore_eos=True, seed=11)
    s = eng.session(B, P, gp.max_new_tokens - 1, gp)
    try:
        with K.use_workspace(s.ws):
            eng._prefill(s, emb, mask, trail, pad, gp.resolve_seed())
        s.hiddens[:, 0].copy_(s.past_hidden)
        snaps, done, F = [_snap(s)], [[0] * B], [0] * B
        for r in range(replays):
            mask_r = sum(1 << b for b in range(B) if r in holds[b])
            eng._run_frame_held(s, P + r + 1, mask_r, use_graph)
            F = [F[b] + (0 if r in holds[b] else 1) for b in range(B)]
            snaps.append(_snap(s))
            done.append(list(F))
        check_handoffs([s])
        return snaps, done
    finally:
        eng.release([s])


def _compare(ref, got, done, what):
    for r, (snap, F) in enumerate(zip(got, done)):
        for b, f in enumerate(F):
            want = ref[f]
            where = f"{what}: after replay {r - 1}, row {b} at frame {f}"
            assert torch.equal(snap["codes"][b, :f], want["codes"][b, :f]), where
            assert snap["codes"][b, f, 0] == want["codes"][b, f, 0], where
            assert torch.equal(snap["ctr"][:, b], want["ctr"][:, b]), where
            assert int(snap["ctr"][0, b]) == f, where
            for k in FIELDS + ("cb0_emb",) + (("cb0_emb16",) if "cb0_emb16" in snap else ()):
                assert torch.equal(_bits(snap[k][b]), _bits(want[k][b])), (where, k)
            assert torch.equal(_bits(snap["hiddens"][b, :f + 1]), _bits(want["hiddens"][b, :f + 1])), where


@pytest.mark.parametrize("sample", [False, True])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_held_rows_decode_what_they_decode_without_holds(tiny, dtype, sample):
    args = ([12, 5, 9], ["auto", "english", "japanese"], ["", None, "dylan"])
    ref, ref_done = _run(tiny[dtype], *args, [set()] * 3, 12, True, sample)
    assert ref_done[-1] == [12, 12, 12]
    got, done = _run(tiny[dtype], *args, HOLDS3, 12, True, sample)
    assert done[-1] == [12, 9, 8]
    _compare(ref, got, done, f"{dtype} sample={sample}")


def test_held_rows_issued_eagerly(tiny):
    args = ([12, 5, 9], ["auto", "english", "japanese"], ["", None, "dylan"])
    ref, _ = _run(tiny["fp32"], *args, [set()] * 3, 12, False, False)
    got, done = _run(tiny["fp32"], *args, HOLDS3, 12, False, False)
    _compare(ref, got, done, "fp32 eager")


def test_held_rows_through_the_engines_at_0p6b_dims():
    _dev()
    from oracle import load_preset, synth_state_dict, talker_param_specs
    from qwen_tts.model import TTSModel
    cfg, _ = load_preset("0.6b-customvoice")
    W = {k: torch.from_numpy(v) for k, v in synth_state_dict(talker_param_specs(cfg), threads=16).items()}
    model = TTSModel(cfg, W, dtype="bf16")
    eng = model.engine
    print(f"code-predictor step engine: {eng.cp_engine}, talker tail engine: {eng.talker_tail}")
    args = ([20, 14], ["english", "english"], ["vivian", "vivian"])
    ref, _ = _run(model, *args, [set(), set()], 8, True, False)
    got, done = _run(model, *args, [set(), {0, 1, 4}], 8, True, False)
    assert done[-1] == [8, 5]
    _compare(ref, got, done, "0.6b bf16")
