"""The stand-alone attention kernels of csrc/attention.hip through qwen_tts.kernels, each against the fp64 reference of
tests/attention_refs.py on that file's seeded cases: qkv_post_k + attn_rows_k, attn_decode_k (split-KV, const_pos and
the sliding window included), attn_small_prefill_k, and the (column group, row) form of attn_oproj_k.

One launch carries many rows with their own key ranges, so the key counts at which a kernel's loops take another path
(1, 2, one block iteration / chunk of keys -1 / +0 / +1, the softmax stride, several chunks) sit in a handful of
launches.  Outputs and caches start at a sentinel, which must survive wherever the kernel has no business writing.
The fp64 reference runs on the device.  Each stage is judged from its own input: the attention from the q rows and
the caches the launch before it (or the kernel itself) actually wrote.

Bounds (none of them taken from what the kernels give; tests/test_attention_refs.py shows that plain torch fp32 meets
them at every launch and that eight mutants of the computation do not):
* fp32 outputs: |got - ref64| <= max(margin x e32 x scale, 4 ulp32(scale)) per element, scale the (row, head)'s
  largest |ref64|, e32 the largest scaled error of plain torch fp32 over the same launch.
  margin 2 for qkv_post_k, attn_rows_k, attn_small_prefill_k: expf and a summation order of the same kind as torch's
  (the project's margin for a reordered fp32 sum).  margin 4 for attn_decode_k and attn_oproj_k: they scale the scores
  by log2(e) (the exponent's absolute rounding error grows 1.44 x), use the hardware exp2 (1 ulp) where torch uses
  expf, and merge online-softmax partials with extra rescales: 2 for the reordering x 2 for these.
* bf16 outputs and bf16 cache rows: small_kernel_refs.bf16_cap, at most one bf16 step from the fp64 value rounded once,
  equal on >= 99.9 %, on tensors of >= 4096 elements.  The builders keep the judged reference elements at >= 2^-10 of
  their row's scale (attention_refs.HAZARD), where one bf16 step is above the fp32 tolerance.
* x of the fused o_proj: fp32 weights margin 4 against x + A64 @ W^T; bf16 weights against x + to_bf16(A64) @ W^T with
  the margin-4 tolerance of that formula in fp32 plus ceil(0.001 Hq D) flips of the A operand, each one bf16 step at
  the row's largest |A| times max |W| (attention_refs.oproj_bf16_tolerance).
The head-split form of the fused o_proj (`ws` given) rounds q and the softmax weights to bf16 by design and stays
anchored to the (column group, row) form (tests/test_gpu_cp_engine.py), which these tests tie to fp64.

measured on the MI355X (profiles/attention_fp64_errors.txt: kernel vs fp64, torch-fp32 vs fp64, their ratio per launch):
  worst kernel / torch ratio: qkv_post_k q 1.08, k rows 1.06; attn_rows_k 1.00; attn_small_prefill_k out 1.33, k rows
  1.32; attn_decode_k out 1.88 (4.1e-7 against 2.2e-7, window 5), k rows 1.19; attn_oproj_k k rows 1.36, x (fp32
  weights) at most 1.00.  bf16 outputs and cache rows: never more than one step, equal on >= 99.967 %.  x with bf16
  weights: up to one row in ten of a launch needed the flip allowance (one flipped A element shifts the whole row),
  none exceeded it.
"""
import pytest
import torch

import attention_refs as A

pytestmark = pytest.mark.gpu

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
S = A.SENTINEL


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _kn():
    from qwen_tts import kernels
    return kernels


def _sent(shape, dtype, dev):
    return torch.full(shape, S, dtype=dtype, device=dev)


def _is_sent(t):
    return bool((t == S).all())


def _tables(Kn, c, dev):
    cos, sin = Kn.rope_tables(c.D, A.ROPE_THETA, c.cos.shape[0], dev)
    assert torch.equal(cos, c.cos) and torch.equal(sin, c.sin)  # the references read the kernels' own tables
    return cos, sin


class _Report:
    """Prints every figure as it comes, asserts at the end."""

    def __init__(self, kernel, case):
        self.kernel, self.case, self.bad = kernel, case, []

    def add(self, launch, recs):
        for line in A.format_records(self.kernel, f"{self.case} {launch}", recs):
            print(line)
        self.bad += [(launch, r) for r in recs if not r[2]]

    def check(self, launch, ok, what):
        if not ok:
            print(f"fp64pin | {self.kernel} | {self.case} {launch} | {what} | FAIL")
            self.bad.append((launch, what))

    def done(self):
        assert not self.bad, self.bad


def _name(dt):
    return "bf16" if dt == BF16 else "fp32"


# ------------------------------------------------------------------------------------------ a. qkv_post + attention
@pytest.mark.parametrize("D,Hq,Hkv,kv,norm", A.ATTN_CASES)
def test_qkv_post_and_attention_rows(D, Hq, Hkv, kv, norm):
    Kn, dev = _kn(), _dev()
    c = A.to_device(A.attn_inputs(D, Hq, Hkv, kv, norm), dev)
    rep = _Report("qkv_post+attn_rows", f"D{D} Hq{Hq} Hkv{Hkv} kv {_name(kv)} norm {int(norm)}")
    i32 = lambda t: torch.tensor(t, dtype=torch.int32, device=dev)  # noqa: E731
    cos, sin = _tables(Kn, c, dev)
    K0, V0 = _sent((c.B, Hkv, c.Lmax, D), kv, dev), _sent((c.B, Hkv, c.Lmax, D), kv, dev)
    Kw, Vw = K0.clone(), V0.clone()
    q = _sent((c.R + 1, Hq * D), F32, dev)
    Kn.qkv_post(c.qkv, c.R, Hq, Hkv, D, c.q_norm, c.k_norm, c.eps, cos, sin, i32(c.rope_pos), i32(c.row_batch),
                i32(c.kv_pos), q, Kw, Vw, c.Lmax)
    rep.add("qkv_post", A.judge_qkv_post(c, K0, V0, q[:c.R], Kw, Vw))
    rep.check("qkv_post", _is_sent(q[c.R:]) and _is_sent(Kw[1]) and _is_sent(Vw[3]), "sentinel")
    Kb, Vb = Kw.clone(), Vw.clone()
    for L in c.launches:
        memo, RL = {}, len(L.q_rows)
        qs = q[torch.tensor(L.q_rows, device=dev)].contiguous()
        for od in (F32, BF16) if kv == BF16 else (F32,):  # qt_attention writes bf16 only from bf16 caches
            out = _sent((RL + 1, Hq * D), od, dev)
            Kn.attention(qs, RL, Hq, Hkv, D, Kw, Vw, c.Lmax, i32(L.row_batch), i32(L.row_start), i32(L.row_len), out,
                         L.max_keys, window=L.window)
            rep.add(f"{L.name} out {_name(od)}", A.judge_attention(c, L, q[:c.R], Kw, Vw, out[:RL], memo))
            rep.check(L.name, _is_sent(out[RL:]) and torch.equal(Kw, Kb) and torch.equal(Vw, Vb), "sentinel / caches")
    rep.done()


# ------------------------------------------------------------------------------------------ b. decode attention
def _decode(Kn, c, L, cos, sin, od, dev, **kw):
    i32 = lambda t: torch.tensor(t, dtype=torch.int32, device=dev)  # noqa: E731
    Kw, Vw = L.Kc.clone(), L.Vc.clone()
    out = _sent((L.R + 1, c.Hq * c.D), od, dev)
    Kn.decode_attention(L.qkv, L.R, c.Hq, c.Hkv, c.D, c.q_norm, c.k_norm, c.eps, cos, sin, i32(L.rope_pos), i32(L.row_batch),
                        i32(L.kv_pos), i32(L.row_start), Kw, Vw, c.Lmax, out, window=L.window, **kw)
    return Kw, Vw, out


@pytest.mark.parametrize("D,Hq,Hkv,kv,short", A.DECODE_CASES)
def test_decode_attention(D, Hq, Hkv, kv, short):
    Kn, dev = _kn(), _dev()
    c = A.decode_inputs(D, Hq, Hkv, kv, short)
    Lc, P = A.decode_const_pos_launch(c)
    c, Lc = A.to_device(c, dev), A.to_device(Lc, dev)
    assert c.waves == A.decode_waves(c.Lmax, Hq // Hkv)
    rep = _Report("decode", f"D{D} Hq{Hq} Hkv{Hkv} kv {_name(kv)} waves {c.waves}")
    cos, sin = _tables(Kn, c, dev)
    for L in c.launches:
        memo, first = {}, None
        runs = [(_name(od), od, {}) for od in (F32, BF16)]
        if L.name == "keys":  # the key counts include n < nsplit (empty splits) and n = nsplit
            runs += [(f"nsplit {ns}", F32, dict(nsplit=ns)) for ns in A.DECODE_SPLITS]
        for tag, od, kw in runs:
            ws = None
            if kw:
                ws = torch.zeros(Kn.decode_attn_ws_bytes(L.R, Hq, Hkv, D, kw["nsplit"]), dtype=torch.uint8, device=dev)
            Kw, Vw, out = _decode(Kn, c, L, cos, sin, od, dev, ws=ws, **kw)
            first = first or (Kw, Vw)
            same = torch.equal(Kw, first[0]) and torch.equal(Vw, first[1])  # the append knows no output dtype, no split
            rep.check(f"{L.name} {tag}", same, "appended rows differ between launches of one input")
            rep.add(f"{L.name} {tag}", A.judge_decode(c, L, Kw, Vw, out[:L.R], memo=memo if same else None))
            rep.check(f"{L.name} {tag}", _is_sent(out[L.R:]), "sentinel")
            if ws is not None:
                rep.check(f"{L.name} {tag}", not ws[:4096].any(), "arrival counters not back at zero")
    # const_pos against the same positions through the arrays: bit-equal
    Ka, Va, oa = _decode(Kn, c, Lc, cos, sin, F32, dev)
    Kc, Vc, oc = _decode(Kn, c, Lc, cos, sin, F32, dev, const_pos=P)
    rep.check("const_pos", torch.equal(oa, oc) and torch.equal(Ka, Kc) and torch.equal(Va, Vc), "const_pos != arrays")
    rep.add("const_pos", A.judge_decode(c, Lc, Kc, Vc, oc[:Lc.R]))
    rep.done()


# ------------------------------------------------------------------------------------------ c. small prefill
@pytest.mark.parametrize("D,Hq,Hkv,kv,norm", A.PREFILL_CASES)
def test_small_prefill_attention(D, Hq, Hkv, kv, norm):
    Kn, dev = _kn(), _dev()
    c = A.to_device(A.prefill_inputs(D, Hq, Hkv, kv, norm), dev)
    L = A.prefill_launch(c)
    rep = _Report("small_prefill", f"D{D} Hq{Hq} Hkv{Hkv} kv {_name(kv)} norm {int(norm)}")
    cos, sin = _tables(Kn, c, dev)
    memo, first = {}, None
    for od in (F32, BF16):
        Kw, Vw = L.Kc.clone(), L.Vc.clone()
        out = _sent((c.R + 1, Hq * D), od, dev)
        Kn.small_prefill_attention(c.qkv, c.R, 2, Hq, Hkv, D, c.q_norm, c.k_norm, c.eps, cos, sin, Kw, Vw, c.Lmax, out)
        first = first or (Kw, Vw)
        same = torch.equal(Kw, first[0]) and torch.equal(Vw, first[1])
        rep.check(_name(od), same, "appended rows differ between launches of one input")
        rep.add(f"out {_name(od)}", A.judge_prefill(c, L, Kw, Vw, out[:c.R], memo=memo if same else None))
        rep.check(_name(od), _is_sent(out[c.R:]) and _is_sent(Kw[:, :, 2:]) and _is_sent(Vw[:, :, 2:]), "sentinel")
    rep.done()


# ------------------------------------------------------------------------------------------ d. fused attention + o_proj
@pytest.mark.parametrize("D,Hq,Hkv,Lk,N,B,dt", A.OPROJ_CASES)
def test_decode_attn_oproj(D, Hq, Hkv, Lk, N, B, dt):
    Kn, dev = _kn(), _dev()
    c = A.to_device(A.oproj_inputs(D, Hq, Hkv, Lk, N, B, dt), dev)
    rep = _Report("attn_oproj", f"D{D} Hq{Hq} Hkv{Hkv} L{Lk} N{N} {_name(dt)}")
    i32 = lambda t: torch.tensor(t, dtype=torch.int32, device=dev)  # noqa: E731
    cos, sin = _tables(Kn, c, dev)
    wo = Kn.tile_linear(c.W, dt)  # c.W is already in dt: the tiled weight stores exactly these values
    for L in c.launches:
        Kw, Vw = L.Kc.clone(), L.Vc.clone()
        xb = _sent((L.R + 1, N + 8), F32, dev)  # a slice of a wider buffer: ldx > N
        xb[:L.R, :N] = L.x
        pos = dict(const_pos=L.const_pos) if L.const_pos >= 0 else \
            dict(rope_pos=i32(L.rope_pos), kv_pos=i32(L.kv_pos), row_start=i32(L.row_start))
        Kn.decode_attn_oproj(L.qkv, L.R, Hq, Hkv, D, c.q_norm, c.k_norm, c.eps, cos, sin, Kw, Vw, c.Lmax, wo, xb, **pos)
        rep.add(L.name, A.judge_oproj(c, L, Kw, Vw, xb[:L.R, :N]))
        rep.check(L.name, _is_sent(xb[L.R:]) and _is_sent(xb[:, N:]), "sentinel")
    rep.done()
