"""CPU checks of tests/attention_refs.py: the references, cases and judges that tests/test_gpu_attention_fp64.py pins
the attention kernels of csrc/attention.hip with.

* The references are the right operation: the RoPE tables are the oracle's (rope_cos_sin, bit for bit), RoPE equals
  oracle.talker.apply_rope and the attention equals a masked softmax written the obvious way, both to 1e-12 in fp64.
  oracle.talker.rmsnorm normalises in fp32 whatever it is given, so it cannot be met to 1e-12 by an fp64 value: the
  reference's fp32 form reproduces it bit for bit instead (same operations in the same order), and the fp64 form is
  that formula widened.
* The judges can tell a wrong kernel from a right one.  At every launch of the GPU tests a "kernel" in plain torch fp32
  (bf16 where the kernel's output is bf16) passes the very judge functions the GPU tests call -- so the caps are
  reachable -- and each mutant of it fails them:
    drop_last_cached   the key before the row's own is skipped
    window_late/early  the window starts one key late / early
    no_row_start       row_start ignored
    interleaved_heads  q head h reads kv head h % Hkv instead of h // NREP
    rope_at_kv_pos     RoPE at kv_pos instead of rope_pos
    unrounded_new_key  the new key used as computed although the cache is bf16
    k_weight_on_q      K's RMSNorm weight applied to q
  A mutant that cannot differ at a launch (no window, NREP 1, no norm, an fp32 cache, one key, no such input) is
  asserted to be exactly that: not applicable for the structural reason written next to it, never silently.
"""
import pytest
import torch

import attention_refs as A

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
ATT_MUTANTS = ("drop_last_cached", "window_late", "window_early", "no_row_start", "interleaved_heads")


# ------------------------------------------------------------------------------------------ the references
@pytest.mark.parametrize("D,Hq,Hkv", [(128, 16, 8), (16, 4, 2)])
def test_references_agree_with_the_oracle(D, Hq, Hkv):
    from oracle.talker import apply_rope, rmsnorm, rope_cos_sin
    c = A.attn_inputs(D, Hq, Hkv, F32, True)
    R, half = 64, D // 2
    pos = torch.tensor(c.rope_pos[:R])
    oc, os_ = rope_cos_sin(pos[None], D, A.ROPE_THETA)  # [1][R][D], the two halves equal
    assert torch.equal(oc[0, :, :half], c.cos[pos]) and torch.equal(os_[0, :, half:], c.sin[pos])
    x = c.qkv[:R].view(R, Hq + 2 * Hkv, D)
    xq = x[:, :Hq]
    assert torch.equal(A.head_rmsnorm(xq, c.q_norm, c.eps, F32), rmsnorm(xq, c.q_norm, A.f32_scalar(c.eps)))
    n32, n64 = A.head_rmsnorm(xq, c.q_norm, c.eps, F32), A.head_rmsnorm(xq, c.q_norm, c.eps)
    assert float(((n32.double() - n64).abs() / n64.abs().clamp_min(1e-30)).max()) < 4 * 2.0 ** -23
    want = apply_rope(n64.transpose(0, 1)[None], oc.double(), os_.double())[0].transpose(0, 1)  # [R][Hq][D]
    torch.testing.assert_close(A.rope(n64, c.cos, c.sin, c.rope_pos[:R]), want, atol=1e-12, rtol=1e-12)
    q, k, v = A.qkv_post_ref(c.qkv[:R], Hq, Hkv, D, c.q_norm, c.k_norm, c.eps, c.cos, c.sin, c.rope_pos[:R], F32)
    torch.testing.assert_close(q, want, atol=1e-12, rtol=1e-12)
    assert torch.equal(v, x[:, Hq + Hkv:].double())
    # attention: a masked softmax over the whole cache, written the obvious way
    g = torch.Generator().manual_seed(D)
    L, nrep = 40, Hq // Hkv
    K, V = torch.randn(Hkv, L, D, generator=g), torch.randn(Hkv, L, D, generator=g)
    for start, length, window in ((0, 40, 0), (3, 17, 0), (0, 40, 5), (30, 40, 20), (0, 4, 72), (7, 8, 0)):
        s = torch.einsum("hd,hld->hl", q[0], K.double().repeat_interleave(nrep, 0)) / D ** 0.5
        j = torch.arange(L)
        allowed = (j >= start) & (j < length)
        if window:
            allowed &= j >= length - window
        want = torch.einsum("hl,hld->hd", torch.softmax(s.masked_fill(~allowed, float("-inf")), -1),
                            V.double().repeat_interleave(nrep, 0))
        torch.testing.assert_close(A.attention_ref(q[0], K, V, start, length, window), want, atol=1e-12, rtol=1e-12)


def test_kernel_strides():
    """The strides the cases are built from, at the model's head dims (the kernels' own definitions, spelled out)."""
    assert [A.attn_rows_block_keys(D) for D in (16, 64, 128)] == [128, 32, 16]
    assert A.decode_waves(64, 2) == 4 and A.decode_waves(65, 2) == 8 and A.decode_waves(64, 4) == 8
    assert A.decode_gic(128, BF16, 8) == 128 and A.decode_gic(128, F32, 8) == 64 and A.decode_gic(16, BF16, 4) == 512
    assert A.oproj_batch_keys(128, 2) == 16 and A.oproj_batch_keys(128, 4) == 8 and A.oproj_batch_keys(16, 4) == 64
    x = torch.tensor([1.0, 3.0, 0.75], dtype=F64)
    assert A.bf16_step(x).tolist() == [2.0 ** -7, 2.0 ** -6, 2.0 ** -8]


# ------------------------------------------------------------------------------------------ plain fp32 "kernels" and mutants
def _sim_qkv(c, qkv, rope_pos, kv_pos, mutant):
    """(q, k, v) in fp32, k / v not yet rounded to the cache's dtype."""
    qn = c.k_norm if mutant == "k_weight_on_q" else c.q_norm
    pos = kv_pos if mutant == "rope_at_kv_pos" else rope_pos
    return A.qkv_post_ref(qkv, c.Hq, c.Hkv, c.D, qn, c.k_norm, c.eps, c.cos, c.sin, pos, F32, F32)


def _sim_attention(c, q, Kw, Vw, row_batch, row_start, row_len, window, mutant, knew=None):
    """Plain fp32 attention rows with one mutation -> (out [R][Hq][D], whether the mutation changed any row's inputs)."""
    outs, changed = [], False
    for r, (b, s, n) in enumerate(zip(row_batch, row_start, row_len)):
        lo, hi = A.key_range(s, n, window)
        keys, hm, K = slice(lo, hi), None, Kw[b]
        if mutant == "drop_last_cached" and hi - lo >= 2:
            keys, changed = torch.tensor(list(range(lo, hi - 2)) + [hi - 1]), True
        elif mutant in ("window_late", "window_early") and window > 0:
            lo2, _ = A.key_range(s, n, window - 1 if mutant == "window_late" else window + 1)
            keys, changed = slice(lo2, hi), changed or lo2 != lo
        elif mutant == "no_row_start":
            lo2, _ = A.key_range(0, n, window)
            keys, changed = slice(lo2, hi), changed or lo2 != lo
        elif mutant == "interleaved_heads":
            hm = [h % c.Hkv for h in range(c.Hq)]
            changed = changed or hm != [h // (c.Hq // c.Hkv) for h in range(c.Hq)]
        elif mutant == "unrounded_new_key":
            K = Kw[b].float().clone()
            changed = changed or not torch.equal(K[:, hi - 1], knew[r])
            K[:, hi - 1] = knew[r]
        outs.append(A.attend(q[r], K, Vw[b], keys, F32, hm))
    return torch.stack(outs), changed


def _all_ok(recs):
    return all(ok for _, _, ok, _, _ in recs)


def _show(kernel, case, recs):
    for line in A.format_records(kernel, case, recs):
        print(line)


# ------------------------------------------------------------------------------------------ a. qkv_post + attention
@pytest.mark.parametrize("D,Hq,Hkv,kv,norm", A.ATTN_CASES)
def test_attention_rows_judges(D, Hq, Hkv, kv, norm):
    c = A.attn_inputs(D, Hq, Hkv, kv, norm)
    case = f"D{D} Hq{Hq} Hkv{Hkv} kv {kv} norm {norm}"
    K0 = torch.full((c.B, Hkv, c.Lmax, D), A.SENTINEL).to(kv)
    V0 = K0.clone()

    def stage1(mutant):
        q, k, v = _sim_qkv(c, c.qkv, c.rope_pos, c.kv_pos, mutant)
        Kw, Vw = A.append_rows(K0, V0, k, v, c.row_batch, c.kv_pos)
        return q.flatten(1), Kw, Vw
    q, Kw, Vw = stage1(None)
    recs = A.judge_qkv_post(c, K0, V0, q, Kw, Vw)
    _show("qkv_post", case, recs)
    assert _all_ok(recs)
    assert bool((Kw[1] == A.SENTINEL).all()) and bool((Kw[3] == A.SENTINEL).all())  # the slots no row names
    assert not _all_ok(A.judge_qkv_post(c, K0, V0, *stage1("rope_at_kv_pos")))  # rope_pos = kv_pos + 5 in sequence 0
    if norm:
        assert not _all_ok(A.judge_qkv_post(c, K0, V0, *stage1("k_weight_on_q")))
    for L in c.launches:
        memo = {}
        qs = q.view(-1, Hq, D)[torch.tensor(L.q_rows)]
        args = (c, qs, Kw, Vw, L.row_batch, L.row_start, L.row_len, L.window)
        out, _ = _sim_attention(*args, None)
        for od in (F32, BF16) if kv == BF16 else (F32,):  # bf16 output goes with bf16 caches
            recs = A.judge_attention(c, L, q, Kw, Vw, out.to(od), memo)
            _show("attention", f"{case} {L.name} out {od}", recs)
            assert _all_ok(recs), (L.name, od, recs)
        for m in ATT_MUTANTS:
            mut, changed = _sim_attention(*args, m)
            applicable = {"window_late": L.window > 0, "window_early": L.window > 0,  # the launch has a window
                          "interleaved_heads": Hq != Hkv}.get(m, True)               # NREP 1: the two maps are one
            assert changed == applicable, (L.name, m)
            for od in (F32, BF16) if kv == BF16 else (F32,):
                if applicable:
                    assert not _all_ok(A.judge_attention(c, L, q, Kw, Vw, mut.to(od), memo)), (L.name, m, od)


# ------------------------------------------------------------------------------------------ b. decode attention
def _decode_like(c, L, judge, kernel, case, window_expected, has_positions=True):
    """A launch of a kernel that appends the new key itself (decode, small prefill): plain fp32 passes `judge` at both
    output dtypes, every applicable mutant fails it."""
    def sim(mutant):
        q, k, v = _sim_qkv(c, L.qkv, L.rope_pos, L.kv_pos, mutant)
        Kw, Vw = A.append_rows(L.Kc, L.Vc, k, v, L.row_batch, L.kv_pos)
        out, changed = _sim_attention(c, q, Kw, Vw, L.row_batch, L.row_start, [p + 1 for p in L.kv_pos], L.window, mutant, k)
        return Kw, Vw, out.flatten(1), changed
    Kw, Vw, out, _ = sim(None)
    memo = {}
    for od in (F32, BF16):
        recs = judge(c, L, Kw, Vw, out.to(od), memo=memo)
        _show(kernel, f"{case} {L.name} out {od}", recs)
        assert _all_ok(recs), (L.name, od, recs)
    applicable = {
        "drop_last_cached": any(p > s for s, p in zip(L.row_start, L.kv_pos)),
        "window_late": window_expected, "window_early": window_expected,  # a window that cuts some row
        "no_row_start": any(s > 0 for s in L.row_start),
        "interleaved_heads": c.Hq != c.Hkv,                               # NREP 1: the two maps are one
        "rope_at_kv_pos": has_positions and L.rope_pos != L.kv_pos,      # the kernel takes a rope_pos of its own
        "unrounded_new_key": c.kv_dtype == BF16,                          # an fp32 cache holds the key as computed
        "k_weight_on_q": c.norm,
    }
    for m, app in applicable.items():
        mKw, mVw, mout, changed = sim(m)
        if m in ATT_MUTANTS or m == "unrounded_new_key":
            assert changed == app, (L.name, m, changed)
        if not app:
            continue
        same_cache = torch.equal(mKw, Kw) and torch.equal(mVw, Vw)
        for od in (F32, BF16):
            assert not _all_ok(judge(c, L, mKw, mVw, mout.to(od), memo=memo if same_cache else None)), (L.name, m, od)


@pytest.mark.parametrize("D,Hq,Hkv,kv,short", A.DECODE_CASES)
def test_decode_judges(D, Hq, Hkv, kv, short):
    c = A.decode_inputs(D, Hq, Hkv, kv, short)
    assert c.waves == (4 if short else 8) and (c.Lmax <= 64) == short
    for L in c.launches + [A.decode_const_pos_launch(c)[0]]:
        cut = L.window > 0 and any(p + 1 > L.window - 1 for p in L.kv_pos)  # w72 at Lmax 64: no row reaches the window
        if L.name == "keys":
            n = {p + 1 - s for s, p in zip(L.row_start, L.kv_pos)}
            assert {1, 2, 3, 8, min(c.gic, c.Lmax)} <= n and (short or {c.gic - 1, c.gic + 1, 2 * c.gic, 3 * c.gic + 5} <= n)
        _decode_like(c, L, A.judge_decode, "decode", f"D{D} Hq{Hq} Hkv{Hkv} kv {kv} waves {c.waves}", cut)


# ------------------------------------------------------------------------------------------ c. small prefill
@pytest.mark.parametrize("D,Hq,Hkv,kv,norm", A.PREFILL_CASES)
def test_small_prefill_judges(D, Hq, Hkv, kv, norm):
    c = A.prefill_inputs(D, Hq, Hkv, kv, norm)
    _decode_like(c, A.prefill_launch(c), A.judge_prefill, "small_prefill", f"D{D} Hq{Hq} Hkv{Hkv} kv {kv} norm {norm}",
                 False, has_positions=False)


# ------------------------------------------------------------------------------------------ d. fused attention + o_proj
@pytest.mark.parametrize("D,Hq,Hkv,Lk,N,B,dt", A.OPROJ_CASES)
def test_oproj_judges(D, Hq, Hkv, Lk, N, B, dt):
    c = A.oproj_inputs(D, Hq, Hkv, Lk, N, B, dt)
    case = f"D{D} Hq{Hq} Hkv{Hkv} L{Lk} N{N} {dt}"
    for L in c.launches:
        def sim(mutant):
            q, k, v = _sim_qkv(c, L.qkv, L.rope_pos, L.kv_pos, mutant)
            Kw, Vw = A.append_rows(L.Kc, L.Vc, k, v, L.row_batch, L.kv_pos)
            att, changed = _sim_attention(c, q, Kw, Vw, L.row_batch, L.row_start, [p + 1 for p in L.kv_pos], 0, mutant, k)
            return Kw, Vw, A.oproj_ref(L.x, att.flatten(1), c.W, dt == BF16, F32), changed
        Kw, Vw, x, _ = sim(None)
        memo = {}
        recs = A.judge_oproj(c, L, Kw, Vw, x, memo)
        _show("attn_oproj", f"{case} {L.name}", recs)
        assert _all_ok(recs), (L.name, recs)
        applicable = {
            "drop_last_cached": any(p > s for s, p in zip(L.row_start, L.kv_pos)),
            "no_row_start": any(s > 0 for s in L.row_start),
            "interleaved_heads": Hq != Hkv,
            "rope_at_kv_pos": L.rope_pos != L.kv_pos,  # const_pos is one position for both
            "unrounded_new_key": dt == BF16 and any(p > s for s, p in zip(L.row_start, L.kv_pos)),  # likewise
            "k_weight_on_q": any(p > s for s, p in zip(L.row_start, L.kv_pos)),  # one key: its weight is 1 whatever q is
        }  # the kernel has no window
        for m, app in applicable.items():
            mKw, mVw, mx, changed = sim(m)
            if m in ATT_MUTANTS:
                assert changed == app, (L.name, m, changed)
            if app:
                same_cache = torch.equal(mKw, Kw) and torch.equal(mVw, Vw)
                assert not _all_ok(A.judge_oproj(c, L, mKw, mVw, mx, memo if same_cache else None)), (L.name, m)
