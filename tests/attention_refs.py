"""Plain references for the stand-alone attention kernels (csrc/attention.hip), the seeded input builders that the
CPU and the GPU tests share, and the judges.

torch only, no project imports; every function runs on CPU or GPU tensors.  Every reference takes a `dtype`:
float64 (the default) is the reference proper, float32 is the "plain torch fp32" computation whose own error
against fp64 the fp32 tolerances are scaled from (small_kernel_refs.fp32_tolerance).  Both read the stored
operands widened to `dtype`: the fp32 qkv rows, the norm weights, the fp32 cos / sin tables, the cache in its own
dtype.

Stages, each judged from its own input (as tests/test_gpu_engine_stages.py does):
  qkv_post_ref     q/k RMSNorm over head_dim (optional), rotate-half RoPE at rope_pos, V unchanged -> q and the
                   k / v rows as the cache will hold them
  attention_ref    GQA softmax(q.k / sqrt(D)) V over the keys [max(start, length - window), length) of a cache
  oproj_ref        x + A @ W^T with the stored weight widened, A exact or rounded once to bf16 (the MFMA's A operand)
and thin wrappers for the contracts of qt_decode_attention, qt_small_prefill_attention and qt_decode_attn_oproj.

Cases: a case is one kernel launch -- a head layout, dtypes, and a list of rows with their own key ranges, so that
one launch carries the key counts at which the kernel's loops take another path.  The strides are computed here from
D, the cache dtype and the wave count as the kernels define them, never copied as numbers.
"""
import math
from types import SimpleNamespace as NS

import torch

from small_kernel_refs import (BF16, F32, F64, SENTINEL, assert_bf16_cap, bf16_cap, f32_scalar,  # noqa: F401
                               fp32_tolerance, judge_fp32, row_scale, to_bf16, ulp32)

ROPE_THETA = 1e6
EPS = 1e-6


# ------------------------------------------------------------------------------------------ references
def rope_tables(head_dim, theta, npos):
    """cos / sin [npos][D/2] in fp32, the computation of qwen_tts.kernels.rope_tables (fp32 on the CPU)."""
    inv = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.int64).to(dtype=F32) / head_dim))
    f = torch.arange(npos, dtype=F32)[:, None] * inv[None, :]
    return f.cos().contiguous(), f.sin().contiguous()


def head_rmsnorm(x, w, eps, dtype=F64):
    """x [...][D]: w * (x * rsqrt(mean(x^2) + eps)), eps as the kernel receives it (a C float)."""
    x = x.to(dtype)
    return w.to(dtype) * (x * torch.rsqrt((x * x).mean(-1, keepdim=True) + f32_scalar(eps)))


def rope(x, cos, sin, pos, dtype=F64):
    """x [R][H][D], cos / sin [npos][D/2], pos: R positions -> x * cos + rotate_half(x) * sin."""
    half = x.shape[-1] // 2
    pos = torch.as_tensor(pos, device=x.device).long()
    c, s = cos[pos].to(dtype)[:, None, :], sin[pos].to(dtype)[:, None, :]
    a, b = x[..., :half].to(dtype), x[..., half:].to(dtype)
    return torch.cat([a * c - b * s, b * c + a * s], -1)


def qkv_post_ref(qkv, Hq, Hkv, D, q_norm, k_norm, eps, cos, sin, rope_pos, kv_dtype, dtype=F64):
    """qkv fp32 [R][(Hq + 2 Hkv) * D] -> (q [R][Hq][D] in dtype, k, v [R][Hkv][D] as the cache will hold them: bf16
    caches get the one-step rounding to_bf16, fp32 caches the value in dtype).  q_norm / k_norm None: no norm."""
    R = qkv.shape[0]
    x = qkv.to(dtype).view(R, Hq + 2 * Hkv, D)
    q, k, v = x[:, :Hq], x[:, Hq:Hq + Hkv], x[:, Hq + Hkv:]
    if q_norm is not None:
        q = head_rmsnorm(q, q_norm, eps, dtype)
    if k_norm is not None:
        k = head_rmsnorm(k, k_norm, eps, dtype)
    q, k = rope(q, cos, sin, rope_pos, dtype), rope(k, cos, sin, rope_pos, dtype)
    if kv_dtype == BF16:
        k, v = to_bf16(k), to_bf16(v)
    return q, k, v


def key_range(start, length, window):
    """The keys a row attends to: [max(start, length - window), length); window 0 = none."""
    return (max(start, length - window) if window > 0 else start), length


def attend(q, K, V, keys, dtype=F64, head_map=None):
    """q [Hq][D], K / V [Hkv][L][D] (any float dtype, widened), keys: the key positions (slice or index tensor),
    head_map: the kv head of each q head (default blocked: h // NREP) -> softmax(q.k / sqrt(D)) V, [Hq][D]."""
    Hq, D = q.shape
    Hkv = K.shape[0]
    if head_map is None:
        head_map = [h // (Hq // Hkv) for h in range(Hq)]
    hm = torch.as_tensor(head_map, device=q.device).long()
    k, v = K[:, keys].to(dtype)[hm], V[:, keys].to(dtype)[hm]  # [Hq][n][D]
    s = torch.einsum("hd,hnd->hn", q.to(dtype), k) / math.sqrt(D)
    return torch.einsum("hn,hnd->hd", torch.softmax(s, -1), v)


def attention_ref(q, K, V, start, length, window, dtype=F64):
    lo, hi = key_range(start, length, window)
    return attend(q, K, V, slice(lo, hi), dtype)


def attention_rows(q, Kc, Vc, row_batch, row_start, row_len, window, dtype=F64):
    """qt_attention: q [R][Hq][D], caches [B][Hkv][Lmax][D], per-row batch / start / length (Python ints)."""
    return torch.stack([attention_ref(q[r], Kc[b], Vc[b], s, n, window, dtype)
                        for r, (b, s, n) in enumerate(zip(row_batch, row_start, row_len))])


def append_rows(Kc, Vc, k, v, row_batch, kv_pos):
    """Copies of the caches with the k / v rows written at (row_batch[r], :, kv_pos[r]) in the cache's dtype."""
    Kc, Vc = Kc.clone(), Vc.clone()
    b, p = torch.as_tensor(row_batch, device=Kc.device).long(), torch.as_tensor(kv_pos, device=Kc.device).long()
    Kc[b, :, p], Vc[b, :, p] = k.to(Kc.dtype), v.to(Vc.dtype)
    return Kc, Vc


def cache_rows(Kc, row_batch, kv_pos):
    """The cache rows [R][Hkv][D] at (row_batch[r], :, kv_pos[r])."""
    b, p = torch.as_tensor(row_batch, device=Kc.device).long(), torch.as_tensor(kv_pos, device=Kc.device).long()
    return Kc[b, :, p]


def decode_attention_ref(q, Kc, Vc, row_batch, kv_pos, row_start, window, dtype=F64):
    """qt_decode_attention: the cached keys [start, kv_pos) plus the new key at kv_pos, read from the cache as
    written (Kc / Vc after the append)."""
    return attention_rows(q, Kc, Vc, row_batch, row_start, [p + 1 for p in kv_pos], window, dtype)


def small_prefill_positions(B, T=2):
    """qt_small_prefill_attention: row b * T + t is batch b at position t (rope and cache), causal over the T new keys."""
    rows = [(b, t) for b in range(B) for t in range(T)]
    return [b for b, _ in rows], [t for _, t in rows]


def oproj_ref(x, A, W, round_a, dtype=F64):
    """qt_decode_attn_oproj: x + A @ W^T.  x fp32 [R][N], A [R][Hq * D], W [N][Hq * D] the tiled weight's stored
    values (fp32 or bf16); round_a: A rounded once to bf16 (bf16 weights)."""
    A = to_bf16(A).to(dtype) if round_a else A.to(dtype)
    return x.to(dtype) + A @ W.to(dtype).T


# ------------------------------------------------------------------------------------------ judges
def judge_heads(got, plain32, ref64, margin=2.0):
    """fp32 outputs [R][H][D]: |got - ref64| <= max(margin * e32 * scale, 4 ulp32(scale)) elementwise, scale the
    (row, head)'s largest |ref64|, e32 the largest scaled error of plain torch fp32 over the case.
    -> (ok, kernel's scaled error, e32)."""
    return judge_fp32(got, plain32, ref64, row_scale(ref64), per_row=False, margin=margin)


def bf16_step(x):
    """Spacing of bf16 numbers at magnitude |x|."""
    return ulp32(x) * 65536.0


def oproj_bf16_tolerance(plain32, ref64, A64, W, margin=4.0):
    """x of the fused o_proj with bf16 weights, against ref64 = x + to_bf16(A64) @ W^T: the margin-4 fp32 tolerance from
    the plain fp32 evaluation of that formula (scale: the row's largest |ref64|), plus an allowance for bf16 rounding
    flips of the A operand: ceil(0.001 * K) flips (the bf16 cap's 0.1 % of the K = Hq * D elements of the A row), each
    one bf16 step at the row's largest |A| times the largest |W|.  -> (base tolerance, allowance [R][1], e32)."""
    base, e32 = fp32_tolerance(plain32, ref64, row_scale(ref64), per_row=False, margin=margin)
    flips = math.ceil(0.001 * A64.shape[-1])
    allow = flips * bf16_step(row_scale(A64.to(F64))) * float(W.abs().max())
    return base, allow, e32


def judge_oproj_bf16(got, plain32, ref64, A64, W, margin=4.0):
    """-> (ok, kernel's scaled error, e32, number of elements that needed the allowance)."""
    base, allow, e32 = oproj_bf16_tolerance(plain32, ref64, A64, W, margin)
    err = (got.to(F64) - ref64).abs()
    ek = float((err / row_scale(ref64).clamp_min(2.0 ** -126)).max())
    return bool((err <= base + allow).all()), ek, float(e32), int((err > base).sum())


# ------------------------------------------------------------------------------------------ kernel strides
def attn_rows_block_keys(D):
    """Keys of one block iteration of attn_rows_k: 4 waves x (64 lanes / (D / 8) lanes per key)."""
    return 4 * (64 // (D // 8))


SOFTMAX_STRIDE = 256  # attn_rows_k's softmax loops stride by the block's 256 threads


def decode_waves(Lmax, nrep):
    """attn_decode_k runs 4 waves for Lmax <= 64 (NREP 1 and 2 only), 8 otherwise."""
    return 4 if Lmax <= 64 and nrep < 4 else 8


def decode_gic(D, kv_dtype, waves):
    """Keys one chunk of attn_decode_k covers: waves x lane groups per wave x IC (4 for bf16 caches, 2 for fp32)."""
    return waves * (64 // (D // 8)) * (4 if kv_dtype == BF16 else 2)


def oproj_batch_keys(D, nrep):
    """Cached keys one batch of attn_oproj_k covers per wave: GPW lane groups x IC (2 at NREP >= 4, else 4)."""
    return (64 // (D // 8)) * (2 if nrep >= 4 else 4)


# ------------------------------------------------------------------------------------------ seeded inputs
LAYOUTS = [(128, 16, 8), (128, 16, 4), (64, 16, 16), (64, 8, 2), (16, 4, 2)]  # (D, Hq, Hkv); (64, 16, 16): the codec's
BF16_MIN = 4096  # elements a tensor judged by the bf16 cap must have: one flip is then under its 0.1 %


def _gen(*key):
    return torch.Generator().manual_seed(sum(int(k) * m for k, m in zip(key, (1, 131, 17161, 7, 1000003, 29, 53))))


def _norm_weights(D, norm, g):
    if not norm:
        return None, None, 0.0  # the encoder's call: no norm, eps = 0
    return 1 + 0.1 * torch.randn(D, generator=g), 1 + 0.1 * torch.randn(D, generator=g), EPS


def _fill_rows(n_have, per_row):
    """Rows to add so that a tensor of per_row elements per row reaches BF16_MIN."""
    return max(0, -(-BF16_MIN // per_row) - n_have)


# The bf16 cap asks for at most one bf16 step from the rounded fp64 value.  At an element far smaller than its row's
# scale one bf16 step is smaller than the fp32 tolerance itself, and a kernel that is as exact as fp32 allows can land
# two steps away.  The builders therefore keep every element of a reference that the cap judges at or above 2^-10 of
# its (row, head)'s largest: one step there is at least 2^-18 of that scale, above the margin-4 fp32 tolerance at the
# measured e32 (4 x 5.5e-7 = 2^-18.8).  This is a property of the fp64 reference alone; a head vector of the qkv row
# that breaks it is drawn again.  Rows with a single key return v itself (no arithmetic, hence no such error).
HAZARD = 2.0 ** -10


def _hazard(ref64):
    """[..][H][D] -> [..][H]: the head holds an element below HAZARD of its largest."""
    return (ref64.abs() < HAZARD * row_scale(ref64)).any(-1)


def _settle_k(c, qkv, rope_pos, g):
    """Redraw the k head vectors of qkv (in place) whose reference row holds a hazard."""
    x = qkv.view(qkv.shape[0], c.Hq + 2 * c.Hkv, c.D)
    for _ in range(100):
        idx = _hazard(_qkv(c, qkv, rope_pos, F64)[1]).nonzero()
        if not len(idx):
            return
        x[idx[:, 0], c.Hq + idx[:, 1]] = torch.randn(len(idx), c.D, generator=g)
    raise AssertionError("k rows did not settle")


def _settle_q(c, qkv, rope_pos, r, uses, g):
    """Redraw the q head vectors of qkv row r (in place) until every use (K, V, lo, hi) of it has a hazard-free
    reference output."""
    x = qkv.view(qkv.shape[0], c.Hq + 2 * c.Hkv, c.D)
    uses = [(K[:, lo:hi].to(F64), V[:, lo:hi].to(F64)) for K, V, lo, hi in uses if hi - lo > 1]
    for _ in range(400):
        q = _qkv(c, qkv[r:r + 1], [rope_pos[r]], F64)[0][0]
        hz = torch.zeros(c.Hq, dtype=torch.bool)
        for K, V in uses:
            hz |= _hazard(attend(q, K, V, slice(None)))
        if not hz.any():
            return
        x[r, :c.Hq][hz] = torch.randn(int(hz.sum()), c.D, generator=g)
    raise AssertionError("q rows did not settle")


def _settle_launch(c, L, g, settle_q=True):
    """A launch whose kernel appends the new key itself: hazard-free k rows, then hazard-free outputs."""
    _settle_k(c, L.qkv, L.rope_pos, g)
    if not settle_q:
        return
    _, k, v = _qkv(c, L.qkv, L.rope_pos, F64)
    Kw, Vw = append_rows(L.Kc, L.Vc, k, v, L.row_batch, L.kv_pos)
    for r, (b, s, p) in enumerate(zip(L.row_batch, L.row_start, L.kv_pos)):
        lo, hi = key_range(s, p + 1, L.window)
        _settle_q(c, L.qkv, L.rope_pos, r, [(Kw[b], Vw[b], lo, hi)], g)


# -- a. qt_qkv_post + qt_attention
ATTN_LONG, ATTN_SHORT = 1200, 300  # the two sequences' lengths
ATTN_SLOTS = (2, 0)                # their cache slots of 4 (a non-identity row_batch; slots 1 and 3 stay untouched)
ATTN_ROPE_OFF = (5, 0)             # rope_pos - kv_pos per sequence


def attn_inputs(D, Hq, Hkv, kv_dtype, norm):
    """One qt_qkv_post launch over every position of two sequences (1200 and 300 keys, in cache slots 2 and 0 of 4),
    then three qt_attention launches over chosen rows of its q:
      keys   no window; key counts 1, 2, one block iteration -1 / +0 / +1, 255 / 256 / 257 (start 0 in the short
             sequence, row_start 400 in the long one), and the long sequence's last row (1200 keys)
      w72    window 72, max_keys 72: lengths 72, 73, 300, 1200; a row shorter than the window; row_start later than
             length - window
      w250   window 250, max_keys 250: lengths 250, 251, 1200; shorter; row_start later than length - window
    A row is (sequence, row_start, length); its q row is the sequence's position length - 1."""
    g = _gen(D, Hq, Hkv, kv_dtype == BF16, norm, 1)
    lens = (ATTN_LONG, ATTN_SHORT)
    R = sum(lens)
    qn, kn, eps = _norm_weights(D, norm, g)
    c = NS(D=D, Hq=Hq, Hkv=Hkv, kv_dtype=kv_dtype, norm=norm, R=R, B=4, Lmax=ATTN_LONG + 3, q_norm=qn, k_norm=kn, eps=eps)
    c.qkv = torch.randn(R, (Hq + 2 * Hkv) * D, generator=g)
    c.cos, c.sin = rope_tables(D, ROPE_THETA, ATTN_LONG + 8)
    c.row_batch = [ATTN_SLOTS[s] for s in (0, 1) for _ in range(lens[s])]
    c.kv_pos = [p for s in (0, 1) for p in range(lens[s])]
    c.rope_pos = [p + ATTN_ROPE_OFF[s] for s in (0, 1) for p in range(lens[s])]
    first = (0, ATTN_LONG)  # first qkv row of each sequence
    kb = attn_rows_block_keys(D)
    counts = [1, 2, kb - 1, kb, kb + 1, SOFTMAX_STRIDE - 1, SOFTMAX_STRIDE, SOFTMAX_STRIDE + 1]
    fill = _fill_rows(0, Hq * D)

    def launch(name, window, max_keys, rows):
        rows = rows + [(1, (3 * i) % 11, 12 + (5 * i) % 200 + min(window, 60)) for i in range(max(0, fill - len(rows)))]
        for s, st, n in rows:
            lo, hi = key_range(st, n, window)
            assert 0 <= st < n <= lens[s] and hi - lo <= max_keys
        return NS(name=name, window=window, max_keys=max_keys, q_rows=[first[s] + n - 1 for s, _, n in rows],
                  row_batch=[ATTN_SLOTS[s] for s, _, _ in rows], row_start=[st for _, st, _ in rows],
                  row_len=[n for _, _, n in rows])

    c.launches = [
        launch("keys", 0, ATTN_LONG,
               [(1, 0, n) for n in counts] + [(0, 400, 400 + n) for n in counts] + [(0, 0, ATTN_LONG)]),
        launch("w72", 72, 72, [(1, 0, 72), (1, 0, 73), (1, 0, 300), (0, 0, 72), (0, 0, 73), (0, 0, ATTN_LONG), (1, 0, 40),
                               (1, 250, 300), (0, 1150, ATTN_LONG), (1, 229, 300)]),
        launch("w250", 250, 250, [(1, 0, 250), (1, 0, 251), (0, 0, 250), (0, 0, 251), (0, 0, ATTN_LONG), (1, 0, 100),
                                  (1, 100, 300), (0, 1000, ATTN_LONG), (1, 51, 300)]),
    ]
    if kv_dtype == BF16:  # the bf16 cap judges the k rows and (bf16 output) the attention rows
        _settle_k(c, c.qkv, c.rope_pos, g)
        _, k, v = _qkv(c, c.qkv, c.rope_pos, F64)
        Kw, Vw = append_rows(torch.zeros(c.B, Hkv, c.Lmax, D, dtype=BF16), torch.zeros(c.B, Hkv, c.Lmax, D, dtype=BF16),
                             k, v, c.row_batch, c.kv_pos)
        uses = {}
        for L in c.launches:
            for r, b, s, n in zip(L.q_rows, L.row_batch, L.row_start, L.row_len):
                uses.setdefault(r, []).append((Kw[b], Vw[b]) + key_range(s, n, L.window))
        for r, u in uses.items():
            _settle_q(c, c.qkv, c.rope_pos, r, u, g)
    return c


ATTN_CASES = [(D, Hq, Hkv, kv, True) for D, Hq, Hkv in LAYOUTS for kv in (F32, BF16)] + \
             [(64, 16, 16, F32, False), (64, 16, 16, BF16, False), (128, 16, 8, BF16, False), (16, 4, 2, F32, False)]


# -- b. qt_decode_attention
def decode_inputs(D, Hq, Hkv, kv_dtype, short, norm=True):
    """qt_decode_attention launches over one set of buffers.  short: Lmax = 64 (4 waves at NREP < 4).  Row r reads cache
    slot row_batch[r] (a rotation, one slot unused); the caches hold the sentinel except the keys [start, kv_pos) of
    each row; rope_pos = kv_pos + 3 + r % 2.  Launches (each a list of rows (row_start, kv_pos)):
      keys   no window: n = 1, 2, GIC - 1, GIC, GIC + 1, 2 GIC, 2 GIC + 1, 3 GIC + 5 keys (capped by Lmax), 3 and 8
             (= nsplit), each with row_start 0 and, where the cache has room, row_start 3; row_start = kv_pos
      w5     window 5: rows shorter than, equal to and longer than it, and row_start later than length - window
      w72    window 72 likewise (at Lmax 64 every row is shorter)
    The split-KV launches reuse `keys`."""
    nrep = Hq // Hkv
    Lmax_short = 64
    waves = decode_waves(Lmax_short if short else 65, nrep)
    gic = decode_gic(D, kv_dtype, waves)
    top = 3 * gic + 5
    Lmax = Lmax_short if short else max(top, 200) + 3
    ns = sorted({min(n, Lmax) for n in (1, 2, 3, 8, gic - 1, gic, gic + 1, 2 * gic, 2 * gic + 1, top)})
    keys = [(0, n - 1) for n in ns] + [(3, n + 2) for n in ns if n + 3 <= Lmax] + [(7, 7)]
    lens5 = [3, 5, 6, 40]
    lens72 = [40, 64] if short else [40, 72, 73, 200]
    w5 = [(0, n - 1) for n in lens5] + [(37, 39), (2, 5), (2, 6)]
    w72 = [(0, n - 1) for n in lens72] + ([] if short else [(150, 199), (2, 72), (2, 73)])
    fill = _fill_rows(0, min(Hq, Hkv) * D)
    g = _gen(D, Hq, Hkv, kv_dtype == BF16, short, 2, norm)
    qn, kn, eps = _norm_weights(D, norm, g)
    c = NS(D=D, Hq=Hq, Hkv=Hkv, kv_dtype=kv_dtype, norm=norm, Lmax=Lmax, waves=waves, gic=gic, q_norm=qn, k_norm=kn,
           eps=eps)
    c.cos, c.sin = rope_tables(D, ROPE_THETA, Lmax + 8)
    c.launches = []
    for name, window, rows in (("keys", 0, keys), ("w5", 5, w5), ("w72", 72, w72)):
        rows = rows + [((3 * i) % 5, 4 + (5 * i) % 37) for i in range(max(0, fill - len(rows)))]
        c.launches.append(decode_launch(c, name, window, rows, g))
    return c


def decode_launch(c, name, window, rows, g, identity=False, settle_q=True):
    R = len(rows)
    L = NS(name=name, window=window, R=R, B=R + 1)
    L.row_start, L.kv_pos = [s for s, _ in rows], [p for _, p in rows]
    assert all(0 <= s <= p < c.Lmax for s, p in rows)
    L.row_batch = list(range(R)) if identity else [(r + 2) % (R + 1) for r in range(R)]
    L.rope_pos = list(L.kv_pos) if identity else [p + 3 + r % 2 for r, p in enumerate(L.kv_pos)]
    L.qkv = torch.randn(R, (c.Hq + 2 * c.Hkv) * c.D, generator=g)
    L.Kc = torch.full((L.B, c.Hkv, c.Lmax, c.D), SENTINEL).to(c.kv_dtype)
    L.Vc = L.Kc.clone()
    for r, (s, p) in enumerate(rows):
        if p > s:
            L.Kc[L.row_batch[r], :, s:p] = torch.randn(c.Hkv, p - s, c.D, generator=g).to(c.kv_dtype)
            L.Vc[L.row_batch[r], :, s:p] = torch.randn(c.Hkv, p - s, c.D, generator=g).to(c.kv_dtype)
    _settle_launch(c, L, g, settle_q)
    return L


def decode_const_pos_launch(c):
    """Every row at one position with row_start 0 and the identity row_batch: what const_pos stands for."""
    g = _gen(c.D, c.Hq, c.Hkv, c.kv_dtype == BF16, c.Lmax, 3)
    P = min(c.gic + 1, c.Lmax) - 1
    rows = max(3, _fill_rows(0, min(c.Hq, c.Hkv) * c.D))
    return decode_launch(c, "const_pos", 0, [(0, P)] * rows, g, identity=True), P


DECODE_SPLITS = (2, 3, 8)
DECODE_CASES = [(D, Hq, Hkv, kv, short) for D, Hq, Hkv in LAYOUTS for kv in (F32, BF16) for short in (False, True)
                if not (short and Hq // Hkv >= 4)]  # NREP 4 has no 4-wave form: Lmax 64 would repeat the 8-wave case


# -- c. qt_small_prefill_attention (T = 2)
PREFILL_LAYOUTS = [(128, 16, 8), (16, 4, 2), (64, 4, 4), (128, 16, 4)]
PREFILL_LMAX = 5


def prefill_inputs(D, Hq, Hkv, kv_dtype, norm):
    g = _gen(D, Hq, Hkv, kv_dtype == BF16, norm, 4)
    B = max(5, -(-_fill_rows(0, min(Hq, Hkv) * D) // 2))
    qn, kn, eps = _norm_weights(D, norm, g)
    c = NS(D=D, Hq=Hq, Hkv=Hkv, kv_dtype=kv_dtype, norm=norm, B=B, R=2 * B, Lmax=PREFILL_LMAX, q_norm=qn, k_norm=kn, eps=eps)
    c.qkv = torch.randn(c.R, (Hq + 2 * Hkv) * D, generator=g)
    c.cos, c.sin = rope_tables(D, ROPE_THETA, 8)
    c.row_batch, c.kv_pos = small_prefill_positions(B)
    L = prefill_launch(c)
    _settle_launch(c, L, g)
    return c


PREFILL_CASES = [(D, Hq, Hkv, kv, norm) for D, Hq, Hkv in PREFILL_LAYOUTS for kv in (F32, BF16) for norm in (True, False)]


# -- d. qt_decode_attn_oproj, the (column group, row) form
OPROJ_SHAPES = [(128, 16, 8, 17, 1024, 8), (128, 16, 8, 3, 1024, 16), (128, 8, 4, 40, 200, 3), (16, 8, 2, 9, 32, 5),
                (64, 4, 4, 64, 96, 1), (128, 16, 4, 20, 256, 4), (128, 16, 8, 16, 1024, 8), (128, 16, 8, 1, 1024, 3)]
OPROJ_LMAX = 70  # room for 64 cached keys after a row_start of 3, and the new one


def oproj_supported(D, Hq, Hkv, dt):
    """fp32 weights: the o_proj K slice of one kv head is at most 16 k tiles of 16 (rejected by design beyond)."""
    return dt == BF16 or (Hq // Hkv) * D // 16 <= 16


def oproj_inputs(D, Hq, Hkv, L, N, B, dt):
    """Two launches over one weight.  const: the shape of the parity test (B rows, L - 1 cached keys, const_pos).
    arrays: per-row positions through rope_pos / kv_pos / row_start -- 0 cached keys, one batch of cached keys per
    lane group and one more, 64 cached keys, L - 1, ragged row_start, rope_pos != kv_pos.  Caches and weights share
    the dtype dt (the kernel's contract); row r owns cache slot r.  W has a flat magnitude (0.0375 .. 0.05, random
    signs) so that the bf16 allowance, which is scaled by the largest |W|, stays near what a few real flips cost."""
    nrep = Hq // Hkv
    g = _gen(D, Hq, Hkv, dt == BF16, L, N, B)
    qn, kn, eps = _norm_weights(D, True, g)
    c = NS(D=D, Hq=Hq, Hkv=Hkv, kv_dtype=dt, w_dtype=dt, norm=True, N=N, Lmax=OPROJ_LMAX, q_norm=qn, k_norm=kn, eps=eps)
    c.cos, c.sin = rope_tables(D, ROPE_THETA, OPROJ_LMAX + 8)
    sign = torch.where(torch.rand(N, Hq * D, generator=g) < 0.5, -1.0, 1.0)
    c.W = (0.05 * sign * (0.75 + 0.25 * torch.rand(N, Hq * D, generator=g))).to(dt)
    bk = oproj_batch_keys(D, nrep)
    ncs = [0, bk, bk + 1, 64, L - 1, 1, 2]
    arr = [(0, n) for n in ncs] + [(2, 2 + bk), (5, 5), (3, 3 + max(L - 1, 1))]
    fill = _fill_rows(0, min(Hq, Hkv) * D) if dt == BF16 else 0
    arr = arr + [((3 * i) % 5, 5 + (5 * i) % 23) for i in range(max(0, fill - len(arr)))]
    cst = [(0, L - 1)] * max(B, fill)

    def launch(name, rows, const):
        Lc = decode_launch(c, name, 0, rows, g, identity=True, settle_q=False)
        Lc.B = Lc.R  # row r = batch entry r: no spare slot
        Lc.Kc, Lc.Vc = Lc.Kc[:Lc.R].clone(), Lc.Vc[:Lc.R].clone()
        Lc.const_pos = rows[0][1] if const else -1
        if not const:
            Lc.rope_pos = [p + 1 + r % 3 for r, p in enumerate(Lc.kv_pos)]
        _settle_k(c, Lc.qkv, Lc.rope_pos, g)
        Lc.x = torch.randn(Lc.R, N, generator=g)
        return Lc

    c.launches = [launch("const", cst, True), launch("arrays", arr, False)]
    return c


OPROJ_CASES = [s + (dt,) for s in OPROJ_SHAPES for dt in (F32, BF16) if oproj_supported(s[0], s[1], s[2], dt)]


def to_device(c, dev):
    """The case with every tensor (its launches' too) on dev."""
    out = NS(**vars(c))
    for k, v in vars(c).items():
        if torch.is_tensor(v):
            setattr(out, k, v.to(dev))
        elif k == "launches":
            out.launches = [to_device(L, dev) for L in v]
    return out


# ------------------------------------------------------------------------------------------ judging a launch
# Every judge_* below takes what a launch left behind (caches, q, outputs) and returns records
# (what, kind, ok, a, b): kind "fp32": a = the kernel's scaled error, b = plain torch fp32's; "bf16": a = the worst
# distance in bf16 steps, b = the fraction of equal elements; "exact": a = b = 0.  The GPU tests pass the kernels'
# results, tests/test_attention_refs.py passes plain torch fp32 (which must pass) and mutants (which must not).
MARGIN_ROWS, MARGIN_EXP2 = 2.0, 4.0  # see tests/test_gpu_attention_fp64.py for where the two margins come from


def _rec_fp32(what, got, plain32, ref64, margin):
    ok, ek, et = judge_heads(got, plain32, ref64, margin)
    return (what, "fp32", ok, ek, et)


def _rec_bf16(what, got, ref64):
    assert got.numel() >= BF16_MIN, (what, got.numel())
    worst, same = bf16_cap(got.contiguous(), ref64)
    return (what, "bf16", worst <= 1 and same >= 0.999, worst, same)


def _rec_exact(what, ok):
    return (what, "exact", bool(ok), 0, 0)


def _memo(memo, key, fn):
    """fn() once per memo: the CPU tests judge several outputs against one launch's references."""
    if memo is None:
        return fn()
    if key not in memo:
        memo[key] = fn()
    return memo[key]


def _qkv(c, qkv, rope_pos, dtype):
    """(q, unrounded k, v) of the case in dtype (the bf16 cap rounds its reference itself)."""
    return qkv_post_ref(qkv, c.Hq, c.Hkv, c.D, c.q_norm, c.k_norm, c.eps, c.cos, c.sin, rope_pos, F32, dtype)


def judge_appended(c, qkv, rope_pos, row_batch, kv_pos, K0, V0, Kw, Vw, margin):
    """The k / v rows a launch wrote at (row_batch[r], :, kv_pos[r]) into caches that were K0 / V0 before: bf16 caches
    by the bf16 cap, fp32 caches by the fp32 judge (v: the qkv row unchanged); every other cache element as before."""
    _, k64, v64 = _qkv(c, qkv, rope_pos, F64)
    gk, gv = cache_rows(Kw, row_batch, kv_pos), cache_rows(Vw, row_batch, kv_pos)
    if c.kv_dtype == BF16:
        recs = [_rec_bf16("k rows", gk, k64), _rec_bf16("v rows", gv, v64)]
    else:
        _, k32, _ = _qkv(c, qkv, rope_pos, F32)
        recs = [_rec_fp32("k rows", gk, k32, k64, margin), _rec_exact("v rows", torch.equal(gv.to(F64), v64))]
    K1, V1 = append_rows(K0, V0, gk, gv, row_batch, kv_pos)
    return recs + [_rec_exact("cache elsewhere", torch.equal(K1, Kw) and torch.equal(V1, Vw))]


def _rec_out(what, out, plain32, ref64, margin):
    if out.dtype == BF16:
        return _rec_bf16(what, out.view(ref64.shape), ref64)
    return _rec_fp32(what, out.view(ref64.shape), plain32, ref64, margin)


def judge_qkv_post(c, K0, V0, q, Kw, Vw):
    """a, stage 1: q [R][Hq * D] fp32 against fp64, the appended rows."""
    q64, q32 = _qkv(c, c.qkv, c.rope_pos, F64)[0], _qkv(c, c.qkv, c.rope_pos, F32)[0]
    return [_rec_fp32("q", q.view(q64.shape), q32, q64, MARGIN_ROWS)] + \
        judge_appended(c, c.qkv, c.rope_pos, c.row_batch, c.kv_pos, K0, V0, Kw, Vw, MARGIN_ROWS)


def judge_attention(c, L, q, Kw, Vw, out, memo=None):
    """a, stage 2: out [R_L][Hq * D] against the attention of the q rows and the caches the kernels produced."""
    qs = q.view(-1, c.Hq, c.D)[torch.as_tensor(L.q_rows, device=q.device)]
    a = (qs, Kw, Vw, L.row_batch, L.row_start, L.row_len, L.window)
    plain, ref = _memo(memo, "out", lambda: (attention_rows(*a, F32), attention_rows(*a, F64)))
    return [_rec_out("out", out, plain, ref, MARGIN_ROWS)]


def judge_decode(c, L, Kw, Vw, out, margin=MARGIN_EXP2, memo=None):
    """b (and c, d): the appended rows, and out [R][Hq * D] against the attention of the reference q (the kernel keeps
    its q to itself) over the caches as written."""
    recs = judge_appended(c, L.qkv, L.rope_pos, L.row_batch, L.kv_pos, L.Kc, L.Vc, Kw, Vw, margin)
    if out is None:
        return recs
    a = (Kw, Vw, L.row_batch, L.kv_pos, L.row_start, L.window)
    plain, ref = _memo(memo, "out", lambda: (decode_attention_ref(_qkv(c, L.qkv, L.rope_pos, F32)[0], *a, F32),
                                             decode_attention_ref(_qkv(c, L.qkv, L.rope_pos, F64)[0], *a, F64)))
    return recs + [_rec_out("out", out, plain, ref, margin)]


def prefill_launch(c):
    """The small prefill as a decode-style launch: both positions of every batch entry appended, sentinel caches."""
    K0 = torch.full((c.B, c.Hkv, c.Lmax, c.D), SENTINEL, device=c.qkv.device).to(c.kv_dtype)
    return NS(name="prefill", window=0, R=c.R, B=c.B, qkv=c.qkv, rope_pos=c.kv_pos, row_batch=c.row_batch, kv_pos=c.kv_pos,
              row_start=[0] * c.R, Kc=K0, Vc=K0.clone())


def judge_prefill(c, L, Kw, Vw, out, memo=None):
    return judge_decode(c, L, Kw, Vw, out, margin=MARGIN_ROWS, memo=memo)


def judge_oproj(c, L, Kw, Vw, x, memo=None):
    """d: the appended rows, and x [R][N] against x0 + A @ W^T with A the fp64 attention over the caches as written
    (bf16 weights: A rounded once to bf16, and the flip allowance of oproj_bf16_tolerance)."""
    recs = judge_appended(c, L.qkv, L.rope_pos, L.row_batch, L.kv_pos, L.Kc, L.Vc, Kw, Vw, MARGIN_EXP2)
    a = (Kw, Vw, L.row_batch, L.kv_pos, L.row_start, 0)
    A64 = _memo(memo, "A64", lambda: decode_attention_ref(_qkv(c, L.qkv, L.rope_pos, F64)[0], *a, F64).flatten(1))
    if c.w_dtype == BF16:
        ref, plain = oproj_ref(L.x, A64, c.W, True), oproj_ref(L.x, A64, c.W, True, F32)
        ok, ek, et, n_allow = judge_oproj_bf16(x, plain, ref, A64, c.W, MARGIN_EXP2)
        return recs + [(f"x ({n_allow} of {x.numel()} needed the flip allowance)", "fp32", ok, ek, et)]
    A32 = _memo(memo, "A32", lambda: decode_attention_ref(_qkv(c, L.qkv, L.rope_pos, F32)[0], *a, F32).flatten(1))
    ref, plain = oproj_ref(L.x, A64, c.W, False), oproj_ref(L.x, A32, c.W, False, F32)
    ok, ek, et = judge_fp32(x, plain, ref, row_scale(ref), per_row=False, margin=MARGIN_EXP2)
    return recs + [("x", "fp32", ok, ek, et)]


def format_records(kernel, case, recs):
    """The lines of profiles/attention_fp64_errors.txt."""
    lines = []
    for what, kind, ok, a, b in recs:
        head, verdict = f"fp64pin | {kernel} | {case} | {what}", "ok" if ok else "FAIL"
        if kind == "fp32":
            ratio = f"{a / b:5.2f}" if b > 0 else "  (floor)"
            lines.append(f"{head} | kernel {a:.3g} | torch-fp32 {b:.3g} | ratio {ratio} | {verdict}")
        elif kind == "bf16":
            lines.append(f"{head} | bf16 worst {a} step | equal {100 * b:.4f} % | {verdict}")
        elif not ok:
            lines.append(f"{head} | FAIL")
    return lines
