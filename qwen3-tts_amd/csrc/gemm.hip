// Weight-tiled MFMA GEMM for gfx950: every Linear / Conv1d of the hot path.
//
//   out[m][n] (op)= epi( rs[m] * sum_k W[n][k] * (gamma[k] * A[m][k]) + bias[n] ) * colscale[n]
//
// * Weights are pre-tiled once at load time (qt_tile_weight) into MFMA B-fragment order:
//   tile (nt, kt) = 16 output rows x KT k-columns = 1 KiB, lane l holds W[nt*16 + (l&15)][kt*KT + (l>>4)*E .. +E)
//   (E = 8 bf16 / 4 fp32, KT = 4E).  A wave streaming one n-tile along K reads 1 KiB contiguous per
//   instruction: fully coalesced HBM traffic, no cross-lane reduction (MFMA does the k-sum).
// * A (activations, fp32 or bf16) is read straight from global/L2 in the matching A-fragment order.
//   Optional prologues: RMSNorm (gamma + per-row rsqrt from the same loads), row gather (embedding
//   lookup), implicit im2col for causal / transposed Conv1d on channels-last [batch][time][cin].
// * K is split across the block's waves; partial 16x16 tiles are reduced through LDS, then the fused
//   epilogue (bias, SiLU/GELU, LayerScale, residual add, SwiGLU pairing) writes the output.
// Decode (M <= 16) is HBM-bound on W: roofline = W bytes / 8 TB/s.
#include "gemm_p.h"
#include <algorithm>
#include <type_traits>
#include <cstdlib>

namespace {

using qt_gemm_impl::GemmP;
using qt_gemm_impl::GemmPlan;
using qt_gemm_impl::GemmRoute;
using qt_gemm_impl::GemmKnobs;
using qt_gemm_impl::gemm_plan;

// SnakeBeta exactly as qt_snake computes it (fp32 math on the stored activation)
QT_DEV float snake1(float v, float al, float ib) {
  const float s = sinf(v * al);
  return v + ib * (s * s);
}

// Load the E-element A fragment of row m at padded k index kk (fp32 out), zero outside.
template <typename AT, int E>
QT_DEV void load_a(const GemmP& p, int m, int kk, float* v) {
#pragma unroll
  for (int i = 0; i < E; ++i) v[i] = 0.f;
  if (m >= p.M) return;
  const AT* A = (const AT*)p.A;
  const AT* src;
  if (p.taps > 0) {  // implicit im2col, channels-last input [batch][t_in][cin]
    int j = kk / p.cin_pad, c = kk - j * p.cin_pad;
    if (c >= p.cin) return;
    int b = m / p.t_out, t = m - b * p.t_out;
    int ti = t + p.t_off + j * p.dil;
    if (ti < 0 || ti >= p.t_in) return;
    src = A + ((long long)b * p.t_in + ti) * p.lda + c;
  } else {
    if (kk >= p.Klog) return;
    long long row = p.a_index ? (long long)p.a_index[m] : (long long)m;
    src = A + row * p.lda + kk;
  }
  if constexpr (E == 8) load8f(src, v); else load4f(src, v);
  if (p.a_elu) {
#pragma unroll
    for (int i = 0; i < E; ++i) v[i] = elu_f(v[i]);
  }
  if (p.sn_a) {
    const int c0 = p.taps > 0 ? (kk % p.cin_pad) : kk;
#pragma unroll
    for (int i = 0; i < E; ++i) v[i] = snake1(v[i], p.sn_a[c0 + i], p.sn_ib[c0 + i]);
  }
}

template <typename WT, typename AT, typename OT, int MT, int WPB>
__global__ __launch_bounds__(WPB * 64) void gemm_wt(GemmP p) {
  constexpr bool BF = sizeof(WT) == 2;
  constexpr int E = BF ? 8 : 4;
  constexpr int KT = 4 * E;
  __shared__ float red[WPB][MT][64][4];
  __shared__ float red_ss[WPB][MT][16];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int lm = lane & 15, lk = lane >> 4;
  const int nt = blockIdx.x;
  const int m0 = blockIdx.y * 16 * MT;
  const int ktiles = p.Kp / KT;
  const int per = (ktiles + WPB - 1) / WPB;
  const int kt0 = w * per, kt1 = min(ktiles, kt0 + per);
  const bool norm = p.rms != 0;
  const bool hasg = p.gamma != nullptr;

  f32x4_t acc[MT];
  float ss[MT];
#pragma unroll
  for (int i = 0; i < MT; ++i) { acc[i] = f32x4_t{0.f, 0.f, 0.f, 0.f}; ss[i] = 0.f; }

  const WT* wp = (const WT*)p.W + ((size_t)nt * ktiles) * 64 * E + lane * E;
  for (int kt = kt0; kt < kt1; ++kt) {
    u32x4_t wv = *(const u32x4_t*)(wp + (size_t)kt * 64 * E);
    const int kk = kt * KT + lk * E;
    float g[E];
    if (hasg) {
#pragma unroll
      for (int i = 0; i < E; ++i) g[i] = (kk + i < p.Klog) ? p.gamma[kk + i] : 0.f;
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      float a[E];
      load_a<AT, E>(p, m0 + mt * 16 + lm, kk, a);
      if (norm) {
#pragma unroll
        for (int i = 0; i < E; ++i) ss[mt] += a[i] * a[i];
      }
      if (hasg) {
#pragma unroll
        for (int i = 0; i < E; ++i) a[i] *= g[i];
      }
      if constexpr (BF) {
        u32x4_t av = {pack2bf(a[0], a[1]), pack2bf(a[2], a[3]), pack2bf(a[4], a[5]), pack2bf(a[6], a[7])};
        acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, av),
                                                          __builtin_bit_cast(bf16x8_t, wv), acc[mt], 0, 0, 0);
      } else {
        f32x4_t wf = __builtin_bit_cast(f32x4_t, wv);
#pragma unroll
        for (int s = 0; s < 4; ++s)
          acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], wf[s], acc[mt], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    red[w][mt][lane][0] = acc[mt][0]; red[w][mt][lane][1] = acc[mt][1];
    red[w][mt][lane][2] = acc[mt][2]; red[w][mt][lane][3] = acc[mt][3];
    if (norm) {
      float s = ss[mt];
      s += __shfl_xor(s, 16, 64);
      s += __shfl_xor(s, 32, 64);
      if (lk == 0) red_ss[w][mt][lm] = s;
    }
  }
  __syncthreads();
  if (threadIdx.x >= MT * 64) return;
  const int mt = threadIdx.x >> 6;  // == w: the epilogue thread block keeps wave boundaries
  float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ww = 0; ww < WPB; ++ww) {
    v[0] += red[ww][mt][lane][0]; v[1] += red[ww][mt][lane][1];
    v[2] += red[ww][mt][lane][2]; v[3] += red[ww][mt][lane][3];
  }
  const int n = nt * 16 + lm;
  const bool nval = n < p.N;
  const float bias = (p.bias && nval) ? p.bias[n] : 0.f;
  const float cs = (p.colscale && nval) ? p.colscale[n] : 1.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int rloc = lk * 4 + i;
    float x = v[i];
    if (norm) {
      float s = 0.f;
#pragma unroll
      for (int ww = 0; ww < WPB; ++ww) s += red_ss[ww][mt][rloc];
      x *= rsqrtf(s / (float)p.Klog + p.eps);
    }
    x += bias;
    x = act_f(x, p.act);
    x *= cs;
    v[i] = x;
  }
  OT* out = (OT*)p.out;
  if (p.epi == QT_EPI_SWIGLU) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float up = __shfl_xor(v[i], 8, 64);
      const int m = m0 + mt * 16 + lk * 4 + i;
      if (lm < 8 && m < p.M && nt * 8 + lm < (p.N >> 1))
        out[(long long)m * p.ldo + nt * 8 + lm] = from_f<OT>(silu_f(v[i]) * up);
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + mt * 16 + lk * 4 + i;
    if (m >= p.M || !nval) continue;
    OT* o = out + (long long)m * p.ldo + n;
    const float r = p.epi == QT_EPI_ADD ? to_f(*o) + v[i] : v[i];
    *o = from_f<OT>(r);
    if (p.out2) p.out2[(long long)m * p.ldo2 + n] = f2bf(r);
  }
}

// Decode GEMV (M <= 16, plain or gathered rows, K % KT == 0): one wave owns a 16-row n-tile over a K
// slice.  Branch-free inner loop: the lane's A row pointer is hoisted, tail tiles are clamped and zeroed
// by select, so every chunk issues its U weight fragments (1 KiB contiguous per wave-instruction), A
// fragments and gamma before a single wait -- the block keeps all of its weight bytes in flight.
// Split-K partials reduce through LDS; the epilogue is shared with gemm_wt.
// Fold F (bf16 weights, rows per block <= 16 / F): the MFMA rows past the block's rows are zero, so the lanes
// feeding them fetch the block's rows of the next F - 1 k tiles instead of re-fetching a clamped row, and DPP row
// rotations (row_ror 16/F * t) hand those fragments to the live lanes for the t-th MFMA: 1/F of the activation
// requests, the same MFMA operands.  Row groups (gridDim.z): block z owns rows [z * p.mr, z * p.mr + p.mr) -- a
// few-column-tile GEMV gets more blocks without a cross-block split-K reduction (its weight tiles are re-read
// from L2 by the z blocks; blockIdx.x-major launch keeps a tile's row blocks ntiles apart, same XCD when
// ntiles % 8 == 0).
// Loads hipcc does not track (see gemv_wt's epilogue prefetch): the destination is only read after an
// asm_wait that names it "+v", so the compiler never reads it before the data has landed.
QT_DEV unsigned asm_load_b32(const void* ptr) {
  unsigned v;
  asm volatile("global_load_dword %0, %1, off" : "=v"(v) : "v"(ptr) : "memory");
  return v;
}
QT_DEV unsigned asm_load_raw(const float* ptr) { return asm_load_b32(ptr); }
QT_DEV unsigned asm_load_raw(const bf16_t* ptr) {
  unsigned v;
  asm volatile("global_load_ushort %0, %1, off" : "=v"(v) : "v"(ptr) : "memory");
  return v;
}
template <typename T> QT_DEV float raw_to_f(unsigned u);
template <> QT_DEV float raw_to_f<float>(unsigned u) { return __uint_as_float(u); }
template <> QT_DEV float raw_to_f<bf16_t>(unsigned u) { return __uint_as_float(u << 16); }

// DPP row_ror:S on each dword of a 16-byte fragment (rotate right: lane l of a 16-lane row receives lane
// (l - S) mod 16)
template <int S>
QT_DEV u32x4_t ror4(u32x4_t x) {
  u32x4_t r;
#pragma unroll
  for (int e = 0; e < 4; ++e) r[e] = (unsigned)__builtin_amdgcn_update_dpp(0, (int)x[e], 0x120 + S, 0xF, 0xF, false);
  return r;
}

template <typename WT, typename AT, typename OT, int WPB, int U, bool NORM, bool NTL, int F>
__global__ __launch_bounds__(WPB * 64) void gemv_wt(GemmP p) {
  constexpr bool BF = sizeof(WT) == 2;
  constexpr int E = BF ? 8 : 4;
  constexpr int KT = 4 * E;
  constexpr int RPF = 16 / F;  // MFMA rows fed by real rows
  static_assert(F == 1 || (BF && U % F == 0), "fold: bf16 weights, U multiple of F");
  __shared__ float red[WPB][64][4];
  __shared__ float red_ss[WPB][16];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int lm = lane & 15, lk = lane >> 4;
  const int nt = blockIdx.x, sp = blockIdx.y;
  const int m0 = blockIdx.z * p.mr;           // first row of this row group
  const int mr = min(p.mr, p.M - m0);         // rows of this block
  const int ktiles = p.Kp / KT;
  const int kps = (ktiles + p.ks - 1) / p.ks;  // k tiles of this split
  const int ks0 = sp * kps, ks1 = min(ktiles, ks0 + kps);
  const int per = (kps + WPB - 1) / WPB;
  const int kt0 = ks0 + w * per, kt1 = min(ks1, kt0 + per);
  const int arow_i = lm % RPF;  // the block row this lane fetches
  const int hsel = lm / RPF;    // which k tile of the fold group it fetches
  const bool rowok = arow_i < mr;
  const int mrow = m0 + (rowok ? arow_i : mr - 1);
  // gathered row (a_index): an untracked load waited for here, so no compiler-visible load is pending at the chunk
  // loop's preheader (hipcc flushes those with a vmcnt(0) that would also wait for the epilogue prefetch)
  unsigned grow = (unsigned)mrow;
  if (p.a_index) {
    grow = asm_load_b32(p.a_index + mrow);
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(grow)::"memory");
  }
  const AT* arow = (const AT*)p.A + (long long)(int)grow * p.lda + lk * E;
  f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
  float ssv[E];
#pragma unroll
  for (int i = 0; i < E; ++i) ssv[i] = 0.f;
  // epilogue operands of wave 0 issued before the weight stream (hides one dependent round trip).  Inline-asm loads
  // (waited for by asm_wait_epi below): hipcc would otherwise flush them with a vmcnt(0) at the chunk loop's
  // preheader, i.e. wait a full round trip before issuing the first weight fragment.
  const int n = nt * 16 + lm;
  const bool nval = n < p.N;
  const int nc = min(n, p.N - 1);  // clamped column: every lane loads, no per-load branch
  unsigned pre_bias = 0u, pre_cs = 0u, pre_out[4] = {0u, 0u, 0u, 0u};
  const bool pre = w == 0;
  if (pre) {
    if (p.bias) pre_bias = asm_load_b32(p.bias + nc);
    if (p.colscale) pre_cs = asm_load_b32(p.colscale + nc);
    if (p.epi == QT_EPI_ADD) {
      const OT* ob = (const OT*)p.out + nc;
#pragma unroll
      for (int i = 0; i < 4; ++i) pre_out[i] = asm_load_raw(ob + (long long)(m0 + min(lk * 4 + i, mr - 1)) * p.ldo);
    }
  }
  const WT* wp = (const WT*)p.W + ((size_t)nt * ktiles) * 64 * E + lane * E;
  constexpr int NA = U / F;  // A fragments per chunk
  for (int c = kt0; c < kt1; c += U) {
    u32x4_t wv[U];
    float a[NA][E];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int kc = min(c + u, kt1 - 1);
      if constexpr (NTL)  // streamed-once weights: non-temporal, so they do not evict re-read data from L2 / MALL
        wv[u] = __builtin_nontemporal_load((const u32x4_t*)(wp + (size_t)kc * 64 * E));
      else
        wv[u] = *(const u32x4_t*)(wp + (size_t)kc * 64 * E);
    }
#pragma unroll
    for (int q = 0; q < NA; ++q) {
      // every lane loads (with F == 1, rows >= M re-fetch row M-1 from L2: predicating the load on the row was
      // measured slower, profiles/r01_gemv_variants_ab.jsonl)
      // (no runtime branch around these loads: hipcc then waits vmcnt(0) after each one, serialising the chunk's
      // round trips -- tools/gemv_probe.hip)
      const int kc = min(c + F * q + hsel, kt1 - 1);
      if constexpr (E == 8) load8f(arow + kc * KT, a[q]); else load4f(arow + kc * KT, a[q]);
    }
#pragma unroll
    for (int q = 0; q < NA; ++q) {
      const bool ok = rowok && (c + F * q + hsel < kt1);
#pragma unroll
      for (int i = 0; i < E; ++i) {
        float x = ok ? a[q][i] : 0.f;
        if constexpr (NORM) ssv[i] += x * x;  // E independent chains (not one 4*U*E-long chain)
        a[q][i] = x;
      }
      if constexpr (F > 1) {
        const u32x4_t own = {pack2bf(a[q][0], a[q][1]), pack2bf(a[q][2], a[q][3]), pack2bf(a[q][4], a[q][5]),
                             pack2bf(a[q][6], a[q][7])};
        const u32x4_t zero = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int t = 0; t < F; ++t) {
          // row_ror:(16 - RPF*t) -- lane r receives lane r + RPF*t: the fold group's t-th k tile
          u32x4_t av = own;
          if constexpr (F >= 2) if (t == 1) av = ror4<16 - RPF>(own);
          if constexpr (F >= 4) if (t == 2) av = ror4<16 - 2 * RPF>(own);
          if constexpr (F >= 4) if (t == 3) av = ror4<16 - 3 * RPF>(own);
          av = hsel ? zero : av;
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, av),
                                                        __builtin_bit_cast(bf16x8_t, wv[F * q + t]), acc, 0, 0, 0);
        }
      } else if constexpr (BF) {
        u32x4_t av = {pack2bf(a[q][0], a[q][1]), pack2bf(a[q][2], a[q][3]), pack2bf(a[q][4], a[q][5]),
                      pack2bf(a[q][6], a[q][7])};
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, av),
                                                      __builtin_bit_cast(bf16x8_t, wv[q]), acc, 0, 0, 0);
      } else {
        f32x4_t wf = __builtin_bit_cast(f32x4_t, wv[q]);
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[q][s], wf[s], acc, 0, 0, 0);
      }
    }
  }
  red[w][lane][0] = acc[0]; red[w][lane][1] = acc[1]; red[w][lane][2] = acc[2]; red[w][lane][3] = acc[3];
  if (NORM) {
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < E; ++i) ss += ssv[i];
    // + the lanes holding the same row's other k tiles of the fold group
    if constexpr (F == 4) ss += dpp_f<0x124>(ss);
    if constexpr (F >= 2) ss += dpp_f<0x128>(ss);
    ss += __shfl_xor(ss, 16, 64);
    ss += __shfl_xor(ss, 32, 64);
    if (lk == 0) red_ss[w][lm] = lm >= RPF ? 0.f : ss;
  }
  __syncthreads();
  if (threadIdx.x >= 64) return;
  // the epilogue prefetch has landed (it was issued before every weight load the loop waited for)
  asm volatile("s_waitcnt vmcnt(0)" : "+v"(pre_bias), "+v"(pre_cs), "+v"(pre_out[0]), "+v"(pre_out[1]), "+v"(pre_out[2]),
               "+v"(pre_out[3])::"memory");
  float v[4] = {0.f, 0.f, 0.f, 0.f}, ssr[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ww = 0; ww < WPB; ++ww) {
    v[0] += red[ww][lane][0]; v[1] += red[ww][lane][1]; v[2] += red[ww][lane][2]; v[3] += red[ww][lane][3];
  }
  if (NORM) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int ww = 0; ww < WPB; ++ww) ssr[i] += red_ss[ww][lk * 4 + i];
  }
  if (p.ks > 1) {
    // deterministic split-K: every split stores its partial, the last to arrive sums them in split order.
    // Agent-scope relaxed atomics (sc1: coherent across the 8 XCD L2s) + an explicit vmcnt drain instead of
    // __threadfence(), whose release half is an XCD-wide L2 writeback (buffer_wbl2) costing ~0.4 us per block.
    constexpr int PS = 64 * 4 + 16;
    float* mine = p.part + ((size_t)nt * p.ks + sp) * PS;
#pragma unroll
    for (int i = 0; i < 4; ++i) __hip_atomic_store(mine + lane * 4 + i, v[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (NORM && lm == 0) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        __hip_atomic_store(mine + 256 + lk * 4 + i, ssr[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __builtin_amdgcn_s_waitcnt(0);  // partial stores acknowledged before the arrival is counted
    unsigned old = 0;
    if (lane == 0) old = __hip_atomic_fetch_add(p.cnt + nt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    old = __shfl(old, 0, 64);
    if (old != (unsigned)p.ks - 1) return;
    if (lane == 0) __hip_atomic_store(p.cnt + nt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // re-arm
    const float* base = p.part + (size_t)nt * p.ks * PS;
#pragma unroll
    for (int i = 0; i < 4; ++i) { v[i] = 0.f; ssr[i] = 0.f; }
    // four splits' partials in flight before their adds (a dependent add per split would serialise the round trips)
    for (int s0 = 0; s0 < p.ks; s0 += 4) {
      float pv[4][4], ps[4][4];
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int sc = min(s0 + s, p.ks - 1);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          pv[s][i] = __hip_atomic_load(base + sc * PS + lane * 4 + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          ps[s][i] = NORM ? __hip_atomic_load(base + sc * PS + 256 + lk * 4 + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.f;
        }
      }
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        if (s0 + s < p.ks) {
#pragma unroll
          for (int i = 0; i < 4; ++i) { v[i] += pv[s][i]; ssr[i] += ps[s][i]; }
        }
      }
    }
  }
  const float bias = (p.bias && nval) ? __uint_as_float(pre_bias) : 0.f;
  const float cs = (p.colscale && nval) ? __uint_as_float(pre_cs) : 1.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float x = v[i];
    if (NORM) x *= rsqrtf(ssr[i] / (float)p.Klog + p.eps);
    x += bias;
    x = act_f(x, p.act);
    v[i] = x * cs;
  }
  OT* out = (OT*)p.out;
  if (p.epi == QT_EPI_SWIGLU) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float up = __shfl_xor(v[i], 8, 64);
      const int m = lk * 4 + i;
      if (lm < 8 && m < mr && nt * 8 + lm < (p.N >> 1))
        out[(long long)(m0 + m) * p.ldo + nt * 8 + lm] = from_f<OT>(silu_f(v[i]) * up);
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = lk * 4 + i;
    if (m >= mr || !nval) continue;
    OT* o = out + (long long)(m0 + m) * p.ldo + n;
    const float r = p.epi == QT_EPI_ADD ? raw_to_f<OT>(pre_out[i]) + v[i] : v[i];
    *o = from_f<OT>(r);
    if (p.out2) p.out2[(long long)(m0 + m) * p.ldo2 + n] = f2bf(r);
  }
}

// LDS-tiled implicit GEMM for large M with bf16 weights (codec convs / transposed convs as taps, prefill
// linears as taps = 1).  Block = 128 output rows x NT*16 columns (NT = 6 or 8), 4 waves; wave w owns rows
// [32w, 32w+32) x all the block's columns = 2 x NT MFMA 16x16x32 tiles.  A tile's rows are one batch item's consecutive time steps, so the
// input window [t0 + t_off, t0 + t_off + 127 + (taps-1)*dil] x 32 channels is staged into LDS once per channel
// chunk (optional SnakeBeta applied while staging, rounded to bf16 like the MFMA operand) and every tap reads
// its shifted rows from it: the im2col expansion (taps x) never leaves the CU.  The next chunk is loaded into
// registers while the current one is multiplied (double-buffered window, one barrier per chunk).  Weights
// are the pre-tiled MFMA B fragments (1 KiB per 16 x 32 tile), read through L1/L2 one tap ahead.
// Row sums of squares (RMSNorm, taps == 1 only) accumulate from the fp32 A values during staging.
// out-of-line activation for the implicit-GEMM epilogue: inlined, the erf / exp bodies make the epilogue too large
// to unroll and the accumulators then go through scratch memory
__attribute__((noinline)) QT_DEV float act_f_call(float x, int act) { return act_f(x, act); }

constexpr int IG_BM = 128, IG_BN = 64, IG_KC = 32, IG_LDSW = 40;  // LDS row stride 40 bf16 (80 B)
constexpr int IG_GPT = 3;  // staged 8-channel groups per thread (window rows <= 192)
#ifndef IG_PD
#define IG_PD 1  // B-fragment prefetch distance in k tiles (2-4 measured slower: codec 41.0 / 34.1 / 38.2 vs 31.0 ms)
#endif

// 2 x 2 wave grid: wave (w >> 1, w & 1) owns BM/2 rows x NT/2 column tiles, so each B fragment is fetched by
// 2 waves instead of 4 (a 4 x 1 layout is L1/TA-bound on the shared B fragments: 4 x NT KiB per k tile per block).
template <typename AT, typename OT, int NT, int MI>
__global__ __launch_bounds__(256) void igemm_k(GemmP p) {
  constexpr int BM = 64 * MI;  // output rows per block
  constexpr int RT = BM / 32;  // 16-row MFMA tiles per wave
  constexpr int CT = NT / 2;   // 16-column tiles per wave
  static_assert(NT % 2 == 0, "2 x 2 wave grid needs an even column tile count");
  extern __shared__ unsigned char ig_smem[];
  bf16_t* win = (bf16_t*)ig_smem;  // [2][WR][IG_LDSW]
  __shared__ float ss_row[BM];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int lm = lane & 15, lk = lane >> 4;
  const bool lin = p.taps == 0;
  const int taps = lin ? 1 : p.taps, dil = lin ? 1 : p.dil;
  const int cin = lin ? p.Klog : p.cin, cin_pad = lin ? p.Kp : p.cin_pad;
  const int t_in = lin ? p.M : p.t_in, t_out = lin ? p.M : p.t_out, t_off = lin ? 0 : p.t_off;
  const int WR = BM + (taps - 1) * dil;
  const int tiles_t = (t_out + BM - 1) / BM;
  const int bi = blockIdx.x / tiles_t, t0 = (blockIdx.x - bi * tiles_t) * BM;
  const int ntl = (p.N + 15) / 16, nt0 = blockIdx.y * NT + (w & 1) * CT;
  const int wrow = (w >> 1) * (BM / 2);  // first output row of this wave in the tile
  const int nch = cin_pad / IG_KC, ktiles = p.Kp / IG_KC;
  const AT* A = (const AT*)p.A + (long long)bi * t_in * p.lda;
  const bool norm = p.rms != 0;

  // staging: group q = tid + i*256 -> window row q/4, channels (q%4)*8 .. +8 of the chunk
  float sst[IG_GPT];
  float stg[IG_GPT][8];
#pragma unroll
  for (int i = 0; i < IG_GPT; ++i) sst[i] = 0.f;
  auto load_chunk = [&](int c) {
#pragma unroll
    for (int i = 0; i < IG_GPT; ++i) {
      const int q = tid + i * 256, r = q >> 2, ch = c * IG_KC + (q & 3) * 8;
      const int ti = t0 + t_off + r;
#pragma unroll
      for (int e = 0; e < 8; ++e) stg[i][e] = 0.f;
      if (r < WR && ti >= 0 && ti < t_in && ch < cin) load8f(A + (long long)ti * p.lda + ch, stg[i]);
    }
  };
  auto store_chunk = [&](int buf, int c) {
    bf16_t* wb = win + (size_t)buf * WR * IG_LDSW;
#pragma unroll
    for (int i = 0; i < IG_GPT; ++i) {
      const int q = tid + i * 256, r = q >> 2, ch = c * IG_KC + (q & 3) * 8;
      if (r >= WR) continue;
      float* v = stg[i];
      if (p.a_elu) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = elu_f(v[e]);
      }
      if (p.sn_a && ch < cin) {  // bf16 operand: the hardware sine's error is far below the bf16 rounding
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float sn = __sinf(v[e] * p.sn_a[ch + e]);
          v[e] = v[e] + p.sn_ib[ch + e] * (sn * sn);
        }
      }
      if (norm) {
#pragma unroll
        for (int e = 0; e < 8; ++e) sst[i] += v[e] * v[e];
      }
      *(u32x4_t*)(wb + r * IG_LDSW + (q & 3) * 8) =
          u32x4_t{pack2bf(v[0], v[1]), pack2bf(v[2], v[3]), pack2bf(v[4], v[5]), pack2bf(v[6], v[7])};
    }
  };

  f32x4_t acc[RT][CT];
#pragma unroll
  for (int i = 0; i < RT; ++i)
#pragma unroll
    for (int j = 0; j < CT; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  const bf16_t* Wb = (const bf16_t*)p.W + lane * 8;
  auto load_b = [&](u32x4_t* bf, int kt) {
#pragma unroll
    for (int j = 0; j < CT; ++j) {
      const int nt = min(nt0 + j, ntl - 1);
      bf[j] = *(const u32x4_t*)(Wb + ((size_t)nt * ktiles + kt) * 512);
    }
  };

  load_chunk(0);
  store_chunk(0, 0);
  __syncthreads();
  // B fragments PD k tiles ahead (a ring of PD register sets, the step loop unrolled by PD so every set index is a
  // compile-time constant): one tap of MFMA work was too little to cover an L2 round trip.  Steps run over
  // (chunk c, tap j) in chunk-major order; k tile = j * nch + c.
  constexpr int PD = IG_PD;
  const int S = nch * taps;
  u32x4_t bb[PD][CT];
  int pc = 0, pj = 0;  // (chunk, tap) of the next k tile to prefetch
#pragma unroll
  for (int u = 0; u < PD; ++u) {
    if (u < S) load_b(bb[u], pj * nch + pc);
    if (++pj == taps) { pj = 0; ++pc; }
  }
  int c = 0, j = 0;
  for (int s0 = 0; s0 < S; s0 += PD) {
#pragma unroll
    for (int u = 0; u < PD; ++u) {
      if (s0 + u < S) {
        if (j == 0 && c + 1 < nch) load_chunk(c + 1);
        const bf16_t* wb = win + (size_t)(c & 1) * WR * IG_LDSW;
        u32x4_t af[RT];
#pragma unroll
        for (int i = 0; i < RT; ++i) af[i] = *(const u32x4_t*)(wb + (wrow + i * 16 + lm + j * dil) * IG_LDSW + lk * 8);
#pragma unroll
        for (int i = 0; i < RT; ++i)
#pragma unroll
          for (int q = 0; q < CT; ++q)
            acc[i][q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, af[i]),
                                                                __builtin_bit_cast(bf16x8_t, bb[u][q]), acc[i][q], 0, 0, 0);
        if (pc < nch) load_b(bb[u], pj * nch + pc);
        if (++pj == taps) { pj = 0; ++pc; }
        if (j == taps - 1) {
          if (c + 1 < nch) store_chunk((c & 1) ^ 1, c + 1);
          __syncthreads();
        }
        if (++j == taps) { j = 0; ++c; }
      }
    }
  }
  if (norm) {  // rows 0..127 staged by 4 consecutive lanes each (window == tile when taps == 1)
#pragma unroll
    for (int i = 0; i < IG_GPT; ++i) {
      float s = sst[i];
      s += __shfl_xor(s, 1, 64);
      s += __shfl_xor(s, 2, 64);
      const int q = tid + i * 256, r = q >> 2;
      if ((q & 3) == 0 && r < BM) ss_row[r] = s;
    }
    __syncthreads();
  }
  OT* out = (OT*)p.out;
#pragma unroll
  for (int i = 0; i < RT; ++i) {
#pragma unroll
    for (int q = 0; q < CT; ++q) {
      const int nt = nt0 + q;
      if (nt >= ntl) continue;
      const int n = nt * 16 + lm;
      const bool nval = n < p.N;
      const float bias = (p.bias && nval) ? p.bias[n] : 0.f;
      const float cs = (p.colscale && nval) ? p.colscale[n] : 1.f;
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int rl = wrow + i * 16 + lk * 4 + e;
        float x = acc[i][q][e];
        if (norm) x *= rsqrtf(ss_row[rl] / (float)p.Klog + p.eps);
        x += bias;
        if (p.act != QT_ACT_NONE) x = act_f_call(x, p.act);
        v[e] = x * cs;
      }
      if (p.epi == QT_EPI_SWIGLU) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float up = __shfl_xor(v[e], 8, 64);
          const int t = t0 + wrow + i * 16 + lk * 4 + e;
          if (lm < 8 && t < t_out && nt * 8 + lm < (p.N >> 1))
            out[((long long)bi * t_out + t) * p.ldo + nt * 8 + lm] = from_f<OT>(silu_f(v[e]) * up);
        }
        continue;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int t = t0 + wrow + i * 16 + lk * 4 + e;
        if (t >= t_out || !nval) continue;
        OT* o = out + ((long long)bi * t_out + t) * p.ldo + n;
        if (p.epi == QT_EPI_ADD) *o = from_f<OT>(to_f(*o) + v[e]);
        else *o = from_f<OT>(v[e]);
      }
    }
  }
}

// Prefill linear GEMM (taps == 0, bf16 pre-tiled weights, M >= 128 rows): block tile 128 rows x NTB*16 columns,
// 4 waves in a 2 x 2 grid (wave = 64 rows x NTB/2 column tiles of 16x16x32 MFMAs), K in 64-wide stages.  Both
// operands are staged through LDS and double-buffered: the next stage's global loads (A rows fp32/bf16 -> bf16 with
// the RMS sums of squares taken on the way, B as the pre-tiled 1 KiB fragments, copied verbatim) are in flight
// while the current stage is multiplied, one barrier per stage.  igemm_k streamed B straight from L2 one k tile
// ahead, which left every MFMA group waiting on an L2 round trip (tools/prefill_gemm_bench.py: M=680 gate-up
// 106.8 us = 320 TFLOP/s).  Same operand rounding and per-element k order as igemm_k.
constexpr int PF_BM = 128, PF_BK = 64, PF_AST = PF_BK + 8;  // A LDS row stride (bf16): 144 B

template <typename AT, typename OT, int NTB>
__global__ __launch_bounds__(256) void gemm_pf_k(GemmP p) {
  constexpr int CT = NTB / 2;                 // column tiles per wave
  constexpr int BT = NTB * 2;                 // B fragments (1 KiB) per stage
  constexpr int BPT = BT * 64 / 256;          // 16-byte B loads per thread per stage
  constexpr int AE = sizeof(AT) == 4 ? 8 : 4; // 16-byte A loads per thread per stage (32 elements)
  __shared__ __attribute__((aligned(16))) bf16_t As[2][PF_BM * PF_AST];
  __shared__ __attribute__((aligned(16))) bf16_t Bs[2][BT * 512];
  __shared__ float ss_row[PF_BM];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int lm = lane & 15, lk = lane >> 4;
  const int m0 = blockIdx.x * PF_BM, nt0 = blockIdx.y * NTB;
  const int ntl = (p.N + 15) / 16, ktiles = p.Kp / 32, S = (ktiles + 1) / 2;
  const int wr = (w >> 1) * 64, wc = (w & 1) * CT;
  const bool norm = p.rms != 0;
  // A staging: thread -> row ar (0..127), k half ah (32 elements)
  const int ar = tid >> 1, ah = tid & 1;
  const bool arow = m0 + ar < p.M;
  const AT* Ar = (const AT*)p.A + (long long)(arow ? m0 + ar : 0) * p.lda;
  float sst = 0.f;
  u32x4_t ra[AE], rb[BPT];
  auto load_stage = [&](int st, u32x4_t* ra, u32x4_t* rb) {
    const int k0 = st * PF_BK + ah * 32;
#pragma unroll
    for (int i = 0; i < AE; ++i) {
      const int k = k0 + i * (32 / AE);
      ra[i] = (arow && k < p.Klog) ? *(const u32x4_t*)(Ar + k) : u32x4_t{0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int i = 0; i < BPT; ++i) {
      const int q = tid + i * 256, ti = q >> 6;      // fragment ti of the stage: column tile ti >> 1, k tile ti & 1
      const int nt = min(nt0 + (ti >> 1), ntl - 1), kt = st * 2 + (ti & 1);
      const bf16_t* src = (const bf16_t*)p.W + ((size_t)nt * ktiles + min(kt, ktiles - 1)) * 512 + (q & 63) * 8;
      rb[i] = kt < ktiles ? *(const u32x4_t*)src : u32x4_t{0u, 0u, 0u, 0u};
    }
  };
  auto store_stage = [&](int buf, const u32x4_t* ra, const u32x4_t* rb) {
    bf16_t* ad = As[buf] + ar * PF_AST + ah * 32;
    if constexpr (sizeof(AT) == 4) {
#pragma unroll
      for (int i = 0; i < AE; i += 2) {  // two 16-byte fp32 loads -> one 16-byte bf16 store
        float v[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) { v[e] = __uint_as_float(ra[i][e]); v[4 + e] = __uint_as_float(ra[i + 1][e]); }
        if (norm) {
#pragma unroll
          for (int e = 0; e < 8; ++e) sst += v[e] * v[e];
        }
        *(u32x4_t*)(ad + i * 4) =
            u32x4_t{pack2bf(v[0], v[1]), pack2bf(v[2], v[3]), pack2bf(v[4], v[5]), pack2bf(v[6], v[7])};
      }
    } else {
#pragma unroll
      for (int i = 0; i < AE; ++i) {
        if (norm) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float lo = __uint_as_float(ra[i][e] << 16), hi = __uint_as_float(ra[i][e] & 0xFFFF0000u);
            sst += lo * lo + hi * hi;
          }
        }
        *(u32x4_t*)(ad + i * 8) = ra[i];
      }
    }
    bf16_t* bd = Bs[buf];
#pragma unroll
    for (int i = 0; i < BPT; ++i) *(u32x4_t*)(bd + (size_t)(tid + i * 256) * 8) = rb[i];
  };
  f32x4_t acc[4][CT];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < CT; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  auto compute = [&](int buf) {
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      u32x4_t af[4], bf[CT];
#pragma unroll
      for (int i = 0; i < 4; ++i) af[i] = *(const u32x4_t*)(As[buf] + (wr + i * 16 + lm) * PF_AST + kk * 32 + lk * 8);
#pragma unroll
      for (int j = 0; j < CT; ++j) bf[j] = *(const u32x4_t*)(Bs[buf] + ((wc + j) * 2 + kk) * 512 + lane * 8);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < CT; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, af[i]),
                                                              __builtin_bit_cast(bf16x8_t, bf[j]), acc[i][j], 0, 0, 0);
    }
  };
  load_stage(0, ra, rb);
  store_stage(0, ra, rb);
  __syncthreads();
  for (int st = 0; st < S; ++st) {
    const int buf = st & 1;
    if (st + 1 < S) load_stage(st + 1, ra, rb);
    compute(buf);
    if (st + 1 < S) store_stage(buf ^ 1, ra, rb);
    __syncthreads();
  }
  if (norm) {
    const float s2 = sst + __shfl_xor(sst, 1, 64);
    if (ah == 0) ss_row[ar] = s2;
    __syncthreads();
  }
  OT* out = (OT*)p.out;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int q = 0; q < CT; ++q) {
      const int nt = nt0 + wc + q;
      if (nt >= ntl) continue;
      const int n = nt * 16 + lm;
      const bool nval = n < p.N;
      const float bias = (p.bias && nval) ? p.bias[n] : 0.f;
      const float cs = (p.colscale && nval) ? p.colscale[n] : 1.f;
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int rl = wr + i * 16 + lk * 4 + e;
        float x = acc[i][q][e];
        if (norm) x *= rsqrtf(ss_row[rl] / (float)p.Klog + p.eps);
        x += bias;
        if (p.act != QT_ACT_NONE) x = act_f_call(x, p.act);
        v[e] = x * cs;
      }
      if (p.epi == QT_EPI_SWIGLU) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float up = __shfl_xor(v[e], 8, 64);
          const int m = m0 + wr + i * 16 + lk * 4 + e;
          if (lm < 8 && m < p.M && nt * 8 + lm < (p.N >> 1))
            out[(long long)m * p.ldo + nt * 8 + lm] = from_f<OT>(silu_f(v[e]) * up);
        }
        continue;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int m = m0 + wr + i * 16 + lk * 4 + e;
        if (m >= p.M || !nval) continue;
        OT* o = out + (long long)m * p.ldo + n;
        const float r = p.epi == QT_EPI_ADD ? to_f(*o) + v[e] : v[e];
        *o = from_f<OT>(r);
        if (p.out2) p.out2[(long long)m * p.ldo2 + n] = f2bf(r);
      }
    }
  }
}


// Single-output-channel causal conv (codec conv_last, Cout = 1): memory-bound, so no MFMA.  A block owns
// 256 consecutive outputs of one batch item; the input window (256 + (taps-1)*dil rows) x 32 channels is staged
// in LDS per channel chunk (SnakeBeta applied on staging) and each thread accumulates its output's taps x cin
// products in fp32.  Weights are read from the row-major [taps][cin_pad] tile row 0 (N = 1 -> tile 0, lane
// group layout: element (k) of tile kt sits at lane (k % 32) / 8 * 16, offset k % 8).
template <typename AT, typename WT, typename OT>
__global__ __launch_bounds__(256) void conv_n1_k(GemmP p) {
  constexpr int KC = 32, WS = KC + 1;
  extern __shared__ float c1_win[];  // [WR][WS]
  const int tid = threadIdx.x;
  const int taps = p.taps, dil = p.dil;
  const int WR = 256 + (taps - 1) * dil;
  const int tiles_t = (p.t_out + 255) / 256;
  const int bi = blockIdx.x / tiles_t, t0 = (blockIdx.x - bi * tiles_t) * 256;
  const AT* A = (const AT*)p.A + (long long)bi * p.t_in * p.lda;
  const WT* W = (const WT*)p.W;
  constexpr int E = sizeof(WT) == 2 ? 8 : 4, KT = 4 * E;
  __shared__ float wsh[2048];  // taps * cin_pad weights of output channel 0 (host checks the size)
  for (int k = tid; k < taps * p.cin_pad; k += 256) {
    const int kt = k / KT, kin = k % KT;
    wsh[k] = to_f(W[(size_t)kt * 64 * E + (kin / E) * 16 * E + (kin % E)]);
  }
  float acc = 0.f;
  // vector staging (8 channels = one 16-byte load per group, every load of a chunk issued before the first use;
  // clamped addresses, no branch around the loads) when the channel layout allows it
  const bool vec = sizeof(AT) == 2 && p.cin % 8 == 0 && p.lda % 8 == 0 && WR * (KC / 8) <= 256 * 8;
  for (int c0 = 0; c0 < p.cin; c0 += KC) {
    __syncthreads();
    if (vec) {
      float v[8][8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int g = tid + i * 256, r = min(g >> 2, WR - 1), ch = min(c0 + (g & 3) * 8, p.cin - 8);
        const int ti = min(max(t0 + p.t_off + r, 0), p.t_in - 1);
        load8f(A + (long long)ti * p.lda + ch, v[i]);
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int g = tid + i * 256, r = g >> 2, cl = (g & 3) * 8, c = c0 + cl;
        const int ti = t0 + p.t_off + r;
        if (r >= WR) continue;
        const bool ok = ti >= 0 && ti < p.t_in && c < p.cin;
        float sa[8], sb[8];  // SnakeBeta parameters of the group's 8 channels: two vector loads
        if (p.sn_a) {
          load8f(p.sn_a + min(c, p.cin - 8), sa);
          load8f(p.sn_ib + min(c, p.cin - 8), sb);
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          float x = 0.f;
          if (ok) {
            x = v[i][e];
            if (p.a_elu) x = elu_f(x);
            if (p.sn_a) x = snake1(x, sa[e], sb[e]);
            if (sizeof(WT) == 2) x = __uint_as_float((unsigned)f2bf(x) << 16);  // bf16 operand, as the MFMA paths
          }
          c1_win[r * WS + cl + e] = x;
        }
      }
    } else {
    for (int q = tid; q < WR * KC; q += 256) {
      const int r = q / KC, c = c0 + q % KC;
      const int ti = t0 + p.t_off + r;
      float v = 0.f;
      if (ti >= 0 && ti < p.t_in && c < p.cin) {
        v = to_f(A[(long long)ti * p.lda + c]);
        if (p.a_elu) v = elu_f(v);
        if (p.sn_a) v = snake1(v, p.sn_a[c], p.sn_ib[c]);
        if (sizeof(WT) == 2) v = __uint_as_float((unsigned)f2bf(v) << 16);  // bf16 operand, as the MFMA paths
      }
      c1_win[r * WS + q % KC] = v;
    }
    }
    __syncthreads();
    for (int j = 0; j < taps; ++j) {
      const float* row = c1_win + (tid + j * dil) * WS;
      const float* wr = wsh + j * p.cin_pad + c0;  // K index of the [1][taps*cin_pad] weight row
      const int nc = min(KC, p.cin - c0);
#pragma unroll 8
      for (int cc = 0; cc < nc; ++cc) acc += wr[cc] * row[cc];
    }
  }
  const int t = t0 + tid;
  if (t < p.t_out) {
    float x = acc + (p.bias ? p.bias[0] : 0.f);
    OT* o = (OT*)p.out + ((long long)bi * p.t_out + t) * p.ldo;
    *o = from_f<OT>(p.epi == QT_EPI_ADD ? to_f(*o) + x : x);
  }
}

// the decode GEMV instantiation of the plan: gemv_wt<WPB, U, NORM, NTL, F>
template <typename WT, typename AT, typename OT, int WPB, int U, int F>
void launch_gemv_f(const GemmP& p, const GemmPlan& pl, hipStream_t s) {
  const dim3 grid((p.N + 15) / 16, p.ks, (p.M + p.mr - 1) / p.mr), block(WPB * 64);
  if (pl.nt_loads) {
    if (p.rms) hipLaunchKernelGGL((gemv_wt<WT, AT, OT, WPB, U, true, true, F>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((gemv_wt<WT, AT, OT, WPB, U, false, true, F>), grid, block, 0, s, p);
  } else {
    if (p.rms) hipLaunchKernelGGL((gemv_wt<WT, AT, OT, WPB, U, true, false, F>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((gemv_wt<WT, AT, OT, WPB, U, false, false, F>), grid, block, 0, s, p);
  }
}
template <typename WT, typename AT, typename OT, int WPB, int U>
void launch_gemv_u(const GemmP& p, const GemmPlan& pl, hipStream_t s) {
  if constexpr (sizeof(WT) == 2) {  // the row folds exist for bf16 weights
    if (pl.fold == 4) return launch_gemv_f<WT, AT, OT, WPB, U, 4>(p, pl, s);
    if (pl.fold == 2) return launch_gemv_f<WT, AT, OT, WPB, U, 2>(p, pl, s);
  }
  launch_gemv_f<WT, AT, OT, WPB, U, 1>(p, pl, s);
}
template <typename WT, typename AT, typename OT, int WPB>
void launch_gemv(const GemmP& p, const GemmPlan& pl, hipStream_t s) {
  if (pl.u == 8) launch_gemv_u<WT, AT, OT, WPB, 8>(p, pl, s);
  else launch_gemv_u<WT, AT, OT, WPB, 4>(p, pl, s);
}

template <typename AT, typename OT>
void launch_igemm(const GemmP& p, const GemmPlan& pl, hipStream_t s) {
  const int nt = (p.N + 15) / 16;
  const int taps = p.taps == 0 ? 1 : p.taps, dil = p.taps == 0 ? 1 : p.dil;
  const int t_out = p.taps == 0 ? p.M : p.t_out, batches = p.taps == 0 ? 1 : p.M / p.t_out;
  const int bm = 64 * pl.mi;
  const int WR = bm + (taps - 1) * dil;
  const size_t smem = (size_t)2 * WR * IG_LDSW * sizeof(bf16_t);
  const dim3 grid(batches * ((t_out + bm - 1) / bm), (nt + pl.ntb - 1) / pl.ntb);
#define IG_GO(N_, M_) hipLaunchKernelGGL((igemm_k<AT, OT, N_, M_>), grid, dim3(256), smem, s, p)
  switch (pl.ntb * 10 + pl.mi) {
    case 62: IG_GO(6, 2); break;
    case 61: IG_GO(6, 1); break;
    case 42: IG_GO(4, 2); break;
    case 41: IG_GO(4, 1); break;
    case 81: IG_GO(8, 1); break;
    default: IG_GO(8, 2); break;
  }
#undef IG_GO
}

// launch the kernel family the plan names (gemm_route.h decides; nothing is decided here)
template <typename WT, typename AT, typename OT>
int launch(const GemmP& p, const GemmPlan& pl, GemmRoute route, hipStream_t s) {
  const int nt = (p.N + 15) / 16;
  constexpr bool BF2 = sizeof(WT) == 2 && sizeof(AT) == 2;  // SK / PF2 / PF: bf16 A and bf16 weights (the planner's rule)
  switch (route) {
    case GemmRoute::SK:
      if constexpr (!BF2) return QT_ERR_DTYPE;
      else if constexpr (std::is_same<OT, float>::value) qt_gemm_impl::launch_sk_f32(p, pl.sk_mi, s);
      else qt_gemm_impl::launch_sk_bf16(p, pl.sk_mi, s);
      break;
    case GemmRoute::GEMV:
      if (pl.wpb == 16) launch_gemv<WT, AT, OT, 16>(p, pl, s);
      else if (pl.wpb == 8) launch_gemv<WT, AT, OT, 8>(p, pl, s);
      else launch_gemv<WT, AT, OT, 4>(p, pl, s);
      break;
    case GemmRoute::CONV_N1: {
      const size_t smem = (size_t)(256 + (p.taps - 1) * p.dil) * 33 * sizeof(float);
      const int batches = p.M / p.t_out;
      hipLaunchKernelGGL((conv_n1_k<AT, WT, OT>), dim3(batches * ((p.t_out + 255) / 256)), dim3(256), smem, s, p);
      break;
    }
    case GemmRoute::WT_1x8: hipLaunchKernelGGL((gemm_wt<WT, AT, OT, 1, 8>), dim3(nt, 1), dim3(512), 0, s, p); break;
    case GemmRoute::PF2:
      if constexpr (!BF2) return QT_ERR_DTYPE;
      else if constexpr (std::is_same<OT, float>::value) qt_gemm_impl::launch_pf2_f32(p, pl.pf2_cfg, pl.pf2_ks, s);
      else qt_gemm_impl::launch_pf2_bf16(p, pl.pf2_cfg, pl.pf2_ks, s);
      break;
    case GemmRoute::PF: {
      const int mt = (p.M + PF_BM - 1) / PF_BM;
      if constexpr (!BF2) return QT_ERR_DTYPE;
      else if (pl.ntb == 4) hipLaunchKernelGGL((gemm_pf_k<AT, OT, 4>), dim3(mt, (nt + 3) / 4), dim3(256), 0, s, p);
      else hipLaunchKernelGGL((gemm_pf_k<AT, OT, 8>), dim3(mt, (nt + 7) / 8), dim3(256), 0, s, p);
      break;
    }
    case GemmRoute::IGEMM: launch_igemm<AT, OT>(p, pl, s); break;
    case GemmRoute::WT_2x8:
      hipLaunchKernelGGL((gemm_wt<WT, AT, OT, 2, 8>), dim3(nt, (p.M + 31) / 32), dim3(512), 0, s, p);
      break;
    case GemmRoute::WT_4x4:
      hipLaunchKernelGGL((gemm_wt<WT, AT, OT, 4, 4>), dim3(nt, (p.M + 63) / 64), dim3(256), 0, s, p);
      break;
    default: return QT_ERR_ARG;  // NONE / IM2COL are resolved by qt_gemm
  }
  return hipGetLastError() == hipSuccess ? 0 : QT_ERR_LAUNCH;
}

// row-major [N][Kp] -> tiled fragments
template <typename T, int E>
__global__ void tile_weight_k(const T* __restrict__ src, T* __restrict__ dst, int N, int Kp) {
  const long long tile = blockIdx.x;  // nt * ktiles + kt
  const int ktiles = Kp / (4 * E);
  const int nt = tile / ktiles, kt = tile % ktiles;
  const int lane = threadIdx.x;
  const int n = nt * 16 + (lane & 15);
  const int k = kt * 4 * E + (lane >> 4) * E;
  T* d = dst + tile * 64 * E + lane * E;
#pragma unroll
  for (int i = 0; i < E; ++i) d[i] = (n < N) ? src[(long long)n * Kp + k + i] : T(0);
}

}  // namespace

namespace {
// im2col for short conv windows (qt_gemm's small-M conv route below): row m = (item b, output step t), column
// j * cin_pad + c = input channel c at time t + t_off + j * dil of item b (zero outside [0, t_in) and past cin), with
// the ELU / SnakeBeta prologue applied and the value rounded to bf16 exactly as igemm_k stages it.  One thread per
// (row, tap, 8-channel group), 16-byte loads and stores.
template <typename AT>
__global__ __launch_bounds__(256) void im2col_k(GemmP p, bf16_t* __restrict__ out) {
  const int g = p.cin_pad / 8, tg = p.taps * g;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)p.M * tg) return;
  const int m = (int)(idx / tg), r = (int)(idx % tg), j = r / g, ch = (r % g) * 8;
  const int b = m / p.t_out, t = m % p.t_out, ti = t + p.t_off + j * p.dil;
  float v[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = 0.f;
  if (ti >= 0 && ti < p.t_in && ch < p.cin) load8f((const AT*)p.A + ((long long)b * p.t_in + ti) * p.lda + ch, v);
  if (p.a_elu) {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = elu_f(v[e]);
  }
  if (p.sn_a && ch < p.cin) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float sn = __sinf(v[e] * p.sn_a[ch + e]);
      v[e] = v[e] + p.sn_ib[ch + e] * (sn * sn);
    }
  }
  *(u32x4_t*)(out + (long long)m * p.Kp + j * p.cin_pad + ch) =
      u32x4_t{pack2bf(v[0], v[1]), pack2bf(v[2], v[3]), pack2bf(v[4], v[5]), pack2bf(v[6], v[7])};
}

// the routing constants: compiled-in defaults, read from the environment once by a probe build (tools/*.sh A/B runs)
const GemmKnobs& gemm_knobs() {
  static const GemmKnobs knobs = [] {
    GemmKnobs k;
    if (kProbe) {
#define QT_K(f, name) k.f = qt_knob(name, k.f)
      QT_K(gemv_fold, "QT_GEMV_FOLD"); QT_K(gemv_u, "QT_GEMV_U"); QT_K(gemv_max_m, "QT_GEMV_MAX_M");
      QT_K(gemv_nt, "QT_GEMV_NT"); QT_K(gemv_wpb, "QT_GEMV_WPB"); QT_K(gemv_split_auto, "QT_GEMV_SPLIT_AUTO");
      QT_K(gemv_rg, "QT_GEMV_RG"); QT_K(skinny, "QT_SKINNY"); QT_K(sk, "QT_SK"); QT_K(sk_max_m, "QT_SK_MAX_M");
      QT_K(im2col, "QT_IM2COL"); QT_K(im2col_max_m, "QT_IM2COL_MAX_M"); QT_K(igemm_min_m, "QT_IGEMM_MIN_M");
      QT_K(no_igemm, "QT_NO_IGEMM"); QT_K(pf, "QT_PF"); QT_K(pf2_split, "QT_PF2_SPLIT"); QT_K(pf2_cfg, "QT_PF2_CFG");
      QT_K(pf2_pp, "QT_PF2_PP");
#undef QT_K
      const char* e = qt_knob_str("QT_IGEMM_CFG");  // "NT,MI"
      k.igemm_cfg = e ? atoi(e) * 10 + atoi(e + 2) : 0;
    }
    return k;
  }();
  return knobs;
}

// the kernels' argument block of one call
GemmP gemm_params(const qt_gemm_args& a, const GemmPlan& pl) {
  GemmP p;
  p.M = a.M; p.N = a.N; p.Kp = pl.kp; p.Klog = a.K;
  p.A = a.A; p.lda = a.lda; p.a_index = a.a_index; p.W = a.W;
  p.gamma = a.gamma; p.eps = a.eps; p.rms = a.rmsnorm || a.gamma != nullptr; p.bias = a.bias; p.colscale = a.colscale;
  p.act = a.act; p.epi = a.epi; p.out = a.out; p.ldo = a.ldo;
  p.taps = a.taps > 0 ? a.taps : 0; p.dil = a.dil > 0 ? a.dil : 1; p.cin = a.cin; p.cin_pad = a.cin_pad;
  p.t_in = a.t_in; p.t_out = a.t_out; p.t_off = a.t_off;
  p.ks = pl.ks; p.mr = std::max(1, pl.mr);
  p.cnt = pl.ws_split ? (unsigned*)a.ws : nullptr;
  p.part = pl.ws_split ? (float*)((char*)a.ws + qt_gemm_impl::WS_CNT_BYTES) : nullptr;
  p.sn_a = a.snake_alpha; p.sn_ib = a.snake_inv_beta;
  p.a_elu = a.a_act == QT_AACT_ELU;
  p.out2 = (bf16_t*)a.out2; p.ldo2 = a.ldo2;
  return p;
}
}  // namespace

extern "C" int qt_gemm_route(const qt_gemm_args* a, qt_gemm_route_info* info) {
  if (!a || !info) return QT_ERR_ARG;
  const GemmPlan pl = gemm_plan(*a, gemm_knobs());
  *info = qt_gemm_route_info{};
  if (pl.route == GemmRoute::NONE) return pl.err;
  *info = qt_gemm_route_info{(int)pl.route, (int)pl.inner, pl.ks, pl.mr, pl.wpb, pl.u, pl.fold, pl.nt_loads,
                             pl.pf2_cfg, pl.pf2_ks, pl.ntb, pl.mi, pl.sk_mi, pl.ws_split ? 1 : 0};
  return 0;
}

extern "C" int qt_gemm(const qt_gemm_args* a, void* stream) {
  if (!a) return QT_ERR_ARG;
  const GemmPlan pl = gemm_plan(*a, gemm_knobs());
  if (pl.route == GemmRoute::NONE) return pl.err;
  hipStream_t s = (hipStream_t)stream;
  GemmRoute route = pl.route;
  qt_gemm_args img;  // IM2COL: the linear call on the image
  if (route == GemmRoute::IM2COL) {
    // the image lives in the upper half of the caller's workspace (gemm_route.h im2col_applies)
    img = qt_gemm_impl::im2col_linear_args(*a);
    const GemmP q = gemm_params(*a, pl);
    const long long n = (long long)a->M * a->taps * (a->cin_pad / 8);
    const dim3 grid((unsigned)((n + 255) / 256));
    if (a->a_dtype == QT_BF16) hipLaunchKernelGGL(im2col_k<bf16_t>, grid, dim3(256), 0, s, q, (bf16_t*)img.A);
    else hipLaunchKernelGGL(im2col_k<float>, grid, dim3(256), 0, s, q, (bf16_t*)img.A);
    if (hipGetLastError() != hipSuccess) return QT_ERR_LAUNCH;
    a = &img;
    route = pl.inner;
  }
  const GemmP p = gemm_params(*a, pl);
  const int w = a->w_dtype, ad = a->a_dtype, o = a->o_dtype;
  if (w == QT_BF16 && ad == QT_F32 && o == QT_F32) return launch<bf16_t, float, float>(p, pl, route, s);
  if (w == QT_BF16 && ad == QT_BF16 && o == QT_BF16) return launch<bf16_t, bf16_t, bf16_t>(p, pl, route, s);
  if (w == QT_BF16 && ad == QT_BF16 && o == QT_F32) return launch<bf16_t, bf16_t, float>(p, pl, route, s);
  if (w == QT_BF16 && ad == QT_F32 && o == QT_BF16) return launch<bf16_t, float, bf16_t>(p, pl, route, s);
  if (w == QT_F32 && ad == QT_F32 && o == QT_F32) return launch<float, float, float>(p, pl, route, s);
  return QT_ERR_DTYPE;
}

extern "C" int qt_tile_weight(const void* src, int dtype, int N, int Kp, void* dst, void* stream) {
  const int E = dtype == QT_BF16 ? 8 : 4;
  if (N <= 0 || Kp % (4 * E)) return QT_ERR_SHAPE;
  const int ntiles = (N + 15) / 16, ktiles = Kp / (4 * E);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == QT_BF16)
    hipLaunchKernelGGL((tile_weight_k<bf16_t, 8>), dim3(ntiles * ktiles), dim3(64), 0, s, (const bf16_t*)src,
                       (bf16_t*)dst, N, Kp);
  else if (dtype == QT_F32)
    hipLaunchKernelGGL((tile_weight_k<float, 4>), dim3(ntiles * ktiles), dim3(64), 0, s, (const float*)src,
                       (float*)dst, N, Kp);
  else
    return QT_ERR_DTYPE;
  return hipGetLastError() == hipSuccess ? 0 : QT_ERR_LAUNCH;
}
