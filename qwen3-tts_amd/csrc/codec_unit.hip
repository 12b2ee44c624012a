// One launch per codec residual unit (DecoderResidualUnit, modeling_qwen3_tts_tokenizer_v2.py:618-634) for the
// 96- and 192-channel decoder blocks, bf16 activations and bf16 pre-tiled weights, channels-last:
//
//   x_out[b, t, :] = bf16( x_in[b, t, :] + W2 . snake2( bf16( sum_j W1_j . snake1(x_in)[b, t - (6 - j) dil, :] + b1 ) ) + b2 )
//
// It replaces two igemm_k launches (k = 7 dilated conv into a scratch tensor, then k = 1 conv with the residual add)
// and is bit-identical to them: the same operand roundings (snake in fp32 with the hardware sine, rounded to bf16; the
// k = 7 output rounded to bf16 before snake2) and, per 16 x 16 output tile, the same v_mfma_f32_16x16x32_bf16 sequence
// (k = 7: 32-channel chunks outer, taps inner; k = 1: chunks ascending).
//
// Block = BM (64 MI) rows of one batch item x all C channels, 4 waves in a 2 x 2 grid (wave = BM/2 rows x C/2
// columns).  One LDS image of (BM + 6 dil) rows x (C + 8) bf16 is used four times in turn:
//   1. the snake1'd input window over all C channels (staged once, not once per column block as igemm_k does);
//   2. after the k = 7 MFMAs: the snake2'd k = 7 output tile, the A operand of the k = 1 MFMAs (it never leaves the CU);
//   3. after the k = 1 MFMAs: the tile's raw x_in rows (re-read as 16-byte loads issued before the k = 1 MFMAs),
//      updated in place by the lane that owns each accumulator element;
//   4. read back as 16-byte rows for the x_out stores.
// The image of the shipped tiles (128 rows for C = 96, 64 rows for C = 192) is at most 37 / 46 KiB at dil = 9, so four /
// three workgroups share a CU (the register budget is held to that) and cover each other's staging, barriers and
// epilogues: latency is hidden by occupancy, and taller tiles that cut it measured slower.  Weights stream from L2
// one k tile ahead as in igemm_k.  No split-K, no atomics, no hand-off between workgroups: x_out must not alias x_in
// (neighbouring tiles read x_in's halo rows).  The template takes any C % 32 == 0 whose image fits (C = 384 at 64
// rows: 90 KiB, one workgroup per CU -- not instantiated: without occupancy it needs an in-block pipeline first).
#include "common.h"

namespace {

constexpr int CU_TAPS = 7;
constexpr int CU_MAX_DIL = 9;  // window rows <= BM + 54

// workgroups (= waves per SIMD) the LDS image lets a CU hold at dil = 9; the register budget is held to it
constexpr int unit_wpe(int C, int MI) { return C == 96 ? (MI == 4 ? 2 : 4) : (MI == 1 ? 3 : 2); }

template <int C, int MI>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(unit_wpe(C, MI)))) void codec_unit_k(
    qt_codec_resunit_args p) {
  constexpr int BM = 64 * MI;      // rows per block
  constexpr int RT = BM / 32;      // 16-row MFMA tiles per wave
  constexpr int NCH = C / 32;      // 32-channel k chunks
  constexpr int CT = C / 32;       // 16-column tiles per wave (half of C / 16)
  constexpr int G = C / 8;         // 16-byte groups per row
  constexpr int LDW = C + 8;       // LDS row stride (bf16): 16-byte rows, b128 fragment reads conflict-free
  constexpr int RPI = 256 / G;     // window rows staged per pass (threads >= RPI * G idle while staging)
  constexpr int NR = BM * G / 256; // 16-byte groups of the output tile per thread
  static_assert(BM * G % 256 == 0, "output tile groups divide over the block");
  extern __shared__ __attribute__((aligned(16))) unsigned char cu_smem[];
  bf16_t* img = (bf16_t*)cu_smem;  // [BM + 6 dil][LDW]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int lm = lane & 15, lk = lane >> 4;
  const int dil = p.dil, halo = (CU_TAPS - 1) * dil, WR = BM + halo;
  const int tiles_t = (p.L + BM - 1) / BM;
  const int bi = blockIdx.x / tiles_t, t0 = (blockIdx.x - bi * tiles_t) * BM;
  const bf16_t* xin = (const bf16_t*)p.x_in + (long long)bi * p.L * C;
  bf16_t* xout = (bf16_t*)p.x_out + (long long)bi * p.L * C;

  // 1. window rows [t0 - halo, t0 + BM) -> snake1 -> bf16 (rows outside [0, L) are zero; snake(0) = 0)
  {
    const int g = tid % G, r0 = tid / G;
    if (r0 < RPI) {
      float sa[8], sib[8];
      load8f(p.s1_alpha + g * 8, sa);
      load8f(p.s1_inv_beta + g * 8, sib);
      for (int rb = r0; rb < WR; rb += 4 * RPI) {
        u32x4_t raw[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int r = rb + u * RPI, ti = t0 - halo + r;
          raw[u] = u32x4_t{0u, 0u, 0u, 0u};
          if (r < WR && ti >= 0 && ti < p.L) raw[u] = *(const u32x4_t*)(xin + (long long)ti * C + g * 8);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int r = rb + u * RPI;
          if (r >= WR) break;
          float v[8];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            v[2 * i] = __uint_as_float(raw[u][i] << 16);
            v[2 * i + 1] = __uint_as_float(raw[u][i] & 0xFFFF0000u);
          }
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float sn = __sinf(v[e] * sa[e]);
            v[e] = v[e] + sib[e] * (sn * sn);
          }
          *(u32x4_t*)(img + r * LDW + g * 8) =
              u32x4_t{pack2bf(v[0], v[1]), pack2bf(v[2], v[3]), pack2bf(v[4], v[5]), pack2bf(v[6], v[7])};
        }
      }
    }
  }

  const int wrow = (w >> 1) * (BM / 2);  // first row of this wave in the tile
  const int nt0 = (w & 1) * CT;          // first 16-column tile of this wave
  f32x4_t acc[RT][CT];
#pragma unroll
  for (int i = 0; i < RT; ++i)
#pragma unroll
    for (int q = 0; q < CT; ++q) acc[i][q] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  // 2. k = 7 conv: k tile of (chunk c, tap j) = j * NCH + c; B fragments (1 KiB per 16 x 32 tile) one step ahead
  {
    constexpr int KT = CU_TAPS * NCH;
    const bf16_t* Wb = (const bf16_t*)p.w1 + lane * 8;
    u32x4_t cur[CT], nxt[CT];
#pragma unroll
    for (int q = 0; q < CT; ++q) cur[q] = *(const u32x4_t*)(Wb + ((size_t)(nt0 + q) * KT) * 512);
    __syncthreads();
#pragma unroll 1  // unrolled, the compiler hoists the B loads of later chunks and spills
    for (int c = 0; c < NCH; ++c) {
      const bf16_t* wa = img + (wrow + lm) * LDW + c * 32 + lk * 8;
#pragma unroll
      for (int j = 0; j < CU_TAPS; ++j) {
        const int kn = j + 1 < CU_TAPS ? (j + 1) * NCH + c : (c + 1 < NCH ? c + 1 : c);
#pragma unroll
        for (int q = 0; q < CT; ++q) nxt[q] = *(const u32x4_t*)(Wb + ((size_t)(nt0 + q) * KT + kn) * 512);
        u32x4_t af[RT];
#pragma unroll
        for (int i = 0; i < RT; ++i) af[i] = *(const u32x4_t*)(wa + (i * 16 + j * dil) * LDW);
#pragma unroll
        for (int i = 0; i < RT; ++i)
#pragma unroll
          for (int q = 0; q < CT; ++q)
            acc[i][q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, af[i]),
                                                                __builtin_bit_cast(bf16x8_t, cur[q]), acc[i][q], 0, 0, 0);
#pragma unroll
        for (int q = 0; q < CT; ++q) cur[q] = nxt[q];
      }
    }
  }
  __syncthreads();  // every wave is done with the window

  // the tile's raw x_in rows for the residual add: 16-byte loads in flight over the k = 1 MFMAs
  u32x4_t xr[NR];
#pragma unroll
  for (int u = 0; u < NR; ++u) {
    const int q = tid + u * 256, r = q / G, g = q - r * G;
    xr[u] = u32x4_t{0u, 0u, 0u, 0u};
    if (t0 + r < p.L) xr[u] = *(const u32x4_t*)(xin + (long long)(t0 + r) * C + g * 8);
  }

  // 3. + b1, round to bf16 (the k = 7 conv's stored output), snake2, round to bf16 -> the k = 1 conv's A tile
#pragma unroll
  for (int q = 0; q < CT; ++q) {
    const int n = (nt0 + q) * 16 + lm;
    const float b1 = p.b1 ? p.b1[n] : 0.f, a2 = p.s2_alpha[n], ib2 = p.s2_inv_beta[n];
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float h = bf2f(f2bf(acc[i][q][e] + b1));
        const float sn = __sinf(h * a2);
        img[(wrow + i * 16 + lk * 4 + e) * LDW + n] = f2bf(h + ib2 * (sn * sn));
        acc[i][q][e] = 0.f;
      }
  }

  // 4. k = 1 conv, chunks ascending
  {
    const bf16_t* Wb = (const bf16_t*)p.w2 + lane * 8;
    u32x4_t cur[CT], nxt[CT];
#pragma unroll
    for (int q = 0; q < CT; ++q) cur[q] = *(const u32x4_t*)(Wb + ((size_t)(nt0 + q) * NCH) * 512);
    __syncthreads();
    const bf16_t* wa = img + (wrow + lm) * LDW + lk * 8;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int kn = c + 1 < NCH ? c + 1 : c;
#pragma unroll
      for (int q = 0; q < CT; ++q) nxt[q] = *(const u32x4_t*)(Wb + ((size_t)(nt0 + q) * NCH + kn) * 512);
      u32x4_t af[RT];
#pragma unroll
      for (int i = 0; i < RT; ++i) af[i] = *(const u32x4_t*)(wa + i * 16 * LDW + c * 32);
#pragma unroll
      for (int i = 0; i < RT; ++i)
#pragma unroll
        for (int q = 0; q < CT; ++q)
          acc[i][q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, af[i]),
                                                              __builtin_bit_cast(bf16x8_t, cur[q]), acc[i][q], 0, 0, 0);
#pragma unroll
      for (int q = 0; q < CT; ++q) cur[q] = nxt[q];
    }
  }
  __syncthreads();  // every wave is done with the A tile

  // 5. raw x_in rows -> LDS; each lane adds its accumulator elements (+ b2) in place, rounding to bf16
#pragma unroll
  for (int u = 0; u < NR; ++u) {
    const int q = tid + u * 256, r = q / G, g = q - r * G;
    *(u32x4_t*)(img + r * LDW + g * 8) = xr[u];
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < CT; ++q) {
    const int n = (nt0 + q) * 16 + lm;
    const float b2 = p.b2 ? p.b2[n] : 0.f;
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        bf16_t* s = img + (wrow + i * 16 + lk * 4 + e) * LDW + n;
        *s = f2bf(bf2f(*s) + (acc[i][q][e] + b2));
      }
  }
  __syncthreads();

  // 6. x_out rows as 16-byte stores
#pragma unroll
  for (int u = 0; u < NR; ++u) {
    const int q = tid + u * 256, r = q / G, g = q - r * G;
    if (t0 + r < p.L) *(u32x4_t*)(xout + (long long)(t0 + r) * C + g * 8) = *(const u32x4_t*)(img + r * LDW + g * 8);
  }
}

size_t unit_smem(int C, int bm, int dil) { return (size_t)(bm + (CU_TAPS - 1) * dil) * (C + 8) * sizeof(bf16_t); }

template <int C, int MI>
int launch_unit(const qt_codec_resunit_args& a, hipStream_t s) {
  constexpr int BM = 64 * MI;
  const size_t smem = unit_smem(C, BM, a.dil);
  // an image past the 64 KiB a kernel may take without asking (C = 192, dil = 9); per launch: the attribute belongs
  // to the current device
  if (smem > (64u << 10) &&
      hipFuncSetAttribute((const void*)codec_unit_k<C, MI>, hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)unit_smem(C, BM, CU_MAX_DIL)) != hipSuccess)
    return QT_ERR_LAUNCH;
  const long long blocks = (long long)a.B * ((a.L + BM - 1) / BM);
  hipLaunchKernelGGL((codec_unit_k<C, MI>), dim3((unsigned)blocks), dim3(256), smem, s, a);
  return hipGetLastError() == hipSuccess ? QT_OK : QT_ERR_LAUNCH;
}

}  // namespace

// QT_OK when qt_codec_resunit would launch these arguments, else the code it returns
static int unit_check(const qt_codec_resunit_args* a) {
  if (!a) return QT_ERR_ARG;
  if (a->a_dtype != QT_BF16 || a->w_dtype != QT_BF16) return QT_ERR_DTYPE;
  if (a->C != 96 && a->C != 192) return QT_ERR_SHAPE;
  if (a->dil != 1 && a->dil != 3 && a->dil != CU_MAX_DIL) return QT_ERR_SHAPE;  // the staged window reaches 6 x 9 rows back
  if (a->B < 1 || a->L < 1 || (long long)a->B * ((a->L + 63) / 64) > 0x7FFFFFFFLL) return QT_ERR_SHAPE;
  if (!a->x_in || !a->x_out || !a->w1 || !a->w2 || !a->s1_alpha || !a->s1_inv_beta || !a->s2_alpha || !a->s2_inv_beta)
    return QT_ERR_ARG;
  // 16-byte row loads / stores; the two activation buffers must not overlap (tiles read their neighbours' x_in rows)
  if ((reinterpret_cast<uintptr_t>(a->x_in) | reinterpret_cast<uintptr_t>(a->x_out) | reinterpret_cast<uintptr_t>(a->w1) |
       reinterpret_cast<uintptr_t>(a->w2) | reinterpret_cast<uintptr_t>(a->s1_alpha) |
       reinterpret_cast<uintptr_t>(a->s1_inv_beta)) & 15)
    return QT_ERR_ARG;
  const unsigned long long bytes = (unsigned long long)a->B * a->L * a->C * sizeof(bf16_t);
  const uintptr_t xi = reinterpret_cast<uintptr_t>(a->x_in), xo = reinterpret_cast<uintptr_t>(a->x_out);
  if (xi < xo + bytes && xo < xi + bytes) return QT_ERR_ARG;
  return QT_OK;
}

extern "C" int qt_codec_resunit_supported(const qt_codec_resunit_args* a) { return unit_check(a) == QT_OK; }

extern "C" int qt_codec_resunit(const qt_codec_resunit_args* a, void* stream) {
  const int rc = unit_check(a);
  if (rc != QT_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  // rows per block / 64: 128-row tiles for C = 96, 64-row tiles for C = 192 (three workgroups per CU instead of two;
  // tools/codec_unit_bench.py, profiles/codec_resunit_tile_height.txt).  Probe builds: QT_CU_MI forces the other heights.
  if constexpr (kProbe) {
    const int mi = qt_knob("QT_CU_MI", 0);
    if (a->C == 96 && mi == 1) return launch_unit<96, 1>(*a, s);
    if (a->C == 96 && mi == 4) return launch_unit<96, 4>(*a, s);
    if (a->C == 192 && (mi == 2 || mi == 4)) return launch_unit<192, 2>(*a, s);
  }
  if (a->C == 96) return launch_unit<96, 2>(*a, s);
  return launch_unit<192, 1>(*a, s);
}
