// Speaking-rate stage (qwen_tts.PcmTempo): a stateful WSOLA time-stretch with an integer-exact search, for
// up to 16 ragged rows per launch.  The row table travels in the kernel arguments; every count is the host's, so the
// call reads nothing back.  One workgroup owns a row and walks its pending blocks in order -- block j's overlap-add
// starts where block j-1's segment would continue, so a row is a chain through `seg`.  The row's input span is staged
// in LDS in tiles of up to kSpan samples, as fp32 beside a 16-bit copy (q + 32768, two per dword).
//
// Per block the 256 candidates go one to a thread and the absolute-difference sums run on the 16-bit copy with
// v_sad_u16, two samples per instruction.  A workgroup alone on its CU is bound by VALU issue and LDS read rate, so
// the loop is kept at one LDS dword and two VALU instructions per sad:
//  * wave w takes the candidates 4 * lane + w, so whether a window starts on an odd sample is the same for a whole
//    wave.  An odd wave starts one sample early and compares against the continuation window moved the same way: no
//    realignment of the candidate's dwords, one dword more, with the two outer half-dwords masked on both sides.
//  * a lane's dwords are then 8-byte aligned up to one dword, again per wave, and are read 8 bytes at a time (lane
//    stride 8 bytes: every bank of a 32-lane half once); the loop is instantiated for both alignments.
//  * the continuation window is the same for all candidates: a wave keeps it in registers, dword k in lane k % 64, and
//    passes it round with v_readlane instead of reading it from LDS per sad.
// The candidate is picked by two DPP wave minima (score, then the tie rank among the lanes that hold it) and one LDS
// exchange between the four waves.  The same workgroup writes the row's next state at the end into the buffer it does
// not read.
#include "common.h"

namespace {

constexpr int kRows = 16;      // rows per launch (80 B each in the argument block)
constexpr int kThreads = 256;  // = candidates per block
constexpr int kHS = 240, kL = 480, kDlo = -128, kDhi = 128, kH = 1024;
constexpr int kNw = kL / 2 + 1;          // dwords of a compared window (one more for a window on an odd sample)
constexpr int kTr = (kNw + 63) / 64;     // registers of a lane that hold the continuation window
constexpr int kPad = 2;                  // samples in front of the 16-bit copy (an odd window starts one early)
constexpr int kSpan = 6144;    // samples of a tile: 24 KiB fp32 + 12 KiB of 16-bit
static_assert(kDhi - kDlo == kThreads, "one candidate per thread");

struct TpState {
  float hist[kH];
  long long seg;
};
static_assert(sizeof(TpState) == QT_TEMPO_STATE_BYTES, "state layout");

struct TpRow {
  const float* src;
  float* out;
  const TpState* state_in;
  TpState* state_out;
  long long pos, j0, block0, a0;  // a0 = a(block0)
  int n, count, S, flush;
};

struct TpArgs {
  TpRow row[kRows];
  const float* window;
};

__host__ __device__ inline long long tp_a(long long j, int S) { return j * kHS * S / 100; }
__host__ __device__ inline int tp_need0(int S) {
  const int m = (kHS - 1) * S / 100 + 1;
  return m > kHS ? m : kHS;
}
// one past the last input position block j reads, and the first one it can read
__host__ __device__ inline long long tp_need(long long j, long long block0, long long a0, int S) {
  if (j == block0) return a0 + tp_need0(S);
  const long long x = tp_a(j, S) + kDhi - 1, y = tp_a(j - 1, S) + kDhi - 1 + kHS;
  return (x > y ? x : y) + kL;
}
__host__ __device__ inline long long tp_low(long long j, long long block0, long long a0, int S) {
  if (j == block0) return a0 + kDlo;  // (not above block0 + 1's)
  const long long x = tp_a(j, S), y = tp_a(j - 1, S) + kHS;
  return (x < y ? x : y) + kDlo;
}

// sample k of the row's timeline
QT_DEV float tp_sample(const TpRow& r, long long k) {
  const long long i = k - r.pos;
  if (i >= 0) return i < r.n ? r.src[i] : 0.f;
  if (k < r.a0 || i < -kH || !r.state_in) return 0.f;
  return r.state_in->hist[kH + i];
}

QT_DEV unsigned tp_wave_min(unsigned v) {  // wave-uniform: DPP inside each 16-lane row, then the four rows
  v = min(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false));   // quad_perm [1,0,3,2]
  v = min(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false));   // quad_perm [2,3,0,1]
  v = min(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, false));  // row_half_mirror
  v = min(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, false));  // row_mirror
  return min(min((unsigned)__builtin_amdgcn_readlane((int)v, 0), (unsigned)__builtin_amdgcn_readlane((int)v, 16)),
             min((unsigned)__builtin_amdgcn_readlane((int)v, 32), (unsigned)__builtin_amdgcn_readlane((int)v, 48)));
}

// sum over the window's kNw dwords of |candidate - continuation|, two samples per dword.  cp: the lane's 8-byte
// aligned dwords, of which the window starts at dword OFF; tr: the wave's continuation window (dword m in lane m % 64
// of tr[m / 64]), already masked; first / last: masks of the candidate's outer dwords.
template <int OFF>
QT_DEV unsigned tp_sad(const uint2* cp, const unsigned (&tr)[kTr], unsigned first, unsigned last) {
  unsigned acc = 0;
#pragma unroll
  for (int p = 0; p < (kNw + OFF + 1) / 2; ++p) {
    const uint2 v = cp[p];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int m = 2 * p + h - OFF;
      if (m >= 0 && m < kNw) {
        unsigned c = h ? v.y : v.x;
        if (m == 0) c &= first;
        if (m == kNw - 1) c &= last;
        acc = __builtin_amdgcn_sad_u16(c, (unsigned)__builtin_amdgcn_readlane((int)tr[m >> 6], m & 63), acc);
      }
    }
  }
  return acc;
}

__global__ __launch_bounds__(kThreads) void tempo_k(const TpArgs a) {
  __shared__ float xf[kSpan];
  // the 16-bit copy behind kPad samples, read a dword or two at a time (slack for the reads past a window's end)
  __shared__ __attribute__((aligned(16))) unsigned xw[(kSpan + kPad) / 2 + 8];
  __shared__ unsigned long long red[2][kThreads / 64];
  unsigned short* xq = (unsigned short*)xw + kPad;
  const TpRow& r = a.row[blockIdx.x];
  const int tid = threadIdx.x;

  if (r.S == 100) {  // verbatim
    for (int i = tid; i < r.count; i += kThreads) r.out[i] = r.src[i];
    return;
  }
  const int S = r.S;
  const long long j1 = r.j0 + (r.count + kHS - 1) / kHS;
  const float w0 = tid < kHS ? a.window[tid] : 0.f, w1 = tid < kHS ? a.window[kHS + tid] : 0.f;
  long long seg = (r.j0 > r.block0 && r.state_in) ? r.state_in->seg : r.a0;
  int par = 0;

  for (long long j = r.j0; j < j1;) {
    const long long lo = tp_low(j, r.block0, r.a0, S);
    long long je = j + 1;
    while (je < j1 && tp_need(je, r.block0, r.a0, S) - lo <= kSpan) ++je;
    const int span = (int)(tp_need(je - 1, r.block0, r.a0, S) - lo);  // <= kSpan: one block alone spans < 1500
    __syncthreads();  // the previous tile's last reads
    for (int i = tid; i < span; i += kThreads) {
      const float v = tp_sample(r, lo + i);
      xf[i] = v;
      xq[i] = (unsigned short)((int)rintf(fminf(fmaxf(v, -1.f), 1.f) * 32767.f) + 32768);
    }
    __syncthreads();

    for (; j < je; ++j) {
      const int ob = (int)(j - r.j0) * kHS;
      const int cut = min(kHS, r.count - ob);
      if (j == r.block0) {
        seg = r.a0;
        if (tid < cut) r.out[ob + tid] = xf[(int)(r.a0 - lo) + tid];
        continue;
      }
      const long long aj = tp_a(j, S), t = seg + kHS;
      const int lane = tid & 63, wv = tid >> 6;
      const int d = kDlo + 4 * lane + wv;
      const int ts = (int)(t - lo);
      const int cs = (int)(aj - lo) + d + kPad;                   // the candidate's first sample in the padded copy
      const int odd = __builtin_amdgcn_readfirstlane(cs & 1);     // (the same for the wave)
      const int cd = (cs - odd) >> 1;                             // its first dword: wave's base + 2 * lane
      const int off = __builtin_amdgcn_readfirstlane(cd & 1);
      const unsigned first = odd ? 0xFFFF0000u : ~0u, last = odd ? 0x0000FFFFu : 0u;
      const int u = ts + kPad - odd;
      const unsigned* tw = xw + (u >> 1);
      const unsigned tsh = (u & 1) * 16;
      unsigned tr[kTr];
#pragma unroll
      for (int q = 0; q < kTr; ++q) {
        const int k = lane + 64 * q;
        unsigned v = k < kNw ? __builtin_amdgcn_alignbit(tw[k + 1], tw[k], tsh) : 0u;
        if (k == 0) v &= first;
        if (k == kNw - 1) v &= last;
        tr[q] = v;
      }
      const uint2* cp = (const uint2*)(xw + (cd - off));
      const unsigned acc = off ? tp_sad<1>(cp, tr, first, last) : tp_sad<0>(cp, tr, first, last);
      // smallest score, then smallest |d|, then the negative d; a candidate before the row's start never wins
      const unsigned score = aj + d < r.a0 ? ~0u : acc;
      const unsigned rank = d < 0 ? (unsigned)(-2 * d - 1) : (unsigned)(2 * d);
      const unsigned smin = tp_wave_min(score);
      const unsigned rmin = tp_wave_min(score == smin ? rank : 0xFFFFu);
      if (lane == 0) red[par][wv] = ((unsigned long long)smin << 16) | rmin;
      __syncthreads();
      unsigned long long key = red[par][0];
#pragma unroll
      for (int w = 1; w < kThreads / 64; ++w) key = red[par][w] < key ? red[par][w] : key;
      par ^= 1;
      const int rk = (int)(key & 0xFFFF);
      seg = aj + ((rk & 1) ? -((rk + 1) >> 1) : (rk >> 1));
      if (tid < cut)
        r.out[ob + tid] = __fmaf_rn(w0, xf[(int)(seg - lo) + tid], __fmul_rn(w1, xf[ts + tid]));
    }
  }

  if (r.n > 0) {  // the next call's state: the last kH inputs and the last block's seg
    const long long k0 = r.pos + r.n - kH;
    for (int i = tid; i < kH; i += kThreads) r.state_out->hist[i] = tp_sample(r, k0 + i);
    if (tid == 0) r.state_out->seg = seg;
  }
}

}  // namespace

extern "C" int qt_tempo(const qt_tempo_args* a, void* s) {
  if (!a || !a->window || !a->rows || ((uintptr_t)a->window & 3)) return QT_ERR_ARG;
  if (a->B <= 0) return QT_ERR_SHAPE;
  const long long kMaxPos = 1ll << 53, kMaxBlock = 1ll << 40;
  for (int b = 0; b < a->B; ++b) {  // every row is checked before the first launch
    const qt_tempo_row& r = a->rows[b];
    if (r.S < 50 || r.S > 200 || r.n < 0 || r.count < 0) return QT_ERR_ARG;
    if (r.block0 < 0 || r.block0 % 5 || r.block0 > kMaxBlock || r.j0 < r.block0 || r.j0 > kMaxBlock) return QT_ERR_ARG;
    const long long a0 = tp_a(r.block0, r.S);
    if (r.pos < a0 || r.pos > kMaxPos) return QT_ERR_ARG;
    if (((uintptr_t)r.src | (uintptr_t)r.out) & 3) return QT_ERR_ARG;
    if ((r.n > 0 && !r.src) || (r.count > 0 && !r.out)) return QT_ERR_ARG;
    if (r.S == 100) {
      if (r.count != r.n) return QT_ERR_ARG;
      continue;
    }
    const long long n_rel = r.pos + r.n - a0, jr0 = r.j0 - r.block0;
    long long want;
    if (r.flush) {
      want = (100 * n_rel + r.S - 1) / r.S - kHS * jr0;
    } else {
      long long j = (n_rel - (kDhi - 1 + kHS + kL)) * 100 / (kHS * r.S);
      if (j < 0) j = 0;
      while (tp_need(j, 0, 0, r.S) <= n_rel) ++j;
      want = kHS * (j - jr0);
    }
    if (r.count != (want > 0 ? want : 0)) return QT_ERR_ARG;
    if (((uintptr_t)r.state_in | (uintptr_t)r.state_out) & 7) return QT_ERR_ARG;
    if (r.n > 0 && (!r.state_out || r.state_out == r.state_in)) return QT_ERR_ARG;
    if (r.pos > a0 && !r.state_in) return QT_ERR_ARG;
    // the first pending block must not reach behind the history
    if (r.count > 0 && tp_low(r.j0, r.block0, a0, r.S) < r.pos - kH && r.pos - kH > a0) return QT_ERR_ARG;
  }
  for (int b0 = 0; b0 < a->B; b0 += kRows) {
    TpArgs k;
    k.window = a->window;
    int nrows = 0;
    for (int b = b0; b < a->B && b < b0 + kRows; ++b) {
      const qt_tempo_row& r = a->rows[b];
      if (r.count == 0 && (r.n == 0 || r.S == 100)) continue;  // nothing to write for this row
      TpRow& d = k.row[nrows++];
      d.src = r.src, d.out = r.out, d.state_in = (const TpState*)r.state_in, d.state_out = (TpState*)r.state_out;
      d.pos = r.pos, d.j0 = r.j0, d.block0 = r.block0, d.a0 = tp_a(r.block0, r.S);
      d.n = r.n, d.count = r.count, d.S = r.S, d.flush = r.flush;
    }
    if (!nrows) continue;
    for (int i = nrows; i < kRows; ++i) k.row[i] = TpRow{nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 0, 0, 0, 100, 0};
    hipLaunchKernelGGL(tempo_k, dim3((unsigned)nrows), dim3(kThreads), 0, (hipStream_t)s, k);
    if (hipGetLastError() != hipSuccess) return QT_ERR_LAUNCH;
  }
  return 0;
}
