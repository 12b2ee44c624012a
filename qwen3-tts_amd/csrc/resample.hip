// PCM output stage (qwen_tts.PcmResampler): a stateful polyphase resampler by up/down with an optional fused s16
// conversion, for up to 16 ragged rows per launch.  The row table travels in the kernel arguments; every count is the
// host's, so the call reads nothing back.  A block owns a tile of one row's outputs: it keeps the phase-major taps and
// the tile's input span in LDS, and each thread sums one output with fmaf over k ascending -- an order that depends on
// m alone, which is what makes the chunking invisible bit for bit.  The first block of a row with new samples also
// writes the row's next history (the last H inputs) into the buffer no block of this launch reads.
#include "common.h"

namespace {

constexpr int kRows = 16;      // rows per launch (64 B each in the argument block)
constexpr int kThreads = 256;
constexpr int kLdsBytes = 48 << 10;

struct RsRow {
  const float* src;
  void* out;
  const float* hist_in;
  float* hist_out;
  long long pos, m0;
  int n, count;
  int tile0;  // first block of this row
  int pad;
};

struct RsArgs {
  RsRow row[kRows];
  const float* table;
  int up, down, half, taps, H, tile, nrows, ntab;
};

// sample k of the row's timeline, by its offset i = k - pos from the first new sample
QT_DEV float rs_sample(const RsRow& r, int H, long long i) {
  if (i >= 0) return i < r.n ? r.src[i] : 0.f;
  return (r.hist_in && i >= -H) ? r.hist_in[H + i] : 0.f;
}

template <int FMT>
__global__ __launch_bounds__(kThreads) void resample_k(const RsArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* tab = lds;            // [up][taps]
  float* xs = lds + a.ntab;    // the tile's input span (ntab is a multiple of 4)
  int ri = 0;
  for (int i = 1; i < a.nrows; ++i)
    if ((int)blockIdx.x >= a.row[i].tile0) ri = i;
  const RsRow& r = a.row[ri];
  const int t = blockIdx.x - r.tile0, tid = threadIdx.x;
  const int H = a.H, T = a.taps;

  if (t == 0 && r.n > 0) {  // next history: the last H samples of history + new (hist_out != hist_in)
    for (int j = tid; j < H; j += kThreads) r.hist_out[j] = rs_sample(r, H, (long long)r.n - H + j);
  }
  const int o0 = t * a.tile;
  const int cnt = min(a.tile, r.count - o0);
  if (cnt <= 0) return;  // block-uniform

  for (int j = tid; j < a.up * T; j += kThreads) tab[j] = a.table[j];
  const long long mt = r.m0 + o0;
  const long long k_first = (mt * a.down + a.half) / a.up - T + 1;
  const long long k_last = ((mt + cnt - 1) * a.down + a.half) / a.up;
  const int span = (int)(k_last - k_first) + 1;
  const long long i0 = k_first - r.pos;
  for (int j = tid; j < span; j += kThreads) xs[j] = rs_sample(r, H, i0 + j);
  __syncthreads();

  if (tid >= cnt) return;
  const long long c = (mt + tid) * a.down + a.half;
  const long long k_hi = c / a.up;
  const float* h = tab + (int)(c - k_hi * a.up) * T;  // the output's phase
  const float* x = xs + (int)(k_hi - k_first);        // x[-j] = input k_hi - j, under tap h[j]
  float acc = 0.f;
  for (int j = T - 1; j >= 0; --j) acc = fmaf(x[-j], h[j], acc);
  if (FMT == QT_PCM_S16)
    ((short*)r.out)[o0 + tid] = (short)rintf(fminf(fmaxf(acc, -1.f), 1.f) * 32767.f);
  else
    ((float*)r.out)[o0 + tid] = acc;
}

long long ceil_div(long long a, long long b) { return (a + b - 1) / b; }
long long floor_div(long long a, long long b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

}  // namespace

extern "C" int qt_resample(const qt_resample_args* a, void* s) {
  if (!a || !a->table || !a->rows) return QT_ERR_ARG;
  if (a->format != QT_PCM_F32 && a->format != QT_PCM_S16) return QT_ERR_DTYPE;
  const int up = a->up, down = a->down, half = a->half, T = a->taps, H = a->H;
  if (up < 1 || up > 160 || down < 1 || down > 160 || half < 0 || a->B <= 0) return QT_ERR_SHAPE;
  if (T != (2 * half + up) / up || H < T) return QT_ERR_SHAPE;
  const int ntab = (up * T + 3) & ~3;
  // the largest tile whose input span fits beside the taps
  int tile = kThreads;
  auto span_max = [&](int tl) { return (long long)(tl - 1) * down / up + 1 + T; };
  while (tile > 1 && (ntab + span_max(tile)) * 4 > kLdsBytes) tile >>= 1;
  if ((ntab + span_max(tile)) * 4 > kLdsBytes) return QT_ERR_SHAPE;
  const size_t lds = (size_t)(ntab + span_max(tile)) * 4;

  for (int b = 0; b < a->B; ++b) {  // every row is checked before the first launch
    const qt_resample_row& r = a->rows[b];
    if (r.n < 0 || r.count < 0 || r.pos < 0 || r.m0 < 0 || r.pos > (1ll << 53) || r.m0 > (1ll << 53)) return QT_ERR_ARG;
    const long long nt = r.pos + r.n, top = ceil_div(nt * up, down);
    long long ready = r.flush ? top : floor_div(nt * up - 1 - half, down) + 1;
    if (ready > top) ready = top;
    if (r.count != (ready > r.m0 ? ready - r.m0 : 0)) return QT_ERR_ARG;
    if ((r.n > 0 && (!r.src || !r.hist_out || r.hist_out == r.hist_in)) || (r.count > 0 && !r.out)) return QT_ERR_ARG;
    if (r.count > 0 && (r.m0 * down + half) / up - T + 1 < r.pos - H) return QT_ERR_ARG;
    if (((uintptr_t)r.src | (uintptr_t)r.hist_in | (uintptr_t)r.hist_out) & 3) return QT_ERR_ARG;
    if ((uintptr_t)r.out & (a->format == QT_PCM_S16 ? 1 : 3)) return QT_ERR_ARG;
  }
  for (int b0 = 0; b0 < a->B; b0 += kRows) {
    RsArgs k;
    k.table = a->table;
    k.up = up, k.down = down, k.half = half, k.taps = T, k.H = H, k.tile = tile, k.ntab = ntab, k.nrows = 0;
    long long blocks = 0;
    for (int b = b0; b < a->B && b < b0 + kRows; ++b) {
      const qt_resample_row& r = a->rows[b];
      if (r.n == 0 && r.count == 0) continue;  // nothing to write for this row
      RsRow& d = k.row[k.nrows++];
      d.src = r.src, d.out = r.out, d.hist_in = r.hist_in, d.hist_out = r.hist_out;
      d.pos = r.pos, d.m0 = r.m0, d.n = r.n, d.count = r.count, d.tile0 = (int)blocks, d.pad = 0;
      blocks += r.count > 0 ? (r.count + tile - 1) / tile : 1;
      if (blocks > 0x7fffffffll) return QT_ERR_SHAPE;
    }
    if (!k.nrows) continue;
    for (int i = k.nrows; i < kRows; ++i) k.row[i] = RsRow{nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 0, 0x7fffffff, 0};
    if (a->format == QT_PCM_S16)
      hipLaunchKernelGGL(resample_k<QT_PCM_S16>, dim3((unsigned)blocks), dim3(kThreads), lds, (hipStream_t)s, k);
    else
      hipLaunchKernelGGL(resample_k<QT_PCM_F32>, dim3((unsigned)blocks), dim3(kThreads), lds, (hipStream_t)s, k);
    if (hipGetLastError() != hipSuccess) return QT_ERR_LAUNCH;
  }
  return 0;
}
