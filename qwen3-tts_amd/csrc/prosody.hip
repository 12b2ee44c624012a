// Pitch and volume stage (qwen_tts.PcmProsody): a stateful polyphase resampler in which every row has its
// own ratio, taps and gain, with a look-ahead peak limiter on the rows that ask for one, for up to 16 ragged rows per
// launch.  The row table travels in the kernel arguments; every count is the host's, so the call reads nothing back.
// A block owns a tile of 256 outputs of one row: it keeps the row's phase-major taps and the tile's input span in LDS,
// and a thread sums an output with fmaf over k ascending and multiplies by the gain -- an order that depends on m
// alone.  A limited tile recomputes v over its outputs -127 .. +127 from the inputs (the same bits, by that rule), so
// the state is input history alone; the sliding minimum and the sliding sum over 128 are seven doubling steps each
// between two LDS arrays, on integers, exact in any order.  The first block of a row with new samples also writes the
// row's next history into the buffer no block of this launch reads.
#include "common.h"

namespace {

constexpr int kRows = 16;      // rows per launch (112 B each in the argument block)
constexpr int kThreads = 256;
constexpr int kTile = 256;     // outputs per block
constexpr int kLA = 128;       // limiter window
constexpr int kH = QT_PROSODY_HIST;
constexpr int kTabMax = 4200;  // floats of a row's taps
constexpr int kSpanMax = 2128; // input samples under a limited tile: 509 * down / up + 1 + taps
constexpr int kNv = kTile + 2 * (kLA - 1);  // v values under a limited tile
constexpr int kW = 512;        // entries of the limiter's arrays that are computed ...
constexpr int kWPad = kW + kLA;  // ... and with the constant pad a doubling step may read
constexpr unsigned kOne = 1u << 24;
static_assert(kNv <= kW && kTile == kThreads, "tile layout");

struct PrRow {
  const float* src;
  float* out;
  const float* hin;
  float* hout;
  const float* table;
  long long pos, m0;
  long long mbeg, mend;  // the signal's outputs: [mbeg, mend)
  int n, count, up, down, half, taps, limited;
  int tile0;  // first block of this row
  float g;
  int pad;
};

struct PrArgs {
  PrRow row[kRows];
  int nrows, pad;
};

// sample k of the row's timeline, by its offset i = k - pos from the first new sample
QT_DEV float pr_sample(const PrRow& r, long long i) {
  if (i >= 0) return i < r.n ? r.src[i] : 0.f;
  return (r.hin && i >= -kH) ? r.hin[kH + i] : 0.f;
}

// v[m] from the staged taps and inputs (xs[0] = input k_first)
QT_DEV float pr_v(const PrRow& r, const float* tab, const float* xs, long long k_first, long long m) {
  float acc;
  if (r.up == r.down) {
    acc = xs[(int)(m - k_first)];
  } else {
    const long long c = m * r.down + r.half;
    const long long k_hi = c / r.up;
    const float* h = tab + (int)(c - k_hi * r.up) * r.taps;  // the output's phase
    const float* x = xs + (int)(k_hi - k_first);             // x[-j] = input k_hi - j, under tap h[j]
    acc = 0.f;
    for (int j = r.taps - 1; j >= 0; --j) acc = fmaf(x[-j], h[j], acc);
  }
  return __fmul_rn(r.g, acc);
}

__global__ __launch_bounds__(kThreads) void prosody_k(const PrArgs a) {
  __shared__ float tab[kTabMax];
  __shared__ float xs[kSpanMax];
  __shared__ float vs[kW];
  __shared__ unsigned wa[kWPad], wb[kWPad];
  int ri = 0;
  for (int i = 1; i < a.nrows; ++i)
    if ((int)blockIdx.x >= a.row[i].tile0) ri = i;
  const PrRow& r = a.row[ri];
  const int t = blockIdx.x - r.tile0, tid = threadIdx.x;

  if (t == 0 && r.n > 0) {  // next history: the last kH samples of history + new (hout != hin)
    for (int j = tid; j < kH; j += kThreads) r.hout[j] = pr_sample(r, (long long)r.n - kH + j);
  }
  const int o0 = t * kTile;
  const int cnt = min(kTile, r.count - o0);
  if (cnt <= 0) return;  // block-uniform

  const bool lim = r.limited != 0;
  const long long mt = r.m0 + o0;
  const long long wl = mt - (kLA - 1);  // the output under entry 0 of the limiter's arrays
  const long long ml = !lim ? mt : wl > r.mbeg ? wl : r.mbeg;
  const long long me = mt + cnt - 1 + (kLA - 1);
  const long long mh = !lim ? mt + cnt - 1 : me < r.mend - 1 ? me : r.mend - 1;  // v is computed on [ml, mh]
  const long long k_first = (ml * r.down + r.half) / r.up - r.taps + 1;
  const long long k_last = (mh * r.down + r.half) / r.up;
  const int span = (int)(k_last - k_first) + 1;
  if (span > kSpanMax) return;  // (the host refuses such a ratio)
  if (r.up != r.down)
    for (int j = tid; j < r.up * r.taps; j += kThreads) tab[j] = r.table[j];
  const long long i0 = k_first - r.pos;
  for (int j = tid; j < span; j += kThreads) xs[j] = pr_sample(r, i0 + j);
  __syncthreads();

  if (!lim) {
    if (tid < cnt) r.out[o0 + tid] = pr_v(r, tab, xs, k_first, mt + tid);
    return;
  }
  for (int i = tid; i < kWPad; i += kThreads) {
    unsigned q = kOne;  // outside the signal, and where |v| <= 1
    if (i < kW) {
      const long long m = wl + i;
      float v = 0.f;
      if (m >= ml && m <= mh) {
        v = pr_v(r, tab, xs, k_first, m);
        const float av = fabsf(v);
        if (av > 1.f) q = (unsigned)(__fdiv_rn(1.f, av) * 16777216.f);
      }
      vs[i] = v;
    }
    wa[i] = q;
    wb[i] = kOne;
  }
  // entry i: min over [i, i + 128) after the first seven steps, then the sum of those over [i, i + 128)
  unsigned *s = wa, *d = wb;
#pragma unroll
  for (int w = 1; w < kLA; w <<= 1) {
    __syncthreads();
    for (int i = tid; i < kW; i += kThreads) d[i] = min(s[i], s[i + w]);
    unsigned* x = s;
    s = d, d = x;
  }
#pragma unroll
  for (int w = 1; w < kLA; w <<= 1) {
    __syncthreads();
    for (int i = tid; i < kW; i += kThreads) d[i] = s[i] + s[i + w];
    unsigned* x = s;
    s = d, d = x;
  }
  __syncthreads();
  if (tid < cnt) {  // output mt + tid: v at entry tid + 127, sm = the sum at entry tid (outputs m - 127 .. m)
    const float v = vs[tid + kLA - 1];
    const float av = fabsf(v);
    const float rr = av > 1.f ? __fdiv_rn(1.f, av) : 1.f;
    const float sc = fminf((float)s[tid] * 0x1p-31f, rr);
    r.out[o0 + tid] = __fmul_rn(v, sc);
  }
}

long long ceil_div(long long a, long long b) { return (a + b - 1) / b; }
long long floor_div(long long a, long long b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

}  // namespace

extern "C" int qt_prosody(const qt_prosody_args* a, void* s) {
  if (!a || !a->rows) return QT_ERR_ARG;
  if (a->B <= 0) return QT_ERR_SHAPE;
  const long long kMaxPos = 1ll << 53;
  for (int b = 0; b < a->B; ++b) {  // every row is checked before the first launch
    const qt_prosody_row& r = a->rows[b];
    const int up = r.up, down = r.down, half = r.half, T = r.taps;
    if (up < 1 || up > 200 || down < 1 || down > 200 || (up == down && up != 1)) return QT_ERR_SHAPE;
    if (half != 10 * (up > down ? up : down) || T != (2 * half + up) / up || up * T > kTabMax) return QT_ERR_SHAPE;
    if (((long long)(kNv - 1) * down + up - 1) / up + T > kSpanMax) return QT_ERR_SHAPE;
    if (r.n < 0 || r.count < 0 || r.pos0 < 0 || r.pos0 % down || r.pos < r.pos0 || r.pos > kMaxPos) return QT_ERR_ARG;
    const long long mbeg = r.pos0 / down * up;
    if (r.m0 < mbeg || r.m0 > kMaxPos || r.cap > kMaxPos) return QT_ERR_ARG;
    const long long nt = r.pos + r.n, top = ceil_div(nt * up, down);
    long long ready;
    if (r.flush) {
      ready = (r.cap >= 0 && mbeg + r.cap < top) ? mbeg + r.cap : top;
    } else {
      ready = up == down ? nt : floor_div(nt * up - 1 - half, down) + 1;
      if (ready > top) ready = top;
      if (r.limited) ready -= kLA - 1;
    }
    if (r.count != (ready > r.m0 ? ready - r.m0 : 0)) return QT_ERR_ARG;
    if (!r.table || (r.n > 0 && (!r.src || !r.state_out || r.state_out == r.state_in)) || (r.count > 0 && !r.out))
      return QT_ERR_ARG;
    if (r.pos > r.pos0 && !r.state_in) return QT_ERR_ARG;
    if (((uintptr_t)r.src | (uintptr_t)r.out | (uintptr_t)r.state_in | (uintptr_t)r.state_out | (uintptr_t)r.table) & 3)
      return QT_ERR_ARG;
    if (r.count > 0) {  // the first v the row computes must not reach behind the history
      long long ml = r.limited ? r.m0 - (kLA - 1) : r.m0;
      if (ml < mbeg) ml = mbeg;
      if ((ml * down + half) / up - T + 1 < r.pos - kH && r.pos - kH > r.pos0) return QT_ERR_ARG;
    }
  }
  for (int b0 = 0; b0 < a->B; b0 += kRows) {
    PrArgs k;
    k.nrows = 0, k.pad = 0;
    long long blocks = 0;
    for (int b = b0; b < a->B && b < b0 + kRows; ++b) {
      const qt_prosody_row& r = a->rows[b];
      if (r.n == 0 && r.count == 0) continue;  // nothing to write for this row
      PrRow& d = k.row[k.nrows++];
      d.src = r.src, d.out = r.out, d.hin = r.state_in, d.hout = r.state_out, d.table = r.table;
      d.pos = r.pos, d.m0 = r.m0, d.mbeg = r.pos0 / r.down * r.up;
      d.mend = ceil_div((r.pos + r.n) * r.up, r.down);
      d.n = r.n, d.count = r.count, d.up = r.up, d.down = r.down, d.half = r.half, d.taps = r.taps;
      d.limited = r.limited ? 1 : 0, d.tile0 = (int)blocks, d.g = r.gain, d.pad = 0;
      blocks += r.count > 0 ? (r.count + kTile - 1) / kTile : 1;
    }
    if (!k.nrows) continue;
    for (int i = k.nrows; i < kRows; ++i) {
      k.row[i] = PrRow{};
      k.row[i].tile0 = 0x7fffffff;
    }
    hipLaunchKernelGGL(prosody_k, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)s, k);
    if (hipGetLastError() != hipSuccess) return QT_ERR_LAUNCH;
  }
  return 0;
}
