// Voice cache (qwen_tts.VoiceCache): the incremental-decode state of one codec.RowCodecStream row moved
// between the stream's slot and a packed, position-independent snapshot block, every job of a call in one launch;
// and the code window of a feed assembled on the device for rows that decode a reference in front of their own codes.
//
// A row's state is its stage histories (region r: bytes [base + row * stride, + bytes)), the positions the
// sliding-window attention can still read at row clock p -- [max(0, p - window), p) of every (K|V, layer, head), one
// contiguous span of the layer's [B][Hkv][Lm][D] fp32 cache -- and the row's device clock.  Block layout, the same for
// every p:  [history r at off_r (16-byte rounded sizes)] [K/V span of segment (kl, h) at kv_off + (kl * Hkv + h) *
// window * D * 4, its first min(p, window) positions used] [clock word].  A segmented copy, bit-exact, no arithmetic:
// 16 B per lane where both sides and the size allow, bytes otherwise (the 4-byte clock on export).
#include "common.h"

namespace {

constexpr int CR_THREADS = 256;
constexpr int CR_UNROLL = 2;
// 8 KiB of a segment per block: a 1.7B snapshot (256 K/V segments of 18 KiB + 21 histories, ~4.7 MiB) is ~800 blocks,
// three per CU, so one adopting row spreads over the whole device
constexpr long long CR_CHUNK = 16ll * CR_THREADS * CR_UNROLL;

struct cr_jobs {
  qt_codec_row_job job[QT_CODEC_ROW_MAX_JOBS];
};

struct cr_layout {
  long long hist_off[QT_CODEC_ROW_MAX_HIST];
  long long kv_off, kv_seg, clock_off, bytes;
};

// grid (chunks of the largest segment, segments, jobs); segments: histories, then (K|V, layer, head) spans, then the
// clock.  Blocks past a shorter segment's end leave.
__global__ __launch_bounds__(CR_THREADS) void codec_row_state_k(const qt_codec_row_table t, const cr_layout lay,
                                                                const cr_jobs jobs) {
  const qt_codec_row_job job = jobs.job[blockIdx.z];
  const int seg = blockIdx.y;
  const long long c0 = (long long)blockIdx.x * CR_CHUNK;
  unsigned char* blk = (unsigned char*)job.block;
  const bool adopt = job.dir == QT_CODEC_ROW_ADOPT;
  unsigned char *live, *snap;
  long long n;
  const int n_kv = 2 * t.n_layers * t.Hkv;
  if (seg < t.n_hist) {
    live = (unsigned char*)t.hist[seg].base + (long long)job.row * t.hist[seg].stride;
    snap = blk + lay.hist_off[seg];
    n = t.hist[seg].bytes;
  } else if (seg < t.n_hist + n_kv) {
    const int r = seg - t.n_hist;
    const int kl = r / t.Hkv, h = r - kl * t.Hkv;
    const int lo = max(job.p - t.window, 0);
    live = (unsigned char*)t.kv[kl] + ((((long long)job.row * t.Hkv + h) * t.Lm + lo) * t.D) * 4;
    snap = blk + lay.kv_off + (long long)r * lay.kv_seg;
    n = (long long)(job.p - lo) * t.D * 4;
  } else {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    if (adopt) {
      t.nf[job.row] = job.p;  // the row's device clock
    } else {
      const unsigned char* s = (const unsigned char*)(t.nf + job.row);
      for (int i = 0; i < 4; ++i) blk[lay.clock_off + i] = s[i];
    }
    return;
  }
  if (c0 >= n) return;
  const unsigned char* src = adopt ? snap : live;
  unsigned char* dst = adopt ? live : snap;
  const long long m = min(n - c0, CR_CHUNK);
  if (!(((uintptr_t)src | (uintptr_t)dst | (uintptr_t)n) & 15)) {
    const u32x4_t* s16 = (const u32x4_t*)(src + c0);
    u32x4_t* d16 = (u32x4_t*)(dst + c0);
    const long long nv = m >> 4;
    u32x4_t v[CR_UNROLL];
#pragma unroll
    for (int u = 0; u < CR_UNROLL; ++u) {
      const long long i = threadIdx.x + u * CR_THREADS;
      if (i < nv) v[u] = s16[i];
    }
#pragma unroll
    for (int u = 0; u < CR_UNROLL; ++u) {
      const long long i = threadIdx.x + u * CR_THREADS;
      if (i < nv) d16[i] = v[u];
    }
  } else {
    for (long long i = c0 + threadIdx.x; i < c0 + m; i += CR_THREADS) dst[i] = src[i];
  }
}

// checks + block layout of the host table; returns the bytes of a snapshot block, or a QT_ERR_* code
long long layout(const qt_codec_row_table* t, cr_layout* lay, long long* max_seg) {
  if (!t) return QT_ERR_ARG;
  if (t->n_hist < 0 || t->n_hist > QT_CODEC_ROW_MAX_HIST || t->n_layers <= 0 || t->n_layers > QT_CODEC_ROW_MAX_LAYERS)
    return QT_ERR_SHAPE;  // too many segments
  if (t->B <= 0 || t->Hkv <= 0 || t->Lm <= 0 || t->D <= 0 || t->window <= 0) return QT_ERR_SHAPE;
  if (2ll * t->n_layers * t->Hkv + t->n_hist + 1 > 65535) return QT_ERR_SHAPE;
  if (!t->nf || ((uintptr_t)t->nf & 3)) return QT_ERR_ARG;
  long long off = 0, mx = 0;
  for (int r = 0; r < t->n_hist; ++r) {
    const qt_row_region& q = t->hist[r];
    if (!q.base) return QT_ERR_ARG;
    if (q.bytes <= 0 || q.bytes > (1ll << 30) || q.stride < q.bytes) return QT_ERR_SHAPE;
    if (lay) lay->hist_off[r] = off;
    off += (q.bytes + 15) & ~15ll;
    mx = q.bytes > mx ? q.bytes : mx;
  }
  for (int kl = 0; kl < 2 * t->n_layers; ++kl)
    if (!t->kv[kl] || ((uintptr_t)t->kv[kl] & 3)) return QT_ERR_ARG;
  const long long seg = (((long long)t->window * t->D * 4) + 15) & ~15ll;
  if (lay) { lay->kv_off = off; lay->kv_seg = seg; }
  off += seg * 2 * t->n_layers * t->Hkv;
  mx = seg > mx ? seg : mx;
  if (lay) lay->clock_off = off;
  off += 16;
  if (lay) lay->bytes = off;
  if (max_seg) *max_seg = mx;
  return off;
}

// out[b][j][:] = pos < 0 ? 0 : pos < R_b ? ref_b[pos] : codes[b][pos - R_b]; one thread per code
__global__ __launch_bounds__(256) void codec_feed_codes_k(const int* __restrict__ pos, const int* const* __restrict__ refs,
                                                         const int* __restrict__ ref_len, const int* __restrict__ codes,
                                                         int B, int n, int F, int Q, int* __restrict__ out) {
  const long long idx = blockIdx.x * 256ll + threadIdx.x;
  if (idx >= (long long)B * n * Q) return;
  const int q = (int)(idx % Q);
  const long long bj = idx / Q;
  const int b = (int)(bj / n);
  const int p = pos[bj];
  const int* ref = refs[b];
  const int R = ref ? max(ref_len[b], 0) : 0;
  int v = 0;
  if (p >= 0) {
    if (p < R) v = ref[(long long)p * Q + q];
    else if (p - R < F) v = codes[((long long)b * F + (p - R)) * Q + q];
  }
  out[idx] = v;
}

}  // namespace

extern "C" long long qt_codec_row_state_bytes(const qt_codec_row_table* t) { return layout(t, nullptr, nullptr); }

extern "C" int qt_codec_row_state(const qt_codec_row_table* t, const qt_codec_row_job* jobs, int n_jobs, void* s) {
  cr_layout lay = {};
  long long mx = 0;
  const long long need = layout(t, &lay, &mx);
  if (need < 0) return (int)need;
  if (n_jobs < 0 || n_jobs > QT_CODEC_ROW_MAX_JOBS) return QT_ERR_SHAPE;
  if (n_jobs == 0) return QT_OK;
  if (!jobs) return QT_ERR_ARG;
  cr_jobs js = {};
  for (int j = 0; j < n_jobs; ++j) {
    const qt_codec_row_job& q = jobs[j];
    if (!q.block || ((uintptr_t)q.block & 15)) return QT_ERR_ARG;
    if (q.dir != QT_CODEC_ROW_ADOPT && q.dir != QT_CODEC_ROW_EXPORT) return QT_ERR_ARG;
    if (q.row < 0 || q.row >= t->B || q.p < 0 || q.p > t->Lm) return QT_ERR_SHAPE;
    const int lo = q.p > t->window ? q.p - t->window : 0;
    if (lo < 0 || q.p - lo > t->window || q.p > t->Lm) return QT_ERR_SHAPE;  // the span leaves the cache / the block
    for (int i = 0; i < j; ++i) {  // two jobs writing the same row / the same block
      if (jobs[i].dir != q.dir) continue;
      if (q.dir == QT_CODEC_ROW_ADOPT ? jobs[i].row == q.row : jobs[i].block == q.block) return QT_ERR_ARG;
    }
    js.job[j] = q;
  }
  const unsigned chunks = (unsigned)((mx + CR_CHUNK - 1) / CR_CHUNK);
  const unsigned segs = (unsigned)(t->n_hist + 2 * t->n_layers * t->Hkv + 1);
  hipLaunchKernelGGL(codec_row_state_k, dim3(chunks, segs, (unsigned)n_jobs), dim3(CR_THREADS), 0, (hipStream_t)s, *t,
                     lay, js);
  return hipGetLastError() == hipSuccess ? QT_OK : QT_ERR_LAUNCH;
}

extern "C" int qt_codec_feed_codes(const int* pos, const int* const* refs, const int* ref_len, const int* codes, int B,
                                   int n, int F, int Q, int* out, void* s) {
  if (B <= 0 || n <= 0 || F <= 0 || Q <= 0) return QT_ERR_SHAPE;
  if (!pos || !refs || !ref_len || !codes || !out) return QT_ERR_ARG;
  if (((uintptr_t)pos | (uintptr_t)ref_len | (uintptr_t)codes | (uintptr_t)out) & 3 || ((uintptr_t)refs & 7))
    return QT_ERR_ARG;
  const long long total = (long long)B * n * Q;
  const long long blocks = (total + 255) / 256;
  if (blocks > 0x7fffffffll) return QT_ERR_SHAPE;
  hipLaunchKernelGGL(codec_feed_codes_k, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)s, pos, refs, ref_len,
                     codes, B, n, F, Q, out);
  return hipGetLastError() == hipSuccess ? QT_OK : QT_ERR_LAUNCH;
}
