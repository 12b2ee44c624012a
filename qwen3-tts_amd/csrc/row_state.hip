// Held frames (TalkerEngine._run_frame_held): the per-row decode state of a subset of batch rows saved
// to, or restored from, a stash, every region of every selected row in one launch.  A region is one piece of
// per-row state {base, row stride, bytes per row}; row b of region r is bytes [base + b * stride, + bytes) on the
// live side and [stash + b * stash_row_bytes + off_r, + bytes) in the stash, off_r = the 16-byte-rounded sizes of the
// regions before it.  A segmented copy, bit-exact, no arithmetic: 16 B per lane where the region's base, stride and
// size allow, bytes otherwise (the 1-byte finished flag, the 4-byte counters).  The table and the row mask are kernel
// arguments: nothing is uploaded per call.
#include "common.h"

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_UNROLL = 4;
constexpr long long RS_CHUNK = 16ll * RS_THREADS * RS_UNROLL;  // bytes of a region row per block

struct rs_table {
  qt_row_region reg[QT_ROW_STATE_MAX_REGIONS];
  long long off[QT_ROW_STATE_MAX_REGIONS];  // region's offset in a stash row (16-byte aligned)
  unsigned vec;                             // bit r: region r takes the 16-byte path
};

// grid (chunks of the largest region, regions, selected rows); blocks past a smaller region's end leave
__global__ __launch_bounds__(RS_THREADS) void row_state_k(const rs_table t, unsigned char* __restrict__ stash,
                                                          long long stash_row_bytes, unsigned long long mask,
                                                          int restore) {
  const int r = blockIdx.y;
  const long long c0 = (long long)blockIdx.x * RS_CHUNK;
  const long long n = t.reg[r].bytes;
  if (c0 >= n) return;
  // the blockIdx.z-th set bit of the mask: the batch row (the host launches popcount(mask) rows)
  unsigned long long m = mask;
  for (int k = 0; k < (int)blockIdx.z; ++k) m &= m - 1;
  const int b = __ffsll((long long)m) - 1;
  unsigned char* live = (unsigned char*)t.reg[r].base + (long long)b * t.reg[r].stride;
  unsigned char* st = stash + (long long)b * stash_row_bytes + t.off[r];
  const unsigned char* src = restore ? st : live;
  unsigned char* dst = restore ? live : st;
  if ((t.vec >> r) & 1u) {
    const u32x4_t* s16 = (const u32x4_t*)(src + c0);
    u32x4_t* d16 = (u32x4_t*)(dst + c0);
    const long long nv = (min(n - c0, RS_CHUNK)) >> 4;
    u32x4_t v[RS_UNROLL];
#pragma unroll
    for (int u = 0; u < RS_UNROLL; ++u) {
      const long long i = threadIdx.x + u * RS_THREADS;
      if (i < nv) v[u] = s16[i];
    }
#pragma unroll
    for (int u = 0; u < RS_UNROLL; ++u) {
      const long long i = threadIdx.x + u * RS_THREADS;
      if (i < nv) d16[i] = v[u];
    }
  } else {
    const long long end = min(n, c0 + RS_CHUNK);
    for (long long i = c0 + threadIdx.x; i < end; i += RS_THREADS) dst[i] = src[i];
  }
}

// checks + stash layout of the host table; returns the bytes a stash row needs, or a QT_ERR_* code
long long layout(const qt_row_state_args* a, rs_table* t, long long* max_bytes) {
  if (!a) return QT_ERR_ARG;
  if (a->n_regions <= 0 || a->n_regions > QT_ROW_STATE_MAX_REGIONS || a->B < 1 || a->B > 64) return QT_ERR_SHAPE;
  long long off = 0, mx = 0;
  unsigned vec = 0;
  for (int r = 0; r < a->n_regions; ++r) {
    const qt_row_region& q = a->regions[r];
    if (!q.base) return QT_ERR_ARG;
    if (q.bytes <= 0 || q.bytes > (1ll << 30) || q.stride < q.bytes) return QT_ERR_SHAPE;
    if (!(((uintptr_t)q.base | (uintptr_t)q.stride | (uintptr_t)q.bytes) & 15)) vec |= 1u << r;
    if (t) { t->reg[r] = q; t->off[r] = off; }
    off += (q.bytes + 15) & ~15ll;
    mx = q.bytes > mx ? q.bytes : mx;
  }
  if (t) t->vec = vec;
  if (max_bytes) *max_bytes = mx;
  return off;
}

}  // namespace

extern "C" long long qt_row_state_row_bytes(const qt_row_state_args* a) { return layout(a, nullptr, nullptr); }

extern "C" int qt_row_state(const qt_row_state_args* a, void* s) {
  rs_table t = {};
  long long mx = 0;
  const long long need = layout(a, &t, &mx);
  if (need < 0) return (int)need;
  if (a->dir != QT_ROW_SAVE && a->dir != QT_ROW_RESTORE) return QT_ERR_ARG;
  if (!a->stash || ((uintptr_t)a->stash & 15)) return QT_ERR_ARG;
  if (a->stash_row_bytes < need || (a->stash_row_bytes & 15)) return QT_ERR_SHAPE;
  if (a->B < 64 && (a->mask >> a->B)) return QT_ERR_SHAPE;  // a row outside [0, B)
  if (!a->mask) return QT_OK;
  const unsigned rows = (unsigned)__builtin_popcountll(a->mask);
  const unsigned chunks = (unsigned)((mx + RS_CHUNK - 1) / RS_CHUNK);
  hipLaunchKernelGGL(row_state_k, dim3(chunks, (unsigned)a->n_regions, rows), dim3(RS_THREADS), 0, (hipStream_t)s, t,
                     (unsigned char*)a->stash, a->stash_row_bytes, a->mask, a->dir == QT_ROW_RESTORE ? 1 : 0);
  return hipGetLastError() == hipSuccess ? QT_OK : QT_ERR_LAUNCH;
}
