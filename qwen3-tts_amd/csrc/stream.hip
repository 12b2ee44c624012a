// Per-row incremental codec decode (codec.RowCodecStream): the stage input window with its history update, and the
// per-row frame clock.  Both read a device row table [2][B] (nrow, begin), so one captured feed graph serves every
// mix of beginning, continuing, idle and ragged batch rows.  Data movement only: 16 B per lane, no arithmetic.
#include "common.h"

namespace {

// One thread per 16-byte channel group of one new row: xin[b][H + j] = x[b][j], or zeros in a beginning row's head.
// The threads of row j = 0 also own their group's history, for all its H rows: each writes the window's history rows,
// then builds the new history from rows m_b.. of the window -- where those are history rows it reads its own writes
// back (window row m_b + t, never hist row m_b + t, which an earlier t may have overwritten), and where they are rows
// of x it reads x itself.  So no thread waits on another, whatever m_b is against H.
__global__ __launch_bounds__(256) void stream_window_k(u32x4_t* hist, const u32x4_t* __restrict__ x, u32x4_t* xin,
                                                       int H, int n, int G, int rpf, int head,
                                                       const int* __restrict__ rows, int B) {
  const long long idx = blockIdx.x * 256ll + threadIdx.x;
  const int b = blockIdx.y;
  if (idx >= (long long)n * G) return;
  const int j = (int)(idx / G), g = (int)(idx - (long long)j * G);
  const int begin = rows[B + b];
  const int z = begin ? head : 0;
  const u32x4_t zero = {0u, 0u, 0u, 0u};
  const u32x4_t* xb = x + (long long)b * n * G + g;
  u32x4_t* wb = xin + (long long)b * (H + n) * G + g;
  wb[(long long)(H + j) * G] = j < z ? zero : xb[(long long)j * G];
  if (j != 0 || H == 0) return;
  u32x4_t* hb = hist + (long long)b * H * G + g;
  for (int t = 0; t < H; ++t) wb[(long long)t * G] = begin ? zero : hb[(long long)t * G];
  const int m = min(max(rows[b], 0) * rpf, n);  // a row never consumes more than the feed holds
  if (m == 0 && !begin) return;                 // the new history is the old one
  for (int t = 0; t < H; ++t) {
    const int src = m + t;
    u32x4_t v;
    if (src < H) v = wb[(long long)src * G];
    else v = (src - H) < z ? zero : xb[(long long)(src - H) * G];
    hb[(long long)t * G] = v;
  }
}

__global__ void stream_rows_k(int* __restrict__ nf, const int* __restrict__ rows, int B, int n, int* __restrict__ pos,
                              int* __restrict__ row_len) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int base = rows[B + b] ? 0 : nf[b];
  for (int j = 0; j < n; ++j) {
    pos[b * n + j] = base + j;
    row_len[b * n + j] = base + j + 1;
  }
  nf[b] = base + min(max(rows[b], 0), n);
}

}  // namespace

extern "C" int qt_stream_window(void* hist, const void* x, void* xin, int dtype, int B, int H, int n, int C,
                                int rows_per_frame, int head, const int* rows, void* s) {
  if (dtype != QT_F32 && dtype != QT_BF16) return QT_ERR_DTYPE;
  const int per = dtype == QT_BF16 ? 8 : 4;  // elements in 16 bytes
  if (B <= 0 || B > 65535 || H < 0 || n <= 0 || C <= 0 || C % per || rows_per_frame <= 0 || head < 0)
    return QT_ERR_SHAPE;
  if (!x || !xin || !rows || (H > 0 && !hist)) return QT_ERR_ARG;
  if (((uintptr_t)x | (uintptr_t)xin | (uintptr_t)hist) & 15) return QT_ERR_ARG;
  const int G = C / per;
  const long long blocks = ((long long)n * G + 255) / 256;
  if (blocks > 0x7fffffffll) return QT_ERR_SHAPE;
  const dim3 grid((unsigned)blocks, B);
  hipLaunchKernelGGL(stream_window_k, grid, dim3(256), 0, (hipStream_t)s, (u32x4_t*)hist, (const u32x4_t*)x,
                     (u32x4_t*)xin, H, n, G, rows_per_frame, head, rows, B);
  return hipGetLastError() == hipSuccess ? 0 : QT_ERR_LAUNCH;
}

extern "C" int qt_stream_rows(int* nf, const int* rows, int B, int n, int* pos, int* row_len, void* s) {
  if (B <= 0 || n <= 0) return QT_ERR_SHAPE;
  if (!nf || !rows || !pos || !row_len) return QT_ERR_ARG;
  hipLaunchKernelGGL(stream_rows_k, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)s, nf, rows, B, n, pos, row_len);
  return hipGetLastError() == hipSuccess ? 0 : QT_ERR_LAUNCH;
}
