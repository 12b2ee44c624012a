// Streaming-text input: projected text rows scattered into a session's trailing-text buffer.
#include "common.h"

namespace {

// Block (j, y): entry j of the slot table, dims [y * 1024, ...) of its row.  An entry whose {row, pos} names no
// position of trailing[B][T][H] is padding of the fixed-size table (or text past the frame cap): skipped, not an error.
__global__ __launch_bounds__(256) void trail_append_k(const float* __restrict__ rows, const int* __restrict__ slots,
                                                      float* __restrict__ trailing, int B, int T, int H) {
  const int j = blockIdx.x;
  const int row = slots[2 * j], pos = slots[2 * j + 1];
  if (row < 0 || row >= B || pos < 0 || pos >= T) return;
  const float* src = rows + (long long)j * H;
  float* dst = trailing + ((long long)row * T + pos) * H;
  for (int i = (blockIdx.y * 256 + threadIdx.x) * 4; i < H; i += gridDim.y * 1024)
    *(f32x4_t*)(dst + i) = *(const f32x4_t*)(src + i);
}

}  // namespace

extern "C" int qt_trail_append(const float* rows, const int* slots, float* trailing, int B, int T, int H, int n,
                               void* s) {
  if (!rows || !slots || !trailing) return QT_ERR_ARG;
  if (B <= 0 || T <= 0 || H <= 0 || n <= 0 || n > 65535 || H % 4) return QT_ERR_SHAPE;
  if (((uintptr_t)rows & 15) || ((uintptr_t)trailing & 15) || ((uintptr_t)slots & 3)) return QT_ERR_ARG;
  hipLaunchKernelGGL(trail_append_k, dim3(n, (H + 1023) / 1024), dim3(256), 0, (hipStream_t)s, rows, slots, trailing,
                     B, T, H);
  return hipGetLastError() == hipSuccess ? 0 : QT_ERR_LAUNCH;
}
