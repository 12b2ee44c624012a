// Prefix cache (qwen_tts.PrefixCache): the talker K/V of an instruction's positions moved between a
// session's cache rows and a cache entry, every job of a prefill call in one launch.  For a fixed (job, K|V, layer,
// KV head) both sides are one contiguous span of n * D elements -- row `row` of the layer's [B][Hkv][Lmax][D] from
// position `pos`, and [n][D] of the entry block [2][n_layers][Hkv][n][D] -- so this is a segmented copy.
// Data movement only: 16 B per lane, four loads in flight per lane before the first store, no arithmetic.
#include "common.h"

namespace {

constexpr int KVP_THREADS = 256;
constexpr int KVP_UNROLL = 4;  // 16 KiB per block: a 76.8 KB segment (n = 300, D = 128, bf16) is 5 blocks

// grid (chunks of the longest segment, jobs x 2 n_layers x Hkv segments); blocks past a shorter job's end leave
__global__ __launch_bounds__(KVP_THREADS) void kv_prefix_k(const qt_kv_prefix_job* __restrict__ jobs,
                                                          void* const* __restrict__ layers, int n_layers, int Hkv,
                                                          int Lmax, int G) {
  const int per_job = 2 * n_layers * Hkv;
  const int seg = blockIdx.y;
  const int j = seg / per_job, r = seg - j * per_job;
  const int kl = r / Hkv, h = r - kl * Hkv;  // kl: K layers 0..n_layers-1, then V layers
  const qt_kv_prefix_job job = jobs[j];
  const long long nvec = (long long)job.n * G;  // 16-byte groups of this segment
  const long long i0 = (long long)blockIdx.x * (KVP_THREADS * KVP_UNROLL) + threadIdx.x;
  if ((long long)blockIdx.x * (KVP_THREADS * KVP_UNROLL) >= nvec) return;
  u32x4_t* sess = (u32x4_t*)layers[kl] + (((long long)job.row * Hkv + h) * Lmax + job.pos) * G;
  u32x4_t* ent = (u32x4_t*)job.block + ((long long)kl * Hkv + h) * nvec;
  const u32x4_t* src = job.dir == QT_KV_ADOPT ? ent : sess;
  u32x4_t* dst = job.dir == QT_KV_ADOPT ? sess : ent;
  u32x4_t v[KVP_UNROLL];
#pragma unroll
  for (int u = 0; u < KVP_UNROLL; ++u) {
    const long long i = i0 + u * KVP_THREADS;
    if (i < nvec) v[u] = src[i];
  }
#pragma unroll
  for (int u = 0; u < KVP_UNROLL; ++u) {
    const long long i = i0 + u * KVP_THREADS;
    if (i < nvec) dst[i] = v[u];
  }
}

}  // namespace

extern "C" int qt_kv_prefix(const qt_kv_prefix_job* jobs_host, const qt_kv_prefix_job* jobs_dev, int n_jobs,
                            void* const* layers_dev, int n_layers, int B, int Hkv, int Lmax, int D, int dtype,
                            void* s) {
  if (dtype != QT_F32 && dtype != QT_BF16) return QT_ERR_DTYPE;
  const int elem = dtype == QT_BF16 ? 2 : 4;
  if (n_jobs < 0 || n_layers <= 0 || B <= 0 || Hkv <= 0 || Lmax <= 0 || D <= 0 || (D * elem) % 16)
    return QT_ERR_SHAPE;
  if (n_jobs == 0) return QT_OK;
  if (!jobs_host || !jobs_dev || !layers_dev) return QT_ERR_ARG;
  int n_max = 0;
  for (int j = 0; j < n_jobs; ++j) {
    const qt_kv_prefix_job& q = jobs_host[j];
    if (q.n < 0) return QT_ERR_SHAPE;
    if (q.n == 0) continue;  // a no-op, whatever else it says
    if (!q.block || ((uintptr_t)q.block & 15) || (q.dir != QT_KV_ADOPT && q.dir != QT_KV_EXPORT)) return QT_ERR_ARG;
    if (q.row < 0 || q.row >= B || q.pos < 0 || q.pos > Lmax - q.n) return QT_ERR_SHAPE;
    n_max = q.n > n_max ? q.n : n_max;
  }
  if (n_max == 0) return QT_OK;
  const int G = D * elem / 16;
  const long long segs = (long long)n_jobs * 2 * n_layers * Hkv;
  const long long chunks = ((long long)n_max * G + KVP_THREADS * KVP_UNROLL - 1) / (KVP_THREADS * KVP_UNROLL);
  if (segs > 65535 || chunks > 0x7fffffffll) return QT_ERR_SHAPE;
  hipLaunchKernelGGL(kv_prefix_k, dim3((unsigned)chunks, (unsigned)segs), dim3(KVP_THREADS), 0, (hipStream_t)s,
                     jobs_dev, layers_dev, n_layers, Hkv, Lmax, G);
  return hipGetLastError() == hipSuccess ? QT_OK : QT_ERR_LAUNCH;
}
