// Internal to the GEMM sources (gemm.hip, gemm_pf2.hip, gemm_sk.hip): the kernel parameter block built by qt_gemm from
// qt_gemm_args and its plan (gemm_route.h), and the launchers that live in their own translation units.
#pragma once
#include "common.h"
#include "gemm_route.h"

namespace qt_gemm_impl {

struct GemmP {
  int M, N, Kp, Klog;          // Kp = padded K (taps * cin_pad), Klog = RMSNorm length
  const void* A; long long lda;
  const int* a_index;
  const void* W;
  const float* gamma; float eps; int rms;
  const float* bias; const float* colscale;
  int act, epi;
  void* out; long long ldo;
  int taps, dil, cin, cin_pad, t_in, t_out, t_off;
  int ks;                       // decode GEMV split-K factor (gridDim.y), 1 = none
  unsigned* cnt; float* part;   // split-K arrival counters [ntiles] + partials [ntiles][ks][64*4+16] (GEMV) /
                                //   gemm_pf2_k split records (17+ rows); null unless the plan splits
  const float* sn_a; const float* sn_ib;  // optional SnakeBeta on A (per input channel)
  int a_elu;                    // ELU on A (tokenizer encoder convs)
  int mr;                       // decode GEMV rows per row group (gridDim.z = ceil(M / mr))
  bf16_t* out2; long long ldo2; // optional bf16 copy of the stored output (decode residual stream shadow)
};

// gemm_pf2_k (gemm_pf2.hip): prefill linears with bf16 A and bf16 pre-tiled W, K % 64 == 0, 16-byte aligned A
// cfg = a Pf2Cfg id of gemm_route.h, ks its split-K factor (> 1: p.cnt / p.part hold the records)
void launch_pf2_f32(const GemmP& p, int cfg, int ks, hipStream_t s);
void launch_pf2_bf16(const GemmP& p, int cfg, int ks, hipStream_t s);
// gemm_sk_k (gemm_sk.hip): 17..64 rows, bf16 A and bf16 pre-tiled W, K % 32 == 0, 16-byte aligned A rows
// mi = 16-row tiles per block (2..4)
void launch_sk_f32(const GemmP& p, int mi, hipStream_t s);
void launch_sk_bf16(const GemmP& p, int mi, hipStream_t s);

}  // namespace qt_gemm_impl
