// Host soundness sweep of qt_gemm's planner (qwen3-tts_amd/csrc/gemm_route.h): plans every argument block read from
// stdin (one per line, qt_gemm_args' fields in order as integers, eps as 0: `python tests/test_gemm_plan_host.py
// --dump`), then `n` seeded random blocks with zero, negative and INT_MAX-sized values.  Meant for the sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/gemm_plan_sweep.cpp -o sweep
//   python tests/test_gemm_plan_host.py --dump | ./sweep 20000
#include "../qwen3-tts_amd/csrc/gemm_route.h"
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <random>
using namespace qt_gemm_impl;

static long long g_routes[11];
static void plan(const qt_gemm_args& a) {
  const GemmPlan pl = gemm_plan(a, GemmKnobs{});
  if ((pl.route == GemmRoute::NONE) != (pl.err != 0)) { printf("plan without route or error\n"); exit(1); }
  ++g_routes[(int)pl.route];
}
static void* ptr(long long v) { return (void*)(uintptr_t)v; }

int main(int argc, char** argv) {
  long long v[34], nread = 0;
  for (;; ++nread) {
    int got = 0;
    while (got < 34 && scanf("%lld", &v[got]) == 1) ++got;
    if (got < 34) break;
    qt_gemm_args a{(int)v[0], (int)v[1], (int)v[2], (int)v[3], (int)v[4], (int)v[5], ptr(v[6]), v[7], (const int*)ptr(v[8]),
                   ptr(v[9]), (const float*)ptr(v[10]), 0.f, (int)v[12], (const float*)ptr(v[13]), (const float*)ptr(v[14]),
                   (int)v[15], (int)v[16], ptr(v[17]), v[18], (int)v[19], (int)v[20], (int)v[21], (int)v[22], (int)v[23],
                   (int)v[24], (int)v[25], ptr(v[26]), v[27], (int)v[28], (const float*)ptr(v[29]),
                   (const float*)ptr(v[30]), (int)v[31], ptr(v[32]), v[33]};
    plan(a);
  }
  std::mt19937_64 g(20240607);
  static const int edge[] = {0, -1, -64, 1, 8, 16, 17, 32, 64, 96, 128, 256, 1024, 2048, 4096, 65536, 1 << 20, INT_MAX,
                             INT_MAX - 15, INT_MIN, INT_MIN + 64};
  auto num = [&] { return g() % 3 ? edge[g() % (sizeof edge / sizeof *edge)] : (int)(g() % 8192) - 64; };
  auto dim = [&] { return g() % 5 ? (g() % 2 ? 1 + (int)(g() % 4100) : 16 << (g() % 14)) : num(); };  // mostly valid
  const int n = argc > 1 ? atoi(argv[1]) : 5000;
  for (int i = 0; i < n; ++i) {
    qt_gemm_args a{};
    a.M = dim(); a.N = dim(); a.K = g() % 4 ? (int)(dim() / 8 * (g() % 2 ? 8ll : 64ll)) : num();
    a.a_dtype = g() % 9 % 3; a.w_dtype = g() % 5 ? 1 : g() % 3; a.o_dtype = g() % 9 % 3;
    a.A = ptr(0x100000 + (g() % 4 ? 0 : 8)); a.W = ptr(0x200000); a.out = ptr(0x300000);
    a.lda = g() % 2 ? a.K : (long long)num() * num();
    a.rmsnorm = g() % 4 == 0; a.act = g() % 4 ? 0 : (int)(g() % 8) - 1; a.epi = g() % 3; a.a_act = g() % 8 ? 0 : 1;
    if (g() % 8 == 0) a.gamma = (const float*)ptr(0x500000);
    if (g() % 8 == 0) a.a_index = (const int*)ptr(0x400000);
    if (g() % 8 == 0) a.out2 = ptr(0xA00000);
    if (g() % 2) { a.taps = g() % 3 ? 1 + (int)(g() % 9) : num(); a.dil = num(); a.cin = g() % 3 ? dim() / 8 * 8 : num();
                   a.cin_pad = g() % 3 ? (int)((a.cin / 32 + 1) * 32ll) : num(); a.t_in = num(); a.t_off = num();
                   a.t_out = g() % 3 ? 1 + (int)(g() % 64) : num(); if (g() % 2) a.M = (int)(a.t_out * (1ll + (int)(g() % 8))); }
    if (g() % 4) { a.ws = ptr(0x10000000); a.ws_bytes = g() % 4 ? (16ll << 20) : (long long)num() * num(); }
    a.splitk = g() % 2 ? 0 : num();
    plan(a);
  }
  printf("%lld blocks read, %d random; per route:", nread, n);
  for (long long c : g_routes) printf(" %lld", c);
  printf("\n");
  return 0;
}
