// Phase stamps of the headline instantiation of the 256x256 BF6 kernel (gemm_w4a4_f6q_kernel<..., TR = true, PAIR = true>) with the K loop
// stamped as a whole: link against a tools library built with -DATOM_TR_LOOP_ONLY (ABFLAGS=-DATOM_TR_LOOP_ONLY tools/ab_build.sh NAME,
// then hipcc -O2 tools/trace_f6q_loop.cpp -Lbuild/ab/NAME -latom_hip).  Without per-step stamps every K step runs the code the product
// build runs, so "K loop" below is the product loop's time; tools/trace_f6q.cpp keeps the per-step and in-step view.
//   trace_f6q_loop [M N K]      (ATOM_B_SCALE_PAIRS is asserted on random scales: the results are garbage, the timing is the real thing)
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <random>
#include "../include/atom_hip.h"
int main(int argc, char **argv) {
  int M = argc > 1 ? atoi(argv[1]) : 4096, N = argc > 2 ? atoi(argv[2]) : 4096, K = argc > 3 ? atoi(argv[3]) : 4096;
  int K4 = K - 128, G = K4 / 128;
  std::mt19937_64 rng(1);
  auto sc = [&]() { return (_Float16)(0.005f + 0.045f * ((rng() >> 11) * (1.0 / 9007199254740992.0))); };
  auto mk = [&](size_t bytes, int kind) { void *d; (void)hipMalloc(&d, bytes); std::vector<uint8_t> h(bytes);
    if (kind == 0) for (auto &x : h) x = rng() & 0xFF;
    else { _Float16 *p = (_Float16 *)h.data(); for (size_t i = 0; i < bytes / 2; ++i) p[i] = sc(); }
    (void)hipMemcpy(d, h.data(), bytes, hipMemcpyHostToDevice); return d; };
  const size_t Mp = (M + 255) / 256 * 256;
  void *A6; { const size_t bytes = (size_t)G * Mp * 104; (void)hipMalloc(&A6, bytes); std::vector<uint8_t> h(bytes);
    for (size_t r = 0; r < bytes / 104; ++r) { for (int i = 0; i < 96; ++i) h[r * 104 + i] = rng() & 0xFF; const _Float16 v = sc(); *(_Float16 *)&h[r * 104 + 96] = v; *(float *)&h[r * 104 + 100] = (float)v; }
    (void)hipMemcpy(A6, h.data(), bytes, hipMemcpyHostToDevice); }
  void *B4 = mk((size_t)N * K4 / 2, 0), *A8 = mk((size_t)M * 128, 0), *B8 = mk((size_t)N * 128, 0);
  void *sA = mk((size_t)G * M * 2, 1), *sB = mk((size_t)G * N * 2, 1), *sA8 = mk(M * 2, 1), *sB8 = mk(N * 2, 1);
  void *B6; (void)hipMalloc(&B6, atom_f6_weight_bytes(N, K));
  if (int st = atom_repack_weight_f6s(B4, sB, N, K, B6, nullptr)) { printf("repack err %d\n", st); return 1; }
  void *D; (void)hipMalloc(&D, (size_t)M * N * 2);
  const size_t WS = 128, TR = 2 * 8 * WS;                   // dwords per wave, two workgroups of 8 waves
  unsigned *tr; (void)hipMalloc(&tr, TR * 4); (void)hipMemset(tr, 0, TR * 4);
  char buf[64]; snprintf(buf, sizeof buf, "%llx", (unsigned long long)tr); setenv("ATOM_TRACE_PTR", buf, 1); setenv("ATOM_F6_CFG", "2016", 1);
  const int layout = ATOM_AB_F6 | ATOM_B_F6S | ATOM_SCALE_LAYOUT_PLAIN | ATOM_B_SCALE_PAIRS;
  hipEvent_t e0, e1; (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
  for (int i = 0; i < 300; ++i) { int st = atom_gemm_w4a4_f16(A6, B6, sA, sB, A8, B8, sA8, sB8, D, M, N, K, 128, 128, layout, nullptr); if (st) { printf("err %d\n", st); return 1; } }
  (void)hipEventRecord(e0, 0);
  for (int i = 0; i < 200; ++i) (void)atom_gemm_w4a4_f16(A6, B6, sA, sB, A8, B8, sA8, sB8, D, M, N, K, 128, 128, layout, nullptr);
  (void)hipEventRecord(e1, 0); (void)hipEventSynchronize(e1);
  float ms; (void)hipEventElapsedTime(&ms, e0, e1);
  printf("traced build: %.2f us per launch (200 launches)\n", ms * 1e3 / 200);
  std::vector<unsigned> h(TR); (void)hipMemcpy(h.data(), tr, TR * 4, hipMemcpyDeviceToHost);
  auto d = [&](unsigned a, unsigned b) { return (int)(a - b); };
  for (int wg = 0; wg < 2; ++wg) {
    const unsigned t00 = h[wg * 8 * WS];
    printf("workgroup %s\n", wg ? "last" : "0");
    for (int w = 0; w < 8; ++w) {
      unsigned *e = &h[(wg * 8 + w) * WS];
      if (e[17]) { printf("this library stamps every K step: build it with -DATOM_TR_LOOP_ONLY\n"); return 1; }
      const double mhz = 100.0 * d(e[8], e[0]) / (double)d(e[63], e[62]);
      printf(" wave %d: entry %+d | dma issued +%d | stage 0 landed +%d | first fragments +%d | K loop (%d steps) +%d = %.1f per step | wait for keeper half 1 +%d | "
             "barrier +%d | keeper + stores issued +%d | stores done +%d | total %d cycles = %.2f us, %.0f MHz\n", w, d(e[0], t00), d(e[1], e[0]), d(e[2], e[1]),
             d(e[3], e[2]), G, d(e[4], e[3]), d(e[4], e[3]) / (double)G, d(e[5], e[4]), d(e[6], e[5]), d(e[7], e[6]), d(e[8], e[7]), d(e[8], e[0]),
             d(e[63], e[62]) / 100.0, mhz);
      if (e[9])                                             // stamps inside the keeper (a library from before them leaves 9..13 zero)
        printf("         keeper: entry +0 | first store issued +%d | slot 8 +%d | last MFMA +%d | last store issued +%d | vmcnt(0) +%d\n", d(e[10], e[9]),
               d(e[11], e[9]), d(e[12], e[9]), d(e[13], e[9]), d(e[8], e[9]));
    }
  }
  return 0;
}
