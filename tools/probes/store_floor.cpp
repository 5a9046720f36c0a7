// Probe: the write floor of the 256x256 BF6 kernel's keeper (profiles/f6q_write/).  256 workgroups of 512 threads write a 4096 x 4096 fp16
// matrix with exactly the keeper's store pattern and no arithmetic: wave (wm, wn) of a tile owns 128 tokens x 64 features; lane (l15, kb)
// writes row 2 l15 + (block & 1) of token block `block` (p_row order: 32 (block >> 1) + (block & 1)) and features 8 kb of each 32-feature
// half, two 16-byte stores 64 B apart, scalar base + 32-bit lane offset + instruction offset as the whole-tile path of q_keeper does.
// Arms: plain, write-through (sc0 sc1) and nt stores; each with the 8 blocks issued back to back and spread over about 2 k, 5 k and 9 k
// cycles by s_sleep (the keeper issues them over 6.7-9.2 k).  Reports, per arm: us per launch by events over 200 launches behind a ramp,
// and the cycles (s_memtime) and ns (s_memrealtime, 100 MHz) from the first store issued to s_waitcnt vmcnt(0), over all 2,048 waves.
//   make -C atom_amd/csrc probes && build/tools/store_floor
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <vector>
typedef unsigned int v4u __attribute__((ext_vector_type(4)));
constexpr int N = 4096, NWG = 256;

template <int FL>   // 0 plain, 1 sc0 sc1, 2 nt
__device__ __forceinline__ void st16(char *sbase, unsigned voff, v4u v) {
  if constexpr (FL == 1) asm volatile("global_store_dwordx4 %0, %1, %2 sc0 sc1\n\ts_nop 1" ::"v"(voff), "v"(v), "s"(sbase) : "memory");
  else if constexpr (FL == 2) __builtin_nontemporal_store(v, reinterpret_cast<v4u *>(sbase + voff));
  else *reinterpret_cast<v4u *>(sbase + voff) = v;
}

template <int FL, int SLEEP>
__global__ __launch_bounds__(512) void keeper_stores(char *D, unsigned long long *stamps) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave >> 2, wn = wave & 3, l15 = lane & 15, kb = lane >> 4;
  int id = blockIdx.x;                                   // the kernel's tile index at 16 x 16 tiles: XCD-contiguous, bands of 4 tile rows
  id = (id & 7) * (NWG / 8) + (id >> 3);
  const int band = id / (4 * (N / 256)), inband = id % (4 * (N / 256));
  const int m0 = (band * 4 + inband % 4) * 256, n0 = (inband / 4) * 256;
  const unsigned voff = (unsigned)(((wm * 128 + 2 * l15) * N + wn * 64 + 8 * kb) * 2);
  v4u v = {threadIdx.x, blockIdx.x, 1u, 2u};
  const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
#pragma unroll
  for (int tb = 0; tb < 8; ++tb) {
    char *dtb = D + ((size_t)(m0 + 32 * (tb >> 1) + (tb & 1)) * N + n0) * 2;
    v.z = tb;
    st16<FL>(dtb, voff, v);
    st16<FL>(dtb + 64, voff, v);
    if constexpr (SLEEP > 0) { if (tb < 7) __builtin_amdgcn_s_sleep(SLEEP); }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
  if (lane == 0) {
    unsigned long long *e = stamps + (blockIdx.x * 8 + wave) * 4;
    e[0] = t0; e[1] = t1; e[2] = r0; e[3] = r1;
  }
}

template <int FL, int SLEEP>
static void arm(const char *name, char *D, unsigned long long *stamps) {
  hipEvent_t e0, e1; (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
  for (int i = 0; i < 400; ++i) hipLaunchKernelGGL((keeper_stores<FL, SLEEP>), dim3(NWG), dim3(512), 0, 0, D, stamps);   // ramp
  float best = 1e30f, tot = 0;
  for (int rep = 0; rep < 5; ++rep) {
    (void)hipEventRecord(e0, 0);
    for (int i = 0; i < 200; ++i) hipLaunchKernelGGL((keeper_stores<FL, SLEEP>), dim3(NWG), dim3(512), 0, 0, D, stamps);
    (void)hipEventRecord(e1, 0); (void)hipEventSynchronize(e1);
    float ms; (void)hipEventElapsedTime(&ms, e0, e1); ms /= 200; tot += ms; best = std::min(best, ms);
  }
  std::vector<unsigned long long> h(NWG * 8 * 4);
  (void)hipMemcpy(h.data(), stamps, h.size() * 8, hipMemcpyDeviceToHost);
  std::vector<long long> cyc, ns;
  unsigned long long rmin = ~0ull, rmax = 0;
  for (int w = 0; w < NWG * 8; ++w) {
    cyc.push_back((long long)(h[w * 4 + 1] - h[w * 4]));
    ns.push_back((long long)(h[w * 4 + 3] - h[w * 4 + 2]) * 10);
    rmin = std::min(rmin, h[w * 4 + 2]); rmax = std::max(rmax, h[w * 4 + 3]);
  }
  std::sort(cyc.begin(), cyc.end()); std::sort(ns.begin(), ns.end());
  const size_t n = cyc.size();
  printf("%-6s sleep %2d: %6.2f us per launch (best of five %6.2f) = %.2f TB/s | first store -> vmcnt(0) per wave: cycles min %lld median %lld "
         "max %lld, ns min %lld median %lld max %lld | first wave's first store -> last wave's vmcnt(0), last launch: %.2f us\n",
         name, SLEEP, tot / 5 * 1e3, best * 1e3, (double)N * N * 2 / (tot / 5 * 1e-3) / 1e12, cyc[0], cyc[n / 2], cyc[n - 1], ns[0], ns[n / 2],
         ns[n - 1], (double)(rmax - rmin) / 100.0);
}

int main() {
  char *D; unsigned long long *stamps;
  if (hipMalloc(&D, (size_t)N * N * 2) != hipSuccess || hipMalloc(&stamps, NWG * 8 * 4 * 8) != hipSuccess) { printf("hipMalloc failed\n"); return 1; }
  // s_sleep n waits about 64 n cycles; 7 gaps between the 8 blocks: 4 -> about 2 k cycles, 11 -> 5 k, 20 -> 9 k
  for (int round = 0; round < 2; ++round) {
    arm<0, 0>("plain", D, stamps); arm<1, 0>("sc0sc1", D, stamps); arm<2, 0>("nt", D, stamps);
    arm<0, 4>("plain", D, stamps); arm<1, 4>("sc0sc1", D, stamps); arm<2, 4>("nt", D, stamps);
    arm<0, 11>("plain", D, stamps); arm<1, 11>("sc0sc1", D, stamps); arm<2, 11>("nt", D, stamps);
    arm<0, 20>("plain", D, stamps); arm<1, 20>("sc0sc1", D, stamps); arm<2, 20>("nt", D, stamps);
  }
  if (hipDeviceSynchronize() != hipSuccess) { printf("HIP error\n"); return 1; }
  return 0;
}
