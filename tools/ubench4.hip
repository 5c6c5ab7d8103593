// tools/ubench4.hip — the FAST scan filter's threshold test, four starts packed into one register, against the per-start test it would
// replace (profiles/scan_packed_test_ubench.txt).  The packed form writes the top byte of min (hf, hr) into one of four byte lanes of an
// accumulator (v_min_u32_sdwa, destination preserved) and asks "which bytes are below N" once for four starts:
// F = (acc - 0x01010101 N) & ~acc & 0x80808080.  Same harness as ubench2 / ubench3: 8 independent chains per lane, 8 waves per SIMD, every CU;
// the products (here: a[], never written in the loop) do not depend on the accumulators, as in the kernel's unrolled phase A.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdint.h>
#define ITERS 32768
#define SDWA_MIN(J) "v_min_u32_sdwa %0, %1, %2 dst_sel:BYTE_" #J " dst_unused:UNUSED_PRESERVE src0_sel:BYTE_3 src1_sel:BYTE_3"
/* gfx940-family hardware does not forward a partly written register: the instruction behind an SDWA write must not read its destination (a
   preserving write reads it too).  So the mins rotate over the eight accumulators, byte lane by byte lane, as the kernel separates them. */
__device__ __forceinline__ void minTop (uint32_t &acc, uint32_t x, uint32_t y, int j)
{
  if (j == 0)      asm volatile (SDWA_MIN (0) : "+v"(acc) : "v"(x), "v"(y));
  else if (j == 1) asm volatile (SDWA_MIN (1) : "+v"(acc) : "v"(x), "v"(y));
  else if (j == 2) asm volatile (SDWA_MIN (2) : "+v"(acc) : "v"(x), "v"(y));
  else             asm volatile (SDWA_MIN (3) : "+v"(acc) : "v"(x), "v"(y));
}
template <int OP>
__global__ __launch_bounds__(256) void k (uint32_t *out, uint32_t s0, uint32_t s1)
{
  uint32_t a[8], acc[8], m = 0, t;
  for (int i = 0; i < 8; ++i) { a[i] = threadIdx.x * 2654435761u + i * 40503u + s0; acc[i] = a[i] * 31u; }
  const uint32_t f = s1 | 1, nRep = 0x04040404u * s0, hi = 0x80808080u * s0;     /* s0 = 1: the launch's argument, so the constants live in registers as the kernel's would */
  for (int it = 0; it < ITERS; ++it)
    {
      if (OP == 1 || OP == 4 || OP == 5)                     /* four mins per accumulator: 4 inst a chain */
        {
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < 8; ++i) minTop (acc[i], a[(i + j) & 7], a[(i + j + 1) & 7], j);
        }
#pragma unroll
      for (int i = 0; i < 8; ++i)
        { const uint32_t x0 = a[i], x1 = a[(i + 1) & 7], x2 = a[(i + 2) & 7], x3 = a[(i + 3) & 7];
          if (OP == 0) asm volatile ("v_mul_lo_u32 %0, %1, %2" : "=v"(acc[i]) : "v"(acc[i]), "v"(f));
          else if (OP == 2) asm volatile ("v_min_u32 %0, %1, %2" : "=v"(acc[i]) : "v"(x0), "v"(x1));
          else if (OP == 3) asm volatile ("v_not_b32 %0, %1" : "=v"(acc[i]) : "v"(acc[i]));
          else if (OP == 4) asm volatile ("v_sub_u32 %1, %0, %3\n\tv_not_b32 %0, %0\n\tv_and_b32 %1, %1, %0\n\tv_and_b32 %1, %1, %4\n\t"       /* the detect as the formula reads and the combine: with the mins 10 inst */
                                          "v_lshrrev_b32 %1, 3, %1\n\tv_or_b32 %2, %2, %1" : "+v"(acc[i]), "=&v"(t), "+v"(m) : "v"(nRep), "v"(hi));
          else if (OP == 5) asm volatile ("v_sub_u32 %1, %0, %3\n\tv_bitop3_b32 %1, %1, %0, %4 bitop3:0x20\n\t"                                    /* the three-way and as one v_bitop3 (t & ~acc & hi: 0x20), what the compiler makes of it: with the mins 8 inst */
                                          "v_lshrrev_b32 %1, 3, %1\n\tv_or_b32 %2, %2, %1" : "+v"(acc[i]), "=&v"(t), "+v"(m) : "v"(nRep), "v"(hi));
          else if (OP == 6) asm volatile ("v_min_u32 %1, %2, %3\n\tv_cmp_gt_u32 vcc, %6, %1\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc\n\t"  /* today's tail, four starts: 12 inst */
                                          "v_min_u32 %1, %3, %4\n\tv_cmp_gt_u32 vcc, %6, %1\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc\n\t"
                                          "v_min_u32 %1, %4, %5\n\tv_cmp_gt_u32 vcc, %6, %1\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc\n\t"
                                          "v_min_u32 %1, %5, %2\n\tv_cmp_gt_u32 vcc, %6, %1\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc"
                                          : "+v"(acc[i]), "=&v"(t) : "v"(x0), "v"(x1), "v"(x2), "v"(x3), "s"(hi) : "vcc");
          else if (OP == 7) asm volatile ("v_bitop3_b32 %0, %1, %2, %3 bitop3:0x20" : "=v"(acc[i]) : "v"(acc[i]), "v"(x0), "v"(hi));
          else if (OP == 8) asm volatile ("v_sub_u32 %0, %0, %1" : "+v"(acc[i]) : "v"(nRep));
        }
    }
  uint32_t r = m; for (int i = 0; i < 8; ++i) r ^= a[i] ^ acc[i];
  out[blockIdx.x * blockDim.x + threadIdx.x] = r;
}
template <int OP> void run (const char *name, uint32_t *d, int perInst = 1)
{
  const int blocks = 256 * 8;
  hipEvent_t e0, e1; hipEventCreate (&e0); hipEventCreate (&e1);
  hipLaunchKernelGGL (k<OP>, dim3 (blocks), dim3 (256), 0, 0, d, 1u, 0x9e3779b9u);
  hipDeviceSynchronize ();
  hipEventRecord (e0);
  for (int r = 0; r < 3; ++r) hipLaunchKernelGGL (k<OP>, dim3 (blocks), dim3 (256), 0, 0, d, 1u, 0x9e3779b9u);
  hipEventRecord (e1); hipEventSynchronize (e1);
  float ms; hipEventElapsedTime (&ms, e0, e1); ms /= 3;
  double ops = (double) blocks * 256 * ITERS * 8 * perInst;
  printf ("%-44s %8.3f ms  %7.2f T lane-ops/s  (%2d inst)\n", name, ms, ops / ms / 1e9, perInst);
}
int main ()
{
  uint32_t *d; hipMalloc (&d, 256 * 8 * 256 * 4);
  run<0> ("v_mul_lo_u32 (warm)", d); run<0> ("v_mul_lo_u32", d);
  run<2> ("v_min_u32", d); run<1> ("v_min_u32_sdwa, preserve, 4 byte lanes", d, 4);
  run<3> ("v_not_b32", d); run<8> ("v_sub_u32", d); run<7> ("v_bitop3_b32 (a & ~b & c)", d);
  run<6> ("4 x (min + cmp + addc): today's, 4 starts", d, 12);
  run<4> ("packed tail, 4 starts (sub/not/and/and)", d, 10);
  run<5> ("packed tail, 4 starts (sub/bitop3)", d, 8);
  if (hipDeviceSynchronize () != hipSuccess) { printf ("device error\n"); return 1; }
  return 0;
}
