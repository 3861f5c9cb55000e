// Digest of a device vector (formula and host form: hdg_checkpoint.hpp):
//   d0 = sum b_i,  d1 = sum b_i (2 i + 1)  mod 2^64  over the 64-bit patterns b_i of n doubles.
// Integer sums: exact in any order, so the result depends on neither grid nor wave order nor reduction tree, and needs no
// atomics: block partials (vector stores by one lane per block), then one fixed single-block second stage.
#pragma once

#include <hip/hip_runtime.h>

namespace hdg {

#define HDG_DIGEST_BLOCK 256
#define HDG_DIGEST_MAX_BLOCKS 4096  // partials the second stage reads; beyond 2 * 256 * 4096 words a thread takes further pairs

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}
// the two sums of a workgroup in its first lane
__device__ __forceinline__ void digest_block_sum(unsigned long long& s0, unsigned long long& s1) {
  __shared__ unsigned long long sm[HDG_DIGEST_BLOCK / 64][2];
  s0 = wave_sum_u64(s0);
  s1 = wave_sum_u64(s1);
  if ((threadIdx.x & 63) == 0) { sm[threadIdx.x >> 6][0] = s0; sm[threadIdx.x >> 6][1] = s1; }
  __syncthreads();
  if (threadIdx.x == 0) {
    s0 = 0; s1 = 0;
    for (int w = 0; w < HDG_DIGEST_BLOCK / 64; w++) { s0 += sm[w][0]; s1 += sm[w][1]; }
  }
}
// v: 16-byte aligned, n words; part: 2 words per block.  One 16-byte pair per thread and trip, like the vector kernels.
__global__ __launch_bounds__(HDG_DIGEST_BLOCK) void k_digest(long n, const unsigned long long* __restrict__ v,
                                                             unsigned long long* __restrict__ part) {
  const long npairs = n >> 1;
  const long stride = (long)gridDim.x * HDG_DIGEST_BLOCK;
  const ulonglong2* __restrict__ v2 = reinterpret_cast<const ulonglong2*>(v);
  unsigned long long s0 = 0, s1 = 0;
  for (long p = (long)blockIdx.x * HDG_DIGEST_BLOCK + threadIdx.x; p < npairs; p += stride) {
    const ulonglong2 w = v2[p];
    const unsigned long long i4 = 4ULL * (unsigned long long)p;  // 2 i for i = 2 p
    s0 += w.x + w.y;
    s1 += w.x * (i4 + 1ULL) + w.y * (i4 + 3ULL);
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {  // the odd last word
    const unsigned long long w = v[n - 1];
    s0 += w;
    s1 += w * (2ULL * (unsigned long long)(n - 1) + 1ULL);
  }
  digest_block_sum(s0, s1);
  if (threadIdx.x == 0) { part[2 * blockIdx.x] = s0; part[2 * blockIdx.x + 1] = s1; }
}
// second stage, one workgroup: out[0 .. 1] = the sums of the nblocks partials
__global__ __launch_bounds__(HDG_DIGEST_BLOCK) void k_digest_final(int nblocks, const unsigned long long* __restrict__ part,
                                                                   unsigned long long* __restrict__ out) {
  unsigned long long s0 = 0, s1 = 0;
  for (int b = threadIdx.x; b < nblocks; b += HDG_DIGEST_BLOCK) { s0 += part[2 * b]; s1 += part[2 * b + 1]; }
  digest_block_sum(s0, s1);
  if (threadIdx.x == 0) { out[0] = s0; out[1] = s1; }
}

}  // namespace hdg
