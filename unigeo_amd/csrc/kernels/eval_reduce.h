// The one fixed-order reduction of the evaluation kernels (metrics.hip, pcd.hip, pointmap.hip).  Every sum there is taken the same way and the
// order is part of the result: thread t of block b takes the elements b * EVAL_NT + t + j * gridDim * EVAL_NT for ascending j, the EVAL_NT
// threads of a block are folded by halves in LDS, and the host (or a one-workgroup kernel) adds the at most EVAL_MAXB block partials in block
// order.  Only additions and comparisons: a file-level `fp contract(off)` above the include changes nothing here.
#pragma once

#define EVAL_NT 256      // threads per block of the streaming evaluation kernels
#define EVAL_MAXB 1024   // most blocks of such a launch: `part` / `counts` arrays are sized by it

static inline int eval_nblocks(long n) { long b = (n + EVAL_NT - 1) / EVAL_NT; return (int)(b > EVAL_MAXB ? EVAL_MAXB : (b < 1 ? 1 : b)); }

// OP 0: sum, 1: min, 2: max of v over the block; sh holds EVAL_NT doubles and is free again on return
template <int OP> __device__ __forceinline__ double eval_block_reduce(double v, double* sh) {
  const int tid = threadIdx.x;
  sh[tid] = v;
  __syncthreads();
  for (int o = EVAL_NT / 2; o > 0; o >>= 1) {
    if (tid < o) {
      const double a = sh[tid], b = sh[tid + o];
      sh[tid] = OP == 0 ? a + b : (OP == 1 ? (b < a ? b : a) : (b > a ? b : a));
    }
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}
// the block sum of an integer count, folded the same way; sh holds EVAL_NT words and is free again on return
__device__ __forceinline__ unsigned eval_block_count(unsigned v, unsigned* sh) {
  const int tid = threadIdx.x;
  sh[tid] = v;
  __syncthreads();
  for (int o = EVAL_NT / 2; o > 0; o >>= 1) {
    if (tid < o) sh[tid] += sh[tid + o];
    __syncthreads();
  }
  const unsigned r = sh[0];
  __syncthreads();
  return r;
}
// the K block sums of a[0 .. K) -> part[blockIdx.x * K + k]
template <int K> __device__ __forceinline__ void eval_store_sums(const double (&a)[K], double* sh, double* part) {
  for (int k = 0; k < K; ++k) {
    const double r = eval_block_reduce<0>(a[k], sh);
    if (threadIdx.x == 0) part[(long)blockIdx.x * K + k] = r;
  }
}
