// The voxel set behind the occupancy IoU of eval_pcd: an open-addressing hash table of packed cell keys (voxkey.h) with
// one flag word per slot - bit 1 for the prediction, bit 2 for the ground truth.  Both clouds go into the same table, so a slot with flags 3 is a
// cell of the intersection.  Plain HIP C++; the only atomics are a 64-bit integer compare-and-swap and 32-bit integer or / add.  The table's
// layout depends on the order in which the threads arrive, the set it holds and therefore every count do not.
#include "../common.h"
#include "eval_reduce.h"
#include "voxkey.h"

typedef unsigned long long u64;

__global__ __launch_bounds__(EVAL_NT) void k_vox_fill(u64* keys, unsigned* flags, long capacity, unsigned* stat) {
  for (long i = (long)blockIdx.x * EVAL_NT + threadIdx.x; i < capacity; i += (long)gridDim.x * EVAL_NT) { keys[i] = VOXEL_EMPTY; flags[i] = 0u; }
  if (blockIdx.x == 0 && threadIdx.x < VOX_STAT_WORDS) stat[threadIdx.x] = 0u;
}

// One point per thread and step.  The home slot is hash & mask (capacity = mask + 1, a power of two), then linear probing.  The probe is a counted
// loop of at most `capacity` steps: a thread that finds neither an empty slot nor its own key in all of them sets stat[VOX_OVERFLOW] and goes on
// to its next point - a full table is reported, it is never waited on.  stat[bit] counts the points skipped by voxel_key (bit is 1 or 2).
__global__ __launch_bounds__(EVAL_NT) void k_vox_insert(const double* pts, long n, double v, unsigned bit, u64* keys, unsigned* flags, u64 mask,
                                                   unsigned* stat) {
  for (long i = (long)blockIdx.x * EVAL_NT + threadIdx.x; i < n; i += (long)gridDim.x * EVAL_NT) {
    u64 key;
    if (!voxel_key(pts[i * 3], pts[i * 3 + 1], pts[i * 3 + 2], v, &key)) { atomicAdd(&stat[bit], 1u); continue; }
    u64 slot = voxel_hash(key) & mask;
    bool placed = false;
    for (u64 step = 0; step <= mask; ++step) {
      const u64 prev = atomicCAS(&keys[slot], (u64)VOXEL_EMPTY, key);
      if (prev == VOXEL_EMPTY || prev == key) { atomicOr(&flags[slot], bit); placed = true; break; }      // this is my slot
      slot = (slot + 1) & mask;
    }
    if (!placed) atomicOr(&stat[VOX_OVERFLOW], 1u);
  }
}

// per workgroup the slots with flags 1, 2 and 3 -> part[b * 3 ..]; the caller adds the rows in block order
__global__ __launch_bounds__(EVAL_NT) void k_vox_count(const unsigned* flags, long capacity, unsigned* part) {
  __shared__ unsigned sh[EVAL_NT];
  unsigned c[3] = {0u, 0u, 0u};
  for (long i = (long)blockIdx.x * EVAL_NT + threadIdx.x; i < capacity; i += (long)gridDim.x * EVAL_NT) {
    const unsigned f = flags[i];
    c[0] += f == 1u; c[1] += f == 2u; c[2] += f == 3u;
  }
  for (int k = 0; k < 3; ++k) {
    const unsigned r = eval_block_count(c[k], sh);
    if (threadIdx.x == 0) part[(long)blockIdx.x * 3 + k] = r;
  }
}

void launch_vox_fill(unsigned long long* keys, unsigned* flags, long capacity, unsigned* stat, hipStream_t s) {
  hipLaunchKernelGGL(k_vox_fill, dim3(eval_nblocks(capacity)), dim3(EVAL_NT), 0, s, (u64*)keys, flags, capacity, stat);
}
void launch_vox_insert(const double* pts, long n, double v, unsigned bit, unsigned long long* keys, unsigned* flags, long capacity, unsigned* stat,
                       hipStream_t s) {
  hipLaunchKernelGGL(k_vox_insert, dim3(eval_nblocks(n)), dim3(EVAL_NT), 0, s, pts, n, v, bit, (u64*)keys, flags, (u64)(capacity - 1), stat);
}
void launch_vox_count(const unsigned* flags, long capacity, unsigned* part, int* nb, hipStream_t s) {
  *nb = eval_nblocks(capacity);
  hipLaunchKernelGGL(k_vox_count, dim3(*nb), dim3(EVAL_NT), 0, s, flags, capacity, part);
}
