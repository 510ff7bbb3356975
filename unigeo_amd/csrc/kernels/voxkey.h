// The voxel key of the occupancy IoU, plain C++ shared by the device kernels (kernels/voxel.hip) and the host
// (tests/voxel_host_main.cpp builds it alone under sanitizers).  A point's cell along one axis is floor(x / v): one IEEE float64 division and one
// floor, the arithmetic of np.floor(x / v) in harness/metrics.py.  Cells within (-2^20, 2^20) per axis are packed into 63 bits, so the all-ones
// word never is a key and marks an empty table slot.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define VOXKEY_HD __host__ __device__
#else
#define VOXKEY_HD
#endif

#define VOXEL_HALF 1048576L                        // 2^20: a cell index lies in (-VOXEL_HALF, VOXEL_HALF)
#define VOXEL_EMPTY 0xffffffffffffffffull          // the empty slot; bit 63 of every packed key is 0

// the cell of coordinate x for edge v -> *out; false (and *out untouched) when x / v is not finite or the cell lies outside (-2^20, 2^20)
VOXKEY_HD inline bool voxel_index(double x, double v, long* out) {
  const double f = floor(x / v);
  if (!(f > -(double)VOXEL_HALF && f < (double)VOXEL_HALF)) return false;      // a NaN fails both comparisons
  *out = (long)f;
  return true;
}
// 21 bits per axis, x highest; every field is in [1, 2^21 - 1]
VOXKEY_HD inline unsigned long long voxel_pack(long ix, long iy, long iz) {
  return ((unsigned long long)(ix + VOXEL_HALF) << 42) | ((unsigned long long)(iy + VOXEL_HALF) << 21) | (unsigned long long)(iz + VOXEL_HALF);
}
// the splitmix64 finaliser
VOXKEY_HD inline unsigned long long voxel_hash(unsigned long long x) {
  x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
  x ^= x >> 27; x *= 0x94d049bb133111ebull;
  x ^= x >> 31;
  return x;
}
// the key of a point, false when any coordinate is skipped
VOXKEY_HD inline bool voxel_key(double x, double y, double z, double v, unsigned long long* key) {
  long ix, iy, iz;
  if (!voxel_index(x, v, &ix) || !voxel_index(y, v, &iy) || !voxel_index(z, v, &iz)) return false;
  *key = voxel_pack(ix, iy, iz);
  return true;
}
