// Stand-alone host program over unigeo_amd/csrc/kernels/voxkey.h, built by tests/test_pcd_scores_cpu.py with the system
// C++ compiler under -fsanitize=address,undefined.  stdin: the voxel edge, then one point "x y z" per line.  stdout per point: "1 ix iy iz key hash"
// (decimal; key and hash unsigned 64-bit) or "0" for a skipped point.  A non-zero exit: voxel_key disagrees with voxel_index / voxel_pack.
#include <cstdio>
#include <cstdlib>

#include "../unigeo_amd/csrc/kernels/voxkey.h"

int main() {
  double v = 0.0, p[3];
  if (scanf("%lf", &v) != 1) return 2;
  while (scanf("%lf %lf %lf", &p[0], &p[1], &p[2]) == 3) {
    long c[3] = {0, 0, 0};
    unsigned long long key = 0;
    const bool each = voxel_index(p[0], v, &c[0]) && voxel_index(p[1], v, &c[1]) && voxel_index(p[2], v, &c[2]);
    const bool whole = voxel_key(p[0], p[1], p[2], v, &key);
    if (each != whole) return 3;
    if (!whole) { printf("0\n"); continue; }
    if (key != voxel_pack(c[0], c[1], c[2]) || key == VOXEL_EMPTY) return 4;
    printf("1 %ld %ld %ld %llu %llu\n", c[0], c[1], c[2], key, voxel_hash(key));
  }
  return 0;
}
