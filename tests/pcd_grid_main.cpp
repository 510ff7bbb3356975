// Stand-alone driver of grid_shape in unigeo_amd/csrc/pcd_host.h for tests/test_pcd_grid_cpu.py: every input line carries the count of finite
// points, their bounding box (min xyz, max xyz), the points per cell to aim at and the cap on the cell count, and is answered with the cell
// edge, the cells per axis, their product and the grid's origin.  Built by the test with the host compiler and -fsanitize=address,undefined;
// no GPU code.
#include <stdio.h>

#include "../unigeo_amd/csrc/pcd_host.h"

int main() {
  long n, cap;
  double box[6], occ;
  while (scanf("%ld", &n) == 1) {
    for (int i = 0; i < 6; ++i) if (scanf("%lf", &box[i]) != 1) return 2;
    if (scanf("%lf %ld", &occ, &cap) != 2) return 2;
    double mn[3], h;
    int G[3];
    long cells;
    pcd_host::grid_shape(box, n, occ, cap, mn, &h, G, &cells);
    printf("%.17g %d %d %d %ld %.17g %.17g %.17g\n", h, G[0], G[1], G[2], cells, mn[0], mn[1], mn[2]);
  }
  return 0;
}
