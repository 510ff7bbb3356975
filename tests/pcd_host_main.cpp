// Stand-alone driver of unigeo_amd/csrc/pcd_host.h for tests/test_pcd_cpu.py: reads 3x3 matrices H (nine numbers each) from standard input
// and prints, per matrix, the rotation of rotation_from_h (nine numbers) and the singular values of svd3 (three numbers).  A line that
// starts with "sums" instead carries the 17 Kabsch sums and is answered with the 16 numbers of umeyama_from_sums.  Built by the test with
// the host compiler and -fsanitize=address,undefined; no GPU code.
#include <stdio.h>
#include <string.h>

#include "../unigeo_amd/csrc/pcd_host.h"

int main() {
  char tag[16];
  while (scanf("%15s", tag) == 1) {
    if (strcmp(tag, "sums") == 0) {
      double a[17], T[16];
      for (int i = 0; i < 17; ++i) if (scanf("%lf", &a[i]) != 1) return 2;
      pcd_host::umeyama_from_sums(a, T);
      for (int i = 0; i < 16; ++i) printf("%.17g ", T[i]);
      printf("\n");
    } else if (strcmp(tag, "h") == 0) {
      double H[3][3], R[3][3], U[3][3], w[3], V[3][3];
      for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) if (scanf("%lf", &H[r][c]) != 1) return 2;
      pcd_host::rotation_from_h(H, R);
      pcd_host::svd3(H, U, w, V);
      for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) printf("%.17g ", R[r][c]);
      printf("%.17g %.17g %.17g\n", w[0], w[1], w[2]);
    } else {
      return 3;
    }
  }
  return 0;
}
