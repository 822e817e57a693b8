// chol8_host_main.cpp - the 8 x 8 Cholesky solve of csrc/chol8.h run on the host: the function prep_fit_kernel,
// refine_step_kernel and uvfit_step_kernel call.  Built and run by tests/test_chol8_host.py with -fsanitize=address,undefined
// and -ffp-contract=off (the library's own setting); it links nothing of the library.
//
//   chol8_host_main < SYSTEMS
//
// SYSTEMS: per system 45 tokens separated by white space - the 36 values of the lower triangle row by row (L[0][0], L[1][0],
// L[1][1], L[2][0], ..) and the 8 right-hand sides as C99 hexadecimal doubles (or inf / nan), then the incoming ok (0 / 1).
// Per system one line: ok (0 / 1) and the 8 words of x as 16 hexadecimal digits each.  The upper triangle is handed over as
// NaN: the solve does not read it.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../sports-field-homography_amd/csrc/chol8.h"

int main() {
  for (;;) {
    double L[8][8], x[8];
    int ok = 0, got = 0;
    for (int i = 0; i < 8; ++i)
      for (int k = 0; k < 8; ++k) {
        L[i][k] = NAN;
        if (k <= i) got += scanf("%la", &L[i][k]) == 1;
      }
    if (got == 0 && feof(stdin)) return 0;
    for (int i = 0; i < 8; ++i) got += scanf("%la", &x[i]) == 1;
    got += scanf("%d", &ok) == 1;
    if (got != 45) {
      fprintf(stderr, "a system of %d tokens (45 expected)\n", got);
      return 2;
    }
    printf("%d", chol8_solve(L, x, ok != 0) ? 1 : 0);
    for (int i = 0; i < 8; ++i) {
      uint64_t w;
      memcpy(&w, &x[i], 8);
      printf(" %016llx", (unsigned long long)w);
    }
    printf("\n");
  }
}
