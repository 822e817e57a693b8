// chol8.h - the 8 x 8 Cholesky solve of the damped normal-equation steps, stated once.
//
// THE RULE.  A x = b for a symmetric A given by its lower triangle, in fp64, one rounding per operation (build.py compiles
// every translation unit with -ffp-contract=off), in this order:
//   factor, column by column (j = 0 .. 7): d = A[j][j] - L[j][0]^2 - .. - L[j][j-1]^2, subtracted in ascending k;
//     ok = ok && d > 0 (a NaN fails); L[j][j] = sqrt(ok ? d : 1.0) - after a failed pivot the factor goes on with sqrt(1.0), so
//     nothing below divides by zero on account of it; then for i = j + 1 .. 7: L[i][j] = (A[i][j] - L[i][0] L[j][0] - .. -
//     L[i][j-1] L[j][j-1]) / L[j][j], ascending k.
//   forward, i = 0 .. 7:  y[i] = (b[i] - L[i][0] y[0] - .. - L[i][i-1] y[i-1]) / L[i][i], ascending k.
//   back, i = 7 .. 0:     x[i] = (y[i] - L[i+1][i] x[i+1] - .. - L[7][i] x[7]) / L[i][i], ascending k.
// ok carries the caller's own preconditions in and comes back false if they failed or any pivot was not > 0.  When ok is false
// x holds no solution: a caller must not let it reach an output.
//
// Called by prep_fit_kernel (prepare.hip), refine_step_kernel (refine.hip) and uvfit_step_kernel (uvfit.hip), every lane for
// itself in registers.  tests/chol8_ref.py restates it in numpy; tests/chol8_host_main.cpp runs this file on the CPU against
// that restatement, bit for bit.
//
// Plain C++, no HIP header: SFH_CHOL_FN marks what the device runs too.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define SFH_CHOL_FN __host__ __device__ __forceinline__
#else
#define SFH_CHOL_FN inline
#endif

// in: the lower triangle of Lm holds A, x holds b.  out: Lm holds the factor L, x the solution.  The upper triangle is not
// read.
SFH_CHOL_FN bool chol8_solve(double (&Lm)[8][8], double (&x)[8], bool ok) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    double d = Lm[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) d -= Lm[j][k] * Lm[j][k];
    ok = ok && (d > 0.0);
    const double dj = sqrt(ok ? d : 1.0);
    Lm[j][j] = dj;
#pragma unroll
    for (int i = j + 1; i < 8; ++i) {
      double v = Lm[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) v -= Lm[i][k] * Lm[j][k];
      Lm[i][j] = v / dj;
    }
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {          // L y = b
    double v = x[i];
#pragma unroll
    for (int k = 0; k < i; ++k) v -= Lm[i][k] * x[k];
    x[i] = v / Lm[i][i];
  }
#pragma unroll
  for (int i = 7; i >= 0; --i) {         // L^T x = y
    double v = x[i];
#pragma unroll
    for (int k = i + 1; k < 8; ++k) v -= Lm[k][i] * x[k];
    x[i] = v / Lm[i][i];
  }
  return ok;
}
