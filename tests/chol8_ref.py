"""numpy restatement (test infrastructure only) of csrc/chol8.h, the 8 x 8 Cholesky solve of the damped normal-equation steps:
the same contract, the same operation order, on Python floats (IEEE double, no contraction) with np.float64 for the square
root and the divisions (a Python division by zero raises; numpy's gives the inf or NaN the device gives).  Nothing here imports
the library.  prep_ref.refine_gn, refine_ref.lm_solve and uvfit_ref.solve call it; tests/test_chol8_host.py holds the header,
compiled for the host, against it bit for bit."""
import numpy as np


def chol8_solve(L, x, ok):
    """L: 8 x 8 list of lists whose lower triangle holds the system, x: list of the 8 right-hand sides; both are overwritten,
    L by the factor, x by the solution.  ok carries the caller's preconditions in; returned False if they failed or a pivot was
    not > 0 (a NaN fails; the factor goes on with sqrt(1.0)).  x is no solution when the result is False."""
    for i in range(8):
        x[i] = float(x[i])
        for k in range(i + 1):
            L[i][k] = float(L[i][k])
    ok = bool(ok)
    with np.errstate(all="ignore"):
        for j in range(8):
            d = L[j][j]
            for k in range(j):
                d -= L[j][k] * L[j][k]
            ok = ok and (d > 0.0)
            dj = float(np.sqrt(np.float64(d if ok else 1.0)))
            L[j][j] = dj
            for i in range(j + 1, 8):
                v = L[i][j]
                for k in range(j):
                    v -= L[i][k] * L[j][k]
                L[i][j] = float(np.float64(v) / np.float64(dj))
        for i in range(8):                  # L y = b
            v = x[i]
            for k in range(i):
                v -= L[i][k] * x[k]
            x[i] = float(np.float64(v) / np.float64(L[i][i]))
        for i in range(7, -1, -1):          # L^T x = y
            v = x[i]
            for k in range(i + 1, 8):
                v -= L[k][i] * x[k]
            x[i] = float(np.float64(v) / np.float64(L[i][i]))
    return ok
