// The regularised quadric solve of the mesh decimators: csrc/simplify.hip places a cell's vertex with it,
// csrc/collapse.hip the vertex an edge collapses to.  One copy, so the two cannot drift apart.
#pragma once
#include "sfmi_common.h"

// x of (A + lam I) x = lam m - b for the symmetric A = (a00 a01 a02; . a11 a12; . . a22) with lam > 0: symmetric positive definite with
// condition <= 1 + trace(A) / lam, by the Cholesky factor L L^T.  Every product, sum, quotient and root is rounded on its own whatever
// the includer's setting, in this order: tests/simplify_ref.py and tests/collapse_ref.py restate it.  -> whether the three pivots were
// positive (x is computed either way; simplify.hip clamps it, collapse.hip refuses the edge).
__device__ __forceinline__ bool sfmi_quadric_solve(double a00, double a01, double a02, double a11, double a12, double a22, double b0,
                                                   double b1, double b2, double lam, const double (&m)[3], double (&x)[3]) {
#pragma clang fp contract(off)
  const double r0 = lam * m[0] - b0, r1 = lam * m[1] - b1, r2 = lam * m[2] - b2;
  const double d0 = a00 + lam;
  const double l00 = sqrt(d0);
  const double l10 = a01 / l00, l20 = a02 / l00;
  const double d1 = a11 + lam - l10 * l10;
  const double l11 = sqrt(d1);
  const double l21 = (a12 - l20 * l10) / l11;
  const double d2 = a22 + lam - l20 * l20 - l21 * l21;
  const double l22 = sqrt(d2);
  const double y0 = r0 / l00;
  const double y1 = (r1 - l10 * y0) / l11;
  const double y2 = (r2 - l20 * y0 - l21 * y1) / l22;
  x[2] = y2 / l22;
  x[1] = (y1 - l21 * x[2]) / l11;
  x[0] = (y0 - l10 * x[1] - l20 * x[2]) / l00;
  return d0 > 0.0 && d1 > 0.0 && d2 > 0.0;
}
