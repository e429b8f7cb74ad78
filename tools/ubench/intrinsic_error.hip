// The device intrinsics of csrc/train.hip that are not correctly rounded - erff, __expf, __logf, rsqrtf - each ALONE against double libm
// over the argument ranges the training-kernel tests use, plus sqrtf and the division (which are correctly rounded: 1.0000).  2^22
// arguments per range; errors in units of U = 2^-24.  tests/train_ref.py records the output and takes twice the maxima as its constants
// E_ERF / E_EXP / E_LOG / E_RSQRT; run it again after a compiler upgrade.
//   hipcc --offload-arch=gfx950 -O3 -o tools/ubench/intrinsic_error tools/ubench/intrinsic_error.hip && tools/ubench/intrinsic_error
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <vector>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); return 2; } } while (0)
__global__ void k(const float* x, float* y, int n, int f) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float v = x[i];
  y[i] = f == 0 ? erff(v) : f == 1 ? __expf(v) : f == 2 ? __logf(v) : f == 3 ? rsqrtf(v) : f == 4 ? sqrtf(v) : 1.0f / v;
}
int main() {
  const int n = 1 << 22;
  const double U = ldexp(1.0, -24);
  std::vector<float> x(n), y(n);
  float *dx, *dy;
  CK(hipMalloc(&dx, n * 4)); CK(hipMalloc(&dy, n * 4));
  struct R { const char* name; int f; double lo, hi; int logspace; } rs[] = {
    {"erff[-29,29]", 0, -29, 29, 0}, {"erff[-4,4]", 0, -4, 4, 0}, {"erff[1e-31,1]", 0, 1e-31, 1, 1},
    {"expf[-1,0]", 1, -1, 0, 0}, {"expf[-10,0]", 1, -10, 0, 0}, {"expf[-20,1]", 1, -20, 1, 0}, {"expf[-87,1]", 1, -87, 1, 0}, {"expf[-800,-87]", 1, -800, -87, 0},
    {"logf[1,8192]", 2, 1, 8192, 1}, {"logf[1,1.01]", 2, 1, 1.01, 0}, {"logf[1,2]", 2, 1, 2, 0},
    {"rsqrtf[1e-5,1e4]", 3, 1e-5, 1e4, 1}, {"sqrtf[1e-30,1e10]", 4, 1e-30, 1e10, 1}, {"rcp[1e-10,1e10]", 5, 1e-10, 1e10, 1}};
  for (auto& r : rs) {
    for (int i = 0; i < n; ++i) {
      double t = (i + 0.5) / n;
      x[i] = (float)(r.logspace ? r.lo * pow(r.hi / r.lo, t) : r.lo + (r.hi - r.lo) * t);
    }
    CK(hipMemcpy(dx, x.data(), n * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k, dim3(n / 256), dim3(256), 0, 0, dx, dy, n, r.f);
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(y.data(), dy, n * 4, hipMemcpyDeviceToHost));
    double mabs = 0, mrel = 0, mrelx = 0, mabslog = 0; float aabs = 0, arel = 0;
    for (int i = 0; i < n; ++i) {
      double v = x[i], t = r.f == 0 ? erf(v) : r.f == 1 ? exp(v) : r.f == 2 ? log(v) : r.f == 3 ? 1.0 / sqrt(v) : r.f == 4 ? sqrt(v) : 1.0 / v;
      double e = fabs((double)y[i] - t);
      if (e > mabs) { mabs = e; aabs = x[i]; }
      if (fabs(t) > 1e-37) {   // normal range of the result
        double rel = e / fabs(t);
        if (rel > mrel) { mrel = rel; arel = x[i]; }
        double rx = rel / (1.0 + fabs(v)); if (rx > mrelx) mrelx = rx;
      }
      double al = e / fmax(1.0, fabs(t)); if (al > mabslog) mabslog = al;
    }
    char line[512];
    snprintf(line, sizeof line, "%-20s max_abs/U %.4f (x=%g)  max_rel/U %.4f (x=%g)  max_rel/((1+|x|)U) %.4f  max_abs/(max(1,|f|)U) %.4f\n", r.name, mabs / U, aabs, mrel / U,
             arel, mrelx / U, mabslog / U);
    printf("%s", line);
  }
  return 0;
}
