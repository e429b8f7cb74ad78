// Hidden-point removal on the GPU (Katz, Tal, Basri 2007): which points of a stored cloud a camera sees.  The reference flips the
// cloud about a huge sphere around the camera and keeps the vertices of the convex hull of the flipped points plus the viewpoint
// (xgutils/geoutil.py:58-74 hidden_point_removal, scipy.spatial.ConvexHull), once per training item
// (shapeformer/data/partial.py:127-146 VirtualScanSelector).  Only hull-vertex MEMBERSHIP is needed, never the hull, and that is an
// independent question per point: exact brute force, in the style of pointdist.hip / meshsdf.hip.
//
// 1. Setup, per shape of a ragged batch: p = x - cam, n = |p|, R = max n * 10^param, f = p + 2 (R - n) p / n in f64, in numpy's
//    operation order with contraction off (the flipped points have magnitude ~3e4 and the decisive differences are ~1e-3: f32
//    flipping moves ~1 % of the hull).  f goes to the workspace as three arrays (x | y | z) so a wave reads 64 points coalesced.
// 2. Visibility, one wave per point i.  With the origin (the viewpoint after the shift) in the set, i is a hull vertex iff a
//    plane through f_i with normal w = u + a e1 + b e2 (u = f_i / |f_i|, e1, e2 an orthonormal complement) has every other point
//    strictly below it:  w . g_j <= -EPS for the unit directions g_j = (f_j - f_i) / |f_j - f_i|.  That is the feasibility of a
//    2-D linear program in (a, b), solved by Seidel's incremental algorithm with the constraints in a FIXED order (below):
//      scan   : the 64 lanes test 64 constraints at a time against the current optimum, __ballot finds the lowest violated one;
//      re-solve: the optimum moves onto that constraint's line; the 1-D program over all EARLIER constraints is a min / max
//               reduction across the lanes (each lane keeps its extreme ratios as fractions, one division per lane at the end).
//    Constraint order.  The caller may pass a permutation of each shape (hpr.py: a Morton sort of the viewing directions, so that
//    neighbours in the order are neighbours on the view sphere); the flipped cloud is stored in that order and point i takes its
//    constraints outwards from its own slot, 64-slot chunk by chunk.  The points that can refute i or pin its plane lie on nearby
//    view rays, so a hidden point is refuted in its first chunks and a visible point's optimum settles early: re-solves, which cost
//    the whole prefix, become rare late in the sequence (counted: DESIGN 5.8).  Feasibility does not depend on the order.
//    Both loops cost two or one dot products of f_j - f_i with wave-uniform vectors and an f32 length per constraint.
//    The objective (min a, then min b, inside a box) only makes the optimum unique.  Results do not depend on the launch geometry:
//    every coefficient is a function of (i, j) alone, the lowest violated index is taken, and min / max are order-free.
//    Exact duplicates: f_j == f_i gives a vacuous constraint, and a point with an earlier bitwise-equal copy is never visible
//    (the lowest index represents its class, as one member of it does in qhull's output).  Copies among the OTHER points give
//    identical constraints: when the line of one is re-solved against the other, the determinant is rounding residue, so a
//    determinant below 1e-13 of its scale counts as parallel (never a divisor), and a parallel pair is infeasible only beyond
//    a tolerance, never by `> 0`.
// 3. Resample for the selector: row k of shape b is the floor(u n_vis)-th visible point in ascending index order, u a counter
//    hash of (seed, shape, k); optional hash-normal jitter clipped to [-1, 1] (partial.py's _jitter); n_vis <= 2: all points.
#include "sfmi_ragged.h"   // the ragged-batch helpers the mesh tools share: DESIGN.md §5.5a

namespace {

constexpr double HPR_EPS = 1e-9;       // margin on the unit directions (the smallest margin of a true vertex seen is ~2e-7)
constexpr double HPR_BOX = 1e3;        // |a|, |b| <= BOX
constexpr double HPR_PAR_TOL = 1e-12;  // parallel constraints: infeasible only beyond this
constexpr double HPR_PAR_REL = 1e-13;  // a determinant this small against its two products is rounding residue: parallel
constexpr int HV_WAVES = 4;            // points (waves) per workgroup of the visibility launch
constexpr int HV_UN = 4;               // 64-constraint chunks in flight per wave
constexpr int HS_THREADS = 1024;

// ---- setup ------------------------------------------------------------------------------------------------------------------

// p = x - cam and n = sqrt((px^2 + py^2) + pz^2): numpy's `points - center` and np.linalg.norm(p, axis=1), operation for operation
template <typename T>
__device__ __forceinline__ double shifted_norm(const T* __restrict__ X, long long i, const double* __restrict__ cam, double& px,
                                               double& py, double& pz) {
#pragma clang fp contract(off)
  px = (double)X[3 * i] - cam[0];
  py = (double)X[3 * i + 1] - cam[1];
  pz = (double)X[3 * i + 2] - cam[2];
  const double sx = px * px, sy = py * py, sz = pz * pz;
  const double s = (sx + sy) + sz;
  return sqrt(s);
}

// one workgroup per shape: R[b] = max n * scale, status[b]: 0 ok, 1 fewer than 4 points, 2 a non-finite coordinate, 3 a point at the camera
template <typename T>
__global__ __launch_bounds__(HS_THREADS) void hpr_radius_kernel(const T* __restrict__ X, const long long* __restrict__ off,
                                                                const double* __restrict__ cam, double scale, double* __restrict__ R,
                                                                int* __restrict__ status) {
#pragma clang fp contract(off)
  __shared__ double smax[HS_THREADS];
  __shared__ int sflag[HS_THREADS];
  const int b = blockIdx.x, tid = threadIdx.x;
  const long long i0 = off[b], n = off[b + 1] - i0;
  double m = 0.0;
  int flag = 0;
  for (long long i = tid; i < n; i += HS_THREADS) {
    double px, py, pz;
    const double nr = shifted_norm(X, i0 + i, cam + 3 * b, px, py, pz);
    if (!(nr < INFINITY)) flag |= 1;            // inf or NaN
    else if (nr == 0.0) flag |= 2;
    else m = fmax(m, nr);
  }
  smax[tid] = m;
  sflag[tid] = flag;
  __syncthreads();
  for (int o = HS_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) {
      smax[tid] = fmax(smax[tid], smax[tid + o]);
      sflag[tid] |= sflag[tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const int fl = sflag[0];
    status[b] = n < 4 ? 1 : (fl & 1) ? 2 : (fl & 2) ? 3 : 0;
    R[b] = smax[0] * scale;
  }
}

// f = p + ((2 (R - n)) p) / n  (numpy evaluates `2.0 * (R - n)[:, None] * p / n[:, None]` left to right); zeros for a flagged shape.
// The flipped cloud is written in CONSTRAINT ORDER: slot r of a shape holds its point order[r] (order == NULL: the index order).
template <typename T>
__global__ void hpr_flip_kernel(const T* __restrict__ X, const long long* __restrict__ off, const double* __restrict__ cam,
                                const double* __restrict__ R, const int* __restrict__ status, const int* __restrict__ order, int B,
                                long long N, double* __restrict__ fx, double* __restrict__ fy, double* __restrict__ fz,
                                int* __restrict__ orig) {
#pragma clang fp contract(off)
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int b = sfmi_owner(off, B, i);
  const long long s0 = off[b], nb = off[b + 1] - s0;
  long long o = order ? (long long)order[i] : i - s0;            // slot i of the constraint order holds point o of its shape
  o = o < 0 ? 0 : (o >= nb ? nb - 1 : o);                        // a bad entry stays inside the shape
  orig[i] = (int)o;
  double x = 0.0, y = 0.0, z = 0.0;
  if (status[b] == 0) {
    double px, py, pz;
    const double nr = shifted_norm(X, s0 + o, cam + 3 * b, px, py, pz);
    const double k = 2.0 * (R[b] - nr);
    const double tx = k * px, ty = k * py, tz = k * pz;
    const double qx = tx / nr, qy = ty / nr, qz = tz / nr;
    x = px + qx;
    y = py + qy;
    z = pz + qz;
  }
  fx[i] = x;
  fy[i] = y;
  fz[i] = z;
}

// ---- visibility -------------------------------------------------------------------------------------------------------------

struct Basis { double ux, uy, uz, ax, ay, az, bx, by, bz; };   // u, e1, e2

// constraint of the direction g (not zero) in the point's basis:  al + be a + ga b <= 0  on the UNIT direction.  The length is
// taken in f32 (it only scales the constraint, 1e-7 relative on EPS).  g == 0 (a copy of the point itself): vacuous.
__device__ __forceinline__ void constraint(const Basis& s, double gx, double gy, double gz, double& al_, double& be, double& ga) {
  const double du = fma(gz, s.uz, fma(gy, s.uy, gx * s.ux));
  const double d1 = fma(gz, s.az, fma(gy, s.ay, gx * s.ax));
  const double d2 = fma(gz, s.bz, fma(gy, s.by, gx * s.bx));
  const float hx = (float)gx, hy = (float)gy, hz = (float)gz;
  const float n2 = fmaf(hz, hz, fmaf(hy, hy, hx * hx));
  const bool zero = gx == 0.0 && gy == 0.0 && gz == 0.0;
  const double r = zero ? 0.0 : (double)__builtin_amdgcn_rsqf(n2);    // v_rsq_f32: 1 ulp, the same bits wherever it is issued
  al_ = zero ? -1.0 : fma(du, r, HPR_EPS);
  be = d1 * r;
  ga = d2 * r;
}

// the r-th 64-slot chunk of a point's constraint sequence: its own chunk ci, then outwards ci + 1, ci - 1, ci + 2, ... and, once one
// end of the shape is reached, on along the other side
__device__ __forceinline__ int chunk_at(int r, int ci, int nch) {
  const int left = ci, right = nch - 1 - ci, m = left < right ? left : right;
  const int near = (r & 1) ? ci + ((r + 1) >> 1) : ci - (r >> 1), far = left > right ? ci - (r - m) : ci + (r - m);
  return r <= 2 * m ? near : far;
}

// one wave per point; grid = ceil(N / HV_WAVES) workgroups of HV_WAVES waves (consecutive points: they scan the same region of the
// flipped cloud at about the same time, so the loads of one wave are cache hits for the next)
__global__ __launch_bounds__(HV_WAVES * 64) void hpr_visible_kernel(const double* __restrict__ fx, const double* __restrict__ fy,
                                                                    const double* __restrict__ fz, const long long* __restrict__ off,
                                                                    const int* __restrict__ status, const int* __restrict__ orig, int B,
                                                                    long long N, unsigned char* __restrict__ vis,
                                                                    unsigned* __restrict__ evals) {
  const int lane = threadIdx.x & 63;
  // the wave index through readfirstlane: everything derived from it (shape, slot, chunk sequence, loop bounds) stays in scalar registers
  const long long i = (long long)blockIdx.x * HV_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (i >= N) return;
  const int b = sfmi_owner(off, B, i);
  const long long s0 = off[b];
  const int n = (int)(off[b + 1] - s0), li = (int)(i - s0);      // N_b < 2^31 (checked on the host)
  const int* __restrict__ O = orig + s0;
  const int my = O[li];                                          // the point's index in its shape; li is its slot in the constraint order
  const long long out = s0 + my;
  if (status[b] != 0) {
    if (lane == 0) {
      vis[out] = 0;
      if (evals) evals[2 * out] = evals[2 * out + 1] = 0;
    }
    return;
  }
  const int nch = (n + 63) >> 6, ci = li >> 6;                   // 64-slot chunks; the point's own chunk comes first
  unsigned n_scan = 0, n_solve = 0;                              // constraint evaluations spent on this point (for the benchmark)
  const double* __restrict__ X = fx + s0;
  const double* __restrict__ Y = fy + s0;
  const double* __restrict__ Z = fz + s0;
  const double pix = X[li], piy = Y[li], piz = Z[li];
  Basis s;
  {
    const double inv = 1.0 / sqrt(fma(piz, piz, fma(piy, piy, pix * pix)));
    s.ux = pix * inv; s.uy = piy * inv; s.uz = piz * inv;
    const double amx = fabs(s.ux), amy = fabs(s.uy), amz = fabs(s.uz);
    const int ax = (amx <= amy && amx <= amz) ? 0 : (amy <= amz ? 1 : 2);      // np.argmin: the first minimum
    const double ex = ax == 0 ? 1.0 : 0.0, ey = ax == 1 ? 1.0 : 0.0, ez = ax == 2 ? 1.0 : 0.0;
    double cx = s.uy * ez - s.uz * ey, cy = s.uz * ex - s.ux * ez, cz = s.ux * ey - s.uy * ex;
    const double cinv = 1.0 / sqrt(fma(cz, cz, fma(cy, cy, cx * cx)));
    s.ax = cx * cinv; s.ay = cy * cinv; s.az = cz * cinv;
    s.bx = s.uy * s.az - s.uz * s.ay; s.by = s.uz * s.ax - s.ux * s.az; s.bz = s.ux * s.ay - s.uy * s.ax;
  }
  double a = -HPR_BOX, bq = -HPR_BOX;                            // current optimum
  int j = 0;                                                     // constraints [0, j) hold at (a, bq)
  bool ok = true;
  while (ok) {
    // normal of the current plane: every constraint is  g . w + EPS |g| <= 0
    const double wx = fma(bq, s.bx, fma(a, s.ax, s.ux)), wy = fma(bq, s.by, fma(a, s.ay, s.uy)), wz = fma(bq, s.bz, fma(a, s.az, s.uz));
    int found = -1;
    for (int r0 = j >> 6; r0 < nch && found < 0 && ok; r0 += HV_UN) {
      double gx[HV_UN], gy[HV_UN], gz[HV_UN];
      unsigned kq[HV_UN];
      bool inside[HV_UN];
#pragma unroll
      for (int c = 0; c < HV_UN; ++c) {
        const unsigned k = (unsigned)(chunk_at(r0 + c < nch ? r0 + c : nch - 1, ci, nch) * 64 + lane), kk = k < (unsigned)n ? k : (unsigned)n - 1;
        kq[c] = kk;
        inside[c] = k < (unsigned)n && r0 + c < nch;
        gx[c] = X[kk] - pix; gy[c] = Y[kk] - piy; gz[c] = Z[kk] - piz;
      }
      unsigned long long viol[HV_UN], dup = 0;
#pragma unroll
      for (int c = 0; c < HV_UN; ++c) {
        const int q = (r0 + c) * 64 + lane;                      // position in the constraint sequence
        const bool valid = q >= j && inside[c];
        const float hx = (float)gx[c], hy = (float)gy[c], hz = (float)gz[c];
        const double len = (double)__builtin_amdgcn_sqrtf(fmaf(hz, hz, fmaf(hy, hy, hx * hx)));   // v_sqrt_f32
        const double t = fma(len, HPR_EPS, fma(gz[c], wz, fma(gy[c], wy, gx[c] * wx)));
        const bool zero = gx[c] == 0.0 && gy[c] == 0.0 && gz[c] == 0.0;
        viol[c] = __ballot(valid && !zero && t > 0.0);
        int other = 0x7FFFFFFF;
        if (valid && zero) other = O[kq[c]];                     // a copy of the point (or the point itself): rare
        dup |= __ballot(other < my);
        n_scan += (unsigned)__popcll(__ballot(valid));
      }
      if (dup) ok = false;                                       // a lower index holds the same point
#pragma unroll
      for (int c = HV_UN - 1; c >= 0; --c)
        if (viol[c]) found = (r0 + c) * 64 + __builtin_ctzll(viol[c]);
    }
    if (!ok || found < 0) break;
    // re-solve on the line of constraint `found` (a sequence position) over the constraints before it
    double alj, bej, gaj;
    const int kf = chunk_at(found >> 6, ci, nch) * 64 + (found & 63);
    constraint(s, X[kf] - pix, Y[kf] - piy, Z[kf] - piz, alj, bej, gaj);
    const double nn = fma(gaj, gaj, bej * bej);
    if (!(nn > 0.0)) { ok = false; break; }                      // f_found straight behind f_i: no such plane
    const double p0x = -alj * bej / nn, p0y = -alj * gaj / nn, d0 = -gaj, d1 = bej;
    n_solve += (unsigned)found;
    // On the line (a, b) = p0 + t d the unit-direction constraint of g reads  t (g . Dv) + g . Pv + EPS |g| <= 0  (times |g| > 0):
    // two dot products with wave-uniform vectors, as in the scan.
    const double Dx = fma(d1, s.bx, d0 * s.ax), Dy = fma(d1, s.by, d0 * s.ay), Dz = fma(d1, s.bz, d0 * s.az);
    const double Px = fma(p0y, s.bx, fma(p0x, s.ax, s.ux)), Py = fma(p0y, s.by, fma(p0x, s.ay, s.uy)), Pz = fma(p0y, s.bz, fma(p0x, s.az, s.uz));
    const double par_scale = HPR_PAR_REL * sqrt(nn);
    double hn = INFINITY, hd = 1.0, ln = -INFINITY, ld = 1.0;    // upper / lower bound of t as fractions, hd, ld > 0
    bool bad = false;
    for (int r0 = 0; r0 * 64 < found; r0 += HV_UN) {
      double gx[HV_UN], gy[HV_UN], gz[HV_UN];
      bool inside[HV_UN];
#pragma unroll
      for (int c = 0; c < HV_UN; ++c) {
        const unsigned k = (unsigned)(chunk_at(r0 + c < nch ? r0 + c : nch - 1, ci, nch) * 64 + lane), kk = k < (unsigned)n ? k : (unsigned)n - 1;
        inside[c] = k < (unsigned)n;
        gx[c] = X[kk] - pix; gy[c] = Y[kk] - piy; gz[c] = Z[kk] - piz;
      }
#pragma unroll
      for (int c = 0; c < HV_UN; ++c) {
        const int q = (r0 + c) * 64 + lane;
        const float hx = (float)gx[c], hy = (float)gy[c], hz = (float)gz[c];
        const double len = (double)__builtin_amdgcn_sqrtf(fmaf(hz, hz, fmaf(hy, hy, hx * hx)));
        const double den = fma(gz[c], Dz, fma(gy[c], Dy, gx[c] * Dx));
        const double num = fma(len, HPR_EPS, fma(gz[c], Pz, fma(gy[c], Py, gx[c] * Px)));
        const bool zero = gx[c] == 0.0 && gy[c] == 0.0 && gz[c] == 0.0;
        if (q < found && inside[c] && !zero) {
          if (fabs(den) <= par_scale * len) {                    // parallel to the line within rounding (a copy of `found` is): never divide
            if (num > HPR_PAR_TOL * len) bad = true;
          } else if (den > 0.0) {
            const double m = -num;
            if (m * hd < hn * den) { hn = m; hd = den; }
          } else {
            const double dd = -den;
            if (num * ld > ln * dd) { ln = num; ld = dd; }
          }
        }
      }
    }
    double hi = wave_min_f64(hn / hd), lo = wave_max_f64(ln / ld);
    const double bA[4] = {d0, -d0, d1, -d1}, bC[4] = {p0x - HPR_BOX, -p0x - HPR_BOX, p0y - HPR_BOX, -p0y - HPR_BOX};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (bA[q] > 0.0) hi = fmin(hi, -bC[q] / bA[q]);
      else if (bA[q] < 0.0) lo = fmax(lo, -bC[q] / bA[q]);
      else if (bC[q] > HPR_PAR_TOL) bad = true;
    }
    if (__any(bad || !(lo <= hi))) { ok = false; break; }       // the same in every lane; __any tells the compiler so (j, found stay scalar)
    const double t = d0 > 0.0 ? lo : d0 < 0.0 ? hi : d1 > 0.0 ? lo : hi;       // min a, then min b
    a = fma(t, d0, p0x);
    bq = fma(t, d1, p0y);
    j = found + 1;
  }
  if (lane == 0) {
    vis[out] = ok ? 1 : 0;
    if (evals) {
      evals[2 * out] = n_scan;
      evals[2 * out + 1] = n_solve;
    }
  }
}

// count[b] = visible points of shape b, summed in a fixed order (one workgroup per shape)
__global__ __launch_bounds__(256) void hpr_count_kernel(const unsigned char* __restrict__ vis, const long long* __restrict__ off,
                                                        int* __restrict__ count) {
  __shared__ int sums[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const long long i0 = off[b], i1 = off[b + 1];
  int c = 0;
  for (long long i = i0 + tid; i < i1; i += 256) c += vis[i];
  sums[tid] = c;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) sums[tid] += sums[tid + o];
    __syncthreads();
  }
  if (tid == 0) count[b] = sums[0];
}

// ---- resample ---------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ unsigned mix32(unsigned h) {
  h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
  return h;
}

// one thread per output row.  prefix: exclusive prefix sum of vis over the whole ragged batch (prefix[i] = visible points before i)
template <typename T>
__global__ void hpr_resample_kernel(const T* __restrict__ X, const unsigned char* __restrict__ vis, const int* __restrict__ prefix,
                                    const long long* __restrict__ off, const int* __restrict__ count, int B, int ctx, unsigned seed,
                                    int shape0, float noise, float* __restrict__ out) {
  const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (long long)B * ctx) return;
  const int b = (int)(g / ctx);
  const unsigned k = (unsigned)(g - (long long)b * ctx);
  const long long i0 = off[b], nb = off[b + 1] - i0;
  if (nb <= 0) {
    out[3 * g] = out[3 * g + 1] = out[3 * g + 2] = __int_as_float(0x7FC00000);
    return;
  }
  const unsigned sb = mix32(seed * 0x9E3779B1u + (unsigned)(shape0 + b) * 0x85EBCA6Bu + 0x27D4EB2Fu);   // (seed, shape) only
  const float u = sfmi_hash_unit(sb, k);
  const int nv = count[b];
  long long src;
  if (nv <= 2) {                                                 // the reference's fallback: the whole cloud
    long long r = (long long)((double)u * (double)nb);
    src = i0 + (r < nb ? r : nb - 1);
  } else {
    int r = (int)((double)u * (double)nv);
    r = r < nv ? r : nv - 1;
    const int want = prefix[i0] + r;                             // the largest index with prefix <= want is the r-th visible point
    long long lo = i0, hi = i0 + nb - 1;
    while (lo < hi) {
      const long long mid = (lo + hi + 1) >> 1;
      if (prefix[mid] <= want) lo = mid; else hi = mid - 1;
    }
    src = lo;
  }
#pragma unroll
  for (int ax = 0; ax < 3; ++ax) {
    float v = (float)X[3 * src + ax];
    if (noise > 0.f) {
      const unsigned c = 2u * (3u * k + (unsigned)ax);
      const float u1 = 1.0f - sfmi_hash_unit(sb ^ 0x68E31DA4u, c);           // (0, 1]
      const float u2 = sfmi_hash_unit(sb ^ 0x68E31DA4u, c + 1u);
      v = fmaf(noise, sqrtf(-2.f * logf(u1)) * cospif(2.f * u2), v);
      v = fminf(fmaxf(v, -1.f), 1.f);
    }
    out[3 * g + ax] = v;
  }
}

struct HprWs { double *fx, *fy, *fz, *R; int* orig; };

// workspace: flipped x | y | z (N f64 each, in constraint order) | R (B f64) | the point of each slot (N int32)
HprWs hpr_ws(SfmiCarver& c, int B, long long N) {
  const size_t n = (size_t)(N > 0 ? N : 1);
  return {c.take<double>(n), c.take<double>(n), c.take<double>(n), c.take<double>((size_t)B), c.take<int>(n)};   // in this order
}

}  // namespace

extern "C" {

size_t sfmi_hpr_workspace_bytes(int B, long long N) {
  if (B <= 0 || N < 0) return 0;
  return sfmi_ws_bytes(hpr_ws, B, N);
}

int sfmi_hpr_visible(const void* X, int is_f64, const long long* off, const double* cam, const int* order, int B, long long N, double param,
                     unsigned char* visible, int* count, int* status, unsigned* evals, void* workspace, void* stream) {
  if (B <= 0 || N < 0 || N >= (1ll << 31) || !off || !cam || !count || !status || !workspace) return SFMI_EINVAL;
  if (N > 0 && (!X || !visible)) return SFMI_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  SfmiCarver carver{(char*)workspace};
  const auto [fx, fy, fz, R, orig] = hpr_ws(carver, B, N);
  if (N > 0 && order) SFMI_TRY(hipMemsetAsync(visible, 0, (size_t)N, st));     // an `order` that is no permutation leaves no byte unwritten
  const double scale = pow(10.0, param);
  const unsigned fb = (unsigned)cdiv(N, 256), vb = (unsigned)cdiv(N, HV_WAVES);
  if (is_f64) {
    hipLaunchKernelGGL(hpr_radius_kernel<double>, dim3((unsigned)B), dim3(HS_THREADS), 0, st, (const double*)X, off, cam, scale, R, status);
    if (N > 0)
      hipLaunchKernelGGL(hpr_flip_kernel<double>, dim3(fb), dim3(256), 0, st, (const double*)X, off, cam, (const double*)R,
                         (const int*)status, order, B, N, fx, fy, fz, orig);
  } else {
    hipLaunchKernelGGL(hpr_radius_kernel<float>, dim3((unsigned)B), dim3(HS_THREADS), 0, st, (const float*)X, off, cam, scale, R, status);
    if (N > 0)
      hipLaunchKernelGGL(hpr_flip_kernel<float>, dim3(fb), dim3(256), 0, st, (const float*)X, off, cam, (const double*)R,
                         (const int*)status, order, B, N, fx, fy, fz, orig);
  }
  if (N > 0)
    hipLaunchKernelGGL(hpr_visible_kernel, dim3(vb), dim3(HV_WAVES * 64), 0, st, (const double*)fx, (const double*)fy, (const double*)fz, off,
                       (const int*)status, (const int*)orig, B, N, visible, evals);
  hipLaunchKernelGGL(hpr_count_kernel, dim3((unsigned)B), dim3(256), 0, st, (const unsigned char*)visible, off, count);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_hpr_resample_f32(const void* X, int is_f64, const unsigned char* visible, const int* prefix, const long long* off,
                          const int* count, int B, long long N, int context_N, unsigned seed, int shape0, float noise, float* out,
                          void* stream) {
  if (B <= 0 || N < 0 || N >= (1ll << 31) || context_N < 0 || shape0 < 0 || !off || !count || !(noise >= 0.f)) return SFMI_EINVAL;
  if (context_N == 0) return SFMI_OK;
  if (!out || (N > 0 && (!X || !visible || !prefix))) return SFMI_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const unsigned blocks = (unsigned)cdiv((long long)B * context_N, 256);
  if (is_f64)
    hipLaunchKernelGGL(hpr_resample_kernel<double>, dim3(blocks), dim3(256), 0, st, (const double*)X, visible, prefix, off, count, B,
                       context_N, seed, shape0, noise, out);
  else
    hipLaunchKernelGGL(hpr_resample_kernel<float>, dim3(blocks), dim3(256), 0, st, (const float*)X, visible, prefix, off, count, B,
                       context_N, seed, shape0, noise, out);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

}  // extern "C"
