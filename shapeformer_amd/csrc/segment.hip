// Plane removal and Euclidean clustering of raw scans: what PCL / Open3D call segment_plane (RANSAC) and EuclideanClusterExtraction /
// cluster_dbscan.  The reference has no such step: its real-scan datasets (shapeformer/data/imnet_datasets/redwood.py, realtest.py)
// serve the clouds as they are read, floor and neighbouring clutter included.  DESIGN.md §5.17.
//
// 1. Plane scoring, H hypotheses x N points.  A hypothesis is three point indices; its plane and the inlier test are written once, in
//    f64 with no contraction, no square root and no division (seg_plane / the loop of ps_score_kernel), so numpy states the same
//    bits.  ps_init_kernel writes count = 0 (valid) or -1 (an index repeats or lies outside the set, or nn > 0 is false).
//    ps_score_kernel: grid (point chunks, hypothesis tiles, sets).  The tile's 64 planes (n, d, thr2 * nn) go to LDS once per
//    workgroup, 5 doubles each, read as broadcasts; a lane keeps 4 points in registers as f64 and walks the tile; the wave's count of
//    a hypothesis is the sum over the 4 points of popcount(ballot(inlier)), a scalar; lane h of the wave keeps the count of hypothesis h,
//    the four waves meet in LDS and one integer atomicAdd per (workgroup, hypothesis) reaches `count` (sfmi_commit_counts).
//    ps_best_kernel: one workgroup per set takes the arg max (sfmi_best_of_row: lowest h among equal counts) and settles the
//    status.  Integer atomics only: the result is a function
//    of the input.
// 2. Plane refit (Open3D's last step), one workgroup per set: the seed plane's inliers, their centroid and covariance in f64 by two
//    passes in a fixed order (a lane's points ascending, wave_sum_f64, a fixed tree over the 16 waves), the eigenvector of the smallest
//    eigenvalue by jacobi_rot (sfmi_ragged.h: the solver of knn_normals_kernel), the sign rule, and the final mask.
// 3. Euclidean clusters: connected components of the graph that joins two points of a set iff the f32 direct-form d2 of nn_kernel is
//    <= r2.  cl_init_kernel: parent[i] = i.  cl_hook_kernel: tiles (i block, j chunk >= i block) as nn_kernel tiles them (the j points
//    through a 256-point float4 LDS tile, the i points in registers); an accepted pair with j > i calls sfmi_uf_hook.  The tile's
//    fourth component carries parent[j] as it was when the tile was loaded and the lane keeps parent[i]: equal values mean a common
//    ancestor, so the pair is skipped without a load (a stale value is an older ancestor: the skip never drops a needed edge).
//    cl_flatten_kernel, a LATER launch as the header's protocol asks: root[i] = the root above i = the lowest index of i's cluster.
//
// Loop discipline: no kernel waits on another workgroup; every loop around a barrier has workgroup-uniform bounds; the only
// data-dependent loops are the union-find walks, whose termination argument is the header's (chains strictly descend).
#include "sfmi_ragged.h"   // the ragged-batch helpers and the RANSAC pieces shared with global_register.hip: DESIGN.md §5.5a

// the plane expressions are written once, here and in numpy: every product and sum rounded on its own
#pragma clang fp contract(off)

namespace {

constexpr int PS_THREADS = 256;
constexpr int PS_WAVES = PS_THREADS / 64;
constexpr int PS_R = 4;                          // points per lane, in registers as f64
constexpr int PS_CHUNK = PS_THREADS * PS_R;      // points per workgroup pass
constexpr int PS_HT = SFMI_HT;                   // hypotheses per tile
constexpr int RF_THREADS = 1024;
constexpr int RF_WAVES = RF_THREADS / 64;
constexpr int CL_THREADS = 256;
constexpr int CL_R = 2;                          // i points per lane
constexpr int CL_IB = CL_THREADS * CL_R;         // i points per block
constexpr int CL_TILE = 256;                     // j points per LDS tile
constexpr int CL_JC = 512;                       // j points per workgroup: equal to CL_IB, so block indices compare directly

// the plane through points i0, i1, i2 of the set that starts at Pb and has n points: normal (not unit), d = n . p0, nn = |n|^2.
// false (and nothing read out of bounds) when an index repeats or lies outside the set, or when nn > 0 is false (collinear, NaN)
__device__ __forceinline__ bool seg_plane(const float* __restrict__ Pb, long long n, int i0, int i1, int i2, double& nx, double& ny,
                                          double& nz, double& d, double& nn) {
  nx = ny = nz = d = nn = 0.0;
  if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= n || i1 >= n || i2 >= n || i0 == i1 || i0 == i2 || i1 == i2) return false;
  const double p0x = (double)Pb[3 * (long long)i0], p0y = (double)Pb[3 * (long long)i0 + 1], p0z = (double)Pb[3 * (long long)i0 + 2];
  const double ux = (double)Pb[3 * (long long)i1] - p0x, uy = (double)Pb[3 * (long long)i1 + 1] - p0y,
               uz = (double)Pb[3 * (long long)i1 + 2] - p0z;
  const double vx = (double)Pb[3 * (long long)i2] - p0x, vy = (double)Pb[3 * (long long)i2 + 1] - p0y,
               vz = (double)Pb[3 * (long long)i2 + 2] - p0z;
  nx = uy * vz - uz * vy;
  ny = uz * vx - ux * vz;
  nz = ux * vy - uy * vx;
  nn = (nx * nx + ny * ny) + nz * nz;
  d = (nx * p0x + ny * p0y) + nz * p0z;
  return nn > 0.0;
}

// ---- plane scoring ------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void ps_init_kernel(const float* __restrict__ P, const long long* __restrict__ off,
                                                      const int* __restrict__ triples, int B, int H, int* __restrict__ count,
                                                      int* __restrict__ status) {
  const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (long long)B * H) return;
  const int b = (int)(g / H);
  const long long base = off[b], n = off[b + 1] - base;
  double nx, ny, nz, d, nn;
  const bool ok = seg_plane(P + 3 * base, n, triples[3 * g], triples[3 * g + 1], triples[3 * g + 2], nx, ny, nz, d, nn);
  count[g] = ok ? 0 : -1;
  if (g % H == 0) status[b] = 0;
}

__global__ __launch_bounds__(PS_THREADS) void ps_score_kernel(const float* __restrict__ P, const long long* __restrict__ off,
                                                              const int* __restrict__ triples, int H, double thr2,
                                                              int* __restrict__ count, int* __restrict__ status) {
  __shared__ double pl[PS_HT][5];                              // (nx, ny, nz, d, thr2 * nn); an invalid hypothesis: (0, 0, 0, 0, -1)
  __shared__ int wc[PS_WAVES][PS_HT];
  const int b = blockIdx.z, tid = threadIdx.x, lane = tid & 63;
  const long long base = off[b], n = off[b + 1] - base;
  if ((long long)blockIdx.x * PS_CHUNK >= n) return;           // workgroup-uniform, before any barrier
  const int h0 = blockIdx.y * PS_HT;
  const float* Pb = P + 3 * base;
  if (tid < PS_HT) {
    const int h = h0 + tid;
    double nx = 0.0, ny = 0.0, nz = 0.0, d = 0.0, nn = 0.0;
    bool ok = false;
    if (h < H) {
      const int* t = triples + 3 * ((long long)b * H + h);
      ok = seg_plane(Pb, n, t[0], t[1], t[2], nx, ny, nz, d, nn);
    }
    pl[tid][0] = ok ? nx : 0.0;
    pl[tid][1] = ok ? ny : 0.0;
    pl[tid][2] = ok ? nz : 0.0;
    pl[tid][3] = ok ? d : 0.0;
    pl[tid][4] = ok ? thr2 * nn : -1.0;                        // s * s <= -1 never holds
  }
  __syncthreads();
  bool bad = false;
  for (long long c = blockIdx.x; c * PS_CHUNK < n; c += gridDim.x) {   // workgroup-uniform bounds
    double x[PS_R], y[PS_R], z[PS_R];
#pragma unroll
    for (int r = 0; r < PS_R; ++r) {
      const long long i = c * PS_CHUNK + r * PS_THREADS + tid;
      const bool in = i < n;
      x[r] = in ? (double)Pb[3 * i] : sfmi_nan_f64();          // padding: NaN is an inlier of nothing
      y[r] = in ? (double)Pb[3 * i + 1] : sfmi_nan_f64();
      z[r] = in ? (double)Pb[3 * i + 2] : sfmi_nan_f64();
      bad |= in && !sfmi_finite3(x[r], y[r], z[r]);
    }
    int mine = 0;
#pragma unroll 4
    for (int hh = 0; hh < PS_HT; ++hh) {
      const double nx = pl[hh][0], ny = pl[hh][1], nz = pl[hh][2], d = pl[hh][3], t = pl[hh][4];   // broadcast reads
      int cnt = 0;
#pragma unroll
      for (int r = 0; r < PS_R; ++r) {
        const double s = ((nx * x[r] + ny * y[r]) + nz * z[r]) - d;
        cnt += __popcll(__ballot(s * s <= t));
      }
      mine = lane == hh ? cnt : mine;
    }
    sfmi_commit_counts(wc, mine, count + (long long)b * H + h0);
  }
  if (blockIdx.y == 0 && __any(bad) && lane == 0) atomicOr(status + b, 2);
}

__global__ __launch_bounds__(SFMI_BEST_THREADS) void ps_best_kernel(int H, int* __restrict__ count, int* __restrict__ best,
                                                                    int* __restrict__ status) {
  const int b = blockIdx.x;
  int* row = count + (long long)b * H;
  const bool nonfinite = (status[b] & 2) != 0;                 // set by ps_score_kernel, an earlier launch; workgroup-uniform
  if (nonfinite)                                               // a lane reads back below what it wrote itself: no count is >= 0
    for (int h = threadIdx.x; h < H; h += SFMI_BEST_THREADS) row[h] = -1;
  int bc, bh;
  sfmi_best_of_row(row, H, bc, bh);
  if (threadIdx.x == 0) {
    best[b] = bc >= 0 ? bh : -1;
    status[b] = nonfinite ? 2 : (bc >= 0 ? 0 : 1);
  }
}

// ---- plane refit --------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(RF_THREADS) void rf_kernel(const float* __restrict__ P, const long long* __restrict__ off,
                                                        const int* __restrict__ triples, const int* __restrict__ best,
                                                        const int* __restrict__ status, const double* __restrict__ seed,
                                                        const double* __restrict__ up, int H, double thr, double thr2, int refit,
                                                        double* __restrict__ plane, unsigned char* __restrict__ inlier,
                                                        int* __restrict__ n_in) {
  __shared__ double red[RF_WAVES];
  const int b = blockIdx.x, tid = threadIdx.x;
  const long long base = off[b], n = off[b + 1] - base;
  const float* Pb = P + 3 * base;
  unsigned char* mask = inlier + base;
  // the seed plane, the same in every lane
  double nx = 0.0, ny = 0.0, nz = 0.0, d = 0.0, nn = 0.0;
  bool ok;
  if (seed) {
    nx = seed[4 * b]; ny = seed[4 * b + 1]; nz = seed[4 * b + 2]; d = -seed[4 * b + 3];
    nn = (nx * nx + ny * ny) + nz * nz;
    ok = nn > 0.0 && isfinite(nn) && isfinite(d);
  } else {
    const int h = best[b];
    ok = h >= 0 && h < H && (!status || status[b] == 0);
    if (ok) {
      const int* t = triples + 3 * ((long long)b * H + h);
      ok = seg_plane(Pb, n, t[0], t[1], t[2], nx, ny, nz, d, nn);
    }
  }
  const double t2 = ok ? thr2 * nn : -1.0;
  // pass 1: the seed's inliers by the scoring rule, their number and their sum
  double sx = 0.0, sy = 0.0, sz = 0.0, sc = 0.0;
  for (long long i = tid; i < n; i += RF_THREADS) {
    const double x = (double)Pb[3 * i], y = (double)Pb[3 * i + 1], z = (double)Pb[3 * i + 2];
    const double s = ((nx * x + ny * y) + nz * z) - d;
    const bool in = s * s <= t2;
    mask[i] = in ? 1 : 0;
    if (in) {
      sx += x; sy += y; sz += z; sc += 1.0;
    }
  }
  sx = sfmi_block_sum_f64<RF_WAVES>(sx, red); sy = sfmi_block_sum_f64<RF_WAVES>(sy, red); sz = sfmi_block_sum_f64<RF_WAVES>(sz, red);
  sc = sfmi_block_sum_f64<RF_WAVES>(sc, red);                  // whole numbers below 2^31: exact in f64
  const int cnt = (int)sc;
  if (!refit) {                                                // the seed's own mask is the result
    if (tid == 0) n_in[b] = cnt;
    return;
  }
  if (cnt < 3) {                                               // workgroup-uniform
    for (long long i = tid; i < n; i += RF_THREADS) mask[i] = 0;
    if (tid < 4) plane[4 * b + tid] = sfmi_nan_f64();
    if (tid == 0) n_in[b] = 0;
    return;
  }
  const double cx = sx / sc, cy = sy / sc, cz = sz / sc;
  // pass 2: the covariance about the centroid (each lane reads back the mask bytes it wrote itself)
  double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0;
  for (long long i = tid; i < n; i += RF_THREADS) {
    if (mask[i]) {
      const double x = (double)Pb[3 * i] - cx, y = (double)Pb[3 * i + 1] - cy, z = (double)Pb[3 * i + 2] - cz;
      a00 += x * x; a01 += x * y; a02 += x * z; a11 += y * y; a12 += y * z; a22 += z * z;
    }
  }
  a00 = sfmi_block_sum_f64<RF_WAVES>(a00, red) / sc; a01 = sfmi_block_sum_f64<RF_WAVES>(a01, red) / sc;
  a02 = sfmi_block_sum_f64<RF_WAVES>(a02, red) / sc; a11 = sfmi_block_sum_f64<RF_WAVES>(a11, red) / sc;
  a12 = sfmi_block_sum_f64<RF_WAVES>(a12, red) / sc; a22 = sfmi_block_sum_f64<RF_WAVES>(a22, red) / sc;
  double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;   // v[row][column]
  for (int sweep = 0; sweep < SFMI_JACOBI_SWEEPS; ++sweep) {
    jacobi_rot(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);   // (0, 1), third axis 2
    jacobi_rot(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);   // (0, 2), third axis 1
    jacobi_rot(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);   // (1, 2), third axis 0
  }
  // the column of the smallest eigenvalue (the first on a tie)
  const bool s1 = a11 < a00;
  double lam = s1 ? a11 : a00, ex = s1 ? v01 : v00, ey = s1 ? v11 : v10, ez = s1 ? v21 : v20;
  const bool s2 = a22 < lam;
  ex = s2 ? v02 : ex; ey = s2 ? v12 : ey; ez = s2 ? v22 : ez;
  const double inv = 1.0 / sqrt((ex * ex + ey * ey) + ez * ez);
  ex *= inv; ey *= inv; ez *= inv;
  bool flip;
  if (up) {
    flip = ((ex * up[3 * b] + ey * up[3 * b + 1]) + ez * up[3 * b + 2]) < 0.0;
  } else {
    double big = ex;
    if (fabs(ey) > fabs(big)) big = ey;
    if (fabs(ez) > fabs(big)) big = ez;
    flip = big < 0.0;
  }
  const double sg = flip ? -1.0 : 1.0;
  ex *= sg; ey *= sg; ez *= sg;
  const double dd = -((ex * cx + ey * cy) + ez * cz);
  // pass 3: the final mask
  int m = 0;
  for (long long i = tid; i < n; i += RF_THREADS) {
    const double x = (double)Pb[3 * i], y = (double)Pb[3 * i + 1], z = (double)Pb[3 * i + 2];
    const bool in = fabs(((ex * x + ey * y) + ez * z) + dd) <= thr;
    mask[i] = in ? 1 : 0;
    m += in ? 1 : 0;
  }
  const double mt = sfmi_block_sum_f64<RF_WAVES>((double)m, red);
  if (tid == 0) {
    plane[4 * b] = ex; plane[4 * b + 1] = ey; plane[4 * b + 2] = ez; plane[4 * b + 3] = dd;
    n_in[b] = (int)mt;
  }
}

// ---- Euclidean clusters -------------------------------------------------------------------------------------------------------------

__global__ void cl_init_kernel(const long long* __restrict__ off, int B, long long N, int* __restrict__ parent) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  parent[i] = (int)(i - off[sfmi_owner(off, B, i)]);
}

__global__ __launch_bounds__(CL_THREADS) void cl_hook_kernel(const float* __restrict__ P, const long long* __restrict__ off, float r2,
                                                             int* __restrict__ parent) {
  static_assert(CL_IB == CL_JC && CL_JC % CL_TILE == 0 && CL_TILE == CL_THREADS, "block indices of i and j compare directly");
  __shared__ float4 tile[CL_TILE];
  const int b = blockIdx.z, tid = threadIdx.x;
  const long long base = off[b];
  const int n = (int)(off[b + 1] - base);                      // below 2^31: the entry point's contract
  const float* Pb = P + 3 * base;
  int* par = parent + base;
  const float fnan = __int_as_float(0x7FC00000);
  // every bound below is workgroup-uniform
  for (long long ib = blockIdx.y; ib * CL_IB < n; ib += gridDim.y) {
    float px[CL_R], py[CL_R], pz[CL_R];
    int il[CL_R], pi[CL_R];
#pragma unroll
    for (int r = 0; r < CL_R; ++r) {
      const long long i = ib * CL_IB + r * CL_THREADS + tid;
      const bool in = i < n;
      il[r] = in ? (int)i : 0x7FFFFFFF;                        // padding: no j is greater
      px[r] = in ? Pb[3 * i] : fnan;
      py[r] = in ? Pb[3 * i + 1] : fnan;
      pz[r] = in ? Pb[3 * i + 2] : fnan;
      pi[r] = in ? sfmi_uf_load(par + i) : -1;
    }
    for (long long jc = blockIdx.x; jc * CL_JC < n; jc += gridDim.x) {
      if (jc < ib) continue;                                   // the pair of blocks belongs to the workgroup (jc, ib) mirrored
      for (int t = 0; t < CL_JC / CL_TILE; ++t) {
        const long long j0 = jc * CL_JC + (long long)t * CL_TILE;
        if (j0 >= n) break;
        __syncthreads();                                       // the previous tile is consumed
        {
          const long long j = j0 + tid;
          tile[tid] = j < n ? make_float4(Pb[3 * j], Pb[3 * j + 1], Pb[3 * j + 2], __int_as_float(sfmi_uf_load(par + j)))
                            : make_float4(fnan, fnan, fnan, __int_as_float(-2));
        }
        __syncthreads();
        for (int jj = 0; jj < CL_TILE; ++jj) {
          const float4 q = tile[jj];                           // broadcast ds_read_b128
          const int jl = (int)j0 + jj;
#pragma unroll
          for (int r = 0; r < CL_R; ++r) {
            const float dx = px[r] - q.x, dy = py[r] - q.y, dz = pz[r] - q.z;
            const float d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
            if (d2 <= r2 && jl > il[r] && __float_as_int(q.w) != pi[r]) {
              sfmi_uf_hook(par, il[r], jl);
              pi[r] = sfmi_uf_load(par + il[r]);
            }
          }
        }
      }
    }
  }
}

// a later launch than the hooks: the forest is final, and a slot that another lane has already flattened holds its root
__global__ void cl_flatten_kernel(const long long* __restrict__ off, int B, long long N, int* __restrict__ parent) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  int* par = parent + off[sfmi_owner(off, B, i)];
  int cur = (int)(parent + i - par), p = sfmi_uf_load(par + cur);
  while (p != cur) {
    cur = p;
    p = sfmi_uf_load(par + cur);
  }
  sfmi_uf_store(parent + i, cur);
}

}  // namespace

extern "C" {

int sfmi_plane_score_f32(const float* P, const long long* off, const int* triples, int B, long long N, int H, long long max_n,
                         double thr2, int* count, int* best, int* status, void* stream) {
  if (B <= 0 || B > (int)SFMI_MAX_GRID || N < 0 || H < 1 || cdiv(H, PS_HT) > SFMI_MAX_GRID || max_n < 0 || max_n >= (1ll << 31) ||
      !(thr2 >= 0.0) || !off || !triples || !count || !best || !status || (N > 0 && !P))
    return SFMI_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(ps_init_kernel, dim3(blocks256((long long)B * H)), dim3(256), 0, st, P, off, triples, B, H, count, status);
  if (N > 0)
    hipLaunchKernelGGL(ps_score_kernel, dim3(sfmi_grid_cap(cdiv(max_n, PS_CHUNK)), (unsigned)cdiv(H, PS_HT), (unsigned)B), dim3(PS_THREADS), 0,
                       st, P, off, triples, H, thr2, count, status);
  hipLaunchKernelGGL(ps_best_kernel, dim3((unsigned)B), dim3(SFMI_BEST_THREADS), 0, st, H, count, best, status);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_plane_refit_f32(const float* P, const long long* off, const int* triples, const int* best, const int* status,
                         const double* seed_plane, const double* up, int B, long long N, int H, double thr, int refit, double* plane,
                         unsigned char* inlier, int* n_in, void* stream) {
  if (B <= 0 || N < 0 || !(thr >= 0.0) || !off || !plane || !n_in || (N > 0 && (!P || !inlier))) return SFMI_EINVAL;
  if (!seed_plane && (H < 1 || !triples || !best)) return SFMI_EINVAL;
  hipLaunchKernelGGL(rf_kernel, dim3((unsigned)B), dim3(RF_THREADS), 0, (hipStream_t)stream, P, off, triples, best, status, seed_plane, up,
                     H, thr, thr * thr, refit, plane, inlier, n_in);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_cluster_f32(const float* P, const long long* off, int B, long long N, long long max_n, float r2, int* root, void* stream) {
  if (B <= 0 || B > (int)SFMI_MAX_GRID || N < 0 || max_n < 0 || max_n >= (1ll << 31) || !off) return SFMI_EINVAL;
  if (N == 0) return SFMI_OK;
  if (!P || !root) return SFMI_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(cl_init_kernel, dim3(blocks256(N)), dim3(256), 0, st, off, B, N, root);
  const unsigned nb = sfmi_grid_cap(cdiv(max_n, CL_IB));
  hipLaunchKernelGGL(cl_hook_kernel, dim3(nb, nb, (unsigned)B), dim3(CL_THREADS), 0, st, P, off, r2, root);
  hipLaunchKernelGGL(cl_flatten_kernel, dim3(blocks256(N)), dim3(256), 0, st, off, B, N, root);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

}  // extern "C"
