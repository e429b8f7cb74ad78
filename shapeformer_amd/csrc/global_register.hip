// Global registration of partial scans: RANSAC over feature correspondences for ragged batches of (source, target) pairs, what Open3D
// calls registration_ransac_based_on_feature_matching.  It gives register.hip's ICP a start inside its basin.  The reference has no
// such step: its real-scan datasets (shapeformer/data/imnet_datasets/redwood.py, realtest.py) serve one cloud in one frame.
// DESIGN.md §5.19; the contract is stated in include/sfmi.h and restated in numpy in tests/global_reg_ref.py.
//
// A correspondence is a pair (source index, target index) local to the pair's sets; a hypothesis is a triple of correspondences.
// 1. greg_pose_kernel: one lane per hypothesis.  The validity rules, then the least-squares rigid motion of the three pairs (Kabsch,
//    proper rotation) in f64.  The cross-covariance of three pairs has rank 2, so its singular vectors come from a one-sided Jacobi
//    iteration on its columns (squaring it first would square its condition number), and the third pair of singular vectors is the
//    cross product of the first two on either side: the rotation is proper by construction.
// 2. greg_score_kernel, built as segment.hip's ps_score_kernel and ending in the same sfmi_commit_counts (sfmi_ragged.h): grid
//    (correspondence chunks, hypothesis tiles, pairs).  The tile's 64 poses
//    go to LDS once per workgroup, read as broadcasts; a lane keeps 4 correspondences in registers; the wave's count of a hypothesis is
//    the sum over the 4 of popcount(ballot(inlier)); lane h keeps the count of hypothesis h, the four waves meet in LDS and one integer
//    atomicAdd per (workgroup, hypothesis) reaches `count`.  greg_best_kernel: sfmi_best_of_row, the lowest h among equal counts.
// 3. greg_refit_kernel, one workgroup per pair: the winner's inliers, their two centroids and the 9 centred cross terms in f64 by two
//    passes in a fixed order (a lane's correspondences ascending, wave_sum_f64, a fixed tree over the 16 waves), Kabsch again, and the
//    final mask under the refit pose.  A batch equals per-pair calls bit for bit.
// The transform is register.hip's (x' = f32(((r0 x + r1 y) + r2 z) + t) in f64) and d2 is nn_dist's f32 fmaf form, so an inlier here is
// an inlier of evaluate_registration_dev's correspondence at the same pose.
//
// Loop discipline: no kernel waits on another workgroup, there are no spins, every loop around a barrier has workgroup-uniform
// bounds.  Integer atomics only.  An index is range-checked before the point it names is read.
#include "sfmi_ragged.h"   // the ragged-batch helpers, the pose row and the RANSAC pieces shared with segment.hip: DESIGN.md §5.5a

// the transform and the inlier test are written once, here and in numpy: every product and sum rounded on its own
#pragma clang fp contract(off)

namespace {

constexpr int GS_THREADS = 256;
constexpr int GS_WAVES = GS_THREADS / 64;
constexpr int GS_R = 4;                          // correspondences per lane
constexpr int GS_CHUNK = GS_THREADS * GS_R;      // correspondences per workgroup pass
constexpr int GS_HT = SFMI_HT;                   // hypotheses per tile
constexpr int GR_THREADS = 1024;
constexpr int GR_WAVES = GR_THREADS / 64;
constexpr int GR_NS = 16;                        // count | sum s (3) | sum q (3) | centred cross terms (9, row-major q x s)
constexpr double GR_RANK_TOL = 1e-12;            // sigma_2 <= tol x sigma_1: degenerate

// one rotation of a one-sided Jacobi iteration: columns p and q of m (and of the accumulated v) are turned so that they are orthogonal
__device__ __forceinline__ void gr_rot(double& m0p, double& m1p, double& m2p, double& m0q, double& m1q, double& m2q, double& v0p, double& v1p,
                                       double& v2p, double& v0q, double& v1q, double& v2q) {
  const double al = (m0p * m0p + m1p * m1p) + m2p * m2p, be = (m0q * m0q + m1q * m1q) + m2q * m2q;
  const double ga = (m0p * m0q + m1p * m1q) + m2p * m2q;
  const double theta = (be - al) / (2.0 * ga);
  double t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));      // |theta| huge: t -> 0
  t = ga == 0.0 ? 0.0 : t;
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  const double a0 = c * m0p - s * m0q, b0 = s * m0p + c * m0q, a1 = c * m1p - s * m1q, b1 = s * m1p + c * m1q;
  const double a2 = c * m2p - s * m2q, b2 = s * m2p + c * m2q;
  m0p = a0; m0q = b0; m1p = a1; m1q = b1; m2p = a2; m2q = b2;
  const double e0 = c * v0p - s * v0q, f0 = s * v0p + c * v0q, e1 = c * v1p - s * v1q, f1 = s * v1p + c * v1q;
  const double e2 = c * v2p - s * v2q, f2 = s * v2p + c * v2q;
  v0p = e0; v0q = f0; v1p = e1; v1q = f1; v2p = e2; v2q = f2;
}

__device__ __forceinline__ void gr_swap(double& a, double& b) { const double t = a; a = b; b = t; }

// M = U S V^T of a 3x3 by one-sided Jacobi.  In: m (row-major).  Out: the columns of m are sigma_i u_i and the columns of v are v_i,
// ordered so that sg[0] >= sg[1] >= sg[2] (sg = the column norms)
__device__ __forceinline__ void gr_svd3(double (&m)[9], double (&v)[9], double (&sg)[3]) {
  v[0] = 1.0; v[1] = 0.0; v[2] = 0.0; v[3] = 0.0; v[4] = 1.0; v[5] = 0.0; v[6] = 0.0; v[7] = 0.0; v[8] = 1.0;
  for (int sweep = 0; sweep < SFMI_JACOBI_SWEEPS; ++sweep) {
    gr_rot(m[0], m[3], m[6], m[1], m[4], m[7], v[0], v[3], v[6], v[1], v[4], v[7]);   // columns (0, 1)
    gr_rot(m[0], m[3], m[6], m[2], m[5], m[8], v[0], v[3], v[6], v[2], v[5], v[8]);   // columns (0, 2)
    gr_rot(m[1], m[4], m[7], m[2], m[5], m[8], v[1], v[4], v[7], v[2], v[5], v[8]);   // columns (1, 2)
  }
  sg[0] = sqrt((m[0] * m[0] + m[3] * m[3]) + m[6] * m[6]);
  sg[1] = sqrt((m[1] * m[1] + m[4] * m[4]) + m[7] * m[7]);
  sg[2] = sqrt((m[2] * m[2] + m[5] * m[5]) + m[8] * m[8]);
#define GR_ORDER(p, q)                                                                                                     \
  if (sg[q] > sg[p]) {                                                                                                     \
    gr_swap(sg[p], sg[q]);                                                                                                 \
    gr_swap(m[p], m[q]); gr_swap(m[3 + p], m[3 + q]); gr_swap(m[6 + p], m[6 + q]);                                         \
    gr_swap(v[p], v[q]); gr_swap(v[3 + p], v[3 + q]); gr_swap(v[6 + p], v[6 + q]);                                         \
  }
  GR_ORDER(0, 1) GR_ORDER(0, 2) GR_ORDER(1, 2)
#undef GR_ORDER
}

// The proper rotation R and translation t that take the source onto the target in the least-squares sense, from the centred
// cross-covariance M = sum q' s'^T (row-major, target rows x source columns) and the two centroids: M = U S V^T, u3 = u1 x u2,
// v3 = v1 x v2, R = sum u_i v_i^T, t = cq - R cs.  false (pose untouched) when sigma_2 <= 1e-12 sigma_1 or something is not finite.
__device__ __forceinline__ bool gr_kabsch(const double (&M)[9], const double (&cs)[3], const double (&cq)[3], double (&pose)[12]) {
  double m[9], v[9], sg[3];
#pragma unroll
  for (int e = 0; e < 9; ++e) m[e] = M[e];
  gr_svd3(m, v, sg);
  if (!(sg[0] > 0.0) || !(sg[1] > GR_RANK_TOL * sg[0]) || !isfinite(sg[0])) return false;
  const double u1x = m[0] / sg[0], u1y = m[3] / sg[0], u1z = m[6] / sg[0];
  const double u2x = m[1] / sg[1], u2y = m[4] / sg[1], u2z = m[7] / sg[1];
  const double u3x = u1y * u2z - u1z * u2y, u3y = u1z * u2x - u1x * u2z, u3z = u1x * u2y - u1y * u2x;
  const double v1x = v[0], v1y = v[3], v1z = v[6], v2x = v[1], v2y = v[4], v2z = v[7];
  const double v3x = v1y * v2z - v1z * v2y, v3y = v1z * v2x - v1x * v2z, v3z = v1x * v2y - v1y * v2x;
  const double R[9] = {(u1x * v1x + u2x * v2x) + u3x * v3x, (u1x * v1y + u2x * v2y) + u3x * v3y, (u1x * v1z + u2x * v2z) + u3x * v3z,
                       (u1y * v1x + u2y * v2x) + u3y * v3x, (u1y * v1y + u2y * v2y) + u3y * v3y, (u1y * v1z + u2y * v2z) + u3y * v3z,
                       (u1z * v1x + u2z * v2x) + u3z * v3x, (u1z * v1y + u2z * v2y) + u3z * v3y, (u1z * v1z + u2z * v2z) + u3z * v3z};
  bool fin = true;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double t = cq[r] - ((R[3 * r] * cs[0] + R[3 * r + 1] * cs[1]) + R[3 * r + 2] * cs[2]);
    pose[4 * r] = R[3 * r]; pose[4 * r + 1] = R[3 * r + 1]; pose[4 * r + 2] = R[3 * r + 2]; pose[4 * r + 3] = t;
    fin = fin && isfinite(R[3 * r]) && isfinite(R[3 * r + 1]) && isfinite(R[3 * r + 2]) && isfinite(t);
  }
  return fin;
}

// correspondence i of the pair -> its points.  false, and nothing read out of bounds, when an index lies outside its set
__device__ __forceinline__ bool gr_gather(const float* __restrict__ Sb, const float* __restrict__ Tb, const int* __restrict__ cb, long long i,
                                          long long ns, long long nt, double (&s)[3], float (&q)[3]) {
  const int ci = cb[2 * i], cj = cb[2 * i + 1];
  if (ci < 0 || ci >= ns || cj < 0 || cj >= nt) return false;
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    s[e] = (double)Sb[3 * (long long)ci + e];
    q[e] = Tb[3 * (long long)cj + e];
  }
  return true;
}

// d2(T s, q) by nn_dist's rule on the f32 transformed point
__device__ __forceinline__ float gr_d2(const double* __restrict__ T, const double (&s)[3], const float (&q)[3]) {
  const float dx = sfmi_pose_row(T, s[0], s[1], s[2]) - q[0], dy = sfmi_pose_row(T + 4, s[0], s[1], s[2]) - q[1],
              dz = sfmi_pose_row(T + 8, s[0], s[1], s[2]) - q[2];
  return fmaf(dz, dz, fmaf(dy, dy, dx * dx));
}

// ---- hypotheses -----------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void greg_pose_kernel(const float* __restrict__ S, const float* __restrict__ T,
                                                        const long long* __restrict__ soff, const long long* __restrict__ toff,
                                                        const int* __restrict__ corr, const long long* __restrict__ coff,
                                                        const int* __restrict__ triples, int B, int H, double sim,
                                                        double* __restrict__ poses, int* __restrict__ valid) {
  const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (long long)B * H) return;
  const int b = (int)(g / H);
  const long long c0 = coff[b], C = coff[b + 1] - c0, ns = soff[b + 1] - soff[b], nt = toff[b + 1] - toff[b];
  const float* Sb = S + 3 * soff[b];
  const float* Tb = T + 3 * toff[b];
  const int* cb = corr + 2 * c0;
  const int t0 = triples[3 * g], t1 = triples[3 * g + 1], t2 = triples[3 * g + 2];
  bool ok = t0 >= 0 && t1 >= 0 && t2 >= 0 && t0 < C && t1 < C && t2 < C && t0 != t1 && t0 != t2 && t1 != t2;
  double s[3][3], q[3][3], pose[12];
#pragma unroll
  for (int e = 0; e < 12; ++e) pose[e] = sfmi_nan_f64();
  if (ok) {
    const int tr[3] = {t0, t1, t2};
#pragma unroll
    for (int p = 0; p < 3; ++p) {
      float qf[3];
      ok = gr_gather(Sb, Tb, cb, tr[p], ns, nt, s[p], qf) && ok;
#pragma unroll
      for (int e = 0; e < 3; ++e) q[p][e] = ok ? (double)qf[e] : 0.0;
    }
  }
  if (ok) {
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int e = 0; e < 3; ++e) ok = ok && isfinite(s[p][e]) && isfinite(q[p][e]);
  }
  if (ok) {
#pragma unroll
    for (int p = 0; p < 3; ++p) {                              // the edges (0, 1), (1, 2), (2, 0)
      const int r = (p + 1) % 3;
      const double ax = s[p][0] - s[r][0], ay = s[p][1] - s[r][1], az = s[p][2] - s[r][2];
      const double bx = q[p][0] - q[r][0], by = q[p][1] - q[r][1], bz = q[p][2] - q[r][2];
      const bool same = (ax == 0.0 && ay == 0.0 && az == 0.0) || (bx == 0.0 && by == 0.0 && bz == 0.0);   // two points coincide
      const double ls = sqrt((ax * ax + ay * ay) + az * az), lt = sqrt((bx * bx + by * by) + bz * bz);
      ok = ok && !same && ls >= sim * lt && lt >= sim * ls;
    }
  }
  if (ok) {
    double cs[3], cq[3], m[9], v[9], sg[3], M[9];
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      cs[e] = ((s[0][e] + s[1][e]) + s[2][e]) / 3.0;
      cq[e] = ((q[0][e] + q[1][e]) + q[2][e]) / 3.0;
    }
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        s[p][e] -= cs[e];
        q[p][e] -= cq[e];
        m[3 * p + e] = s[p][e];
      }
    gr_svd3(m, v, sg);                                         // the centred source triangle: rows are points
    ok = sg[0] > 0.0 && sg[1] > GR_RANK_TOL * sg[0];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) M[3 * r + c] = (q[0][r] * s[0][c] + q[1][r] * s[1][c]) + q[2][r] * s[2][c];
    ok = ok && gr_kabsch(M, cs, cq, pose);
    if (!ok) {
#pragma unroll
      for (int e = 0; e < 12; ++e) pose[e] = sfmi_nan_f64();
    }
  }
#pragma unroll
  for (int e = 0; e < 12; ++e) poses[12 * g + e] = pose[e];
  valid[g] = ok ? 1 : 0;
}

// ---- scoring --------------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void greg_init_kernel(const int* __restrict__ valid, const int* __restrict__ bad, int B, int H,
                                                        int* __restrict__ count) {
  const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (long long)B * H) return;
  const bool ok = (!valid || valid[g] != 0) && !(bad && bad[g / H] != 0);
  count[g] = ok ? 0 : -1;
}

__global__ __launch_bounds__(GS_THREADS) void greg_score_kernel(const float* __restrict__ S, const float* __restrict__ T,
                                                                const long long* __restrict__ soff, const long long* __restrict__ toff,
                                                                const int* __restrict__ corr, const long long* __restrict__ coff,
                                                                const double* __restrict__ poses, const int* __restrict__ valid,
                                                                const int* __restrict__ bad, int H, float maxd2, int* __restrict__ count) {
  __shared__ double ps[GS_HT][12];                             // an invalid hypothesis: NaN, the pose of no inlier
  __shared__ int wc[GS_WAVES][GS_HT];
  const int b = blockIdx.z, tid = threadIdx.x, lane = tid & 63;
  const long long c0 = coff[b], C = coff[b + 1] - c0;
  if ((long long)blockIdx.x * GS_CHUNK >= C) return;           // workgroup-uniform, before any barrier
  const long long ns = soff[b + 1] - soff[b], nt = toff[b + 1] - toff[b];
  const float* Sb = S + 3 * soff[b];
  const float* Tb = T + 3 * toff[b];
  const int* cb = corr + 2 * c0;
  const int h0 = blockIdx.y * GS_HT;
  const bool pair_bad = bad && bad[b] != 0;
  for (int e = tid; e < GS_HT * 12; e += GS_THREADS) {
    const int hh = e / 12, k = e - 12 * hh, h = h0 + hh;
    const bool ok = h < H && !pair_bad && (!valid || valid[(long long)b * H + h] != 0);
    ps[hh][k] = ok ? poses[12 * ((long long)b * H + h) + k] : sfmi_nan_f64();
  }
  __syncthreads();
  for (long long c = blockIdx.x; c * GS_CHUNK < C; c += gridDim.x) {   // workgroup-uniform bounds
    double s[GS_R][3];
    float q[GS_R][3];
#pragma unroll
    for (int r = 0; r < GS_R; ++r) {
      const long long i = c * GS_CHUNK + r * GS_THREADS + tid;
      if (!(i < C && gr_gather(Sb, Tb, cb, i, ns, nt, s[r], q[r]))) {
#pragma unroll
        for (int e = 0; e < 3; ++e) {                          // padding: NaN is an inlier of nothing
          s[r][e] = sfmi_nan_f64();
          q[r][e] = __int_as_float(0x7FC00000);
        }
      }
    }
    int mine = 0;
#pragma unroll 2
    for (int hh = 0; hh < GS_HT; ++hh) {
      const double* Tp = ps[hh];                               // broadcast reads
      int cnt = 0;
#pragma unroll
      for (int r = 0; r < GS_R; ++r) cnt += __popcll(__ballot(gr_d2(Tp, s[r], q[r]) <= maxd2));
      mine = lane == hh ? cnt : mine;
    }
    sfmi_commit_counts(wc, mine, count + (long long)b * H + h0);
  }
}

__global__ __launch_bounds__(SFMI_BEST_THREADS) void greg_best_kernel(int H, const int* __restrict__ count,
                                                                      const int* __restrict__ bad,
                                                                      int* __restrict__ best, int* __restrict__ status) {
  const int b = blockIdx.x;
  int bc, bh;
  sfmi_best_of_row(count + (long long)b * H, H, bc, bh);
  if (threadIdx.x == 0) {
    best[b] = bc >= 0 ? bh : -1;
    status[b] = (bad && bad[b] != 0) ? 4 : (bc >= 0 ? 0 : 1);
  }
}

// ---- the refit ------------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(GR_THREADS) void greg_refit_kernel(const float* __restrict__ S, const float* __restrict__ T,
                                                                const long long* __restrict__ soff, const long long* __restrict__ toff,
                                                                const int* __restrict__ corr, const long long* __restrict__ coff,
                                                                const double* __restrict__ poses, const int* __restrict__ best, int H,
                                                                float maxd2, int refit, int* __restrict__ status, double* __restrict__ pose,
                                                                unsigned char* __restrict__ inlier, int* __restrict__ n_in,
                                                                double* __restrict__ sums) {
  __shared__ double red[GR_WAVES];
  const int b = blockIdx.x, tid = threadIdx.x;
  const long long c0 = coff[b], C = coff[b + 1] - c0, ns = soff[b + 1] - soff[b], nt = toff[b + 1] - toff[b];
  const float* Sb = S + 3 * soff[b];
  const float* Tb = T + 3 * toff[b];
  const int* cb = corr + 2 * c0;
  unsigned char* mask = inlier + c0;
  const int h = best[b];
  const bool ok = status[b] == 0 && h >= 0 && h < H;           // workgroup-uniform
  double W[12];
#pragma unroll
  for (int e = 0; e < 12; ++e) W[e] = ok ? poses[12 * ((long long)b * H + h) + e] : sfmi_nan_f64();
  // pass 1: the winner's inliers, their number and the sums of their points
  double acc[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (long long i = tid; i < C; i += GR_THREADS) {
    double s[3];
    float q[3];
    const bool in = gr_gather(Sb, Tb, cb, i, ns, nt, s, q) && gr_d2(W, s, q) <= maxd2;
    mask[i] = in ? 1 : 0;
    if (in) {
      acc[0] += 1.0;
      acc[1] += s[0]; acc[2] += s[1]; acc[3] += s[2];
      acc[4] += (double)q[0]; acc[5] += (double)q[1]; acc[6] += (double)q[2];
    }
  }
#pragma unroll
  for (int e = 0; e < 7; ++e) acc[e] = sfmi_block_sum_f64<GR_WAVES>(acc[e], red);   // the count: whole numbers below 2^31, exact in f64
  const int cnt = (int)acc[0];
  double P[12] = {1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0};
  double M[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  bool good = ok && cnt >= 3;                                  // workgroup-uniform: every lane holds the same sums
  if (good && refit) {
    const double cs[3] = {acc[1] / acc[0], acc[2] / acc[0], acc[3] / acc[0]}, cq[3] = {acc[4] / acc[0], acc[5] / acc[0], acc[6] / acc[0]};
    // pass 2: the cross terms about the centroids (each lane reads back the mask bytes it wrote itself)
    for (long long i = tid; i < C; i += GR_THREADS) {
      if (mask[i]) {
        double s[3];
        float q[3];
        gr_gather(Sb, Tb, cb, i, ns, nt, s, q);
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
          for (int c = 0; c < 3; ++c) M[3 * r + c] += ((double)q[r] - cq[r]) * (s[c] - cs[c]);
      }
    }
#pragma unroll
    for (int e = 0; e < 9; ++e) M[e] = sfmi_block_sum_f64<GR_WAVES>(M[e], red);
    good = gr_kabsch(M, cs, cq, P);
  } else if (good) {
#pragma unroll
    for (int e = 0; e < 12; ++e) P[e] = W[e];
  }
  if (tid == 0) {                                              // constant indices: the sums stay in registers
#pragma unroll
    for (int e = 0; e < 7; ++e) sums[(long long)b * GR_NS + e] = acc[e];
#pragma unroll
    for (int e = 0; e < 9; ++e) sums[(long long)b * GR_NS + 7 + e] = M[e];
  }
  if (!good) {                                                 // fewer than 3 inliers or a degenerate refit: the identity, no inliers
    for (long long i = tid; i < C; i += GR_THREADS) mask[i] = 0;
    if (tid < 12) pose[12 * b + tid] = (tid == 0 || tid == 5 || tid == 10) ? 1.0 : 0.0;
    if (tid == 0) {
      n_in[b] = 0;
      if (ok) status[b] = 2;
    }
    return;
  }
  int mcount = cnt;
  if (refit) {
    // pass 3: the mask under the refit pose
    int mm = 0;
    for (long long i = tid; i < C; i += GR_THREADS) {
      double s[3];
      float q[3];
      const bool in = gr_gather(Sb, Tb, cb, i, ns, nt, s, q) && gr_d2(P, s, q) <= maxd2;
      mask[i] = in ? 1 : 0;
      mm += in ? 1 : 0;
    }
    mcount = (int)sfmi_block_sum_f64<GR_WAVES>((double)mm, red);
  }
  if (tid == 0) {
#pragma unroll
    for (int e = 0; e < 12; ++e) pose[12 * b + e] = P[e];
    n_in[b] = mcount;
  }
}

}  // namespace

extern "C" {

int sfmi_greg_poses_f32(const float* src, const float* tgt, const long long* soff, const long long* toff, const int* corr,
                        const long long* coff, const int* triples, int B, int H, long long C, double similarity, double* poses,
                        int* valid, void* stream) {
  if (B <= 0 || B > (int)SFMI_MAX_GRID || H < 1 || C < 0 || !(similarity >= 0.0 && similarity <= 1.0) || !soff || !toff || !coff ||
      !triples || !poses || !valid || (C > 0 && (!src || !tgt || !corr)))
    return SFMI_EINVAL;
  hipLaunchKernelGGL(greg_pose_kernel, dim3(blocks256((long long)B * H)), dim3(256), 0, (hipStream_t)stream, src, tgt, soff, toff, corr, coff,
                     triples, B, H, similarity, poses, valid);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_greg_score_f32(const float* src, const float* tgt, const long long* soff, const long long* toff, const int* corr,
                        const long long* coff, const double* poses, const int* valid, const int* bad, int B, int H, long long max_c,
                        float maxd2, int* count, int* best, int* status, void* stream) {
  if (B <= 0 || B > (int)SFMI_MAX_GRID || H < 1 || cdiv(H, GS_HT) > SFMI_MAX_GRID || max_c < 0 || max_c >= (1ll << 31) ||
      !(maxd2 >= 0.f) || !soff || !toff || !coff || !poses || !count || !best || !status || (max_c > 0 && (!src || !tgt || !corr)))
    return SFMI_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(greg_init_kernel, dim3(blocks256((long long)B * H)), dim3(256), 0, st, valid, bad, B, H, count);
  if (max_c > 0)
    hipLaunchKernelGGL(greg_score_kernel, dim3(sfmi_grid_cap(cdiv(max_c, GS_CHUNK)), (unsigned)cdiv(H, GS_HT), (unsigned)B),
                       dim3(GS_THREADS), 0, st, src, tgt, soff, toff, corr, coff, poses, valid, bad, H, maxd2, count);
  hipLaunchKernelGGL(greg_best_kernel, dim3((unsigned)B), dim3(SFMI_BEST_THREADS), 0, st, H, (const int*)count, bad, best, status);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_greg_refit_f32(const float* src, const float* tgt, const long long* soff, const long long* toff, const int* corr,
                        const long long* coff, const double* poses, const int* best, int B, int H, long long C, float maxd2, int refit,
                        int* status, double* pose, unsigned char* inlier, int* n_in, double* sums, void* stream) {
  if (B <= 0 || H < 1 || C < 0 || !(maxd2 >= 0.f) || !soff || !toff || !coff || !poses || !best || !status || !pose || !n_in || !sums ||
      (C > 0 && (!src || !tgt || !corr || !inlier)))
    return SFMI_EINVAL;
  hipLaunchKernelGGL(greg_refit_kernel, dim3((unsigned)B), dim3(GR_THREADS), 0, (hipStream_t)stream, src, tgt, soff, toff, corr, coff, poses,
                     best, H, maxd2, refit, status, pose, inlier, n_in, sums);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

}  // extern "C"
