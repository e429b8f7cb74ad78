// Rigid registration of partial scans: iterative closest point for ragged batches of (source, target) pairs, what Open3D calls
// registration_icp (point-to-point and point-to-plane).  The reference has no such step: its real-scan datasets
// (shapeformer/data/imnet_datasets/redwood.py, realtest.py) serve one cloud in one frame.  DESIGN.md §5.18.
//
// The pose of a pair is 12 doubles on the device, row-major [R | t]; it is always applied to the ORIGINAL f32 source, so nothing
// accumulates in f32.  One iteration is three launches (four when the target is split), and nothing is read back:
// 1. icp_correspond_kernel: sfmi_search.h's sfmi_search3, the search pointdist.hip's nn_kernel runs - 256 lanes x 8 queries in registers,
//    the target through a 256-point float4 LDS tile read as a broadcast, d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx)), a strict `<` over
//    ascending indices - with the pose applied as the query is loaded.  (idx, d2) are the bits nn_dist gives on the transformed cloud.
//    When there are too few query blocks the target is cut into S chunks (grid.y) and the shared merge, skipping frozen pairs, merges
//    them in ascending chunk order.
// 2. icp_accumulate_kernel: grid (source chunks of 1024 points, pairs).  A lane gathers q (and n) of its 4 points, ascending, into
//    29 f64 accumulators (the 21 upper entries of A = sum J^T J, the 6 of sum J^T r, sum d2, count); sfmi_ragged.h's
//    sfmi_chunk_partial ends the chunk: wave_sum_f64, the 4 waves in order, one partial per chunk.  Chunks start at the set's first
//    point: a pair's sums do not depend on the batch around it.
// 3. icp_update_kernel: one wave per pair.  Lane e adds entry e of the chunk partials in ascending chunk order (sfmi_chunk_total);
//    lane 0 takes the statistics, tests convergence, solves A xi = g by Cholesky, and writes the pose and the state.
// A pair that has ended (state != 0) is frozen: its workgroups leave at once (block-uniform exits, before any barrier) and none of
// its outputs changes again, so the result does not depend on how often the host looks at the states.
//
// Loop discipline: no kernel waits on another workgroup, there are no spins, every loop around a barrier has workgroup-uniform
// bounds.  No float atomics: every sum has one fixed order.  An index is range-checked before the point it names is read.
#include "sfmi_search.h"   // the split search (plan, block offsets, scan, merge) and the ragged-batch helpers: DESIGN.md §5.5a

// the transform and the residuals are written once, here and in numpy (tests/icp_ref.py): every product and sum rounded on its own
#pragma clang fp contract(off)

namespace {

constexpr int IC_THREADS = SFMI_SCAN_TILE;
constexpr int IC_R = 8;                          // queries per lane
constexpr int IC_QB = IC_THREADS * IC_R;         // queries per workgroup
constexpr int IC_TARGET_BLOCKS = 2048;           // 256 CUs x 8 workgroups
constexpr int IC_NS = 29;                        // A (21, upper, row-major) | J^T r (6) | sum d2 | count
constexpr int IC_SD2 = 27, IC_CNT = 28;
constexpr int ICP_POINT = 0, ICP_PLANE = SFMI_METRIC_PLANE;

inline int ic_splits(int B, long long N, long long M) { return sfmi_splits(B, N, M, IC_TARGET_BLOCKS, IC_QB); }

// ---- start of a call (the finite check of the pairs is sfmi_ragged.h's sfmi_pairs_finite) -------------------------------------------

// one lane per pair: the state of iteration 0, and (lane 0) which query blocks belong to which pair
__global__ void icp_begin_kernel(const long long* __restrict__ soff, const double* __restrict__ pose, const int* __restrict__ bad,
                                 int B, long long* __restrict__ block_off, int* __restrict__ state, int* __restrict__ status,
                                 int* __restrict__ iterations, double* __restrict__ fitness, double* __restrict__ rmse) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b == 0) sfmi_block_offsets(soff, block_off, B, IC_QB);
  if (b >= B) return;
  const bool ok = bad[b] == 0 && sfmi_pose_finite(pose + 12 * b);
  state[b] = ok ? 0 : 1;
  status[b] = ok ? 1 : 4;
  iterations[b] = 0;
  fitness[b] = 0.0;
  rmse[b] = 0.0;
}

// ---- correspondences ----------------------------------------------------------------------------------------------------------------

// grid (query blocks upper bound, S).  S == 1: d_out / i_out are the results; S > 1: partial buffers, chunk s at d_out + s * N.
__global__ __launch_bounds__(IC_THREADS) void icp_correspond_kernel(const float* __restrict__ P, const float* __restrict__ Q,
                                                                    const long long* __restrict__ poff,
                                                                    const long long* __restrict__ qoff,
                                                                    const long long* __restrict__ block_off,
                                                                    const double* __restrict__ pose, const int* __restrict__ state, int B,
                                                                    long long N, float* __restrict__ d_out, int* __restrict__ i_out) {
  const long long g = blockIdx.x;
  if (g >= block_off[B]) return;                               // block-uniform: the grid is an upper bound
  const int b = sfmi_owner(block_off, B, g);
  if (state[b] != 0) return;                                   // a frozen pair: block-uniform, before any barrier
  const double* T = pose + 12 * b;
  const auto load = [P, T](long long i, bool ok, float& px, float& py, float& pz) {   // the pose is applied as the query is loaded
    const double x = ok ? (double)P[3 * i] : 0.0, y = ok ? (double)P[3 * i + 1] : 0.0, z = ok ? (double)P[3 * i + 2] : 0.0;
    px = sfmi_pose_row(T, x, y, z);
    py = sfmi_pose_row(T + 4, x, y, z);
    pz = sfmi_pose_row(T + 8, x, y, z);
  };
  sfmi_search3<IC_R>(Q, qoff[b], qoff[b + 1], poff[b] + (g - block_off[b]) * IC_QB, poff[b + 1], load,
                      d_out + (long long)blockIdx.y * N, i_out + (long long)blockIdx.y * N);
}

// ---- the normal equations -----------------------------------------------------------------------------------------------------------

// one inlier's terms.  a: the transformed point (f32, widened); q: its target point; n: the target normal (plane metric)
template <int METRIC>
__device__ __forceinline__ void ia_add(double (&acc)[IC_NS], double ax, double ay, double az, double qx, double qy, double qz, double nx,
                                       double ny, double nz) {
  const double dx = ax - qx, dy = ay - qy, dz = az - qz;
  if (METRIC == ICP_PLANE) {
    // r = (a - q).n, J = [a x n, n]
    const double r = (dx * nx + dy * ny) + dz * nz;
    const double J[6] = {ay * nz - az * ny, az * nx - ax * nz, ax * ny - ay * nx, nx, ny, nz};
    int e = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = i; j < 6; ++j) acc[e++] += J[i] * J[j];
#pragma unroll
    for (int i = 0; i < 6; ++i) acc[21 + i] += J[i] * r;
  } else {
    // r = a - q (three rows), J = [-[a]x | I]: J^T J = [[|a|^2 I - a a^T, [a]x], [., I]], J^T r = [a x r, r]
    acc[0] += ay * ay + az * az;  acc[1] += -(ax * ay);         acc[2] += -(ax * az);
    acc[6] += ax * ax + az * az;  acc[7] += -(ay * az);         acc[11] += ax * ax + ay * ay;
    acc[4] += -az;  acc[5] += ay;                               // row 0, columns 4 and 5 of [a]x
    acc[8] += az;   acc[10] += -ax;                             // row 1, columns 3 and 5
    acc[12] += -ay; acc[13] += ax;                              // row 2, columns 3 and 4
    acc[15] += 1.0; acc[18] += 1.0; acc[20] += 1.0;             // the identity block's diagonal
    acc[21] += ay * dz - az * dy;
    acc[22] += az * dx - ax * dz;
    acc[23] += ax * dy - ay * dx;
    acc[24] += dx; acc[25] += dy; acc[26] += dz;
  }
}

// grid (source chunks, pairs): part[(b * gridDim.x + chunk) * 29 + e].  metric[b] and maxd2[b] are the pair's: workgroup-uniform
__global__ __launch_bounds__(SFMI_CHUNK_THREADS) void icp_accumulate_kernel(
    const float* __restrict__ P, const float* __restrict__ Q, const float* __restrict__ Nrm, const long long* __restrict__ poff,
    const long long* __restrict__ qoff, const double* __restrict__ pose, const int* __restrict__ state, const int* __restrict__ idx,
    const float* __restrict__ d2, const int* __restrict__ metric, const float* __restrict__ maxd2v, double* __restrict__ part) {
  __shared__ double red[SFMI_CHUNK_THREADS / 64][IC_NS];
  const int b = blockIdx.y, tid = threadIdx.x;
  if (state[b] != 0) return;                                   // a frozen pair: block-uniform, before any barrier
  const long long p0 = poff[b], n = poff[b + 1] - p0;
  if ((long long)blockIdx.x * SFMI_CHUNK >= n) return;         // block-uniform
  const long long q0 = qoff[b], m = qoff[b + 1] - q0;
  const double* T = pose + 12 * b;
  const bool plane = metric[b] == ICP_PLANE;
  const float maxd2 = maxd2v[b];
  double acc[IC_NS];
#pragma unroll
  for (int e = 0; e < IC_NS; ++e) acc[e] = 0.0;
#pragma unroll
  for (int r = 0; r < SFMI_CHUNK_R; ++r) {                     // a lane's points in ascending order
    const long long i = (long long)blockIdx.x * SFMI_CHUNK + r * SFMI_CHUNK_THREADS + tid;
    if (i < n) {
      const int j = idx[p0 + i];
      const float d = d2[p0 + i];
      if (sfmi_inlier(j, m, d, maxd2)) {                       // the index is checked before the point is read
        const double x = (double)P[3 * (p0 + i)], y = (double)P[3 * (p0 + i) + 1], z = (double)P[3 * (p0 + i) + 2];
        const double ax = (double)sfmi_pose_row(T, x, y, z), ay = (double)sfmi_pose_row(T + 4, x, y, z),
                     az = (double)sfmi_pose_row(T + 8, x, y, z);
        const float* q = Q + 3 * (q0 + j);
        if (plane) {
          const float* nn = Nrm + 3 * (q0 + j);
          ia_add<ICP_PLANE>(acc, ax, ay, az, (double)q[0], (double)q[1], (double)q[2], (double)nn[0], (double)nn[1], (double)nn[2]);
        } else {
          ia_add<ICP_POINT>(acc, ax, ay, az, (double)q[0], (double)q[1], (double)q[2], 0.0, 0.0, 0.0);
        }
        acc[IC_SD2] += (double)d;
        acc[IC_CNT] += 1.0;
      }
    }
  }
  sfmi_chunk_partial(acc, red, part + ((long long)b * gridDim.x + blockIdx.x) * IC_NS);
}

// ---- the step -----------------------------------------------------------------------------------------------------------------------

// A (6x6, full, symmetric) x = g by Cholesky in f64; false for a pivot that is not positive and finite or is <= 1e-12 x the largest
// diagonal entry
__device__ bool ic_cholesky6(double (&A)[6][6], const double (&g)[6], double (&x)[6]) {
  double big = 0.0;
  for (int i = 0; i < 6; ++i) big = fmax(big, A[i][i]);
  for (int j = 0; j < 6; ++j) {
    double d = A[j][j];
    for (int k = 0; k < j; ++k) d -= A[j][k] * A[j][k];
    if (!(d > 0.0) || !isfinite(d) || d <= 1e-12 * big) return false;
    const double l = sqrt(d);
    A[j][j] = l;
    for (int i = j + 1; i < 6; ++i) {
      double s = A[i][j];
      for (int k = 0; k < j; ++k) s -= A[i][k] * A[j][k];
      A[i][j] = s / l;
    }
  }
  double y[6];
  for (int i = 0; i < 6; ++i) {
    double s = g[i];
    for (int k = 0; k < i; ++k) s -= A[i][k] * y[k];
    y[i] = s / A[i][i];
  }
  for (int i = 5; i >= 0; --i) {
    double s = y[i];
    for (int k = i + 1; k < 6; ++k) s -= A[k][i] * x[k];
    x[i] = s / A[i][i];
  }
  return true;
}

// one wave per pair.  k: the iteration; last: this is the evaluation after the last step
__global__ __launch_bounds__(64) void icp_update_kernel(const long long* __restrict__ poff, const double* __restrict__ part, int chunks,
                                                        const int* __restrict__ metricv, int k, int last, double rel_fitness, double rel_rmse,
                                                        double* __restrict__ pose, int* __restrict__ state, int* __restrict__ status,
                                                        int* __restrict__ iterations, double* __restrict__ fitness,
                                                        double* __restrict__ rmse, double* __restrict__ sums, double* __restrict__ xi) {
  __shared__ double s[IC_NS];
  const int b = blockIdx.x, lane = threadIdx.x;
  if (state[b] != 0) return;                                   // frozen: the whole wave leaves
  const long long n = poff[b + 1] - poff[b];
  const int metric = metricv[b];
  if (lane < IC_NS) {
    const double v = sfmi_chunk_total<IC_NS>(part, b, chunks, (int)cdiv(n, SFMI_CHUNK));   // ascending chunk order
    s[lane] = v;
    sums[(long long)b * IC_NS + lane] = v;
  }
  __syncthreads();
  if (lane != 0) return;
  const double count = s[IC_CNT];
  const double fit = n > 0 ? count / (double)n : 0.0;
  const double rm = count > 0.0 ? sqrt(s[IC_SD2] / count) : 0.0;
  const double pfit = fitness[b], prm = rmse[b];
  fitness[b] = fit;
  rmse[b] = rm;
  iterations[b] = k;
  int end = -1;
  if (last) end = 1;
  else if (k > 0 && fabs(fit - pfit) < rel_fitness && fabs(rm - prm) < rel_rmse) end = 0;
  else if (count < (metric == ICP_PLANE ? 6.0 : 3.0)) end = 2;
  double w[6];
  if (end < 0) {
    double A[6][6], g[6];
    int e = 0;
    for (int i = 0; i < 6; ++i)
      for (int j = i; j < 6; ++j) {
        A[i][j] = s[e];
        A[j][i] = s[e];
        ++e;
      }
    for (int i = 0; i < 6; ++i) g[i] = -s[21 + i];
    if (!ic_cholesky6(A, g, w)) end = 3;
  }
  if (end >= 0) {
    status[b] = end;
    state[b] = 1;
    return;
  }
  // dR = Rodrigues(w) = I + a K + c K^2, K = [w]x, a = sin t / t, c = (1 - cos t) / t^2; the series below t = 1e-4
  const double wx = w[0], wy = w[1], wz = w[2];
  const double t2 = (wx * wx + wy * wy) + wz * wz, t = sqrt(t2);
  double a, c;
  if (t < 1e-4) {
    a = 1.0 - t2 / 6.0 + t2 * t2 / 120.0;
    c = 0.5 - t2 / 24.0 + t2 * t2 / 720.0;
  } else {
    a = sin(t) / t;
    c = (1.0 - cos(t)) / t2;
  }
  double dR[3][3];
  dR[0][0] = 1.0 - c * (wy * wy + wz * wz); dR[0][1] = c * (wx * wy) - a * wz;        dR[0][2] = c * (wx * wz) + a * wy;
  dR[1][0] = c * (wx * wy) + a * wz;        dR[1][1] = 1.0 - c * (wx * wx + wz * wz); dR[1][2] = c * (wy * wz) - a * wx;
  dR[2][0] = c * (wx * wz) - a * wy;        dR[2][1] = c * (wy * wz) + a * wx;        dR[2][2] = 1.0 - c * (wx * wx + wy * wy);
  double* T = pose + 12 * b;
  double old[12], nw[12];
  for (int e = 0; e < 12; ++e) old[e] = T[e];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 4; ++j) nw[4 * i + j] = (dR[i][0] * old[j] + dR[i][1] * old[4 + j]) + dR[i][2] * old[8 + j];
    nw[4 * i + 3] += w[3 + i];
  }
  for (int e = 0; e < 12; ++e) T[e] = nw[e];
  for (int e = 0; e < 6; ++e) xi[6 * b + e] = w[e];
}

// ---- the public transform -----------------------------------------------------------------------------------------------------------

__global__ void icp_transform_kernel(const float* __restrict__ P, const long long* __restrict__ off, const double* __restrict__ pose,
                                     int B, long long N, float* __restrict__ out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const double* T = pose + 12 * sfmi_owner(off, B, i);
  const double x = (double)P[3 * i], y = (double)P[3 * i + 1], z = (double)P[3 * i + 2];
  out[3 * i] = sfmi_pose_row(T, x, y, z);
  out[3 * i + 1] = sfmi_pose_row(T + 4, x, y, z);
  out[3 * i + 2] = sfmi_pose_row(T + 8, x, y, z);
}

}  // namespace

extern "C" {

int sfmi_icp_query_block(void) { return IC_QB; }
int sfmi_icp_chunk(void) { return SFMI_CHUNK; }
int sfmi_icp_splits(int B, long long N, long long M) { return (B <= 0 || N < 0 || M < 0) ? 0 : ic_splits(B, N, M); }

int sfmi_icp_transform_f32(const float* P, const long long* off, const double* pose, int B, long long N, float* out, void* stream) {
  if (B <= 0 || N < 0 || !off || !pose) return SFMI_EINVAL;
  if (N == 0) return SFMI_OK;
  if (!P || !out) return SFMI_EINVAL;
  hipLaunchKernelGGL(icp_transform_kernel, dim3(blocks256(N)), dim3(256), 0, (hipStream_t)stream, P, off, pose, B, N, out);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_icp_begin_f32(const float* src, const float* tgt, const float* nrm, const long long* soff, const long long* toff,
                       const double* pose, const int* metric, int B, long long N, long long M, long long max_n, long long max_m,
                       int* bad, long long* block_off, int* state, int* status, int* iterations, double* fitness, double* rmse, void* stream) {
  if (B <= 0 || B > 65535 || N < 0 || M < 0 || max_n < 0 || max_m < 0 || max_n >= (1ll << 31) || max_m >= (1ll << 31) || !soff || !toff ||
      !pose || !metric || !bad || !block_off || !state || !status || !iterations || !fitness || !rmse || (N > 0 && !src) || (M > 0 && !tgt))
    return SFMI_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (const int rc = sfmi_pairs_finite<true>(src, tgt, nrm, soff, toff, metric, B, max_n, max_m, bad, st)) return rc;
  hipLaunchKernelGGL(icp_begin_kernel, dim3(blocks256(B)), dim3(256), 0, st, soff, pose, (const int*)bad, B, block_off, state, status,
                     iterations, fitness, rmse);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_icp_iterate_f32(const float* src, const float* tgt, const float* nrm, const long long* soff, const long long* toff,
                         const long long* block_off, int B, long long N, long long M, long long max_n, const int* metric, const float* maxd2, int k,
                         int last, double rel_fitness, double rel_rmse, double* pose, int* state, int* status, int* iterations,
                         double* fitness, double* rmse, int* idx, float* d2, float* part_d2, int* part_idx, double* part, double* sums,
                         double* xi, void* stream) {
  if (B <= 0 || B > 65535 || N < 0 || M < 0 || M >= (1ll << 31) || max_n < 0 || max_n >= (1ll << 31) ||
      !metric || !maxd2 || k < 0 || !soff || !toff || !block_off || !pose || !state || !status || !iterations ||
      !fitness || !rmse || !part || !sums || !xi || (N > 0 && (!src || !idx || !d2)) || (M > 0 && !tgt))
    return SFMI_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int S = ic_splits(B, N, M);
  if (N > 0 && S > 1 && (!part_d2 || !part_idx)) return SFMI_EINVAL;
  const int chunks = (int)(max_n > 0 ? cdiv(max_n, SFMI_CHUNK) : 1);
  if (N > 0) {
    const dim3 grid((unsigned)sfmi_qblocks(B, N, IC_QB), (unsigned)S);
    if (S == 1) {
      hipLaunchKernelGGL(icp_correspond_kernel, grid, dim3(IC_THREADS), 0, st, src, tgt, soff, toff, block_off, (const double*)pose,
                         (const int*)state, B, N, d2, idx);
    } else {
      hipLaunchKernelGGL(icp_correspond_kernel, grid, dim3(IC_THREADS), 0, st, src, tgt, soff, toff, block_off, (const double*)pose,
                         (const int*)state, B, N, part_d2, part_idx);
      sfmi_nn_merge<true, true>(part_d2, part_idx, soff, state, B, S, N, d2, idx, st);   // a frozen pair's (idx, d2) stay
    }
    const dim3 agrid((unsigned)chunks, (unsigned)B);
    hipLaunchKernelGGL(icp_accumulate_kernel, agrid, dim3(SFMI_CHUNK_THREADS), 0, st, src, tgt, nrm, soff, toff, (const double*)pose,
                       (const int*)state, (const int*)idx, (const float*)d2, metric, maxd2, part);
  }
  hipLaunchKernelGGL(icp_update_kernel, dim3((unsigned)B), dim3(64), 0, st, soff, (const double*)part, chunks, metric, k, last, rel_fitness,
                     rel_rmse, pose, state, status, iterations, fitness, rmse, sums, xi);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

}  // extern "C"
