// Multiway registration of partial scans: the information matrix of a registered pair and a pose-graph optimiser, what Open3D calls
// get_information_matrix_from_point_clouds and global_optimization (Levenberg-Marquardt with a line process over the uncertain
// edges).  The reference has no such step: its real-scan datasets serve one cloud in one frame.  DESIGN.md §5.20; the contract is
// stated in include/sfmi.h and restated in numpy in tests/posegraph_ref.py.
//
// 1. pg_info_kernel / pg_info_reduce_kernel: Lambda = sum G^T G, G = [-[q]x | I], over the inliers (sfmi_inlier) of correspondences the
//    caller already has.  Ten f64 sums per pair (six quadratic entries, sum q, count) through the code register.hip's accumulate /
//    update pair runs, so in §5.18's order bit for bit (tests/test_search_shared_gpu.py): a lane's 4 points ascending, then
//    sfmi_ragged.h's sfmi_chunk_partial (wave_sum_f64, the 4 waves in order) and, by one wave per pair, sfmi_chunk_total (the chunk
//    partials in ascending order).  The finite checks are sfmi_pairs_finite and sfmi_pose_finite.
// 2. pg_optimize_kernel: one workgroup per graph runs the whole Levenberg-Marquardt loop.  Per outer iteration: one lane per edge
//    evaluates the residual, its Jacobian and the edge's 6 x 6 block M = l J^T Lambda J and b = l J^T Lambda r (J_tgt = -J_src, so one
//    block serves the four places an edge touches); one lane per pair of free nodes adds the blocks of its edges in ascending edge
//    index into H (packed lower triangle, in the caller's workspace: it stays in L2 and is read once per solve); one lane per unknown
//    does the same for g.  A solve copies H + lambda I and g (as one more row) into LDS and factors there: right-looking Cholesky,
//    one element one owner, so the forward substitution comes for free; then the back substitution, the step, and the cost under the
//    trial poses.  Lane 0 writes the decision into one LDS word that every lane reads.
//
// Loop discipline (§5.17 / §5.18): nothing waits on another workgroup, there are no spins, every loop around a barrier has
// workgroup-uniform bounds (the graph's sizes, max_iter, PG_MAX_TRIES, words read from LDS after a barrier).  No float atomics: every
// sum has one fixed order, so a graph's result depends on that graph alone.  Indices are range-checked before they are used.
#include "sfmi_ragged.h"

#pragma clang fp contract(off)

namespace {

constexpr int PI_NS = 10;                        // qy^2+qz^2 | -qx qy | -qx qz | qx^2+qz^2 | -qy qz | qx^2+qy^2 | qx | qy | qz | count

constexpr int PG_THREADS = 256;
constexpr int PG_MAX_NODES = 32;
constexpr int PG_MAX_EDGES = 496;
constexpr int PG_EW = 27;                        // per edge: M (21 upper entries, row-major) | b (6)
constexpr int PG_MAX_TRIES = 128;                // lambda doubles from >= 1e-12 past 1e12 in 80 tries
constexpr double PG_THETA_MAX = 3.1;
constexpr double PG_LAMBDA_MIN = 1e-12, PG_LAMBDA_MAX = 1e12;

// ---- the information matrix ---------------------------------------------------------------------------------------------------------

// grid (source chunks, pairs): part[(b * gridDim.x + chunk) * 10 + e]
__global__ __launch_bounds__(SFMI_CHUNK_THREADS) void pg_info_kernel(
    const float* __restrict__ Q, const long long* __restrict__ poff, const long long* __restrict__ qoff, const double* __restrict__ pose,
    const int* __restrict__ bad, const int* __restrict__ idx, const float* __restrict__ d2, const float* __restrict__ maxd2v,
    double* __restrict__ part) {
  __shared__ double red[SFMI_CHUNK_THREADS / 64][PI_NS];
  const int b = blockIdx.y, tid = threadIdx.x;
  if (bad[b] != 0 || !sfmi_pose_finite(pose + 12 * b)) return;  // block-uniform, before any barrier: the reduce writes zeros
  const long long p0 = poff[b], n = poff[b + 1] - p0;
  if ((long long)blockIdx.x * SFMI_CHUNK >= n) return;         // block-uniform
  const long long q0 = qoff[b], m = qoff[b + 1] - q0;
  const float maxd2 = maxd2v[b];
  double acc[PI_NS];
#pragma unroll
  for (int e = 0; e < PI_NS; ++e) acc[e] = 0.0;
#pragma unroll
  for (int r = 0; r < SFMI_CHUNK_R; ++r) {                     // a lane's points in ascending order
    const long long i = (long long)blockIdx.x * SFMI_CHUNK + r * SFMI_CHUNK_THREADS + tid;
    if (i < n) {
      const int j = idx[p0 + i];
      const float d = d2[p0 + i];
      if (sfmi_inlier(j, m, d, maxd2)) {                       // the index is checked before the point is read
        const float* q = Q + 3 * (q0 + j);
        const double ax = (double)q[0], ay = (double)q[1], az = (double)q[2];
        acc[0] += ay * ay + az * az;  acc[1] += -(ax * ay);  acc[2] += -(ax * az);
        acc[3] += ax * ax + az * az;  acc[4] += -(ay * az);  acc[5] += ax * ax + ay * ay;
        acc[6] += ax;  acc[7] += ay;  acc[8] += az;
        acc[9] += 1.0;
      }
    }
  }
  sfmi_chunk_partial(acc, red, part + ((long long)b * gridDim.x + blockIdx.x) * PI_NS);
}

// one wave per pair: lane e adds entry e of the chunk partials in ascending chunk order; lane 0 writes the 6 x 6 matrix
__global__ __launch_bounds__(64) void pg_info_reduce_kernel(const long long* __restrict__ poff, const double* __restrict__ pose,
                                                            const int* __restrict__ bad, const double* __restrict__ part, int chunks,
                                                            double* __restrict__ info, int* __restrict__ count, int* __restrict__ flag) {
  __shared__ double s[PI_NS];
  const int b = blockIdx.x, lane = threadIdx.x;
  const bool ok = bad[b] == 0 && sfmi_pose_finite(pose + 12 * b);
  const long long n = poff[b + 1] - poff[b];
  if (lane < PI_NS) s[lane] = sfmi_chunk_total<PI_NS>(part, b, chunks, ok ? (int)cdiv(n, SFMI_CHUNK) : 0);
  __syncthreads();
  if (lane != 0) return;
  double* L = info + 36ll * b;
  for (int e = 0; e < 36; ++e) L[e] = 0.0;
  L[0] = s[0];  L[1] = s[1];  L[2] = s[2];
  L[6] = s[1];  L[7] = s[3];  L[8] = s[4];
  L[12] = s[2]; L[13] = s[4]; L[14] = s[5];
  // [q]x in the upper right block, its transpose in the lower left
  L[4] = -s[8];  L[5] = s[7];  L[9] = s[8];  L[11] = -s[6];  L[15] = -s[7];  L[16] = s[6];
  L[24] = -s[8]; L[30] = s[7]; L[19] = s[8]; L[31] = -s[6];  L[20] = -s[7];  L[26] = s[6];
  L[21] = s[9];  L[28] = s[9]; L[35] = s[9];
  count[b] = (int)s[9];
  flag[b] = ok ? 0 : 1;
}

// ---- the optimiser: per-edge terms ---------------------------------------------------------------------------------------------------

struct PgArgs {
  const long long* noff;
  const long long* eoff;
  double* X;
  const int* src;
  const int* tgt;
  const double* T;
  const double* Lam;
  const int* unc;
  const int* alive;
  const double* mu;
  int max_iter;
  double tol;
  int max_s;
  double* l;
  double* cost;
  int* iterations;
  int* status;
  double* ew;
  double* H;
  double* g;
  double* delta;
  double* lam;
};

__device__ __forceinline__ int pg_upper(int i, int j) { return i * 6 - i * (i - 1) / 2 + (j - i); }   // entry (i, j), i <= j, of the 21

// One alive edge under the poses xs, xt (12 doubles each, LDS): r = (w, v) of D = T^-1 xt^-1 xs, q = r^T Lam r, the line-process
// weight l and the edge's cost term; with J also M = l J^T Lam J (21 upper entries) and b = l J^T Lam r into w27.  -> theta
template <bool WITH_J>
__device__ __forceinline__ double pg_edge(const double* xs, const double* xt, const double* __restrict__ T, const double* __restrict__ Lm,
                                          bool line, double mu, double& l, double& cost, double* __restrict__ w27) {
  double RA[3][3], tA[3], RD[3][3], r[6];
  {
    // A = T^-1 xt^-1: R_A = R_T^T R_xt^T, t_A = -R_T^T (R_xt^T t_xt + t_T)
    double u[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) u[i] = ((xt[i] * xt[3] + xt[4 + i] * xt[7]) + xt[8 + i] * xt[11]) + T[4 * i + 3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j) RA[i][j] = (T[i] * xt[4 * j] + T[4 + i] * xt[4 * j + 1]) + T[8 + i] * xt[4 * j + 2];
      tA[i] = -((T[i] * u[0] + T[4 + i] * u[1]) + T[8 + i] * u[2]);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j) RD[i][j] = (RA[i][0] * xs[j] + RA[i][1] * xs[4 + j]) + RA[i][2] * xs[8 + j];
      r[3 + i] = ((RA[i][0] * xs[3] + RA[i][1] * xs[7]) + RA[i][2] * xs[11]) + tA[i];
    }
  }
  // w = theta / (2 sin theta) vee(R - R^T), theta = atan2(|vee| / 2, (tr - 1) / 2)
  const double vx = RD[2][1] - RD[1][2], vy = RD[0][2] - RD[2][0], vz = RD[1][0] - RD[0][1];
  const double sn = 0.5 * sqrt((vx * vx + vy * vy) + vz * vz);
  const double cs = 0.5 * (((RD[0][0] + RD[1][1]) + RD[2][2]) - 1.0);
  const double th = atan2(sn, cs), t2 = th * th;
  const double f = th < 1e-4 ? 0.5 * (1.0 + t2 / 6.0 + 7.0 * t2 * t2 / 360.0) : th / (2.0 * sin(th));
  r[0] = f * vx; r[1] = f * vy; r[2] = f * vz;
  double lr[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < 6; ++j) s += Lm[6 * i + j] * r[j];
    lr[i] = s;
  }
  double q = 0.0;
#pragma unroll
  for (int i = 0; i < 6; ++i) q += r[i] * lr[i];
  if (line) {
    const double s = mu / (mu + q);
    l = s * s;
    cost = l * q + mu * ((s - 1.0) * (s - 1.0));
  } else {
    l = 1.0;
    cost = q;
  }
  if (WITH_J) {
    // Jl^-1 = I - K / 2 + k K^2, K = [w]x, K^2 = w w^T - |w|^2 I
    const double k = th < 1e-4 ? 1.0 / 12.0 + t2 / 720.0 : 1.0 / t2 - (1.0 + cos(th)) / (2.0 * th * sin(th));
    const double w0 = r[0], w1 = r[1], w2 = r[2], ww = (w0 * w0 + w1 * w1) + w2 * w2;
    double Ji[3][3];
    Ji[0][0] = 1.0 + k * (w0 * w0 - ww); Ji[0][1] = 0.5 * w2 + k * (w0 * w1);  Ji[0][2] = -0.5 * w1 + k * (w0 * w2);
    Ji[1][0] = -0.5 * w2 + k * (w0 * w1); Ji[1][1] = 1.0 + k * (w1 * w1 - ww); Ji[1][2] = 0.5 * w0 + k * (w1 * w2);
    Ji[2][0] = 0.5 * w1 + k * (w0 * w2);  Ji[2][1] = -0.5 * w0 + k * (w1 * w2); Ji[2][2] = 1.0 + k * (w2 * w2 - ww);
    // J = [[Jl^-1 R_A, 0], [-R_A [t_s]x, R_A]]
    const double sx = xs[3], sy = xs[7], sz = xs[11];
    double J[6][6];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        J[i][j] = (Ji[i][0] * RA[0][j] + Ji[i][1] * RA[1][j]) + Ji[i][2] * RA[2][j];
        J[i][3 + j] = 0.0;
        J[3 + i][3 + j] = RA[i][j];
      }
      // -R_A [t]x: column 0 = -(R_A[:,1] tz - R_A[:,2] ty), column 1 = -(R_A[:,2] tx - R_A[:,0] tz), column 2 = -(R_A[:,0] ty - R_A[:,1] tx)
      J[3 + i][0] = RA[i][2] * sy - RA[i][1] * sz;
      J[3 + i][1] = RA[i][0] * sz - RA[i][2] * sx;
      J[3 + i][2] = RA[i][1] * sx - RA[i][0] * sy;
    }
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      double v[6];
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < 6; ++j) s += Lm[6 * i + j] * J[j][c];
        v[i] = s;
      }
#pragma unroll
      for (int a = 0; a <= c; ++a) {
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < 6; ++i) s += J[i][a] * v[i];
        w27[pg_upper(a, c)] = l * s;
      }
      double s = 0.0;
#pragma unroll
      for (int i = 0; i < 6; ++i) s += J[i][c] * lr[i];
      w27[21 + c] = l * s;
    }
  }
  return th;
}

// the words every lane reads after a barrier
enum { PG_F_BAD = 0, PG_F_THETA = 1, PG_F_DEC = 2, PG_F_N = 4 };
enum { PG_V_F = 0, PG_V_FN = 1, PG_V_LAM = 2, PG_V_N = 4 };
enum { PG_REJECT = 0, PG_ACCEPT = 1, PG_DONE = 2, PG_FAIL = 3, PG_FIXED = 4 };

// one workgroup per graph; dynamic LDS: (n + 1)(n + 2) / 2 doubles for the largest graph of the batch, n = 6 (max_s - 1)
__global__ __launch_bounds__(PG_THREADS) void pg_optimize_kernel(PgArgs a) {
  extern __shared__ double Lm[];                               // the packed lower triangle of H + lambda I, row n = g
  __shared__ double sX[PG_MAX_NODES * 12], sXn[PG_MAX_NODES * 12];
  __shared__ double sCost[512];
  __shared__ double sDelta[6 * PG_MAX_NODES];
  __shared__ double sVal[PG_V_N];
  __shared__ int sEdge[PG_MAX_EDGES];                          // src | tgt << 8 | alive << 16 | uncertain << 17
  __shared__ int sLab[PG_MAX_NODES];
  __shared__ int sFlag[PG_F_N];
  const int b = blockIdx.x, tid = threadIdx.x;
  const long long n0 = a.noff[b], e0 = a.eoff[b];
  const long long Sl = a.noff[b + 1] - n0, El = a.eoff[b + 1] - e0;
  const int nmax = 6 * (a.max_s - 1);
  const long long hp = (long long)nmax * (nmax + 1) / 2;
  double* Hg = a.H + hp * b;
  double* gg = a.g + (long long)nmax * b;
  double* dg = a.delta + (long long)nmax * b;
  if (Sl < 1 || Sl > a.max_s || Sl > PG_MAX_NODES || El < 0 || El > PG_MAX_EDGES) {   // sizes the host refuses: nothing is touched
    if (tid == 0) { a.status[b] = 4; a.iterations[b] = 0; a.cost[b] = 0.0; a.lam[b] = 0.0; }
    return;
  }
  const int S = (int)Sl, E = (int)El, n = 6 * (S - 1), rown = n * (n + 1) / 2;
  const double mu = a.mu[b];
  double* X = a.X + 12 * n0;
  const double* T = a.T + 12 * e0;
  const double* Lam = a.Lam + 36 * e0;
  double* ew = a.ew + (long long)PG_EW * e0;

  // ---- the inputs: finite, indices inside the graph
  if (tid < PG_F_N) sFlag[tid] = 0;
  if (tid < S) sLab[tid] = tid;
  __syncthreads();
  {
    bool bad = !isfinite(mu) || !isfinite(a.tol);
    for (int i = tid; i < S * 12; i += PG_THREADS) {
      const double v = X[i];
      sX[i] = v;
      bad |= !isfinite(v);
    }
    for (int i = tid; i < E * 12; i += PG_THREADS) bad |= !isfinite(T[i]);
    for (int i = tid; i < E * 36; i += PG_THREADS) bad |= !isfinite(Lam[i]);
    for (int e = tid; e < E; e += PG_THREADS) {
      const int s = a.src[e0 + e], t = a.tgt[e0 + e];
      const bool in = s >= 0 && s < S && t >= 0 && t < S && s != t;
      bad |= !in;
      sEdge[e] = in ? (s | (t << 8) | ((a.alive[e0 + e] != 0) << 16) | ((a.unc[e0 + e] != 0) << 17)) : 0;
    }
    if (bad) atomicOr(&sFlag[PG_F_BAD], 1);
  }
  for (int i = tid; i < nmax; i += PG_THREADS) { gg[i] = 0.0; dg[i] = 0.0; }
  for (int i = tid; i < 6 * PG_MAX_NODES; i += PG_THREADS) sDelta[i] = 0.0;
  __syncthreads();
  if (sFlag[PG_F_BAD] != 0) {                                  // one LDS word: workgroup-uniform
    for (int e = tid; e < E; e += PG_THREADS) a.l[e0 + e] = 0.0;
    if (tid == 0) { a.status[b] = 4; a.iterations[b] = 0; a.cost[b] = 0.0; a.lam[b] = 0.0; }
    return;
  }

  // ---- is every node joined to node 0 by alive edges?  Label propagation, S rounds (the longest chain has S - 1 edges)
  for (int round = 0; round < S; ++round) {
    for (int e = tid; e < E; e += PG_THREADS) {
      const int pk = sEdge[e];
      if (pk & (1 << 16)) {
        const int s = pk & 255, t = (pk >> 8) & 255;
        const int m = min(sLab[s], sLab[t]);
        atomicMin(&sLab[s], m);
        atomicMin(&sLab[t], m);
      }
    }
    __syncthreads();
  }
  bool joined = true;
  for (int i = 0; i < S; ++i) joined = joined && sLab[i] == 0; // every lane reads the same words

  // the cost of the alive edges under poses P (LDS) -> sVal[slot]; with J the edges' blocks too.  Lane i of wave 0 adds the terms of
  // edges 8 i .. 8 i + 7 in ascending order, then the xor butterfly.
  const auto evaluate = [&](const double* P, int slot, bool with_j, bool write_l) {
    for (int e = tid; e < 512; e += PG_THREADS) {
      double c = 0.0, l = 0.0;
      if (e < E) {
        const int pk = sEdge[e];
        if (pk & (1 << 16)) {
          const bool line = (pk & (1 << 17)) && mu > 0.0;
          const double* xs = P + 12 * (pk & 255);
          const double* xt = P + 12 * ((pk >> 8) & 255);
          const double th = with_j ? pg_edge<true>(xs, xt, T + 12 * e, Lam + 36 * e, line, mu, l, c, ew + PG_EW * e)
                                   : pg_edge<false>(xs, xt, T + 12 * e, Lam + 36 * e, line, mu, l, c, nullptr);
          if (!(th <= PG_THETA_MAX)) atomicOr(&sFlag[PG_F_THETA], 1);
        }
        if (write_l) a.l[e0 + e] = l;
      }
      sCost[e] = c;
    }
    __syncthreads();
    if (tid < 64) {
      double c = 0.0;
#pragma unroll
      for (int k = 0; k < 8; ++k) c += sCost[8 * tid + k];
      c = wave_sum_f64(c);
      if (tid == 0) sVal[slot] = c;
    }
    __syncthreads();
  };

  int status = 1, iterations = 0;
  double lam_used = 0.0;
  if (!joined) status = 2;
  else if (n == 0) status = 0;
  else {
    for (int it = 0; it < a.max_iter; ++it) {                  // uniform: every exit below is decided by words read from LDS
      evaluate(sX, PG_V_F, true, false);
      if (sFlag[PG_F_THETA] != 0) { status = 3; break; }
      iterations = it + 1;
      // g: one lane per unknown, the edges in ascending order (J_tgt = -J_src: the source gets -b, the target +b)
      if (tid < n) {
        const int node = tid / 6 + 1, c = tid % 6;
        double s = 0.0;
        for (int e = 0; e < E; ++e) {
          const int pk = sEdge[e];
          if (pk & (1 << 16)) {
            if ((pk & 255) == node) s -= ew[PG_EW * e + 21 + c];
            else if (((pk >> 8) & 255) == node) s += ew[PG_EW * e + 21 + c];
          }
        }
        gg[tid] = s;
      }
      // H: one lane per pair of free nodes (na >= nb); a diagonal block gets +M of every edge at the node, an off-diagonal one -M of
      // every edge between the two
      const int Sf = S - 1;
      for (int p = tid; p < Sf * (Sf + 1) / 2; p += PG_THREADS) {
        int na = 0;
        while ((na + 1) * (na + 2) / 2 <= p) ++na;
        const int nb = p - na * (na + 1) / 2;
        double acc[21];
#pragma unroll
        for (int k = 0; k < 21; ++k) acc[k] = 0.0;
        for (int e = 0; e < E; ++e) {
          const int pk = sEdge[e];
          if (!(pk & (1 << 16))) continue;
          const int s = (pk & 255) - 1, t = ((pk >> 8) & 255) - 1;
          const double* w = ew + PG_EW * e;
          if (na == nb) {
            if (s == na || t == na) {
#pragma unroll
              for (int k = 0; k < 21; ++k) acc[k] += w[k];
            }
          } else if ((s == na && t == nb) || (s == nb && t == na)) {
#pragma unroll
            for (int k = 0; k < 21; ++k) acc[k] -= w[k];
          }
        }
#pragma unroll
        for (int ci = 0; ci < 6; ++ci) {
          const int i = 6 * na + ci;
#pragma unroll
          for (int cj = 0; cj < 6; ++cj) {
            if (na == nb && cj > ci) continue;
            Hg[i * (i + 1) / 2 + 6 * nb + cj] = acc[ci <= cj ? pg_upper(ci, cj) : pg_upper(cj, ci)];
          }
        }
      }
      __syncthreads();                                         // H and g are written (global, this workgroup's own: the barrier orders them)
      if (it == 0) {
        if (tid < 64) {
          double m = 0.0;
          for (int i = tid; i < n; i += 64) m = fmax(m, Hg[i * (i + 1) / 2 + i]);
          m = wave_max_f64(m);
          if (tid == 0) sVal[PG_V_LAM] = 1e-5 * m;
        }
        __syncthreads();
      }
      int dec = PG_REJECT;
      for (int tries = 0; tries < PG_MAX_TRIES && dec == PG_REJECT; ++tries) {
        const double lam = sVal[PG_V_LAM];
        lam_used = lam;
        // H + lambda I and g into LDS
        for (int i = tid; i < rown; i += PG_THREADS) Lm[i] = Hg[i];
        for (int i = tid; i <= n; i += PG_THREADS) Lm[rown + i] = i < n ? gg[i] : 0.0;
        __syncthreads();
        if (tid < n) Lm[tid * (tid + 1) / 2 + tid] += lam;
        // right-looking Cholesky over rows 0 .. n (row n is g: it leaves as y = L^-1 g)
        bool fail = false;
        const int tx = tid & 15, ty = tid >> 4;
        for (int k = 0; k < n; ++k) {
          __syncthreads();
          const double d = Lm[k * (k + 1) / 2 + k];            // one LDS word: uniform
          if (!(d > 0.0) || !isfinite(d)) { fail = true; break; }
          const double lkk = sqrt(d);
          for (int i = k + 1 + tid; i <= n; i += PG_THREADS) Lm[i * (i + 1) / 2 + k] /= lkk;
          __syncthreads();
          if (tid == 0) Lm[k * (k + 1) / 2 + k] = lkk;
          for (int i = k + 1 + ty; i <= n; i += 16) {
            const double lik = Lm[i * (i + 1) / 2 + k];
            const int jend = i < n ? i : n - 1;
            for (int j = k + 1 + tx; j <= jend; j += 16) Lm[i * (i + 1) / 2 + j] -= lik * Lm[j * (j + 1) / 2 + k];
          }
        }
        if (fail) { dec = PG_FAIL; break; }
        // L^T delta = y
        for (int k = n - 1; k >= 0; --k) {
          __syncthreads();
          const double xk = Lm[rown + k] / Lm[k * (k + 1) / 2 + k];
          if (tid == 0) sDelta[k] = xk;
          for (int j = tid; j < k; j += PG_THREADS) Lm[rown + j] -= Lm[k * (k + 1) / 2 + j] * xk;
        }
        __syncthreads();
        // the trial poses: R <- dR R, t <- dR t + dv (§5.18's step); node 0 stays
        if (tid < S) {
          const double* o = sX + 12 * tid;
          double* nw = sXn + 12 * tid;
          if (tid == 0) {
            for (int e = 0; e < 12; ++e) nw[e] = o[e];
          } else {
            const double* w = sDelta + 6 * (tid - 1);
            const double wx = w[0], wy = w[1], wz = w[2];
            const double t2 = (wx * wx + wy * wy) + wz * wz, t = sqrt(t2);
            double sa, c;
            if (t < 1e-4) {
              sa = 1.0 - t2 / 6.0 + t2 * t2 / 120.0;
              c = 0.5 - t2 / 24.0 + t2 * t2 / 720.0;
            } else {
              sa = sin(t) / t;
              c = (1.0 - cos(t)) / t2;
            }
            double dR[3][3];
            dR[0][0] = 1.0 - c * (wy * wy + wz * wz); dR[0][1] = c * (wx * wy) - sa * wz;       dR[0][2] = c * (wx * wz) + sa * wy;
            dR[1][0] = c * (wx * wy) + sa * wz;       dR[1][1] = 1.0 - c * (wx * wx + wz * wz); dR[1][2] = c * (wy * wz) - sa * wx;
            dR[2][0] = c * (wx * wz) - sa * wy;       dR[2][1] = c * (wy * wz) + sa * wx;       dR[2][2] = 1.0 - c * (wx * wx + wy * wy);
#pragma unroll
            for (int i = 0; i < 3; ++i) {
#pragma unroll
              for (int j = 0; j < 4; ++j) nw[4 * i + j] = (dR[i][0] * o[j] + dR[i][1] * o[4 + j]) + dR[i][2] * o[8 + j];
              nw[4 * i + 3] += w[3 + i];
            }
          }
        }
        __syncthreads();
        evaluate(sXn, PG_V_FN, false, false);
        if (tid == 0) {                                        // the decision: one lane writes it, every lane reads it
          double big = 0.0;
          for (int i = 0; i < n; ++i) big = fmax(big, fabs(sDelta[i]));
          const bool small = big < a.tol;
          int d = PG_REJECT;
          if (sFlag[PG_F_THETA] != 0) d = PG_FAIL;
          else if (sVal[PG_V_FN] < sVal[PG_V_F]) {
            d = small ? PG_DONE : PG_ACCEPT;
            sVal[PG_V_LAM] = fmax(lam / 3.0, PG_LAMBDA_MIN);
          } else if (small) d = PG_FIXED;                   // a fixed point: F cannot fall any more in f64; the poses stay
          else {
            sVal[PG_V_LAM] = 2.0 * lam;
            if (2.0 * lam > PG_LAMBDA_MAX) d = PG_FAIL;
          }
          sFlag[PG_F_DEC] = d;
        }
        __syncthreads();
        dec = sFlag[PG_F_DEC];
        if (dec == PG_ACCEPT || dec == PG_DONE)
          for (int i = tid; i < S * 12; i += PG_THREADS) sX[i] = sXn[i];
        __syncthreads();
      }
      if (dec == PG_FAIL || dec == PG_REJECT) { status = 3; break; }   // PG_REJECT here: the tries ran out
      if (dec != PG_ACCEPT) { status = 0; break; }                     // PG_DONE or PG_FIXED
    }
  }
  // ---- the outputs: l and the cost under the returned poses
  for (int i = tid; i < n; i += PG_THREADS) dg[i] = sDelta[i];
  __syncthreads();
  evaluate(sX, PG_V_F, false, true);
  for (int i = tid; i < S * 12; i += PG_THREADS) X[i] = sX[i];
  if (tid == 0) {
    a.status[b] = status;
    a.iterations[b] = iterations;
    a.cost[b] = sVal[PG_V_F];
    a.lam[b] = lam_used;
  }
}

}  // namespace

extern "C" {

int sfmi_pg_chunk(void) { return SFMI_CHUNK; }
int sfmi_pg_max_nodes(void) { return PG_MAX_NODES; }
int sfmi_pg_max_edges(void) { return PG_MAX_EDGES; }

int sfmi_pg_information_f32(const float* src, const float* tgt, const long long* soff, const long long* toff, const double* pose,
                            const int* idx, const float* d2, const float* maxd2, int B, long long N, long long M, long long max_n,
                            long long max_m, int* bad, double* part, double* info, int* count, int* flag, void* stream) {
  if (B <= 0 || B > 65535 || N < 0 || M < 0 || max_n < 0 || max_m < 0 || max_n >= (1ll << 31) || max_m >= (1ll << 31) || !soff || !toff ||
      !pose || !maxd2 || !bad || !part || !info || !count || !flag || (N > 0 && (!src || !idx || !d2)) || (M > 0 && !tgt))
    return SFMI_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (const int rc = sfmi_pairs_finite<false>(src, tgt, nullptr, soff, toff, nullptr, B, max_n, max_m, bad, st)) return rc;
  const int chunks = (int)(max_n > 0 ? cdiv(max_n, SFMI_CHUNK) : 1);
  if (N > 0 && M > 0)
    hipLaunchKernelGGL(pg_info_kernel, dim3((unsigned)chunks, (unsigned)B), dim3(SFMI_CHUNK_THREADS), 0, st, tgt, soff, toff, pose,
                       (const int*)bad, idx, d2, maxd2, part);
  hipLaunchKernelGGL(pg_info_reduce_kernel, dim3((unsigned)B), dim3(64), 0, st, soff, pose, (const int*)bad, (const double*)part,
                     (N > 0 && M > 0) ? chunks : 0, info, count, flag);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_pg_optimize_f64(const long long* noff, const long long* eoff, int Bg, int max_s, double* X, const int* src, const int* tgt,
                         const double* T, const double* Lam, const int* uncertain, const int* alive, const double* mu, int max_iter,
                         double tol, double* l, double* cost, int* iterations, int* status, double* ework, double* H, double* g,
                         double* delta, double* lam, void* stream) {
  if (Bg <= 0 || max_s < 1 || max_s > PG_MAX_NODES || max_iter < 0 || !(tol >= 0.0) || !noff || !eoff || !X || !src || !tgt || !T || !Lam ||
      !uncertain || !alive || !mu || !l || !cost || !iterations || !status || !ework || !H || !g || !delta || !lam)
    return SFMI_EINVAL;
  const int nmax = 6 * (max_s - 1);
  const size_t lds = (size_t)(nmax + 1) * (nmax + 2) / 2 * sizeof(double);
  // up to 137.3 KB for 32 nodes, above the 64 KB default: raised once per process; a refusal is an error the caller sees
  constexpr int lds_cap = (6 * (PG_MAX_NODES - 1) + 1) * (6 * (PG_MAX_NODES - 1) + 2) / 2 * (int)sizeof(double);
  if (!SFMI_LDS_ONCE(lds_cap, pg_optimize_kernel)) return SFMI_ELDS;
  PgArgs a;
  a.noff = noff; a.eoff = eoff; a.X = X; a.src = src; a.tgt = tgt; a.T = T; a.Lam = Lam; a.unc = uncertain; a.alive = alive; a.mu = mu;
  a.max_iter = max_iter; a.tol = tol; a.max_s = max_s; a.l = l; a.cost = cost; a.iterations = iterations; a.status = status; a.ew = ework;
  a.H = H; a.g = g; a.delta = delta; a.lam = lam;
  hipLaunchKernelGGL(pg_optimize_kernel, dim3((unsigned)Bg), dim3(PG_THREADS), lds, (hipStream_t)stream, a);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

}  // extern "C"
