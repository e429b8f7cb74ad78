// Fast point feature histograms (FPFH, 33 bins) of oriented point clouds and the nearest-neighbour search in their 33-dimensional
// space: what Open3D calls compute_fpfh_feature and the correspondence step of registration_ransac_based_on_feature_matching.  The
// reference has no such step: its real-scan datasets (shapeformer/data/imnet_datasets/redwood.py, realtest.py) serve one cloud in one
// frame.  DESIGN.md §5.19; the contract is stated in include/sfmi.h and restated in numpy in tests/global_reg_ref.py.
//
// 1. spfh_kernel: one wave per point, lane = column of the point's row of sfmi_knn_f32 (k <= 64 = the lanes of a wave).  The pair
//    feature runs across the lanes in f64 with no contraction; the 33 counts are popcount(ballot(bin == b)): no atomics, and no
//    runtime-indexed private array.
// 2. fpfh_kernel: one wave per point, lane j < 33 owns bin j; the neighbours' rows of counts are 132-byte coalesced reads; the three
//    group sums run through the lanes in ascending bin order.
//    orient_kernel: one workgroup per set turns the normals away from the set's centroid (f64 sums in a fixed order), the
//    frame-covariant orientation global_registration_dev uses without viewpoints.
// 3. feature_nn_kernel: sfmi_search.h's split plan, chunk ranges and merge around a tile scan of its own for rows of 33 floats: Q
//    queries per lane in registers (33 VGPRs each), the targets through an LDS tile of 64 rows padded to 36 floats = 9 float4, read
//    as broadcast ds_read_b128; acc = d0 d0, then acc = fmaf(dj, dj, acc) for j = 1..32 (the three pad columns would add fmaf(0, 0,
//    acc) = acc and are not computed); a strict `<` over ascending indices.  When there are too few query blocks the targets are cut
//    into S chunks (grid.y) and the shared merge takes them in ascending chunk order with a strict `<`.
//
// Loop discipline: no kernel waits on another workgroup, there are no spins, every loop around a barrier has workgroup-uniform
// bounds.  An index is range-checked before the row it names is read.
#include "sfmi_search.h"   // the split search (plan, chunk ranges, merge) and the ragged-batch helpers: DESIGN.md §5.5a

// the pair feature and the second stage are written once, here and in numpy: every product and sum rounded on its own
#pragma clang fp contract(off)

namespace {

constexpr int FP_NB = 33;                        // 3 features x 11 bins
constexpr int FP_THREADS = 256;
constexpr int FP_WAVES = FP_THREADS / 64;        // points per workgroup
constexpr int FP_MAX_K = 64;
constexpr double FP_PI = 3.14159265358979323846, FP_TWO_PI = 6.28318530717958647692;
constexpr int OR_THREADS = 1024;
constexpr int OR_WAVES = OR_THREADS / 64;
constexpr int FN_THREADS = 256;
constexpr int FN_TILE = 64;                      // target rows per LDS tile
constexpr int FN_W = 36;                         // floats per row of the tile: 33 padded to 9 float4
constexpr int FN_TARGET_BLOCKS = 2048;           // 256 CUs x 8 workgroups
constexpr int FN_Q_DEFAULT = 2;

inline bool fn_q_ok(int q) { return q == 2 || q == 4; }
inline int fn_splits(int B, long long N, long long M, int q) { return sfmi_splits(B, N, M, FN_TARGET_BLOCKS, FN_THREADS * q); }

// clamp(floor(t), 0, 10); a NaN falls into bin 0 (fmax returns its other argument)
__device__ __forceinline__ int fp_bin(double t) { return (int)fmin(fmax(floor(t), 0.0), 10.0); }

// ---- simplified point feature histograms ----------------------------------------------------------------------------------------------

__global__ __launch_bounds__(FP_THREADS) void spfh_kernel(const float* __restrict__ P, const float* __restrict__ Nrm,
                                                          const long long* __restrict__ off, const int* __restrict__ idx,
                                                          const float* __restrict__ d2, int B, long long N, int k, int use_radius, float r2,
                                                          int* __restrict__ spfh, int* __restrict__ m) {
  const int lane = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * FP_WAVES + (threadIdx.x >> 6);
  if (i >= N) return;                                          // wave-uniform; the kernel has no barrier
  const int b = sfmi_owner(off, B, i);
  const long long base = off[b], n = off[b + 1] - base;
  int j = -1;
  float dd = INFINITY;
  if (lane < k) {
    j = idx[i * k + lane];
    dd = d2[i * k + lane];
  }
  bool ok = j >= 0 && j < n && (!use_radius || dd <= r2);      // the index is checked before the point is read
  int b0 = 0, b1 = 0, b2 = 0;
  if (ok) {
    const long long g = base + j;
    const double n1x = (double)Nrm[3 * i], n1y = (double)Nrm[3 * i + 1], n1z = (double)Nrm[3 * i + 2];
    const double n2x = (double)Nrm[3 * g], n2y = (double)Nrm[3 * g + 1], n2z = (double)Nrm[3 * g + 2];
    double dx = (double)P[3 * g] - (double)P[3 * i], dy = (double)P[3 * g + 1] - (double)P[3 * i + 1],
           dz = (double)P[3 * g + 2] - (double)P[3 * i + 2];
    const double d = sqrt((dx * dx + dy * dy) + dz * dz);
    const double a1 = ((n1x * dx + n1y * dy) + n1z * dz) / d, a2 = ((n2x * dx + n2y * dy) + n2z * dz) / d;
    const bool sw = fabs(a1) < fabs(a2);                       // Open3D's comparison of the two angles, without the acos
    const double nax = sw ? n2x : n1x, nay = sw ? n2y : n1y, naz = sw ? n2z : n1z;
    const double nbx = sw ? n1x : n2x, nby = sw ? n1y : n2y, nbz = sw ? n1z : n2z;
    dx = sw ? -dx : dx; dy = sw ? -dy : dy; dz = sw ? -dz : dz;
    const double f2 = sw ? -a2 : a1;
    double vx = dy * naz - dz * nay, vy = dz * nax - dx * naz, vz = dx * nay - dy * nax;
    const double vn = sqrt((vx * vx + vy * vy) + vz * vz);
    ok = d > 0.0 && vn > 0.0;
    vx = vx / vn; vy = vy / vn; vz = vz / vn;
    const double wx = nay * vz - naz * vy, wy = naz * vx - nax * vz, wz = nax * vy - nay * vx;
    const double f1 = (vx * nbx + vy * nby) + vz * nbz;
    const double f0 = atan2((wx * nbx + wy * nby) + wz * nbz, (nax * nbx + nay * nby) + naz * nbz);
    b0 = fp_bin((11.0 * (f0 + FP_PI)) / FP_TWO_PI);
    b1 = fp_bin((11.0 * (f1 + 1.0)) * 0.5);
    b2 = fp_bin((11.0 * (f2 + 1.0)) * 0.5);
  }
  int mine = 0;
#pragma unroll
  for (int bb = 0; bb < 11; ++bb) {                            // every lane of the wave is here: the ballots see all 64
    const int c0 = __popcll(__ballot(ok && b0 == bb)), c1 = __popcll(__ballot(ok && b1 == bb)), c2 = __popcll(__ballot(ok && b2 == bb));
    mine = lane == bb ? c0 : mine;
    mine = lane == 11 + bb ? c1 : mine;
    mine = lane == 22 + bb ? c2 : mine;
  }
  const int total = __popcll(__ballot(ok));
  if (lane < FP_NB) spfh[i * FP_NB + lane] = mine;
  if (lane == 0) m[i] = total;
}

// ---- the weighted sum over the neighbours ---------------------------------------------------------------------------------------------

__global__ __launch_bounds__(FP_THREADS) void fpfh_kernel(const long long* __restrict__ off, const int* __restrict__ idx,
                                                          const float* __restrict__ d2, const int* __restrict__ spfh,
                                                          const int* __restrict__ m, int B, long long N, int k, int use_radius, float r2,
                                                          float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * FP_WAVES + (threadIdx.x >> 6);
  if (i >= N) return;                                          // wave-uniform; the kernel has no barrier
  const int b = sfmi_owner(off, B, i);
  const long long base = off[b], n = off[b + 1] - base;
  const int col = lane < FP_NB ? lane : 0;                     // lanes 33..63 shadow bin 0 and write nothing
  const int mi = m[i];
  const double s = mi > 0 ? (double)spfh[i * FP_NB + col] * (100.0 / (double)mi) : 0.0;
  double F = 0.0;
  for (int c = 0; c < k; ++c) {                                // wave-uniform: every lane reads the same (idx, d2)
    const int nb = idx[i * k + c];
    const float dd = d2[i * k + c];
    if (nb < 0 || nb >= n || (use_radius && !(dd <= r2)) || !(dd > 0.f)) continue;
    const long long g = base + nb;
    const int mn = m[g];
    const double sn = mn > 0 ? (double)spfh[g * FP_NB + col] * (100.0 / (double)mn) : 0.0;
    F = F + sn / (double)dd;
  }
  const int g0 = (col / 11) * 11;
  double t = __shfl(F, g0, 64);
#pragma unroll
  for (int bb = 1; bb < 11; ++bb) t = t + __shfl(F, g0 + bb, 64);   // the group's bins in ascending order
  if (t != 0.0) F = F * (100.0 / t);
  if (lane < FP_NB) out[i * FP_NB + lane] = (float)(F + s);
}

// ---- normals turned away from the set's centroid ----------------------------------------------------------------------------------------

// one workgroup per set: the centroid of the set's finite points in f64 in a fixed order (a lane's points ascending, wave_sum_f64, a
// fixed tree over the 16 waves), then n <- -n where (p - c).n < 0.  A set's result depends on that set alone.
__global__ __launch_bounds__(OR_THREADS) void orient_kernel(const float* __restrict__ P, const long long* __restrict__ off,
                                                            float* __restrict__ Nrm) {
  __shared__ double red[OR_WAVES];
  const int b = blockIdx.x, tid = threadIdx.x;
  const long long base = off[b], n = off[b + 1] - base;
  const float* Pb = P + 3 * base;
  float* Nb = Nrm + 3 * base;
  double cx, cy, cz;
  if (!sfmi_centroid_f64<OR_WAVES>(Pb, n, red, cx, cy, cz)) return;   // workgroup-uniform: no finite point, nothing is turned
  for (long long i = tid; i < n; i += OR_THREADS) {
    const double x = (double)Pb[3 * i] - cx, y = (double)Pb[3 * i + 1] - cy, z = (double)Pb[3 * i + 2] - cz;
    const float nx = Nb[3 * i], ny = Nb[3 * i + 1], nz = Nb[3 * i + 2];
    if (((x * (double)nx + y * (double)ny) + z * (double)nz) < 0.0) {   // a NaN turns nothing
      Nb[3 * i] = -nx; Nb[3 * i + 1] = -ny; Nb[3 * i + 2] = -nz;
    }
  }
}

// ---- nearest neighbours in feature space ------------------------------------------------------------------------------------------------

// grid (query blocks, S).  S == 1: d_out / i_out are the results; S > 1: partial buffers, chunk s at d_out + s * N.
template <int Q>
__global__ __launch_bounds__(FN_THREADS) void feature_nn_kernel(const float* __restrict__ A, const float* __restrict__ Bf,
                                                                const long long* __restrict__ aoff, const long long* __restrict__ boff,
                                                                const long long* __restrict__ block_off, int B, long long N,
                                                                float* __restrict__ d_out, int* __restrict__ i_out) {
  constexpr int QB = FN_THREADS * Q;
  __shared__ __attribute__((aligned(16))) float tile[FN_TILE * FN_W];
  const long long g = blockIdx.x;
  if (g >= block_off[B]) return;                               // block-uniform, before any barrier
  const int b = sfmi_owner(block_off, B, g);
  const int tid = threadIdx.x;
  const long long aend = aoff[b + 1];
  const long long qbase = aoff[b] + (g - block_off[b]) * QB;
  float a[Q][FP_NB], best[Q];
  int bi[Q];
#pragma unroll
  for (int r = 0; r < Q; ++r) {
    const long long i = qbase + r * FN_THREADS + tid;
    const bool ok = i < aend;
#pragma unroll
    for (int j = 0; j < FP_NB; ++j) a[r][j] = ok ? A[i * FP_NB + j] : 0.f;
    best[r] = INFINITY;
    bi[r] = -1;
  }
  const long long q0 = boff[b];
  long long j0, j1;
  sfmi_chunk_range(q0, boff[b + 1], gridDim.y, blockIdx.y, j0, j1);
  for (long long t0 = j0; t0 < j1; t0 += FN_TILE) {            // workgroup-uniform bounds
    __syncthreads();                                           // the previous tile is consumed
    for (int e = tid; e < FN_TILE * FN_W; e += FN_THREADS) {
      const int row = e / FN_W, col = e - row * FN_W;
      const long long j = t0 + row;
      // padding past the chunk: +inf gives d2 = inf (or NaN), never < best (strict), so it is never selected
      tile[e] = j < j1 ? (col < FP_NB ? Bf[j * FP_NB + col] : 0.f) : INFINITY;
    }
    __syncthreads();
    const int jb = (int)(t0 - q0);                             // local index of the tile's first row (M_b < 2^31)
#pragma unroll 2
    for (int jj = 0; jj < FN_TILE; ++jj) {
      const float4* row = reinterpret_cast<const float4*>(tile + jj * FN_W);
      float q[FN_W];
#pragma unroll
      for (int c = 0; c < FN_W / 4; ++c) {                     // broadcast ds_read_b128
        const float4 v = row[c];
        q[4 * c] = v.x; q[4 * c + 1] = v.y; q[4 * c + 2] = v.z; q[4 * c + 3] = v.w;
      }
#pragma unroll
      for (int r = 0; r < Q; ++r) {
        float d = a[r][0] - q[0];
        float acc = d * d;
#pragma unroll
        for (int j = 1; j < FP_NB; ++j) {
          d = a[r][j] - q[j];
          acc = fmaf(d, d, acc);
        }
        const bool lt = acc < best[r];
        best[r] = lt ? acc : best[r];
        bi[r] = lt ? jb + jj : bi[r];
      }
    }
  }
  float* dd = d_out + (long long)blockIdx.y * N;
  int* ii = i_out + (long long)blockIdx.y * N;
#pragma unroll
  for (int r = 0; r < Q; ++r) {
    const long long i = qbase + r * FN_THREADS + tid;
    if (i < aend) {
      dd[i] = best[r];
      ii[i] = bi[r];
    }
  }
}

template <int Q>
void fn_launch(const float* A, const float* Bf, const long long* aoff, const long long* boff, const long long* block_off, int B, long long N,
               long long n_blocks, int S, float* d, int* i, hipStream_t st) {
  hipLaunchKernelGGL(feature_nn_kernel<Q>, dim3((unsigned)n_blocks, (unsigned)S), dim3(FN_THREADS), 0, st, A, Bf, aoff, boff, block_off, B, N,
                     d, i);
}

}  // namespace

extern "C" {

int sfmi_fpfh_query_block(int q) { return fn_q_ok(q ? q : FN_Q_DEFAULT) ? FN_THREADS * (q ? q : FN_Q_DEFAULT) : 0; }
int sfmi_fpfh_tile(void) { return FN_TILE; }
int sfmi_fpfh_nn_splits(int B, long long N, long long M, int q) {
  q = q ? q : FN_Q_DEFAULT;
  return (B <= 0 || N < 0 || M < 0 || !fn_q_ok(q)) ? 0 : fn_splits(B, N, M, q);
}

int sfmi_fpfh_spfh_f32(const float* P, const float* Nrm, const long long* off, const int* idx, const float* d2, int B, long long N, int k,
                       int use_radius, float r2, int* spfh, int* m, void* stream) {
  if (B <= 0 || N < 0 || k < 1 || k > FP_MAX_K || !off || (use_radius && !(r2 >= 0.f))) return SFMI_EINVAL;
  if (N == 0) return SFMI_OK;
  if (!P || !Nrm || !idx || !d2 || !spfh || !m) return SFMI_EINVAL;
  hipLaunchKernelGGL(spfh_kernel, dim3((unsigned)cdiv(N, FP_WAVES)), dim3(FP_THREADS), 0, (hipStream_t)stream, P, Nrm, off, idx, d2, B, N, k,
                     use_radius, r2, spfh, m);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_fpfh_features_f32(const long long* off, const int* idx, const float* d2, const int* spfh, const int* m, int B, long long N, int k,
                           int use_radius, float r2, float* out, void* stream) {
  if (B <= 0 || N < 0 || k < 1 || k > FP_MAX_K || !off || (use_radius && !(r2 >= 0.f))) return SFMI_EINVAL;
  if (N == 0) return SFMI_OK;
  if (!idx || !d2 || !spfh || !m || !out) return SFMI_EINVAL;
  hipLaunchKernelGGL(fpfh_kernel, dim3((unsigned)cdiv(N, FP_WAVES)), dim3(FP_THREADS), 0, (hipStream_t)stream, off, idx, d2, spfh, m, B, N, k,
                     use_radius, r2, out);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_fpfh_orient_f32(const float* P, const long long* off, int B, long long N, float* Nrm, void* stream) {
  if (B <= 0 || B > 65535 || N < 0 || !off) return SFMI_EINVAL;
  if (N == 0) return SFMI_OK;
  if (!P || !Nrm) return SFMI_EINVAL;
  hipLaunchKernelGGL(orient_kernel, dim3((unsigned)B), dim3(OR_THREADS), 0, (hipStream_t)stream, P, off, Nrm);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_fpfh_nn_f32(const float* A, const float* Bf, const long long* aoff, const long long* boff, const long long* block_off, int B,
                     long long N, long long M, long long n_blocks, int splits, int q, int* idx, float* d2, float* part_d2, int* part_idx,
                     void* stream) {
  q = q ? q : FN_Q_DEFAULT;
  if (B <= 0 || B > 65535 || N < 0 || M < 0 || n_blocks < 0 || n_blocks >= (1ll << 31) || !fn_q_ok(q) || splits < 0 ||
      splits > SFMI_MAX_SPLITS || !aoff || !boff || !block_off)
    return SFMI_EINVAL;
  if (N == 0 || n_blocks == 0) return SFMI_OK;
  if (!A || !idx || !d2 || (M > 0 && !Bf)) return SFMI_EINVAL;
  const int S = splits ? splits : fn_splits(B, N, M, q);
  if (S > 1 && (!part_d2 || !part_idx)) return SFMI_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  float* d = S > 1 ? part_d2 : d2;
  int* i = S > 1 ? part_idx : idx;
  if (q == 2) fn_launch<2>(A, Bf, aoff, boff, block_off, B, N, n_blocks, S, d, i, st);
  else fn_launch<4>(A, Bf, aoff, boff, block_off, B, N, n_blocks, S, d, i, st);
  if (S > 1) sfmi_nn_merge<true, false>(part_d2, part_idx, nullptr, nullptr, B, S, N, d2, idx, st);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

}  // extern "C"
