// Point-set distances and mesh surface sampling on the GPU: the evaluation metrics of a completion (Chamfer distance, F-score,
// UHD, TMD) straight from the marching-cubes output, without a device-to-host copy.  The reference scores point sets on the CPU
// with scipy cKDTree (xgutils/geoutil.py:362-377 points_dist / chamfer_dist; shapeformer/models/vqdif/common.py:39-122
// chamfer_distance) and samples meshes with igl.random_points_on_mesh (xgutils/geoutil.py:236-253 sampleMesh).
//
// 1. Exact batched 1-nearest-neighbour, brute force (10^5 x 10^5 = 10^10 pairs, ~9 VALU lane-ops each).
//    Ragged sets P_b (queries) and Q_b (references) given by int64 offsets.  A workgroup holds 256 lanes x NN_R queries per
//    lane in registers; Q is fed through an LDS tile of float4 read as a broadcast ds_read_b128 (every lane the same address),
//    so one LDS read feeds NN_R distance evaluations.  Distance in ONE expression order, the direct form:
//        d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx)),  (dx, dy, dz) = p - q
//    (never |p|^2 - 2 p.q + |q|^2: at surface-sample spacing its cancellation error ~|p|^2 2^-24 is a large relative error).
//    Ties: Q is scanned in ascending order with a strict `<`, so the lowest index among equal f32 distances wins.
//    Filling the chip: when there are too few query blocks, Q_b is cut into S contiguous chunks (grid.y); chunk s writes a
//    partial (d2, idx) per query and a second launch merges the S partials in ascending chunk order with a strict `<` (the
//    lower index wins a tie again).  No atomics: results are bit-identical from run to run and do not depend on S.
//    The plan, the block offsets, the search and the merge are sfmi_search.h's, shared with knn.hip, register.hip and features.hip;
//    nn_kernel is the block's owner and the plain query load around sfmi_search3.
// 2. Area-weighted surface sampling of a batch of indexed meshes: per-face areas in f64, a per-shape inclusive f64 CDF (one
//    workgroup per shape, fixed summation order), then one thread per sample: the face by binary search on a counter-hash
//    uniform of (seed, sample), barycentric weights 1-sqrt(u), sqrt(u)(1-v), sqrt(u) v as in geoutil.sampleMesh.
#include "sfmi_search.h"   // the split search (plan, block offsets, scan, merge) and the ragged-batch helpers: DESIGN.md §5.5a

namespace {

constexpr int NN_THREADS = SFMI_SCAN_TILE;
constexpr int NN_R = 8;                          // queries per lane (registers: 3 coordinates + best d2 + best index each)
constexpr int NN_QB = NN_THREADS * NN_R;         // queries per workgroup
constexpr int NN_TARGET_BLOCKS = 2048;           // 256 CUs x 8 workgroups

inline int nn_splits(int B, long long N, long long M) { return sfmi_splits(B, N, M, NN_TARGET_BLOCKS, NN_QB); }

// grid (query blocks upper bound, S).  S == 1: d_out / i_out are the results (i_out may be null); S > 1: partial buffers,
// chunk s at d_out + s * N.
__global__ __launch_bounds__(NN_THREADS) void nn_kernel(const float* __restrict__ P, const float* __restrict__ Q,
                                                        const long long* __restrict__ poff, const long long* __restrict__ qoff,
                                                        const long long* __restrict__ block_off, int B, long long N,
                                                        float* __restrict__ d_out, int* __restrict__ i_out) {
  const long long g = blockIdx.x;
  if (g >= block_off[B]) return;                               // block-uniform: the grid is an upper bound
  const int b = sfmi_owner(block_off, B, g);
  const auto load = [P](long long i, bool ok, float& x, float& y, float& z) {
    x = ok ? P[3 * i] : 0.f;
    y = ok ? P[3 * i + 1] : 0.f;
    z = ok ? P[3 * i + 2] : 0.f;
  };
  sfmi_search3<NN_R>(Q, qoff[b], qoff[b + 1], poff[b] + (g - block_off[b]) * NN_QB, poff[b + 1], load,
                      d_out + (long long)blockIdx.y * N, i_out ? i_out + (long long)blockIdx.y * N : nullptr);
}

// ---- mesh sampling ---------------------------------------------------------------------------------------------------------

// per-face area (f64) of face t; a vertex index outside its shape gives NaN, which flags the shape
__global__ void mesh_area_kernel(const float* __restrict__ verts, const int* __restrict__ faces, const long long* __restrict__ voff,
                                 const long long* __restrict__ toff, int B, long long T, double* __restrict__ area) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= T) return;
  const int b = sfmi_owner(toff, B, t);
  const long long v0 = voff[b], nv = voff[b + 1] - v0;
  double p[3][3];
  bool ok = true;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int k = faces[3 * t + c];
    ok = ok && k >= 0 && k < nv;
    const long long v = v0 + (ok ? k : 0);
#pragma unroll
    for (int a = 0; a < 3; ++a) p[c][a] = ok ? (double)verts[3 * v + a] : 0.0;
  }
  const double e1x = p[1][0] - p[0][0], e1y = p[1][1] - p[0][1], e1z = p[1][2] - p[0][2];
  const double e2x = p[2][0] - p[0][0], e2y = p[2][1] - p[0][1], e2z = p[2][2] - p[0][2];
  const double cx = e1y * e2z - e1z * e2y, cy = e1z * e2x - e1x * e2z, cz = e1x * e2y - e1y * e2x;
  area[t] = ok ? 0.5 * sqrt(cx * cx + cy * cy + cz * cz) : sfmi_nan_f64();
}

// one workgroup per shape: area -> inclusive CDF in place, in a fixed order (each lane a contiguous run, Hillis-Steele over the
// 256 run sums); status[b] = 0 when the total area is finite and > 0, else 1 (no faces, zero area, or a bad vertex index)
constexpr int CDF_THREADS = 256;
__global__ __launch_bounds__(CDF_THREADS) void mesh_cdf_kernel(const long long* __restrict__ toff, double* __restrict__ cdf,
                                                              int* __restrict__ status) {
  __shared__ double sums[CDF_THREADS];
  const int b = blockIdx.x, tid = threadIdx.x;
  const long long t0 = toff[b], nt = toff[b + 1] - t0;
  if (nt <= 0) {
    if (tid == 0) status[b] = 1;
    return;
  }
  const long long run = cdiv(nt, CDF_THREADS);
  const long long r0 = t0 + tid * run, r1 = (r0 + run < t0 + nt) ? r0 + run : t0 + nt;
  double s = 0.0;
  for (long long t = r0; t < r1; ++t) s += cdf[t];
  sums[tid] = s;
  __syncthreads();
  for (int o = 1; o < CDF_THREADS; o <<= 1) {
    const double add = tid >= o ? sums[tid - o] : 0.0;
    __syncthreads();
    sums[tid] += add;
    __syncthreads();
  }
  double acc = tid ? sums[tid - 1] : 0.0;
  for (long long t = r0; t < r1; ++t) {
    acc += cdf[t];
    cdf[t] = acc;
  }
  if (r0 < r1 && r1 == t0 + nt) status[b] = (acc > 0.0 && acc < INFINITY) ? 0 : 1;   // the lane that wrote the total
}

__global__ void mesh_sample_kernel(const float* __restrict__ verts, const int* __restrict__ faces, const long long* __restrict__ voff,
                                   const long long* __restrict__ toff, const double* __restrict__ cdf, int B, long long n,
                                   unsigned long long seed, float* __restrict__ out, int* __restrict__ face_out) {
  const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (long long)B * n) return;
  const int b = (int)(g / n);
  const long long k = g - (long long)b * n;
  const long long t0 = toff[b], nt = toff[b + 1] - t0;
  const double tot = nt > 0 ? cdf[t0 + nt - 1] : 0.0;
  if (!(tot > 0.0 && tot < INFINITY)) {
    out[3 * g] = out[3 * g + 1] = out[3 * g + 2] = __int_as_float(0x7FC00000);
    if (face_out) face_out[g] = -1;
    return;
  }
  // the stream depends on (seed, k) only: shape b's samples do not depend on the batch around it
  const unsigned long long s0 = sfmi_mix64(seed);
  const unsigned long long hf = sfmi_mix64(s0 + 3 * (unsigned long long)k), hu = sfmi_mix64(s0 + 3 * (unsigned long long)k + 1),
                           hv = sfmi_mix64(s0 + 3 * (unsigned long long)k + 2);
  const double target = (double)(hf >> 11) * 0x1.0p-53 * tot;
  long long lo = 0, hi = nt - 1;                               // first face with cdf > target (clamped to the last)
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (cdf[t0 + mid] > target) hi = mid; else lo = mid + 1;
  }
  const long long t = t0 + lo;
  const float u = (float)(hu >> 40) * 0x1.0p-24f, v = (float)(hv >> 40) * 0x1.0p-24f;
  const float su = sqrtf(u);
  const float w0 = 1.f - su, w1 = su * (1.f - v), w2 = su * v;
  const long long v0 = voff[b];
  const long long ia = v0 + faces[3 * t], ib = v0 + faces[3 * t + 1], ic = v0 + faces[3 * t + 2];   // valid: tot is finite
#pragma unroll
  for (int a = 0; a < 3; ++a)
    out[3 * g + a] = fmaf(w2, verts[3 * ic + a], fmaf(w1, verts[3 * ib + a], w0 * verts[3 * ia + a]));
  if (face_out) face_out[g] = (int)lo;
}

struct NnWs { int S; long long* block_off; float* pd; int* pi; };   // pd, pi: S > 1 only

// workspace: block offsets (B+1 int64) | S > 1: partial d2 (S*N f32) | partial idx (S*N int32)
NnWs nn_ws(SfmiCarver& c, int B, long long N, long long M) {
  NnWs w{nn_splits(B, N, M), c.take<long long>((size_t)(B + 1)), nullptr, nullptr};
  if (w.S > 1) {
    w.pd = c.take<float>((size_t)w.S * N);
    w.pi = c.take<int>((size_t)w.S * N);
  }
  return w;
}

}  // namespace

extern "C" {

size_t sfmi_nn_dist_workspace_bytes(int B, long long N, long long M) {
  if (B <= 0 || N < 0 || M < 0) return 0;
  return sfmi_ws_bytes(nn_ws, B, N, M);
}

int sfmi_nn_dist_f32(const float* P, const float* Q, const long long* poff, const long long* qoff, int B, long long N, long long M,
                     float* d2, int* idx, void* workspace, void* stream) {
  if (B <= 0 || N < 0 || M < 0 || M >= (1ll << 31) || !poff || !qoff || !workspace) return SFMI_EINVAL;
  if (N == 0) return SFMI_OK;
  if (!P || !Q || !d2) return SFMI_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  SfmiCarver carver{(char*)workspace};
  const NnWs w = nn_ws(carver, B, N, M);
  hipLaunchKernelGGL(sfmi_block_offsets_kernel<NN_QB>, dim3(1), dim3(64), 0, st, poff, w.block_off, B);
  const dim3 grid((unsigned)sfmi_qblocks(B, N, NN_QB), (unsigned)w.S);
  if (w.S == 1) {
    hipLaunchKernelGGL(nn_kernel, grid, dim3(NN_THREADS), 0, st, P, Q, poff, qoff, (const long long*)w.block_off, B, N, d2, idx);
  } else {
    hipLaunchKernelGGL(nn_kernel, grid, dim3(NN_THREADS), 0, st, P, Q, poff, qoff, (const long long*)w.block_off, B, N, w.pd, w.pi);
    if (idx) sfmi_nn_merge<true, false>(w.pd, w.pi, nullptr, nullptr, B, w.S, N, d2, idx, st);
    else sfmi_nn_merge<false, false>(w.pd, w.pi, nullptr, nullptr, B, w.S, N, d2, idx, st);
  }
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

// workspace: per-face CDF (T f64)
size_t sfmi_mesh_sample_workspace_bytes(int B, long long T) {
  if (B <= 0 || T < 0) return 0;
  return align256((size_t)(T > 0 ? T : 1) * 8);
}

int sfmi_mesh_sample_f32(const float* verts, const int* faces, const long long* voff, const long long* toff, int B, long long T,
                         long long n, unsigned long long seed, void* workspace, float* out, int* face_out, int* status, void* stream) {
  if (B <= 0 || T < 0 || n < 0 || !voff || !toff || !workspace || !status || (T > 0 && (!verts || !faces))) return SFMI_EINVAL;
  if (n > 0 && !out) return SFMI_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  double* cdf = (double*)workspace;
  if (T > 0) hipLaunchKernelGGL(mesh_area_kernel, dim3((unsigned)cdiv(T, 256)), dim3(256), 0, st, verts, faces, voff, toff, B, T, cdf);
  hipLaunchKernelGGL(mesh_cdf_kernel, dim3((unsigned)B), dim3(CDF_THREADS), 0, st, toff, cdf, status);
  if (n > 0)
    hipLaunchKernelGGL(mesh_sample_kernel, dim3((unsigned)cdiv((long long)B * n, 256)), dim3(256), 0, st, verts, faces, voff, toff,
                       (const double*)cdf, B, n, seed, out, face_out);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

}  // extern "C"
