// Exact k-nearest neighbours over ragged point sets, and what a scan-cleaning front end builds on them: the mean neighbour distance
// of statistical outlier removal (PCL StatisticalOutlierRemoval) and point normals by local PCA.  The reference asks scipy for them on
// the host (xgutils/geoutil.py:362-366 points_dist: cKDTree(p2).query(p1, k)); its real-scan datasets (shapeformer/data/imnet_datasets/
// redwood.py, realtest.py) feed raw .pts clouds, flying pixels included, straight to the encoder.  DESIGN.md §5.14.
//
// 1. knn_kernel<K, R, EXCL, SLOTS>: brute force, on sfmi_search.h's split plan, block offsets and chunk ranges like nn_kernel in
//    pointdist.hip.  The feed of sfmi_search3 (256 lanes x R queries per lane in registers, Q through a 256-point float4 LDS tile read
//    as a broadcast ds_read_b128) and its distance expression in the same order, d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx)), so column 0
//    is nn_kernel's result bit for bit; the inner loop is its own, because it keeps a list.
//    Each query keeps a sorted list of K (d2, index) pairs in registers.  A candidate is first compared with the list's last entry
//    (the common case ends there: one compare on top of nn_kernel's work); only a smaller one runs a fully unrolled
//    compare-and-shift chain through the K slots.  Every list index is a compile-time constant: nothing goes to scratch.
//    Ties: Q is scanned in ascending order and every compare is a strict `<`, so an entry never passes an equal one that came before
//    it: rows are ascending in (d2, index), the lower index first among equal f32 distances.
//    Instances K = 8, 16, 32, 64 with R = 4, 2, 1, 1; a requested k runs the smallest K >= k and writes its first k columns.
//    K = 32 and 64 park candidates in SLOTS lane-private LDS slots and insert them wave-wide (knn_flush below says why).
//    EXCL (P and Q are the same sets): the candidate whose local index is the query's own is skipped, by index and not by distance, so
//    duplicates of a point remain its neighbours.
//    Filling the chip: with few query blocks Q_b is cut into S contiguous chunks (grid.y), chunk s writes a partial list per query
//    (column-major, so both sides are coalesced) and knn_merge_kernel<K> feeds the S lists, in ascending chunk order, through the
//    same insertion.  No atomics: the result is bit-identical from run to run and does not depend on S.
// 2. knn_mean_dist_kernel: per point the mean over the k columns of sqrt(d2) in f64, in column order.
// 3. knn_normals_kernel: one lane per point: centroid and 3x3 covariance of its neighbours in f64 in the table's column order, the
//    eigenvector of the smallest eigenvalue by a fixed number of cyclic Jacobi sweeps in f64 (no data-dependent trip count).
#include "sfmi_search.h"   // the split search (plan, block offsets, chunk ranges) and the ragged-batch helpers: DESIGN.md §5.5a

namespace {

constexpr int KNN_THREADS = 256;
constexpr int KNN_TILE = 256;                    // Q points per LDS tile (float4: 4 KiB)
constexpr int KNN_MAX_K = 64;
constexpr size_t KNN_MAX_PARTIAL = (size_t)256 << 20;   // bytes of partial lists: the split is cut down to stay below it

// the instance that serves k: its list length, its queries per lane, and how many workgroups the split aims at (a workgroup is one
// wave per SIMD; 256 CUs x 3 .. 5 resident workgroups.  The timings of DESIGN.md §5.14 were taken with these values)
inline int knn_instance(int k) { return k <= 8 ? 8 : (k <= 16 ? 16 : (k <= 32 ? 32 : 64)); }
inline int knn_r(int K) { return K == 8 ? 4 : (K == 16 ? 2 : 1); }
inline int knn_target_blocks(int K) { return K <= 16 ? 1280 : (K == 32 ? 1024 : 768); }

// the split is also cut down to keep the partial lists below KNN_MAX_PARTIAL
inline int knn_splits(int B, long long N, long long M, int K) {
  return sfmi_splits(B, N, M, knn_target_blocks(K), KNN_THREADS * knn_r(K), (long long)(KNN_MAX_PARTIAL / ((size_t)(N > 0 ? N : 1) * K * 8)));
}

// (d, j) enters the sorted list when it is smaller than the last entry: every entry that d is strictly smaller than moves one slot
// back and d takes the slot in front of them - behind every entry <= d, so an equal entry that came earlier stays in front.  Written
// slot by slot from the back (slot s takes its predecessor, d, or stays) and not as exchanges of neighbours: the compares are of the
// one d against K entries, independent of each other, and the compiler keeps it linear (it expanded the exchange form of K = 32 into
// 2000 selects per insertion).  All indices are compile-time constants after unrolling.
template <int K>
__device__ __forceinline__ void knn_insert(float (&dl)[K], int (&il)[K], float d, int j) {
  if (d < dl[K - 1]) {
    bool here = true;                                          // d < dl[s], the list as it was
#pragma unroll
    for (int s = K - 1; s > 0; --s) {
      const bool before = d < dl[s - 1];
      dl[s] = before ? dl[s - 1] : (here ? d : dl[s]);
      il[s] = before ? il[s - 1] : (here ? j : il[s]);
      here = before;
    }
    dl[0] = here ? d : dl[0];
    il[0] = here ? j : il[0];
  }
}

// The long lists (K = 32, 64) do not insert candidate by candidate: a wave runs the chain whenever ANY of its 64 lanes inserts, and with
// K ln(M / K) insertions per lane that is most candidates (measured: 160 x the k = 1 time).  There a candidate that beats the lane's
// threshold - the last list entry as of the latest flush, so never tighter than the true one - is parked in one of SLOTS lane-private
// LDS slots, and the wave flushes together when some lane runs out of slots: each lane feeds its slots, in arrival order, through
// knn_insert, which compares with the true last entry again.  The chain then runs about once per insertion of the busiest lane, not
// once per insertion of any lane.  A lane's candidates still reach its list in ascending index order: the tie rule is untouched.
template <int K, int SLOTS>
__device__ __forceinline__ void knn_flush(float (&dl)[K], int (&il)[K], const float2* park, int tid, int cnt) {
#pragma unroll 1
  for (int s = 0; s < SLOTS; ++s) {
    if (s < cnt) {
      const float2 e = park[s * KNN_THREADS + tid];
      knn_insert<K>(dl, il, e.x, __float_as_int(e.y));
    }
  }
}

// grid (query blocks upper bound, S).  S == 1: d_out / i_out are the (N, k) results; S > 1: partial lists, column c of query i of
// chunk s at [(s * K + c) * N + i] (all K columns).
template <int K, int R, bool EXCL, int SLOTS>
__global__ __launch_bounds__(KNN_THREADS) void knn_kernel(const float* __restrict__ P, const float* __restrict__ Q,
                                                          const long long* __restrict__ poff, const long long* __restrict__ qoff,
                                                          const long long* __restrict__ block_off, int B, long long N, int k,
                                                          float* __restrict__ d_out, int* __restrict__ i_out) {
  constexpr int QB = KNN_THREADS * R;
  constexpr int CHECK = SLOTS / 2;                             // candidates between two looks at the pending counts
  static_assert(SLOTS == 0 || (R == 1 && CHECK >= 1 && KNN_TILE % CHECK == 0), "pending slots go with one query per lane");
  __shared__ float4 tile[KNN_TILE];
  __shared__ float2 park[SLOTS > 0 ? SLOTS * KNN_THREADS : 1];  // slot s of lane t at [s * 256 + t]: (d2, index bits), lane-private
  const long long g = blockIdx.x;
  if (g >= block_off[B]) return;                               // block-uniform: the grid is an upper bound
  const int b = sfmi_owner(block_off, B, g);
  const int tid = threadIdx.x;
  const long long pbeg = poff[b], pend = poff[b + 1];
  const long long qbase = pbeg + (g - block_off[b]) * QB;
  float px[R], py[R], pz[R];
  int self[R];
  float dl[R][K];
  int il[R][K];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const long long i = qbase + r * KNN_THREADS + tid;
    const bool ok = i < pend;
    px[r] = ok ? P[3 * i] : 0.f;
    py[r] = ok ? P[3 * i + 1] : 0.f;
    pz[r] = ok ? P[3 * i + 2] : 0.f;
    self[r] = (int)(i - pbeg);                                 // local index of the query (N_b = M_b < 2^31 with EXCL)
#pragma unroll
    for (int c = 0; c < K; ++c) {
      dl[r][c] = INFINITY;
      il[r][c] = -1;
    }
  }
  const long long q0 = qoff[b];
  long long j0, j1;
  sfmi_chunk_range(q0, qoff[b + 1], gridDim.y, blockIdx.y, j0, j1);
  float thr = INFINITY;                                        // SLOTS > 0: the last list entry as of the latest flush
  int cnt = 0;                                                 //            pending candidates of this lane
  for (long long t0 = j0; t0 < j1; t0 += KNN_TILE) {
    __syncthreads();                                           // the previous tile is consumed
    {
      const long long j = t0 + tid;
      // padding past the chunk: +inf coordinates give d2 = inf (or NaN), never < the last entry, so they are never inserted
      tile[tid] = j < j1 ? make_float4(Q[3 * j], Q[3 * j + 1], Q[3 * j + 2], 0.f) : make_float4(INFINITY, INFINITY, INFINITY, 0.f);
    }
    __syncthreads();
    const int jb = (int)(t0 - q0);                             // local index of the tile's first point (M_b < 2^31)
    if constexpr (SLOTS == 0) {
#pragma unroll 2
      for (int jj = 0; jj < KNN_TILE; ++jj) {
        const float4 q = tile[jj];                             // broadcast ds_read_b128
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const float dx = px[r] - q.x, dy = py[r] - q.y, dz = pz[r] - q.z;
          float d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
          if (EXCL) d2 = (jb + jj == self[r]) ? INFINITY : d2;
          knn_insert<K>(dl[r], il[r], d2, jb + jj);
        }
      }
    } else {
      for (int jj = 0; jj < KNN_TILE; jj += CHECK) {
#pragma unroll
        for (int u = 0; u < CHECK; ++u) {
          const float4 q = tile[jj + u];                       // broadcast ds_read_b128
          const float dx = px[0] - q.x, dy = py[0] - q.y, dz = pz[0] - q.z;
          float d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
          if (EXCL) d2 = (jb + jj + u == self[0]) ? INFINITY : d2;
          if (d2 < thr) {                                      // cnt <= SLOTS - CHECK before the group: the slot exists
            park[cnt * KNN_THREADS + tid] = make_float2(d2, __int_as_float(jb + jj + u));
            ++cnt;
          }
        }
        if (__any(cnt > SLOTS - CHECK)) {                      // wave-uniform: some lane could overflow in the next group
          knn_flush<K, SLOTS>(dl[0], il[0], park, tid, cnt);
          cnt = 0;
          thr = dl[0][K - 1];
        }
      }
    }
  }
  if constexpr (SLOTS > 0) knn_flush<K, SLOTS>(dl[0], il[0], park, tid, cnt);
  if (gridDim.y == 1) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const long long i = qbase + r * KNN_THREADS + tid;
      if (i < pend) {
#pragma unroll
        for (int c = 0; c < K; ++c)
          if (c < k) {
            d_out[i * k + c] = dl[r][c];
            i_out[i * k + c] = il[r][c];
          }
      }
    }
  } else {
    float* dd = d_out + (long long)blockIdx.y * K * N;
    int* ii = i_out + (long long)blockIdx.y * K * N;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const long long i = qbase + r * KNN_THREADS + tid;
      if (i < pend) {
#pragma unroll
        for (int c = 0; c < K; ++c) {
          dd[(long long)c * N + i] = dl[r][c];
          ii[(long long)c * N + i] = il[r][c];
        }
      }
    }
  }
}

// one lane per query: the S partial lists in ascending chunk order through the same insertion.  A chunk's list is sorted, so its
// first entry that does not enter ends that chunk.  Indices ascend from chunk to chunk, so ties keep the lower index first.
template <int K>
__global__ __launch_bounds__(256) void knn_merge_kernel(const float* __restrict__ pd, const int* __restrict__ pi, int S, long long N,
                                                        int k, float* __restrict__ d2, int* __restrict__ idx) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  float dl[K];
  int il[K];
#pragma unroll
  for (int c = 0; c < K; ++c) {
    dl[c] = pd[(long long)c * N + i];
    il[c] = pi[(long long)c * N + i];
  }
  for (int s = 1; s < S; ++s) {
    const float* sd = pd + (long long)s * K * N + i;
    const int* si = pi + (long long)s * K * N + i;
    for (int c = 0; c < K; ++c) {
      const float d = sd[(long long)c * N];
      if (!(d < dl[K - 1])) break;
      knn_insert<K>(dl, il, d, si[(long long)c * N]);
    }
  }
#pragma unroll
  for (int c = 0; c < K; ++c)
    if (c < k) {
      d2[i * k + c] = dl[c];
      idx[i * k + c] = il[c];
    }
}

template <int K, int R, int SLOTS>
void knn_launch(const float* P, const float* Q, const long long* poff, const long long* qoff, long long* block_off, int B,
                long long N, int k, int S, bool excl, float* d2, int* idx, float* pd, int* pi, hipStream_t st) {
  hipLaunchKernelGGL(sfmi_block_offsets_kernel<KNN_THREADS * R>, dim3(1), dim3(64), 0, st, poff, block_off, B);
  const dim3 grid((unsigned)sfmi_qblocks(B, N, KNN_THREADS * R), (unsigned)S);
  float* dd = S == 1 ? d2 : pd;
  int* ii = S == 1 ? idx : pi;
  if (excl)
    hipLaunchKernelGGL((knn_kernel<K, R, true, SLOTS>), grid, dim3(KNN_THREADS), 0, st, P, Q, poff, qoff, block_off, B, N, k, dd, ii);
  else
    hipLaunchKernelGGL((knn_kernel<K, R, false, SLOTS>), grid, dim3(KNN_THREADS), 0, st, P, Q, poff, qoff, block_off, B, N, k, dd, ii);
  if (S > 1)
    hipLaunchKernelGGL((knn_merge_kernel<K>), dim3(blocks256(N)), dim3(256), 0, st, (const float*)pd, (const int*)pi, S, N, k, d2, idx);
}

// ---- mean neighbour distance -----------------------------------------------------------------------------------------------------

__global__ void knn_mean_dist_kernel(const float* __restrict__ d2, long long N, int k, double* __restrict__ out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  double acc = 0.0;
  for (int c = 0; c < k; ++c) acc += sqrt((double)d2[i * k + c]);
  out[i] = acc / (double)k;
}

// ---- normals by local PCA -------------------------------------------------------------------------------------------------------

// jacobi_rot and SFMI_JACOBI_SWEEPS: sfmi_ragged.h (csrc/segment.hip's plane refit runs the same solver)
__global__ void knn_normals_kernel(const float* __restrict__ P, const long long* __restrict__ off, const int* __restrict__ idx, int B,
                                   long long N, int k, const double* __restrict__ view, float* __restrict__ normal,
                                   float* __restrict__ variation) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int b = sfmi_owner(off, B, i);
  const long long base = off[b], nb = off[b + 1] - base;
  const int* row = idx + i * k;
  double cx = 0.0, cy = 0.0, cz = 0.0;
  int n = 0;
  for (int c = 0; c < k; ++c) {
    const int j = row[c];
    if (j < 0 || j >= nb) continue;                            // -1: no neighbour; anything else outside the set is ignored too
    const long long g = base + j;
    cx += (double)P[3 * g]; cy += (double)P[3 * g + 1]; cz += (double)P[3 * g + 2];
    ++n;
  }
  if (n < 3) {
    normal[3 * i] = normal[3 * i + 1] = normal[3 * i + 2] = 0.f;
    variation[i] = __int_as_float(0x7FC00000);
    return;
  }
  cx /= n; cy /= n; cz /= n;
  double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0;
  for (int c = 0; c < k; ++c) {
    const int j = row[c];
    if (j < 0 || j >= nb) continue;
    const long long g = base + j;
    const double x = (double)P[3 * g] - cx, y = (double)P[3 * g + 1] - cy, z = (double)P[3 * g + 2] - cz;
    a00 += x * x; a01 += x * y; a02 += x * z; a11 += y * y; a12 += y * z; a22 += z * z;
  }
  a00 /= n; a01 /= n; a02 /= n; a11 /= n; a12 /= n; a22 /= n;
  double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;   // v[row][column]
  for (int sweep = 0; sweep < SFMI_JACOBI_SWEEPS; ++sweep) {
    jacobi_rot(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);   // (0, 1), third axis 2
    jacobi_rot(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);   // (0, 2), third axis 1
    jacobi_rot(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);   // (1, 2), third axis 0
  }
  // the column of the smallest eigenvalue (the first on a tie)
  const bool s1 = a11 < a00;
  double lam = s1 ? a11 : a00, nx = s1 ? v01 : v00, ny = s1 ? v11 : v10, nz = s1 ? v21 : v20;
  const bool s2 = a22 < lam;
  lam = s2 ? a22 : lam; nx = s2 ? v02 : nx; ny = s2 ? v12 : ny; nz = s2 ? v22 : nz;
  const double inv = 1.0 / sqrt(nx * nx + ny * ny + nz * nz);
  nx *= inv; ny *= inv; nz *= inv;
  bool flip;
  if (view) {
    const double dot = nx * (view[3 * b] - (double)P[3 * i]) + ny * (view[3 * b + 1] - (double)P[3 * i + 1]) +
                       nz * (view[3 * b + 2] - (double)P[3 * i + 2]);
    flip = dot < 0.0;
  } else {
    double big = nx;
    if (fabs(ny) > fabs(big)) big = ny;
    if (fabs(nz) > fabs(big)) big = nz;
    flip = big < 0.0;
  }
  const double sg = flip ? -1.0 : 1.0;
  normal[3 * i] = (float)(sg * nx);
  normal[3 * i + 1] = (float)(sg * ny);
  normal[3 * i + 2] = (float)(sg * nz);
  variation[i] = (float)(lam / (a00 + a11 + a22));
}

struct KnnWs { int K, S; long long* block_off; float* pd; int* pi; };   // the instance that serves k, its split; pd, pi: S > 1 only

// workspace: block offsets (B+1 int64) | S > 1: partial d2 (S*K*N f32) | partial idx (S*K*N int32), K the instance that serves k
KnnWs knn_ws(SfmiCarver& c, int B, long long N, long long M, int k) {
  const int K = knn_instance(k);
  KnnWs w{K, knn_splits(B, N, M, K), c.take<long long>((size_t)(B + 1)), nullptr, nullptr};
  if (w.S > 1) {
    w.pd = c.take<float>((size_t)w.S * w.K * N);
    w.pi = c.take<int>((size_t)w.S * w.K * N);
  }
  return w;
}

}  // namespace

extern "C" {

size_t sfmi_knn_workspace_bytes(int B, long long N, long long M, int k) {
  if (B <= 0 || N < 0 || M < 0 || k < 1 || k > KNN_MAX_K) return 0;
  return sfmi_ws_bytes(knn_ws, B, N, M, k);
}

int sfmi_knn_f32(const float* P, const float* Q, const long long* poff, const long long* qoff, int B, long long N, long long M, int k,
                 int exclude_self, float* d2, int* idx, void* workspace, void* stream) {
  if (B <= 0 || N < 0 || M < 0 || M >= (1ll << 31) || k < 1 || k > KNN_MAX_K || !poff || !qoff || !workspace) return SFMI_EINVAL;
  if (exclude_self && N != M) return SFMI_EINVAL;
  if (N == 0) return SFMI_OK;
  if (!P || !Q || !d2 || !idx) return SFMI_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  SfmiCarver carver{(char*)workspace};
  const KnnWs w = knn_ws(carver, B, N, M, k);
  const bool ex = exclude_self != 0;
  if (w.K == 8) knn_launch<8, 4, 0>(P, Q, poff, qoff, w.block_off, B, N, k, w.S, ex, d2, idx, w.pd, w.pi, st);
  else if (w.K == 16) knn_launch<16, 2, 0>(P, Q, poff, qoff, w.block_off, B, N, k, w.S, ex, d2, idx, w.pd, w.pi, st);
  else if (w.K == 32) knn_launch<32, 1, 8>(P, Q, poff, qoff, w.block_off, B, N, k, w.S, ex, d2, idx, w.pd, w.pi, st);
  else knn_launch<64, 1, 8>(P, Q, poff, qoff, w.block_off, B, N, k, w.S, ex, d2, idx, w.pd, w.pi, st);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_knn_mean_dist_f64(const float* d2, long long N, int k, double* out, void* stream) {
  if (N < 0 || k < 1 || k > KNN_MAX_K) return SFMI_EINVAL;
  if (N == 0) return SFMI_OK;
  if (!d2 || !out) return SFMI_EINVAL;
  hipLaunchKernelGGL(knn_mean_dist_kernel, dim3(blocks256(N)), dim3(256), 0, (hipStream_t)stream, d2, N, k, out);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_knn_normals_f32(const float* P, const long long* off, const int* idx, int B, long long N, int k, const double* viewpoint,
                         float* normal, float* variation, void* stream) {
  if (B <= 0 || N < 0 || k < 1 || k > KNN_MAX_K || !off) return SFMI_EINVAL;
  if (N == 0) return SFMI_OK;
  if (!P || !idx || !normal || !variation) return SFMI_EINVAL;
  hipLaunchKernelGGL(knn_normals_kernel, dim3(blocks256(N)), dim3(256), 0, (hipStream_t)stream, P, off, idx, B, N, k, viewpoint, normal,
                     variation);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

}  // extern "C"
