// Shared pieces of the mesh and scan tools: what csrc/pointdist.hip, meshsdf.hip, meshtree.hip, hpr.hip, iso_sparse.hip, simplify.hip,
// components.hip, collapse.hip, morph.hip, knn.hip, downsample.hip, poisson.hip, segment.hip, register.hip, features.hip, global_register.hip, posegraph.hip, tangent.hip and emd.hip need
// for ragged batches (the split nearest-neighbour search of the scan tools is sfmi_search.h, which includes this file).  A ragged batch
// is B sets stored back to back with (B+1) nondecreasing offsets, off[0] = 0 and off[B] = the item count: item x belongs to the set b
// with off[b] <= x < off[b+1].  Everything here is inlined into its caller.  The host one-liners at the end hold SfmiCarver, through
// which every tool with a `void* workspace` states that buffer's layout once, for its size function and its launchers.  A caller's
// `#pragma clang fp contract(off)` comes after this include, so it changes nothing in here.  Two functions below have a product feeding a sum: sfmi_pose_row, whose callers all
// compile without contraction, carries `#pragma clang fp contract(off)` in its body; jacobi_rot is compiled under the build's setting.
#pragma once
#include "sfmi_common.h"

// ---- which set owns item x --------------------------------------------------------------------------------------------------------
// Two forms of one function: for nondecreasing offsets with off[0] <= x < off[B] both return the largest b in [0, B) with
// off[b] <= x, so empty sets are skipped.
//   sfmi_owner     binary search: ~log2 B dependent loads.  Used by the kernels over point sets, queries, faces and query blocks of
//                  pointdist / meshsdf / hpr and of the scan tools knn / downsample / poisson / segment / register / features
//                  (64-bit offsets) and over the points of morph (32-bit offsets).
//   sfmi_shape_of  linear count: B - 1 independent loads at wave-uniform addresses, no branch.  Used by the kernels over mesh
//                  vertices, faces, cells and bitmap words of components / simplify / iso_sparse, whose batches are a few shapes.
// They are different code, so which kernel runs which is part of that kernel's recorded timings: switch one only with a measurement.
template <typename O, typename X>
__device__ __forceinline__ int sfmi_owner(const O* __restrict__ off, int B, X x) {
  int lo = 0, hi = B;                       // invariant: off[lo] <= x < off[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= x) lo = mid; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ int sfmi_shape_of(const int* __restrict__ off, int B, int j) {
  int b = 0;
  for (int i = 1; i < B; ++i) b += (j >= off[i]);
  return b;
}

// ---- lock-free union-find over an int32 `parent` array, in the manner of ECL-CC ------------------------------------------------------
// The caller initialises parent[v] <= v (parent[v] = v, or a smaller member of v's set that is known beforehand), runs hooks from any
// number of threads in ONE launch, and reads the forest in a LATER launch (the kernel boundary makes every hook visible).
// Invariant: parent[v] <= v always holds, because a hook links the larger root under the smaller and halving stores an ancestor.  So
// chains strictly descend, every walk ends, and the root of a finished tree is the smallest index of its set whatever order the hooks
// came in: the result is a function of the input, not of the schedule.
//
// parent is read and written by other workgroups during the hook launch: relaxed agent-scope accesses (they pass the CU's L1).  A stale
// value is an older value of the slot, which is the vertex itself or an ancestor of it: it costs steps, never correctness
__device__ __forceinline__ int sfmi_uf_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void sfmi_uf_store(int* p, int x) { __hip_atomic_store(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root above v as this thread sees it, halving the path on the way (a slot that is not a root never becomes one again, and only root
// slots are targets of the CAS, so the plain store of a grandparent into a non-root slot races with nothing that matters)
__device__ __forceinline__ int sfmi_uf_find(int* parent, int v) {
  int cur = v, p = sfmi_uf_load(parent + cur);
  while (p != cur) {
    const int g = sfmi_uf_load(parent + p);
    if (g != p) sfmi_uf_store(parent + cur, g);
    cur = p;
    p = g;
  }
  return cur;
}

__device__ __forceinline__ void sfmi_uf_hook(int* parent, int u, int v) {
  int ru = sfmi_uf_find(parent, u), rv = sfmi_uf_find(parent, v);
  while (ru != rv) {
    const int hi = max(ru, rv), lo = min(ru, rv);
    const int old = atomicCAS(parent + hi, hi, lo);
    if (old == hi) return;
    // hi had stopped being a root: `old` is its parent as memory holds it, so the walk goes on from there even if this CU's view of
    // the slot is stale
    ru = sfmi_uf_find(parent, old);
    rv = sfmi_uf_find(parent, lo);
  }
}

// ---- f64 butterflies over the 64 lanes of a wave: a fixed tree, the result in every lane --------------------------------------------
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_min_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

// the sum over a workgroup of WAVES waves (a power of two; 16 in orient_kernel, rf_kernel and greg_refit_kernel) in every lane:
// wave_sum_f64, then the WAVES wave sums through the same xor tree.  red: WAVES doubles of LDS; every lane of the workgroup calls.
// NOT the order of poisson.hip's cg_block_sum ((r0 + r1) + (r2 + r3)) nor of sfmi_chunk_partial below (the waves in order): each of
// the three is a different f64 rounding fixed by its numpy restatement, so the three stay three.
template <int WAVES>
__device__ __forceinline__ double sfmi_block_sum_f64(double v, double* red) {
  v = wave_sum_f64(v);
  __syncthreads();                                             // the previous use of red is over
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = red[threadIdx.x & (WAVES - 1)];
#pragma unroll
  for (int o = WAVES / 2; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
  return t;
}

// splitmix64 finalizer: the counter hash of the mesh samplers
__device__ __forceinline__ unsigned long long sfmi_mix64(unsigned long long x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// ---- symmetric 3x3 eigen-solver in f64: the cyclic Jacobi step of knn.hip's normals and segment.hip's plane refit -------------------
// (products feeding sums, compiled under the build's contraction setting in every includer, because each includer's
// `#pragma clang fp contract(off)` comes after this include)
// one Jacobi rotation of the symmetric 3x3 matrix in the plane (p, q), r the third axis: zeroes a_pq.  v*p / v*q: columns p and q of
// the accumulated eigenvector matrix.  Branch-free: a_pq == 0 is the identity rotation.
__device__ __forceinline__ void jacobi_rot(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p, double& v0q,
                                           double& v1p, double& v1q, double& v2p, double& v2q) {
  const double theta = (aqq - app) / (2.0 * apq);
  double t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));      // |theta| huge: t -> 0
  t = apq == 0.0 ? 0.0 : t;
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  app -= t * apq;
  aqq += t * apq;
  apq = 0.0;
  const double rp = c * arp - s * arq, rq = s * arp + c * arq;
  arp = rp; arq = rq;
  const double a0 = c * v0p - s * v0q, b0 = s * v0p + c * v0q;
  const double a1 = c * v1p - s * v1q, b1 = s * v1p + c * v1q;
  const double a2 = c * v2p - s * v2q, b2 = s * v2p + c * v2q;
  v0p = a0; v0q = b0; v1p = a1; v1q = b1; v2p = a2; v2q = b2;
}

// sweeps of jacobi_rot (knn.hip, segment.hip) and of global_register.hip's one-sided gr_rot: no data-dependent trip count
constexpr int SFMI_JACOBI_SWEEPS = 8;            // a 3x3 in f64 is converged to the last bit after 5 or 6

// ---- points and poses of the scan tools ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double sfmi_nan_f64() { return __longlong_as_double(0x7FF8000000000000ll); }

template <typename T>
__device__ __forceinline__ bool sfmi_finite3(T x, T y, T z) { return isfinite(x) && isfinite(y) && isfinite(z); }
__device__ __forceinline__ bool sfmi_finite3(const float* __restrict__ p) { return sfmi_finite3(p[0], p[1], p[2]); }

// the centroid of a set's finite points by one workgroup of WAVES waves, in f64 in a fixed order: a lane's points ascending (lane t takes
// points t, t + 64 WAVES, ...), then sfmi_block_sum_f64.  WAVES is part of the order: features.hip's orient_kernel and tangent.hip's
// tg_centroid_kernel both run it with 16 waves and so get the same bits.  Pb: the set's first point, n its size; red: WAVES doubles of
// LDS; every lane of the workgroup calls.  false (workgroup-uniform, c untouched) for a set without a finite point.  Sums and one
// division: nothing here contracts.
template <int WAVES>
__device__ __forceinline__ bool sfmi_centroid_f64(const float* __restrict__ Pb, long long n, double* red, double& cx, double& cy,
                                                  double& cz) {
  double sx = 0.0, sy = 0.0, sz = 0.0, sc = 0.0;
  for (long long i = threadIdx.x; i < n; i += WAVES * 64) {
    const double x = (double)Pb[3 * i], y = (double)Pb[3 * i + 1], z = (double)Pb[3 * i + 2];
    if (sfmi_finite3(x, y, z)) {
      sx += x; sy += y; sz += z; sc += 1.0;
    }
  }
  sx = sfmi_block_sum_f64<WAVES>(sx, red); sy = sfmi_block_sum_f64<WAVES>(sy, red); sz = sfmi_block_sum_f64<WAVES>(sz, red);
  sc = sfmi_block_sum_f64<WAVES>(sc, red);                     // whole numbers below 2^31: exact in f64
  if (!(sc > 0.0)) return false;
  cx = sx / sc; cy = sy / sc; cz = sz / sc;
  return true;
}

// x' = f32(((r0 x + r1 y) + r2 z) + t) in f64, the f32 point widened first; T: one row of the pose (4 doubles).  Every product and sum
// is rounded on its own, whatever the build's setting: the numpy restatements (tests/icp_ref.py, global_reg_ref.py) fix these bits.
__device__ __forceinline__ float sfmi_pose_row(const double* __restrict__ T, double x, double y, double z) {
#pragma clang fp contract(off)
  return (float)(((T[0] * x + T[1] * y) + T[2] * z) + T[3]);
}

__device__ __forceinline__ bool sfmi_pose_finite(const double* __restrict__ T) {
  bool ok = true;
  for (int e = 0; e < 12; ++e) ok = ok && isfinite(T[e]);
  return ok;
}

// is correspondence (j, d) of a pair whose target set has m points an inlier?  The index is tested here, before the caller reads the
// point it names.
__device__ __forceinline__ bool sfmi_inlier(int j, long long m, float d, float maxd2) { return j >= 0 && j < m && d <= maxd2; }

// ---- the chunked f64 sums of register.hip (29 entries per pair) and posegraph.hip (10): DESIGN.md §5.18's order -------------------------
// A workgroup of 4 waves takes a chunk of 1024 source points, 4 per lane, counted from the pair's first point, so a pair's sums do not
// depend on the batch around it.  sfmi_icp_chunk() and sfmi_pg_chunk() report this size: the host sizes `part` by it.
constexpr int SFMI_CHUNK_THREADS = 256;
constexpr int SFMI_CHUNK_R = 4;                  // points per lane, taken in ascending order
constexpr int SFMI_CHUNK = SFMI_CHUNK_THREADS * SFMI_CHUNK_R;
constexpr int SFMI_METRIC_PLANE = 1;             // include/sfmi.h's metric code of point-to-plane ICP

// the end of a chunk: wave_sum_f64 per entry, lane 0 of each wave into red, the WAVES waves added in order by lanes < NS, which store
// the chunk's partial out[e].  Sums only: nothing here contracts.  Every lane of the workgroup calls (one barrier).
template <int NS, int WAVES>
__device__ __forceinline__ void sfmi_chunk_partial(const double (&acc)[NS], double (&red)[WAVES][NS], double* __restrict__ out) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int e = 0; e < NS; ++e) {
    const double v = wave_sum_f64(acc[e]);
    if ((tid & 63) == 0) red[tid >> 6][e] = v;
  }
  __syncthreads();
  if (tid < NS) {
    double s = red[0][tid];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) s += red[w][tid];          // the waves in order
    out[tid] = s;
  }
}

// entry threadIdx.x (< NS) of pair b: its chunk partials added in ascending chunk order.  nc: the pair's own chunks (<= chunks, the
// row length of part)
template <int NS>
__device__ __forceinline__ double sfmi_chunk_total(const double* __restrict__ part, int b, int chunks, int nc) {
  double v = 0.0;
  for (int c = 0; c < nc && c < chunks; ++c) v += part[((long long)b * chunks + c) * NS + threadIdx.x];
  return v;
}

// grid (chunks of 256 x 4 items, pairs): bad[b] |= 1 when a source or target coordinate of the pair is not finite; with NORMALS also
// a target normal of a pair whose metric[b] is the plane metric (without, nrm and metric are not read)
template <bool NORMALS>
static __global__ __launch_bounds__(SFMI_CHUNK_THREADS) void sfmi_pairs_finite_kernel(
    const float* __restrict__ src, const float* __restrict__ tgt, const float* __restrict__ nrm, const long long* __restrict__ soff,
    const long long* __restrict__ toff, const int* __restrict__ metric, int* __restrict__ bad) {
  const int b = blockIdx.y;
  const bool plane = NORMALS && metric[b] == SFMI_METRIC_PLANE;
  const long long s0 = soff[b], n = soff[b + 1] - s0, t0 = toff[b], m = toff[b + 1] - t0;
  bool x = false;
  for (int r = 0; r < SFMI_CHUNK_R; ++r) {
    const long long i = ((long long)blockIdx.x * SFMI_CHUNK_R + r) * SFMI_CHUNK_THREADS + threadIdx.x;
    if (i < n) x |= !sfmi_finite3(src + 3 * (s0 + i));
    if (i < m) {
      x |= !sfmi_finite3(tgt + 3 * (t0 + i));
      if (plane) x |= !sfmi_finite3(nrm + 3 * (t0 + i));
    }
  }
  if (__any(x) && (threadIdx.x & 63) == 0) atomicOr(bad + b, 1);
}

// bad[0 .. B) <- 0, then the kernel above over the largest set of the batch.  SFMI_ELAUNCH: the memset was refused
template <bool NORMALS>
inline int sfmi_pairs_finite(const float* src, const float* tgt, const float* nrm, const long long* soff, const long long* toff,
                             const int* metric, int B, long long max_n, long long max_m, int* bad, hipStream_t st) {
  SFMI_TRY(hipMemsetAsync(bad, 0, (size_t)B * sizeof(int), st));
  const long long most = max_n > max_m ? max_n : max_m;
  if (most > 0)
    hipLaunchKernelGGL(sfmi_pairs_finite_kernel<NORMALS>, dim3((unsigned)((most + SFMI_CHUNK - 1) / SFMI_CHUNK), (unsigned)B),
                       dim3(SFMI_CHUNK_THREADS), 0, st, src, tgt, nrm, soff, toff, metric, bad);
  return SFMI_OK;
}

// ---- RANSAC over hypotheses (segment.hip's planes, global_register.hip's poses): integer counts, so the result is a function of the input
constexpr int SFMI_HT = 64;                      // hypotheses per tile: lane h of a wave keeps the count of hypothesis h
constexpr int SFMI_BEST_THREADS = 256;

// the end of a score kernel's pass over a tile of SFMI_HT hypotheses: `mine` is the count of the wave's points for hypothesis `lane`;
// the WAVES wave counts are added and one atomicAdd per hypothesis with a positive total reaches tile_count[h] (a positive total
// belongs to a valid hypothesis, so that slot exists).  Every lane of the workgroup calls; wc is free again on return.
template <int WAVES>
__device__ __forceinline__ void sfmi_commit_counts(int (&wc)[WAVES][SFMI_HT], int mine, int* __restrict__ tile_count) {
  const int tid = threadIdx.x;
  wc[tid >> 6][tid & 63] = mine;
  __syncthreads();
  if (tid < SFMI_HT) {
    int tot = 0;
#pragma unroll
    for (int v = 0; v < WAVES; ++v) tot += wc[v][tid];
    if (tot > 0) atomicAdd(tile_count + tid, tot);
  }
  __syncthreads();                                             // wc is consumed before the next pass writes it
}

// (c, h) <- the better of the two under (larger count, then lower h)
__device__ __forceinline__ void sfmi_take(int& c, int& h, int oc, int oh) {
  const bool take = oc > c || (oc == c && oh < h);
  c = take ? oc : c;
  h = take ? oh : h;
}

// the arg max of row[0 .. H) under sfmi_take, by a workgroup of SFMI_BEST_THREADS: per lane, the wave's butterfly, the four waves in
// order.  (bc, bh) is the result in thread 0 only; bc = -1 when no count is >= 0.  Every lane of the workgroup calls.
__device__ __forceinline__ void sfmi_best_of_row(const int* row, int H, int& bc, int& bh) {
  __shared__ int sc[SFMI_BEST_THREADS / 64], sh[SFMI_BEST_THREADS / 64];
  const int tid = threadIdx.x;
  bc = -1;
  bh = 0x7FFFFFFF;
  for (int h = tid; h < H; h += SFMI_BEST_THREADS) sfmi_take(bc, bh, row[h], h);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sfmi_take(bc, bh, __shfl_xor(bc, o, 64), __shfl_xor(bh, o, 64));
  if ((tid & 63) == 0) {
    sc[tid >> 6] = bc;
    sh[tid >> 6] = bh;
  }
  __syncthreads();
  if (tid == 0)
    for (int v = 1; v < SFMI_BEST_THREADS / 64; ++v) sfmi_take(bc, bh, sc[v], sh[v]);
}

// ---- per-shape mesh validation: flag bits that kernels OR into flags[b], and the status code they stand for ------------------------
constexpr int SFMI_MESH_NO_VERTS = 1, SFMI_MESH_BAD_INDEX = 2, SFMI_MESH_NON_FINITE = 4;   // the status is the lowest one set
__device__ __forceinline__ int sfmi_mesh_status(int flags) {
  return (flags & SFMI_MESH_NO_VERTS) ? 1 : ((flags & SFMI_MESH_BAD_INDEX) ? 2 : ((flags & SFMI_MESH_NON_FINITE) ? 3 : 0));
}

// ---- host one-liners ----------------------------------------------------------------------------------------------------------------
__host__ __device__ inline long long cdiv(long long a, long long b) { return (a + b - 1) / b; }
inline size_t align256(size_t x) { return (x + 255) / 256 * 256; }                    // workspace sections start on 256 bytes

// a `void* workspace` cut into sections, in the order they are taken.  A tool names its sections in ONE layout function that takes a
// carver: over a null carver it only counts (sfmi_*_workspace_bytes returns bytes()), over the caller's buffer it hands the launcher the
// same sections' pointers, so the size and the offsets cannot drift apart.  Host only.
struct SfmiCarver {
  char* base;                                                  // nullptr: count only, every take() is nullptr
  size_t off = 0;
  template <typename T>
  T* take(size_t count) {
    T* p = base ? (T*)(base + off) : nullptr;
    off += align256(count * sizeof(T));
    return p;
  }
  size_t bytes() const { return off; }
};
// what a layout function takes in all: it is run over a null carver.  args: the layout's arguments after the carver
template <typename F, typename... A>
inline size_t sfmi_ws_bytes(F layout, A... args) {
  SfmiCarver c{nullptr};
  layout(c, args...);
  return c.bytes();
}
inline unsigned blocks256(long long n) { return (unsigned)((n + 255) / 256); }         // workgroups of 256 threads over n items
constexpr unsigned SFMI_MAX_GRID = 65535;                                              // the y and z limits of a grid
inline unsigned sfmi_grid_cap(long long n) { return (unsigned)(n < 1 ? 1 : (n > SFMI_MAX_GRID ? SFMI_MAX_GRID : n)); }   // for grid-stride loops
