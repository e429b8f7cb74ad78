// Shared pieces of the mesh tools: what csrc/pointdist.hip, meshsdf.hip, hpr.hip, iso_sparse.hip, simplify.hip,
// components.hip and morph.hip all need for ragged batches.  A ragged batch is B sets stored back to back with (B+1) nondecreasing
// offsets, off[0] = 0 and off[B] = the item count: item x belongs to the set b with off[b] <= x < off[b+1].  Everything here is
// inlined into its caller; apart from jacobi_rot below none of it holds a multiply-add, and a caller's `#pragma clang fp contract(off)`
// comes after this include, so it changes nothing in here.
#pragma once
#include "sfmi_common.h"

// ---- which set owns item x --------------------------------------------------------------------------------------------------------
// Two forms of one function: for nondecreasing offsets with off[0] <= x < off[B] both return the largest b in [0, B) with
// off[b] <= x, so empty sets are skipped.
//   sfmi_owner     binary search: ~log2 B dependent loads.  Used by the kernels over point sets, queries, faces and query blocks of
//                  pointdist / meshsdf / hpr (64-bit offsets) and over the points of morph (32-bit offsets).
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

// splitmix64 finalizer: the counter hash of the mesh samplers
__device__ __forceinline__ unsigned long long sfmi_mix64(unsigned long long x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// ---- symmetric 3x3 eigen-solver in f64: the cyclic Jacobi step of knn.hip's normals and segment.hip's plane refit -------------------
// (the one piece of this header with products feeding sums: it is compiled under the build's contraction setting in every includer,
// because each includer's `#pragma clang fp contract(off)` comes after this include)
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

constexpr int KNN_JACOBI_SWEEPS = 8;             // a 3x3 in f64 is converged to the last bit after 5 or 6

// ---- per-shape mesh validation: flag bits that kernels OR into flags[b], and the status code they stand for ------------------------
constexpr int SFMI_MESH_NO_VERTS = 1, SFMI_MESH_BAD_INDEX = 2, SFMI_MESH_NON_FINITE = 4;   // the status is the lowest one set
__device__ __forceinline__ int sfmi_mesh_status(int flags) {
  return (flags & SFMI_MESH_NO_VERTS) ? 1 : ((flags & SFMI_MESH_BAD_INDEX) ? 2 : ((flags & SFMI_MESH_NON_FINITE) ? 3 : 0));
}

// ---- host one-liners ----------------------------------------------------------------------------------------------------------------
__host__ __device__ inline long long cdiv(long long a, long long b) { return (a + b - 1) / b; }
inline size_t align256(size_t x) { return (x + 255) / 256 * 256; }                    // workspace sections start on 256 bytes
inline unsigned blocks256(long long n) { return (unsigned)((n + 255) / 256); }         // workgroups of 256 threads over n items
