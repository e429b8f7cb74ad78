// Mesh queries through a bounding-volume tree: the hierarchical route next to csrc/meshsdf.hip's brute force.
// Exact closest-point queries (|S|, I, C bit-identical to sfmi_mesh_sdf_f32) and approximate generalized winding numbers by a tree
// code: the third-order far-field expansion of Barill et al. 2018, "Fast winding numbers for soups and clouds".  For 256^3 lattices and
// meshes of 10^5 faces, where O(G^3 T) brute force takes seconds per mesh.
//
// 1. Order.  Faces are sorted by (shape, 30-bit Morton key of the face centroid in the shape's vertex bounding box, face index); the
//    keys come from mt_keys_kernel, the stable sort is the host's (torch.sort, as simplify does).
// 2. Topology, implicit: leaves are runs of MT_LEAF = 64 consecutive faces in that order (the last may be short); level l + 1 groups
//    8 consecutive nodes of level l, until a level has one node, the root.  Node j of level l covers the leaves
//    [j 8^l, min((j + 1) 8^l, L0)).  A shape's nodes are stored level by level, leaves first; no pointers exist.
// 3. Per node (9 x float4):  n0 = (aabb min, r)   n1 = (aabb max, noprune)   n2 = (p~, tr Q)   n3 = (dipole, 0)   n4 .. n8 = the second
//    and third moments as the expansion reads them (mt_finish_kernel, mt_expansion)
//    aabb     of the three vertices of every face below the node; min / max are exact.
//    p~       the area-weighted centroid  sum a_t c_t / sum a_t  (the middle of the aabb when the area is zero), rounded to f32
//    dipole   D = sum a_t n_t = sum (b - a) x (c - a) / 2 over the non-degenerate faces, rounded to f32
//    moments  Q = sum (c_t - p~) (x) a_t n_t and M = sum S_t (x) a_t n_t about the stored p~, S_t the face's second moment per unit area
//             (c_t - p~)(c_t - p~)^T + sum_k (v_k - c_t)(v_k - c_t)^T / 12; stored as tr Q, the symmetric part of Q (6), the vector
//             g_j = -6 sum_i M_iji - 3 sum_i M_iij and the 10 coefficients K of the cubic form sum M_ijk r_i r_j r_k.  Dipole alone errs
//             by 1.6e-2 at beta = 2 and the second order makes it worse; with the third the error is 2.4e-3
//    r        max |v - p~| over the vertices below the node, about the stored f32 p~, in f64, rounded UP to f32
//    noprune  1 when a face below the node is a sliver (width <= 2^-8 of its longest edge): see the bound below
//    The sums are f64 in a fixed order (a leaf's faces in order by one thread, a node's children in order by one thread) and kept
//    in `mom` (36 doubles per node: area, a c (3), dipole (3), R2 = sum c (x) a n (9), R3 = sum S (x) a n about the ORIGIN (18), the
//    sliver flag, a pad); mt_finish_kernel shifts R2 and R3 to the stored p~ in f64.  One launch per level, kernel boundaries are the
//    only synchronisation, no float atomics.  A shape's tree depends on that shape alone.
// 4. Queries: packet traversal.  One wave (one workgroup of 64 lanes) owns 64 spatially close queries: a 4 x 4 x 4 block of lattice
//    points, or 64 consecutive queries of a set the host sorted by Morton code.  The walk's state (level, index, level base) is
//    wave-uniform and there is no stack: after a node the walk goes to its next sibling, or climbs while it stands on a last child.
//    It visits nodes in depth-first order, every node at most once, so it ends after at most `nodes` steps.
//    Winding: a lane that is not muted tests |q - p~|^2 > (beta r)^2 in f32 (direct form).  True: it adds the node's expansion
//      (mt_expansion: a half solid angle, as half_solid_angle) and mutes itself until the walk leaves the node's
//      subtree, whatever its wave-mates do.  False at a leaf: it adds the exact half solid angles of the leaf's faces (an f32 run in
//      face order, as meshsdf's runs of 64).  False at an internal node: it needs the children.  Every contribution is added as a
//      2^-29 fixed-point integer (w_flush), so a lane's sum is a function of (query, mesh, beta) alone.
//    Distance: a lane needs a node unless bound(q, node) > its current best d2 (equality never prunes).  Every lane evaluates every
//      face of a leaf the wave enters: a face of a node the lane could have pruned has d2 >= bound > best and changes nothing.  The
//      compare is lexicographic on (d2, original face index), so the lowest original index wins an f32 tie, as in the brute route.
//      `best` is seeded from the leaf a greedy descent finds nearest to the wave's first query.
//    A node is entered when __any lane needs it; a leaf's face records go through LDS and are read as broadcasts.
//
// The pruning bound.  closest_vw returns d2 = fl(|q - C|^2) with C = fl(a + v ab + w ac) computed in f32, so a bound must allow for
// (i) rounding: ab, ac, the two fmaf of C, q - C and the sum of squares each err by at most a few u = 2^-24 relative to the coordinate
// magnitude M = max(|q|_inf, |box|_inf), together < 32 u M per axis; and (ii) region misclassification: the regions are chosen by the
// signs of va, vb, vc, whose error moves a region's border in the plane by at most delta ~ 16 u |q - a| L / h (L the longest edge, h
// the width).  A wrong edge or vertex region still yields a point ON the face (d2 can only grow); the interior region chosen for a
// query whose projection lies up to delta outside yields a point of the PLANE, so d2 >= d_true^2 - delta^2.  With L / h < 2^8 (a
// sliver beyond that sets `noprune` on its leaf and all its ancestors: their bound is 0) and |q - a| <= 2 sqrt(3) M, delta < 2^-10 M.
// The bound is therefore  sum over axes of max(g - eps, 0)^2 * (1 - 2^-20),  g = max(lo - q, q - hi, 0) in f32, eps = 2^-9 M:
// on an axis with g >= eps, (g - eps)^2 <= g^2 - eps^2, so the sum is <= G^2 - eps^2 <= d_true^2 - delta^2 - rounding <= d2, and the
// factor covers the f32 rounding of the sum itself.  At unit scale eps is 2e-3, a quarter of a 256^3 lattice step.
#include "sfmi_ragged.h"
#include "sfmi_triangle.h"
#pragma clang fp contract(off)

namespace {

constexpr int MT_LEAF = 64;                      // faces per leaf = lanes per wave = meshsdf's run of the winding sum
constexpr int MT_NODE = 9;                       // float4 per node
constexpr int MT_MOM = 36;                       // doubles per node: area, a c (3), dipole (3), R2 (9), R3 (18), sliver flag, pad
constexpr int MT_FLAG = 34;                      // where the sliver flag sits; the sums are the 34 entries before it
constexpr double MT_SLIVER = 0x1.0p-16;          // (h / L)^2 at and below which a face forbids pruning above it
constexpr float MT_EPS = 0x1.0p-9f;              // the bound's deflation per axis, relative to the coordinate magnitude
constexpr float MT_SHRINK = 1.f - 0x1.0p-20f;

__host__ __device__ inline long long mt_level_nodes(long long L0, int l) { return (L0 + ((1ll << (3 * l)) - 1)) >> (3 * l); }
__host__ __device__ inline int mt_top(long long L0) {
  int l = 0;
  while (mt_level_nodes(L0, l) > 1) ++l;
  return l;
}

// ---- keys ---------------------------------------------------------------------------------------------------------------------------

constexpr int MT_BB_THREADS = 256;
// one workgroup per shape: bbox[6 b ..] = min xyz, max xyz of its vertices (0 without vertices); flags[b] = NON_FINITE or 0
__global__ __launch_bounds__(MT_BB_THREADS) void mt_bbox_kernel(const float* __restrict__ verts, const long long* __restrict__ voff, int B,
                                                                float* __restrict__ bbox, int* __restrict__ flags) {
  __shared__ float red[6][MT_BB_THREADS / 64];
  __shared__ int bad_s;
  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    const long long v0 = voff[b], v1 = voff[b + 1];
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    int bad = 0;
    for (long long v = v0 + threadIdx.x; v < v1; v += MT_BB_THREADS) {
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const float x = verts[3 * v + a];
        bad |= !isfinite(x);
        lo[a] = fminf(lo[a], x);
        hi[a] = fmaxf(hi[a], x);
      }
    }
    bad = __syncthreads_or(bad);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        lo[a] = fminf(lo[a], __shfl_xor(lo[a], o, 64));
        hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], o, 64));
      }
      if ((threadIdx.x & 63) == 0) {
        red[a][threadIdx.x >> 6] = lo[a];
        red[3 + a][threadIdx.x >> 6] = hi[a];
      }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
      float m = red[threadIdx.x][0];
      for (int w = 1; w < MT_BB_THREADS / 64; ++w) m = threadIdx.x < 3 ? fminf(m, red[threadIdx.x][w]) : fmaxf(m, red[threadIdx.x][w]);
      bbox[6 * b + threadIdx.x] = v1 > v0 ? m : 0.f;
    }
    if (threadIdx.x == 0) flags[b] = bad ? SFMI_MESH_NON_FINITE : 0;
    __syncthreads();
  }
}

// the three vertices of global face g of shape b (v0: its first vertex, nv: its vertex count); false (p zeroed) for an index outside
__device__ __forceinline__ bool mt_face_verts(const float* __restrict__ verts, const int* __restrict__ faces, long long v0, long long nv,
                                              long long g, float (&p)[3][3]) {
  bool ok = true;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int k = faces[3 * g + c];
    const bool in = k >= 0 && k < nv;
    ok = ok && in;
    const long long v = v0 + (in ? k : 0);
#pragma unroll
    for (int a = 0; a < 3; ++a) p[c][a] = in ? verts[3 * v + a] : 0.f;
  }
  if (!ok) {
#pragma unroll
    for (int c = 0; c < 3; ++c) p[c][0] = p[c][1] = p[c][2] = 0.f;
  }
  return ok;
}

__device__ __forceinline__ unsigned mt_spread(unsigned x) {      // 10 bits -> every third bit
  x = (x | (x << 16)) & 0x030000FFu;
  x = (x | (x << 8)) & 0x0300F00Fu;
  x = (x | (x << 4)) & 0x030C30C3u;
  x = (x | (x << 2)) & 0x09249249u;
  return x;
}

// one thread per face: key = shape << 30 | Morton(ux, uy, uz), x in the highest bit of each triple; u = clamp(floor(t 1024), 0, 1023),
// t = ((a + b) + c) / 3 - lo) / (hi - lo) in f32, each operation rounded on its own; a flat axis, and anything not finite, gives 0
__global__ void mt_keys_kernel(const float* __restrict__ verts, const int* __restrict__ faces, const long long* __restrict__ voff,
                               const long long* __restrict__ toff, const float* __restrict__ bbox, int B, long long T,
                               long long* __restrict__ keys, int* __restrict__ flags) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= T) return;
  const int b = sfmi_owner(toff, B, t);
  float p[3][3];
  if (!mt_face_verts(verts, faces, voff[b], voff[b + 1] - voff[b], t, p)) atomicOr(flags + b, SFMI_MESH_BAD_INDEX);
  unsigned u[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float lo = bbox[6 * b + a], hi = bbox[6 * b + 3 + a];
    const float c = __fdiv_rn(__fadd_rn(__fadd_rn(p[0][a], p[1][a]), p[2][a]), 3.f);
    const float w = __fsub_rn(hi, lo);
    float x = w > 0.f ? __fdiv_rn(__fsub_rn(c, lo), w) : 0.f;
    x = floorf(__fmul_rn(x, 1024.f));
    x = x >= 0.f ? x : 0.f;                                    // NaN -> 0
    u[a] = (unsigned)(x < 1023.f ? x : 1023.f);
  }
  keys[t] = ((long long)b << 30) | (long long)((mt_spread(u[0]) << 2) | (mt_spread(u[1]) << 1) | mt_spread(u[2]));
}

// ---- build --------------------------------------------------------------------------------------------------------------------------

// one thread per sorted slot s: the record of face order[s] and its index local to the shape
__global__ void mt_records_kernel(const float* __restrict__ verts, const int* __restrict__ faces, const long long* __restrict__ voff,
                                  const long long* __restrict__ toff, const long long* __restrict__ order, int B, long long T,
                                  float4* __restrict__ rec, int* __restrict__ orig) {
  const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= T) return;
  const int b = sfmi_owner(toff, B, s);
  long long g = order[s];
  g = g >= toff[b] && g < toff[b + 1] ? g : s;                 // the order is a permutation within each shape; never read outside
  float p[3][3];
  const bool ok = mt_face_verts(verts, faces, voff[b], voff[b + 1] - voff[b], g, p);
  float4* r = rec + SFMI_FACE_REC * s;
  orig[s] = (int)(g - toff[b]);
  if (!ok) {
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    r[0] = z; r[1] = z; r[2] = z; r[3] = z;
    r[4] = make_float4(0.f, 0.f, 0.f, 1.f);
    return;
  }
  sfmi_pack_face(p, r);
}

__global__ void mt_status_kernel(const long long* __restrict__ toff, const int* __restrict__ flags, int B, int* __restrict__ status) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) status[b] = toff[b + 1] <= toff[b] ? 1 : sfmi_mesh_status(flags[b] & ~SFMI_MESH_NO_VERTS);
}

// grid (leaf blocks, shapes): one thread per leaf.  Its faces in order: aabb, f64 sums, sliver flag
__global__ __launch_bounds__(MT_LEAF) void mt_leaf_kernel(const float* __restrict__ verts, const int* __restrict__ faces, const long long* __restrict__ voff,
                               const long long* __restrict__ toff, const long long* __restrict__ noff, const long long* __restrict__ order,
                               const float4* __restrict__ rec, int B, float4* __restrict__ nodes, double* __restrict__ mom) {
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const long long t0 = toff[b], Tb = toff[b + 1] - t0, L0 = (Tb + MT_LEAF - 1) / MT_LEAF;
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= L0) continue;
    const long long v0 = voff[b], nv = voff[b + 1] - v0;
    const long long s0 = t0 + j * MT_LEAF, s1 = s0 + MT_LEAF < t0 + Tb ? s0 + MT_LEAF : t0 + Tb;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    double area = 0.0, ac[3] = {0.0, 0.0, 0.0}, dip[3] = {0.0, 0.0, 0.0}, r2[9] = {}, r3[18] = {};
    bool sliver = false;
    for (long long s = s0; s < s1; ++s) {
      long long g = order[s];
      g = g >= t0 && g < t0 + Tb ? g : s;
      float p[3][3];
      mt_face_verts(verts, faces, v0, nv, g, p);
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          lo[a] = fminf(lo[a], p[c][a]);
          hi[a] = fmaxf(hi[a], p[c][a]);
        }
      if (rec[SFMI_FACE_REC * s + 3].w == 0.f) continue;       // degenerate or bad: no area
      double e1[3], e2[3], e3[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        e1[a] = (double)p[1][a] - (double)p[0][a];
        e2[a] = (double)p[2][a] - (double)p[0][a];
        e3[a] = (double)p[2][a] - (double)p[1][a];
      }
      const double nx = e1[1] * e2[2] - e1[2] * e2[1], ny = e1[2] * e2[0] - e1[0] * e2[2], nz = e1[0] * e2[1] - e1[1] * e2[0];
      const double cr2 = (nx * nx + ny * ny) + nz * nz;
      const double l1 = (e1[0] * e1[0] + e1[1] * e1[1]) + e1[2] * e1[2], l2 = (e2[0] * e2[0] + e2[1] * e2[1]) + e2[2] * e2[2],
                   l3 = (e3[0] * e3[0] + e3[1] * e3[1]) + e3[2] * e3[2];
      const double lm = fmax(l1, fmax(l2, l3));
      sliver = sliver || cr2 <= MT_SLIVER * lm * lm;
      const double at = 0.5 * sqrt(cr2);
      area += at;
      dip[0] += 0.5 * nx; dip[1] += 0.5 * ny; dip[2] += 0.5 * nz;
      const double an[3] = {0.5 * nx, 0.5 * ny, 0.5 * nz};
      double c[3], d[3][3];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        c[a] = (((double)p[0][a] + (double)p[1][a]) + (double)p[2][a]) / 3.0;
        ac[a] += at * c[a];
#pragma unroll
        for (int k = 0; k < 3; ++k) d[k][a] = (double)p[k][a] - c[a];
      }
      // second moment of the face about the origin, per unit area: c c^T + sum_k (v_k - c)(v_k - c)^T / 12; order xx yy zz xy xz yz
      constexpr int SI[6] = {0, 1, 2, 0, 0, 1}, SJ[6] = {0, 1, 2, 1, 2, 2};
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) r2[3 * i + k] += c[i] * an[k];
#pragma unroll
      for (int q = 0; q < 6; ++q) {
        const int i = SI[q], j = SJ[q];
        const double s0 = c[i] * c[j] + ((d[0][i] * d[0][j] + d[1][i] * d[1][j]) + d[2][i] * d[2][j]) / 12.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) r3[3 * q + k] += s0 * an[k];
      }
    }
    float4* n = nodes + MT_NODE * (noff[b] + j);
    n[0] = make_float4(lo[0], lo[1], lo[2], 0.f);
    n[1] = make_float4(hi[0], hi[1], hi[2], sliver ? 1.f : 0.f);
    double* m = mom + MT_MOM * (noff[b] + j);
    m[0] = area; m[1] = ac[0]; m[2] = ac[1]; m[3] = ac[2]; m[4] = dip[0]; m[5] = dip[1]; m[6] = dip[2];
#pragma unroll
    for (int e = 0; e < 9; ++e) m[7 + e] = r2[e];
#pragma unroll
    for (int e = 0; e < 18; ++e) m[16 + e] = r3[e];
    m[MT_FLAG] = sliver ? 1.0 : 0.0;
    m[MT_FLAG + 1] = 0.0;
  }
}

// grid (node blocks, shapes): one thread per node of level l >= 1 of every shape that has that level: its children in order
__global__ __launch_bounds__(MT_LEAF) void mt_up_kernel(const long long* __restrict__ toff, const long long* __restrict__ noff, int B, int l, float4* __restrict__ nodes,
                             double* __restrict__ mom) {
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const long long Tb = toff[b + 1] - toff[b], L0 = (Tb + MT_LEAF - 1) / MT_LEAF;
    if (L0 < 1 || l > mt_top(L0)) continue;
    const long long nl = mt_level_nodes(L0, l), nc = mt_level_nodes(L0, l - 1);
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nl) continue;
    long long cbase = noff[b];
    for (int k = 0; k < l - 1; ++k) cbase += mt_level_nodes(L0, k);
    const long long base = cbase + nc;
    const long long c0 = 8 * j, c1 = c0 + 8 < nc ? c0 + 8 : nc;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    double s[MT_MOM] = {};
    for (long long c = c0; c < c1; ++c) {
      const float4 a = nodes[MT_NODE * (cbase + c)], h = nodes[MT_NODE * (cbase + c) + 1];
      lo[0] = fminf(lo[0], a.x); lo[1] = fminf(lo[1], a.y); lo[2] = fminf(lo[2], a.z);
      hi[0] = fmaxf(hi[0], h.x); hi[1] = fmaxf(hi[1], h.y); hi[2] = fmaxf(hi[2], h.z);
      const double* m = mom + MT_MOM * (cbase + c);
#pragma unroll
      for (int e = 0; e < MT_FLAG; ++e) s[e] += m[e];
      s[MT_FLAG] = fmax(s[MT_FLAG], m[MT_FLAG]);
    }
    float4* n = nodes + MT_NODE * (base + j);
    n[0] = make_float4(lo[0], lo[1], lo[2], 0.f);
    n[1] = make_float4(hi[0], hi[1], hi[2], s[MT_FLAG] != 0.0 ? 1.f : 0.f);
    double* m = mom + MT_MOM * (base + j);
#pragma unroll
    for (int e = 0; e < MT_MOM; ++e) m[e] = s[e];
  }
}

// grid (nodes of the largest shape, shapes): one workgroup per node.  p~ and the dipole rounded to f32, then the radius about the stored p~
constexpr int MT_FIN_THREADS = 256;
__global__ __launch_bounds__(MT_FIN_THREADS) void mt_finish_kernel(const float* __restrict__ verts, const int* __restrict__ faces,
                                                                  const long long* __restrict__ voff, const long long* __restrict__ toff,
                                                                  const long long* __restrict__ noff, const long long* __restrict__ order,
                                                                  int B, float4* __restrict__ nodes, const double* __restrict__ mom) {
  __shared__ double red[MT_FIN_THREADS / 64];
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const long long t0 = toff[b], Tb = toff[b + 1] - t0, L0 = (Tb + MT_LEAF - 1) / MT_LEAF;
    const long long n = blockIdx.x;                             // block-uniform
    if (n >= noff[b + 1] - noff[b]) continue;
    int l = 0;
    long long j = n;
    while (j >= mt_level_nodes(L0, l)) { j -= mt_level_nodes(L0, l); ++l; }
    float4* nd = nodes + MT_NODE * (noff[b] + n);
    const double* m = mom + MT_MOM * (noff[b] + n);
    const float4 a = nd[0], h = nd[1];
    float pc[3];
    if (m[0] > 0.0) {
      pc[0] = (float)(m[1] / m[0]); pc[1] = (float)(m[2] / m[0]); pc[2] = (float)(m[3] / m[0]);
    } else {
      pc[0] = (float)(((double)a.x + (double)h.x) * 0.5); pc[1] = (float)(((double)a.y + (double)h.y) * 0.5);
      pc[2] = (float)(((double)a.z + (double)h.z) * 0.5);
    }
    const long long v0 = voff[b], nv = voff[b + 1] - v0;
    const long long s0 = t0 + ((j * MT_LEAF) << (3 * l));
    long long s1 = t0 + (((j + 1) * MT_LEAF) << (3 * l));
    s1 = s1 < t0 + Tb ? s1 : t0 + Tb;
    double d2m = 0.0;
    for (long long s = s0 + threadIdx.x; s < s1; s += MT_FIN_THREADS) {
      long long g = order[s];
      g = g >= t0 && g < t0 + Tb ? g : s;
      float p[3][3];
      mt_face_verts(verts, faces, v0, nv, g, p);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double dx = (double)p[c][0] - (double)pc[0], dy = (double)p[c][1] - (double)pc[1], dz = (double)p[c][2] - (double)pc[2];
        d2m = fmax(d2m, (dx * dx + dy * dy) + dz * dz);
      }
    }
    d2m = wave_max_f64(d2m);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = d2m;
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int w = 1; w < MT_FIN_THREADS / 64; ++w) d2m = fmax(d2m, red[w]);
      const double r = sqrt(d2m);
      float rf = (float)r;
      if (!((double)rf >= r)) rf = nextafterf(rf, INFINITY);   // rounded up (a NaN of a non-finite shape stays what it is)
      nd[0] = make_float4(a.x, a.y, a.z, rf);
      // the moments about the stored p~ from the sums about the origin: Q_ik = R2_ik - p_i D_k,
      // M_(ij)k = ((R3_(ij)k - R2_ik p_j) - p_i R2_jk) + (p_i p_j) D_k; then what the expansion reads: tr Q, the symmetric part of Q,
      // g_j = -6 sum_i M_(ij)i - 3 sum_i M_(ii)j, and the 10 coefficients of the cubic form sum M_ijk r_i r_j r_k
      constexpr int SYM[3][3] = {{0, 3, 4}, {3, 1, 5}, {4, 5, 2}}, SI[6] = {0, 1, 2, 0, 0, 1}, SJ[6] = {0, 1, 2, 1, 2, 2};
      const double P[3] = {(double)pc[0], (double)pc[1], (double)pc[2]}, D[3] = {m[4], m[5], m[6]};
      double Q[3][3], M[6][3];
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) Q[i][k] = m[7 + 3 * i + k] - P[i] * D[k];
#pragma unroll
      for (int q = 0; q < 6; ++q)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const int i = SI[q], j = SJ[q];
          M[q][k] = ((m[16 + 3 * q + k] - m[7 + 3 * i + k] * P[j]) - P[i] * m[7 + 3 * j + k]) + (P[i] * P[j]) * D[k];
        }
      double g[3];
#pragma unroll
      for (int j = 0; j < 3; ++j)
        g[j] = -6.0 * ((M[SYM[0][j]][0] + M[SYM[1][j]][1]) + M[SYM[2][j]][2]) - 3.0 * ((M[0][j] + M[1][j]) + M[2][j]);
      nd[2] = make_float4(pc[0], pc[1], pc[2], (float)((Q[0][0] + Q[1][1]) + Q[2][2]));
      nd[3] = make_float4((float)D[0], (float)D[1], (float)D[2], 0.f);
      nd[4] = make_float4((float)Q[0][0], (float)Q[1][1], (float)Q[2][2], (float)(Q[0][1] + Q[1][0]));
      nd[5] = make_float4((float)(Q[0][2] + Q[2][0]), (float)(Q[1][2] + Q[2][1]), (float)g[0], (float)g[1]);
      nd[6] = make_float4((float)g[2], (float)M[0][0], (float)M[1][1], (float)M[2][2]);
      nd[7] = make_float4((float)(M[0][1] + 2.0 * M[3][0]), (float)(M[0][2] + 2.0 * M[4][0]), (float)(M[1][0] + 2.0 * M[3][1]),
                          (float)(M[1][2] + 2.0 * M[5][1]));
      nd[8] = make_float4((float)(M[2][0] + 2.0 * M[4][2]), (float)(M[2][1] + 2.0 * M[5][2]),
                          (float)(2.0 * ((M[3][2] + M[4][1]) + M[5][0])), 0.f);
    }
  }
}

// ---- queries ------------------------------------------------------------------------------------------------------------------------

// a lower bound of closest_vw's d2 for every face below the node (n0, n1): the derivation is at the top of this file
__device__ __forceinline__ float mt_bound(float qx, float qy, float qz, const float4 n0, const float4 n1) {
  const float bm = fmaxf(fmaxf(fmaxf(fabsf(n0.x), fabsf(n0.y)), fabsf(n0.z)), fmaxf(fmaxf(fabsf(n1.x), fabsf(n1.y)), fabsf(n1.z)));
  const float eps = MT_EPS * fmaxf(bm, fmaxf(fmaxf(fabsf(qx), fabsf(qy)), fabsf(qz)));
  const float gx = fmaxf(fmaxf(fmaxf(n0.x - qx, qx - n1.x), 0.f) - eps, 0.f);
  const float gy = fmaxf(fmaxf(fmaxf(n0.y - qy, qy - n1.y), 0.f) - eps, 0.f);
  const float gz = fmaxf(fmaxf(fmaxf(n0.z - qz, qz - n1.z), 0.f) - eps, 0.f);
  const float g2 = fmaf(gz, gz, fmaf(gy, gy, gx * gx)) * MT_SHRINK;
  return n1.w != 0.f ? 0.f : g2;
}

// the node's third-order expansion of the half solid angle seen from q, r = p~ - q (Barill et al. 2018, triangle soups):
//   ((D . r + tr Q) / |r|^3 + (g . r / 2 - 3 r^T Q r) / |r|^5 + 7.5 K(r, r, r) / |r|^7) / 2
__device__ __forceinline__ float mt_expansion(const float4* __restrict__ nd, float trq, const float4 n3, float x, float y, float z, float d2) {
  const float4 n4 = nd[4], n5 = nd[5], n6 = nd[6], n7 = nd[7], n8 = nd[8];
  const float xx = x * x, yy = y * y, zz = z * z;
  const float qf = fmaf(n5.y, y * z, fmaf(n5.x, x * z, fmaf(n4.w, x * y, fmaf(n4.z, zz, fmaf(n4.y, yy, n4.x * xx)))));
  const float gr = dot3(n5.z, n5.w, n6.x, x, y, z);
  float cf = fmaf(n6.w, zz * z, fmaf(n6.z, yy * y, n6.y * (xx * x)));
  cf = fmaf(n7.w, yy * z, fmaf(n7.z, yy * x, fmaf(n7.y, xx * z, fmaf(n7.x, xx * y, cf))));
  cf = fmaf(n8.z, (x * y) * z, fmaf(n8.y, zz * y, fmaf(n8.x, zz * x, cf)));
  const float i3 = __fdiv_rn(1.f, d2 * sqrtf(d2)), i5 = __fdiv_rn(i3, d2), i7 = __fdiv_rn(i5, d2);
  const float t1 = (dot3(n3.x, n3.y, n3.z, x, y, z) + trq) * i3, t2 = fmaf(0.5f, gr, -3.f * qf) * i5, t3 = 7.5f * cf * i7;
  return 0.5f * ((t1 + t2) + t3);
}

struct MtLane {
  float qx, qy, qz;
  bool live;
  float best;                                                  // FULL: the least d2 so far,
  int bi, bs;                                                  //       its original face index and its sorted slot local to the shape
  long long wacc;                                              // the winding sum, 2^-29 fixed point (w_flush)
  unsigned faces, approx;                                      // counters: faces evaluated, expansions taken
};

// the wave enters leaf j of the shape (first sorted face t0, Tb faces): its records through LDS, then every lane over every face
template <bool FULL>
__device__ __forceinline__ void mt_leaf(MtLane& q, const float4* __restrict__ rec, const int* __restrict__ orig, long long t0, int Tb, int j,
                                        bool wneed, bool dwave, float4 (*tile)[MT_LEAF], int* otile) {
  constexpr int NREC = FULL ? SFMI_FACE_REC : 3;
  const int lane = threadIdx.x;
  const int f0 = j * MT_LEAF, cnt = Tb - f0 < MT_LEAF ? Tb - f0 : MT_LEAF;
  __syncthreads();                                             // the previous leaf is consumed
  if (lane < cnt) {
    const float4* src = rec + SFMI_FACE_REC * (t0 + f0 + lane);
    if (FULL) {
#pragma unroll
      for (int k = 0; k < SFMI_FACE_REC; ++k) tile[k][lane] = src[k];
      otile[lane] = orig[t0 + f0 + lane];
    } else {
      tile[0][lane] = src[0];
      tile[1][lane] = src[3];
      tile[2][lane] = src[4];
    }
  }
  __syncthreads();
  const bool wwave = __any(wneed);
  float run = 0.f;
  for (int jj = 0; jj < cnt; ++jj) {
    const float4 r0 = tile[0][jj], r3 = tile[NREC - 2][jj], r4 = tile[NREC - 1][jj];   // broadcast reads
    if (FULL && dwave) {
      const float4 r1 = tile[1][jj], r2 = tile[2][jj];
      const int oi = otile[jj];
      float v, w;
      const float d2 = closest_vw(q.qx, q.qy, q.qz, r0, r1, r2, v, w);
      const bool lt = d2 < q.best || (d2 == q.best && oi < q.bi);
      q.best = lt ? d2 : q.best;
      q.bi = lt ? oi : q.bi;
      q.bs = lt ? f0 + jj : q.bs;
    }
    if (wwave) {
      const float nr = fmaf(r3.w, half_solid_angle(q.qx, q.qy, q.qz, r0, r3, r4), run);
      run = wneed ? nr : run;
    }
  }
  w_flush(run, q.wacc);
  q.faces += q.live ? (unsigned)cnt : 0u;
}

// the walk of one wave over one shape's tree.  nodes: the shape's first node; every lane of the workgroup calls (barriers inside)
template <bool FULL>
__device__ __forceinline__ void mt_walk(MtLane& q, const float4* __restrict__ rec, const int* __restrict__ orig, const float4* __restrict__ nodes,
                                        long long t0, int Tb, float beta, float4 (*tile)[MT_LEAF], int* otile) {
  const int L0 = (Tb + MT_LEAF - 1) / MT_LEAF, top = mt_top(L0);
  long long rootbase = 0;
  for (int k = 0; k < top; ++k) rootbase += mt_level_nodes(L0, k);
  if (FULL) {                                                  // seed `best`: greedy descent by the first lane's query (always live)
    const float cx = __shfl(q.qx, 0, 64), cy = __shfl(q.qy, 0, 64), cz = __shfl(q.qz, 0, 64);
    int l = top, j = 0;
    long long base = rootbase;
    while (l > 0) {
      --l;
      const long long nc = mt_level_nodes(L0, l);
      base -= nc;
      const int c0 = 8 * j, c1 = c0 + 8 < nc ? c0 + 8 : (int)nc;
      float bd = INFINITY;
      int bc = c0;
      for (int c = c0; c < c1; ++c) {
        const float4 n0 = nodes[MT_NODE * (base + c)], n1 = nodes[MT_NODE * (base + c) + 1];
        const float gx = fmaxf(fmaxf(n0.x - cx, cx - n1.x), 0.f), gy = fmaxf(fmaxf(n0.y - cy, cy - n1.y), 0.f),
                    gz = fmaxf(fmaxf(n0.z - cz, cz - n1.z), 0.f);
        const float d = fmaf(gz, gz, fmaf(gy, gy, gx * gx));
        if (d < bd) { bd = d; bc = c; }
      }
      j = bc;
    }
    mt_leaf<true>(q, rec, orig, t0, Tb, j, false, true, tile, otile);
  }
  int l = top, j = 0, mute = -1;
  long long base = rootbase;
  while (true) {
    const float4* nd = nodes + MT_NODE * (base + j);           // wave-uniform address
    const float4 n0 = nd[0], n1 = nd[1], n2 = nd[2], n3 = nd[3];
    mute = l >= mute ? -1 : mute;                              // the walk has left the subtree this lane approximated
    bool wneed = false;
    if (q.live && mute < 0) {
      const float dx = n2.x - q.qx, dy = n2.y - q.qy, dz = n2.z - q.qz;
      const float d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
      const float br = beta * n0.w;
      if (d2 > br * br) {
        float c = mt_expansion(nd, n2.w, n3, dx, dy, dz, d2);
        w_flush(c, q.wacc);
        q.approx += 1u;
        mute = l;
      } else {
        wneed = true;
      }
    }
    bool dneed = false;
    if (FULL) dneed = q.live && !(mt_bound(q.qx, q.qy, q.qz, n0, n1) > q.best);
    if (__any(wneed || dneed)) {
      if (l > 0) {                                             // descend to the first child
        --l;
        base -= mt_level_nodes(L0, l);
        j *= 8;
        continue;
      }
      mt_leaf<FULL>(q, rec, orig, t0, Tb, j, wneed, FULL && __any(dneed), tile, otile);
    }
    while (true) {                                             // the next node in depth-first order
      if (l == top) return;
      const int jn = j + 1;
      if ((jn & 7) != 0 && jn < mt_level_nodes(L0, l)) { j = jn; break; }
      base += mt_level_nodes(L0, l);
      ++l;
      j >>= 3;
    }
  }
}

__device__ __forceinline__ MtLane mt_lane(float x, float y, float z, bool live) {
  return MtLane{x, y, z, live, INFINITY, -1, 0, 0ll, 0u, 0u};
}

__device__ __forceinline__ float mt_winding(const MtLane& q) {
  long long ws = 0;
  bool bad = false;
  w_add(q.wacc, ws, bad);
  return w_value(ws, bad) * INV_2PI;
}

__device__ __forceinline__ void mt_count(const MtLane& q, unsigned long long* __restrict__ counters) {
  if (!counters) return;
  unsigned long long f = q.faces, a = q.approx, n = q.live ? 1u : 0u;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { f += __shfl_xor(f, o, 64); a += __shfl_xor(a, o, 64); n += __shfl_xor(n, o, 64); }
  if (threadIdx.x == 0) { atomicAdd(counters, f); atomicAdd(counters + 1, a); atomicAdd(counters + 2, n); }
}

// one workgroup of 64 lanes per 64 consecutive queries of a set; boff (B+1): the sets' first workgroups
__global__ __launch_bounds__(MT_LEAF) void mt_query_kernel(const float* __restrict__ Q, const long long* __restrict__ qoff,
                                                           const long long* __restrict__ boff, const long long* __restrict__ toff,
                                                           const long long* __restrict__ noff, const float4* __restrict__ rec,
                                                           const int* __restrict__ orig, const float4* __restrict__ nodes,
                                                           const int* __restrict__ status, int B, float beta, float* __restrict__ Sd,
                                                           int* __restrict__ I, float* __restrict__ C, float* __restrict__ W,
                                                           unsigned long long* __restrict__ counters) {
  __shared__ float4 tile[SFMI_FACE_REC][MT_LEAF];
  __shared__ int otile[MT_LEAF];
  const long long g = blockIdx.x;
  if (g >= boff[B]) return;
  const int b = sfmi_owner(boff, B, g);
  const long long i = qoff[b] + (g - boff[b]) * MT_LEAF + threadIdx.x;
  const bool live = i < qoff[b + 1];
  const float nan = __int_as_float(0x7FC00000);
  const long long t0 = toff[b], Tb = toff[b + 1] - t0;
  if (status[b] != 0 || Tb <= 0) {                              // block-uniform
    if (live) {
      Sd[i] = nan;
      if (I) I[i] = -1;
      if (C) C[3 * i] = C[3 * i + 1] = C[3 * i + 2] = nan;
      if (W) W[i] = 0.f;
    }
    return;
  }
  MtLane q = mt_lane(live ? Q[3 * i] : 0.f, live ? Q[3 * i + 1] : 0.f, live ? Q[3 * i + 2] : 0.f, live);
  mt_walk<true>(q, rec, orig, nodes + MT_NODE * noff[b], t0, (int)Tb, beta, tile, otile);
  mt_count(q, counters);
  if (!live) return;
  const float wn = mt_winding(q);
  Sd[i] = fabsf(wn) > 0.5f ? -sqrtf(q.best) : sqrtf(q.best);
  if (I) I[i] = q.bi;
  if (W) W[i] = wn;
  if (C) {
    const float4* r = rec + SFMI_FACE_REC * (t0 + q.bs);        // bs = 0 when no face had a finite d2
    float v, w;
    closest_vw(q.qx, q.qy, q.qz, r[0], r[1], r[2], v, w);
    C[3 * i] = fmaf(w, r[2].x, fmaf(v, r[1].x, r[0].x));
    C[3 * i + 1] = fmaf(w, r[2].y, fmaf(v, r[1].y, r[0].y));
    C[3 * i + 2] = fmaf(w, r[2].z, fmaf(v, r[1].z, r[0].z));
  }
}

// one workgroup of 64 lanes per 4 x 4 x 4 block of lattice points of one shape: occ = |W_tree| > 0.5.  nb = ceil(G / 4)
__global__ __launch_bounds__(MT_LEAF) void mt_occ_kernel(const long long* __restrict__ toff, const long long* __restrict__ noff,
                                                         const float4* __restrict__ rec, const float4* __restrict__ nodes,
                                                         const int* __restrict__ status, int nb, Lattice lat, float beta,
                                                         unsigned char* __restrict__ occ, unsigned long long* __restrict__ counters) {
  __shared__ float4 tile[3][MT_LEAF];
  const long long g = blockIdx.x, nb3 = (long long)nb * nb * nb;
  const int b = (int)(g / nb3);
  const long long k = g - (long long)b * nb3;
  const int lane = threadIdx.x;
  const long long G = lat.G;
  const long long ix = 4 * (k / ((long long)nb * nb)) + (lane >> 4), iy = 4 * ((k / nb) % nb) + ((lane >> 2) & 3), iz = 4 * (k % nb) + (lane & 3);
  const bool live = ix < G && iy < G && iz < G;
  const long long out = (((long long)b * G + ix) * G + iy) * G + iz;
  const long long t0 = toff[b], Tb = toff[b + 1] - t0;
  if (status[b] != 0 || Tb <= 0) {                              // block-uniform
    if (live) occ[out] = 0;
    return;
  }
  MtLane q = mt_lane(lattice_coord(lat, 0, live ? ix : 0), lattice_coord(lat, 1, live ? iy : 0), lattice_coord(lat, 2, live ? iz : 0), live);
  mt_walk<false>(q, rec, nullptr, nodes + MT_NODE * noff[b], t0, (int)Tb, beta, tile, nullptr);
  mt_count(q, counters);
  if (live) occ[out] = fabsf(mt_winding(q)) > 0.5f ? 1 : 0;
}

}  // namespace

extern "C" {

int sfmi_meshtree_leaf_faces(void) { return MT_LEAF; }

long long sfmi_meshtree_nodes(long long T) {
  if (T <= 0) return 0;
  const long long L0 = (T + MT_LEAF - 1) / MT_LEAF;
  long long n = 0;
  for (int l = 0; l <= mt_top(L0); ++l) n += mt_level_nodes(L0, l);
  return n;
}

int sfmi_meshtree_keys_f32(const float* verts, const int* faces, const long long* voff, const long long* toff, int B, long long T,
                           float* bbox, long long* keys, int* flags, void* stream) {
  if (B <= 0 || T < 0 || !voff || !toff || !bbox || !flags || (T > 0 && (!verts || !faces || !keys))) return SFMI_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(mt_bbox_kernel, dim3(sfmi_grid_cap(B)), dim3(MT_BB_THREADS), 0, st, verts, voff, B, bbox, flags);
  if (T > 0) hipLaunchKernelGGL(mt_keys_kernel, dim3(blocks256(T)), dim3(256), 0, st, verts, faces, voff, toff, (const float*)bbox, B, T, keys, flags);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_meshtree_build_f32(const float* verts, const int* faces, const long long* voff, const long long* toff, const long long* noff,
                            const long long* order, const int* flags, int B, long long T, long long max_faces, void* rec, int* orig,
                            void* nodes, double* mom, int* status, void* stream) {
  if (B <= 0 || T < 0 || max_faces < 0 || max_faces > T || max_faces >= (1ll << 31) || !voff || !toff || !noff || !flags || !status)
    return SFMI_EINVAL;
  if (T > 0 && (!verts || !faces || !order || !rec || !orig || !nodes || !mom)) return SFMI_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(mt_status_kernel, dim3(blocks256(B)), dim3(256), 0, st, toff, flags, B, status);
  if (T > 0) {
    const long long L0 = (max_faces + MT_LEAF - 1) / MT_LEAF;
    const int top = mt_top(L0);
    const unsigned gy = sfmi_grid_cap(B);
    hipLaunchKernelGGL(mt_records_kernel, dim3(blocks256(T)), dim3(256), 0, st, verts, faces, voff, toff, order, B, T, (float4*)rec, orig);
    hipLaunchKernelGGL(mt_leaf_kernel, dim3((unsigned)cdiv(L0, 64), gy), dim3(64), 0, st, verts, faces, voff, toff, noff, order,
                       (const float4*)rec, B, (float4*)nodes, mom);
    for (int l = 1; l <= top; ++l)
      hipLaunchKernelGGL(mt_up_kernel, dim3((unsigned)cdiv(mt_level_nodes(L0, l), 64), gy), dim3(64), 0, st, toff, noff, B, l, (float4*)nodes, mom);
    hipLaunchKernelGGL(mt_finish_kernel, dim3((unsigned)sfmi_meshtree_nodes(max_faces), gy), dim3(MT_FIN_THREADS), 0, st, verts, faces, voff, toff,
                       noff, order, B, (float4*)nodes, (const double*)mom);
  }
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_meshtree_query_f32(const float* Q, const long long* qoff, const long long* boff, long long blocks, const long long* toff,
                            const long long* noff, const void* rec, const int* orig, const void* nodes, const int* status, int B, long long N,
                            float beta, float* S, int* I, float* C, float* W, unsigned long long* counters, void* stream) {
  if (B <= 0 || N < 0 || blocks < 0 || blocks >= (1ll << 31) || !qoff || !boff || !toff || !noff || !status || !(beta >= 0.f)) return SFMI_EINVAL;
  if (N > 0 && (!Q || !S || !rec || !orig || !nodes)) return SFMI_EINVAL;
  if (N == 0 || blocks == 0) return SFMI_OK;
  hipLaunchKernelGGL(mt_query_kernel, dim3((unsigned)blocks), dim3(MT_LEAF), 0, (hipStream_t)stream, Q, qoff, boff, toff, noff, (const float4*)rec,
                     orig, (const float4*)nodes, status, B, beta, S, I, C, W, counters);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_meshtree_occupancy_f32(const long long* toff, const long long* noff, const void* rec, const void* nodes, const int* status, int B, int G,
                                const double* lo, const double* hi, float beta, unsigned char* occ, unsigned long long* counters, void* stream) {
  if (B <= 0 || G <= 0 || !lo || !hi || !toff || !noff || !status || !occ || !(beta >= 0.f)) return SFMI_EINVAL;
  const long long nb = (G + 3) / 4, blocks = nb * nb * nb * B;
  if (blocks >= (1ll << 31)) return SFMI_EINVAL;
  Lattice lat;
  lat.G = G;
  for (int a = 0; a < 3; ++a) {
    lat.lo[a] = lo[a];
    lat.hi[a] = hi[a];
    lat.step[a] = G > 1 ? (hi[a] - lo[a]) / (double)(G - 1) : 0.0;
  }
  hipLaunchKernelGGL(mt_occ_kernel, dim3((unsigned)blocks), dim3(MT_LEAF), 0, (hipStream_t)stream, toff, noff, (const float4*)rec,
                     (const float4*)nodes, status, (int)nb, lat, beta, occ, counters);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

}  // extern "C"
