// Mesh decimation on the device: quadric vertex clustering of the ragged indexed meshes of csrc/mcubes.hip /
// csrc/iso_sparse.hip on a per-shape G^3 grid over a box.  The reference decimates on the host, xgutils/geoutil.py:175-233
// (array2mesh(..., if_decimate, decimate_face) -> igl.decimate, an edge-collapse method); what is kept is its interface, a face budget
// that leaves a mesh at or below it alone, not igl's output.  The contract is in include/sfmi.h, its numpy statement in
// tests/simplify_ref.py.
//
// Data structure: per shape a bit set of G^3 bits keyed by the cell key (c0 G + c1) G + c2 and per 32-bit word the inclusive prefix
// count of set bits over the batch - the scheme of csrc/iso_sparse.hip with a word offset per shape, since G differs per shape.
// atomicOr de-duplicates, rank + popcount gives a cell's slot in O(1), and the ascending order of the output vertices comes for free.
//   cells   vertex -> cell key and its bit; the shape's flags: no vertices, a face index outside the shape, a non-finite vertex
//   popc    set bits per word (0 for a flagged shape), and the status codes
//   slots   vertex -> batch-wide cell slot
//   faces   face -> survive flag (three distinct cells), the corner records' slots, survivors per shape: the counting pass
//   solve   one wave per cell: mean of its vertices and the quadric of its corners' face planes in f64, a 3x3 Cholesky solve, clamp
//   emit    surviving faces, re-indexed to slots local to the shape
// Integer atomicOr / atomicAdd only.  The solve walks each cell's records in a stably sorted order with lane l taking entries
// l, l+64, ... and reduces with a fixed butterfly, so a cell's vertex depends on its shape alone and is the same bits every run.
#include "sfmi_ragged.h"   // the ragged-batch helpers the mesh tools share: DESIGN.md §5.5a
#include "sfmi_quadric.h"  // the 3x3 Cholesky solve, shared with csrc/collapse.hip

// the f32 cell expression and the f64 plane terms are written once, here and in numpy: no contraction into fused multiply-adds
#pragma clang fp contract(off)

namespace {

constexpr int SIMP_GMAX = 512;
constexpr int SIMP_NONE = 0x7fffffff;   // the slot of a flagged shape's vertices and corners: sorts behind every cell

struct SimpBoxF { float lo[3], hi[3]; };
struct SimpBoxD { double lo[3], hi[3]; };

// threads [0,V): vertices; [V,V+T): faces; [V+T,V+T+B): shapes
__global__ __launch_bounds__(256) void simp_cells_kernel(const float* __restrict__ verts, const int* __restrict__ faces,
                                                         const int* __restrict__ voff, const int* __restrict__ toff,
                                                         const int* __restrict__ grid, const int* __restrict__ woff, int B, int V, int T,
                                                         SimpBoxF box, int* __restrict__ vkey, unsigned* __restrict__ bits,
                                                         int* __restrict__ flags) {
  const long long t = blockIdx.x * 256ll + threadIdx.x;
  unsigned w = 0xFFFFFFFFu, m = 0;      // the bit this lane has to set (m == 0: none)
  if (t < V) {
    const int i = (int)t, b = sfmi_shape_of(voff, B, i);
    const float p[3] = {verts[3ll * i], verts[3ll * i + 1], verts[3ll * i + 2]};
    if (isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2])) {
      const int G = grid[b];
      const float fg = (float)G;
      int key = 0;
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        const float u = __fdiv_rn(p[d] - box.lo[d], box.hi[d] - box.lo[d]);
        // clamped as a float, then converted: the value of clamp((int)floorf(u G), 0, G-1) wherever that cast is defined
        const int c = (int)fminf(fmaxf(floorf(u * fg), 0.0f), fg - 1.0f);
        key = key * G + c;
      }
      vkey[i] = key;
      w = (unsigned)woff[b] + ((unsigned)key >> 5);
      m = 1u << (key & 31);
    } else {
      vkey[i] = 0;
      atomicOr(&flags[b], SFMI_MESH_NON_FINITE);
    }
  } else if (t < (long long)V + T) {
    const int j = (int)(t - V), b = sfmi_shape_of(toff, B, j);
    const int nv = voff[b + 1] - voff[b];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int a = faces[3ll * j + k];
      ok = ok && a >= 0 && a < nv;
    }
    if (!ok) atomicOr(&flags[b], SFMI_MESH_BAD_INDEX);
  } else if (t < (long long)V + T + B) {
    const int b = (int)(t - V - T);
    if (voff[b + 1] <= voff[b]) atomicOr(&flags[b], SFMI_MESH_NO_VERTS);
  }
  // Mesh vertices come in lattice order, so on a coarse grid whole runs of lanes name the same bit, and before the first atomicOr
  // lands every thread in flight would issue its own on a handful of words.  A lane whose left neighbour names the same bit leaves
  // it to that neighbour (all 64 lanes reach the shuffles: no branch above returns).
  const unsigned pw = __shfl_up(w, 1, 64), pm = __shfl_up(m, 1, 64);
  if (m && ((threadIdx.x & 63) == 0 || pw != w || pm != m) && !(bits[w] & m)) atomicOr(&bits[w], m);
}

__global__ __launch_bounds__(256) void simp_popc_kernel(const unsigned* __restrict__ bits, const int* __restrict__ flags,
                                                        const int* __restrict__ woff, int B, int nW, int* __restrict__ cnt,
                                                        int* __restrict__ status) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < B) status[i] = sfmi_mesh_status(flags[i]);
  if (i >= nW) return;
  cnt[i] = flags[sfmi_shape_of(woff, B, i)] ? 0 : __popc(bits[i]);
}

// vslot[i] = the batch-wide slot of vertex i's cell (inclusive count up to the key's word minus the bits at or above it), SIMP_NONE for
// a vertex of a flagged shape.  Slots are sort keys and values only: nothing is indexed by one
__global__ __launch_bounds__(256) void simp_slots_kernel(const int* __restrict__ vkey, const int* __restrict__ voff,
                                                         const int* __restrict__ woff, const unsigned* __restrict__ bits,
                                                         const int* __restrict__ rank, const int* __restrict__ flags, int B, int V,
                                                         int* __restrict__ vslot) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= V) return;
  const int b = sfmi_shape_of(voff, B, i);
  if (flags[b]) { vslot[i] = SIMP_NONE; return; }
  const int key = vkey[i];
  const unsigned w = (unsigned)woff[b] + ((unsigned)key >> 5);
  vslot[i] = rank[w] - __popc(bits[w] >> (key & 31));
}

__global__ __launch_bounds__(256) void simp_faces_kernel(const int* __restrict__ faces, const int* __restrict__ voff,
                                                         const int* __restrict__ toff, const int* __restrict__ vslot,
                                                         const int* __restrict__ flags, int B, int T, int* __restrict__ cslot,
                                                         unsigned char* __restrict__ surv, int* __restrict__ count) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  int b = -1;
  bool keep = false;
  if (j < T) {
    b = sfmi_shape_of(toff, B, j);
    int s[3] = {SIMP_NONE, SIMP_NONE, SIMP_NONE};
    if (!flags[b]) {           // the indices of an unflagged shape are all inside it
      const int vb = voff[b];
#pragma unroll
      for (int k = 0; k < 3; ++k) s[k] = vslot[vb + faces[3ll * j + k]];
      keep = s[0] != s[1] && s[1] != s[2] && s[0] != s[2];
    }
    surv[j] = keep ? 1 : 0;
    if (cslot) {
#pragma unroll
      for (int k = 0; k < 3; ++k) cslot[3ll * j + k] = s[k];
    }
  }
  // one atomicAdd per wave and shape where the wave's faces are of one shape (the common case), else one per face
  const int b0 = __shfl(b, 0, 64);
  const unsigned long long same = __ballot(keep && b == b0);
  if ((threadIdx.x & 63) == 0 && same) atomicAdd(&count[b0], __popcll(same));
  if (keep && b != b0) atomicAdd(&count[b], 1);
}

// one wave64 per cell.  vorder / corder: the vertices / the corner records (3 f + k) stably sorted by slot; vseg / cseg (nC+1): where
// each cell's run starts.  Every cell holds at least one vertex, which names its shape and key.
__global__ __launch_bounds__(256) void simp_solve_kernel(const float* __restrict__ verts, const int* __restrict__ faces,
                                                         const int* __restrict__ voff, const int* __restrict__ vkey,
                                                         const int* __restrict__ grid, const int* __restrict__ vorder,
                                                         const int* __restrict__ vseg, const int* __restrict__ corder,
                                                         const int* __restrict__ cseg, int B, int nC, SimpBoxD box, double reg,
                                                         float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= nC) return;
  const int v0 = vseg[c], v1 = vseg[c + 1];
  if (v1 <= v0) return;
  const int first = vorder[v0];
  const int b = sfmi_shape_of(voff, B, first);
  const int G = min(max(grid[b], 1), SIMP_GMAX), key = vkey[first], vb = voff[b];
  const int cc[3] = {key / (G * G), (key / G) % G, key % G};
  double h[3], ctr[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    h[d] = (box.hi[d] - box.lo[d]) / (double)G;
    ctr[d] = box.lo[d] + ((double)cc[d] + 0.5) * h[d];
  }
  double m0 = 0, m1 = 0, m2 = 0;
  for (int i = v0 + lane; i < v1; i += 64) {
    const float* p = verts + 3ll * vorder[i];
    m0 += (double)p[0] - ctr[0];
    m1 += (double)p[1] - ctr[1];
    m2 += (double)p[2] - ctr[2];
  }
  double a00 = 0, a01 = 0, a02 = 0, a11 = 0, a12 = 0, a22 = 0, b0 = 0, b1 = 0, b2 = 0;
  for (int i = cseg[c] + lane, e = cseg[c + 1]; i < e; i += 64) {
    const int* f = faces + 3ll * (corder[i] / 3);
    const float *q0 = verts + 3ll * (vb + f[0]), *q1 = verts + 3ll * (vb + f[1]), *q2 = verts + 3ll * (vb + f[2]);
    const double p0[3] = {q0[0], q0[1], q0[2]};
    const double e1[3] = {(double)q1[0] - p0[0], (double)q1[1] - p0[1], (double)q1[2] - p0[2]};
    const double e2[3] = {(double)q2[0] - p0[0], (double)q2[1] - p0[1], (double)q2[2] - p0[2]};
    const double n0 = e1[1] * e2[2] - e1[2] * e2[1], n1 = e1[2] * e2[0] - e1[0] * e2[2], n2 = e1[0] * e2[1] - e1[1] * e2[0];
    const double d = -(n0 * (p0[0] - ctr[0]) + n1 * (p0[1] - ctr[1]) + n2 * (p0[2] - ctr[2]));
    a00 += n0 * n0; a01 += n0 * n1; a02 += n0 * n2; a11 += n1 * n1; a12 += n1 * n2; a22 += n2 * n2;
    b0 += d * n0; b1 += d * n1; b2 += d * n2;
  }
  m0 = wave_sum_f64(m0); m1 = wave_sum_f64(m1); m2 = wave_sum_f64(m2);
  a00 = wave_sum_f64(a00); a01 = wave_sum_f64(a01); a02 = wave_sum_f64(a02);
  a11 = wave_sum_f64(a11); a12 = wave_sum_f64(a12); a22 = wave_sum_f64(a22);
  b0 = wave_sum_f64(b0); b1 = wave_sum_f64(b1); b2 = wave_sum_f64(b2);
  if (lane) return;
  const double nv = (double)(v1 - v0);
  const double m[3] = {m0 / nv, m1 / nv, m2 / nv};
  double x[3] = {m[0], m[1], m[2]};
  const double tr = a00 + a11 + a22;
  if (tr > 0.0) {
    // (A + lam I) x = -b + lam m, symmetric positive definite with condition <= 1 + 1/reg: Cholesky L L^T
    sfmi_quadric_solve(a00, a01, a02, a11, a12, a22, b0, b1, b2, reg * tr, m, x);
  }
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const double hh = 0.5 * h[d];
    out[3ll * c + d] = (float)(ctr[d] + fmin(fmax(x[d], -hh), hh));   // a continuous clamp (NaN -> -h/2): no branch a rounding could flip
  }
}

__global__ __launch_bounds__(256) void simp_emit_kernel(const int* __restrict__ faces, const int* __restrict__ voff,
                                                        const int* __restrict__ toff, const int* __restrict__ vslot,
                                                        const unsigned char* __restrict__ surv, const int* __restrict__ sincl,
                                                        const int* __restrict__ coff, int B, int T, int nS, int* __restrict__ out) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= T || !surv[j]) return;
  const int dst = sincl[j] - 1;
  if (dst < 0 || dst >= nS) return;
  const int b = sfmi_shape_of(toff, B, j), vb = voff[b], cb = coff[b];
#pragma unroll
  for (int k = 0; k < 3; ++k) out[3ll * dst + k] = vslot[vb + faces[3ll * j + k]] - cb;
}

// every G in [1, 512]; -> the bit sets' words, or -1
inline long long simp_words(const int* grid_host, int B) {
  if (!grid_host || B <= 0) return -1;
  long long n = 0;
  for (int b = 0; b < B; ++b) {
    const long long G = grid_host[b];
    if (G < 1 || G > SIMP_GMAX) return -1;
    n += (G * G * G + 31) >> 5;
  }
  return n < (1ll << 31) ? n : -1;
}

// a box with lo < hi whose f32 form keeps a finite, positive extent
inline bool simp_box(const double* lo, const double* hi, SimpBoxF* f, SimpBoxD* d) {
  if (!lo || !hi) return false;
  for (int k = 0; k < 3; ++k) {
    const float l = (float)lo[k], h = (float)hi[k];
    if (!(lo[k] < hi[k]) || !std::isfinite(l) || !std::isfinite(h) || !(h - l > 0.0f) || !std::isfinite(h - l)) return false;
    if (f) { f->lo[k] = l; f->hi[k] = h; }
    if (d) { d->lo[k] = lo[k]; d->hi[k] = hi[k]; }
  }
  return true;
}

}  // namespace

extern "C" {

long long sfmi_simplify_words(const int* grid_host, int B) { return simp_words(grid_host, B); }

int sfmi_simplify_cells_f32(const float* verts, const int* faces, const int* voff, const int* toff, const int* grid_host, const int* grid,
                            const int* woff, int B, int V, int T, const double* lo, const double* hi, int* vkey, unsigned* bits, int* flags,
                            void* stream) {
  SimpBoxF box;
  const long long nW = simp_words(grid_host, B);
  if (nW < 0 || V < 0 || T < 0 || (long long)V + T + B >= (1ll << 31) || !simp_box(lo, hi, &box, nullptr)) return SFMI_EINVAL;
  if (!voff || !toff || !grid || !woff || !bits || !flags || (V > 0 && (!verts || !vkey)) || (T > 0 && !faces)) return SFMI_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  SFMI_TRY(hipMemsetAsync(bits, 0, (size_t)nW * 4, st));
  SFMI_TRY(hipMemsetAsync(flags, 0, (size_t)B * 4, st));
  hipLaunchKernelGGL(simp_cells_kernel, dim3(blocks256((long long)V + T + B)), dim3(256), 0, st, verts, faces, voff, toff, grid, woff, B, V, T, box,
                     vkey, bits, flags);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_simplify_popc_i32(const unsigned* bits, const int* flags, const int* woff, const int* grid_host, int B, int* cnt, int* status,
                           void* stream) {
  const long long nW = simp_words(grid_host, B);
  if (nW < 0 || !bits || !flags || !woff || !cnt || !status) return SFMI_EINVAL;
  hipLaunchKernelGGL(simp_popc_kernel, dim3(blocks256(nW)), dim3(256), 0, (hipStream_t)stream, bits, flags, woff, B, (int)nW, cnt, status);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_simplify_slots_i32(const int* vkey, const int* voff, const int* woff, const unsigned* bits, const int* rank, const int* flags,
                            const int* grid_host, int B, int V, int* vslot, void* stream) {
  if (simp_words(grid_host, B) < 0 || V < 0 || !voff || !woff || !bits || !rank || !flags || (V > 0 && (!vkey || !vslot)))
    return SFMI_EINVAL;
  if (V == 0) return SFMI_OK;
  hipLaunchKernelGGL(simp_slots_kernel, dim3(blocks256(V)), dim3(256), 0, (hipStream_t)stream, vkey, voff, woff, bits, rank, flags, B, V, vslot);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_simplify_faces_i32(const int* faces, const int* voff, const int* toff, const int* vslot, const int* flags, int B, int T,
                            int* cslot, unsigned char* surv, int* count, void* stream) {
  if (B <= 0 || T < 0 || 3ll * T >= (1ll << 31) || !voff || !toff || !flags || !count || (T > 0 && (!faces || !vslot || !surv)))
    return SFMI_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  SFMI_TRY(hipMemsetAsync(count, 0, (size_t)B * 4, st));
  if (T > 0)
    hipLaunchKernelGGL(simp_faces_kernel, dim3(blocks256(T)), dim3(256), 0, st, faces, voff, toff, vslot, flags, B, T, cslot, surv, count);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_simplify_solve_f32(const float* verts, const int* faces, const int* voff, const int* vkey, const int* grid_host, const int* grid,
                            const int* vorder, const int* vseg, const int* corder, const int* cseg, int B, int nC, const double* lo,
                            const double* hi, double reg, float* out, void* stream) {
  SimpBoxD box;
  if (simp_words(grid_host, B) < 0 || nC < 0 || !simp_box(lo, hi, nullptr, &box) || !(reg > 0.0) || !std::isfinite(reg)) return SFMI_EINVAL;
  if (!voff || !grid || !vseg || !cseg || (nC > 0 && (!verts || !vkey || !vorder || !out))) return SFMI_EINVAL;
  if (nC == 0) return SFMI_OK;
  hipLaunchKernelGGL(simp_solve_kernel, dim3((unsigned)((nC + 3) / 4)), dim3(256), 0, (hipStream_t)stream, verts, faces, voff, vkey, grid, vorder,
                     vseg, corder, cseg, B, nC, box, reg, out);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_simplify_emit_i32(const int* faces, const int* voff, const int* toff, const int* vslot, const unsigned char* surv, const int* sincl,
                           const int* coff, int B, int T, int nS, int* out, void* stream) {
  if (B <= 0 || T < 0 || nS < 0 || !voff || !toff || !coff || (T > 0 && (!faces || !vslot || !surv || !sincl)) || (nS > 0 && !out))
    return SFMI_EINVAL;
  if (T == 0 || nS == 0) return SFMI_OK;
  hipLaunchKernelGGL(simp_emit_kernel, dim3(blocks256(T)), dim3(256), 0, (hipStream_t)stream, faces, voff, toff, vslot, surv, sincl, coff, B, T, nS,
                     out);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

}  // extern "C"
