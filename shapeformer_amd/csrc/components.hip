// Mesh connected components on the device: labels, per-component statistics and compaction of the ragged indexed
// meshes of csrc/mcubes.hip / csrc/iso_sparse.hip / csrc/simplify.hip.  The reference has a stub for this step, xgutils/geoutil.py:151-163
// (filterMesh, a vertex-mask filter with "# TODO filterF").  The contract is in include/sfmi.h, its numpy statement in
// tests/components_ref.py.
//
// One int32 `parent` array over the batch's vertices (batch-wide indices), the lock-free union-find of csrc/sfmi_ragged.h (DESIGN.md
// §5.5a, where its race argument is written down once):
//   init     parent[v] = v; the shape's flags: no vertices, a face index outside the shape, a non-finite vertex
//   hook     one thread per face: the union of its corners; marks the vertices a face names
//   flatten  a launch of its own (the kernel boundary makes every hook visible): root[v], and which vertices are roots
//   number   labels from the exclusive count of roots (a prefix sum between the launches), and the batch-wide component of every vertex
//            and face: the sort keys whose runs give the vertices / faces per component (no counter that every wave would add to)
//   partial  one wave per chunk of 1024 faces of a component's run (faces stably sorted by component): the f64 area / volume sums
//   total    one wave per component: its chunks' partial sums
//   mark     keep flags of vertices and faces from the keep flag of their component
//   emit     kept vertices and re-indexed kept faces at the slots an exclusive count gives
// parent[v] <= v always holds, so the root of a finished tree is the smallest index of its component whatever order the hooks came
// in: the labels are a function of the mesh.  Integer atomics only; every f64 sum runs in a fixed order over a fixed tree.
#include "sfmi_ragged.h"

// the f64 face terms are written once, here and in numpy: no contraction into fused multiply-adds
#pragma clang fp contract(off)

namespace {

constexpr int CC_CHUNK = 1024;          // faces per chunk of a component's run, counted from the run's own start
constexpr int CC_NONE = 0x7fffffff;     // the sort key of a flagged shape's faces: sorts behind every component

// threads [0,V): vertices; [V,V+T): faces; [V+T,V+T+B): shapes
__global__ __launch_bounds__(256) void cc_init_kernel(const float* __restrict__ verts, const int* __restrict__ faces,
                                                      const int* __restrict__ voff, const int* __restrict__ toff, int B, int V, int T,
                                                      int* __restrict__ parent, int* __restrict__ flags) {
  const long long t = blockIdx.x * 256ll + threadIdx.x;
  if (t < V) {
    const int i = (int)t;
    parent[i] = i;
    if (!(isfinite(verts[3ll * i]) && isfinite(verts[3ll * i + 1]) && isfinite(verts[3ll * i + 2])))
      atomicOr(&flags[sfmi_shape_of(voff, B, i)], SFMI_MESH_NON_FINITE);
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
}

__global__ __launch_bounds__(256) void cc_hook_kernel(const int* __restrict__ faces, const int* __restrict__ voff,
                                                      const int* __restrict__ toff, const int* __restrict__ flags, int B, int T,
                                                      int* parent, unsigned char* __restrict__ ref) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= T) return;
  const int b = sfmi_shape_of(toff, B, j);
  if (flags[b]) return;          // the indices of an unflagged shape are all inside it
  const int vb = voff[b];
  const int a = vb + faces[3ll * j], c = vb + faces[3ll * j + 1], d = vb + faces[3ll * j + 2];
  ref[a] = 1; ref[c] = 1; ref[d] = 1;
  if (c != a) sfmi_uf_hook(parent, a, c);
  if (d != a && d != c) sfmi_uf_hook(parent, a, d);
}

// parent is only read here
__global__ __launch_bounds__(256) void cc_flatten_kernel(const int* __restrict__ parent, const unsigned char* __restrict__ ref, int V,
                                                         int* __restrict__ root, int* __restrict__ isroot) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= V) return;
  int r = v, p = parent[r];
  while (p != r) { r = p; p = parent[r]; }
  root[v] = r;
  isroot[v] = (ref[v] && r == v) ? 1 : 0;
}

// threads [0,V): vertices; [V,V+T): faces; [V+T,V+T+B): shapes.  rank: the INCLUSIVE prefix sum of isroot; coff (B+1): the roots before
// each shape's first vertex.  vkey / fkey: the batch-wide component, CC_NONE where there is none
__global__ __launch_bounds__(256) void cc_number_kernel(const int* __restrict__ faces, const int* __restrict__ voff,
                                                        const int* __restrict__ toff, const int* __restrict__ flags,
                                                        const int* __restrict__ root, const unsigned char* __restrict__ ref,
                                                        const int* __restrict__ rank, const int* __restrict__ coff, int B, int V, int T,
                                                        int* __restrict__ vlabel, int* __restrict__ flabel, int* __restrict__ vkey,
                                                        int* __restrict__ fkey, int* __restrict__ status) {
  const long long t = blockIdx.x * 256ll + threadIdx.x;
  if (t < V) {
    const int v = (int)t;
    int lab = -1, key = CC_NONE;
    if (ref[v]) {
      key = rank[root[v]] - 1;
      lab = key - coff[sfmi_shape_of(voff, B, v)];
    }
    vlabel[v] = lab;
    vkey[v] = key;
  } else if (t < (long long)V + T) {
    const int j = (int)(t - V), b = sfmi_shape_of(toff, B, j);
    int lab = -1, key = CC_NONE;
    if (!flags[b]) {
      key = rank[root[voff[b] + faces[3ll * j]]] - 1;
      lab = key - coff[b];
    }
    flabel[j] = lab;
    fkey[j] = key;
  } else if (t < (long long)V + T + B) {
    const int b = (int)(t - V - T);
    status[b] = sfmi_mesh_status(flags[b]);
  }
}

// one wave64 per chunk.  forder: the faces stably sorted by fkey; seg (nC+1): where each component's run starts; choff (nC+1): where its
// chunks start.  Lane l takes entries l, l+64, ... of the chunk; a fixed xor butterfly adds the lanes
__global__ __launch_bounds__(256) void cc_partial_kernel(const float* __restrict__ verts, const int* __restrict__ faces,
                                                         const int* __restrict__ voff, const int* __restrict__ toff,
                                                         const int* __restrict__ forder, const int* __restrict__ seg,
                                                         const int* __restrict__ choff, int B, int T, int nC, int nW,
                                                         double* __restrict__ part) {
  const int lane = threadIdx.x & 63;
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= nW || w >= choff[nC]) return;
  int lo = 0, hi = nC;           // the component c with choff[c] <= w < choff[c+1]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (choff[mid] <= w) lo = mid; else hi = mid;
  }
  const int c = lo;
  const int s = seg[c] + (w - choff[c]) * CC_CHUNK, e = min(seg[c + 1], s + CC_CHUNK);
  if (s < 0 || e > T || s >= e) { if (!lane) { part[2ll * w] = 0.0; part[2ll * w + 1] = 0.0; } return; }
  const int vb = voff[sfmi_shape_of(toff, B, forder[s])];
  double area = 0.0, vol = 0.0;
  for (int i = s + lane; i < e; i += 64) {
    const int* f = faces + 3ll * forder[i];
    const float *q0 = verts + 3ll * (vb + f[0]), *q1 = verts + 3ll * (vb + f[1]), *q2 = verts + 3ll * (vb + f[2]);
    const double a[3] = {q0[0], q0[1], q0[2]}, p[3] = {q1[0], q1[1], q1[2]}, q[3] = {q2[0], q2[1], q2[2]};
    const double e1[3] = {p[0] - a[0], p[1] - a[1], p[2] - a[2]}, e2[3] = {q[0] - a[0], q[1] - a[1], q[2] - a[2]};
    const double n0 = e1[1] * e2[2] - e1[2] * e2[1], n1 = e1[2] * e2[0] - e1[0] * e2[2], n2 = e1[0] * e2[1] - e1[1] * e2[0];
    area += sqrt(n0 * n0 + n1 * n1 + n2 * n2) * 0.5;
    const double x0 = p[1] * q[2] - p[2] * q[1], x1 = p[2] * q[0] - p[0] * q[2], x2 = p[0] * q[1] - p[1] * q[0];
    vol += (a[0] * x0 + a[1] * x1 + a[2] * x2) / 6.0;
  }
  area = wave_sum_f64(area);
  vol = wave_sum_f64(vol);
  if (!lane) { part[2ll * w] = area; part[2ll * w + 1] = vol; }
}

// one wave64 per component: lane l takes its chunks l, l+64, ...; the same butterfly
__global__ __launch_bounds__(256) void cc_total_kernel(const double* __restrict__ part, const int* __restrict__ choff, int nC, int nW,
                                                       double* __restrict__ area, double* __restrict__ volume) {
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= nC) return;
  const int c0 = choff[c], c1 = min(choff[c + 1], nW);
  if (c1 - c0 <= 1) {            // no chunk: zero; one chunk: its sums as they are (what the butterfly over p, 0, .., 0 gives)
    if (!lane) { area[c] = c1 > c0 ? part[2ll * c0] + 0.0 : 0.0; volume[c] = c1 > c0 ? part[2ll * c0 + 1] + 0.0 : 0.0; }
    return;
  }
  double a = 0.0, v = 0.0;
  for (int i = c0 + lane, e = c1; i < e; i += 64) {
    a += part[2ll * i];
    v += part[2ll * i + 1];
  }
  a = wave_sum_f64(a);
  v = wave_sum_f64(v);
  if (!lane) { area[c] = a; volume[c] = v; }
}

// threads [0,V): vertices; [V,V+T): faces.  keep (nC) uint8 per batch-wide component
__global__ __launch_bounds__(256) void cc_mark_kernel(const int* __restrict__ vlabel, const int* __restrict__ flabel,
                                                      const int* __restrict__ voff, const int* __restrict__ toff,
                                                      const int* __restrict__ coff, const unsigned char* __restrict__ keep, int B, int V,
                                                      int T, int nC, unsigned char* __restrict__ vkeep, unsigned char* __restrict__ fkeep) {
  const long long t = blockIdx.x * 256ll + threadIdx.x;
  if (t < V) {
    const int v = (int)t, lab = vlabel[v];
    const int gc = lab < 0 ? -1 : lab + coff[sfmi_shape_of(voff, B, v)];
    vkeep[v] = (gc >= 0 && gc < nC && keep[gc]) ? 1 : 0;
  } else if (t < (long long)V + T) {
    const int j = (int)(t - V), lab = flabel[j];
    const int gc = lab < 0 ? -1 : lab + coff[sfmi_shape_of(toff, B, j)];
    fkeep[j] = (gc >= 0 && gc < nC && keep[gc]) ? 1 : 0;
  }
}

// vincl / fincl: inclusive prefix sums of vkeep / fkeep; nvoff (B+1): the kept vertices before each shape.  A kept face's corners are
// kept vertices of its shape (they carry the face's component)
__global__ __launch_bounds__(256) void cc_emit_kernel(const float* __restrict__ verts, const int* __restrict__ faces,
                                                      const int* __restrict__ voff, const int* __restrict__ toff,
                                                      const unsigned char* __restrict__ vkeep, const unsigned char* __restrict__ fkeep,
                                                      const int* __restrict__ vincl, const int* __restrict__ fincl,
                                                      const int* __restrict__ nvoff, int B, int V, int T, int nVo, int nTo,
                                                      float* __restrict__ out_v, int* __restrict__ out_f) {
  const long long t = blockIdx.x * 256ll + threadIdx.x;
  if (t < V) {
    const int v = (int)t;
    if (!vkeep[v]) return;
    const int dst = vincl[v] - 1;
    if (dst < 0 || dst >= nVo) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) out_v[3ll * dst + k] = verts[3ll * v + k];
  } else if (t < (long long)V + T) {
    const int j = (int)(t - V);
    if (!fkeep[j]) return;
    const int dst = fincl[j] - 1;
    if (dst < 0 || dst >= nTo) return;
    const int b = sfmi_shape_of(toff, B, j), vb = voff[b], nb = nvoff[b];
#pragma unroll
    for (int k = 0; k < 3; ++k) out_f[3ll * dst + k] = vincl[vb + faces[3ll * j + k]] - 1 - nb;
  }
}

inline bool cc_sizes(int B, int V, int T) {
  return B > 0 && V >= 0 && T >= 0 && (long long)V + T + B < (1ll << 31) && 3ll * T < (1ll << 31);
}

}  // namespace

extern "C" {

int sfmi_cc_chunk(void) { return CC_CHUNK; }

int sfmi_cc_init_f32(const float* verts, const int* faces, const int* voff, const int* toff, int B, int V, int T, int* parent,
                     unsigned char* ref, int* flags, void* stream) {
  if (!cc_sizes(B, V, T) || !voff || !toff || !flags || (V > 0 && (!verts || !parent || !ref)) || (T > 0 && !faces)) return SFMI_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  SFMI_TRY(hipMemsetAsync(flags, 0, (size_t)B * 4, st));
  if (V > 0) SFMI_TRY(hipMemsetAsync(ref, 0, (size_t)V, st));
  hipLaunchKernelGGL(cc_init_kernel, dim3(blocks256((long long)V + T + B)), dim3(256), 0, st, verts, faces, voff, toff, B, V, T, parent, flags);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_cc_hook_i32(const int* faces, const int* voff, const int* toff, const int* flags, int B, int V, int T, int* parent,
                     unsigned char* ref, void* stream) {
  if (!cc_sizes(B, V, T) || !voff || !toff || !flags || (T > 0 && (!faces || !parent || !ref))) return SFMI_EINVAL;
  if (T == 0 || V == 0) return SFMI_OK;
  hipLaunchKernelGGL(cc_hook_kernel, dim3(blocks256(T)), dim3(256), 0, (hipStream_t)stream, faces, voff, toff, flags, B, T, parent, ref);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_cc_flatten_i32(const int* parent, const unsigned char* ref, int V, int* root, int* isroot, void* stream) {
  if (V < 0 || (V > 0 && (!parent || !ref || !root || !isroot))) return SFMI_EINVAL;
  if (V == 0) return SFMI_OK;
  hipLaunchKernelGGL(cc_flatten_kernel, dim3(blocks256(V)), dim3(256), 0, (hipStream_t)stream, parent, ref, V, root, isroot);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_cc_number_i32(const int* faces, const int* voff, const int* toff, const int* flags, const int* root, const unsigned char* ref,
                       const int* rank, const int* coff, int B, int V, int T, int* vlabel, int* flabel, int* vkey, int* fkey, int* status,
                       void* stream) {
  if (!cc_sizes(B, V, T) || !voff || !toff || !flags || !coff || !status) return SFMI_EINVAL;
  if ((V > 0 && (!root || !ref || !rank || !vlabel || !vkey)) || (T > 0 && (!faces || !flabel || !fkey))) return SFMI_EINVAL;
  hipLaunchKernelGGL(cc_number_kernel, dim3(blocks256((long long)V + T + B)), dim3(256), 0, (hipStream_t)stream, faces, voff, toff, flags, root, ref,
                     rank, coff, B, V, T, vlabel, flabel, vkey, fkey, status);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_cc_stats_f64(const float* verts, const int* faces, const int* voff, const int* toff, const int* forder, const int* seg,
                      const int* choff, int B, int V, int T, int nC, int nW, double* part, double* area, double* volume, void* stream) {
  if (!cc_sizes(B, V, T) || nC < 1 || nW < 0 || !voff || !toff || !seg || !choff || !area || !volume) return SFMI_EINVAL;
  if ((T > 0 && (!verts || !faces || !forder)) || (nW > 0 && !part)) return SFMI_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (nW > 0 && T > 0)
    hipLaunchKernelGGL(cc_partial_kernel, dim3((unsigned)((nW + 3) / 4)), dim3(256), 0, st, verts, faces, voff, toff, forder, seg, choff, B, T, nC,
                       nW, part);
  hipLaunchKernelGGL(cc_total_kernel, dim3((unsigned)((nC + 3) / 4)), dim3(256), 0, st, part, choff, nC, (T > 0 ? nW : 0), area, volume);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_cc_mark_i32(const int* vlabel, const int* flabel, const int* voff, const int* toff, const int* coff, const unsigned char* keep,
                     int B, int V, int T, int nC, unsigned char* vkeep, unsigned char* fkeep, void* stream) {
  if (!cc_sizes(B, V, T) || nC < 1 || !voff || !toff || !coff || !keep || (V > 0 && (!vlabel || !vkeep)) || (T > 0 && (!flabel || !fkeep)))
    return SFMI_EINVAL;
  if (V + T == 0) return SFMI_OK;
  hipLaunchKernelGGL(cc_mark_kernel, dim3(blocks256((long long)V + T)), dim3(256), 0, (hipStream_t)stream, vlabel, flabel, voff, toff, coff, keep, B,
                     V, T, nC, vkeep, fkeep);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_cc_emit_f32(const float* verts, const int* faces, const int* voff, const int* toff, const unsigned char* vkeep,
                     const unsigned char* fkeep, const int* vincl, const int* fincl, const int* nvoff, int B, int V, int T, int nVo, int nTo,
                     float* out_v, int* out_f, void* stream) {
  if (!cc_sizes(B, V, T) || nVo < 0 || nTo < 0 || nVo > V || nTo > T || !voff || !toff || !nvoff) return SFMI_EINVAL;
  if ((V > 0 && (!verts || !vkeep || !vincl)) || (T > 0 && (!faces || !fkeep || !fincl)) || (nVo > 0 && !out_v) || (nTo > 0 && !out_f))
    return SFMI_EINVAL;
  if (nVo + nTo == 0) return SFMI_OK;
  hipLaunchKernelGGL(cc_emit_kernel, dim3(blocks256((long long)V + T)), dim3(256), 0, (hipStream_t)stream, verts, faces, voff, toff, vkeep, fkeep,
                     vincl, fincl, nvoff, B, V, T, nVo, nTo, out_v, out_f);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

}  // extern "C"
