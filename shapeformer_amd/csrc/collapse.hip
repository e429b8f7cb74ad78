// Edge-collapse mesh decimation on the device: rounds of independent quadric edge collapses on the ragged indexed
// meshes of csrc/mcubes.hip / csrc/iso_sparse.hip, to an exact face budget.  The reference decimates on the host, xgutils/geoutil.py:175-233
// (array2mesh(..., if_decimate, decimate_face) -> igl.decimate, an edge collapse); csrc/simplify.hip keeps its interface by vertex
// clustering, this file is the edge collapse itself, stated as a pure function of (verts, faces, target, reg).  The contract is in
// include/sfmi.h, its plain Python statement in tests/collapse_ref.py.
//
// A round is rebuilt from the alive faces, so nothing incremental can drift:
//   records   face -> three half-edge keys lo << 32 | hi (batch-wide vertex indices) and three corner keys (the vertex); faces that are
//             dead, of a finished shape or with a repeated index sort behind everything (the last kind freezes its vertices)
//             [the host sorts both: the edge table is the runs of the sorted half-edges, the vertex -> face CSR the runs of the corners]
//   runs      sorted half-edge record -> the length of the run it starts (an edge's face count); a count other than 2 freezes both ends
//   quadrics  (once) vertex -> the planes of its faces added in ascending face index
//   eval      one thread per edge of count 2 between unfrozen vertices: the quadric solve, the cost, the three validity rules by
//             walking the two CSR ranges, then the 64-bit atomicMin of its key onto every face of its region
//   win       an edge whose region holds its own key everywhere is a winner; winners per shape are counted
//             [the host sorts the winners' keys, by shape when there is more than one: the budget takes the first `allowed`]
//   apply     one thread per collapsing edge: the regions of a round's winners are disjoint, so the threads share no face, no vertex
//             that they write and no quadric
//   status    one thread per shape: alive faces, rounds, the stop rules, the next round's budget
// Integer atomics only (atomicMin on 64-bit keys, atomicAdd / atomicOr on counters); all floating-point work is f64 in a fixed order
// inside one thread.  No kernel keeps a per-lane array: the one-rings are walked through the CSR ranges.
#include "sfmi_ragged.h"   // the ragged-batch helpers the mesh tools share: DESIGN.md §5.5a
#include "sfmi_quadric.h"  // the 3x3 Cholesky solve, shared with csrc/simplify.hip

// every expression below is restated operation for operation in tests/collapse_ref.py: no contraction into fused multiply-adds
#pragma clang fp contract(off)

namespace {

constexpr unsigned long long COL_NONE = 0xFFFFFFFFFFFFFFFFull;   // no key: a face nobody marked, an edge that is no valid candidate
constexpr long long COL_LAST = 0x7FFFFFFFFFFFFFFFll;             // the sort key of a record that is none: behind every real one
constexpr int COL_STALLED = 4, COL_CAPPED = 5;

struct ColState {
  int* gf;                   // (3T) the faces with batch-wide vertex indices, rewritten by the collapses
  int* fshape;               // (T) the shape of every face
  unsigned char* alive;      // (T)
  float* pos;                // (3V) the current positions
  double* Q;                 // (10V) a00 a01 a02 a11 a12 a22 b0 b1 b2 c
  unsigned char* removed;    // (V) the vertex was collapsed into another
  unsigned char* frozen;     // (V) this round: on an edge whose count is not 2, or on a face with a repeated index
  unsigned long long* fkey;  // (T) this round: the smallest key of the candidates whose region holds the face
  int *flags, *status, *nalive, *allowed, *nwin, *active, *rounds;   // (B) each
  int* nactive;              // (1) shapes that go on
};

void col_layout(SfmiCarver& c, ColState& s, int B, int V, int T) {
  s.gf = c.take<int>(3 * (size_t)T);
  s.fshape = c.take<int>(T);
  s.alive = c.take<unsigned char>(T);
  s.pos = c.take<float>(3 * (size_t)V);
  s.Q = c.take<double>(10 * (size_t)V);
  s.removed = c.take<unsigned char>(V);
  s.frozen = c.take<unsigned char>(V);
  s.fkey = c.take<unsigned long long>(T);
  s.flags = c.take<int>(B);
  s.status = c.take<int>(B);
  s.nalive = c.take<int>(B);
  s.allowed = c.take<int>(B);
  s.nwin = c.take<int>(B);
  s.active = c.take<int>(B);
  s.rounds = c.take<int>(B);
  s.nactive = c.take<int>(1);
}

bool col_sizes(int B, int V, int T) { return B > 0 && V >= 0 && T >= 0 && (long long)V + T + B < (1ll << 31) && 9ll * T < (1ll << 31); }

ColState col_state(void* workspace, int B, int V, int T) {
  SfmiCarver c{(char*)workspace};
  ColState s;
  col_layout(c, s, B, V, T);
  return s;
}

// one atomicAdd per wave where the wave's items are of one shape (the common case), else one per item; every lane of the wave calls
__device__ __forceinline__ void col_count(int* __restrict__ slot, int b, bool pred) {
  const int b0 = __shfl(b, 0, 64);
  const unsigned long long same = __ballot(pred && b == b0);
  if ((threadIdx.x & 63) == 0 && same) atomicAdd(&slot[b0], __popcll(same));
  if (pred && b != b0) atomicAdd(&slot[b], 1);
}

__device__ __forceinline__ bool col_has(int a, int b, int c, int w) { return a == w || b == w || c == w; }

// threads [0,V): vertices; [V,V+T): faces; [V+T,V+T+B): shapes.  flags was cleared
__global__ __launch_bounds__(256) void col_validate_kernel(const float* __restrict__ verts, const int* __restrict__ faces,
                                                           const int* __restrict__ voff, const int* __restrict__ toff, int B, int V, int T,
                                                           ColState s) {
  const long long t = blockIdx.x * 256ll + threadIdx.x;
  if (t < V) {
    const int i = (int)t;
    if (!sfmi_finite3(verts + 3ll * i)) atomicOr(&s.flags[sfmi_owner(voff, B, i)], SFMI_MESH_NON_FINITE);
  } else if (t < (long long)V + T) {
    const int j = (int)(t - V), b = sfmi_owner(toff, B, j);
    const int nv = voff[b + 1] - voff[b];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int a = faces[3ll * j + k];
      ok = ok && a >= 0 && a < nv;
    }
    if (!ok) atomicOr(&s.flags[b], SFMI_MESH_BAD_INDEX);
  } else if (t < (long long)V + T + B) {
    const int b = (int)(t - V - T);
    if (voff[b + 1] <= voff[b]) atomicOr(&s.flags[b], SFMI_MESH_NO_VERTS);
  }
}

__global__ __launch_bounds__(256) void col_setup_kernel(const float* __restrict__ verts, const int* __restrict__ faces,
                                                        const int* __restrict__ voff, const int* __restrict__ toff, int B, int V, int T,
                                                        int target, int max_rounds, ColState s) {
  const long long t = blockIdx.x * 256ll + threadIdx.x;
  if (t < V) {
    const int i = (int)t;
#pragma unroll
    for (int k = 0; k < 3; ++k) s.pos[3ll * i + k] = verts[3ll * i + k];
    s.removed[i] = 0;
  } else if (t < (long long)V + T) {
    const int j = (int)(t - V), b = sfmi_owner(toff, B, j);
    const bool ok = !s.flags[b];           // the indices of an unflagged shape are all inside it
    s.fshape[j] = b;
    s.alive[j] = ok ? 1 : 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) s.gf[3ll * j + k] = ok ? voff[b] + faces[3ll * j + k] : 0;
  } else if (t < (long long)V + T + B) {
    const int b = (int)(t - V - T), fl = s.flags[b];
    const int n = fl ? 0 : toff[b + 1] - toff[b];
    const bool go = !fl && n > target && max_rounds > 0;
    s.status[b] = fl ? sfmi_mesh_status(fl) : (n > target && max_rounds <= 0 ? COL_CAPPED : 0);
    s.nalive[b] = n;
    s.allowed[b] = go ? (n - target + 1) / 2 : 0;
    s.nwin[b] = 0;
    s.rounds[b] = 0;
    s.active[b] = go ? 1 : 0;
    if (go) atomicAdd(s.nactive, 1);
  }
}

__global__ __launch_bounds__(256) void col_records_kernel(int V, int T, ColState s, long long* __restrict__ ekey, int* __restrict__ ckey) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= T) return;
  long long e[3] = {COL_LAST, COL_LAST, COL_LAST};
  int c[3] = {V, V, V};
  if (s.alive[j] && s.active[s.fshape[j]]) {
    const int a0 = s.gf[3ll * j], a1 = s.gf[3ll * j + 1], a2 = s.gf[3ll * j + 2];
    if (a0 == a1 || a1 == a2 || a0 == a2) {
      s.frozen[a0] = 1; s.frozen[a1] = 1; s.frozen[a2] = 1;      // plain stores of the same value from any number of threads
    } else {
      e[0] = ((long long)min(a0, a1) << 32) | (unsigned)max(a0, a1);
      e[1] = ((long long)min(a1, a2) << 32) | (unsigned)max(a1, a2);
      e[2] = ((long long)min(a2, a0) << 32) | (unsigned)max(a2, a0);
      c[0] = a0; c[1] = a1; c[2] = a2;
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    ekey[3ll * j + k] = e[k];
    ckey[3ll * j + k] = c[k];
  }
}

// skey: the sorted half-edge keys.  ecnt[i] = the length of the run that starts at i, 0 where none does
__global__ __launch_bounds__(256) void col_runs_kernel(const long long* __restrict__ skey, int n, ColState s, int* __restrict__ ecnt) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long long key = skey[i];
  int cnt = 0;
  if (key != COL_LAST && (i == 0 || skey[i - 1] != key)) {
    cnt = 1;
    while (i + cnt < n && skey[i + cnt] == key) ++cnt;
    if (cnt != 2) {
      s.frozen[(int)(key >> 32)] = 1;
      s.frozen[(int)(key & 0xFFFFFFFFll)] = 1;
    }
  }
  ecnt[i] = cnt;
}

// the plane of face (p0, p1, p2) added to q: n = (p1 - p0) x (p2 - p0), d = -n.p0
__device__ __forceinline__ void col_normal(const float* __restrict__ q0, const float* __restrict__ q1, const float* __restrict__ q2,
                                           double& n0, double& n1, double& n2) {
  const double e10 = (double)q1[0] - (double)q0[0], e11 = (double)q1[1] - (double)q0[1], e12 = (double)q1[2] - (double)q0[2];
  const double e20 = (double)q2[0] - (double)q0[0], e21 = (double)q2[1] - (double)q0[1], e22 = (double)q2[2] - (double)q0[2];
  n0 = e11 * e22 - e12 * e21;
  n1 = e12 * e20 - e10 * e22;
  n2 = e10 * e21 - e11 * e20;
}

// corder / cseg: the corner records 3 f + k stably sorted by vertex and where each vertex's run starts: its faces, ascending
__global__ __launch_bounds__(256) void col_quadrics_kernel(const int* __restrict__ corder, const int* __restrict__ cseg, int V, ColState s) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= V) return;
  double a00 = 0, a01 = 0, a02 = 0, a11 = 0, a12 = 0, a22 = 0, b0 = 0, b1 = 0, b2 = 0, c = 0;
  for (int i = cseg[v], e = cseg[v + 1]; i < e; ++i) {
    const int* f = s.gf + 3ll * (corder[i] / 3);
    const float* q0 = s.pos + 3ll * f[0];
    double n0, n1, n2;
    col_normal(q0, s.pos + 3ll * f[1], s.pos + 3ll * f[2], n0, n1, n2);
    const double d = -((n0 * (double)q0[0] + n1 * (double)q0[1]) + n2 * (double)q0[2]);
    a00 += n0 * n0; a01 += n0 * n1; a02 += n0 * n2; a11 += n1 * n1; a12 += n1 * n2; a22 += n2 * n2;
    b0 += d * n0; b1 += d * n1; b2 += d * n2;
    c += d * d;
  }
  double* q = s.Q + 10ll * v;
  q[0] = a00; q[1] = a01; q[2] = a02; q[3] = a11; q[4] = a12; q[5] = a22; q[6] = b0; q[7] = b1; q[8] = b2; q[9] = c;
}

// the r-th face of the region of (u, v): u's faces, then v's (a face of both comes up twice; callers skip it or do not mind)
struct ColRing {
  const int* corder;
  int u0, du, v0, n;
  __device__ __forceinline__ ColRing(const int* __restrict__ co, const int* __restrict__ cseg, int u, int v)
      : corder(co), u0(cseg[u]), du(cseg[u + 1] - cseg[u]), v0(cseg[v]), n(cseg[u + 1] - cseg[u] + cseg[v + 1] - cseg[v]) {}
  __device__ __forceinline__ int face(int r) const { return (r < du ? corder[u0 + r] : corder[v0 + (r - du)]) / 3; }
};

__global__ __launch_bounds__(256) void col_eval_kernel(const long long* __restrict__ skey, const int* __restrict__ ecnt,
                                                       const int* __restrict__ erank, const int* __restrict__ corder,
                                                       const int* __restrict__ cseg, int n, double reg, ColState s,
                                                       unsigned long long* __restrict__ cand, float* __restrict__ xs) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  cand[i] = COL_NONE;
  if (ecnt[i] != 2) return;
  const long long ek = skey[i];
  const int u = (int)(ek >> 32), v = (int)(ek & 0xFFFFFFFFll);
  if (s.frozen[u] || s.frozen[v]) return;
  const double *qu = s.Q + 10ll * u, *qv = s.Q + 10ll * v;
  const double a00 = qu[0] + qv[0], a01 = qu[1] + qv[1], a02 = qu[2] + qv[2], a11 = qu[3] + qv[3], a12 = qu[4] + qv[4],
               a22 = qu[5] + qv[5], b0 = qu[6] + qv[6], b1 = qu[7] + qv[7], b2 = qu[8] + qv[8], c = qu[9] + qv[9];
  const float *pu = s.pos + 3ll * u, *pv = s.pos + 3ll * v;
  const double m[3] = {((double)pu[0] + (double)pv[0]) / 2.0, ((double)pu[1] + (double)pv[1]) / 2.0, ((double)pu[2] + (double)pv[2]) / 2.0};
  double x[3] = {m[0], m[1], m[2]};
  const double tr = a00 + a11 + a22;
  bool ok = true;
  if (tr > 0.0) ok = sfmi_quadric_solve(a00, a01, a02, a11, a12, a22, b0, b1, b2, reg * tr, m, x);
  if (!ok || !sfmi_finite3(x[0], x[1], x[2])) return;
  const float x32[3] = {(float)x[0], (float)x[1], (float)x[2]};
  const double x0 = x32[0], x1 = x32[1], x2 = x32[2];
  const double t0 = (a00 * x0 + a01 * x1) + a02 * x2;
  const double t1 = (a01 * x0 + a11 * x1) + a12 * x2;
  const double t2 = (a02 * x0 + a12 * x1) + a22 * x2;
  const double xax = (x0 * t0 + x1 * t1) + x2 * t2;
  const double bx = (b0 * x0 + b1 * x1) + b2 * x2;
  double cost = (xax + 2.0 * bx) + c;
  if (!isfinite(cost)) return;
  cost = cost > 0.0 ? cost : 0.0;
  const ColRing ring(corder, cseg, u, v);
  // (a) exactly two common neighbours: every edge at u lies in two faces, so each one is met twice among u's faces
  int pairs = 0;
  for (int r = 0; r < ring.du; ++r) {
    const int* f = s.gf + 3ll * ring.face(r);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int w = f[k];
      if (w == u || w == v) continue;
      bool adj = false;
      for (int q = ring.du; q < ring.n && !adj; ++q) {
        const int* g = s.gf + 3ll * ring.face(q);
        adj = col_has(g[0], g[1], g[2], w);
      }
      pairs += adj ? 1 : 0;
    }
  }
  if (pairs != 4) return;
  for (int r = 0; r < ring.n; ++r) {
    const int* f = s.gf + 3ll * ring.face(r);
    const int f0 = f[0], f1 = f[1], f2 = f[2];
    if (col_has(f0, f1, f2, u) && col_has(f0, f1, f2, v)) continue;      // one of the edge's two faces
    // (c) the face keeps its side when its corner at u or v moves to x32
    double o0, o1, o2, n0, n1, n2;
    col_normal(s.pos + 3ll * f0, s.pos + 3ll * f1, s.pos + 3ll * f2, o0, o1, o2);
    col_normal((f0 == u || f0 == v) ? x32 : s.pos + 3ll * f0, (f1 == u || f1 == v) ? x32 : s.pos + 3ll * f1,
               (f2 == u || f2 == v) ? x32 : s.pos + 3ll * f2, n0, n1, n2);
    if (!((o0 * n0 + o1 * n1) + o2 * n2 > 0.0)) return;
    // (b) with v renamed u no later face of the region has the same three vertices
    const int g0 = f0 == v ? u : f0, g1 = f1 == v ? u : f1, g2 = f2 == v ? u : f2;
    for (int q = r + 1; q < ring.n; ++q) {
      const int* h = s.gf + 3ll * ring.face(q);
      int h0 = h[0], h1 = h[1], h2 = h[2];
      if (col_has(h0, h1, h2, u) && col_has(h0, h1, h2, v)) continue;
      h0 = h0 == v ? u : h0; h1 = h1 == v ? u : h1; h2 = h2 == v ? u : h2;
      if (col_has(h0, h1, h2, g0) && col_has(h0, h1, h2, g1) && col_has(h0, h1, h2, g2)) return;
    }
  }
  const unsigned long long key = ((unsigned long long)__float_as_uint((float)cost) << 32) | (unsigned)erank[i];
  cand[i] = key;
#pragma unroll
  for (int k = 0; k < 3; ++k) xs[3ll * i + k] = x32[k];
  for (int r = 0; r < ring.n; ++r) {
    unsigned long long* slot = s.fkey + ring.face(r);
    if (key < __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(slot, key);
  }
}

__global__ __launch_bounds__(256) void col_win_kernel(const long long* __restrict__ skey, const long long* __restrict__ sidx,
                                                      const unsigned long long* __restrict__ cand, const int* __restrict__ corder,
                                                      const int* __restrict__ cseg, int n, int B, ColState s, long long* __restrict__ wkey,
                                                      int* __restrict__ wshape) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  bool win = false;
  int b = B;
  if (i < n) {
    const unsigned long long key = cand[i];
    if (key != COL_NONE) {
      const long long ek = skey[i];
      const ColRing ring(corder, cseg, (int)(ek >> 32), (int)(ek & 0xFFFFFFFFll));
      win = true;
      for (int r = 0; r < ring.n; ++r) win = win && s.fkey[ring.face(r)] == key;
      if (win) b = s.fshape[(int)(sidx[i] / 3)];
    }
    wkey[i] = win ? (long long)key : COL_LAST;         // a cost is not negative: the key's top bit is clear
    wshape[i] = b;
  }
  col_count(s.nwin, b, win);
}

// order: the sorted half-edge records of the winners by (shape, key); sshape: their shapes in that order (B behind the last winner);
// sstart (B): where each shape's winners start
__global__ __launch_bounds__(256) void col_apply_kernel(const long long* __restrict__ skey, const long long* __restrict__ order,
                                                        const int* __restrict__ sshape, const int* __restrict__ sstart,
                                                        const float* __restrict__ xs, const int* __restrict__ corder,
                                                        const int* __restrict__ cseg, int n, int B, ColState s) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const int b = sshape[p];
  if (b < 0 || b >= B || p - sstart[b] >= s.allowed[b]) return;
  const long long i = order[p];
  if (i < 0 || i >= n) return;
  const long long ek = skey[i];
  const int u = (int)(ek >> 32), v = (int)(ek & 0xFFFFFFFFll);     // u < v: u stays
#pragma unroll
  for (int k = 0; k < 3; ++k) s.pos[3ll * u + k] = xs[3ll * i + k];
  for (int r = cseg[v], e = cseg[v + 1]; r < e; ++r) {
    const int f = corder[r] / 3;
    int* g = s.gf + 3ll * f;
    if (col_has(g[0], g[1], g[2], u)) {
      s.alive[f] = 0;
    } else {
#pragma unroll
      for (int k = 0; k < 3; ++k)
        if (g[k] == v) g[k] = u;
    }
  }
  double *qu = s.Q + 10ll * u, *qv = s.Q + 10ll * v;
#pragma unroll
  for (int k = 0; k < 10; ++k) qu[k] = qu[k] + qv[k];
  s.removed[v] = 1;
}

// nactive was cleared
__global__ __launch_bounds__(256) void col_status_kernel(int B, int target, int max_rounds, ColState s) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B || !s.active[b]) return;
  const int w = s.nwin[b];
  s.nwin[b] = 0;
  bool go = false;
  if (w == 0) {
    s.status[b] = COL_STALLED;
  } else {
    const int left = s.nalive[b] - 2 * min(w, s.allowed[b]), r = s.rounds[b] + 1;
    s.nalive[b] = left;
    s.rounds[b] = r;
    s.allowed[b] = (left - target + 1) / 2;
    if (left > target) {
      go = r < max_rounds;
      if (!go) s.status[b] = COL_CAPPED;
    }
  }
  s.active[b] = go ? 1 : 0;
  if (go) atomicAdd(s.nactive, 1);
}

__global__ __launch_bounds__(256) void col_finish_kernel(const int* __restrict__ voff, int B, int V, int T, ColState s,
                                                         float* __restrict__ out_v, int* __restrict__ out_f,
                                                         unsigned char* __restrict__ vkeep, unsigned char* __restrict__ fkeep) {
  const long long t = blockIdx.x * 256ll + threadIdx.x;
  if (t < V) {
    const int i = (int)t;
#pragma unroll
    for (int k = 0; k < 3; ++k) out_v[3ll * i + k] = s.pos[3ll * i + k];
    vkeep[i] = (!s.removed[i] && !s.flags[sfmi_owner(voff, B, i)]) ? 1 : 0;
  } else if (t < (long long)V + T) {
    const int j = (int)(t - V), vb = voff[s.fshape[j]];
    const bool keep = s.alive[j];
#pragma unroll
    for (int k = 0; k < 3; ++k) out_f[3ll * j + k] = keep ? s.gf[3ll * j + k] - vb : 0;
    fkeep[j] = keep ? 1 : 0;
  }
}

// threads [0,n): the sorted half-edge records, n = 3T; [n,n+T): faces.  counts (B,3): edges, boundary edges, non-manifold edges
__global__ __launch_bounds__(256) void col_topology_kernel(const long long* __restrict__ skey, const long long* __restrict__ sidx,
                                                           const int* __restrict__ ecnt, int n, int B, int T, ColState s,
                                                           unsigned char* __restrict__ ref, int* __restrict__ counts) {
  const long long t = blockIdx.x * 256ll + threadIdx.x;
  int b = B, cnt = 0;
  if (t < n) {
    cnt = ecnt[t];
    if (cnt > 0) b = s.fshape[(int)(sidx[t] / 3)];
  } else if (t < (long long)n + T) {
    const int j = (int)(t - n);
    if (s.alive[j]) {
#pragma unroll
      for (int k = 0; k < 3; ++k) ref[s.gf[3ll * j + k]] = 1;
    }
  }
  col_count(counts, b, cnt > 0);
  col_count(counts + B, b, cnt == 1);
  col_count(counts + 2 * B, b, cnt > 2);
}

}  // namespace

extern "C" {

size_t sfmi_collapse_workspace_bytes(int B, int V, int T) {
  if (!col_sizes(B, V, T)) return 0;
  ColState s;
  return sfmi_ws_bytes([](SfmiCarver& c, ColState* st, int b, int v, int t) { col_layout(c, *st, b, v, t); }, &s, B, V, T);
}

int sfmi_collapse_init_f32(const float* verts, const int* faces, const int* voff, const int* toff, int B, int V, int T, int target,
                           int max_rounds, void* workspace, void* stream) {
  if (!col_sizes(B, V, T) || target < 0 || !voff || !toff || !workspace || (V > 0 && !verts) || (T > 0 && !faces)) return SFMI_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const ColState s = col_state(workspace, B, V, T);
  SFMI_TRY(hipMemsetAsync(s.flags, 0, (size_t)B * 4, st));
  SFMI_TRY(hipMemsetAsync(s.nactive, 0, 4, st));
  const unsigned g = blocks256((long long)V + T + B);
  hipLaunchKernelGGL(col_validate_kernel, dim3(g), dim3(256), 0, st, verts, faces, voff, toff, B, V, T, s);
  hipLaunchKernelGGL(col_setup_kernel, dim3(g), dim3(256), 0, st, verts, faces, voff, toff, B, V, T, target, max_rounds, s);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_collapse_records_i32(int B, int V, int T, long long* ekey, int* ckey, void* workspace, void* stream) {
  if (!col_sizes(B, V, T) || !workspace || (T > 0 && (!ekey || !ckey))) return SFMI_EINVAL;
  if (T == 0) return SFMI_OK;
  hipStream_t st = (hipStream_t)stream;
  const ColState s = col_state(workspace, B, V, T);
  if (V > 0) SFMI_TRY(hipMemsetAsync(s.frozen, 0, (size_t)V, st));
  SFMI_TRY(hipMemsetAsync(s.fkey, 0xFF, (size_t)T * 8, st));
  hipLaunchKernelGGL(col_records_kernel, dim3(blocks256(T)), dim3(256), 0, st, V, T, s, ekey, ckey);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_collapse_runs_i32(const long long* skey, int B, int V, int T, int* ecnt, void* workspace, void* stream) {
  if (!col_sizes(B, V, T) || !workspace || (T > 0 && (!skey || !ecnt))) return SFMI_EINVAL;
  if (T == 0) return SFMI_OK;
  hipLaunchKernelGGL(col_runs_kernel, dim3(blocks256(3ll * T)), dim3(256), 0, (hipStream_t)stream, skey, 3 * T, col_state(workspace, B, V, T), ecnt);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_collapse_quadrics_f64(const int* corder, const int* cseg, int B, int V, int T, void* workspace, void* stream) {
  if (!col_sizes(B, V, T) || !workspace || !cseg || (T > 0 && !corder)) return SFMI_EINVAL;
  if (V == 0) return SFMI_OK;
  hipLaunchKernelGGL(col_quadrics_kernel, dim3(blocks256(V)), dim3(256), 0, (hipStream_t)stream, corder, cseg, V, col_state(workspace, B, V, T));
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_collapse_eval_f64(const long long* skey, const int* ecnt, const int* erank, const int* corder, const int* cseg, int B, int V, int T,
                           double reg, unsigned long long* cand, float* xs, void* workspace, void* stream) {
  if (!col_sizes(B, V, T) || !(reg > 0.0) || !std::isfinite(reg) || !workspace || !cseg) return SFMI_EINVAL;
  if (T > 0 && (!skey || !ecnt || !erank || !corder || !cand || !xs)) return SFMI_EINVAL;
  if (T == 0) return SFMI_OK;
  hipLaunchKernelGGL(col_eval_kernel, dim3(blocks256(3ll * T)), dim3(256), 0, (hipStream_t)stream, skey, ecnt, erank, corder, cseg, 3 * T, reg,
                     col_state(workspace, B, V, T), cand, xs);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_collapse_win_i32(const long long* skey, const long long* sidx, const unsigned long long* cand, const int* corder, const int* cseg,
                          int B, int V, int T, long long* wkey, int* wshape, void* workspace, void* stream) {
  if (!col_sizes(B, V, T) || !workspace || !cseg || (T > 0 && (!skey || !sidx || !cand || !corder || !wkey || !wshape))) return SFMI_EINVAL;
  if (T == 0) return SFMI_OK;
  hipLaunchKernelGGL(col_win_kernel, dim3(blocks256(3ll * T)), dim3(256), 0, (hipStream_t)stream, skey, sidx, cand, corder, cseg, 3 * T, B,
                     col_state(workspace, B, V, T), wkey, wshape);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_collapse_apply_f32(const long long* skey, const long long* order, const int* sshape, const int* sstart, const float* xs,
                            const int* corder, const int* cseg, int B, int V, int T, int target, int max_rounds, void* workspace,
                            void* stream) {
  if (!col_sizes(B, V, T) || target < 0 || !workspace || !cseg || !sstart) return SFMI_EINVAL;
  if (T > 0 && (!skey || !order || !sshape || !xs || !corder)) return SFMI_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const ColState s = col_state(workspace, B, V, T);
  if (T > 0)
    hipLaunchKernelGGL(col_apply_kernel, dim3(blocks256(3ll * T)), dim3(256), 0, st, skey, order, sshape, sstart, xs, corder, cseg, 3 * T, B, s);
  SFMI_TRY(hipMemsetAsync(s.nactive, 0, 4, st));
  hipLaunchKernelGGL(col_status_kernel, dim3(blocks256(B)), dim3(256), 0, st, B, target, max_rounds, s);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_collapse_report_i32(int B, int V, int T, const void* workspace, int* status, int* rounds, int* nalive, int* nactive, void* stream) {
  if (!col_sizes(B, V, T) || !workspace) return SFMI_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const ColState s = col_state((void*)workspace, B, V, T);
  if (status) SFMI_TRY(hipMemcpyAsync(status, s.status, (size_t)B * 4, hipMemcpyDeviceToDevice, st));
  if (rounds) SFMI_TRY(hipMemcpyAsync(rounds, s.rounds, (size_t)B * 4, hipMemcpyDeviceToDevice, st));
  if (nalive) SFMI_TRY(hipMemcpyAsync(nalive, s.nalive, (size_t)B * 4, hipMemcpyDeviceToDevice, st));
  if (nactive) SFMI_TRY(hipMemcpyAsync(nactive, s.nactive, 4, hipMemcpyDeviceToDevice, st));
  return SFMI_OK;
}

int sfmi_collapse_finish_f32(const int* voff, int B, int V, int T, const void* workspace, float* out_v, int* out_f, unsigned char* vkeep,
                             unsigned char* fkeep, void* stream) {
  if (!col_sizes(B, V, T) || !workspace || !voff || (V > 0 && (!out_v || !vkeep)) || (T > 0 && (!out_f || !fkeep))) return SFMI_EINVAL;
  if (V + T == 0) return SFMI_OK;
  hipLaunchKernelGGL(col_finish_kernel, dim3(blocks256((long long)V + T)), dim3(256), 0, (hipStream_t)stream, voff, B, V, T,
                     col_state((void*)workspace, B, V, T), out_v, out_f, vkeep, fkeep);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_collapse_topology_i32(const long long* skey, const long long* sidx, const int* ecnt, int B, int V, int T, const void* workspace,
                               unsigned char* ref, int* counts, void* stream) {
  if (!col_sizes(B, V, T) || !workspace || !counts || (V > 0 && !ref) || (T > 0 && (!skey || !sidx || !ecnt))) return SFMI_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (V > 0) SFMI_TRY(hipMemsetAsync(ref, 0, (size_t)V, st));
  SFMI_TRY(hipMemsetAsync(counts, 0, (size_t)B * 12, st));
  if (T > 0)
    hipLaunchKernelGGL(col_topology_kernel, dim3(blocks256(4ll * T)), dim3(256), 0, st, skey, sidx, ecnt, 3 * T, B, T,
                       col_state((void*)workspace, B, V, T), ref, counts);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

}  // extern "C"
