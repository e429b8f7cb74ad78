// Poisson surface reconstruction of oriented point clouds on a uniform lattice.  The device counterpart of the reference's
// Open3D_Toolbox.poisson_recon / Meshlab_Toolbox.poisson_recon (xgutils/geoutil.py:297-342): the interface of that call, not Open3D's
// octree output.  DESIGN.md §5.16; the numpy statement of the contract is tests/poisson_ref.py.
//
// Lattice: R nodes per axis over a box [lo, hi], spacing h = (hi - lo) / (R - 1), tensor axes 0,1,2 = x,y,z (marching_cubes_dev's).
// The lattice coordinate of a point is t = (double(x) - lo) / h per axis, clamped to [0, R - 1]; a point is inside when lo <= x <= hi
// on every axis (compared in f64).  hat(d) = max(0, 1 - |d|) is the trilinear weight of a site at distance d (in cells).
//
// 1. poisson_key_kernel: the cell of every point, key = ((set * C + cx) * C + cy) * C + cz with C = R - 1 cells per axis and
//    c = min(floor(t), C - 1); a point outside the box is counted per set (an integer atomic: exact in any order) and gets the key
//    B * C^3, behind every cell; a non-finite coordinate or normal sets status bit 1.  The host sorts the keys (stable);
//    poisson_cells_kernel marks where each cell's run begins (cell_start, B * C^3 + 1 entries: a lower bound per cell).
// 2. poisson_splat_kernel: a GATHER, one lane per lattice node (b, i, j, k).  The lane walks the 27 cells around its node in ascending
//    cell order and each cell's points in ascending input order (the sort is stable) and keeps four f64 sums:
//      W [i,j,k]        += hat(tx - i)       hat(ty - j)       hat(tz - k)
//      Vx[i,j,k]        += nx hat(tx - i - ½) hat(ty - j)       hat(tz - k)          the site ((i + ½), j, k), i < R - 1
//      Vy, Vz likewise on their own staggered sites.
//    A point that is too far from a site adds a zero.  Each sum is rounded to f32 once.  No float atomics: the order of every sum
//    is a function of the set alone, so the result is bit-identical from run to run and in any batch.
// 3. poisson_rhs_kernel: b = -G^T V, G the forward difference from nodes to edges with the lattice surrounded by zeros:
//    b[i,j,k] = (Vx[i] - Vx[i-1]) + (Vy[j] - Vy[j-1]) + (Vz[k] - Vz[k-1]) in f64 in this order, sites outside the arrays zero.
// 4. Conjugate gradients on A = G^T G (7 points, 6 on every diagonal entry, the faces included; SPD), from x0 = 0.  x, r, p, q are
//    f32 lattices; dot products are f64 over a fixed tree: per-workgroup partials (lane sums in a fixed stride, wave_sum_f64, four
//    waves in order), finished by EVERY workgroup of the next launch for itself (the same sum in the same order everywhere), so
//    the kernel boundary is the only grid-wide barrier: no cooperative launch, no counter, nothing waits on another workgroup.
//    Per iteration three launches:
//      cg_apply_kernel      q = A p                      + partials of <p, q>
//      cg_update_kernel     alpha = rr / <p, q>;  x += alpha p;  r -= alpha q     + partials of <r, r>
//      cg_direction_kernel  beta = rr' / rr;  p = r + beta p;  workgroup 0 of each shape writes the NEXT state (rr', iteration, done)
//    The per-shape state is double-buffered by the parity of the global iteration index: a launch reads one copy and writes the other.
//    A shape is frozen at the first iteration with rr' <= tol^2 bb (and from the start when b = 0): alpha = beta = 0 from then on, its
//    counter stops, x and r no longer change.  Nothing is read back inside sfmi_poisson_cg_steps_f32.
//    cg_apply_kernel marches along axis 0: a workgroup owns a 16 x 64 (j, k) tile for TI planes, lanes along k (the contiguous axis),
//    four j per lane.  The planes i - 1 and i + 1 of a lane's own columns live in its registers; the in-plane neighbours come from
//    an LDS image of plane i with a one-node halo (18 x 66 floats, double-buffered: one barrier per plane).  Each p value is read
//    once per workgroup that owns it, plus the halo (2/16 + 2/64 of a plane, an L2 hit: the neighbour tile reads it as its own).
// 5. poisson_iso_kernel: iso[b] = the mean of the trilinear chi over the set's in-box points, f64: 1024 lanes, each sums a contiguous
//    chunk of the set in input order, then a fixed tree; poisson_sub_kernel: field = float(double(chi) - iso[b]).
// 6. poisson_sample_kernel: the trilinear sample of a lattice at points (f64 weights, rounded to f32 once): the vertex densities.
#include "sfmi_ragged.h"   // the ragged-batch helpers the mesh tools share: DESIGN.md §5.5a
#pragma clang fp contract(off)

namespace {

struct PBox { double lo[3], hi[3], h[3]; };

__device__ __forceinline__ double p_hat(double d) {
  d = 1.0 - fabs(d);
  return d > 0.0 ? d : 0.0;
}

// lattice coordinates of a point, clamped onto the box -> whether the point lies inside the closed box (false for a NaN)
__device__ __forceinline__ bool p_coord(const PBox& bx, int R, const float* __restrict__ p, double t[3]) {
  bool in = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double x = (double)p[a];
    in = in && x >= bx.lo[a] && x <= bx.hi[a];
    const double u = (x - bx.lo[a]) / bx.h[a];
    t[a] = fmin(fmax(u, 0.0), (double)(R - 1));                // fmax(NaN, 0) = 0: a NaN never becomes an index
  }
  return in;
}

// trilinear sample of one shape's lattice L (R^3) at lattice coordinates t in [0, R - 1]: f64, the 8 corners in (dx, dy, dz) order
__device__ __forceinline__ double p_sample(const float* __restrict__ L, int R, const double t[3]) {
  int c[3];
  double f[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    c[a] = min((int)t[a], R - 2);
    f[a] = t[a] - (double)c[a];
  }
  double s = 0.0;
#pragma unroll
  for (int d = 0; d < 8; ++d) {
    const int dx = d >> 2, dy = (d >> 1) & 1, dz = d & 1;
    const double w = ((dx ? f[0] : 1.0 - f[0]) * (dy ? f[1] : 1.0 - f[1])) * (dz ? f[2] : 1.0 - f[2]);
    s += w * (double)L[((long long)(c[0] + dx) * R + (c[1] + dy)) * R + (c[2] + dz)];
  }
  return s;
}

__global__ __launch_bounds__(256) void poisson_key_kernel(const float* __restrict__ P, const float* __restrict__ Nrm,
                                                          const long long* __restrict__ off, int B, long long N, int R, PBox bx,
                                                          long long* __restrict__ keys, int* __restrict__ outside,
                                                          int* __restrict__ status) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int b = sfmi_owner(off, B, i);
  const long long C = R - 1, behind = (long long)B * C * C * C;
  bool finite = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) finite = finite && isfinite(P[3 * i + a]) && isfinite(Nrm[3 * i + a]);
  double t[3];
  const bool in = p_coord(bx, R, P + 3 * i, t);
  if (!finite) {
    atomicOr(status, 1);
    keys[i] = behind;
    return;
  }
  if (!in) {
    atomicAdd(outside + b, 1);
    keys[i] = behind;
    return;
  }
  long long key = b;
#pragma unroll
  for (int a = 0; a < 3; ++a) key = key * C + min((long long)t[a], C - 1);
  keys[i] = key;
}

// one lane per cell (and one for the end): cstart[c] = the number of sorted keys below c = where the run of cell c begins
__global__ __launch_bounds__(256) void poisson_cells_kernel(const long long* __restrict__ sorted, int N, long long ncell,
                                                            int* __restrict__ cstart) {
  const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c > ncell) return;
  int lo = 0, hi = N;                                          // invariant: sorted[< lo] < c <= sorted[>= hi]
  while (lo < hi) {
    const int mid = (int)(((long long)lo + hi) >> 1);
    if (sorted[mid] < c) lo = mid + 1; else hi = mid;
  }
  cstart[c] = lo;
}

// one lane per lattice node; order (N) int64: the points sorted by key (stable); cstart (B C^3 + 1) int32: where each cell's run begins
__global__ __launch_bounds__(256) void poisson_splat_kernel(const float* __restrict__ P, const float* __restrict__ Nrm,
                                                            const long long* __restrict__ order, const int* __restrict__ cstart, int B,
                                                            int R, PBox bx, float* __restrict__ Vx, float* __restrict__ Vy,
                                                            float* __restrict__ Vz, float* __restrict__ W) {
  const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long n3 = (long long)R * R * R;
  if (g >= (long long)B * n3) return;
  const int k = (int)(g % R), j = (int)((g / R) % R), i = (int)((g / ((long long)R * R)) % R);
  const long long b = g / n3;
  const int C = R - 1;
  double sw = 0.0, sx = 0.0, sy = 0.0, sz = 0.0;
  const int k0 = max(k - 1, 0), k1 = min(k + 1, C - 1);
  for (int ci = max(i - 1, 0); ci <= min(i + 1, C - 1); ++ci)
    for (int cj = max(j - 1, 0); cj <= min(j + 1, C - 1); ++cj) {
      const long long base = ((b * C + ci) * C + cj) * C;
      const int beg = cstart[base + k0], end = cstart[base + k1 + 1];      // cells along z are consecutive keys: one ascending run
      for (int rec = beg; rec < end; ++rec) {
        const long long pi = order[rec];
        double t[3];
        p_coord(bx, R, P + 3 * pi, t);
        const double hx = p_hat(t[0] - (double)i), hy = p_hat(t[1] - (double)j), hz = p_hat(t[2] - (double)k);
        const double gx = p_hat(t[0] - ((double)i + 0.5)), gy = p_hat(t[1] - ((double)j + 0.5)), gz = p_hat(t[2] - ((double)k + 0.5));
        sw += (hx * hy) * hz;
        sx += (double)Nrm[3 * pi] * ((gx * hy) * hz);
        sy += (double)Nrm[3 * pi + 1] * ((hx * gy) * hz);
        sz += (double)Nrm[3 * pi + 2] * ((hx * hy) * gz);
      }
    }
  W[g] = (float)sw;
  if (i < C) Vx[((b * C + i) * R + j) * R + k] = (float)sx;
  if (j < C) Vy[((b * R + i) * C + j) * R + k] = (float)sy;
  if (k < C) Vz[((b * R + i) * R + j) * C + k] = (float)sz;
}

__global__ __launch_bounds__(256) void poisson_rhs_kernel(const float* __restrict__ Vx, const float* __restrict__ Vy,
                                                          const float* __restrict__ Vz, int B, int R, float* __restrict__ rhs) {
  const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long n3 = (long long)R * R * R;
  if (g >= (long long)B * n3) return;
  const int k = (int)(g % R), j = (int)((g / R) % R), i = (int)((g / ((long long)R * R)) % R);
  const long long b = g / n3;
  const int C = R - 1;
  const double xa = i < C ? (double)Vx[((b * C + i) * R + j) * R + k] : 0.0, xb = i > 0 ? (double)Vx[((b * C + i - 1) * R + j) * R + k] : 0.0;
  const double ya = j < C ? (double)Vy[((b * R + i) * C + j) * R + k] : 0.0, yb = j > 0 ? (double)Vy[((b * R + i) * C + j - 1) * R + k] : 0.0;
  const double za = k < C ? (double)Vz[((b * R + i) * R + j) * C + k] : 0.0, zb = k > 0 ? (double)Vz[((b * R + i) * R + j) * C + k - 1] : 0.0;
  rhs[g] = (float)(((xa - xb) + (ya - yb)) + (za - zb));
}

// ---- conjugate gradients ------------------------------------------------------------------------------------------------------------

constexpr int CG_THREADS = 256, CG_TJ = 16, CG_TK = 64, CG_HALO = 2 * CG_TK + 2 * CG_TJ;

// planes a workgroup of cg_apply_kernel marches through, and nodes a workgroup of the element-wise kernels owns: functions of R alone,
// so that a shape's reduction tree does not depend on the batch around it
inline int cg_ti(int R) { return R <= 129 ? 8 : (R <= 257 ? 16 : 32); }
inline int cg_span(int R) {
  const long long n3 = (long long)R * R * R;                   // at most ~2 100 partials per shape: every workgroup re-reads them all
  return n3 <= (1ll << 22) ? 4096 : (n3 <= (1ll << 25) ? 16384 : 65536);
}

struct CgLayout {
  long long n3;
  int ti, span, np_apply, np_elem, tiles;
  float *r, *p, *q;            // (B n3) each
  double *part_pq, *part_rr;   // (B np_apply), (B np_elem)
  double *rr, *bb, *tol2;      // (2 B), (B), one
  int *iter, *done;            // (2 B) each
};

inline CgLayout cg_layout(SfmiCarver& c, int B, int R) {
  CgLayout l;
  l.n3 = (long long)R * R * R;
  l.ti = cg_ti(R);
  l.span = cg_span(R);
  l.tiles = (int)(cdiv(R, CG_TK) * cdiv(R, CG_TJ));
  l.np_apply = l.tiles * (int)cdiv(R, l.ti);
  l.np_elem = (int)cdiv(l.n3, l.span);
  const size_t lat = (size_t)B * l.n3;
  l.r = c.take<float>(lat); l.p = c.take<float>(lat); l.q = c.take<float>(lat);
  l.part_pq = c.take<double>((size_t)B * l.np_apply); l.part_rr = c.take<double>((size_t)B * l.np_elem);
  l.rr = c.take<double>((size_t)2 * B); l.bb = c.take<double>((size_t)B); l.tol2 = c.take<double>(1);
  l.iter = c.take<int>((size_t)2 * B); l.done = c.take<int>((size_t)2 * B);
  return l;
}

// the sum of v over the workgroup's 256 lanes in every lane: wave_sum_f64, then the four waves in order
__device__ __forceinline__ double cg_block_sum(double v, double* red) {
  v = wave_sum_f64(v);
  __syncthreads();                                             // red may still be read from an earlier call
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// a dot product finished from the n partials an earlier launch left: every workgroup takes the same sum in the same order
__device__ __forceinline__ double cg_finish(const double* __restrict__ part, int n, double* red) {
  double s = 0.0;
  for (int t = threadIdx.x; t < n; t += CG_THREADS) s += part[t];
  return cg_block_sum(s, red);
}

// grid (tiles, planes / TI, B).  q = A p over a 16 x 64 tile of TI planes; part[b][blockIdx.y * tiles + blockIdx.x] = its share of <p, q>
__global__ __launch_bounds__(CG_THREADS) void cg_apply_kernel(const float* __restrict__ p, float* __restrict__ q, int R, int TI,
                                                              double* __restrict__ part) {
  __shared__ float plane[2][CG_TJ + 2][CG_TK + 2];
  __shared__ double red[4];
  const int tid = threadIdx.x, tk = tid & 63, tg = tid >> 6;
  const int tiles_k = (R + CG_TK - 1) / CG_TK;
  const int k0 = (blockIdx.x % tiles_k) * CG_TK, j0 = (blockIdx.x / tiles_k) * CG_TJ;
  const int i0 = blockIdx.y * TI, i1 = min(i0 + TI, R);
  const long long RR = (long long)R * R, n3 = RR * R;
  const float* __restrict__ pb = p + blockIdx.z * n3;
  float* __restrict__ qb = q + blockIdx.z * n3;
  // the lane's own columns: (j0 + 4 tg + m, k0 + tk); outside the lattice they hold the zeros that surround it
  bool in[4];
  long long col[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int j = j0 + 4 * tg + m, k = k0 + tk;
    in[m] = j < R && k < R;
    col[m] = (long long)j * R + k;
  }
  // lanes 0 .. 159 also carry one halo node each: the rows j0 - 1 and j0 + 16, the columns k0 - 1 and k0 + 64
  int hj = -1, hk = -1, lj = 0, lk = 0;
  if (tid < CG_TK) { hj = j0 - 1; hk = k0 + tid; lj = 0; lk = tid + 1; }
  else if (tid < 2 * CG_TK) { hj = j0 + CG_TJ; hk = k0 + tid - CG_TK; lj = CG_TJ + 1; lk = tid - CG_TK + 1; }
  else if (tid < 2 * CG_TK + CG_TJ) { hj = j0 + tid - 2 * CG_TK; hk = k0 - 1; lj = tid - 2 * CG_TK + 1; lk = 0; }
  else if (tid < CG_HALO) { hj = j0 + tid - 2 * CG_TK - CG_TJ; hk = k0 + CG_TK; lj = tid - 2 * CG_TK - CG_TJ + 1; lk = CG_TK + 1; }
  const bool hin = tid < CG_HALO && hj >= 0 && hj < R && hk >= 0 && hk < R;
  const long long hcol = (long long)hj * R + hk;
  float prev[4], cur[4], nxt[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    prev[m] = in[m] && i0 > 0 ? pb[(i0 - 1) * RR + col[m]] : 0.f;
    cur[m] = in[m] ? pb[i0 * RR + col[m]] : 0.f;
  }
  float hcur = hin ? pb[i0 * RR + hcol] : 0.f;
  double acc = 0.0;
  for (int i = i0; i < i1; ++i) {
    const bool more = i + 1 < R;
#pragma unroll
    for (int m = 0; m < 4; ++m) nxt[m] = in[m] && more ? pb[(i + 1) * RR + col[m]] : 0.f;
    const float hnext = hin && more ? pb[(i + 1) * RR + hcol] : 0.f;
    // buffer (i & 1) is written again two planes on, behind the barrier of plane i + 1, which every lane reaches after its reads here
    float (*pl)[CG_TK + 2] = plane[i & 1];
#pragma unroll
    for (int m = 0; m < 4; ++m) pl[4 * tg + m + 1][tk + 1] = cur[m];
    if (tid < CG_HALO) pl[lj][lk] = hcur;
    __syncthreads();
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int y = 4 * tg + m + 1;
      const float s = ((prev[m] + nxt[m]) + (pl[y - 1][tk + 1] + pl[y + 1][tk + 1])) + (pl[y][tk] + pl[y][tk + 2]);
      const float v = 6.f * cur[m] - s;
      if (in[m]) {
        qb[i * RR + col[m]] = v;
        acc += (double)cur[m] * (double)v;
      }
      prev[m] = cur[m];
      cur[m] = nxt[m];
    }
    hcur = hnext;
  }
  acc = cg_block_sum(acc, red);
  if (tid == 0) part[(long long)blockIdx.z * gridDim.x * gridDim.y + (long long)blockIdx.y * gridDim.x + blockIdx.x] = acc;
}

// grid (n3 / span, B)
__global__ __launch_bounds__(CG_THREADS) void cg_init_kernel(const float* __restrict__ rhs, float* __restrict__ x, float* __restrict__ r,
                                                             float* __restrict__ p, long long n3, int span, double* __restrict__ part) {
  __shared__ double red[4];
  const long long base = blockIdx.y * n3, s0 = (long long)blockIdx.x * span, s1 = min(s0 + span, n3);
  double acc = 0.0;
  for (long long e = s0 + threadIdx.x; e < s1; e += CG_THREADS) {
    const float v = rhs[base + e];
    x[base + e] = 0.f;
    r[base + e] = v;
    p[base + e] = v;
    acc += (double)v * (double)v;
  }
  acc = cg_block_sum(acc, red);
  if (threadIdx.x == 0) part[(long long)blockIdx.y * gridDim.x + blockIdx.x] = acc;
}

// grid (B): the state of iteration 0 (copy 0)
__global__ __launch_bounds__(CG_THREADS) void cg_init_state_kernel(const double* __restrict__ part, int np, double tol, double* __restrict__ rr,
                                                                   double* __restrict__ bb, double* __restrict__ tol2, int* __restrict__ iter,
                                                                   int* __restrict__ done) {
  __shared__ double red[4];
  const int b = blockIdx.x;
  const double s = cg_finish(part + (long long)b * np, np, red);
  if (threadIdx.x == 0) {
    rr[b] = s;
    bb[b] = s;
    iter[b] = 0;
    done[b] = !(s > 0.0) || s <= (tol * tol) * s;              // b = 0 (or not finite): frozen from the start, x stays 0
    if (b == 0) tol2[0] = tol * tol;
  }
}

__global__ __launch_bounds__(CG_THREADS) void cg_update_kernel(float* __restrict__ x, float* __restrict__ r, const float* __restrict__ p,
                                                               const float* __restrict__ q, long long n3, int span,
                                                               const double* __restrict__ part_pq, int np_pq, const double* __restrict__ rr,
                                                               const int* __restrict__ done, double* __restrict__ part_rr) {
  __shared__ double red[4];
  const int b = blockIdx.y;
  const double pq = cg_finish(part_pq + (long long)b * np_pq, np_pq, red);
  const float alpha = (done[b] || !(pq > 0.0)) ? 0.f : (float)(rr[b] / pq);
  const long long base = b * n3, s0 = (long long)blockIdx.x * span, s1 = min(s0 + span, n3);
  double acc = 0.0;
#pragma unroll 4
  for (long long e = s0 + threadIdx.x; e < s1; e += CG_THREADS) {
    const float xv = fmaf(alpha, p[base + e], x[base + e]);
    const float rv = fmaf(-alpha, q[base + e], r[base + e]);
    x[base + e] = xv;
    r[base + e] = rv;
    acc += (double)rv * (double)rv;
  }
  acc = cg_block_sum(acc, red);
  if (threadIdx.x == 0) part_rr[(long long)b * gridDim.x + blockIdx.x] = acc;
}

// reads the state copy `cur`, writes the copy `nxt` (workgroup 0 of each shape): no lane reads what this launch writes
__global__ __launch_bounds__(CG_THREADS) void cg_direction_kernel(float* __restrict__ p, const float* __restrict__ r, long long n3, int span,
                                                                  const double* __restrict__ part_rr, int np_rr,
                                                                  const double* __restrict__ bb, const double* __restrict__ tol2,
                                                                  const double* __restrict__ rr_cur, const int* __restrict__ iter_cur,
                                                                  const int* __restrict__ done_cur, double* __restrict__ rr_nxt,
                                                                  int* __restrict__ iter_nxt, int* __restrict__ done_nxt) {
  __shared__ double red[4];
  const int b = blockIdx.y;
  const double rrn = cg_finish(part_rr + (long long)b * np_rr, np_rr, red);
  const int d = done_cur[b];
  const double rro = rr_cur[b];
  const float beta = (d || !(rro > 0.0)) ? 0.f : (float)(rrn / rro);
  const long long base = b * n3, s0 = (long long)blockIdx.x * span, s1 = min(s0 + span, n3);
#pragma unroll 4
  for (long long e = s0 + threadIdx.x; e < s1; e += CG_THREADS) p[base + e] = fmaf(beta, p[base + e], r[base + e]);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    rr_nxt[b] = d ? rro : rrn;
    iter_nxt[b] = iter_cur[b] + (d ? 0 : 1);
    done_nxt[b] = d || rrn <= tol2[0] * bb[b];
  }
}

__global__ void cg_read_kernel(const double* __restrict__ rr, const double* __restrict__ bb, const int* __restrict__ iter,
                               const int* __restrict__ done, int B, int* __restrict__ iters, double* __restrict__ residual,
                               int* __restrict__ done_out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  iters[b] = iter[b];
  residual[b] = bb[b] > 0.0 ? sqrt(rr[b] / bb[b]) : 0.0;
  done_out[b] = done[b];
}

// ---- iso-value, subtraction, samples ------------------------------------------------------------------------------------------------

constexpr int ISO_THREADS = 1024;

// grid (B): iso[b] = mean of the trilinear chi over the in-box points of set b (0 for a set without one)
__global__ __launch_bounds__(ISO_THREADS) void poisson_iso_kernel(const float* __restrict__ chi, const float* __restrict__ P,
                                                                  const long long* __restrict__ off, int R, PBox bx,
                                                                  double* __restrict__ iso) {
  __shared__ double rs[ISO_THREADS / 64], rc[ISO_THREADS / 64];
  const int b = blockIdx.x, tid = threadIdx.x;
  const long long beg = off[b], end = off[b + 1];
  const long long per = cdiv(end - beg, (long long)ISO_THREADS);
  const long long j0 = min(beg + tid * per, end), j1 = min(j0 + per, end);
  const float* __restrict__ L = chi + (long long)b * R * R * R;
  double s = 0.0, c = 0.0;
  for (long long j = j0; j < j1; ++j) {                        // the lane's chunk in input order
    double t[3];
    if (p_coord(bx, R, P + 3 * j, t)) {
      s += p_sample(L, R, t);
      c += 1.0;
    }
  }
  s = wave_sum_f64(s);
  c = wave_sum_f64(c);
  if ((tid & 63) == 0) {
    rs[tid >> 6] = s;
    rc[tid >> 6] = c;
  }
  __syncthreads();
  if (tid == 0) {
    s = 0.0;
    c = 0.0;
    for (int w = 0; w < ISO_THREADS / 64; ++w) {
      s += rs[w];
      c += rc[w];
    }
    iso[b] = c > 0.0 ? s / c : 0.0;
  }
}

__global__ __launch_bounds__(256) void poisson_sub_kernel(const float* __restrict__ chi, const double* __restrict__ iso, long long n3,
                                                          long long total, float* __restrict__ field) {
  const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= total) return;
  field[g] = (float)((double)chi[g] - iso[g / n3]);
}

__global__ __launch_bounds__(256) void poisson_sample_kernel(const float* __restrict__ L, const float* __restrict__ P,
                                                             const long long* __restrict__ off, int B, long long N, int R, PBox bx,
                                                             float* __restrict__ out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int b = sfmi_owner(off, B, i);
  double t[3];
  p_coord(bx, R, P + 3 * i, t);
  out[i] = (float)p_sample(L + (long long)b * R * R * R, R, t);
}

constexpr int POISSON_MIN_R = 5, POISSON_MAX_R = 513;

inline bool p_dims_ok(int B, int R) {
  return B > 0 && R >= POISSON_MIN_R && R <= POISSON_MAX_R && (long long)B * R * R * R < (1ll << 31) && B <= 65535;
}

// box: 6 doubles on the host, lo xyz then hi xyz -> false for a box without extent
inline bool p_box(const double* box, int R, PBox& bx) {
  if (!box) return false;
  for (int a = 0; a < 3; ++a) {
    bx.lo[a] = box[a];
    bx.hi[a] = box[3 + a];
    bx.h[a] = (box[3 + a] - box[a]) / (double)(R - 1);
    if (!(bx.h[a] > 0.0) || !(bx.h[a] < INFINITY)) return false;
  }
  return true;
}

}  // namespace

extern "C" {

int sfmi_poisson_keys_f32(const float* P, const float* Nrm, const long long* off, int B, long long N, int R, const double* box,
                          long long* keys, int* outside, int* status, void* stream) {
  PBox bx;
  if (!p_dims_ok(B, R) || N < 0 || N >= (1ll << 31) || !p_box(box, R, bx) || !off || !outside || !status) return SFMI_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  SFMI_TRY(hipMemsetAsync(status, 0, sizeof(int), st));
  SFMI_TRY(hipMemsetAsync(outside, 0, (size_t)B * sizeof(int), st));
  if (N == 0) return SFMI_OK;
  if (!P || !Nrm || !keys) return SFMI_EINVAL;
  hipLaunchKernelGGL(poisson_key_kernel, dim3(blocks256(N)), dim3(256), 0, st, P, Nrm, off, B, N, R, bx, keys, outside, status);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_poisson_cells_i32(const long long* sorted_keys, int B, long long N, int R, int* cell_start, void* stream) {
  if (!p_dims_ok(B, R) || N < 0 || N >= (1ll << 31) || !cell_start || (N > 0 && !sorted_keys)) return SFMI_EINVAL;
  const long long C = R - 1, ncell = B * C * C * C;
  hipLaunchKernelGGL(poisson_cells_kernel, dim3(blocks256(ncell + 1)), dim3(256), 0, (hipStream_t)stream, sorted_keys, (int)N, ncell,
                     cell_start);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_poisson_splat_f32(const float* P, const float* Nrm, const long long* order, const int* cell_start, int B, long long N, int R,
                           const double* box, float* Vx, float* Vy, float* Vz, float* W, void* stream) {
  PBox bx;
  if (!p_dims_ok(B, R) || N < 0 || N >= (1ll << 31) || !p_box(box, R, bx) || !cell_start || !Vx || !Vy || !Vz || !W) return SFMI_EINVAL;
  if (N > 0 && (!P || !Nrm || !order)) return SFMI_EINVAL;
  hipLaunchKernelGGL(poisson_splat_kernel, dim3(blocks256((long long)B * R * R * R)), dim3(256), 0, (hipStream_t)stream, P, Nrm, order,
                     cell_start, B, R, bx, Vx, Vy, Vz, W);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_poisson_rhs_f32(const float* Vx, const float* Vy, const float* Vz, int B, int R, float* rhs, void* stream) {
  if (!p_dims_ok(B, R) || !Vx || !Vy || !Vz || !rhs) return SFMI_EINVAL;
  hipLaunchKernelGGL(poisson_rhs_kernel, dim3(blocks256((long long)B * R * R * R)), dim3(256), 0, (hipStream_t)stream, Vx, Vy, Vz, B, R, rhs);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

size_t sfmi_poisson_cg_workspace_bytes(int B, int R) {
  if (!p_dims_ok(B, R)) return 0;
  return sfmi_ws_bytes(cg_layout, B, R);
}

int sfmi_poisson_cg_init_f32(const float* rhs, int B, int R, double tol, float* x, void* workspace, void* stream) {
  if (!p_dims_ok(B, R) || !(tol > 0.0) || !rhs || !x || !workspace) return SFMI_EINVAL;
  SfmiCarver c{(char*)workspace};
  const CgLayout l = cg_layout(c, B, R);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(cg_init_kernel, dim3((unsigned)l.np_elem, (unsigned)B), dim3(CG_THREADS), 0, st, rhs, x, l.r, l.p, l.n3, l.span,
                     l.part_rr);
  hipLaunchKernelGGL(cg_init_state_kernel, dim3((unsigned)B), dim3(CG_THREADS), 0, st, (const double*)l.part_rr, l.np_elem, tol, l.rr,
                     l.bb, l.tol2, l.iter, l.done);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_poisson_cg_steps_f32(int B, int R, int n, long long it0, float* x, void* workspace, void* stream) {
  if (!p_dims_ok(B, R) || n < 0 || it0 < 0 || !x || !workspace) return SFMI_EINVAL;
  SfmiCarver c{(char*)workspace};
  const CgLayout l = cg_layout(c, B, R);
  hipStream_t st = (hipStream_t)stream;
  float *r = l.r, *p = l.p, *q = l.q;
  double *ppq = l.part_pq, *prr = l.part_rr, *rr = l.rr, *bb = l.bb, *tol2 = l.tol2;
  int *iter = l.iter, *done = l.done;
  const dim3 ga((unsigned)l.tiles, (unsigned)cdiv(R, l.ti), (unsigned)B), ge((unsigned)l.np_elem, (unsigned)B);
  for (int t = 0; t < n; ++t) {
    const int cur = (int)((it0 + t) & 1), nxt = cur ^ 1;
    hipLaunchKernelGGL(cg_apply_kernel, ga, dim3(CG_THREADS), 0, st, (const float*)p, q, R, l.ti, ppq);
    hipLaunchKernelGGL(cg_update_kernel, ge, dim3(CG_THREADS), 0, st, x, r, (const float*)p, (const float*)q, l.n3, l.span,
                       (const double*)ppq, l.np_apply, (const double*)(rr + cur * B), (const int*)(done + cur * B), prr);
    hipLaunchKernelGGL(cg_direction_kernel, ge, dim3(CG_THREADS), 0, st, p, (const float*)r, l.n3, l.span, (const double*)prr, l.np_elem,
                       (const double*)bb, (const double*)tol2, (const double*)(rr + cur * B), (const int*)(iter + cur * B),
                       (const int*)(done + cur * B), rr + nxt * B, iter + nxt * B, done + nxt * B);
  }
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_poisson_cg_read_i32(int B, int R, long long it, const void* workspace, int* iterations, double* residual, int* done, void* stream) {
  if (!p_dims_ok(B, R) || it < 0 || !workspace || !iterations || !residual || !done) return SFMI_EINVAL;
  SfmiCarver c{(char*)const_cast<void*>(workspace)};           // read only: the kernel below takes const pointers
  const CgLayout l = cg_layout(c, B, R);
  const int cur = (int)(it & 1);
  hipLaunchKernelGGL(cg_read_kernel, dim3(blocks256(B)), dim3(256), 0, (hipStream_t)stream, (const double*)l.rr + cur * B,
                     (const double*)l.bb, (const int*)l.iter + cur * B, (const int*)l.done + cur * B, B, iterations, residual, done);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_poisson_iso_f32(const float* chi, const float* P, const long long* off, int B, long long N, int R, const double* box, double* iso,
                         float* field, void* stream) {
  PBox bx;
  if (!p_dims_ok(B, R) || N < 0 || !p_box(box, R, bx) || !chi || !off || !iso || !field) return SFMI_EINVAL;
  if (N > 0 && !P) return SFMI_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const long long n3 = (long long)R * R * R;
  hipLaunchKernelGGL(poisson_iso_kernel, dim3((unsigned)B), dim3(ISO_THREADS), 0, st, chi, P, off, R, bx, iso);
  hipLaunchKernelGGL(poisson_sub_kernel, dim3(blocks256(B * n3)), dim3(256), 0, st, chi, (const double*)iso, n3, B * n3, field);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_poisson_sample_f32(const float* lattice, const float* P, const long long* off, int B, long long N, int R, const double* box,
                            float* out, void* stream) {
  PBox bx;
  if (!p_dims_ok(B, R) || N < 0 || !p_box(box, R, bx) || !lattice || !off) return SFMI_EINVAL;
  if (N == 0) return SFMI_OK;
  if (!P || !out) return SFMI_EINVAL;
  hipLaunchKernelGGL(poisson_sample_kernel, dim3(blocks256(N)), dim3(256), 0, (hipStream_t)stream, lattice, P, off, B, N, R, bx, out);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

}  // extern "C"
