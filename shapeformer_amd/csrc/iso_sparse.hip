// Coarse-to-fine sparse iso-surface extraction: the structure side of a mesh at Q = (Q0-1) 2^L + 1 points per axis that
// never materialises the Q^3 lattice.  The reference meshes a dense grid only (xgutils/geoutil.py:175-233 array2mesh over the Q^3
// occupancy that shapeformer.py:382-391 / vqdif.py:60-76 decode); the multi-resolution route of occupancy-network codebases is the model.
//
// Data structure: per shape a bitmap of Q^3 bits keyed by the fine lattice index p = (i0 Q + i1) Q + i2 (i0 slowest), and per 32-bit
// word the inclusive prefix count of set bits over the whole batch.  atomicOr de-duplicates, the prefix count plus a popcount gives a
// key's slot in O(1), and walking the words in order gives the ascending key list without a sort.  Two such sets exist: the points
// whose field value is known at this level, and the cells of the next level.  Everything else is proportional to the active counts.
//   seed      level 0: every coarse point and cell
//   popc      set bits per word (the caller's inclusive scan of it is the rank table)
//   compact   bitmap + rank -> ascending shape-local keys
//   carry     where the keys of the level before sit in the new point set, so their values are moved instead of evaluated again
//   classify  a cell is cut when its 8 corner values are not all on one side of iso (v > iso, as csrc/mcubes.hip); its flag byte
//             is its cube index, which the marching-cubes passes read instead of the values
//   refine    cut cells, dilated by `margin` and clipped -> their children's keys and the children's corner points, as bits
//   mc_count  over the cut cells of the last level: triangles per cell, and per point the axes of its cut edges (3-bit mask)
//   mc_emit   vertices by (shape, p, axis), triangles by (shape, cell p, table order): the dense order of csrc/mcubes.hip, the vertex
//             id of an edge found through its low point's slot, and the same vertex expressions
// Integer atomicOr only: the result does not depend on the order in which threads run.
#include "sfmi_ragged.h"   // the ragged-batch helpers the mesh tools share: DESIGN.md §5.5a

namespace {
#include "mc_table.h"   // internal linkage: csrc/mcubes.hip owns the exported copy

struct IsoLat {
  int B, Q;
  unsigned W;   // bitmap words per shape
};

// slot of key p of shape b in the batch-wide ascending list: inclusive count up to p's word minus the bits at or above p
__device__ __forceinline__ int iso_slot(const IsoLat g, const unsigned* __restrict__ bits, const int* __restrict__ rank, int b, int p, int n) {
  const unsigned w = (unsigned)b * g.W + ((unsigned)p >> 5);
  const int s = rank[w] - __popc(bits[w] >> (p & 31));
  return min(max(s, 0), n - 1);   // a key that is not in the set can never index outside the value array
}

__device__ __forceinline__ void iso_set(unsigned* bits, unsigned w, unsigned m) {
  if (m && (bits[w] & m) != m) atomicOr(&bits[w], m);
}

// keys row + z*h for z0 <= z <= z1 (one lattice row along the fastest axis), one atomicOr per touched word
__device__ __forceinline__ void iso_mark_row(unsigned* bits, unsigned wbase, int row, int z0, int z1, int h) {
  unsigned cur = 0xFFFFFFFFu, m = 0;
  for (int z = z0; z <= z1; ++z) {
    const unsigned key = (unsigned)(row + z * h), w = key >> 5;
    if (w != cur) {
      if (cur != 0xFFFFFFFFu) iso_set(bits, wbase + cur, m);
      cur = w; m = 0;
    }
    m |= 1u << (key & 31);
  }
  if (cur != 0xFFFFFFFFu) iso_set(bits, wbase + cur, m);
}

__global__ __launch_bounds__(256) void iso_seed_kernel(IsoLat g, int Q0, int s, unsigned* __restrict__ pbits, unsigned* __restrict__ cbits) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int n0 = Q0 * Q0 * Q0;
  if (t >= g.B * n0) return;
  const int b = t / n0, r = t - b * n0;
  const int i0 = r / (Q0 * Q0), i1 = (r / Q0) % Q0, i2 = r % Q0;
  const unsigned key = (unsigned)(((i0 * s) * g.Q + i1 * s) * g.Q + i2 * s);
  const unsigned w = (unsigned)b * g.W + (key >> 5), m = 1u << (key & 31);
  atomicOr(&pbits[w], m);
  if (i0 + 1 < Q0 && i1 + 1 < Q0 && i2 + 1 < Q0) atomicOr(&cbits[w], m);
}

__global__ __launch_bounds__(256) void iso_popc_kernel(const unsigned* __restrict__ bits, int* __restrict__ cnt, unsigned n) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i < n) cnt[i] = __popc(bits[i]);
}

__global__ __launch_bounds__(256) void iso_compact_kernel(IsoLat g, const unsigned* __restrict__ bits, const int* __restrict__ rank,
                                                          int* __restrict__ keys, int n) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= (unsigned)g.B * g.W) return;
  unsigned word = bits[i];
  if (!word) return;
  int o = rank[i] - __popc(word);
  const unsigned w = i % g.W;
  while (word) {
    const int bit = __ffs(word) - 1;
    if (o >= 0 && o < n) keys[o] = (int)((w << 5) + bit);
    ++o;
    word &= word - 1;
  }
}

// dst[j] = the slot of key j of an earlier list in the set, or -1 where the set does not hold it: values known from the level
// before are carried over instead of evaluated again
__global__ __launch_bounds__(256) void iso_carry_kernel(IsoLat g, const int* __restrict__ keys, const int* __restrict__ off, int n,
                                                        const unsigned* __restrict__ bits, const int* __restrict__ rank, int* __restrict__ dst) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const int p = keys[j];
  const unsigned w = (unsigned)sfmi_shape_of(off, g.B, j) * g.W + ((unsigned)p >> 5);
  const unsigned up = bits[w] >> (p & 31);
  dst[j] = (up & 1) ? rank[w] - __popc(up) : -1;
}

// corner c of the cell at p with stride s: bit 0 of c steps axis 0 (slowest), bit 1 axis 1, bit 2 axis 2 - csrc/mcubes.hip's mc_cube_index
__device__ __forceinline__ int iso_corner(const IsoLat g, int p, int s, int c) {
  return p + ((c & 1) * g.Q * g.Q + ((c >> 1) & 1) * g.Q + ((c >> 2) & 1)) * s;
}

__device__ __forceinline__ int iso_cube_index(const IsoLat g, const unsigned* __restrict__ pbits, const int* __restrict__ prank,
                                              const float* __restrict__ vals, int nP, float iso, int b, int p, int s) {
  int ci = 0;
#pragma unroll
  for (int c = 0; c < 8; ++c) ci |= (vals[iso_slot(g, pbits, prank, b, iso_corner(g, p, s, c), nP)] > iso) << c;
  return ci;
}

__global__ __launch_bounds__(256) void iso_classify_kernel(IsoLat g, const int* __restrict__ cells, const int* __restrict__ coff, int nC, int s,
                                                           const unsigned* __restrict__ pbits, const int* __restrict__ prank,
                                                           const float* __restrict__ vals, int nP, float iso, unsigned char* __restrict__ flag) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= nC) return;
  const int ci = iso_cube_index(g, pbits, prank, vals, nP, iso, sfmi_shape_of(coff, g.B, j), cells[j], s);
  flag[j] = (unsigned char)(ci == 255 ? 0 : ci);   // the cube index of a cut cell (1..254), 0 where the cell is not cut
}

// the carried values land in their new slots; known marks them
__global__ __launch_bounds__(256) void iso_carry_apply_kernel(const int* __restrict__ dst, const float* __restrict__ old, int n,
                                                              float* __restrict__ vals, unsigned char* __restrict__ known, int nNew) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const int d = dst[j];
  if (d >= 0 && d < nNew) { vals[d] = old[j]; known[d] = 1; }
}

// sel[k] = the index of the k-th slot without a value (uincl: inclusive prefix count of such slots)
__global__ __launch_bounds__(256) void iso_select_kernel(const unsigned char* __restrict__ known, const int* __restrict__ uincl, int n,
                                                         int* __restrict__ sel, int nE) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n || known[i]) return;
  const int k = uincl[i] - 1;
  if (k >= 0 && k < nE) sel[k] = i;
}

__global__ __launch_bounds__(256) void iso_refine_kernel(IsoLat g, const int* __restrict__ cells, const int* __restrict__ coff,
                                                         const unsigned char* __restrict__ flag, int nC, int s, int margin,
                                                         unsigned* __restrict__ pbits, unsigned* __restrict__ cbits) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= nC || !flag[j]) return;
  const int b = sfmi_shape_of(coff, g.B, j);
  const unsigned p = (unsigned)cells[j], uq = (unsigned)g.Q;
  const unsigned r = p / uq;
  const int i2 = (int)(p - r * uq), i0 = (int)(r / uq), i1 = (int)(r - (unsigned)i0 * uq);
  const int h = s >> 1;                 // the children's stride
  const int nch = (g.Q - 1) / h;        // child cells per axis
  int lo[3], hi[3];
  const int c[3] = {i0 / s, i1 / s, i2 / s};
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    lo[d] = max(0, 2 * (c[d] - margin));
    hi[d] = min(nch - 1, 2 * (c[d] + margin) + 1);
  }
  const unsigned wbase = (unsigned)b * g.W;
  for (int x = lo[0]; x <= hi[0] + 1; ++x)
    for (int y = lo[1]; y <= hi[1] + 1; ++y) {
      const int row = ((x * h) * g.Q + y * h) * g.Q;
      iso_mark_row(pbits, wbase, row, lo[2], hi[2] + 1, h);
      if (x <= hi[0] && y <= hi[1]) iso_mark_row(cbits, wbase, row, lo[2], hi[2], h);
    }
}

__global__ __launch_bounds__(256) void iso_mc_count_kernel(IsoLat g, const int* __restrict__ cells, const int* __restrict__ coff,
                                                           const unsigned char* __restrict__ flag, int nC, const unsigned* __restrict__ pbits,
                                                           const int* __restrict__ prank, int nP, int* __restrict__ emask,
                                                           int* __restrict__ ntri) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= nC) return;
  const int ci = flag[j];                  // the cube index classify stored
  ntri[j] = MC_NTRI[ci];
  if (!ci) return;
  const int b = sfmi_shape_of(coff, g.B, j), p = cells[j];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int uv = 0; uv < 4; ++uv) {
      const int u = uv & 1, v = uv >> 1;
      const int c0 = a == 0 ? (u << 1) | (v << 2) : (a == 1 ? u | (v << 2) : u | (v << 1));
      const int c1 = c0 | (1 << a);
      if (((ci >> c0) & 1) != ((ci >> c1) & 1)) {
        const int sl = iso_slot(g, pbits, prank, b, iso_corner(g, p, 1, c0), nP);
        if (!((emask[sl] >> a) & 1)) atomicOr(&emask[sl], 1 << a);
      }
    }
}

struct IsoBox { float lo[3], hi[3]; };

__global__ __launch_bounds__(256) void iso_mc_verts_kernel(IsoLat g, const int* __restrict__ pkeys, const int* __restrict__ poff, int nP,
                                                           const unsigned* __restrict__ pbits, const int* __restrict__ prank,
                                                           const float* __restrict__ vals, float iso, const int* __restrict__ emask,
                                                           const int* __restrict__ vincl, IsoBox box, float* __restrict__ verts) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= 3u * (unsigned)nP) return;
  const int j = (int)(i / 3u), a = (int)(i - 3u * (unsigned)j);
  const int m = emask[j] & 7;
  if (!((m >> a) & 1)) return;
  const unsigned p = (unsigned)pkeys[j], uq = (unsigned)g.Q;
  const unsigned r = p / uq;
  int idx[3];
  idx[2] = (int)(p - r * uq); idx[0] = (int)(r / uq); idx[1] = (int)(r - (unsigned)idx[0] * uq);
  if (idx[a] + 1 >= g.Q) return;
  const int step = a == 0 ? g.Q * g.Q : (a == 1 ? g.Q : 1);
  const int b = sfmi_shape_of(poff, g.B, j);
  const float f0 = vals[j], f1 = vals[iso_slot(g, pbits, prank, b, (int)p + step, nP)];
  const float t = __fdiv_rn(iso - f0, f1 - f0);
  float* o = verts + 3ll * (vincl[j] - __popc(m) + __popc(m & ((1 << a) - 1)));
  const float inv = (float)(g.Q - 1);
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const float pos = (float)idx[d] + (d == a ? t : 0.f);
    o[d] = __fmaf_rn(__fdiv_rn(pos, inv), box.hi[d] - box.lo[d], box.lo[d]);
  }
}

__global__ __launch_bounds__(256) void iso_mc_faces_kernel(IsoLat g, const int* __restrict__ cells, const int* __restrict__ coff,
                                                           const unsigned char* __restrict__ flag, int nC, const unsigned* __restrict__ pbits,
                                                           const int* __restrict__ prank, int nP, const int* __restrict__ emask,
                                                           const int* __restrict__ vincl, const int* __restrict__ tincl,
                                                           const int* __restrict__ voff, int* __restrict__ faces) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= nC) return;
  const int ci = flag[j];
  const int nt = MC_NTRI[ci];
  if (!nt) return;
  const int b = sfmi_shape_of(coff, g.B, j), p = cells[j];
  const int vbase = voff[b];
  int* o = faces + 3ll * (tincl[j] - nt);
  for (int k = 0; k < 3 * nt; ++k) {
    const int e = MC_TRI[ci][k];
    const int a = e >> 2, u = e & 1, v = (e >> 1) & 1;
    // edge e runs along axis a from the corner whose other two offsets (increasing axis order) are (u, v)
    const int d0 = a == 0 ? 0 : u, d1 = a == 0 ? u : (a == 1 ? 0 : v), d2 = a == 2 ? 0 : v;
    const int sl = iso_slot(g, pbits, prank, b, p + (d0 * g.Q + d1) * g.Q + d2, nP);
    const int m = emask[sl] & 7;
    o[k] = vincl[sl] - __popc(m) + __popc(m & ((1 << a) - 1)) - vbase;
  }
}

// Q = (Q0-1) 2^L + 1, Q0 >= 2, L >= 1, Q^3 < 2^31, B >= 1 and the batch's bitmap words countable in 32 bits
inline bool iso_ok(int B, int Q0, int L, int Q) {
  if (B <= 0 || Q0 < 2 || L < 1 || L > 30 || Q < 3) return false;
  if ((long long)Q * Q * Q >= (1ll << 31)) return false;
  if ((((long long)Q0 - 1) << L) + 1 != (long long)Q) return false;
  return (long long)B * (((long long)Q * Q * Q + 31) >> 5) < (1ll << 31);
}
inline IsoLat iso_lat(int B, int Q) { return IsoLat{B, Q, (unsigned)(((long long)Q * Q * Q + 31) >> 5)}; }

}  // namespace

extern "C" {

// [point bits | point rank | cell bits | cell rank], a quarter of the size each
size_t sfmi_iso_sparse_workspace_bytes(int B, int Q) {
  if (B <= 0 || Q < 2 || (long long)Q * Q * Q >= (1ll << 31)) return 0;
  return 4 * align256((size_t)B * iso_lat(B, Q).W * 4);
}

int sfmi_iso_seed_i32(int B, int Q0, int L, int Q, unsigned* pbits, unsigned* cbits, void* stream) {
  if (!pbits || !cbits || !iso_ok(B, Q0, L, Q) || (long long)B * Q0 * Q0 * Q0 >= (1ll << 31)) return SFMI_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const IsoLat g = iso_lat(B, Q);
  SFMI_TRY(hipMemsetAsync(pbits, 0, (size_t)B * g.W * 4, st));
  SFMI_TRY(hipMemsetAsync(cbits, 0, (size_t)B * g.W * 4, st));
  hipLaunchKernelGGL(iso_seed_kernel, dim3(blocks256((long long)B * Q0 * Q0 * Q0)), dim3(256), 0, st, g, Q0, 1 << L, pbits, cbits);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_iso_popc_i32(const unsigned* bits, int* cnt, int B, int Q0, int L, int Q, void* stream) {
  if (!bits || !cnt || !iso_ok(B, Q0, L, Q)) return SFMI_EINVAL;
  const IsoLat g = iso_lat(B, Q);
  hipLaunchKernelGGL(iso_popc_kernel, dim3(blocks256((long long)B * g.W)), dim3(256), 0, (hipStream_t)stream, bits, cnt, (unsigned)B * g.W);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_iso_compact_i32(const unsigned* bits, const int* rank, int B, int Q0, int L, int Q, int* keys, int n, void* stream) {
  if (!bits || !rank || !iso_ok(B, Q0, L, Q) || n < 0 || (n > 0 && !keys)) return SFMI_EINVAL;
  if (n == 0) return SFMI_OK;
  const IsoLat g = iso_lat(B, Q);
  hipLaunchKernelGGL(iso_compact_kernel, dim3(blocks256((long long)B * g.W)), dim3(256), 0, (hipStream_t)stream, g, bits, rank, keys, n);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_iso_carry_i32(const int* keys, const int* off, int n, const unsigned* bits, const int* rank, int B, int Q0, int L, int Q, int* dst,
                       void* stream) {
  if (!iso_ok(B, Q0, L, Q) || n < 0 || !off || !bits || !rank || (n > 0 && (!keys || !dst))) return SFMI_EINVAL;
  if (n == 0) return SFMI_OK;
  hipLaunchKernelGGL(iso_carry_kernel, dim3(blocks256(n)), dim3(256), 0, (hipStream_t)stream, iso_lat(B, Q), keys, off, n, bits, rank, dst);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_iso_carry_apply_f32(const int* dst, const float* old, int n, float* vals, unsigned char* known, int n_new, void* stream) {
  if (n < 0 || n_new < 0 || (n > 0 && (!dst || !old || !vals || !known))) return SFMI_EINVAL;
  if (n == 0 || n_new == 0) return SFMI_OK;
  hipLaunchKernelGGL(iso_carry_apply_kernel, dim3(blocks256(n)), dim3(256), 0, (hipStream_t)stream, dst, old, n, vals, known, n_new);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_iso_select_i32(const unsigned char* known, const int* uincl, int n, int* sel, int n_sel, void* stream) {
  if (n < 0 || n_sel < 0 || (n > 0 && (!known || !uincl)) || (n_sel > 0 && !sel)) return SFMI_EINVAL;
  if (n == 0 || n_sel == 0) return SFMI_OK;
  hipLaunchKernelGGL(iso_select_kernel, dim3(blocks256(n)), dim3(256), 0, (hipStream_t)stream, known, uincl, n, sel, n_sel);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_iso_classify_f32(const int* cells, const int* coff, int nC, int level, const unsigned* pbits, const int* prank, const float* vals,
                          int nP, float iso, int B, int Q0, int L, int Q, unsigned char* flag, void* stream) {
  if (!iso_ok(B, Q0, L, Q) || level < 0 || level > L || nC < 0 || nP < 0 || !coff || !pbits || !prank) return SFMI_EINVAL;
  if (nC > 0 && (!cells || !vals || !flag || nP == 0)) return SFMI_EINVAL;
  if (nC == 0) return SFMI_OK;
  hipLaunchKernelGGL(iso_classify_kernel, dim3(blocks256(nC)), dim3(256), 0, (hipStream_t)stream, iso_lat(B, Q), cells, coff, nC, 1 << (L - level),
                     pbits, prank, vals, nP, iso, flag);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_iso_refine_i32(const int* cells, const int* coff, const unsigned char* flag, int nC, int level, int margin, int B, int Q0, int L, int Q,
                        unsigned* pbits, unsigned* cbits, void* stream) {
  if (!iso_ok(B, Q0, L, Q) || level < 0 || level >= L || margin < 0 || margin > 1 || nC < 0 || !coff || !pbits || !cbits) return SFMI_EINVAL;
  if (nC > 0 && (!cells || !flag)) return SFMI_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const IsoLat g = iso_lat(B, Q);
  SFMI_TRY(hipMemsetAsync(pbits, 0, (size_t)B * g.W * 4, st));
  SFMI_TRY(hipMemsetAsync(cbits, 0, (size_t)B * g.W * 4, st));
  if (nC > 0)
    hipLaunchKernelGGL(iso_refine_kernel, dim3(blocks256(nC)), dim3(256), 0, st, g, cells, coff, flag, nC, 1 << (L - level), margin, pbits, cbits);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_iso_mc_count_i32(const int* cells, const int* coff, const unsigned char* flag, int nC, const unsigned* pbits, const int* prank, int nP,
                          int B, int Q0, int L, int Q, int* emask, int* ntri, void* stream) {
  if (!iso_ok(B, Q0, L, Q) || nC < 0 || nP < 0 || !coff || !pbits || !prank) return SFMI_EINVAL;
  if (nP > 0 && !emask) return SFMI_EINVAL;
  if (nC > 0 && (!cells || !flag || !ntri || nP == 0)) return SFMI_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (nP > 0) SFMI_TRY(hipMemsetAsync(emask, 0, (size_t)nP * 4, st));
  if (nC > 0)
    hipLaunchKernelGGL(iso_mc_count_kernel, dim3(blocks256(nC)), dim3(256), 0, st, iso_lat(B, Q), cells, coff, flag, nC, pbits, prank, nP, emask, ntri);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_iso_mc_emit_f32(const int* cells, const int* coff, const unsigned char* flag, int nC, const int* pkeys, const int* poff, int nP,
                         const unsigned* pbits, const int* prank, const float* vals, float iso, const int* emask, const int* vincl,
                         const int* tincl, const int* voff, int B, int Q0, int L, int Q, float lo0, float lo1, float lo2, float hi0, float hi1,
                         float hi2, float* verts, int* faces, void* stream) {
  if (!iso_ok(B, Q0, L, Q) || nC < 0 || nP < 0 || !coff || !poff || !pbits || !prank || !voff || !verts || !faces) return SFMI_EINVAL;
  if (nP > 0 && (!pkeys || !vals || !emask || !vincl)) return SFMI_EINVAL;
  if (nC > 0 && (!cells || !flag || !tincl || nP == 0)) return SFMI_EINVAL;
  if (nP >= (1 << 30)) return SFMI_EINVAL;
  if (nC == 0 || nP == 0) return SFMI_OK;
  hipStream_t st = (hipStream_t)stream;
  const IsoLat g = iso_lat(B, Q);
  IsoBox box{{lo0, lo1, lo2}, {hi0, hi1, hi2}};
  hipLaunchKernelGGL(iso_mc_verts_kernel, dim3(blocks256(3ll * nP)), dim3(256), 0, st, g, pkeys, poff, nP, pbits, prank, vals, iso, emask, vincl, box,
                     verts);
  hipLaunchKernelGGL(iso_mc_faces_kernel, dim3(blocks256(nC)), dim3(256), 0, st, g, cells, coff, flag, nC, pbits, prank, nP, emask, vincl, tincl, voff,
                     faces);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

}  // extern "C"
