// Mesh signed distance and occupancy on the GPU: the data-preparation half of the mesh story (a user's meshes -> an IMNet2-style
// store of surface samples and lattice occupancy).  The reference does this on the CPU with libigl: igl.signed_distance in
// xgutils/geoutil.py:265-269 (signed_distance), :282-291 (mesh2sdf on the makeGrid 'ij' lattice) and :455-490 (SDF_sampling),
// chained by shapeformer/data/imnet_datasets/utils.py:33-70.  Here every query is exact brute force over the faces of its mesh.
//
// 1. Setup: one thread per face packs a 5 x float4 record into the workspace and validates the face's vertex indices;
//    one workgroup per shape then turns the per-face flags into the shape's status (no atomics).
//      r0 = (a, |ab|^2)   r1 = (ab, ab.ac)   r2 = (ac, |ac|^2)   r3 = (b, wt)   r4 = (c, bad)
//    A degenerate face (zero area: repeated vertex, collinear vertices, or a width below 2^-22 of its longest edge) is stored
//    as the segment of its longest edge, (P, Q-P, 0), for which the region form below yields exactly the closest point of the
//    segment (or of the point when P == Q), and with wt = 0: it adds nothing to the winding number.
// 2. Main launch (grid: query blocks x S face chunks): 256 lanes x SD_R queries per lane in registers; face records through an
//    LDS tile, read as broadcasts (every lane the same address).  Per pair:
//    - closest point: Ericson's region form (Real-Time Collision Detection 5.1.5) with the regions turned into selects in
//      reverse priority (interior, BC, AC, C, AB, B, A): one reciprocal, no branches;
//    - d2 = fmaf(dz,dz,fmaf(dy,dy,dx*dx)) of q - C; faces scanned in ascending order with a strict `<` (lowest face wins a tie);
//    - solid angle (van Oosterom & Strackee 1983): tan(Omega/2) = a.(b x c) / (|a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|)
//      with a, b, c relative to q; W = sum Omega / 4 pi.  The sum is taken in f32 over runs of SD_WRUN faces aligned to the
//      shape's first face, and the runs are added as 2^-29 fixed-point integers: integer addition is associative, so W does not
//      depend on where the chunks are cut, and a shape in a batch gets the bits it gets alone.
//    The occupancy (lattice) instance needs only the sign: it skips the closest point and generates its queries from the
//    lattice index (makeGrid 'on' mode, numpy linspace in f64, then f32).
// 3. Merge launch, always: chunk minima in ascending chunk order with a strict `<`, the integer W partials added up,
//    C recomputed from the winning face, the sign applied, bad shapes overwritten.  Nothing depends on S.
#include "sfmi_ragged.h"   // the ragged-batch helpers the mesh tools share: DESIGN.md §5.5a
#include "sfmi_triangle.h" // closest_vw, half_solid_angle, sfmi_pack_face: shared with csrc/meshtree.hip

namespace {

constexpr int SD_THREADS = 256;
constexpr int SD_TILE = 256;                     // faces per LDS tile
constexpr int SD_REC = SFMI_FACE_REC;            // float4 per face record
constexpr int SD_TARGET_BLOCKS = 2048;           // 256 CUs x 8 workgroups
constexpr int SD_MAX_SPLITS = 64;
constexpr int SD_MIN_CHUNK = 64;                 // fewest faces (on average) per chunk
constexpr int SD_WRUN = 64;                      // faces per f32 run of the winding sum; chunks are cut at its multiples

template <bool OCC> struct SdR { static constexpr int R = 4; };       // queries per lane: full form
template <> struct SdR<true> { static constexpr int R = 8; };         // winding number only

inline long long sd_qblocks(int B, long long N, int R) { return cdiv(N, (long long)SD_THREADS * R) + B; }

inline int sd_splits(int B, long long N, long long T, int R) {
  long long s = cdiv(SD_TARGET_BLOCKS, sd_qblocks(B, N, R));
  const long long by_t = T / ((long long)B * SD_MIN_CHUNK);
  if (s > by_t) s = by_t;
  if (s > SD_MAX_SPLITS) s = SD_MAX_SPLITS;
  return s < 1 ? 1 : (int)s;
}

// ---- setup ------------------------------------------------------------------------------------------------------------------

__global__ void sdf_setup_kernel(const float* __restrict__ verts, const int* __restrict__ faces, const long long* __restrict__ voff,
                                 const long long* __restrict__ toff, int B, long long T, float4* __restrict__ rec) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= T) return;
  const int b = sfmi_owner(toff, B, t);
  const long long v0 = voff[b], nv = voff[b + 1] - v0;
  float p[3][3];
  bool ok = true;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int k = faces[3 * t + c];
    const bool in = k >= 0 && k < nv;
    ok = ok && in;
    const long long v = v0 + (in ? k : 0);
#pragma unroll
    for (int a = 0; a < 3; ++a) p[c][a] = in ? verts[3 * v + a] : 0.f;
  }
  float4* r = rec + SD_REC * t;
  if (!ok) {
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    r[0] = z; r[1] = z; r[2] = z; r[3] = z;
    r[4] = make_float4(0.f, 0.f, 0.f, 1.f);
    return;
  }
  sfmi_pack_face(p, r);
}

// one workgroup per shape: status[b] = 1 (no faces), 2 (a vertex index outside the shape) or 0
constexpr int ST_THREADS = 256;
__global__ __launch_bounds__(ST_THREADS) void sdf_status_kernel(const long long* __restrict__ toff, const float4* __restrict__ rec,
                                                               int* __restrict__ status) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const long long t0 = toff[b], t1 = toff[b + 1];
  int bad = 0;
  for (long long t = t0 + tid; t < t1; t += ST_THREADS) bad |= rec[SD_REC * t + 4].w != 0.f;
  bad = __syncthreads_or(bad);
  if (tid == 0) status[b] = t1 <= t0 ? 1 : (bad ? 2 : 0);
}

// query-block offsets of ragged query sets (one lane; B is small)
__global__ void sdf_block_offsets_kernel(const long long* __restrict__ qoff, long long* __restrict__ block_off, int B, int QB) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  long long acc = 0;
  for (int b = 0; b < B; ++b) {
    block_off[b] = acc;
    acc += cdiv(qoff[b + 1] - qoff[b], QB);
  }
  block_off[B] = acc;
}

// ---- main launch ------------------------------------------------------------------------------------------------------------

// grid (query blocks upper bound, S).  Writes the chunk partials: pd / pi (full form) and pw at chunk s, offset s * N.
// OCC: the queries are the G^3 lattice points of every shape (N = B G^3, qoff unused, block_off unused).
// amdgpu_waves_per_eu(4): with the integer partials the full form would otherwise take 136 VGPRs and lose the fourth wave per SIMD
template <bool OCC>
__global__ __launch_bounds__(SD_THREADS) __attribute__((amdgpu_waves_per_eu(4))) void sdf_kernel(const float* __restrict__ Q, const long long* __restrict__ qoff,
                                                          const long long* __restrict__ toff, const float4* __restrict__ rec,
                                                          const long long* __restrict__ block_off, int B, long long N, Lattice lat,
                                                          float* __restrict__ pd, int* __restrict__ pi, long long* __restrict__ pw) {
  constexpr int R = SdR<OCC>::R;
  constexpr int QB = SD_THREADS * R;
  constexpr int NREC = OCC ? 3 : SD_REC;                      // OCC: a, b, c only (r0, r3, r4)
  __shared__ float4 tile[NREC][SD_TILE];
  const long long g = blockIdx.x;
  int b;
  long long qbase, pend;
  const long long G3 = (long long)lat.G * lat.G * lat.G;
  if (OCC) {
    const long long per = cdiv(G3, QB);
    if (g >= per * B) return;                                 // block-uniform: the grid is an upper bound
    b = (int)(g / per);
    qbase = (long long)b * G3 + (g - (long long)b * per) * QB;
    pend = (long long)(b + 1) * G3;
  } else {
    if (g >= block_off[B]) return;
    b = sfmi_owner(block_off, B, g);
    qbase = qoff[b] + (g - block_off[b]) * QB;
    pend = qoff[b + 1];
  }
  const int tid = threadIdx.x;
  float qx[R], qy[R], qz[R], best[R], wsum[R];
  long long wacc[R];
  int bi[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const long long i = qbase + r * SD_THREADS + tid;
    const bool ok = i < pend;
    if (OCC) {
      const long long k = ok ? i - (long long)b * G3 : 0;
      const long long G = lat.G, ix = k / (G * G), iy = (k / G) % G, iz = k % G;
      qx[r] = lattice_coord(lat, 0, ix);
      qy[r] = lattice_coord(lat, 1, iy);
      qz[r] = lattice_coord(lat, 2, iz);
    } else {
      qx[r] = ok ? Q[3 * i] : 0.f;
      qy[r] = ok ? Q[3 * i + 1] : 0.f;
      qz[r] = ok ? Q[3 * i + 2] : 0.f;
    }
    best[r] = INFINITY;
    bi[r] = -1;
    wsum[r] = 0.f;
    wacc[r] = 0;
  }
  const long long t0b = toff[b], t1b = toff[b + 1];
  const long long chunk = cdiv(cdiv(t1b - t0b, (long long)gridDim.y), (long long)SD_WRUN) * SD_WRUN;   // tiles start at multiples of SD_WRUN
  const long long j0 = t0b + (long long)blockIdx.y * chunk;
  const long long j1 = j0 + chunk < t1b ? j0 + chunk : t1b;
  for (long long t0 = j0; t0 < j1; t0 += SD_TILE) {
    __syncthreads();                                          // the previous tile is consumed
    const int nt = (int)(j1 - t0 < SD_TILE ? j1 - t0 : SD_TILE);
    if (tid < nt) {
      const float4* src = rec + SD_REC * (t0 + tid);
      if (OCC) {
        tile[0][tid] = src[0];
        tile[1][tid] = src[3];
        tile[2][tid] = src[4];
      } else {
#pragma unroll
        for (int k = 0; k < SD_REC; ++k) tile[k][tid] = src[k];
      }
    }
    __syncthreads();
    const int jb = (int)(t0 - t0b);                           // local index of the tile's first face (T_b < 2^31)
    for (int j0r = 0; j0r < nt; j0r += SD_WRUN) {             // nt is block-uniform: no divergence
      const int j1r = j0r + SD_WRUN < nt ? j0r + SD_WRUN : nt;
      for (int jj = j0r; jj < j1r; ++jj) {
        if (OCC) {
          const float4 a = tile[0][jj], bb = tile[1][jj], c = tile[2][jj];   // broadcast reads
#pragma unroll
          for (int r = 0; r < R; ++r) wsum[r] = fmaf(bb.w, half_solid_angle(qx[r], qy[r], qz[r], a, bb, c), wsum[r]);
        } else {
          const float4 r0 = tile[0][jj], r1 = tile[1][jj], r2 = tile[2][jj], r3 = tile[3][jj], r4 = tile[4][jj];
#pragma unroll
          for (int r = 0; r < R; ++r) {
            float v, w;
            const float d2 = closest_vw(qx[r], qy[r], qz[r], r0, r1, r2, v, w);
            const bool lt = d2 < best[r];
            best[r] = lt ? d2 : best[r];
            bi[r] = lt ? jb + jj : bi[r];
            wsum[r] = fmaf(r3.w, half_solid_angle(qx[r], qy[r], qz[r], r0, r3, r4), wsum[r]);
          }
        }
      }
#pragma unroll
      for (int r = 0; r < R; ++r) w_flush(wsum[r], wacc[r]);
    }
  }
  const long long so = (long long)blockIdx.y * N;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const long long i = qbase + r * SD_THREADS + tid;
    if (i < pend) {
      pw[so + i] = wacc[r];
      if (!OCC) {
        pd[so + i] = best[r];
        pi[so + i] = bi[r];
      }
    }
  }
}

// ---- merge ------------------------------------------------------------------------------------------------------------------

__global__ void sdf_merge_kernel(const float* __restrict__ Q, const long long* __restrict__ qoff, const long long* __restrict__ toff,
                                 const float4* __restrict__ rec, const int* __restrict__ status, int B, long long N, int S,
                                 const float* __restrict__ pd, const int* __restrict__ pi, const long long* __restrict__ pw,
                                 float* __restrict__ Sd, int* __restrict__ I, float* __restrict__ C, float* __restrict__ W) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int b = sfmi_owner(qoff, B, i);
  const float nan = __int_as_float(0x7FC00000);
  if (status[b] != 0) {
    Sd[i] = nan;
    if (I) I[i] = -1;
    if (C) C[3 * i] = C[3 * i + 1] = C[3 * i + 2] = nan;
    if (W) W[i] = 0.f;
    return;
  }
  float best = pd[i];
  long long ws = 0;
  bool bad = false;
  w_add(pw[i], ws, bad);
  int bi = pi[i];
  for (int s = 1; s < S; ++s) {
    const float d = pd[(long long)s * N + i];
    const int k = pi[(long long)s * N + i];
    if (d < best) { best = d; bi = k; }
    w_add(pw[(long long)s * N + i], ws, bad);
  }
  const float wn = w_value(ws, bad) * INV_2PI;
  Sd[i] = fabsf(wn) > 0.5f ? -sqrtf(best) : sqrtf(best);
  if (I) I[i] = bi;
  if (W) W[i] = wn;
  if (C) {
    const float qx = Q[3 * i], qy = Q[3 * i + 1], qz = Q[3 * i + 2];
    const float4* r = rec + SD_REC * (toff[b] + (bi >= 0 ? bi : 0));   // bi >= 0: status 0 means T_b > 0 and finite d2
    float v, w;
    closest_vw(qx, qy, qz, r[0], r[1], r[2], v, w);
    C[3 * i] = fmaf(w, r[2].x, fmaf(v, r[1].x, r[0].x));
    C[3 * i + 1] = fmaf(w, r[2].y, fmaf(v, r[1].y, r[0].y));
    C[3 * i + 2] = fmaf(w, r[2].z, fmaf(v, r[1].z, r[0].z));
  }
}

__global__ void occ_merge_kernel(const int* __restrict__ status, long long G3, long long N, int S, const long long* __restrict__ pw,
                                 unsigned char* __restrict__ occ) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  long long ws = 0;
  bool bad = false;
  for (int s = 0; s < S; ++s) w_add(pw[(long long)s * N + i], ws, bad);
  occ[i] = (status[i / G3] == 0 && fabsf(w_value(ws, bad) * INV_2PI) > 0.5f) ? 1 : 0;
}

// ---- SDF_sampling's jitter --------------------------------------------------------------------------------------------------

// one thread per coordinate of B*n points: normal(seed, k, axis) * (k < n_near ? near_std : far_std); outside +-0.99 -> uniform
// in [-1, 1); then clipped to +-0.99.  Sample k of a shape depends on (seed, k) only.
__global__ void sdf_jitter_kernel(const float* __restrict__ X, int B, long long n, long long n_near, float near_std, float far_std,
                                  unsigned long long seed, float* __restrict__ out) {
  const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (long long)B * n * 3) return;
  const long long p = g / 3, k = p % n;
  const int a = (int)(g - 3 * p);
  const unsigned long long s0 = sfmi_mix64(seed), base = 9 * (unsigned long long)k + 3 * (unsigned long long)a;
  const unsigned long long h1 = sfmi_mix64(s0 + base), h2 = sfmi_mix64(s0 + base + 1), h3 = sfmi_mix64(s0 + base + 2);
  const float u1 = (float)((h1 >> 40) + 1) * 0x1.0p-24f;     // (0, 1]
  const float u2 = (float)(h2 >> 40) * 0x1.0p-24f;           // [0, 1)
  const float z = sqrtf(-2.f * logf(u1)) * cospif(2.f * u2);
  float x = fmaf(k < n_near ? near_std : far_std, z, X[g]);
  if (x > 0.99f || x < -0.99f) x = fmaf((float)(h3 >> 40), 0x1.0p-23f, -1.f);
  out[g] = fminf(fmaxf(x, -0.99f), 0.99f);
}

struct SdWs { int splits; long long* block_off; float4* rec; long long* pw; float* pd; int* pi; };   // pd, pi: full form only

// workspace: block offsets (B+1 int64) | face records (T x 80 B) | W partials (S*N int64) | full form: d2, idx partials (S*N each)
// occ: the occupancy form, whose sections are the first three of the full form at the same offsets (its S differs)
SdWs sdf_ws(SfmiCarver& c, int B, long long N, long long T, bool occ) {
  const int S = sd_splits(B, N, T, occ ? SdR<true>::R : SdR<false>::R);
  const size_t sn = (size_t)S * N;
  SdWs w{S, c.take<long long>((size_t)(B + 1)), c.take<float4>((size_t)(T > 0 ? T : 1) * SD_REC), c.take<long long>(sn), nullptr,
         nullptr};
  if (!occ) {
    w.pd = c.take<float>(sn);
    w.pi = c.take<int>(sn);
  }
  return w;
}

}  // namespace

extern "C" {

size_t sfmi_mesh_sdf_workspace_bytes(int B, long long N, long long T) {
  if (B <= 0 || N < 0 || T < 0) return 0;
  const size_t full = sfmi_ws_bytes(sdf_ws, B, N, T, false), occ = sfmi_ws_bytes(sdf_ws, B, N, T, true);
  return full > occ ? full : occ;                              // the caller's buffer serves either form
}

int sfmi_mesh_sdf_f32(const float* Q, const long long* qoff, const float* verts, const int* faces, const long long* voff,
                      const long long* toff, int B, long long N, long long T, float* S, int* I, float* C, float* W, int* status,
                      void* workspace, void* stream) {
  if (B <= 0 || N < 0 || T < 0 || T >= (1ll << 31) || !qoff || !voff || !toff || !status || !workspace) return SFMI_EINVAL;
  if (T > 0 && (!verts || !faces)) return SFMI_EINVAL;
  if (N > 0 && (!Q || !S)) return SFMI_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  SfmiCarver carver{(char*)workspace};
  const SdWs w = sdf_ws(carver, B, N, T, false);
  if (T > 0) hipLaunchKernelGGL(sdf_setup_kernel, dim3((unsigned)cdiv(T, 256)), dim3(256), 0, st, verts, faces, voff, toff, B, T, w.rec);
  hipLaunchKernelGGL(sdf_status_kernel, dim3((unsigned)B), dim3(ST_THREADS), 0, st, toff, (const float4*)w.rec, status);
  if (N > 0) {
    constexpr int QB = SD_THREADS * SdR<false>::R;
    hipLaunchKernelGGL(sdf_block_offsets_kernel, dim3(1), dim3(64), 0, st, qoff, w.block_off, B, QB);
    const dim3 grid((unsigned)sd_qblocks(B, N, SdR<false>::R), (unsigned)w.splits);
    Lattice lat{};
    hipLaunchKernelGGL(sdf_kernel<false>, grid, dim3(SD_THREADS), 0, st, Q, qoff, toff, (const float4*)w.rec,
                       (const long long*)w.block_off, B, N, lat, w.pd, w.pi, w.pw);
    hipLaunchKernelGGL(sdf_merge_kernel, dim3((unsigned)cdiv(N, 256)), dim3(256), 0, st, Q, qoff, toff, (const float4*)w.rec,
                       (const int*)status, B, N, w.splits, (const float*)w.pd, (const int*)w.pi, (const long long*)w.pw, S, I, C, W);
  }
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_mesh_occupancy_f32(const float* verts, const int* faces, const long long* voff, const long long* toff, int B, long long T,
                            int G, const double* lo, const double* hi, unsigned char* occ, int* status, void* workspace, void* stream) {
  if (B <= 0 || T < 0 || T >= (1ll << 31) || G <= 0 || !lo || !hi || !voff || !toff || !status || !workspace || !occ) return SFMI_EINVAL;
  if (T > 0 && (!verts || !faces)) return SFMI_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const long long G3 = (long long)G * G * G, N = (long long)B * G3;
  SfmiCarver carver{(char*)workspace};
  const SdWs w = sdf_ws(carver, B, N, T, true);
  Lattice lat;
  lat.G = G;
  for (int a = 0; a < 3; ++a) {
    lat.lo[a] = lo[a];
    lat.hi[a] = hi[a];
    lat.step[a] = G > 1 ? (hi[a] - lo[a]) / (double)(G - 1) : 0.0;
  }
  if (T > 0) hipLaunchKernelGGL(sdf_setup_kernel, dim3((unsigned)cdiv(T, 256)), dim3(256), 0, st, verts, faces, voff, toff, B, T, w.rec);
  hipLaunchKernelGGL(sdf_status_kernel, dim3((unsigned)B), dim3(ST_THREADS), 0, st, toff, (const float4*)w.rec, status);
  constexpr int QB = SD_THREADS * SdR<true>::R;
  const dim3 grid((unsigned)(cdiv(G3, QB) * B), (unsigned)w.splits);
  hipLaunchKernelGGL(sdf_kernel<true>, grid, dim3(SD_THREADS), 0, st, (const float*)nullptr, (const long long*)nullptr, toff,
                     (const float4*)w.rec, (const long long*)nullptr, B, N, lat, (float*)nullptr, (int*)nullptr, w.pw);
  hipLaunchKernelGGL(occ_merge_kernel, dim3((unsigned)cdiv(N, 256)), dim3(256), 0, st, (const int*)status, G3, N, w.splits,
                     (const long long*)w.pw, occ);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_sdf_jitter_f32(const float* X, int B, long long n, long long n_near, float near_std, float far_std, unsigned long long seed,
                        float* out, void* stream) {
  if (B <= 0 || n < 0 || n_near < 0 || n_near > n || (n > 0 && (!X || !out))) return SFMI_EINVAL;
  if (n == 0) return SFMI_OK;
  hipLaunchKernelGGL(sdf_jitter_kernel, dim3((unsigned)cdiv((long long)B * n * 3, 256)), dim3(256), 0, (hipStream_t)stream, X, B, n, n_near,
                     near_std, far_std, seed, out);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

}  // extern "C"
