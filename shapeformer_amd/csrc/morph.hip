// Watertight voxelization of triangle soups on the device: point -> voxel scatter, exact binary morphology with a
// discrete ball, and a flood fill of the lattice from voxel (0,0,0).  The reference does this on one core with skimage:
// xgutils/geoutil.py:383-401 (morph_voxelization), xgutils/ptutil.py:425-450 (point2index), :520-550 (point2voxel).  The contract is in
// include/sfmi.h, its numpy / scipy statement in tests/morph_ref.py.
//
// A shape's grid is a bit set: word ((i*G + j)*Wz + k/32), bit k%32, Wz = ceil(G/32), [i][j][k] = x, y, z.  Pad bits (k >= G) are masked
// on every load and are 0 in every word written.
//   voxelize  one thread per point: the reference's f32 index, one atomicOr
//   dilate    zplanes: for every row word its z-dilations by h = 0..r (shifts and ORs with the two neighbouring words) into r+1 bit planes;
//             disc: every output word ORs plane floor(sqrt(r^2 - dx^2 - dy^2)) of row (i+dx, j+dy) over the disc dx^2 + dy^2 <= r^2.
//             invert_in / invert_out complement the grid on the way in / out: erode(M) = NOT dilate(NOT M), border counted as set
//   flood     the voxels whose value equals the seed voxel's are eligible.  The union-find of csrc/sfmi_ragged.h
//             over them; what is specific here is that a run of eligible bits inside a word is linked by its initial parents:
//               init    one thread per voxel: parent = the start of the voxel's run of eligible bits inside its word
//               hook    one thread per word: the run across the word boundary, and per forward row (4 of them) the links that the
//                       runs do not already imply (of the 13 forward neighbours of 26-connectivity)
//               region  one thread per word: a run belongs to the region iff its root is the shape's voxel 0 (the smallest index
//                       of the shape, so the root of its tree in whatever order the hooks came)
// Three launches for a flood whatever the grid holds; integer atomics only: every output is a function of the input bits.
#include "sfmi_ragged.h"

// the voxel index is the reference's f32 expression, one rounding per operation: no fused multiply-add
#pragma clang fp contract(off)

namespace {

constexpr int MORPH_MAX_R = 16;

// the lattice bits of word w of a row
__device__ __forceinline__ unsigned mv_valid(int w, int G) {
  const int n = G - w * 32;
  return n >= 32 ? 0xffffffffu : ((1u << n) - 1u);
}

// ptutil.point2index on one coordinate: clamp(round(((p + 1) / 2) * G - 0.5), 0, G - 1) in f32, round half to even
__device__ __forceinline__ int mv_index(float p, int G) {
  const float p01 = __fdiv_rn(__fadd_rn(p, 1.0f), 2.0f);
  const float s = __fsub_rn(__fmul_rn(p01, (float)G), 0.5f);
  return (int)fminf(fmaxf(rintf(s), 0.0f), (float)(G - 1));
}

__global__ __launch_bounds__(256) void mv_voxelize_kernel(const float* __restrict__ pts, const int* __restrict__ off, int B, int N, int G,
                                                          int Wz, unsigned* __restrict__ bits) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= N) return;
  const float x = pts[3ll * t], y = pts[3ll * t + 1], z = pts[3ll * t + 2];
  if (!(isfinite(x) && isfinite(y) && isfinite(z))) return;
  const int b = sfmi_owner(off, B, t);
  const int i = mv_index(x, G), j = mv_index(y, G), k = mv_index(z, G);
  // the result is not used: the atomic is issued and not waited for.  Testing the bit first (10^6 samples fall on ~10^5 voxels) puts a
  // load's latency in front of it and was slower on batches (profiles/r17_kbench_morph.txt)
  atomicOr(&bits[((b * G + i) * G + j) * Wz + (k >> 5)], 1u << (k & 31));
}

// out (N) uint8: the voxel of the cell that holds each point (0 for a non-finite point)
__global__ __launch_bounds__(256) void mv_lookup_kernel(const float* __restrict__ pts, const int* __restrict__ off, int B, int N, int G,
                                                        int Wz, const unsigned* __restrict__ bits, unsigned char* __restrict__ out) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= N) return;
  const float x = pts[3ll * t], y = pts[3ll * t + 1], z = pts[3ll * t + 2];
  unsigned char o = 0;
  if (isfinite(x) && isfinite(y) && isfinite(z)) {
    const int b = sfmi_owner(off, B, t);
    const int i = mv_index(x, G), j = mv_index(y, G), k = mv_index(z, G);
    o = (unsigned char)((bits[((b * G + i) * G + j) * Wz + (k >> 5)] >> (k & 31)) & 1u);
  }
  out[t] = o;
}

// one thread per word: planes[h * NW + t] = the row's bits dilated by h along z, h = 0..r
__global__ __launch_bounds__(256) void mv_zplanes_kernel(const unsigned* __restrict__ in, int G, int Wz, int NW, int r, int invert,
                                                         unsigned* __restrict__ planes) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= NW) return;
  const int w = t % Wz;
  const unsigned flip = invert ? 0xffffffffu : 0u;
  const unsigned cur = (in[t] ^ flip) & mv_valid(w, G);
  const unsigned prev = w > 0 ? ((in[t - 1] ^ flip) & mv_valid(w - 1, G)) : 0u;
  const unsigned next = w + 1 < Wz ? ((in[t + 1] ^ flip) & mv_valid(w + 1, G)) : 0u;
  unsigned acc = cur;
  planes[t] = acc;
  for (int h = 1; h <= r; ++h) {          // h <= 16: the shifts stay below 32
    acc |= (cur << h) | (prev >> (32 - h)) | (cur >> h) | (next << (32 - h));
    planes[(size_t)h * NW + t] = acc;
  }
}

// one thread per output word
__global__ __launch_bounds__(256) void mv_disc_kernel(const unsigned* __restrict__ planes, int G, int Wz, int NW, int r, int invert,
                                                      unsigned* __restrict__ out) {
  __shared__ signed char hh[(2 * MORPH_MAX_R + 1) * (2 * MORPH_MAX_R + 1)];
  const int side = 2 * r + 1;
  for (int e = threadIdx.x; e < side * side; e += 256) {
    const int dx = e / side - r, dy = e % side - r;
    const int rem = r * r - dx * dx - dy * dy;
    int h = -1;
    if (rem >= 0) { h = 0; while ((h + 1) * (h + 1) <= rem) ++h; }
    hh[e] = (signed char)h;
  }
  __syncthreads();
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= NW) return;
  const int w = t % Wz, row = t / Wz, j = row % G, i = (row / G) % G;
  unsigned acc = 0u;
  const int dx0 = max(-r, -i), dx1 = min(r, G - 1 - i), dy0 = max(-r, -j), dy1 = min(r, G - 1 - j);
  for (int dx = dx0; dx <= dx1; ++dx) {
    const signed char* hrow = hh + (dx + r) * side + r;
    for (int dy = dy0; dy <= dy1; ++dy) {
      const int h = hrow[dy];
      if (h >= 0) acc |= planes[(size_t)h * NW + (t + (dx * G + dy) * Wz)];
    }
  }
  if (invert) acc = ~acc;
  out[t] = acc & mv_valid(w, G);
}

// the eligible bits of word t (word w of its row): the lattice bits whose value is the seed voxel's
__device__ __forceinline__ unsigned mv_elig(const unsigned* __restrict__ in, int t, int w, int G, unsigned seed) {
  return (seed ? in[t] : ~in[t]) & mv_valid(w, G);
}

// one thread per voxel v = row * G + k: parent = the start of its run of eligible bits inside its word (itself where it is not eligible:
// such a slot is never read)
__global__ __launch_bounds__(256) void mv_flood_init_kernel(const unsigned* __restrict__ in, int G, int Wz, int NV, int* __restrict__ parent) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= NV) return;
  const int row = v / G, k = v - row * G, w = k >> 5, kb = k & 31;
  const int shape_word = (row / (G * G)) * (G * G * Wz);
  const unsigned seed = in[shape_word] & 1u;
  const unsigned e = mv_elig(in, row * Wz + w, w, G, seed);
  int p = v;
  if ((e >> kb) & 1u) {
    const unsigned zeros_below = ~e & ((1u << kb) - 1u);
    const int start = zeros_below ? 32 - __clz(zeros_below) : 0;
    p = v - (kb - start);
  }
  parent[v] = p;
}

// one thread per word.  For a forward row with eligible bits N (Nm / Np: N seen from k-1 / k+1) and own bits E (Em / Ep likewise), voxel k
// links to the row's k where both are eligible unless the pair at k-1 is eligible too (it links, and both runs carry the link on);
// where the row's k is not eligible, to k-1 / k+1 unless the own neighbour at k-1 / k+1 is eligible (its pair links)
__global__ __launch_bounds__(256) void mv_flood_hook_kernel(const unsigned* __restrict__ in, int G, int Wz, int NW, int* parent) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= NW) return;
  const int w = t % Wz, row = t / Wz, j = row % G, i = (row / G) % G;
  const unsigned seed = in[(row / (G * G)) * (G * G * Wz)] & 1u;
  const unsigned E = mv_elig(in, t, w, G, seed);
  if (!E) return;
  const unsigned Eprev = w > 0 ? mv_elig(in, t - 1, w - 1, G, seed) : 0u;
  const unsigned Enext = w + 1 < Wz ? mv_elig(in, t + 1, w + 1, G, seed) : 0u;
  const unsigned Em = (E << 1) | (Eprev >> 31), Ep = (E >> 1) | (Enext << 31);
  const int v0 = row * G + w * 32;
  if ((E & 1u) && (Eprev >> 31)) sfmi_uf_hook(parent, v0, v0 - 1);
  const int DI[4] = {0, 1, 1, 1}, DJ[4] = {1, -1, 0, 1};
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    const int ii = i + DI[n], jj = j + DJ[n];
    if (ii >= G || jj < 0 || jj >= G) continue;
    const int d = DI[n] * G + DJ[n];
    const int nt = t + d * Wz, n0 = v0 + d * G;
    const unsigned N = mv_elig(in, nt, w, G, seed);
    const unsigned Nprev = w > 0 ? mv_elig(in, nt - 1, w - 1, G, seed) : 0u;
    const unsigned Nnext = w + 1 < Wz ? mv_elig(in, nt + 1, w + 1, G, seed) : 0u;
    const unsigned Nm = (N << 1) | (Nprev >> 31), Np = (N >> 1) | (Nnext << 31);
    unsigned H0 = E & N & ~(Em & Nm), Hm = E & Nm & ~N & ~Em, Hp = E & Np & ~N & ~Ep;
    while (H0) { const int k = __ffs(H0) - 1; H0 &= H0 - 1; sfmi_uf_hook(parent, v0 + k, n0 + k); }
    while (Hm) { const int k = __ffs(Hm) - 1; Hm &= Hm - 1; sfmi_uf_hook(parent, v0 + k, n0 + k - 1); }
    while (Hp) { const int k = __ffs(Hp) - 1; Hp &= Hp - 1; sfmi_uf_hook(parent, v0 + k, n0 + k + 1); }
  }
}

// one thread per word; parent is only read here.  status (B): 3 where the seed voxel is set
__global__ __launch_bounds__(256) void mv_flood_region_kernel(const unsigned* __restrict__ in, const int* __restrict__ parent, int G, int Wz,
                                                              int NW, unsigned* __restrict__ region, int* __restrict__ status) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= NW) return;
  const int w = t % Wz, row = t / Wz, b = row / (G * G);
  const int shape_word = b * (G * G * Wz), root0 = b * (G * G * G);
  const unsigned seed = in[shape_word] & 1u;
  if (t == shape_word) status[b] = seed ? 3 : 0;
  unsigned m = mv_elig(in, t, w, G, seed), out = 0u;
  const int v0 = row * G + w * 32;
  while (m) {
    const int s = __ffs(m) - 1;
    const unsigned x = ~(m >> s);                       // the first 0 above s ends the run
    const int len = x ? __ffs(x) - 1 : 32;
    const unsigned mask = (len >= 32 ? 0xffffffffu : ((1u << len) - 1u)) << s;
    int rt = v0 + s, p = parent[rt];
    while (p != rt) { rt = p; p = parent[rt]; }
    if (rt == root0) out |= mask;
    m &= ~mask;
  }
  region[t] = out;
}

// one thread per word: bit k = (vox != 0)
__global__ __launch_bounds__(256) void mv_pack_kernel(const unsigned char* __restrict__ vox, int G, int Wz, int NW, unsigned* __restrict__ bits) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= NW) return;
  const int w = t % Wz, row = t / Wz, n = min(32, G - w * 32);
  const unsigned char* src = vox + (size_t)row * G + w * 32;
  unsigned x = 0u;
  for (int k = 0; k < n; ++k) x |= (src[k] ? 1u : 0u) << k;
  bits[t] = x;
}

// one thread per voxel
__global__ __launch_bounds__(256) void mv_unpack_kernel(const unsigned* __restrict__ bits, int G, int Wz, int NV, unsigned char* __restrict__ vox) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= NV) return;
  const int row = v / G, k = v - row * G;
  vox[v] = (unsigned char)((bits[row * Wz + (k >> 5)] >> (k & 31)) & 1u);
}

inline bool mv_sizes(int B, int G) { return B > 0 && G > 0 && (long long)B * G * G * G < (1ll << 31); }
inline int mv_wz(int G) { return (G + 31) / 32; }

}  // namespace

extern "C" {

int sfmi_morph_max_radius(void) { return MORPH_MAX_R; }

long long sfmi_morph_words(int B, int G) { return mv_sizes(B, G) ? (long long)B * G * G * mv_wz(G) : 0; }

size_t sfmi_morph_workspace_bytes(int B, int G, int r) {
  if (!mv_sizes(B, G) || r < 0 || r > MORPH_MAX_R) return 0;
  const size_t planes = (size_t)(r + 1) * (size_t)B * G * G * mv_wz(G) * 4, parent = (size_t)B * G * G * G * 4;
  return planes > parent ? planes : parent;
}

int sfmi_voxelize_points_f32(const float* points, const int* off, int B, long long N, int G, unsigned* bits, void* stream) {
  if (!mv_sizes(B, G) || N < 0 || 3 * N >= (1ll << 31) || !off || !bits || (N > 0 && !points)) return SFMI_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int Wz = mv_wz(G);
  SFMI_TRY(hipMemsetAsync(bits, 0, (size_t)B * G * G * Wz * 4, st));
  if (N > 0) hipLaunchKernelGGL(mv_voxelize_kernel, dim3(blocks256(N)), dim3(256), 0, st, points, off, B, (int)N, G, Wz, bits);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_voxelize_lookup_f32(const float* points, const int* off, int B, long long N, int G, const unsigned* bits, unsigned char* out,
                             void* stream) {
  if (!mv_sizes(B, G) || N < 0 || 3 * N >= (1ll << 31) || !off || !bits || (N > 0 && (!points || !out))) return SFMI_EINVAL;
  if (N == 0) return SFMI_OK;
  hipLaunchKernelGGL(mv_lookup_kernel, dim3(blocks256(N)), dim3(256), 0, (hipStream_t)stream, points, off, B, (int)N, G, mv_wz(G), bits, out);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_morph_dilate_u32(const unsigned* in, int B, int G, int r, int invert_in, int invert_out, unsigned* out, void* ws, void* stream) {
  if (!mv_sizes(B, G) || r < 0 || r > MORPH_MAX_R || !in || !out || !ws) return SFMI_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int Wz = mv_wz(G), NW = B * G * G * Wz;
  hipLaunchKernelGGL(mv_zplanes_kernel, dim3(blocks256(NW)), dim3(256), 0, st, in, G, Wz, NW, r, invert_in ? 1 : 0, (unsigned*)ws);
  hipLaunchKernelGGL(mv_disc_kernel, dim3(blocks256(NW)), dim3(256), 0, st, (const unsigned*)ws, G, Wz, NW, r, invert_out ? 1 : 0, out);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_morph_flood_u32(const unsigned* in, int B, int G, unsigned* region, int* status, void* ws, void* stream) {
  if (!mv_sizes(B, G) || !in || !region || !status || !ws || in == region) return SFMI_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int Wz = mv_wz(G), NW = B * G * G * Wz, NV = B * G * G * G;
  int* parent = (int*)ws;
  hipLaunchKernelGGL(mv_flood_init_kernel, dim3(blocks256(NV)), dim3(256), 0, st, in, G, Wz, NV, parent);
  hipLaunchKernelGGL(mv_flood_hook_kernel, dim3(blocks256(NW)), dim3(256), 0, st, in, G, Wz, NW, parent);
  hipLaunchKernelGGL(mv_flood_region_kernel, dim3(blocks256(NW)), dim3(256), 0, st, in, (const int*)parent, G, Wz, NW, region, status);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_morph_pack_u8(const unsigned char* vox, int B, int G, unsigned* bits, void* stream) {
  if (!mv_sizes(B, G) || !vox || !bits) return SFMI_EINVAL;
  const int Wz = mv_wz(G), NW = B * G * G * Wz;
  hipLaunchKernelGGL(mv_pack_kernel, dim3(blocks256(NW)), dim3(256), 0, (hipStream_t)stream, vox, G, Wz, NW, bits);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_morph_unpack_u8(const unsigned* bits, int B, int G, unsigned char* vox, void* stream) {
  if (!mv_sizes(B, G) || !vox || !bits) return SFMI_EINVAL;
  const int NV = B * G * G * G;
  hipLaunchKernelGGL(mv_unpack_kernel, dim3(blocks256(NV)), dim3(256), 0, (hipStream_t)stream, bits, G, mv_wz(G), NV, vox);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

}  // extern "C"
