// Smooth fields from binary voxel grids on the device: the exact squared Euclidean distance transform, the signed
// distance, a separable Gaussian filter and a constrained smoothing solve in a narrow band (Lempitsky, CVPR 2010).  The reference does
// this on one core inside array2mesh: xgutils/geoutil.py:194-197 (mcubes.smooth in front of marching cubes).  The contract is in
// include/sfmi.h, its numpy / scipy statement in tests/voxfield_ref.py.
//
// Grids are morph.hip's bit sets: word ((b*G + i)*G + j)*Wz + k/32, bit k%32; pad bits are masked on every load.
//   edt     k     one thread per voxel: the nearest set bit of its row below and above, by clz / ffs over the row's words -> g^2
//           j, i  one thread per line, neighbouring lanes on neighbouring k: the integer lower envelope of sfmi_edt_line.h, its two
//                 uint16 stacks in the workspace laid out like the grid, so that every access of a wave is one run of addresses
//           finish  one thread per voxel: "no set voxel" becomes 3 G^2, and the status.  Four launches whatever the grid holds
//   signed  the two transforms (clear voxels, set voxels) and one launch that takes the square roots in f64
//   gauss   three launches, one thread per voxel: the axis-0 pass reads the bits, every pass sums the taps in scipy's order
//   solve   flag (band and its one-step support, per-chunk counts) -> scan of the chunk counts by one workgroup -> emit (ranks from wave
//           ballots: ascending flat index) and then, per iteration, L u over the support and the projected step over the band: two
//           launches over the lists, a fixed grid that strides over a count it reads on the device.  Nothing is read back.
// Integer and f64 arithmetic in a fixed order, no atomics: every output is a function of the input bits.
#include "sfmi_ragged.h"
#include "sfmi_edt_line.h"

// every f64 operation of the contract is rounded on its own
#pragma clang fp contract(off)

namespace {

constexpr int VF_MAX_G = 513, VF_MAX_RADIUS = 64;
constexpr int VF_CHUNK = 4096;                 // voxels per workgroup of the compaction: 16 rounds of 256
constexpr int VF_SCAN_THREADS = 1024;
constexpr unsigned VF_ITER_GRID = 2048;        // workgroups of an iteration's launches: they stride over the lists

inline bool vf_sizes(int B, int G) { return B > 0 && G >= 1 && G <= VF_MAX_G && (long long)B * G * G * G < (1ll << 31); }
inline int vf_wz(int G) { return (G + 31) / 32; }

// the lattice bits of word w of a row
__device__ __forceinline__ unsigned vf_valid(int w, int G) {
  const int n = G - w * 32;
  return n >= 32 ? 0xffffffffu : ((1u << n) - 1u);
}

__device__ __forceinline__ int vf_bit(const unsigned* __restrict__ bits, int v, int G, int Wz) {
  const int row = v / G, k = v - row * G;
  return (int)((bits[(size_t)row * Wz + (k >> 5)] >> (k & 31)) & 1u);
}

// ---- distance transform ---------------------------------------------------------------------------------------------------------------

// one thread per voxel: (distance to the nearest set voxel of the row)^2, SFMI_EDT_INF for a row without one
__global__ __launch_bounds__(256) void edt_k_kernel(const unsigned* __restrict__ bits, int G, int Wz, int NV, int invert, int* __restrict__ out) {
  const unsigned vu = blockIdx.x * 256u + threadIdx.x;      // unsigned: the last workgroup may reach past 2^31
  if (vu >= (unsigned)NV) return;
  const int v = (int)vu;
  const int row = v / G, k = v - row * G, w = k >> 5, kb = k & 31;
  const unsigned* __restrict__ words = bits + (size_t)row * Wz;
  const unsigned flip = invert ? 0xffffffffu : 0u;
  int g = G;                                                   // larger than any distance inside the row
  unsigned m = ((words[w] ^ flip) & vf_valid(w, G)) & (0xffffffffu >> (31 - kb));
  for (int ww = w;;) {
    if (m) { g = k - (ww * 32 + 31 - __clz(m)); break; }
    if (--ww < 0) break;
    m = (words[ww] ^ flip) & vf_valid(ww, G);
  }
  m = ((words[w] ^ flip) & vf_valid(w, G)) & (0xffffffffu << kb);
  for (int ww = w;;) {
    if (m) { g = min(g, ww * 32 + __ffs(m) - 1 - k); break; }
    if (++ww >= Wz) break;
    m = (words[ww] ^ flip) & vf_valid(ww, G);
  }
  out[v] = g >= G ? SFMI_EDT_INF : g * g;
}

// one thread per line.  Lines: n_outer blocks of G * n_inner voxels, the line (outer, inner) holds the G voxels outer * G * n_inner +
// u * n_inner + inner: the j pass has n_inner = G (outer = b * G + i), the i pass n_inner = G^2 (outer = b)
__global__ __launch_bounds__(256) void edt_line_kernel(const int* __restrict__ in, int* __restrict__ out, unsigned short* __restrict__ S,
                                                       unsigned short* __restrict__ T, int G, int n_inner, int n_lines) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n_lines) return;
  const int outer = t / n_inner, inner = t - outer * n_inner;
  const size_t base = (size_t)outer * G * n_inner + inner;
  sfmi_edt_line(in + base, out + base, S + base, T + base, G, n_inner);
}

// one thread per voxel, after the i pass: a grid without a set voxel holds values >= SFMI_EDT_INF everywhere
__global__ __launch_bounds__(256) void edt_finish_kernel(int* __restrict__ d2, int G, int NV, int* __restrict__ status) {
  const unsigned vu = blockIdx.x * 256u + threadIdx.x;      // unsigned: the last workgroup may reach past 2^31
  if (vu >= (unsigned)NV) return;
  const int v = (int)vu;
  const int x = d2[v];
  const bool empty = x >= SFMI_EDT_INF;
  if (empty) d2[v] = 3 * G * G;
  const int G3 = G * G * G;
  if (v % G3 == 0) status[v / G3] = empty ? 1 : 0;
}

// one thread per voxel: the signed distance from the two transforms
__global__ __launch_bounds__(256) void edt_signed_kernel(const unsigned* __restrict__ bits, const int* __restrict__ to_clear,
                                                         const int* __restrict__ to_set, const int* __restrict__ st, int B, int G, int Wz,
                                                         int NV, double* __restrict__ d, int* __restrict__ status) {
  const unsigned vu = blockIdx.x * 256u + threadIdx.x;      // unsigned: the last workgroup may reach past 2^31
  if (vu >= (unsigned)NV) return;
  const int v = (int)vu;
  d[v] = vf_bit(bits, v, G, Wz) ? __dsqrt_rn((double)to_clear[v]) - 0.5 : -__dsqrt_rn((double)to_set[v]) + 0.5;
  const int G3 = G * G * G;
  if (v % G3 == 0) status[v / G3] = (st[v / G3] | st[B + v / G3]) ? 1 : 0;
}

struct EdtWs { int *tmp, *to_clear, *to_set, *st; unsigned short *S, *T; };
EdtWs edt_ws(SfmiCarver& c, int B, int G, int is_signed) {
  const size_t NV = (size_t)B * G * G * G;
  EdtWs w{};
  w.tmp = c.take<int>(NV);
  w.S = c.take<unsigned short>(NV);
  w.T = c.take<unsigned short>(NV);
  if (is_signed) {
    w.to_clear = c.take<int>(NV);
    w.to_set = c.take<int>(NV);
    w.st = c.take<int>(2 * (size_t)B);
  }
  return w;
}

// the three passes and the finish: 4 launches
void edt_run(const unsigned* bits, int B, int G, int invert, int* d2, int* status, const EdtWs& w, hipStream_t st) {
  const int Wz = vf_wz(G), NV = B * G * G * G, n_lines = B * G * G;
  hipLaunchKernelGGL(edt_k_kernel, dim3(blocks256(NV)), dim3(256), 0, st, bits, G, Wz, NV, invert ? 1 : 0, d2);
  hipLaunchKernelGGL(edt_line_kernel, dim3(blocks256(n_lines)), dim3(256), 0, st, (const int*)d2, w.tmp, w.S, w.T, G, G, n_lines);
  hipLaunchKernelGGL(edt_line_kernel, dim3(blocks256(n_lines)), dim3(256), 0, st, (const int*)w.tmp, d2, w.S, w.T, G, G * G, n_lines);
  hipLaunchKernelGGL(edt_finish_kernel, dim3(blocks256(NV)), dim3(256), 0, st, d2, G, NV, status);
}

// ---- Gaussian filter ------------------------------------------------------------------------------------------------------------------

// scipy's "reflect": (d c b a | a b c d | d c b a), repeated for an index further out than one lattice
__device__ __forceinline__ int vf_reflect(int p, int G) {
  if (p >= 0 && p < G) return p;
  const int P = 2 * G;
  int m = p % P;
  if (m < 0) m += P;
  return m < G ? m : P - 1 - m;
}

// one thread per voxel: the taps along `axis`, summed as scipy's correlate1d sums a symmetric kernel: the centre, then the pairs from
// the farthest to the nearest, (left + right) * weight.  in == NULL: the axis-0 pass over the bits, value bit - 0.5
__global__ __launch_bounds__(256) void vf_gauss_kernel(const unsigned* __restrict__ bits, const double* __restrict__ in,
                                                       const double* __restrict__ wgt, int r, int G, int Wz, int NV, int axis,
                                                       double* __restrict__ out) {
  const unsigned vu = blockIdx.x * 256u + threadIdx.x;      // unsigned: the last workgroup may reach past 2^31
  if (vu >= (unsigned)NV) return;
  const int v = (int)vu;
  const int k = v % G, j = (v / G) % G, i = (v / (G * G)) % G;
  const int l = axis == 0 ? i : (axis == 1 ? j : k), stride = axis == 0 ? G * G : (axis == 1 ? G : 1);
  const int base = v - l * stride;
  double acc;
  if (in) {
    acc = in[v] * wgt[r];
    for (int d = r; d >= 1; --d)
      acc += (in[base + vf_reflect(l - d, G) * stride] + in[base + vf_reflect(l + d, G) * stride]) * wgt[r - d];
  } else {
    const unsigned* __restrict__ col = bits + (size_t)(base / G) * Wz + (k >> 5);      // row (b, 0, j), the word of k
    const size_t rs = (size_t)G * Wz;                                                  // words between rows i and i + 1
    const int sh = k & 31;
    acc = ((double)((col[i * rs] >> sh) & 1u) - 0.5) * wgt[r];
    for (int d = r; d >= 1; --d) {
      const double a = (double)((col[vf_reflect(i - d, G) * rs] >> sh) & 1u) - 0.5;
      const double b = (double)((col[vf_reflect(i + d, G) * rs] >> sh) & 1u) - 0.5;
      acc += (a + b) * wgt[r - d];
    }
  }
  out[v] = acc;
}

// ---- constrained smoothing ------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ bool vf_in_band(double d, double R) { return fabs(d) <= R; }

// the six neighbours of v with the index clamped to the lattice (edge replication)
struct VfNb { int im, ip, jm, jp, km, kp; };
__device__ __forceinline__ VfNb vf_neighbours(int v, int G) {
  const int k = v % G, j = (v / G) % G, i = (v / (G * G)) % G, G2 = G * G;
  VfNb n;
  n.im = i > 0 ? v - G2 : v;
  n.ip = i + 1 < G ? v + G2 : v;
  n.jm = j > 0 ? v - G : v;
  n.jp = j + 1 < G ? v + G : v;
  n.km = k > 0 ? v - 1 : v;
  n.kp = k + 1 < G ? v + 1 : v;
  return n;
}
// L x (v), in the contract's order
__device__ __forceinline__ double vf_laplace(const double* __restrict__ x, int v, int G) {
  const VfNb n = vf_neighbours(v, G);
  return (((((x[n.ip] + x[n.im]) + x[n.jp]) + x[n.jm]) + x[n.kp]) + x[n.km]) - 6.0 * x[v];
}

// sum over the workgroup of two counts held by lane 0 of each of its 4 waves; the result in thread 0
__device__ __forceinline__ void vf_block_counts(int cb, int cs, int* sh, int& tb, int& ts) {
  const int tid = threadIdx.x;
  if ((tid & 63) == 0) { sh[tid >> 6] = cb; sh[4 + (tid >> 6)] = cs; }
  __syncthreads();
  tb = (sh[0] + sh[1]) + (sh[2] + sh[3]);
  ts = (sh[4] + sh[5]) + (sh[6] + sh[7]);
}

// one workgroup per chunk of VF_CHUNK voxels: u = d; flag bit 0 = band, bit 1 = support (the voxel or one of its six neighbours is
// in the band); cnt[chunk] = (band voxels, support voxels) of the chunk
__global__ __launch_bounds__(256) void vf_flag_kernel(const double* __restrict__ d, int G, int NV, double R, double* __restrict__ u,
                                                      unsigned char* __restrict__ flag, int2* __restrict__ cnt) {
  __shared__ int sh[8];
  int cb = 0, cs = 0;
  const unsigned v0 = blockIdx.x * (unsigned)VF_CHUNK + threadIdx.x;      // unsigned: the last chunk may reach past 2^31
  for (int rd = 0; rd < VF_CHUNK / 256; ++rd) {
    const unsigned vu = v0 + rd * 256u;
    const int v = (int)vu;
    int f = 0;
    if (vu < (unsigned)NV) {
      const double x = d[v];
      const VfNb n = vf_neighbours(v, G);
      const bool band = vf_in_band(x, R);
      const bool sup = band | vf_in_band(d[n.im], R) | vf_in_band(d[n.ip], R) | vf_in_band(d[n.jm], R) | vf_in_band(d[n.jp], R) |
                       vf_in_band(d[n.km], R) | vf_in_band(d[n.kp], R);
      f = (band ? 1 : 0) | (sup ? 2 : 0);
      u[v] = x;
      flag[v] = (unsigned char)f;
    }
    cb += __popcll(__ballot(f & 1));            // the same number in every lane of the wave
    cs += __popcll(__ballot(f & 2));
  }
  int tb, ts;
  vf_block_counts(cb, cs, sh, tb, ts);
  if (threadIdx.x == 0) cnt[blockIdx.x] = make_int2(tb, ts);
}

// one workgroup: cnt (n) -> its exclusive prefix sums in place, total[0 .. 1] = the sums.  Thread t takes a run of ceil(n / 1024) chunks
__global__ __launch_bounds__(VF_SCAN_THREADS) void vf_scan_kernel(int2* __restrict__ cnt, int n, int* __restrict__ total) {
  __shared__ int sb[VF_SCAN_THREADS], ss[VF_SCAN_THREADS];
  const int tid = threadIdx.x, per = (n + VF_SCAN_THREADS - 1) / VF_SCAN_THREADS;
  const int lo = min(n, tid * per), hi = min(n, lo + per);
  int ab = 0, as = 0;
  for (int c = lo; c < hi; ++c) { ab += cnt[c].x; as += cnt[c].y; }
  sb[tid] = ab;
  ss[tid] = as;
  __syncthreads();
  // Hillis-Steele over the 1024 run sums (integers: any order gives the same numbers)
  for (int o = 1; o < VF_SCAN_THREADS; o <<= 1) {
    const int xb = tid >= o ? sb[tid - o] : 0, xs = tid >= o ? ss[tid - o] : 0;
    __syncthreads();
    sb[tid] += xb;
    ss[tid] += xs;
    __syncthreads();
  }
  int rb = sb[tid] - ab, rs = ss[tid] - as;     // exclusive
  for (int c = lo; c < hi; ++c) {
    const int2 x = cnt[c];
    cnt[c] = make_int2(rb, rs);
    rb += x.x;
    rs += x.y;
  }
  if (tid == VF_SCAN_THREADS - 1) { total[0] = sb[tid]; total[1] = ss[tid]; }
}

// one workgroup per chunk: the flagged voxels into the two lists at the chunk's offsets, in ascending flat index
__global__ __launch_bounds__(256) void vf_emit_kernel(const unsigned char* __restrict__ flag, const int2* __restrict__ off, int NV,
                                                      int* __restrict__ band, int* __restrict__ sup) {
  __shared__ int sh[8];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  const int2 o = off[blockIdx.x];
  int rb = o.x, rs = o.y;
  for (int rd = 0; rd < VF_CHUNK / 256; ++rd) {
    const unsigned vu = blockIdx.x * (unsigned)VF_CHUNK + rd * 256u + tid;      // unsigned: as in the flag kernel
    const int v = (int)vu;
    const int f = vu < (unsigned)NV ? flag[vu] : 0;
    const unsigned long long mb = __ballot(f & 1), ms = __ballot(f & 2);
    if (lane == 0) { sh[wave] = __popcll(mb); sh[4 + wave] = __popcll(ms); }
    __syncthreads();
    int pb = 0, ps = 0;
    for (int w = 0; w < wave; ++w) { pb += sh[w]; ps += sh[4 + w]; }
    if (f & 1) band[rb + pb + __popcll(mb & below)] = v;
    if (f & 2) sup[rs + ps + __popcll(ms & below)] = v;
    rb += (sh[0] + sh[1]) + (sh[2] + sh[3]);
    rs += (sh[4] + sh[5]) + (sh[6] + sh[7]);
    __syncthreads();
  }
}

// Lu = L u on the support list (n[1] entries)
__global__ __launch_bounds__(256) void vf_lap_kernel(const double* __restrict__ u, const int* __restrict__ sup, const int* __restrict__ n,
                                                     int G, double* __restrict__ Lu) {
  const int count = n[1];
  for (int e = blockIdx.x * 256 + threadIdx.x; e < count; e += gridDim.x * 256) {
    const int v = sup[e];
    Lu[v] = vf_laplace(u, v, G);
  }
}

// u <- max(lo, min(hi, u - L(Lu) / 84)) on the band list (n[0] entries); Lu is the previous iterate's, so the update is Jacobi
__global__ __launch_bounds__(256) void vf_step_kernel(const unsigned* __restrict__ bits, const double* __restrict__ Lu,
                                                      const int* __restrict__ band, const int* __restrict__ n, int G, int Wz,
                                                      double* __restrict__ u) {
  const int count = n[0];
  for (int e = blockIdx.x * 256 + threadIdx.x; e < count; e += gridDim.x * 256) {
    const int v = band[e];
    const double x = u[v] - vf_laplace(Lu, v, G) / 84.0;
    // set: [0, +inf); clear: (-inf, 0]
    u[v] = vf_bit(bits, v, G, Wz) ? (x < 0.0 ? 0.0 : x) : (x > 0.0 ? 0.0 : x);
  }
}

struct VcWs { double* Lu; unsigned char* flag; int *band, *sup, *total; int2* cnt; };
VcWs vc_ws(SfmiCarver& c, int B, int G) {
  const size_t NV = (size_t)B * G * G * G;
  VcWs w{};
  w.Lu = c.take<double>(NV);
  w.band = c.take<int>(NV);
  w.sup = c.take<int>(NV);
  w.flag = c.take<unsigned char>(NV);
  w.cnt = c.take<int2>(cdiv(NV, VF_CHUNK));
  w.total = c.take<int>(2);
  return w;
}

}  // namespace

extern "C" {

int sfmi_vox_max_grid(void) { return VF_MAX_G; }
int sfmi_vox_gaussian_max_radius(void) { return VF_MAX_RADIUS; }

size_t sfmi_edt_workspace_bytes(int B, int G, int is_signed) {
  return vf_sizes(B, G) ? sfmi_ws_bytes(edt_ws, B, G, is_signed ? 1 : 0) : 0;
}

int sfmi_edt_sq_u32(const unsigned* bits, int B, int G, int invert, int* d2, int* status, void* ws, void* stream) {
  if (!vf_sizes(B, G) || !bits || !d2 || !status || !ws) return SFMI_EINVAL;
  SfmiCarver c{(char*)ws};
  const EdtWs w = edt_ws(c, B, G, 0);
  edt_run(bits, B, G, invert, d2, status, w, (hipStream_t)stream);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_edt_signed_f64(const unsigned* bits, int B, int G, double* d, int* status, void* ws, void* stream) {
  if (!vf_sizes(B, G) || !bits || !d || !status || !ws) return SFMI_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  SfmiCarver c{(char*)ws};
  const EdtWs w = edt_ws(c, B, G, 1);
  const int NV = B * G * G * G;
  edt_run(bits, B, G, 1, w.to_clear, w.st, w, st);
  edt_run(bits, B, G, 0, w.to_set, w.st + B, w, st);
  hipLaunchKernelGGL(edt_signed_kernel, dim3(blocks256(NV)), dim3(256), 0, st, bits, (const int*)w.to_clear, (const int*)w.to_set,
                     (const int*)w.st, B, G, vf_wz(G), NV, d, status);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

size_t sfmi_vox_gaussian_workspace_bytes(int B, int G) {
  if (!vf_sizes(B, G)) return 0;
  SfmiCarver c{nullptr};
  c.take<double>((size_t)B * G * G * G);
  return c.bytes();
}

int sfmi_vox_gaussian_f64(const unsigned* bits, int B, int G, const double* weights, int radius, double* out, void* ws, void* stream) {
  if (!vf_sizes(B, G) || radius < 0 || radius > VF_MAX_RADIUS || !bits || !weights || !out || !ws) return SFMI_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  SfmiCarver c{(char*)ws};
  const int NV = B * G * G * G, Wz = vf_wz(G);
  double* tmp = c.take<double>((size_t)NV);
  const dim3 grid(blocks256(NV));
  hipLaunchKernelGGL(vf_gauss_kernel, grid, dim3(256), 0, st, bits, (const double*)nullptr, weights, radius, G, Wz, NV, 0, out);
  hipLaunchKernelGGL(vf_gauss_kernel, grid, dim3(256), 0, st, bits, (const double*)out, weights, radius, G, Wz, NV, 1, tmp);
  hipLaunchKernelGGL(vf_gauss_kernel, grid, dim3(256), 0, st, bits, (const double*)tmp, weights, radius, G, Wz, NV, 2, out);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

size_t sfmi_vox_constrained_workspace_bytes(int B, int G) { return vf_sizes(B, G) ? sfmi_ws_bytes(vc_ws, B, G) : 0; }

int sfmi_vox_constrained_f64(const unsigned* bits, const double* d, int B, int G, double band_radius, int iters, double* u, void* ws,
                             void* stream) {
  if (!vf_sizes(B, G) || iters < 0 || !(band_radius >= 0.0 && band_radius <= 1.7976931348623157e308) || !bits || !d || !u || !ws || u == d)
    return SFMI_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  SfmiCarver c{(char*)ws};
  const VcWs w = vc_ws(c, B, G);
  const int NV = B * G * G * G, Wz = vf_wz(G), chunks = (int)cdiv(NV, VF_CHUNK);
  hipLaunchKernelGGL(vf_flag_kernel, dim3(chunks), dim3(256), 0, st, d, G, NV, band_radius, u, w.flag, w.cnt);
  hipLaunchKernelGGL(vf_scan_kernel, dim3(1), dim3(VF_SCAN_THREADS), 0, st, w.cnt, chunks, w.total);
  hipLaunchKernelGGL(vf_emit_kernel, dim3(chunks), dim3(256), 0, st, (const unsigned char*)w.flag, (const int2*)w.cnt, NV, w.band, w.sup);
  const dim3 grid(blocks256(NV) < VF_ITER_GRID ? blocks256(NV) : VF_ITER_GRID);
  for (int it = 0; it < iters; ++it) {
    hipLaunchKernelGGL(vf_lap_kernel, grid, dim3(256), 0, st, (const double*)u, (const int*)w.sup, (const int*)w.total, G, w.Lu);
    hipLaunchKernelGGL(vf_step_kernel, grid, dim3(256), 0, st, bits, (const double*)w.Lu, (const int*)w.band, (const int*)w.total, G, Wz, u);
  }
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_vox_constrained_lists_i32(const void* ws, int B, int G, int* band, int* support, int* counts, void* stream) {
  if (!vf_sizes(B, G) || !ws || !band || !support || !counts) return SFMI_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  SfmiCarver c{(char*)const_cast<void*>(ws)};                  // read only
  const VcWs w = vc_ws(c, B, G);
  const size_t bytes = (size_t)B * G * G * G * sizeof(int);
  SFMI_TRY(hipMemcpyAsync(band, w.band, bytes, hipMemcpyDeviceToDevice, st));
  SFMI_TRY(hipMemcpyAsync(support, w.sup, bytes, hipMemcpyDeviceToDevice, st));
  SFMI_TRY(hipMemcpyAsync(counts, w.total, 2 * sizeof(int), hipMemcpyDeviceToDevice, st));
  return SFMI_OK;
}

}  // extern "C"
