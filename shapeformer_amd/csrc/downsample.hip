// Downsampling of raw scans over ragged point sets: farthest point sampling and a voxel grid.  What every scan pipeline runs before the
// cleaning front end of knn.hip (PCL VoxelGrid / Open3D voxel_down_sample in front of StatisticalOutlierRemoval; FPS to bring a cloud
// to the 2 048 / 16 384 points of the completion benchmarks).  DESIGN.md §5.15.
//
// 1. fps_kernel: one workgroup of 1024 lanes per set, persistent over that set's picks.  The contract, in full:
//      candidates of set b: its points, or those with valid[i] != 0;  count[b] = min(n, number of candidates)
//      dist[i] = +inf for every candidate.  The first pick is start[b] when given, else the arg max below (the candidate of lowest index).
//      after each pick s:  dist[i] = min(dist[i], fmaf(dz, dz, fmaf(dy, dy, dx * dx))) with f32 differences to s (the direct form of
//      nn_kernel / knn_kernel, the same bits), and s leaves the candidates for good
//      next pick: arg max dist, among equal f32 values the LOWER index;  d2[b,t] = the winner's dist when it was picked (d2[b,0] = +inf)
//      columns t >= count[b] hold (-1, 0.0f);  status 0 ok, 1 no candidate, 2 a non-finite coordinate among the candidates (both: the
//      row is all tail), 3 a set of 2^31 points or more (refused by the host)
//    min, fmaf and an arg max under a total order are all exact and order-free: the result is a function of the set alone, whichever
//    form below serves it, bit-identical from run to run, and a run with smaller n is a prefix of a run with larger n.  No atomics.
//    Resident form (sets up to FPS_RESIDENT_MAX = 1024 x 16): lane t holds points t, t + 1024, ... and their running distances in R
//    registers each, R = 1, 4 or 16 by the set's size (a workgroup-uniform branch; every register index a compile-time constant).
//    Per pick: R updates per lane with the lane's own best (dist, index) kept on the way, a butterfly per wave under the explicit
//    (greater dist, then lower index) compare (four DPP steps inside each row of 16 lanes, two shuffles across the rows), 16 wave
//    results through double-buffered LDS slots behind ONE barrier, a second butterfly over 16 lanes (DPP only), and the winner's
//    coordinates by one wave-uniform read (a scalar load of an L2-resident line).
//    Streaming form (larger sets): the same workgroup sweeps the set from global memory each pick, four points per lane and step with
//    16-byte loads; dist lives in the caller's workspace in a slice of the set's own, so no two workgroups share a 16-byte group.
//    Loop discipline: the pick count comes from one workgroup reduction of the candidate count, the loop runs exactly that many
//    iterations, every branch around a barrier is workgroup-uniform; no spins, nothing waits on another workgroup.
// 2. Voxel grid: per set lo = the componentwise f32 minimum (vox_bounds_kernel: integer atomicMin on an order-preserving encoding: a
//    minimum does not depend on the order), cell = floor((double(x) - double(lo)) / voxel) per axis in IEEE f64, key =
//    ((set * 65536 + cz) * 65536 + cy) * 65536 + cx (vox_key_kernel; status bits: 1 a non-finite coordinate, 2 an axis of 65 536 cells
//    or more).  The host sorts the keys (stable) and marks the run starts; vox_reduce_kernel is one lane per run: count, the lowest
//    local index (the run's first record: the sort is stable), and the centroid: an f64 sum in record order by the lane itself for
//    runs up to 64 points, and for longer runs by the lane's whole wave (lane l sums records l, l + 64, ... in order, then the fixed
//    tree of wave_sum_f64).  The order of the sum depends on the run alone: bit-identical from run to run and in any batch.
#include "sfmi_ragged.h"   // the ragged-batch helpers the mesh tools share: DESIGN.md §5.5a

namespace {

constexpr int FPS_THREADS = 1024;
constexpr int FPS_WAVES = FPS_THREADS / 64;
constexpr int FPS_RESIDENT_MAX = FPS_THREADS * 16;

// (d, i) <- the better of (d, i) and (od, oi) under (greater dist, then lower index): a total order, so two lanes that exchange their
// pairs agree afterwards
__device__ __forceinline__ void fps_take(float& d, int& i, float od, int oi) {
  const bool take = od > d || (od == d && oi < i);
  d = take ? od : d;
  i = take ? oi : i;
}

// one butterfly step inside an aligned group of 16 lanes by a DPP operand modifier, no trip through the LDS crossbar: quad_perm
// [1,0,3,2] (0xB1), quad_perm [2,3,0,1] (0x4E), row_half_mirror (0x141), row_mirror (0x140).  As in sfmi_common.h's row16_max the
// mirrors stand for xor 4 / xor 8: after the quad steps the four lanes of a quad agree, so lane 7 - i delivers what lane i ^ 4 holds
template <int CTRL>
__device__ __forceinline__ void fps_dpp_step(float& d, int& i) {
  const int di = __float_as_int(d);
  fps_take(d, i, __int_as_float(__builtin_amdgcn_update_dpp(di, di, CTRL, 0xF, 0xF, false)),
           __builtin_amdgcn_update_dpp(i, i, CTRL, 0xF, 0xF, false));
}

// (d, i) <- the best pair of each aligned group of WIDTH lanes (16 or 64), in every lane of the group.  Every lane of the wave is active
template <int WIDTH>
__device__ __forceinline__ void fps_butterfly(float& d, int& i) {
  fps_dpp_step<0xB1>(d, i);
  fps_dpp_step<0x4E>(d, i);
  fps_dpp_step<0x141>(d, i);
  fps_dpp_step<0x140>(d, i);
#pragma unroll
  for (int o = 16; o < WIDTH; o <<= 1) fps_take(d, i, __shfl_xor(d, o, 64), __shfl_xor(i, o, 64));
}

// the workgroup's best pair of pick t from every lane's own best; one barrier.  slot: [2][FPS_WAVES], buffer t & 1: a wave that
// writes buffer t & 1 again (pick t + 2) has passed the barrier of pick t + 1, which every wave reaches after its reads of pick t
__device__ __forceinline__ void fps_pick(float bd, int bi, int t, float2 (*slot)[FPS_WAVES], float& wd, int& wi) {
  fps_butterfly<64>(bd, bi);
  if ((threadIdx.x & 63) == 0) slot[t & 1][threadIdx.x >> 6] = make_float2(bd, __int_as_float(bi));
  __syncthreads();
  const float2 e = slot[t & 1][threadIdx.x & (FPS_WAVES - 1)];
  wd = e.x;
  wi = __float_as_int(e.y);
  fps_butterfly<FPS_WAVES>(wd, wi);
  wi = __builtin_amdgcn_readfirstlane(wi);                     // the same in every lane: scalar from here on
}

// sum of c and OR of f over the workgroup, in every lane (two barriers; called once per set, before the pick loop)
__device__ __forceinline__ void fps_block_count(int& c, int& f, int* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    c += __shfl_xor(c, o, 64);
    f |= __shfl_xor(f, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6] = c;
    red[FPS_WAVES + (threadIdx.x >> 6)] = f;
  }
  __syncthreads();
  c = 0;
  f = 0;
#pragma unroll
  for (int w = 0; w < FPS_WAVES; ++w) {
    c += red[w];
    f |= red[FPS_WAVES + w];
  }
  __syncthreads();                                             // red may be written again (never is: one call per workgroup)
}


// P / valid: the set's own base; nb <= FPS_THREADS * R.  -> the number of picks made (0 with status != 0)
template <int R>
__device__ __forceinline__ int fps_resident(const float* __restrict__ P, const unsigned char* __restrict__ valid, int nb, int n, int start,
                                            int* __restrict__ idx_row, float* __restrict__ d2_row, int& status,
                                            float2 (*slot)[FPS_WAVES], int* red) {
  const int tid = threadIdx.x;
  float x[R], y[R], z[R], d[R];
  int cand = 0, bad = 0;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int i = r * FPS_THREADS + tid;
    const bool in = i < nb;
    const bool ok = in && (!valid || valid[i] != 0);
    x[r] = in ? P[3 * (long long)i] : 0.f;
    y[r] = in ? P[3 * (long long)i + 1] : 0.f;
    z[r] = in ? P[3 * (long long)i + 2] : 0.f;
    d[r] = ok ? INFINITY : -1.f;                               // -1: not (or no longer) a candidate; min(-1, d2 >= 0) stays -1
    cand += ok;
    bad |= ok && !sfmi_finite3(x[r], y[r], z[r]);
  }
  fps_block_count(cand, bad, red);
  status = cand == 0 ? 1 : (bad ? 2 : 0);
  const int count = status ? 0 : min(n, cand);                 // workgroup-uniform
  float bd = d[0];
  int bi = tid;
#pragma unroll
  for (int r = 1; r < R; ++r)                                  // a lane's indices ascend with r: a strict > keeps the lower on a tie
    if (d[r] > bd) {
      bd = d[r];
      bi = r * FPS_THREADS + tid;
    }
  for (int t = 0; t < count; ++t) {
    float wd;
    int wi;
    fps_pick(bd, bi, t, slot, wd, wi);
    if (t == 0 && start >= 0) wi = start;                      // every candidate is at +inf: wd is +inf either way
    if (tid == 0) {
      idx_row[t] = wi;
      d2_row[t] = wd;
    }
    const float wx = P[3 * (long long)wi], wy = P[3 * (long long)wi + 1], wz = P[3 * (long long)wi + 2];   // wave-uniform address
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int i = r * FPS_THREADS + tid;
      const float dx = x[r] - wx, dy = y[r] - wy, dz = z[r] - wz;
      float v = fminf(d[r], fmaf(dz, dz, fmaf(dy, dy, dx * dx)));
      v = i == wi ? -1.f : v;
      d[r] = v;
      if (r == 0 || v > bd) {
        bd = v;
        bi = i;
      }
    }
  }
  return count;
}

// The set from global memory each pick.  P / valid: the WHOLE batch (N points), the set is [pbeg, pend); dist: the set's slice of
// the workspace, dist[g - g0] for global index g, g0 = pbeg rounded down to 4: groups of four points at 16-byte aligned addresses
// of P (P itself is 16-byte aligned: the launcher checks) and of dist.  Points of a group outside the set stay at -1.
__device__ __forceinline__ int fps_streaming(const float* __restrict__ P, const unsigned char* __restrict__ valid, long long pbeg,
                                             long long pend, long long N, int n, int start, float* __restrict__ dist,
                                             int* __restrict__ idx_row, float* __restrict__ d2_row, int& status,
                                             float2 (*slot)[FPS_WAVES], int* red) {
  const int tid = threadIdx.x;
  const long long g0 = pbeg & ~3ll;
  const long long groups = (pend - g0 + 3) >> 2;
  int cand = 0, bad = 0;
  float bd = -1.f;
  int bi = 0x7FFFFFFF;
  for (long long q = tid; q < groups; q += FPS_THREADS) {
    const long long g = g0 + 4 * q;
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const long long j = g + e;
      const bool in = j >= pbeg && j < pend;
      const bool ok = in && (!valid || valid[j] != 0);
      v[e] = ok ? INFINITY : -1.f;
      cand += ok;
      if (ok) bad |= !sfmi_finite3(P[3 * j], P[3 * j + 1], P[3 * j + 2]);
      if (v[e] > bd) {
        bd = v[e];
        bi = (int)(j - pbeg);
      }
    }
    *(float4*)(dist + 4 * q) = make_float4(v[0], v[1], v[2], v[3]);
  }
  fps_block_count(cand, bad, red);
  status = cand == 0 ? 1 : (bad ? 2 : 0);
  const int count = status ? 0 : min(n, cand);                 // workgroup-uniform
  for (int t = 0; t < count; ++t) {
    float wd;
    int wi;
    fps_pick(bd, bi, t, slot, wd, wi);
    if (t == 0 && start >= 0) wi = start;
    if (tid == 0) {
      idx_row[t] = wi;
      d2_row[t] = wd;
    }
    const long long wg = pbeg + wi;
    const float wx = P[3 * wg], wy = P[3 * wg + 1], wz = P[3 * wg + 2];
    bd = -2.f;
    bi = 0x7FFFFFFF;
    for (long long q = tid; q < groups; q += FPS_THREADS) {    // each lane rewrites only the groups it wrote: no barrier needed
      const long long g = g0 + 4 * q;
      const float4 dv = *(const float4*)(dist + 4 * q);
      float c[12];
      if (g + 4 <= N) {
        const float4 a = *(const float4*)(P + 3 * g), b = *(const float4*)(P + 3 * g + 4), cc = *(const float4*)(P + 3 * g + 8);
        c[0] = a.x; c[1] = a.y; c[2] = a.z; c[3] = a.w; c[4] = b.x; c[5] = b.y; c[6] = b.z; c[7] = b.w;
        c[8] = cc.x; c[9] = cc.y; c[10] = cc.z; c[11] = cc.w;
      } else {                                                 // the batch's last group: nothing is read past point N - 1
#pragma unroll
        for (int e = 0; e < 12; ++e) c[e] = g + e / 3 < N ? P[3 * g + e] : 0.f;
      }
      float v[4] = {dv.x, dv.y, dv.z, dv.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float dx = c[3 * e] - wx, dy = c[3 * e + 1] - wy, dz = c[3 * e + 2] - wz;
        v[e] = fminf(v[e], fmaf(dz, dz, fmaf(dy, dy, dx * dx)));   // fminf(-1, NaN) = -1: a neighbour set's NaN stays outside
        v[e] = g + e == wg ? -1.f : v[e];
        if (v[e] > bd) {
          bd = v[e];
          bi = (int)(g + e - pbeg);
        }
      }
      *(float4*)(dist + 4 * q) = make_float4(v[0], v[1], v[2], v[3]);
    }
  }
  return count;
}

__global__ __launch_bounds__(FPS_THREADS) void fps_kernel(const float* __restrict__ P, const long long* __restrict__ off,
                                                          const unsigned char* __restrict__ valid, const int* __restrict__ start, int B,
                                                          long long N, int n, int* __restrict__ idx, float* __restrict__ d2,
                                                          int* __restrict__ count, int* __restrict__ status, float* __restrict__ ws) {
  __shared__ float2 slot[2][FPS_WAVES];
  __shared__ int red[2 * FPS_WAVES];
  const int b = blockIdx.x;
  const long long pbeg = off[b], pend = off[b + 1], nb = pend - pbeg;
  int* idx_row = idx + (long long)b * n;
  float* d2_row = d2 + (long long)b * n;
  int s0 = start ? start[b] : -1;
  if (s0 < 0 || s0 >= nb || valid) s0 = -1;                    // the host refuses these; the kernel never reads outside the set
  const unsigned char* vb = valid ? valid + pbeg : nullptr;
  int st = 3, picks = 0;                                       // every branch below is workgroup-uniform: nb is
  if (nb <= FPS_THREADS) picks = fps_resident<1>(P + 3 * pbeg, vb, (int)nb, n, s0, idx_row, d2_row, st, slot, red);
  else if (nb <= FPS_THREADS * 4) picks = fps_resident<4>(P + 3 * pbeg, vb, (int)nb, n, s0, idx_row, d2_row, st, slot, red);
  else if (nb <= FPS_RESIDENT_MAX) picks = fps_resident<16>(P + 3 * pbeg, vb, (int)nb, n, s0, idx_row, d2_row, st, slot, red);
  else if (nb < (1ll << 31))
    picks = fps_streaming(P, valid, pbeg, pend, N, n, s0, ws + (pbeg & ~3ll) + 4ll * b, idx_row, d2_row, st, slot, red);
  for (int t = picks + threadIdx.x; t < n; t += FPS_THREADS) {
    idx_row[t] = -1;
    d2_row[t] = 0.f;
  }
  if (threadIdx.x == 0) {
    count[b] = picks;
    status[b] = st;
  }
}

// ---- voxel grid ------------------------------------------------------------------------------------------------------------------

constexpr int VOX_NON_FINITE = 1, VOX_TOO_FINE = 2;
constexpr int VOX_MAX_SETS = 32768;
constexpr double VOX_MAX_CELLS = 65536.0;
constexpr int VOX_SHORT = 64;                                  // longest run a lane sums alone

// f32 -> u32, order-preserving (-0 below +0; a NaN lands at one end or the other and is flagged by vox_key_kernel)
__device__ __forceinline__ unsigned vox_enc(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float vox_dec(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

__device__ __forceinline__ float wave_min_f32(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}

// grid (S, B): chunk blockIdx.x of set blockIdx.y -> atomicMin into lo[3 b ..] (encoded; the launcher fills it with 0xFF)
__global__ __launch_bounds__(256) void vox_bounds_kernel(const float* __restrict__ P, const long long* __restrict__ off,
                                                         unsigned* __restrict__ lo) {
  __shared__ float red[3][4];
  const int b = blockIdx.y;
  const long long pbeg = off[b], pend = off[b + 1];
  const long long chunk = cdiv(pend - pbeg, (long long)gridDim.x);
  const long long j0 = pbeg + blockIdx.x * chunk, j1 = min(j0 + chunk, pend);
  if (j0 >= j1) return;                                        // block-uniform
  float mx = INFINITY, my = INFINITY, mz = INFINITY;
  for (long long j = j0 + threadIdx.x; j < j1; j += 256) {
    mx = fminf(mx, P[3 * j]);
    my = fminf(my, P[3 * j + 1]);
    mz = fminf(mz, P[3 * j + 2]);
  }
  mx = wave_min_f32(mx); my = wave_min_f32(my); mz = wave_min_f32(mz);
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = mx; red[1][threadIdx.x >> 6] = my; red[2][threadIdx.x >> 6] = mz;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const float m = fminf(fminf(red[threadIdx.x][0], red[threadIdx.x][1]), fminf(red[threadIdx.x][2], red[threadIdx.x][3]));
    atomicMin(lo + 3 * b + threadIdx.x, vox_enc(m));
  }
}

__global__ __launch_bounds__(256) void vox_key_kernel(const float* __restrict__ P, const long long* __restrict__ off,
                                                      const unsigned* __restrict__ lo, int B, long long N, double voxel,
                                                      long long* __restrict__ keys, int* __restrict__ status) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int b = sfmi_owner(off, B, i);
  int flags = 0;
  long long key = b;
#pragma unroll
  for (int a = 2; a >= 0; --a) {                               // z, y, x: x varies fastest
    const float x = P[3 * i + a];
    double c = floor(((double)x - (double)vox_dec(lo[3 * b + a])) / voxel);
    if (!isfinite(x)) {
      flags |= VOX_NON_FINITE;
      c = 0.0;
    } else if (!(c >= 0.0 && c < VOX_MAX_CELLS)) {             // also a NaN from a non-finite lo: that point is flagged itself
      flags |= VOX_TOO_FINE;
      c = 0.0;
    }
    key = key * 65536 + (long long)c;
  }
  keys[i] = key;
  if (flags) atomicOr(status, flags);
}

// one lane per run of the sorted records.  order (N): the records sorted by key (stable); starts (M+1): where each run begins, starts[M] = N
__global__ __launch_bounds__(256) void vox_reduce_kernel(const float* __restrict__ P, const long long* __restrict__ off,
                                                         const long long* __restrict__ order, const long long* __restrict__ starts,
                                                         int B, long long M, int centroid, float* __restrict__ out,
                                                         int* __restrict__ first, int* __restrict__ count) {
  const long long m = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = m < M;
  const long long beg = live ? starts[m] : 0, end = live ? starts[m + 1] : 0, cnt = end - beg;
  const long long g = live ? order[beg] : 0;                   // the run's lowest index: the sort is stable
  double sx = 0.0, sy = 0.0, sz = 0.0;
  if (centroid) {
    if (cnt <= VOX_SHORT)
      for (long long k = beg; k < end; ++k) {
        const long long j = order[k];
        sx += (double)P[3 * j]; sy += (double)P[3 * j + 1]; sz += (double)P[3 * j + 2];
      }
    unsigned long long longs = __ballot(cnt > VOX_SHORT);      // wave-uniform from here: the wave sums its long runs one by one
    const int lane = threadIdx.x & 63;
    while (longs) {
      const int l = __ffsll((long long)longs) - 1;
      longs &= longs - 1;
      const long long lb = __shfl(beg, l, 64), le = __shfl(end, l, 64);
      double ax = 0.0, ay = 0.0, az = 0.0;
#pragma unroll 4
      for (long long k = lb + lane; k < le; k += 64) {
        const long long j = order[k];
        ax += (double)P[3 * j]; ay += (double)P[3 * j + 1]; az += (double)P[3 * j + 2];
      }
      ax = wave_sum_f64(ax); ay = wave_sum_f64(ay); az = wave_sum_f64(az);
      if (lane == l) {
        sx = ax; sy = ay; sz = az;
      }
    }
  }
  if (!live) return;
  if (centroid) {
    out[3 * m] = (float)(sx / (double)cnt);
    out[3 * m + 1] = (float)(sy / (double)cnt);
    out[3 * m + 2] = (float)(sz / (double)cnt);
  } else {
    out[3 * m] = P[3 * g]; out[3 * m + 1] = P[3 * g + 1]; out[3 * m + 2] = P[3 * g + 2];
  }
  first[m] = (int)(g - off[sfmi_owner(off, B, g)]);
  count[m] = (int)cnt;
}

}  // namespace

extern "C" {

int sfmi_fps_resident_max(void) { return FPS_RESIDENT_MAX; }

// workspace: the running distances of the streaming form, N + 4 B + 8 floats (each set's slice starts on a group of four); only a
// batch of more than FPS_RESIDENT_MAX points can hold a set that streams
size_t sfmi_fps_workspace_bytes(int B, long long N, int n) {
  if (B <= 0 || N < 0 || n < 0) return 0;
  if (N <= FPS_RESIDENT_MAX) return 256;
  return align256((size_t)(N + 4ll * B + 8) * 4);
}

int sfmi_fps_f32(const float* P, const long long* off, const unsigned char* valid, const int* start, int B, long long N, int n, int* idx,
                 float* d2, int* count, int* status, void* workspace, void* stream) {
  if (B <= 0 || N < 0 || n < 0 || !off || !count || !status) return SFMI_EINVAL;
  if (n > 0 && (!idx || !d2)) return SFMI_EINVAL;
  if (N > 0 && !P) return SFMI_EINVAL;
  if (N > FPS_RESIDENT_MAX && (!workspace || ((uintptr_t)P & 15) || ((uintptr_t)workspace & 15))) return SFMI_EINVAL;
  hipLaunchKernelGGL(fps_kernel, dim3((unsigned)B), dim3(FPS_THREADS), 0, (hipStream_t)stream, P, off, valid, start, B, N, n, idx, d2,
                     count, status, (float*)workspace);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_voxel_keys_f32(const float* P, const long long* off, int B, long long N, double voxel, unsigned* lo, long long* keys,
                        int* status, void* stream) {
  if (B <= 0 || B >= VOX_MAX_SETS || N < 0 || !(voxel > 0.0) || !(voxel < INFINITY) || !off || !lo || !status) return SFMI_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  SFMI_TRY(hipMemsetAsync(status, 0, sizeof(int), st));
  if (N == 0) return SFMI_OK;
  if (!P || !keys) return SFMI_EINVAL;
  SFMI_TRY(hipMemsetAsync(lo, 0xFF, (size_t)B * 3 * sizeof(unsigned), st));
  long long S = N / ((long long)B * 16384);
  S = S < 1 ? 1 : (S > 256 ? 256 : S);
  hipLaunchKernelGGL(vox_bounds_kernel, dim3((unsigned)S, (unsigned)B), dim3(256), 0, st, P, off, lo);
  hipLaunchKernelGGL(vox_key_kernel, dim3(blocks256(N)), dim3(256), 0, st, P, off, (const unsigned*)lo, B, N, voxel, keys, status);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_voxel_reduce_f32(const float* P, const long long* off, const long long* order, const long long* starts, int B, long long N,
                          long long M, int centroid, float* out, int* first, int* count, void* stream) {
  if (B <= 0 || N < 0 || M < 0 || M > N || !off) return SFMI_EINVAL;
  if (M == 0) return SFMI_OK;
  if (!P || !order || !starts || !out || !first || !count) return SFMI_EINVAL;
  hipLaunchKernelGGL(vox_reduce_kernel, dim3(blocks256(M)), dim3(256), 0, (hipStream_t)stream, P, off, order, starts, B, M,
                     centroid != 0, out, first, count);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

}  // extern "C"
