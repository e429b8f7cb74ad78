// The split brute-force nearest-neighbour search of the scan tools, written once for pointdist.hip (nn_dist), knn.hip,
// register.hip (ICP correspondences) and features.hip (FPFH matching).  Queries P_b and references Q_b are ragged sets with int64
// offsets.  A workgroup of 256 lanes holds QB queries in registers (a "query block"; blocks never straddle two sets) and walks Q_b
// through an LDS tile.  With too few query blocks to fill the chip, Q_b is cut into S contiguous chunks (grid.y): chunk s writes a
// partial result per query at [s * N + i] and a second launch merges the S partials.
// The tie rule, everywhere: references are scanned in ascending order with a strict `<`, chunks are merged in ascending order with a
// strict `<`, so the lowest index among equal f32 distances wins and the result does not depend on S.  No atomics.
// Nothing here has a product feeding a sum outside an explicit fmaf, so no includer's contraction setting changes its bits.
#pragma once
#include "sfmi_ragged.h"

// ---- the split plan -------------------------------------------------------------------------------------------------------------------
constexpr int SFMI_MAX_SPLITS = 64;
constexpr int SFMI_MIN_CHUNK = 512;              // fewest reference points (on average) per chunk

// query-block upper bound, the grid's x: sum_b ceil(N_b / QB) <= ceil(N / QB) + B
inline long long sfmi_qblocks(int B, long long N, int QB) { return cdiv(N, QB) + B; }

// S: enough chunks to reach target_blocks workgroups, at most SFMI_MAX_SPLITS, `cap` (a tool's workspace limit) and what leaves
// SFMI_MIN_CHUNK references per chunk and set; at least 1
inline int sfmi_splits(int B, long long N, long long M, int target_blocks, int QB, long long cap = SFMI_MAX_SPLITS) {
  long long s = cdiv(target_blocks, sfmi_qblocks(B, N, QB));
  const long long by_m = M / ((long long)B * SFMI_MIN_CHUNK);
  if (s > by_m) s = by_m;
  if (s > SFMI_MAX_SPLITS) s = SFMI_MAX_SPLITS;
  if (s > cap) s = cap;
  return s < 1 ? 1 : (int)s;
}

// block_off[b] = sum_{b' < b} ceil(N_b' / QB): which query blocks belong to which set (one lane calls; B is small)
__device__ __forceinline__ void sfmi_block_offsets(const long long* __restrict__ poff, long long* __restrict__ block_off, int B, int QB) {
  long long acc = 0;
  for (int b = 0; b < B; ++b) {
    block_off[b] = acc;
    acc += cdiv(poff[b + 1] - poff[b], QB);
  }
  block_off[B] = acc;
}

// (`static`: every includer is its own translation unit of one library and gets its own copy of the instances it launches)
template <int QB>
static __global__ void sfmi_block_offsets_kernel(const long long* __restrict__ poff, long long* __restrict__ block_off, int B) {
  if (threadIdx.x == 0 && blockIdx.x == 0) sfmi_block_offsets(poff, block_off, B, QB);
}

// chunk s of S of the references [q0, q1) -> [j0, j1) (S = gridDim.y, s = blockIdx.y: workgroup-uniform)
__device__ __forceinline__ void sfmi_chunk_range(long long q0, long long q1, unsigned S, unsigned s, long long& j0, long long& j1) {
  const long long chunk = cdiv(q1 - q0, (long long)S);
  j0 = q0 + (long long)s * chunk;
  j1 = j0 + chunk;
  if (j1 > q1) j1 = q1;
}

// ---- the 3-D search -------------------------------------------------------------------------------------------------------------------
constexpr int SFMI_SCAN_TILE = 256;              // references per LDS tile (float4: 4 KiB) = lanes per workgroup

// One query block against this workgroup's chunk (gridDim.y, blockIdx.y) of the references [q0, q1) of Q.  Lane `tid` holds the R queries
// i = qbase + r * 256 + tid; load(i, i < pend, x, y, z) fetches one (zeros past the set's end `pend`): the tool's own prologue, e.g.
// register.hip applies the pose there.  The tile is read as a broadcast ds_read_b128 (every lane the same address), so one LDS read feeds
// R distance evaluations.  Distance in ONE expression order, the direct form d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx)), (dx, dy, dz) = p - q.
// -> dd[i] and, unless ii is null, ii[i] (the chunk's outputs, the caller's d_out + blockIdx.y * N): the index local to q0 (M_b < 2^31),
// -1 when nothing was < +inf.  Every lane of the workgroup calls, with workgroup-uniform arguments.  The queries live in arrays of THIS
// function, and dd / ii are formed by the caller: arrays of the kernel handed in by reference, or the output pointers formed in here,
// each cost register copies inside the tile loop.
template <int R, typename Load>
__device__ __forceinline__ void sfmi_search3(const float* __restrict__ Q, long long q0, long long q1, long long qbase, long long pend,
                                             Load load, float* __restrict__ dd, int* __restrict__ ii) {
  __shared__ float4 tile[SFMI_SCAN_TILE];
  const int tid = threadIdx.x;
  float px[R], py[R], pz[R], best[R];
  int bi[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const long long i = qbase + r * SFMI_SCAN_TILE + tid;
    load(i, i < pend, px[r], py[r], pz[r]);
    best[r] = INFINITY;
    bi[r] = -1;
  }
  long long j0, j1;
  sfmi_chunk_range(q0, q1, gridDim.y, blockIdx.y, j0, j1);
  for (long long t0 = j0; t0 < j1; t0 += SFMI_SCAN_TILE) {     // workgroup-uniform bounds
    __syncthreads();                                           // the previous tile is consumed
    {
      const long long j = t0 + tid;
      // padding past the chunk: +inf coordinates give d2 = inf (or NaN), never < best (strict), so they are never selected
      tile[tid] = j < j1 ? make_float4(Q[3 * j], Q[3 * j + 1], Q[3 * j + 2], 0.f) : make_float4(INFINITY, INFINITY, INFINITY, 0.f);
    }
    __syncthreads();
    const int jb = (int)(t0 - q0);                             // local index of the tile's first point
#pragma unroll 4
    for (int jj = 0; jj < SFMI_SCAN_TILE; ++jj) {
      const float4 q = tile[jj];                               // broadcast ds_read_b128
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const float dx = px[r] - q.x, dy = py[r] - q.y, dz = pz[r] - q.z;
        const float d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
        const bool lt = d2 < best[r];
        best[r] = lt ? d2 : best[r];
        bi[r] = lt ? jb + jj : bi[r];
      }
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const long long i = qbase + r * SFMI_SCAN_TILE + tid;
    if (i < pend) {
      dd[i] = best[r];
      if (ii) ii[i] = bi[r];
    }
  }
}

// ---- the merge ------------------------------------------------------------------------------------------------------------------------
// one lane per query: its S partials in ascending chunk order (strict `<`: the lower index wins a tie).  IDX: the index is wanted (else
// pi and idx are not touched).  FROZEN: a query whose set b has state[b] != 0 is left as it is (poff, state, B are read only then).
template <bool IDX, bool FROZEN>
static __global__ void sfmi_nn_merge_kernel(const float* __restrict__ pd, const int* __restrict__ pi, const long long* __restrict__ poff,
                                            const int* __restrict__ state, int B, int S, long long N, float* __restrict__ d2,
                                            int* __restrict__ idx) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  if constexpr (FROZEN) {
    if (state[sfmi_owner(poff, B, i)] != 0) return;
  }
  float best = pd[i];
  int bi = IDX ? pi[i] : 0;
  for (int s = 1; s < S; ++s) {
    const float d = pd[(long long)s * N + i];
    if constexpr (IDX) {
      const int k = pi[(long long)s * N + i];
      if (d < best) { best = d; bi = k; }
    } else {
      if (d < best) best = d;
    }
  }
  d2[i] = best;
  if constexpr (IDX) idx[i] = bi;
}

template <bool IDX, bool FROZEN>
inline void sfmi_nn_merge(const float* pd, const int* pi, const long long* poff, const int* state, int B, int S, long long N, float* d2,
                          int* idx, hipStream_t st) {
  hipLaunchKernelGGL((sfmi_nn_merge_kernel<IDX, FROZEN>), dim3(blocks256(N)), dim3(256), 0, st, pd, pi, poff, state, B, S, N, d2, idx);
}
