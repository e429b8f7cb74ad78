// Earth mover's distance between point clouds of equal size: a bijection of least mean Euclidean cost, by Bertsekas' forward auction in
// its Jacobi form with epsilon scaling.  The reference scores completions with Chamfer distance only (xgutils/geoutil.py:362-377); the
// completion literature (PCN, MSN, PoinTr) reports EMD beside it, and the set-level metrics MMD / COV / 1-NNA (Achlioptas et al.;
// PointFlow) need it pair by pair over two collections.  DESIGN.md §5.22; the contract is stated in include/sfmi.h and restated in numpy
// in tests/emd_ref.py.
//
// One persistent workgroup of 16 waves per pair, for the whole call (farthest point sampling is the precedent): a distance matrix has
// thousands of pairs and fills the chip by itself; a single pair runs on one CU, which is accepted.
//
// State.  Per object j: coordinates bx / by / bz (separate arrays: consecutive lanes read consecutive words), price (f64), owner, and
// the round's largest bid (its bits) and lowest bidder among equal bids.  Per person i: assign (the object owned; -1 unassigned;
// -2 - j1 between a round's bid and its resolution: the object bid for), mybid (the bits of the bid).  list: the unassigned persons.
//   resident form, n <= EMD_N_RES = 2048: all of it in LDS, 52 bytes per point (104 KB at 2048: one workgroup per CU); a bidder's own
//   coordinates come from global memory (keeping A in LDS as well was measured and changed nothing: DESIGN.md §5.22)
//   streaming form, n <= 8192: the two atomic targets (best bid, best bidder: 12 bytes per point, 96 KB at 8192) in LDS, the rest in the
//   global workspace, where a pair's 36 bytes per point stay in L2
// One kernel body serves both; the form only says where the arrays are.
//
// A round (all waves, barriers between the steps):
//   list     the persons with assign < 0, compacted by wave ballots; the order within the list is not part of any result
//   bid      few bidders: one wave per bidder, lane l scans objects l, l + 64, ...; the wave merges (v1, j1, v2) by a butterfly.  With
//            fewer than 9 bidders several waves share a bidder (each a slice of the objects) and their partial triples are merged by a
//            second butterfly.  Many bidders (>= EMD_LANE_MIN): one lane per bidder, every object read as a broadcast.  The merge is
//            the maximum under the strict total order (larger v, then lower j), which is commutative and associative, so every split of
//            the objects over lanes, waves and slices gives the same triple
//   offer    64-bit integer maximum of the bid's bits into the object's slot in LDS (bids are positive doubles: their bits order as
//            integers); after a barrier, the bidders whose bid equals the slot offer their index to a 32-bit minimum
//   resolve  one lane per object that received a bid: price, owner and the two assignments
// Only integer atomics in LDS, whose results are order-free; no float atomics, no compare-and-swap loops; barriers inside the
// workgroup are the only synchronisation.  Every loop has a bound the host passes: chunk_rounds rounds per launch, max_rounds per
// pair; a launch leaves prices, owners, eps and the round count in the workspace, a finished pair is frozen, and the host reads one
// counter of unfinished pairs per launch.
#include "sfmi_ragged.h"   // ragged offsets, the f64 block sum: DESIGN.md §5.5a

// the bounding box's diagonal has inexact f64 products: every product and sum rounded on its own, here and in numpy
#pragma clang fp contract(off)

namespace {

constexpr int EMD_THREADS = 1024;
constexpr int EMD_WAVES = EMD_THREADS / 64;
constexpr int EMD_N_RES = 2048;                  // the largest pair of the resident form
constexpr int EMD_N_MAX = 8192;
#ifndef EMD_LANE_MIN
#define EMD_LANE_MIN 1024                        // bidders from which a round bids one lane per bidder (measured: DESIGN.md §5.22)
#endif
constexpr int EMD_CAP_MUL = 320, EMD_CAP_ADD = 256;    // the default round cap per pair: 16 x (20 n + 16), the worst total found
constexpr int EMD_CHUNK_DEFAULT = 16384;         // rounds per launch (measured: DESIGN.md §5.22)
constexpr int EMD_CHUNK_MAX = 1 << 30;            // a larger chunk_rounds means this: the pass counter below stays an int
constexpr int EMD_MAX_PHASES = 64;               // eps falls by 4 from diag / 2 to >= 1e-9 diag: at most 16 phases
constexpr int EMD_NONE = 0x7FFFFFFF;
constexpr int EMD_FEW = 16;                      // `ticks` separates the rounds with fewer bidders than this: the long tail
constexpr int EMD_RES_BYTES = 52, EMD_STREAM_BYTES = 12;   // LDS per point

struct EmdState {                                // per pair, between launches
  double eps, eps_final;
  long long t_few, t_all;                        // ticks of the 100 MHz clock in rounds with fewer than EMD_FEW bidders, in all rounds
  int rounds, status, fin, started;
};

struct EmdArgs {
  const float* A; const long long* aoff; int SA;
  const float* B; const long long* boff; int SB;
  const int* pa; const int* pb; const long long* poff;
  int max_n, max_rounds, chunk_rounds;
  double eps_rel;
  int* assign; double* emd; int* rounds; int* status; double* eps_final; double* price; long long* ticks;
  EmdState* state; int* unfinished;
  int* owner; int* list; unsigned long long* mybid; float* bx; float* by; float* bz;
};

// workspace: per-pair state (P) | the unfinished counter (one int) | owner, list (N int32 each) | bids (N u64) | the streaming form's
// copy of B as three arrays (N f32 each).  Fills the workspace members of a
inline void emd_ws(SfmiCarver& c, int P, long long N, EmdArgs& a) {
  const size_t n = (size_t)N;
  a.state = c.take<EmdState>((size_t)P); a.unfinished = c.take<int>(1);
  a.owner = c.take<int>(n); a.list = c.take<int>(n); a.mybid = c.take<unsigned long long>(n);
  a.bx = c.take<float>(n); a.by = c.take<float>(n); a.bz = c.take<float>(n);
}

__device__ __forceinline__ double emd_cost(float ax, float ay, float az, float x, float y, float z) {
  const float dx = ax - x, dy = ay - y, dz = az - z;
  return (double)sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx * dx)));
}

// (v1, j1, v2) of a set of objects: the largest v with the lowest j among equals, and the largest v of the others
struct EmdTop { double v1, v2; int j1; };

__device__ __forceinline__ void emd_take(EmdTop& t, double v, int j) {   // j above every j taken so far
  if (v > t.v1) { t.v2 = t.v1; t.v1 = v; t.j1 = j; }
  else if (v > t.v2) t.v2 = v;
}

// the triple of the union of two disjoint sets
__device__ __forceinline__ void emd_merge(EmdTop& a, double bv1, double bv2, int bj1) {
  const bool bw = bv1 > a.v1 || (bv1 == a.v1 && bj1 < a.j1);
  const double lose = bw ? a.v1 : bv1;
  a.v2 = fmax(fmax(a.v2, bv2), lose);
  a.v1 = bw ? bv1 : a.v1;
  a.j1 = bw ? bj1 : a.j1;
}

// a lane's triple merged with that of the lane a DPP control names: 0xB1 quad_perm[1,0,3,2], 0x4E quad_perm[2,3,0,1], 0x141
// row_half_mirror, 0x140 row_mirror (sfmi_common.h's row16 butterfly).  After each step the lanes that merged hold the same triple,
// because the merge is commutative, so the mirrored partner stands for the lane an xor butterfly would name
template <int CTRL>
__device__ __forceinline__ void emd_dpp_merge(EmdTop& t) {
  const int l1 = __double2loint(t.v1), h1 = __double2hiint(t.v1), l2 = __double2loint(t.v2), h2 = __double2hiint(t.v2);
  const double bv1 = __hiloint2double(__builtin_amdgcn_update_dpp(h1, h1, CTRL, 0xF, 0xF, false),
                                      __builtin_amdgcn_update_dpp(l1, l1, CTRL, 0xF, 0xF, false));
  const double bv2 = __hiloint2double(__builtin_amdgcn_update_dpp(h2, h2, CTRL, 0xF, 0xF, false),
                                      __builtin_amdgcn_update_dpp(l2, l2, CTRL, 0xF, 0xF, false));
  emd_merge(t, bv1, bv2, __builtin_amdgcn_update_dpp(t.j1, t.j1, CTRL, 0xF, 0xF, false));
}

// the triple of the wave's 64 lanes, in every lane: four DPP steps inside each row of 16 lanes, two shuffles across the rows
__device__ __forceinline__ void emd_wave_merge(EmdTop& t) {
  emd_dpp_merge<0xB1>(t);
  emd_dpp_merge<0x4E>(t);
  emd_dpp_merge<0x141>(t);
  emd_dpp_merge<0x140>(t);
#pragma unroll
  for (int o = 16; o <= 32; o <<= 1) {
    const double bv1 = __shfl_xor(t.v1, o, 64), bv2 = __shfl_xor(t.v2, o, 64);
    const int bj1 = __shfl_xor(t.j1, o, 64);
    emd_merge(t, bv1, bv2, bj1);
  }
}

// person i's bid for the best object of its finished triple: the bid's bits to the object's slot, the object and the bits kept for the
// second step.  The index is tested before the slot it names is touched (it is in range whenever a finite value was scanned)
__device__ __forceinline__ void emd_offer(EmdTop t, int i, int n, double eps, const double* price, int* assign, unsigned long long* mybid,
                                          unsigned long long* bestbits) {
  if ((unsigned)t.j1 >= (unsigned)n) return;
  if (n == 1) t.v2 = t.v1;
  const double bid = (price[t.j1] + (t.v1 - t.v2)) + eps;
  const unsigned long long bits = (unsigned long long)__double_as_longlong(bid);
  assign[i] = -2 - t.j1;
  mybid[i] = bits;
  atomicMax(bestbits + t.j1, bits);
}

template <bool RES>
__global__ __launch_bounds__(EMD_THREADS) void emd_kernel(EmdArgs a) {
  extern __shared__ unsigned long long emd_lds[];
  __shared__ double s_red[EMD_WAVES];
  __shared__ float s_box[EMD_WAVES][6];
  __shared__ double s_pv1[EMD_WAVES], s_pv2[EMD_WAVES];
  __shared__ int s_pj[EMD_WAVES];
  __shared__ int s_cnt, s_bad;
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  EmdState* stp = a.state + p;
  if (stp->fin) return;                                        // frozen: workgroup-uniform
  const double nan = sfmi_nan_f64();

  // ---- the pair, checked before anything it names is read --------------------------------------------------------------------------
  const long long q0 = a.poff[p], np_ = a.poff[p + 1] - q0;
  const int ia = a.pa[p], ib = a.pb[p];
  bool ok = ia >= 0 && ia < a.SA && ib >= 0 && ib < a.SB && np_ >= 0;
  long long a0 = 0, b0 = 0;
  if (ok) {
    a0 = a.aoff[ia]; b0 = a.boff[ib];
    ok = a.aoff[ia + 1] - a0 == np_ && a.boff[ib + 1] - b0 == np_ && np_ <= a.max_n && np_ <= EMD_N_MAX;
  }
  if (!ok) {                                                   // the host wrapper refuses these: status 3, nothing else is touched
    if (RES && tid == 0) {
      a.emd[p] = nan; a.eps_final[p] = nan; a.rounds[p] = 0; a.status[p] = 3;
      stp->fin = 1;
    }
    return;
  }
  if ((np_ <= EMD_N_RES) != RES) return;                       // the other launch's pair
  const int n = (int)np_;
  if (n == 0) {
    if (tid == 0) {
      a.emd[p] = nan; a.eps_final[p] = nan; a.rounds[p] = 0; a.status[p] = 0;
      stp->fin = 1;
    }
    return;
  }
  const float* A = a.A + 3 * a0;
  const float* B = a.B + 3 * b0;

  // ---- where the state lives -------------------------------------------------------------------------------------------------------
  const int n2 = (n + 1) & ~1;                                 // the 8-byte arrays stay aligned
  unsigned long long *bestbits = emd_lds, *mybid;
  double* price;
  int *bestwho, *owner, *assign, *list;
  float *bx, *by, *bz;
  if constexpr (RES) {
    price = (double*)(emd_lds + n2);
    mybid = emd_lds + 2 * n2;
    bestwho = (int*)(emd_lds + 3 * n2);
    owner = bestwho + n2; assign = owner + n2; list = assign + n2;
    bx = (float*)(list + n2); by = bx + n2; bz = by + n2;      // 3 x 8 + 7 x 4 = 52 bytes per point
  } else {
    bestwho = (int*)(emd_lds + n2);                            // 8 + 4 = 12 bytes per point
    price = a.price + q0; mybid = a.mybid + q0;
    owner = a.owner + q0; assign = a.assign + q0; list = a.list + q0;
    bx = a.bx + q0; by = a.by + q0; bz = a.bz + q0;
  }

  double eps = stp->eps, eps_final = stp->eps_final;
  int rounds = stp->rounds;
  const int started = stp->started;
  const long long cap_l = a.max_rounds > 0 ? (long long)a.max_rounds : (long long)EMD_CAP_MUL * n + EMD_CAP_ADD;
  const int cap = cap_l > 0x7FFFFFFFll ? 0x7FFFFFFF : (int)cap_l;
  const int chunk = a.chunk_rounds > 0 ? min(a.chunk_rounds, EMD_CHUNK_MAX) : EMD_CHUNK_DEFAULT;

  if (tid == 0) { s_cnt = 0; s_bad = 0; }
  for (int j = tid; j < n; j += EMD_THREADS) {
    bestbits[j] = 0ull;
    bestwho[j] = EMD_NONE;
    if (RES || !started) { bx[j] = B[3 * j]; by[j] = B[3 * j + 1]; bz[j] = B[3 * j + 2]; }
  }
  __syncthreads();

  if (!started) {
    // the bounding box of A and B together in f32 (min and max are order-free), and whether every coordinate is finite
    const float inf = __int_as_float(0x7F800000);
    float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
    bool bad = false;
    for (int i = tid; i < n; i += EMD_THREADS) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float x = A[3 * i + c], y = B[3 * i + c];
        bad |= !isfinite(x) || !isfinite(y);
        lo[c] = fminf(lo[c], fminf(x, y));
        hi[c] = fmaxf(hi[c], fmaxf(x, y));
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        lo[c] = fminf(lo[c], __shfl_xor(lo[c], o, 64));
        hi[c] = fmaxf(hi[c], __shfl_xor(hi[c], o, 64));
      }
    if (lane == 0)
      for (int c = 0; c < 3; ++c) { s_box[w][c] = lo[c]; s_box[w][3 + c] = hi[c]; }
    if (bad) s_bad = 1;                                        // the same value from every lane that writes
    __syncthreads();
    for (int v = 0; v < EMD_WAVES; ++v)
      for (int c = 0; c < 3; ++c) { lo[c] = fminf(lo[c], s_box[v][c]); hi[c] = fmaxf(hi[c], s_box[v][3 + c]); }
    const double ex = (double)hi[0] - (double)lo[0], ey = (double)hi[1] - (double)lo[1], ez = (double)hi[2] - (double)lo[2];
    const double diag = sqrt((ex * ex + ey * ey) + ez * ez);
    if (s_bad || !(diag < 9223372036854775808.0)) {            // not finite, or a box of 2^63 across whose f32 squares overflow
      for (int i = tid; i < n; i += EMD_THREADS) { a.assign[q0 + i] = -1; a.price[q0 + i] = nan; }
      if (tid == 0) {
        a.emd[p] = nan; a.eps_final[p] = nan; a.rounds[p] = 0; a.status[p] = 2;
        stp->fin = 1;
      }
      return;
    }
    if (diag == 0.0) {                                         // every point is the same point: the identity
      for (int i = tid; i < n; i += EMD_THREADS) { a.assign[q0 + i] = i; a.price[q0 + i] = 0.0; }
      if (tid == 0) {
        a.emd[p] = 0.0; a.eps_final[p] = 0.0; a.rounds[p] = 0; a.status[p] = 0;
        stp->fin = 1;
      }
      return;
    }
    eps_final = a.eps_rel * diag;
    eps = fmax(diag * 0.5, eps_final);
    for (int j = tid; j < n; j += EMD_THREADS) { price[j] = 0.0; owner[j] = -1; assign[j] = -1; }
  } else if (RES) {
    for (int j = tid; j < n; j += EMD_THREADS) { price[j] = a.price[q0 + j]; owner[j] = a.owner[q0 + j]; assign[j] = -1; }
    __syncthreads();
    for (int j = tid; j < n; j += EMD_THREADS) {
      const int i = owner[j];
      if (i >= 0 && i < n) assign[i] = j;
    }
  }
  __syncthreads();

  // ---- rounds ----------------------------------------------------------------------------------------------------------------------
  int done = 0, status = 0;
  bool fin = false;
  long long t_few = stp->t_few, t_all = stp->t_all;            // thread 0's; a timing, not part of the result
  for (int it = 0; it < chunk + EMD_MAX_PHASES + 1; ++it) {    // a pass is a round or a change of phase
    // the unassigned persons (s_cnt is 0 here)
    for (int base = 0; base < n; base += EMD_THREADS) {
      const int i = base + tid;
      const bool un = i < n && assign[i] < 0;
      const unsigned long long mask = __ballot(un);
      if (mask) {                                              // wave-uniform
        const int leader = __ffsll((long long)mask) - 1;
        int at = 0;
        if (lane == leader) at = atomicAdd(&s_cnt, __popcll(mask));
        at = __shfl(at, leader, 64);
        if (un) list[at + __popcll(mask & ((1ull << lane) - 1ull))] = i;
      }
    }
    __syncthreads();
    const int nb = s_cnt;
    if (nb == 0) {                                             // the phase is over
      if (eps == eps_final) { fin = true; break; }
      eps = fmax(eps * 0.25, eps_final);
      for (int j = tid; j < n; j += EMD_THREADS) { owner[j] = -1; assign[j] = -1; }
      __syncthreads();
      continue;
    }
    if (rounds >= cap) { status = 1; fin = true; break; }
    if (done >= chunk) break;
    const long long tick0 = a.ticks && tid == 0 ? wall_clock64() : 0;

    // bids against the prices as they stand: nothing below writes a price before the barrier
    if (nb >= EMD_LANE_MIN) {
      for (int k = tid; k < nb; k += EMD_THREADS) {
        const int i = list[k];
        const float ax = A[3 * i], ay = A[3 * i + 1], az = A[3 * i + 2];
        EmdTop t = {-INFINITY, -INFINITY, EMD_NONE};
        for (int j = 0; j < n; ++j) emd_take(t, (-emd_cost(ax, ay, az, bx[j], by[j], bz[j])) - price[j], j);
        emd_offer(t, i, n, eps, price, assign, mybid, bestbits);
      }
    } else {
      int S = 1;                                               // waves that share a bidder: the largest power of two with nb S <= 16
      while (nb * S * 2 <= EMD_WAVES) S *= 2;
      const int seg = (n + S - 1) / S;
      for (int item = w; item < nb * S; item += EMD_WAVES) {   // S > 1: at most one pass
        const int k = item / S, s = item - k * S;
        const int i = list[k];
        const float ax = A[3 * i], ay = A[3 * i + 1], az = A[3 * i + 2];
        const int jend = min(n, (s + 1) * seg);
        EmdTop t = {-INFINITY, -INFINITY, EMD_NONE};
        for (int j = s * seg + lane; j < jend; j += 64) emd_take(t, (-emd_cost(ax, ay, az, bx[j], by[j], bz[j])) - price[j], j);
        emd_wave_merge(t);
        if (S > 1) {
          if (lane == 0) { s_pv1[item] = t.v1; s_pv2[item] = t.v2; s_pj[item] = t.j1; }
        } else if (lane == 0) {
          emd_offer(t, i, n, eps, price, assign, mybid, bestbits);
        }
      }
      if (S > 1) {                                             // workgroup-uniform
        __syncthreads();
        if (w < nb) {
          EmdTop t = {-INFINITY, -INFINITY, EMD_NONE};
          if (lane < S) { t.v1 = s_pv1[w * S + lane]; t.v2 = s_pv2[w * S + lane]; t.j1 = s_pj[w * S + lane]; }
          emd_wave_merge(t);
          if (lane == 0) {
            emd_offer(t, list[w], n, eps, price, assign, mybid, bestbits);
          }
        }
      }
    }
    __syncthreads();
    // among equal largest bids the lowest bidder
    for (int k = tid; k < nb; k += EMD_THREADS) {
      const int i = list[k];
      const int j1 = -2 - assign[i];
      if (j1 >= 0 && j1 < n && mybid[i] == bestbits[j1]) atomicMin(bestwho + j1, i);
    }
    if (tid == 0) s_cnt = 0;                                   // every lane has read it; the next list is behind two barriers
    __syncthreads();
    // an object that received a bid changes hands.  Its previous owner did not bid and the winner bid for this object alone, so no two
    // lanes write one slot; a loser keeps assign < -1 and is unassigned by that
    for (int j = tid; j < n; j += EMD_THREADS) {
      const unsigned long long bits = bestbits[j];
      if (bits != 0ull) {
        const int who = bestwho[j], prev = owner[j];
        if ((unsigned)who < (unsigned)n) {                        // always: the bidder of the largest bid offered its index
          price[j] = __longlong_as_double((long long)bits);
          if (prev >= 0 && prev < n) assign[prev] = -1;
          owner[j] = who;
          assign[who] = j;
        }
        bestbits[j] = 0ull;
        bestwho[j] = EMD_NONE;
      }
    }
    __syncthreads();
    if (a.ticks && tid == 0) {
      const long long dt = wall_clock64() - tick0;
      t_all += dt;
      if (nb < EMD_FEW) t_few += dt;
    }
    ++rounds;
    ++done;
  }

  // ---- the end of the launch -------------------------------------------------------------------------------------------------------
  if (fin) {
    double sum = 0.0;
    for (int i = tid; i < n; i += EMD_THREADS) {
      int j = assign[i];
      j = j < 0 ? -1 : j;
      a.assign[q0 + i] = j;
      if (RES) a.price[q0 + i] = price[i];
      if (status == 0 && j >= 0) sum += emd_cost(A[3 * i], A[3 * i + 1], A[3 * i + 2], bx[j], by[j], bz[j]);
    }
    sum = sfmi_block_sum_f64<EMD_WAVES>(sum, s_red);
    if (tid == 0) {
      a.emd[p] = status == 0 ? sum / (double)n : nan;
      a.eps_final[p] = eps_final;
      a.rounds[p] = rounds;
      a.status[p] = status;
    }
  } else if (RES) {
    for (int j = tid; j < n; j += EMD_THREADS) { a.price[q0 + j] = price[j]; a.owner[q0 + j] = owner[j]; }
  }
  if (tid == 0) {
    stp->t_few = t_few; stp->t_all = t_all;
    if (a.ticks) { a.ticks[2 * p] = t_few; a.ticks[2 * p + 1] = t_all; }
    stp->eps = eps; stp->eps_final = eps_final; stp->rounds = rounds; stp->status = status; stp->fin = fin ? 1 : 0; stp->started = 1;
    if (!fin) atomicAdd(a.unfinished, 1);
  }
}

}  // namespace

extern "C" {

int sfmi_emd_resident_max(void) { return EMD_N_RES; }
int sfmi_emd_max_points(void) { return EMD_N_MAX; }
int sfmi_emd_default_cap(int n) { return n < 0 || n > EMD_N_MAX ? 0 : EMD_CAP_MUL * n + EMD_CAP_ADD; }
int sfmi_emd_default_chunk(void) { return EMD_CHUNK_DEFAULT; }

size_t sfmi_emd_workspace_bytes(int P, long long N) {
  if (P <= 0 || N < 0 || N >= (1ll << 40)) return 0;
  SfmiCarver c{nullptr};
  EmdArgs a;
  emd_ws(c, P, N, a);
  return c.bytes();
}

int sfmi_emd_f32(const float* A, const long long* aoff, int SA, const float* B, const long long* boff, int SB, const int* pa, const int* pb,
                 const long long* poff, int P, long long N, int max_n, double eps_rel, int max_rounds, int chunk_rounds, int* assign,
                 double* emd, int* rounds, int* status, double* eps_final, double* price, long long* ticks, void* workspace,
                 void* stream) {
  if (P <= 0 || SA <= 0 || SB <= 0 || N < 0 || N >= (1ll << 40) || max_n < 0 || max_n > EMD_N_MAX || !aoff || !boff || !pa || !pb ||
      !poff || !emd || !rounds || !status || !eps_final || !workspace)
    return SFMI_EINVAL;
  if (!(eps_rel >= 1e-9 && eps_rel <= 1.0)) return SFMI_EINVAL;
  if (N > 0 && (!A || !B || !assign || !price)) return SFMI_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  // above the 64 KB default: raised once per process; a refusal is an error the caller sees
  const bool lds_res = SFMI_LDS_ONCE(EMD_RES_BYTES * EMD_N_RES, emd_kernel<true>);
  const bool lds_stream = SFMI_LDS_ONCE(EMD_STREAM_BYTES * EMD_N_MAX, emd_kernel<false>);
  if (!lds_res || !lds_stream) return SFMI_ELDS;

  EmdArgs a;
  a.A = A; a.aoff = aoff; a.SA = SA; a.B = B; a.boff = boff; a.SB = SB; a.pa = pa; a.pb = pb; a.poff = poff;
  a.max_n = max_n; a.max_rounds = max_rounds; a.chunk_rounds = chunk_rounds; a.eps_rel = eps_rel;
  a.assign = assign; a.emd = emd; a.rounds = rounds; a.status = status; a.eps_final = eps_final; a.price = price; a.ticks = ticks;
  SfmiCarver carver{(char*)workspace};
  emd_ws(carver, P, N, a);

  const int res_n = max_n < EMD_N_RES ? max_n : EMD_N_RES;
  const size_t lds_r = (size_t)EMD_RES_BYTES * (size_t)((res_n + 1) & ~1), lds_s = (size_t)EMD_STREAM_BYTES * (size_t)((max_n + 1) & ~1);
  const int chunk = chunk_rounds > 0 ? (chunk_rounds < EMD_CHUNK_MAX ? chunk_rounds : EMD_CHUNK_MAX) : EMD_CHUNK_DEFAULT;
  const long long cap = max_rounds > 0 ? (long long)max_rounds : (long long)EMD_CAP_MUL * max_n + EMD_CAP_ADD;
  const long long max_launches = cap / chunk + 2;              // a pair does `chunk` rounds per launch until it is done or capped

  SFMI_TRY(hipMemsetAsync(a.state, 0, sizeof(EmdState) * (size_t)P, st));
  if (ticks) SFMI_TRY(hipMemsetAsync(ticks, 0, 2 * sizeof(long long) * (size_t)P, st));
  int left = 0;
  for (long long launch = 0; launch < max_launches; ++launch) {
    SFMI_TRY(hipMemsetAsync(a.unfinished, 0, sizeof(int), st));
    hipLaunchKernelGGL(emd_kernel<true>, dim3((unsigned)P), dim3(EMD_THREADS), lds_r, st, a);
    if (max_n > EMD_N_RES) hipLaunchKernelGGL(emd_kernel<false>, dim3((unsigned)P), dim3(EMD_THREADS), lds_s, st, a);
    SFMI_CHECK_LAUNCH();
    SFMI_TRY(hipMemcpyAsync(&left, a.unfinished, sizeof(int), hipMemcpyDeviceToHost, st));
    const hipError_t e = hipStreamSynchronize(st);
    if (e != hipSuccess) return (int)e;
    if (left == 0) return SFMI_OK;
  }
  return SFMI_ELAUNCH;                                         // cannot be: every pair is done or capped by then
}

}  // extern "C"
