// Consistent orientation of the normals of a cloud that has no viewpoint: Hoppe et al.'s tangent-plane propagation, what Open3D calls
// orient_normals_consistent_tangent_plane.  The minimum spanning forest of the k-nearest-neighbour graph under the weight 1 - |n_i.n_j|,
// a sign carried along the forest, one global sign per tree by an integer vote.  The reference has no such step: its real-scan datasets
// (shapeformer/data/imnet_datasets/redwood.py, realtest.py) read .pts clouds without normals.  DESIGN.md §5.21; the contract is stated
// in include/sfmi.h and restated in numpy in tests/orient_ref.py.
//
// 1. The forest, Boruvka rounds.  Per vertex: label (its tree's current root, a batch index) and par (the XOR of flip along the tree
//    path to that root).  Per root slot: best_w, best_e, parent, hookflip.  A round is five launches, one thread per vertex:
//      tg_best_kernel<1>  a vertex walks its row; an entry whose ends carry different labels offers bits(w) to best_w of both labels
//                         (64-bit atomicMin; the vertex's own label gets the minimum of the row, folded in registers).
//      tg_best_kernel<2>  entries whose bits(w) equal a label's best_w offer lo << 32 | hi to its best_e: weight and edge identity do
//                         not fit one 64-bit key, so the order (bits(w), lo, hi) is taken in two steps.
//      tg_hook_kernel     a root c with a best edge finds the label o on its other side.  The edges chosen under a strict total order
//                         form a forest apart from mutual pairs (c and o chose the same edge): there the smaller stays root.  Every
//                         other c writes parent[c] = o, hookflip[c] and row c of `tree`: its own slots only, so no CAS.
//      tg_resolve_kernel  an old root follows parent to the new root, XOR-ing hookflip (reads only what the hook launch wrote).
//      tg_relabel_kernel  label = newroot[label], par ^= acc[label]; the old roots' best slots are reset.
//    Every offer is preceded by a relaxed load and skipped when the slot is already smaller: late rounds have few labels and would
//    otherwise serialise on a handful of addresses.
//    The host fixes the number of rounds at ceil(log2(max_n)) (a round at least halves the trees that still have an outgoing edge).
//    flags[r] says whether round r has anything to do: tg_hook_kernel of round r - 1 sets it with its first hook, and every kernel of a
//    round whose flag is 0 returns at once, so the rounds past the last useful one cost five empty launches and no read-back.
// 2. After the rounds: cmin[root] = the smallest local index of the tree (32-bit atomicMin), component = cmin[label], parity relative
//    to that vertex.
// 3. The anchor: the set's centroid (sfmi_centroid_f64, orient_kernel's sum) or its viewpoint gives a direction per point; the votes of
//    a tree are two integer counts (a wave adds up the lanes of equal component before one atomicAdd each); the tree is negated when
//    the second count exceeds the first.  The output is the input normal or its negation, bit for bit.
//
// Only integer atomics whose result is order-free (min, max, add of counts), so every output is a function of the input: no float
// atomics anywhere.  Loop discipline: kernel boundaries are the only synchronisation; no kernel waits on another workgroup and there
// are no spins.  The one data-dependent loop is the resolve walk, capped at the set's size: a cycle would be a bug, and at the cap the
// walk stops and sets status[b].  An index is range-checked before the row it names is read.
#include "sfmi_ragged.h"   // ragged offsets, sfmi_owner, the shared centroid: DESIGN.md §5.5a

// the vote's dot product against p - c has inexact products: every product and sum rounded on its own, here and in numpy
#pragma clang fp contract(off)

namespace {

constexpr int TG_THREADS = 256;
constexpr int TG_MAX_K = 64;
constexpr int TG_MAX_ROUNDS = 31;                // ceil(log2(max_n)) for max_n < 2^31
constexpr int TG_CEN_THREADS = 1024;             // 16 waves, as orient_kernel: the wave count is part of the centroid's summation order
constexpr int TG_CEN_WAVES = TG_CEN_THREADS / 64;
constexpr unsigned long long TG_NONE = ~0ull;    // above every key: bits(w) of a finite w >= 0, and lo << 32 | hi with lo < 2^31

struct TgState {
  int* label;                  // (N) the root of the vertex's tree, a batch index
  int* parent;                 // (N) at a root slot: where it hooked (itself: still a root)
  int* newroot;                // (N) at an old root: the root after the round
  int* cmin;                   // (N) at a final root: the smallest local index of its tree
  unsigned long long* best_w;  // (N) at a root: the least bits(w) among its outgoing edges
  unsigned long long* best_e;  // (N) at a root: the least lo << 32 | hi among those of that weight
  unsigned char* par;          // (N) XOR of flip from the vertex to its root
  unsigned char* hookflip;     // (N) at a hooked root: the parity of the hook
  unsigned char* acc;          // (N) at an old root: the parity from it to the new root
  unsigned char* alive;        // (N)
  int* flags;                  // (TG_MAX_ROUNDS + 2) flags[r] != 0: round r has work
};

// workspace of the forest: best_w, best_e (N u64 each) | label, parent, newroot, cmin (N int32 each) | par, hookflip, acc, alive
// (N bytes each) | flags.  sfmi_tangent_apply_f32 reuses the buffer's start for B centroids (3 f64 each)
inline TgState tg_ws(SfmiCarver& c, long long N) {
  const size_t n = (size_t)N;
  TgState s;
  s.best_w = c.take<unsigned long long>(n); s.best_e = c.take<unsigned long long>(n);
  s.label = c.take<int>(n); s.parent = c.take<int>(n); s.newroot = c.take<int>(n); s.cmin = c.take<int>(n);
  s.par = c.take<unsigned char>(n); s.hookflip = c.take<unsigned char>(n); s.acc = c.take<unsigned char>(n);
  s.alive = c.take<unsigned char>(n);
  s.flags = c.take<int>(TG_MAX_ROUNDS + 2);
  return s;
}

// a vertex is dead when its normal is not finite or is (0,0,0): what sfmi_knn_normals_f32 writes for fewer than 3 neighbours
__device__ __forceinline__ bool tg_alive(const float* __restrict__ n) {
  return sfmi_finite3(n) && (n[0] != 0.f || n[1] != 0.f || n[2] != 0.f);
}

// the f32 components widened to f64: the products are exact, the two sums round
__device__ __forceinline__ double tg_dot(const float* __restrict__ a, const float* __restrict__ b) {
  return ((double)a[0] * (double)b[0] + (double)a[1] * (double)b[1]) + (double)a[2] * (double)b[2];
}

// bits of w = max(0, 1 - |dot|): a non-negative double, whose bits order as integers
__device__ __forceinline__ unsigned long long tg_wbits(double dot) {
  const double w = 1.0 - fabs(dot);
  return (unsigned long long)__double_as_longlong(w > 0.0 ? w : 0.0);
}

// atomicMin behind a relaxed load: the atomic is skipped when the slot is already no larger.  A stale load is an older, larger value:
// it costs an atomic, never a result
__device__ __forceinline__ void tg_offer(unsigned long long* slot, unsigned long long v) {
  if (v < __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(slot, v);
}

__global__ __launch_bounds__(TG_THREADS) void tg_init_kernel(const float* __restrict__ Nrm, int B, long long N, TgState s,
                                                             int* __restrict__ tree, int* __restrict__ rounds,
                                                             int* __restrict__ status) {
  const long long i = (long long)blockIdx.x * TG_THREADS + threadIdx.x;
  if (i < N) {
    s.alive[i] = tg_alive(Nrm + 3 * i) ? 1 : 0;
    s.label[i] = (int)i;
    s.parent[i] = (int)i;
    s.par[i] = 0;
    s.best_w[i] = TG_NONE;
    s.best_e[i] = TG_NONE;
    s.cmin[i] = 0x7FFFFFFF;
    tree[2 * i] = -1;
    tree[2 * i + 1] = -1;
  }
  if (i < B) {
    rounds[i] = 0;
    status[i] = 0;
  }
  if (i < TG_MAX_ROUNDS + 2) s.flags[i] = i == 0 ? 1 : 0;
}

// PHASE 1: the least weight per label.  PHASE 2: among the edges of that weight, the least (lo, hi).
template <int PHASE>
__global__ __launch_bounds__(TG_THREADS) void tg_best_kernel(const float* __restrict__ Nrm, const long long* __restrict__ off,
                                                             const int* __restrict__ idx, int B, long long N, int k, TgState s, int r) {
  if (!s.flags[r]) return;
  const long long i = (long long)blockIdx.x * TG_THREADS + threadIdx.x;
  if (i >= N || !s.alive[i]) return;
  const int b = sfmi_owner(off, B, i);
  const long long base = off[b], n = off[b + 1] - base;
  const int il = (int)(i - base);
  const int li = s.label[i];
  const unsigned long long bw = PHASE == 2 ? s.best_w[li] : 0ull;
  unsigned long long mine = TG_NONE;                           // the row's offers to the vertex's own label, folded in registers
  for (int c = 0; c < k; ++c) {
    const int j = idx[i * k + c];
    if (j < 0 || j >= n || j == il) continue;                  // the index is checked before anything it names is read
    const long long g = base + j;
    if (!s.alive[g]) continue;
    const int lj = s.label[g];
    if (lj == li) continue;
    const unsigned long long w = tg_wbits(tg_dot(Nrm + 3 * i, Nrm + 3 * g));
    if (PHASE == 1) {
      mine = w < mine ? w : mine;
      tg_offer(s.best_w + lj, w);
    } else {
      const unsigned long long e = ((unsigned long long)(unsigned)min(il, j) << 32) | (unsigned)max(il, j);
      if (w == bw) mine = e < mine ? e : mine;
      if (w == s.best_w[lj]) tg_offer(s.best_e + lj, e);
    }
  }
  if (mine != TG_NONE) tg_offer((PHASE == 1 ? s.best_w : s.best_e) + li, mine);
}

__global__ __launch_bounds__(TG_THREADS) void tg_hook_kernel(const float* __restrict__ Nrm, const long long* __restrict__ off, int B,
                                                             long long N, TgState s, int r, int* __restrict__ tree,
                                                             int* __restrict__ rounds) {
  if (!s.flags[r]) return;
  const long long i = (long long)blockIdx.x * TG_THREADS + threadIdx.x;
  if (i >= N) return;
  const int c = (int)i;
  if (s.label[i] != c || s.best_w[i] == TG_NONE) return;       // not a root, or a root without an outgoing edge
  const unsigned long long e = s.best_e[i];
  if (e == TG_NONE) return;                                    // cannot be: the second phase walks the entries the first one walked
  const int b = sfmi_owner(off, B, i);
  const long long base = off[b];
  const long long glo = base + (long long)(e >> 32), ghi = base + (long long)(e & 0xFFFFFFFFull);
  const int la = s.label[glo], lb = s.label[ghi];
  const int o = la == c ? lb : la;
  if (s.best_e[o] == e && c < o) return;                       // a mutual pair: the smaller root stays, the larger hooks
  s.parent[i] = o;
  s.hookflip[i] = (unsigned char)(s.par[glo] ^ s.par[ghi] ^ (tg_dot(Nrm + 3 * glo, Nrm + 3 * ghi) < 0.0 ? 1 : 0));
  tree[2 * i] = (int)(e >> 32);
  tree[2 * i + 1] = (int)(e & 0xFFFFFFFFull);
  // the same value from every thread that hooks; the next launch reads it
  if (!__hip_atomic_load(s.flags + r + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
    __hip_atomic_store(s.flags + r + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (__hip_atomic_load(rounds + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < r + 1) atomicMax(rounds + b, r + 1);
}

// flags[r + 1] != 0: round r hooked something.  An old root follows parent to the root that stayed.  Every slot on the way is a root of
// this round (a label value), so a parent left behind by an earlier round is never read.
__global__ __launch_bounds__(TG_THREADS) void tg_resolve_kernel(const long long* __restrict__ off, int B, long long N, TgState s, int r,
                                                                int* __restrict__ status) {
  if (!s.flags[r + 1]) return;
  const long long i = (long long)blockIdx.x * TG_THREADS + threadIdx.x;
  if (i >= N || s.label[i] != (int)i) return;
  const int b = sfmi_owner(off, B, i);
  const long long n = off[b + 1] - off[b];
  int rt = (int)i, p = s.parent[i];
  unsigned a = 0;
  for (long long step = 0; p != rt && step < n; ++step) {      // a chain has fewer than n links: the cap is reached only by a cycle
    a ^= s.hookflip[rt];
    rt = p;
    p = s.parent[rt];
  }
  if (p != rt) __hip_atomic_store(status + b, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  s.newroot[i] = rt;
  s.acc[i] = (unsigned char)a;
}

__global__ __launch_bounds__(TG_THREADS) void tg_relabel_kernel(long long N, TgState s, int r) {
  if (!s.flags[r + 1]) return;
  const long long i = (long long)blockIdx.x * TG_THREADS + threadIdx.x;
  if (i >= N) return;
  const int l = s.label[i];
  s.label[i] = s.newroot[l];
  s.par[i] ^= s.acc[l];
  if (l == (int)i) {                                           // an old root: the only slots the round's offers reached
    s.best_w[i] = TG_NONE;
    s.best_e[i] = TG_NONE;
  }
}

__global__ __launch_bounds__(TG_THREADS) void tg_cmin_kernel(const long long* __restrict__ off, int B, long long N, TgState s) {
  const long long i = (long long)blockIdx.x * TG_THREADS + threadIdx.x;
  if (i >= N) return;
  const int il = (int)(i - off[sfmi_owner(off, B, i)]);
  int* slot = s.cmin + s.label[i];
  if (il < __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(slot, il);
}

__global__ __launch_bounds__(TG_THREADS) void tg_component_kernel(const long long* __restrict__ off, int B, long long N, TgState s,
                                                                  int* __restrict__ component, unsigned char* __restrict__ parity) {
  const long long i = (long long)blockIdx.x * TG_THREADS + threadIdx.x;
  if (i >= N) return;
  const long long base = off[sfmi_owner(off, B, i)];
  const int cm = s.cmin[s.label[i]];
  component[i] = cm;
  parity[i] = (unsigned char)(s.par[i] ^ s.par[base + cm]);
}

// ---- the anchor: one global sign per tree -------------------------------------------------------------------------------------------

// one workgroup per set: cen[3 b .. 3 b + 2] the centroid of its finite points, NaN for a set without one (then nobody votes)
__global__ __launch_bounds__(TG_CEN_THREADS) void tg_centroid_kernel(const float* __restrict__ P, const long long* __restrict__ off,
                                                                     double* __restrict__ cen) {
  __shared__ double red[TG_CEN_WAVES];
  const int b = blockIdx.x;
  const long long base = off[b], n = off[b + 1] - base;
  double cx = sfmi_nan_f64(), cy = cx, cz = cx;
  sfmi_centroid_f64<TG_CEN_WAVES>(P + 3 * base, n, red, cx, cy, cz);
  if (threadIdx.x == 0) {
    cen[3 * b] = cx; cen[3 * b + 1] = cy; cen[3 * b + 2] = cz;
  }
}

// ref (B,3) f64.  outward != 0: d = p - ref[b] (the centroid); else d = ref[b] - p (the viewpoint).  A dead vertex, and a dot product that
// is 0 or NaN, does not vote.  votes (N,2) int32, zeroed by the caller: row base + c holds the counts of the tree whose component is c.
__global__ __launch_bounds__(TG_THREADS) void tg_vote_kernel(const float* __restrict__ P, const float* __restrict__ Nrm,
                                                             const long long* __restrict__ off, const int* __restrict__ component,
                                                             const unsigned char* __restrict__ parity, const double* __restrict__ ref,
                                                             int outward, int B, long long N, int* __restrict__ votes) {
  const long long i = (long long)blockIdx.x * TG_THREADS + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int key = -1;
  bool pos = false, neg = false;
  if (i < N && tg_alive(Nrm + 3 * i)) {
    const int b = sfmi_owner(off, B, i);
    const double sg = parity[i] ? -1.0 : 1.0;
    const double mx = sg * (double)Nrm[3 * i], my = sg * (double)Nrm[3 * i + 1], mz = sg * (double)Nrm[3 * i + 2];
    const double px = (double)P[3 * i], py = (double)P[3 * i + 1], pz = (double)P[3 * i + 2];
    const double rx = ref[3 * b], ry = ref[3 * b + 1], rz = ref[3 * b + 2];
    const double dx = outward ? px - rx : rx - px, dy = outward ? py - ry : ry - py, dz = outward ? pz - rz : rz - pz;
    const double t = (mx * dx + my * dy) + mz * dz;
    pos = t > 0.0;
    neg = t < 0.0;
    if (pos || neg) key = (int)(off[b] + component[i]);
  }
  // every lane of the wave is here.  The lanes of one tree are counted by ballots and their leader adds the two counts
  unsigned long long todo = __ballot(key >= 0);
  while (todo) {                                               // wave-uniform: one pass per distinct tree among the wave's voters
    const int leader = __ffsll((long long)todo) - 1;
    const int k0 = __shfl(key, leader, 64);
    const bool same = key == k0;
    const unsigned long long m = __ballot(same);
    const int np = __popcll(__ballot(same && pos)), nn = __popcll(__ballot(same && neg));
    if (lane == leader) {
      if (np) atomicAdd(votes + 2ll * k0, np);
      if (nn) atomicAdd(votes + 2ll * k0 + 1, nn);
    }
    todo &= ~m;
  }
}

// out = the input normal, or its negation where parity XOR (the tree's second count exceeds its first): the sign bit alone changes
__global__ __launch_bounds__(TG_THREADS) void tg_apply_kernel(const unsigned* __restrict__ Nrm, const long long* __restrict__ off,
                                                              const int* __restrict__ component, const unsigned char* __restrict__ parity,
                                                              const int* __restrict__ votes, int B, long long N, unsigned* __restrict__ out) {
  const long long i = (long long)blockIdx.x * TG_THREADS + threadIdx.x;
  if (i >= N) return;
  const long long key = off[sfmi_owner(off, B, i)] + component[i];
  const unsigned flip = ((parity[i] != 0) != (votes[2 * key + 1] > votes[2 * key])) ? 0x80000000u : 0u;
  out[3 * i] = Nrm[3 * i] ^ flip;
  out[3 * i + 1] = Nrm[3 * i + 1] ^ flip;
  out[3 * i + 2] = Nrm[3 * i + 2] ^ flip;
}

inline int tg_round_count(long long max_n) {                   // ceil(log2(max_n)); 0 for max_n <= 1
  int r = 0;
  while ((1ll << r) < max_n) ++r;
  return r;
}

}  // namespace

extern "C" {

size_t sfmi_tangent_workspace_bytes(int B, long long N) {
  if (B <= 0 || N < 0 || N >= (1ll << 31)) return 0;
  const size_t forest = sfmi_ws_bytes(tg_ws, N), anchor = align256(sizeof(double) * 3 * (size_t)B);
  return forest > anchor ? forest : anchor;                    // the caller's buffer serves the forest, then apply's centroids
}

int sfmi_tangent_forest_f32(const float* normal, const long long* off, const int* idx, int B, long long N, int k, long long max_n,
                            int* component, int* tree, unsigned char* parity, int* rounds, int* status, void* workspace, void* stream) {
  if (B <= 0 || N < 0 || N >= (1ll << 31) || k < 1 || k > TG_MAX_K || max_n < 0 || max_n > N || !off || !rounds || !status)
    return SFMI_EINVAL;
  if (N > 0 && (!normal || !idx || !component || !tree || !parity || !workspace)) return SFMI_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  SfmiCarver carver{(char*)workspace};
  const TgState s = tg_ws(carver, N);
  const long long items = N > B ? (N > TG_MAX_ROUNDS + 2 ? N : TG_MAX_ROUNDS + 2) : (B > TG_MAX_ROUNDS + 2 ? B : TG_MAX_ROUNDS + 2);
  if (N == 0) {                                                // no workspace: rounds and status alone
    SFMI_TRY(hipMemsetAsync(rounds, 0, sizeof(int) * (size_t)B, st));
    SFMI_TRY(hipMemsetAsync(status, 0, sizeof(int) * (size_t)B, st));
    SFMI_CHECK_LAUNCH();
    return SFMI_OK;
  }
  const dim3 grid(blocks256(N)), block(TG_THREADS);
  hipLaunchKernelGGL(tg_init_kernel, dim3(blocks256(items)), block, 0, st, normal, B, N, s, tree, rounds, status);
  const int R = tg_round_count(max_n);
  for (int r = 0; r < R; ++r) {
    hipLaunchKernelGGL(tg_best_kernel<1>, grid, block, 0, st, normal, off, idx, B, N, k, s, r);
    hipLaunchKernelGGL(tg_best_kernel<2>, grid, block, 0, st, normal, off, idx, B, N, k, s, r);
    hipLaunchKernelGGL(tg_hook_kernel, grid, block, 0, st, normal, off, B, N, s, r, tree, rounds);
    hipLaunchKernelGGL(tg_resolve_kernel, grid, block, 0, st, off, B, N, s, r, status);
    hipLaunchKernelGGL(tg_relabel_kernel, grid, block, 0, st, N, s, r);
  }
  hipLaunchKernelGGL(tg_cmin_kernel, grid, block, 0, st, off, B, N, s);
  hipLaunchKernelGGL(tg_component_kernel, grid, block, 0, st, off, B, N, s, component, parity);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

int sfmi_tangent_apply_f32(const float* P, const float* normal, const long long* off, const int* component, const unsigned char* parity,
                           const double* viewpoint, int B, long long N, int* votes, float* out, void* workspace, void* stream) {
  if (B <= 0 || B > (int)SFMI_MAX_GRID || N < 0 || N >= (1ll << 31) || !off) return SFMI_EINVAL;
  if (N == 0) return SFMI_OK;
  if (!P || !normal || !component || !parity || !votes || !out || (!viewpoint && !workspace)) return SFMI_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(blocks256(N)), block(TG_THREADS);
  SFMI_TRY(hipMemsetAsync(votes, 0, sizeof(int) * 2 * (size_t)N, st));
  const double* ref = viewpoint;
  if (!viewpoint) {
    SfmiCarver carver{(char*)workspace};
    double* cen = carver.take<double>(3 * (size_t)B);          // the `anchor` of sfmi_tangent_workspace_bytes
    hipLaunchKernelGGL(tg_centroid_kernel, dim3((unsigned)B), dim3(TG_CEN_THREADS), 0, st, P, off, cen);
    ref = cen;
  }
  hipLaunchKernelGGL(tg_vote_kernel, grid, block, 0, st, P, normal, off, component, parity, ref, viewpoint ? 0 : 1, B, N, votes);
  hipLaunchKernelGGL(tg_apply_kernel, grid, block, 0, st, (const unsigned*)normal, off, component, parity, votes, B, N, (unsigned*)out);
  SFMI_CHECK_LAUNCH();
  return SFMI_OK;
}

}  // extern "C"
