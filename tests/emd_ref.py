"""The numpy statement of the deterministic auction of csrc/emd.hip (include/sfmi.h), operation for operation, and of
the set-level metrics MMD / COV / 1-NNA of shapeformer_amd/metrics.py.  Host only.

Bertsekas' forward auction in its Jacobi form with epsilon scaling, as a pure function of the two clouds:

  cost     c_ij = (double) sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx * dx))), (dx, dy, dz) = a_i - b_j in f32
  scale    lo / hi = the f32 minimum / maximum of every coordinate over A and B together; e = (double) hi - (double) lo per axis;
           diag = sqrt((ex ex + ey ey) + ez ez) in f64, every product and sum rounded on its own
  phases   eps_final = eps_rel diag; eps_0 = max(diag / 2, eps_final); eps_{k+1} = max(eps_k / 4, eps_final); the phase run at
           eps_final is the last.  Prices are f64, start at 0 and are kept; every assignment is cleared when a phase starts
  round    every unassigned i bids against the prices of the round's start: v_j = (-c_ij) - price_j; j1 = arg max v, the lowest j among
           equals; v2 = max of v over j != j1 (n = 1: v2 = v1); bid = (price_j1 + (v1 - v2)) + eps.  An object takes its largest bid,
           the lowest i among equals: the bid is its price, its previous owner is unassigned, the bidder owns it
  result   emd = S / n with S the f64 sum of c[i, assign[i]] in the order of `fixed_sum`; rounds = the total over the phases;
           status 0 done, 1 the round cap was reached (emd NaN, assign -1 where unassigned), 2 a coordinate that is not finite or a
           bounding box of 2^63 or more across (emd NaN, assign -1, prices NaN); n = 0: emd NaN, status 0; diag = 0: the identity, emd 0

f32 arithmetic is restated in f64: a difference and a product of f32 values are rounded once by .astype(float32) (the f64 result is
exact or correctly rounded from an exact value), and the fused multiply-add goes through `fmaf32` (round to odd in f64, then to f32).
"""
import numpy as np

N_MAX = 8192
CAP_MUL, CAP_ADD = 320, 256                # the default round cap per pair: CAP_MUL n + CAP_ADD (csrc/emd.hip)
SUM_LANES = 1024                          # the workgroup of the kernel: part of the order of the final sum


def fmaf32(a, b, c):
    """fmaf(a, b, c) of f32 arrays, correctly rounded: the product is exact in f64; the f64 sum is rounded to odd (the inexact result
    whose last bit is even moves one step towards the exact value), after which the rounding to f32 is the rounding of the exact
    value (53 >= 2 * 24 + 2 bits)."""
    p = np.asarray(a, np.float64) * np.asarray(b, np.float64)
    c = np.asarray(c, np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)                                # TwoSum: s + err = p + c exactly
    even = (s.view(np.int64) & 1) == 0
    fix = (err != 0) & even & np.isfinite(s)
    s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def cost_matrix(A, B):
    """(n,3), (m,3) f32 -> (n,m) f64: the kernel's c_ij"""
    A, B = np.asarray(A, np.float32), np.asarray(B, np.float32)
    dx = (A[:, None, 0] - B[None, :, 0]).astype(np.float32)
    dy = (A[:, None, 1] - B[None, :, 1]).astype(np.float32)
    dz = (A[:, None, 2] - B[None, :, 2]).astype(np.float32)
    xx = (dx.astype(np.float64) * dx.astype(np.float64)).astype(np.float32)
    d2 = fmaf32(dz, dz, fmaf32(dy, dy, xx))
    return np.sqrt(d2).astype(np.float64)                          # numpy's f32 sqrt is correctly rounded


def diag_of(A, B):
    P = np.concatenate([np.asarray(A, np.float32), np.asarray(B, np.float32)])
    e = P.max(0).astype(np.float64) - P.min(0).astype(np.float64)
    return float(np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]))


def fixed_sum(x):
    """the kernel's sum of n doubles: lane t of 1024 adds entries t, t + 1024, ... in ascending order from 0.0; the 64 lanes of a wave
    through the xor butterfly (offsets 32, 16, ..., 1), then the 16 wave sums through the same butterfly (offsets 8, 4, 2, 1)"""
    x = np.asarray(x, np.float64)
    pad = (-len(x)) % SUM_LANES
    rows = np.concatenate([x, np.zeros(pad)]).reshape(-1, SUM_LANES)
    acc = np.zeros(SUM_LANES)
    for r in rows:
        acc = acc + r
    v = acc.reshape(16, 64)
    while v.shape[1] > 1:
        h = v.shape[1] // 2
        v = v[:, :h] + v[:, h:]
    v = v[:, 0]
    while len(v) > 1:
        h = len(v) // 2
        v = v[:h] + v[h:]
    return float(v[0])


def default_cap(n):
    return CAP_MUL * n + CAP_ADD


def auction(A, B, eps_rel=1e-4, max_rounds=None, C=None):
    """-> dict(assign (n,) int32, emd, rounds, status, price (n,) f64, eps_final, bids, phase_rounds)"""
    A, B = np.asarray(A, np.float32).reshape(-1, 3), np.asarray(B, np.float32).reshape(-1, 3)
    n = len(A)
    assert len(B) == n and n <= N_MAX and 1e-9 <= eps_rel <= 1
    out = dict(assign=np.full(n, -1, np.int32), emd=float("nan"), rounds=0, status=0, price=np.zeros(n), eps_final=float("nan"),
               bids=0, phase_rounds=[])
    if n == 0:
        return out
    diag = diag_of(A, B) if np.isfinite(A).all() and np.isfinite(B).all() else float("nan")
    if not diag < 2.0 ** 63:
        out.update(status=2, price=np.full(n, np.nan))
        return out
    if diag == 0.0:
        out.update(assign=np.arange(n, dtype=np.int32), emd=0.0, eps_final=0.0)
        return out
    cap = default_cap(n) if max_rounds is None else int(max_rounds)
    C = cost_matrix(A, B) if C is None else C
    eps_final = eps_rel * diag
    eps = max(diag * 0.5, eps_final)
    price = np.zeros(n)
    assign = np.full(n, -1, np.int64)
    owner = np.full(n, -1, np.int64)
    rounds = bids = 0
    status = 0
    in_phase = 0
    while True:
        un = np.nonzero(assign < 0)[0]
        if len(un) == 0:
            out["phase_rounds"].append(in_phase)
            in_phase = 0
            if eps == eps_final:
                break
            eps = max(eps * 0.25, eps_final)
            assign[:] = -1
            owner[:] = -1
            continue
        if rounds >= cap:
            status = 1
            break
        V = (-C[un]) - price[None, :]
        r = np.arange(len(un))
        j1 = np.argmax(V, 1)                                       # the first maximum: the lowest j
        v1 = V[r, j1]
        if n == 1:
            v2 = v1
        else:
            V[r, j1] = -np.inf
            v2 = V.max(1)
        bid = (price[j1] + (v1 - v2)) + eps
        order = np.lexsort((un, -bid, j1))                         # by object, then the larger bid, then the lower bidder
        first = np.ones(len(un), bool)
        first[1:] = j1[order][1:] != j1[order][:-1]
        win = order[first]
        jw, iw = j1[win], un[win]
        prev = owner[jw]
        assign[prev[prev >= 0]] = -1
        price[jw] = bid[win]
        owner[jw] = iw
        assign[iw] = jw
        rounds += 1
        in_phase += 1
        bids += len(un)
    out.update(rounds=rounds, status=status, price=price, eps_final=eps_final, bids=bids)
    a32 = np.where(assign < 0, -1, assign).astype(np.int32)
    out["assign"] = a32
    if status == 0:
        out["emd"] = fixed_sum(C[np.arange(n), assign]) / n
    return out


# ---- set-level metrics on distance matrices (Achlioptas et al. 2018; Yang et al. 2019, PointFlow) -------------------------------------

def first_argmin(D, axis):
    return np.argmin(D, axis)                                      # numpy returns the first minimum: the lowest index


def mmd(D_gr):
    """D_gr (G,R): mean over the reference shapes of the distance to their nearest generated shape"""
    return float(np.asarray(D_gr, np.float64).min(0).mean())


def cov(D_gr):
    """share of the reference shapes that are the nearest reference of some generated shape"""
    D_gr = np.asarray(D_gr, np.float64)
    return len(set(first_argmin(D_gr, 1).tolist())) / D_gr.shape[1]


def one_nna(D_gg, D_gr, D_rr):
    """leave-one-out 1-nearest-neighbour accuracy over the union (generated first): 0.5 is ideal, 1 means the sets are told apart"""
    D_gg, D_gr, D_rr = (np.asarray(x, np.float64) for x in (D_gg, D_gr, D_rr))
    G, R = D_gr.shape
    M = np.block([[D_gg, D_gr], [D_gr.T, D_rr]]).copy()
    np.fill_diagonal(M, np.inf)
    label = np.concatenate([np.zeros(G, int), np.ones(R, int)])
    return float((label[first_argmin(M, 1)] == label).mean())


# ---- the families of tests/test_emd_cpu.py and tests/test_emd_gpu.py ----------------------------------------------------------------------

def shell(n, seed, r=0.5, jitter=0.01):
    rs = np.random.RandomState(seed)
    u = rs.randn(n, 3)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    return (u * r + rs.randn(n, 3) * jitter).astype(np.float32)


def lattice(k=8):
    g = np.arange(k, dtype=np.float32) / np.float32(k)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)


def families(seed=0):
    """name -> (A, B) f32: the CPU test's cases beyond the random shells"""
    rs = np.random.RandomState(seed)
    L = lattice(8)
    base = shell(64, seed + 1)
    t = np.linspace(0, 1, 512).astype(np.float32)
    line = np.stack([t, np.float32(0.5) * t, np.float32(0.25) * t], 1).astype(np.float32)
    c1 = (rs.randn(300, 3) * 0.01).astype(np.float32)
    c2 = (rs.randn(212, 3) * 0.01 + [1, 0, 0]).astype(np.float32)
    d1 = (rs.randn(100, 3) * 0.01).astype(np.float32)
    d2 = (rs.randn(412, 3) * 0.01 + [1, 0, 0]).astype(np.float32)
    far = shell(128, seed + 2)
    return {
        "lattice_reversed": (L, L[::-1].copy()),
        "lattice_half_cell": (L, (L + np.float32(1 / 16)).astype(np.float32)),
        "identical": (shell(200, seed + 3),) * 2,
        "repeated_8x": (np.tile(base, (8, 1)), np.tile(shell(64, seed + 4), (8, 1))),
        "unequal_clusters": (np.concatenate([c1, c2]), np.concatenate([d1, d2])),
        "ten_diameters": (far, (shell(128, seed + 5) + np.float32([10, 0, 0])).astype(np.float32)),
        "collinear_mirror": (line, (-line).astype(np.float32)),
    }
