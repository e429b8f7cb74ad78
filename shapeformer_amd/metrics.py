"""Completion metrics on the device — host side of csrc/pointdist.hip.

How good is a completion: fidelity to the full shape (Chamfer distance, F-score against `Xbd`), faithfulness to the input
(UHD from the partial cloud `Xct`) and diversity over the `sample_n` completions (TMD).  The reference computes distances on
the CPU with scipy cKDTree after a device-to-host copy (xgutils/geoutil.py:362-377 points_dist / chamfer_dist,
shapeformer/models/vqdif/common.py:39-122 chamfer_distance); here every nearest-neighbour query is exact brute force on the
device and the surface samples come straight from `mcubes.marching_cubes_dev`'s tensors.  There is no CPU fallback.

Definitions (d2(a, S) = min_{s in S} |a - s|^2 in f32, direct form; means and sums in f64):
  CD(A, B)           = mean_a d2(a, B) + mean_b d2(b, A)
  fscore(pred, gt)   : P = share of pred points within tau (Euclidean, sqrt(d2) <= tau) of gt, R = share of gt points within
                       tau of pred, F = 2PR / (P + R), and 0 when P + R = 0
  uhd(partial, C)    = per completion c: max_p min_c |p - c| (Euclidean); returned with its mean over the completions
  tmd(S_1..S_k)      = sum_i 1/(k-1) sum_{j != i} CD(S_i, S_j), k >= 2; all k(k-1) directions in one launch
  emd(A, B)          = min over bijections of mean_i |a_i - b_assign(i)| (Euclidean, |A| = |B|), to within eps_rel times the pair's
                       bounding-box diagonal: the deterministic auction of csrc/emd.hip
  set_metrics        MMD, COV and 1-NNA of a generated against a reference collection, under CD or EMD (Achlioptas et al.; PointFlow)
Ragged sets are (points (N,3), offsets (B+1,)) pairs or lists of (n_i,3) tensors; reductions over them are per-set torch sums on
the device (fixed order: deterministic).  The offset convention and the argument checks are _ragged.py's.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L
from . import _ragged
from ._ragged import check_count, check_number, f32_dev, host_offsets, i32_dev, offsets_dev, on_device, pair_sets, point_sets, points_arg


# ---- nearest neighbours over ragged sets (the argument checks are _ragged.py's: DESIGN.md §5.5a) ----------------------------

def _launch_nn(pf, qf, po, qo, want_index):
    """pf (N,3), qf (M,3) f32 contiguous on one device, po / qo validated host offsets -> d2 (N,), idx (N,) int32 or None."""
    dev = pf.device
    B, N, M = len(po) - 1, pf.shape[0], qf.shape[0]
    lib = L.lib()
    d2 = torch.empty(N, device=dev, dtype=torch.float32)
    idx = torch.empty(N, device=dev, dtype=torch.int32) if want_index else None
    if N == 0:
        return d2, idx
    pod, qod = offsets_dev(po, dev), offsets_dev(qo, dev)
    ws = _ragged.workspace(lib.sfmi_nn_dist_workspace_bytes(B, N, M), dev)
    L.check(lib.sfmi_nn_dist_f32(L.ptr(pf), L.ptr(qf), L.ptr(pod), L.ptr(qod), B, N, M, L.ptr(d2), L.ptr(idx), L.ptr(ws),
                                 L.stream_ptr()), "sfmi_nn_dist_f32")
    return d2, idx


def nn_dist(p, q, p_off=None, q_off=None, return_index=False):
    """Exact squared distance from every point of p to its nearest point of q, set by set.

    p (N,3) / q (M,3) f32 HIP tensors with (B+1,) exclusive offsets p_off / q_off (None: one set), or p (B,N,3) / q (B,M,3)
    batches (set b of p against set b of q; offsets must then be None).  -> d2 (N,) f32 (or (B,N)) and, with return_index, the
    int32 index of that nearest point local to its set of q: the lowest index among equal f32 distances.  Bit-identical from
    run to run.  A set of q with no points while its set of p has some raises SfmiError."""
    p, q, po, qo, shape = pair_sets(p, q, p_off, q_off, "nn_dist", ("p", "q"), None)
    if ((np.diff(qo) == 0) & (np.diff(po) > 0)).any():
        raise L.SfmiError("nn_dist: a reference set is empty while its query set is not")
    on_device("nn_dist", p, q)
    d2, idx = _launch_nn(p.float().contiguous(), q.float().contiguous(), po, qo, return_index)
    if shape:
        d2 = d2.reshape(shape)
        idx = idx.reshape(shape) if idx is not None else None
    return (d2, idx) if return_index else d2


def _pack(sets, what):
    """list of (n_i,3) tensors or a (k,n,3) tensor -> (points (sum n_i,3) f32 contiguous, host offsets)."""
    if isinstance(sets, torch.Tensor):
        points_arg(sets, what)
        on_device(what, sets)
        if sets.dim() == 2:
            sets = sets[None]
        k, n = sets.shape[0], sets.shape[1]
        return sets.reshape(-1, 3).float().contiguous(), np.arange(k + 1, dtype=np.int64) * n
    sets = [points_arg(s, what) for s in sets]
    if not sets or any(s.dim() != 2 for s in sets):
        raise L.SfmiError(f"{what}: expected a non-empty list of (n_i,3) tensors")
    on_device(what, *sets)
    off = np.concatenate([[0], np.cumsum([s.shape[0] for s in sets])]).astype(np.int64)
    return torch.cat([s.float() for s in sets]).contiguous(), off


def _directions(pairs, want_index=False):
    """[(P_i (n_i,3), Q_i (m_i,3))] -> ONE ragged launch: d2 (sum n_i,), host offsets (, idx)."""
    for a, b in pairs:
        if b.shape[0] == 0 and a.shape[0] > 0:
            raise L.SfmiError("nn_dist: a reference set is empty while its query set is not")
    on_device("metrics", *[t for pq in pairs for t in pq])
    po = np.concatenate([[0], np.cumsum([a.shape[0] for a, _ in pairs])]).astype(np.int64)
    qo = np.concatenate([[0], np.cumsum([b.shape[0] for _, b in pairs])]).astype(np.int64)
    pf = torch.cat([a for a, _ in pairs]).float().contiguous()
    qf = torch.cat([b for _, b in pairs]).float().contiguous()
    d2, idx = _launch_nn(pf, qf, po, qo, want_index)
    return (d2, po, idx) if want_index else (d2, po)


def _seg(d, off, op):
    """per-set f64 sum / max of the ragged vector d (B tensors on the device, fixed reduction order)."""
    B = len(off) - 1
    n = np.diff(off)
    if B > 1 and (n == n[0]).all() and n[0] > 0:
        v = d.double().reshape(B, int(n[0]))
        return v.sum(1) if op == "sum" else v.max(1).values
    out = []
    for b in range(B):
        s = d[int(off[b]):int(off[b + 1])].double()
        out.append(s.sum() if op == "sum" else (s.max() if s.numel() else torch.tensor(float("nan"), device=d.device, dtype=torch.float64)))
    return torch.stack(out)


def _seg_mean(d, off):
    return _seg(d, off, "sum") / torch.from_numpy(np.diff(off).astype(np.float64)).to(d.device)


# ---- metrics ------------------------------------------------------------------------------------------------------------------

def chamfer(a, b):
    """CD(A, B) = mean_a d2(a, B) + mean_b d2(b, A) (squared distances, f64 means) -> float."""
    a, b = points_arg(a, "chamfer a"), points_arg(b, "chamfer b")
    d, off = _directions([(a.reshape(-1, 3), b.reshape(-1, 3)), (b.reshape(-1, 3), a.reshape(-1, 3))])
    return float(_seg_mean(d, off).sum())


def fscore(pred, gt, tau=0.01, return_pr=False):
    """F-score at threshold tau: precision P = share of pred points within tau (Euclidean: sqrt(d2) <= tau, in f64) of gt,
    recall R = share of gt points within tau of pred, F = 2PR/(P+R), 0 when P+R = 0.  -> F (, P, R)."""
    pred, gt = points_arg(pred, "fscore pred").reshape(-1, 3), points_arg(gt, "fscore gt").reshape(-1, 3)
    d, off = _directions([(pred, gt), (gt, pred)])
    within = (d.double().sqrt() <= tau).double()
    pr = (_seg(within, off, "sum") / torch.from_numpy(np.diff(off).astype(np.float64)).to(d.device)).cpu().numpy()
    P, R = float(pr[0]), float(pr[1])
    F = 0.0 if P + R == 0 else 2 * P * R / (P + R)
    return (F, P, R) if return_pr else F


def uhd(partial, completions):
    """Unidirectional Hausdorff distance from the partial cloud to each completion: max_p min_c |p - c| (Euclidean).
    completions: list of (n_i,3) tensors or a (k,n,3) tensor.  -> (per-completion f64 numpy (k,), their mean)."""
    partial = points_arg(partial, "uhd partial").reshape(-1, 3)
    cf, co = _pack(completions, "uhd completions")
    k = len(co) - 1
    d, off = _directions([(partial, cf[int(co[i]):int(co[i + 1])]) for i in range(k)])
    per = _seg(d, off, "max").sqrt().cpu().numpy()
    return per, float(per.mean())


def tmd_directions(completions):
    """The k(k-1) Chamfer directions of TMD as ONE ragged launch: direction (i, j), i != j in row-major order, queries S_i
    against S_j.  -> (d2 ragged (sum,), host offsets (k(k-1)+1,), [(i, j), ...])."""
    cf, co = _pack(completions, "tmd completions")
    k = len(co) - 1
    if k < 2:
        raise L.SfmiError("tmd needs k >= 2 completions")
    S = [cf[int(co[i]):int(co[i + 1])] for i in range(k)]
    pairs = [(i, j) for i in range(k) for j in range(k) if i != j]
    d, off = _directions([(S[i], S[j]) for i, j in pairs])
    return d, off, pairs


def _tmd_from(d, off, pairs, k):
    m = _seg_mean(d, off).cpu().numpy()
    mean = {pq: m[n] for n, pq in enumerate(pairs)}
    return float(sum(sum(mean[(i, j)] + mean[(j, i)] for j in range(k) if j != i) / (k - 1) for i in range(k)))


def tmd(completions):
    """Total mutual difference: sum_i 1/(k-1) sum_{j != i} CD(S_i, S_j), CD(A, B) = mean_a d2(a, B) + mean_b d2(b, A), k >= 2.
    completions: list of (n_i,3) tensors or a (k,n,3) tensor.  All k(k-1) directions run in one launch.  -> float."""
    d, off, pairs = tmd_directions(completions)
    return _tmd_from(d, off, pairs, pairs[-1][0] + 1)


def evaluate(Xct, completions, Xbd=None, tau=0.01, emd_n=None):
    """Metrics of the completions of ONE partial cloud: {"k", "uhd", "uhd_per", "tmd" (k >= 2)} and, with the full shape Xbd,
    {"cd", "cd_per", "fscore", "fscore_per", "tau"} (CD / F-score of each completion against Xbd; *_per in completion order,
    the plain key is their mean).  Definitions in the module docstring.  numpy inputs are moved to the completions' device.
    emd_n (needs Xbd): every completion and Xbd are brought to emd_n points by farthest point sampling and {"emd", "emd_per",
    "emd_n"} are added (a pair the auction did not finish is NaN); a cloud with fewer points raises SfmiError.  Without emd_n the
    result is what it was before the key existed."""
    if emd_n is not None:
        emd_n = check_count(emd_n, "evaluate", "emd_n")
        if emd_n > EMD_MAX_POINTS:
            raise L.SfmiError(f"evaluate: emd_n must be at most {EMD_MAX_POINTS}, got {emd_n}")
        if Xbd is None:
            raise L.SfmiError("evaluate: emd_n needs the full shape Xbd")
    if isinstance(completions, torch.Tensor):
        dev = completions.device
    else:
        dev = completions[0].device if len(completions) and isinstance(completions[0], torch.Tensor) else torch.device("cuda")
        completions = [f32_dev(c, dev) for c in completions]
    Xct = f32_dev(Xct, dev).reshape(-1, 3)
    cf, co = _pack(completions, "evaluate completions")
    on_device("evaluate", cf, Xct, *([Xbd] if isinstance(Xbd, torch.Tensor) else []))       # every cloud, before the first launch
    k = len(co) - 1
    S = [cf[int(co[i]):int(co[i + 1])] for i in range(k)]
    per, mean = uhd(Xct, S)
    out = {"k": k, "uhd": mean, "uhd_per": per.tolist()}
    if k >= 2:
        out["tmd"] = tmd(S)
    if Xbd is not None:
        X = f32_dev(Xbd, dev).reshape(-1, 3)
        d, off = _directions([(s, X) for s in S] + [(X, s) for s in S])
        m = _seg_mean(d, off).cpu().numpy()
        cd = m[:k] + m[k:]
        within = (d.double().sqrt() <= tau).double()
        frac = (_seg(within, off, "sum") / torch.from_numpy(np.diff(off).astype(np.float64)).to(d.device)).cpu().numpy()
        f = [0.0 if P + R == 0 else 2 * P * R / (P + R) for P, R in zip(frac[:k].tolist(), frac[k:].tolist())]
        out.update(cd=float(cd.mean()), cd_per=cd.tolist(), fscore=float(np.mean(f)), fscore_per=f, tau=float(tau))
        if emd_n is not None:
            from .scan import farthest_point_sample_dev
            if X.shape[0] < emd_n or (np.diff(co) < emd_n).any():
                raise L.SfmiError(f"evaluate: emd_n = {emd_n} but a cloud has fewer points")
            pts, po = torch.cat([cf, X.float()]).contiguous(), np.concatenate([co, [co[-1] + X.shape[0]]]).astype(np.int64)
            idx = farthest_point_sample_dev(pts, po, emd_n)[0].long() + torch.from_numpy(po[:-1]).to(dev)[:, None]
            sub = pts[idx.reshape(-1)].reshape(k + 1, emd_n, 3)
            per = emd_dev(sub[:k], sub[k:], pairs=np.stack([np.arange(k), np.zeros(k, np.int64)], 1)).cpu().numpy()
            out.update(emd=float(per.mean()), emd_per=per.tolist(), emd_n=emd_n)
    return out


# ---- earth mover's distance (csrc/emd.hip) ---------------------------------------------------------------------

EMD_MAX_POINTS = 8192                  # csrc/emd.hip EMD_N_MAX, checked here before the library loads
EMD_BUDGET = 512 << 20                 # bytes of outputs and workspace per launch string of pairwise_emd_dev (48 per point)
CD_BUDGET = 256 << 20                  # bytes of gathered points and distances per launch of pairwise_chamfer_dev (32 per point)


def _collection(x, off, what):
    """(N,3) points with offsets, a (B,n,3) batch or a list of (n_i,3) tensors -> (points (N,3), host offsets (S+1,))"""
    if isinstance(x, (list, tuple)):
        if off is not None:
            raise L.SfmiError(f"{what}: offsets go with (N,3) points, not with a list of clouds")
        sets = [points_arg(t, what) for t in x]
        if not sets or any(t.dim() != 2 for t in sets):
            raise L.SfmiError(f"{what}: expected a non-empty list of (n_i,3) tensors")
        o = np.concatenate([[0], np.cumsum([t.shape[0] for t in sets])]).astype(np.int64)
        return torch.cat([t.float() for t in sets]), o
    pts, o, _ = point_sets(x, off, what)
    return pts, o


def emd_dev(a, b, a_off=None, b_off=None, pairs=None, eps_rel=1e-4, max_rounds=None, chunk_rounds=None, details=False, ticks=False):
    """Earth mover's distance of pairs of equal-sized clouds: the mean Euclidean cost of a bijection that is optimal to within
    eps_final = eps_rel x the diagonal of the pair's bounding box (emd_opt <= emd <= emd_opt + eps_final), by a deterministic auction.

    a / b: two collections of clouds, each (N,3) f32 points with (S+1,) exclusive offsets, a (S,n,3) batch or a list of (n_i,3)
    tensors, on the HIP device.  pairs None: set s of a against set s of b.  pairs (P,2) integers: cloud pairs[k,0] of a against cloud
    pairs[k,1] of b; the points are indexed, never copied per pair.  The two clouds of a pair must have the same number of points, at
    most 8192, else SfmiError.  eps_rel in [1e-9, 1].  max_rounds: the cap on auction rounds per pair (None: 320 n + 256, 16 times the
    worst total found: DESIGN.md §5.22); chunk_rounds: rounds per launch (None: the measured default).  The result does not depend on
    chunk_rounds, on the batch around a pair or on the run, bit for bit; the call synchronises once per launch.
    -> emd (P,) f64 on the device; with details also a dict: assign (sum n,) int32 (b's point for each of a's, local to the cloud),
    offsets (P+1,) host int64 cutting it, price (sum n,) f64, rounds (P,) int32, status (P,) int32, eps_final (P,) f64.
    With ticks (a timing for tools/kbench_emd.py, no part of the result) the dict also holds ticks (P,2) int64: the device's 100 MHz
    clock spent in rounds with fewer than 16 bidders, and in all rounds.
    status 0 done; 1 max_rounds reached (emd NaN, assign -1 where unassigned); 2 a non-finite coordinate (emd NaN, assign -1).
    An empty pair: emd NaN, status 0.  Clouds that are one repeated point: the identity, emd 0.
    The auction is not symmetric in its arguments: emd_dev(b, a) is within eps_final of emd_dev(a, b), not equal to it."""
    what = "emd_dev"
    a, ao = _collection(a, a_off, f"{what} a")
    b, bo = _collection(b, b_off, f"{what} b")
    SA, SB = len(ao) - 1, len(bo) - 1
    if pairs is None:
        if SA != SB:
            raise L.SfmiError(f"{what}: a has {SA} clouds, b has {SB}; unequal collections need `pairs`")
        pa = pb = np.arange(SA, dtype=np.int64)
    else:
        pr = pairs.detach().cpu().numpy() if isinstance(pairs, torch.Tensor) else np.asarray(pairs)
        if pr.ndim != 2 or pr.shape[1] != 2 or not np.issubdtype(pr.dtype, np.integer):
            raise L.SfmiError(f"{what}: pairs must be a (P,2) integer array")
        pa, pb = pr[:, 0].astype(np.int64), pr[:, 1].astype(np.int64)
        if ((pa < 0) | (pa >= SA) | (pb < 0) | (pb >= SB)).any():
            raise L.SfmiError(f"{what}: a pair names a cloud outside its collection ({SA} and {SB} clouds)")
    na, nb = np.diff(ao)[pa], np.diff(bo)[pb]
    if (na != nb).any():
        k = int(np.nonzero(na != nb)[0][0])
        raise L.SfmiError(f"{what}: the clouds of a pair must have equal sizes; pair {k} has {int(na[k])} and {int(nb[k])} points")
    if (na > EMD_MAX_POINTS).any():
        raise L.SfmiError(f"{what}: a cloud has more than {EMD_MAX_POINTS} points")
    eps_rel = check_number(eps_rel, what, "eps_rel", 1e-9, 1.0)
    max_rounds = 0 if max_rounds is None else check_count(max_rounds, what, "max_rounds")
    chunk_rounds = 0 if chunk_rounds is None else check_count(chunk_rounds, what, "chunk_rounds")
    P = len(pa)
    if P >= 2 ** 31:
        raise L.SfmiError(f"{what}: at most 2^31 - 1 pairs")
    dev = on_device(what, a, b)
    po = np.concatenate([[0], np.cumsum(na)]).astype(np.int64)
    N = int(po[-1])
    emd_ = torch.empty(P, device=dev, dtype=torch.float64)
    rounds, status = (torch.empty(P, device=dev, dtype=torch.int32) for _ in range(2))
    eps_final = torch.empty(P, device=dev, dtype=torch.float64)
    assign = torch.empty(N, device=dev, dtype=torch.int32)
    price = torch.empty(N, device=dev, dtype=torch.float64)
    tk = torch.zeros(P, 2, device=dev, dtype=torch.int64) if ticks else None
    if P > 0:
        lib = L.lib()
        af, bf = a.float().contiguous(), b.float().contiguous()
        aod, bod, pod = offsets_dev(ao, dev), offsets_dev(bo, dev), offsets_dev(po, dev)
        pad, pbd = i32_dev(pa, dev), i32_dev(pb, dev)
        ws = _ragged.workspace(lib.sfmi_emd_workspace_bytes(P, N), dev)
        L.check(lib.sfmi_emd_f32(L.ptr(af), L.ptr(aod), SA, L.ptr(bf), L.ptr(bod), SB, L.ptr(pad), L.ptr(pbd), L.ptr(pod), P, N,
                                 int(na.max()), eps_rel, max_rounds, chunk_rounds, L.ptr(assign), L.ptr(emd_), L.ptr(rounds),
                                 L.ptr(status), L.ptr(eps_final), L.ptr(price), L.ptr(tk), L.ptr(ws), L.stream_ptr()), "sfmi_emd_f32")
    if details:
        d = dict(assign=assign, offsets=po, price=price, rounds=rounds, status=status, eps_final=eps_final)
        if ticks:
            d["ticks"] = tk
        return emd_, d
    return emd_


def emd(a, b, **kw):
    """EMD of ONE pair of (n,3) clouds of equal size (emd_dev's contract and keywords) -> float."""
    a, b = points_arg(a, "emd a"), points_arg(b, "emd b")
    return float(emd_dev(a.reshape(-1, 3), b.reshape(-1, 3), **kw)[0])


def _grid(kx, ky, within):
    """the pairs of a distance matrix: every (i, j), or i < j of a matrix within one collection"""
    if within:
        i, j = np.triu_indices(kx, 1)
    else:
        i, j = np.divmod(np.arange(kx * ky), ky)
    return i.astype(np.int64), j.astype(np.int64)


def _chunks(cost, budget):
    """cut the pairs, in order, into runs whose summed cost (bytes) stays within budget; a run has at least one pair"""
    out, lo, acc = [], 0, 0
    for k, c in enumerate(cost.tolist()):
        if k > lo and acc + c > budget:
            out.append((lo, k))
            lo, acc = k, 0
        acc += c
    if len(cost) > lo:
        out.append((lo, len(cost)))
    return out


def _mirror(D, within):
    return D + D.T if within else D


def pairwise_chamfer_dev(X, Y=None):
    """The (len(X), len(Y)) f64 matrix of Chamfer distances CD(X_i, Y_j) (the module's definition) on the device.  X / Y: lists of
    (n_i,3) tensors or (k,n,3) batches; no cloud may be empty.  Y None: the matrix within X: i < j is computed and mirrored (CD is
    symmetric bit for bit: its two means are added in f64), the diagonal is 0.  The directions of a run of pairs are one launch of the
    nearest-neighbour kernel; a run holds as many pairs as keep its gathered points and distances within 256 MiB."""
    within = Y is None
    xf, xo = _pack(X, "pairwise_chamfer_dev X")
    yf, yo = (xf, xo) if within else _pack(Y, "pairwise_chamfer_dev Y")
    if (np.diff(xo) == 0).any() or (np.diff(yo) == 0).any():
        raise L.SfmiError("pairwise_chamfer_dev: a cloud is empty")
    dev = on_device("pairwise_chamfer_dev", xf, yf)
    kx, ky = len(xo) - 1, len(yo) - 1
    D = torch.zeros(kx, ky, device=dev, dtype=torch.float64)
    pi, pj = _grid(kx, ky, within)
    Xs = [xf[int(xo[i]):int(xo[i + 1])] for i in range(kx)]
    Ys = Xs if within else [yf[int(yo[j]):int(yo[j + 1])] for j in range(ky)]
    for lo, hi in _chunks((np.diff(xo)[pi] + np.diff(yo)[pj]) * 32, CD_BUDGET):
        ii, jj = pi[lo:hi], pj[lo:hi]
        d, off = _directions([(Xs[i], Ys[j]) for i, j in zip(ii, jj)] + [(Ys[j], Xs[i]) for i, j in zip(ii, jj)])
        m = _seg_mean(d, off)
        D[torch.from_numpy(ii).to(dev), torch.from_numpy(jj).to(dev)] = m[:hi - lo] + m[hi - lo:]
    return _mirror(D, within)


def pairwise_emd_dev(X, Y=None, **kw):
    """The (len(X), len(Y)) f64 matrix of emd_dev(X_i, Y_j, **kw) on the device (NaN where a pair's status is not 0).  X / Y: lists of
    (n,3) tensors or (k,n,3) batches, every cloud of one size.  The pairs index the two collections, one workgroup per pair; a run of
    pairs holds as many as keep its outputs and workspace within 512 MiB.  Y None: the matrix within X: i < j is computed as
    emd_dev(X_i, X_j) and mirrored, the diagonal is 0.  The auction is not symmetric in its arguments (emd_dev(b, a) is within
    eps_final of emd_dev(a, b), not equal), so the mirrored entry is the one of the upper triangle by definition."""
    within = Y is None
    xf, xo = _collection(X, None, "pairwise_emd_dev X")
    yf, yo = (xf, xo) if within else _collection(Y, None, "pairwise_emd_dev Y")
    kx, ky = len(xo) - 1, len(yo) - 1
    if len(set(np.diff(xo).tolist()) | set(np.diff(yo).tolist())) > 1:
        raise L.SfmiError("pairwise_emd_dev: the clouds of a pair must have equal sizes, so every cloud must have one size")
    pi, pj = _grid(kx, ky, within)
    dev = on_device("pairwise_emd_dev", xf, yf)
    D = torch.zeros(kx, ky, device=dev, dtype=torch.float64)
    for lo, hi in _chunks(np.diff(xo)[pi] * 48 + 64, EMD_BUDGET):
        ii, jj = pi[lo:hi], pj[lo:hi]
        D[torch.from_numpy(ii).to(dev), torch.from_numpy(jj).to(dev)] = emd_dev(xf, yf, xo, yo, pairs=np.stack([ii, jj], 1), **kw)
    return _mirror(D, within)


def _first_argmin(D, dim):
    """arg min along dim, the lowest index among equal values (torch.argmin leaves that open on the device)"""
    n = D.shape[dim]
    idx = torch.arange(n, device=D.device).reshape([-1 if d == dim else 1 for d in range(D.dim())])
    return torch.where(D == D.min(dim, keepdim=True).values, idx, n).min(dim).values


def metrics_from_matrices(D_gr, D_gg, D_rr):
    """MMD, COV and 1-NNA from the distance matrices generated x reference (G,R), within generated (G,G), within reference (R,R):
      mmd   the mean over the reference shapes of the distance to their nearest generated shape
      cov   the share of the reference shapes that are the nearest reference of some generated shape
      1nna  the leave-one-out 1-nearest-neighbour accuracy over the union: 0.5 when the two sets cannot be told apart
    Every arg min takes the lowest index among equal values (in the union the generated shapes come first).  Small torch arithmetic
    on the matrices' device.  -> {"mmd", "cov", "1nna"} floats."""
    G, R = D_gr.shape
    if G == 0 or R == 0 or D_gg.shape != (G, G) or D_rr.shape != (R, R):
        raise L.SfmiError(f"set metrics: expected (G,R), (G,G) and (R,R) matrices with G, R >= 1, got {tuple(D_gr.shape)}, "
                          f"{tuple(D_gg.shape)}, {tuple(D_rr.shape)}")
    D_gr, D_gg, D_rr = D_gr.double(), D_gg.double(), D_rr.double()
    mmd = D_gr.min(0).values.mean()
    hit = torch.zeros(R, device=D_gr.device, dtype=torch.bool)
    hit[_first_argmin(D_gr, 1)] = True
    M = torch.cat([torch.cat([D_gg, D_gr], 1), torch.cat([D_gr.T, D_rr], 1)], 0).clone()
    M.fill_diagonal_(float("inf"))
    label = torch.cat([torch.zeros(G, device=M.device, dtype=torch.long), torch.ones(R, device=M.device, dtype=torch.long)])
    acc = (label[_first_argmin(M, 1)] == label).double().mean()
    return {"mmd": float(mmd), "cov": float(hit.double().mean()), "1nna": float(acc)}


def set_metrics(gen, ref, metric="cd", **kw):
    """How well a collection of generated shapes covers a collection of reference shapes: {"mmd", "cov", "1nna"}
    (metrics_from_matrices) and "D_gr", the (len(gen), len(ref)) f64 distance matrix on the device, under metric "cd"
    (pairwise_chamfer_dev) or "emd" (pairwise_emd_dev; kw are emd_dev's eps_rel / max_rounds / chunk_rounds).  gen / ref: lists of
    (n,3) tensors or (k,n,3) batches."""
    if metric not in ("cd", "emd"):
        raise L.SfmiError(f'set_metrics: metric must be "cd" or "emd", got {metric!r}')
    if metric == "cd" and kw:
        raise L.SfmiError(f"set_metrics: {sorted(kw)} go with metric=\"emd\"")
    pw = pairwise_chamfer_dev if metric == "cd" else (lambda X, Y=None: pairwise_emd_dev(X, Y, **kw))
    D_gr = pw(gen, ref)
    out = metrics_from_matrices(D_gr, pw(gen), pw(ref))
    out["D_gr"] = D_gr
    return out


# ---- surface sampling ---------------------------------------------------------------------------------------------------------

def sample_mesh_dev(verts, faces, voff, toff, n, seed=0, return_face=False):
    """n area-weighted surface points per shape of a batch of indexed meshes (marching_cubes_dev's output: verts (V,3) f32,
    faces (T,3) int32 local per shape, host voff / toff (B+1,)).  Face by binary search of a counter-hash uniform of (seed, k)
    in the shape's f64 area CDF; barycentric weights 1-sqrt(u), sqrt(u)(1-v), sqrt(u) v (geoutil.sampleMesh).  Sample k of a
    shape depends on (seed, k) and that mesh only, so a batch equals per-shape calls.  Does not touch any global RNG.
    -> points (B*n,3) f32, status (B,) int32 (1: zero / non-finite total area, its points NaN) (, face (B*n,) int32 local).
    A shape without faces raises SfmiError."""
    if not isinstance(verts, torch.Tensor) or not isinstance(faces, torch.Tensor):
        raise L.SfmiError("sample_mesh_dev: verts / faces must be torch tensors on the HIP device")
    if verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise L.SfmiError("sample_mesh_dev: expected verts (V,3) and faces (T,3)")
    vo, to = host_offsets(voff, verts.shape[0], "sample_mesh_dev voff"), host_offsets(toff, faces.shape[0], "sample_mesh_dev toff")
    if len(vo) != len(to):
        raise L.SfmiError("sample_mesh_dev: voff and toff describe different batch sizes")
    if (np.diff(to) == 0).any():
        raise L.SfmiError("sample_mesh_dev: a shape has no faces")
    if int(n) < 0:
        raise L.SfmiError("sample_mesh_dev: n must be >= 0")
    dev = on_device("sample_mesh_dev", verts, faces)
    lib = L.lib()
    B, T, n = len(vo) - 1, faces.shape[0], int(n)
    vf, ff = verts.float().contiguous(), faces.to(torch.int32).contiguous()
    out = torch.empty(B * n, 3, device=dev, dtype=torch.float32)
    face = torch.empty(B * n, device=dev, dtype=torch.int32) if return_face else None
    status = torch.empty(B, device=dev, dtype=torch.int32)
    vod, tod = offsets_dev(vo, dev), offsets_dev(to, dev)
    ws = _ragged.workspace(lib.sfmi_mesh_sample_workspace_bytes(B, T), dev)
    L.check(lib.sfmi_mesh_sample_f32(L.ptr(vf), L.ptr(ff), L.ptr(vod), L.ptr(tod), B, T, n, int(seed) & (2 ** 64 - 1), L.ptr(ws),
                                     L.ptr(out), L.ptr(face), L.ptr(status), L.stream_ptr()), "sfmi_mesh_sample_f32")
    return (out, status, face) if return_face else (out, status)


# ---- reference signatures (numpy in, numpy out) ------------------------------------------------------------------------------

def points_dist(p1, p2, k=1, return_ind=False):
    """geoutil.points_dist: Euclidean distance from each point of p1 to its nearest point of p2 (f64 numpy) (, the int64 index of
    that point).  2 <= k <= 64: (N,k) distances (, indices) to the k nearest, ascending, as cKDTree.query(p1, k) returns them
    (scan.knn_dev; fewer than k points in p2: inf, and -1 where scipy writes len(p2))."""
    if k != 1:
        from .scan import knn_dev
        d2, idx = knn_dev(f32_dev(p1).reshape(-1, 3), f32_dev(p2).reshape(-1, 3), k)
        dist = np.sqrt(d2.cpu().numpy().astype(np.float64))
        return (dist, idx.cpu().numpy().astype(np.int64)) if return_ind else dist
    d2, idx = nn_dist(f32_dev(p1).reshape(-1, 3), f32_dev(p2).reshape(-1, 3), return_index=True)
    dist = np.sqrt(d2.cpu().numpy().astype(np.float64))
    return (dist, idx.cpu().numpy().astype(np.int64)) if return_ind else dist


def chamfer_dist(p1, p2):
    """geoutil.chamfer_dist: (squared distances p1 -> p2, squared distances p2 -> p1), f64 numpy, in one launch."""
    a, b = f32_dev(p1).reshape(-1, 3), f32_dev(p2).reshape(-1, 3)
    d, off = _directions([(a, b), (b, a)])
    d = d.cpu().numpy().astype(np.float64)
    return d[:off[1]], d[off[1]:]


def chamfer_distance(points1, points2, use_kdtree=True, give_id=False):
    """vqdif/common.py chamfer_distance on (B,N,3) / (B,M,3) batches: chamfer1 = mean d2(points1 -> points2), chamfer2 =
    mean d2(points2 -> points1) per batch item; returns chamfer1 + chamfer2, or (chamfer1, chamfer2, idx_nn_12, idx_nn_21)
    with give_id.  torch in -> torch out on the input's device (means in points1's dtype, int64 indices; the search itself is f32); numpy in -> numpy out.
    use_kdtree is accepted and ignored (the search is exact either way)."""
    as_np = not isinstance(points1, torch.Tensor)
    a = f32_dev(points1)
    b = f32_dev(points2, a.device)
    B, n, m = a.shape[0], a.shape[1], b.shape[1]
    d, off, idx = _directions([(a[i], b[i]) for i in range(B)] + [(b[i], a[i]) for i in range(B)], want_index=True)
    mean = _seg_mean(d, off)
    c1, c2 = mean[:B].to(a.dtype), mean[B:].to(a.dtype)
    i12, i21 = idx[:B * n].long().reshape(B, n), idx[B * n:].long().reshape(B, m)
    res = (c1, c2, i12, i21) if give_id else c1 + c2
    if as_np:
        return tuple(r.cpu().numpy() for r in res) if give_id else res.cpu().numpy()
    return res
