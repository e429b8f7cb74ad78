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
Ragged sets are (points (N,3), offsets (B+1,)) pairs or lists of (n_i,3) tensors; reductions over them are per-set torch sums on
the device (fixed order: deterministic).  The offset convention and the argument checks are _ragged.py's.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L
from ._ragged import f32_dev, host_offsets, offsets_dev, on_device, pair_sets, points_arg


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
    ws = torch.empty(max(int(lib.sfmi_nn_dist_workspace_bytes(B, N, M)), 1), device=dev, dtype=torch.uint8)
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


def evaluate(Xct, completions, Xbd=None, tau=0.01):
    """Metrics of the completions of ONE partial cloud: {"k", "uhd", "uhd_per", "tmd" (k >= 2)} and, with the full shape Xbd,
    {"cd", "cd_per", "fscore", "fscore_per", "tau"} (CD / F-score of each completion against Xbd; *_per in completion order,
    the plain key is their mean).  Definitions in the module docstring.  numpy inputs are moved to the completions' device."""
    if isinstance(completions, torch.Tensor):
        dev = completions.device
    else:
        dev = completions[0].device if len(completions) and isinstance(completions[0], torch.Tensor) else torch.device("cuda")
        completions = [f32_dev(c, dev) for c in completions]
    Xct = f32_dev(Xct, dev).reshape(-1, 3)
    cf, co = _pack(completions, "evaluate completions")
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
    ws = torch.empty(int(lib.sfmi_mesh_sample_workspace_bytes(B, T)), device=dev, dtype=torch.uint8)
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
    with give_id.  torch in -> torch out on the input's device (f32 means, int64 indices); numpy in -> numpy out.
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
