"""Exact k-nearest neighbours on the device and a cleaning front end for real scans — host side of csrc/knn.hip.

The reference completes real scans: its Redwood / RealTest datasets (shapeformer/data/imnet_datasets/redwood.py, realtest.py) read raw
.pts clouds, and every point - flying pixels and stray clusters included - becomes an occupied cell of the encoder's grid.  The one
primitive a cleaning step needs is k-nearest neighbours (the reference has it on the host: geoutil.points_dist hands k to scipy's
cKDTree.query); here it is exact brute force on the device, the sibling of metrics.nn_dist, and on it sit

  knn_dev(p, q, k, p_off, q_off, exclude_self)            -> d2 (N,k) f32, idx (N,k) int32
  knn_mean_dist_dev(points, off, k)                       -> (N,) f64 mean distance to the k nearest other points
  statistical_outlier_mask_dev(points, off, k, std_ratio) -> keep (N,) uint8, count (B,) int32, stat (N,) f64   (PCL's rule)
  radius_outlier_mask_dev(points, off, radius, min_neighbors) -> keep, count
  estimate_normals_dev(points, off, k, viewpoint)         -> normal (N,3) f32, variation (N,) f32               (local PCA)
  normalize_scan(points, mode, scale)                     -> the four normalisations of the reference's real-scan datasets (host or device)
  clean_cloud_dev(X, k, std_ratio, out_N, seed)           -> (B, out_N, 3) cleaned clouds of a fixed size, count (B,)

Ragged batches and their argument checks are _ragged.py's: every refusal is an SfmiError raised on the host before
the library is loaded, and where the tensors live is checked last.  There is no CPU fallback.

Ordering contract of knn_dev: each row ascends in (d2, index) lexicographic order, d2 the f32 direct form of nn_dist (column 0 with
exclude_self=False IS nn_dist, bit for bit), so among equal f32 distances the lower index comes first.  Results are bit-identical
from run to run and do not depend on how the library cuts the work.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L
from ._ragged import excl_at, host_offsets, on_device, point_sets, points_arg

MAX_K = 64


def _check_k(k, what):
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= MAX_K:
        raise L.SfmiError(f"{what}: k must be an integer in [1, {MAX_K}], got {k!r}")
    return int(k)


def _launch_knn(pf, qf, po, qo, k, exclude_self):
    """pf (N,3), qf (M,3) f32 contiguous on one device, po / qo validated host offsets -> d2 (N,k) f32, idx (N,k) int32."""
    dev = pf.device
    B, N, M = len(po) - 1, pf.shape[0], qf.shape[0]
    lib = L.lib()
    d2 = torch.empty(N, k, device=dev, dtype=torch.float32)
    idx = torch.empty(N, k, device=dev, dtype=torch.int32)
    if N == 0:
        return d2, idx
    pod, qod = torch.from_numpy(po).to(dev), torch.from_numpy(qo).to(dev)
    ws = torch.empty(max(int(lib.sfmi_knn_workspace_bytes(B, N, M, k)), 1), device=dev, dtype=torch.uint8)
    L.check(lib.sfmi_knn_f32(L.ptr(pf), L.ptr(qf), L.ptr(pod), L.ptr(qod), B, N, M, k, int(bool(exclude_self)), L.ptr(d2), L.ptr(idx),
                             L.ptr(ws), L.stream_ptr()), "sfmi_knn_f32")
    return d2, idx


def knn_dev(p, q, k, p_off=None, q_off=None, exclude_self=False):
    """The k nearest points of q to every point of p, set by set, exact.

    p (N,3) / q (M,3) f32 HIP tensors with (B+1,) exclusive offsets p_off / q_off (None: one set), or p (B,N,3) / q (B,M,3) batches
    (set b of p against set b of q; offsets must then be None).  -> d2 (N,k) f32 squared distances and idx (N,k) int32 indices local
    to the set of q ((B,N,k) for batches).  Each row ascends in (d2, index); among equal f32 distances the lower index comes first.
    A set of q offering fewer than k candidates fills the tail of its rows with d2 = +inf, idx = -1.  1 <= k <= 64.
    exclude_self: p and q must be the same sets (equal offsets and sizes; pass the same tensor); the candidate with the query's own
    index is skipped - by index, not by distance, so duplicates of a point remain its neighbours.
    A set of q that is empty while its set of p is not raises SfmiError.  Bit-identical from run to run; with exclude_self=False
    column 0 equals metrics.nn_dist(..., return_index=True) bit for bit."""
    k = _check_k(k, "knn_dev")
    p, q = points_arg(p, "knn_dev p"), points_arg(q, "knn_dev q")
    batched = p.dim() == 3
    if batched:
        if q.dim() != 3 or q.shape[0] != p.shape[0] or p_off is not None or q_off is not None:
            raise L.SfmiError("knn_dev: batched (B,N,3) inputs need a (B,M,3) q of the same B and no offsets")
        B, n, m = p.shape[0], p.shape[1], q.shape[1]
        po, qo = np.arange(B + 1, dtype=np.int64) * n, np.arange(B + 1, dtype=np.int64) * m
    else:
        if q.dim() != 2:
            raise L.SfmiError("knn_dev: (N,3) p needs an (M,3) q")
        po, qo = host_offsets(p_off, p.shape[0], "knn_dev p_off"), host_offsets(q_off, q.shape[0], "knn_dev q_off")
        if len(po) != len(qo):
            raise L.SfmiError(f"knn_dev: p has {len(po) - 1} sets, q has {len(qo) - 1}")
    if exclude_self and not np.array_equal(po, qo):
        raise L.SfmiError("knn_dev: exclude_self needs p and q to be the same sets (equal sizes and offsets)")
    if ((np.diff(qo) == 0) & (np.diff(po) > 0)).any():
        raise L.SfmiError("knn_dev: a reference set is empty while its query set is not")
    if (np.diff(qo) >= 2 ** 31).any():
        raise L.SfmiError("knn_dev: a reference set has 2^31 points or more")
    on_device("knn_dev", p, q)
    pf, qf = p.reshape(-1, 3).float().contiguous(), q.reshape(-1, 3).float().contiguous()
    d2, idx = _launch_knn(pf, qf, po, qo, k, exclude_self)
    if batched:
        d2, idx = d2.reshape(p.shape[0], p.shape[1], k), idx.reshape(p.shape[0], p.shape[1], k)
    return d2, idx


def _self_knn(points, off, k, what, exclude_self=True):
    """points / off as point_sets takes them -> (flat f32 points, host offsets, batch shape or None, d2 (N,k), idx (N,k))."""
    k = _check_k(k, what)
    x, o, shape = point_sets(points, off, what)
    on_device(what, x)
    xf = x.float().contiguous()
    d2, idx = _launch_knn(xf, xf, o, o, k, exclude_self)
    return xf, o, shape, d2, idx


def _mean_dist(d2):
    N, k = d2.shape
    out = torch.empty(N, device=d2.device, dtype=torch.float64)
    L.check(L.lib().sfmi_knn_mean_dist_f64(L.ptr(d2), N, k, L.ptr(out), L.stream_ptr()), "sfmi_knn_mean_dist_f64")
    return out


def knn_mean_dist_dev(points, off, k):
    """(N,) f64 (or (B,N)): the mean Euclidean distance from each point to the k nearest OTHER points of its set (exclude_self), the
    mean of sqrt(d2) taken in f64 in column order by the library.  A set with fewer than k + 1 points gives +inf."""
    _, _, shape, d2, _ = _self_knn(points, off, k, "knn_mean_dist_dev")
    m = _mean_dist(d2)
    return m.reshape(shape) if shape else m


def _counts(keep, o):
    """per-set sums of a (N,) uint8 mask -> (B,) int32 on the device"""
    z = excl_at(torch.cumsum(keep, 0, dtype=torch.int32), torch.from_numpy(o).to(keep.device))
    return (z[1:] - z[:-1]).to(torch.int32)


def statistical_outlier_mask_dev(points, off=None, k=16, std_ratio=2.0):
    """PCL's StatisticalOutlierRemoval: with m_i = knn_mean_dist (k nearest other points) and, per set, mu = mean(m), sigma = std(m)
    with n - 1 in the denominator, both in f64: keep_i = m_i <= mu + std_ratio * sigma.  A set with fewer than k + 1 points keeps
    everything (its statistic is +inf).  -> keep (N,) uint8, count (B,) int32 kept points per set, stat (N,) f64 = m (all on the
    device; (B,N) shapes for a (B,N,3) batch)."""
    _, o, shape, d2, _ = _self_knn(points, off, k, "statistical_outlier_mask_dev")
    k = d2.shape[1]
    m = _mean_dist(d2)
    n = np.diff(o)
    parts = []                           # set by set, so that a set's mask does not depend on the batch around it
    for b in range(len(o) - 1):
        v = m[int(o[b]):int(o[b + 1])]
        parts.append(torch.ones_like(v, dtype=torch.bool) if n[b] < k + 1 else v <= v.mean() + float(std_ratio) * v.std(unbiased=True))
    keep = torch.cat(parts).to(torch.uint8)
    count = _counts(keep, o)
    return (keep.reshape(shape), count, m.reshape(shape)) if shape else (keep, count, m)


def radius_outlier_mask_dev(points, off, radius, min_neighbors):
    """Radius outlier removal: a point is kept when at least min_neighbors (<= 64) OTHER points of its set lie within `radius`, i.e.
    d2[:, min_neighbors - 1] <= radius^2 with the square rounded to f32 and the compare in f32.  -> keep (N,) uint8, count (B,) int32."""
    if not float(radius) >= 0:
        raise L.SfmiError(f"radius_outlier_mask_dev: radius must be >= 0, got {radius!r}")
    _, o, shape, d2, _ = _self_knn(points, off, min_neighbors, "radius_outlier_mask_dev")
    keep = (d2[:, -1] <= float(np.float32(float(radius) ** 2))).to(torch.uint8)
    count = _counts(keep, o)
    return (keep.reshape(shape) if shape else keep), count


def estimate_normals_dev(points, off=None, k=16, viewpoint=None):
    """Point normals by local PCA over the k nearest neighbours, the point itself included (as Open3D and PCL do): the eigenvector
    of the smallest eigenvalue of the neighbourhood's 3x3 covariance, everything in f64 on the device.
    -> normal (N,3) f32 unit vectors, variation (N,) f32 = l0 / (l0 + l1 + l2) (surface variation, 0 on a plane).
    viewpoint: (B,3) (or (3,) for one set) positions, used in f64: the sign is chosen so that n . (viewpoint - p) >= 0.  None: the
    component of largest magnitude is positive (the first such component on a tie).  A point with fewer than 3 neighbours (a set of
    fewer than 3 points) gets normal (0,0,0) and variation NaN."""
    k = _check_k(k, "estimate_normals_dev")
    x, o, shape = point_sets(points, off, "estimate_normals_dev")
    B = len(o) - 1
    view = None
    if viewpoint is not None:
        view = viewpoint.detach().cpu().numpy() if isinstance(viewpoint, torch.Tensor) else np.asarray(viewpoint)
        view = np.asarray(view, np.float64)
        if view.shape == (3,) and B == 1:
            view = view[None]
        if view.shape != (B, 3):
            raise L.SfmiError(f"estimate_normals_dev: expected ({B},3) viewpoints, got {tuple(view.shape)}")
        view = np.ascontiguousarray(view)
    dev = on_device("estimate_normals_dev", x)
    xf = x.float().contiguous()
    N = xf.shape[0]
    _, idx = _launch_knn(xf, xf, o, o, k, False)
    normal = torch.empty(N, 3, device=dev, dtype=torch.float32)
    variation = torch.empty(N, device=dev, dtype=torch.float32)
    od = torch.from_numpy(o).to(dev)
    vd = torch.from_numpy(view).to(dev) if view is not None else None
    L.check(L.lib().sfmi_knn_normals_f32(L.ptr(xf), L.ptr(od), L.ptr(idx), B, N, k, L.ptr(vd), L.ptr(normal), L.ptr(variation),
                                         L.stream_ptr()), "sfmi_knn_normals_f32")
    return (normal.reshape(*shape, 3), variation.reshape(shape)) if shape else (normal, variation)


# ---- the reference's real-scan normalisations (host or device: plain array arithmetic) ---------------------------------------------

NORMALIZE_MODES = ("mean_max", "bbox")


def normalize_scan(points, mode="mean_max", scale=0.7):
    """The normalisations of the reference's real-scan datasets, operation for operation in f32; numpy in -> numpy out, torch in ->
    torch out (on the tensor's device).  points (N,>=3): the first three columns are used.
      "mean_max": subtract the per-axis mean, divide by the global maximum coordinate points.max() (NOT the maximum magnitude: the
                  reference's `points /= points.max()`), multiply by scale.  redwood.py:53-58 Redwood (0.7), realtest.py:55-62
                  RealTest_dataset (0.8).
      "bbox":     subtract the bounding-box centre (max + min) / 2, divide by abs(points).max(), multiply by scale.  redwood.py:99-102
                  Redwood2 (0.9), realtest.py:105-109 RealTest2_dataset (0.85)."""
    if mode not in NORMALIZE_MODES:
        raise L.SfmiError(f"normalize_scan: mode must be one of {NORMALIZE_MODES}, got {mode!r}")
    if isinstance(points, torch.Tensor):
        p = points[:, :3].to(torch.float32).clone()
        if mode == "mean_max":
            p -= p.mean(0, keepdim=True)
            p /= p.max()
        else:
            p -= (p.max(0).values + p.min(0).values) / 2
            p /= p.abs().max()
        return p * float(scale)
    p = np.array(np.asarray(points)[:, :3], dtype=np.float32)
    if mode == "mean_max":
        p[:, 0] -= np.mean(p[:, 0])
        p[:, 1] -= np.mean(p[:, 1])
        p[:, 2] -= np.mean(p[:, 2])
        p /= p.max()
    else:
        p -= (p.max(axis=0) + p.min(axis=0)) / 2
        p /= np.abs(p).max()
    return p * np.float32(scale)


# ---- the cleaning front end --------------------------------------------------------------------------------------------------------

def clean_cloud_dev(X, k=16, std_ratio=2.0, out_N=None, seed=0):
    """Statistical outlier removal of a batch of clouds, back at a fixed size: X (B,N,3) HIP tensor -> (B, out_N or N, 3) f32, each row
    a uniformly drawn kept point of its cloud (hpr.resample_visible_dev with the mask as `visible`: a counter hash of (seed, cloud
    index, row), no global RNG), and count (B,) int32 kept points per cloud.  That function's fallback applies: a cloud with two or
    fewer kept points is resampled from all its points."""
    from .hpr import resample_visible_dev
    x = points_arg(X, "clean_cloud_dev")
    if x.dim() != 3:
        raise L.SfmiError(f"clean_cloud_dev: expected (B,N,3) points, got {tuple(x.shape)}")
    n_out = x.shape[1] if out_N is None else int(out_N)
    if n_out < 0:
        raise L.SfmiError("clean_cloud_dev: out_N must be >= 0")
    keep, count, _ = statistical_outlier_mask_dev(x, None, k, std_ratio)
    B, n = x.shape[:2]
    xf, o = x.reshape(B * n, 3).float().contiguous(), np.arange(B + 1, dtype=np.int64) * n
    return resample_visible_dev(xf, o, keep.reshape(-1), count, n_out, 0., seed), count
