"""Exact k-nearest neighbours on the device and a cleaning front end for real scans — host side of csrc/knn.hip.

The reference completes real scans: its Redwood / RealTest datasets (shapeformer/data/imnet_datasets/redwood.py, realtest.py) read raw
.pts clouds, and every point - flying pixels and stray clusters included - becomes an occupied cell of the encoder's grid.  The one
primitive a cleaning step needs is k-nearest neighbours (the reference has it on the host: geoutil.points_dist hands k to scipy's
cKDTree.query); here it is exact brute force on the device, the sibling of metrics.nn_dist, and on it sit

  knn_dev(p, q, k, p_off, q_off, exclude_self)            -> d2 (N,k) f32, idx (N,k) int32
  knn_mean_dist_dev(points, off, k)                       -> (N,) f64 mean distance to the k nearest other points
  statistical_outlier_mask_dev(points, off, k, std_ratio) -> keep (N,) uint8, count (B,) int32, stat (N,) f64   (PCL's rule)
  radius_outlier_mask_dev(points, off, radius, min_neighbors) -> keep, count
  estimate_normals_dev(points, off, k, viewpoint, orient) -> normal (N,3) f32, variation (N,) f32               (local PCA)
  orient_normals_dev(points, normals, off, k, idx, anchor, viewpoint, details) -> normals of consistent sign (csrc/tangent.hip, §5.21)
  normalize_scan(points, mode, scale)                     -> the four normalisations of the reference's real-scan datasets (host or device)
  farthest_point_sample_dev(points, off, n, start, valid) -> idx (B,n) int32, d2 (B,n) f32, count (B,), status (B,)   (csrc/downsample.hip,
  voxel_downsample_dev(points, off, voxel, pick)          -> out (M,3) f32, out_off (B+1,) host, first (M,), count (M,)       DESIGN.md §5.15)
  plane_hypotheses(sizes, H, seed)                        -> (B,H,3) int32 RANSAC draws on the host                   (csrc/segment.hip,
  segment_plane_dev(points, off, threshold, hypotheses, ...) -> plane (B,4) f64, inlier (N,), n_in, count (B,H), best, status  DESIGN.md §5.17)
  refit_plane_dev(points, off, plane, threshold, up)      -> plane (B,4) f64, inlier (N,), n_in: the refit seeded by any plane
  remove_planes_dev(points, off, threshold, max_planes, min_ratio, ...) -> keep (N,) uint8, planes (B,max_planes,4), taken (B,)
  euclidean_clusters_dev(points, off, radius, min_points) -> label (N,) int32, sizes, c_off (B+1,) host
  largest_cluster_mask_dev(points, off, radius, min_points) -> keep (N,) uint8, count (B,)
  upright_rotation(normal, up)                            -> (B,3,3) f64 (host or device)
  isolate_object_dev(points, off, plane_threshold, cluster_radius, ...) -> kept points, offsets, mask, planes, rotation
  clean_cloud_dev(X, k, std_ratio, out_N, seed, voxel, resample, remove_planes, keep_cluster) -> (B, out_N, 3) cleaned clouds, count (B,)

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
from . import _ragged
from ._ragged import (check_count, check_nonneg, check_number, excl_at, offsets_dev, on_device, pair_sets, point_sets, points_arg,
                      run_starts, set_ids, sorted_runs)

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
    pod, qod = offsets_dev(po, dev), offsets_dev(qo, dev)
    ws = _ragged.workspace(lib.sfmi_knn_workspace_bytes(B, N, M, k), dev)
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
    p, q, po, qo, shape = pair_sets(p, q, p_off, q_off, "knn_dev", ("p", "q"), None)
    if exclude_self and not np.array_equal(po, qo):
        raise L.SfmiError("knn_dev: exclude_self needs p and q to be the same sets (equal sizes and offsets)")
    if ((np.diff(qo) == 0) & (np.diff(po) > 0)).any():
        raise L.SfmiError("knn_dev: a reference set is empty while its query set is not")
    if (np.diff(qo) >= 2 ** 31).any():
        raise L.SfmiError("knn_dev: a reference set has 2^31 points or more")
    on_device("knn_dev", p, q)
    d2, idx = _launch_knn(p.float().contiguous(), q.float().contiguous(), po, qo, k, exclude_self)
    return (d2.reshape(*shape, k), idx.reshape(*shape, k)) if shape else (d2, idx)


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
    z = excl_at(torch.cumsum(keep, 0, dtype=torch.int32), offsets_dev(o, keep.device))
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


def estimate_normals_dev(points, off=None, k=16, viewpoint=None, orient=None):
    """Point normals by local PCA over the k nearest neighbours, the point itself included (as Open3D and PCL do): the eigenvector
    of the smallest eigenvalue of the neighbourhood's 3x3 covariance, everything in f64 on the device.
    -> normal (N,3) f32 unit vectors, variation (N,) f32 = l0 / (l0 + l1 + l2) (surface variation, 0 on a plane).
    viewpoint: (B,3) (or (3,) for one set) positions, used in f64: the sign is chosen so that n . (viewpoint - p) >= 0.  None: the
    component of largest magnitude is positive (the first such component on a tie).  A point with fewer than 3 neighbours (a set of
    fewer than 3 points) gets normal (0,0,0) and variation NaN.
    orient="tangent": the signs are then made consistent by orient_normals_dev on the same neighbour table, with anchor "viewpoint"
    when a viewpoint is given and "outward" otherwise.  None: the signs above, as ever."""
    k = _check_k(k, "estimate_normals_dev")
    if orient not in ORIENT_MODES:
        raise L.SfmiError(f"estimate_normals_dev: orient must be one of {ORIENT_MODES}, got {orient!r}")
    x, o, shape = point_sets(points, off, "estimate_normals_dev")
    B = len(o) - 1
    view = None
    if viewpoint is not None:
        view = _viewpoints(viewpoint, B, "estimate_normals_dev")
    dev = on_device("estimate_normals_dev", x)
    xf = x.float().contiguous()
    N = xf.shape[0]
    _, idx = _launch_knn(xf, xf, o, o, k, False)
    normal = torch.empty(N, 3, device=dev, dtype=torch.float32)
    variation = torch.empty(N, device=dev, dtype=torch.float32)
    od = offsets_dev(o, dev)
    vd = torch.from_numpy(view).to(dev) if view is not None else None
    L.check(L.lib().sfmi_knn_normals_f32(L.ptr(xf), L.ptr(od), L.ptr(idx), B, N, k, L.ptr(vd), L.ptr(normal), L.ptr(variation),
                                         L.stream_ptr()), "sfmi_knn_normals_f32")
    if orient == "tangent":
        normal = _orient_launch("estimate_normals_dev", xf, normal, o, idx, vd)["normal"]
    return (normal.reshape(*shape, 3), variation.reshape(shape)) if shape else (normal, variation)


# ---- consistent orientation without a viewpoint: the kNN graph's minimum spanning forest (csrc/tangent.hip) ---------

ORIENT_MODES = (None, "tangent")
ANCHORS = ("outward", "viewpoint")


def _viewpoints(viewpoint, B, what):
    view = viewpoint.detach().cpu().numpy() if isinstance(viewpoint, torch.Tensor) else np.asarray(viewpoint)
    view = np.asarray(view, np.float64)
    if view.shape == (3,) and B == 1:
        view = view[None]
    if view.shape != (B, 3):
        raise L.SfmiError(f"{what}: expected ({B},3) viewpoints, got {tuple(view.shape)}")
    return np.ascontiguousarray(view)


def _orient_launch(what, xf, nf, o, idx, vd):
    """xf, nf (N,3) f32 contiguous, idx (N,k) int32 contiguous on one device, o validated host offsets, vd (B,3) f64 device viewpoints
    or None (outward) -> dict of device tensors.  Reads the (B,) status back: one synchronisation."""
    dev = xf.device
    B, N, k = len(o) - 1, xf.shape[0], idx.shape[1]
    out = torch.empty_like(nf)
    component = torch.empty(N, device=dev, dtype=torch.int32)
    tree = torch.empty(N, 2, device=dev, dtype=torch.int32)
    parity = torch.empty(N, device=dev, dtype=torch.uint8)
    votes = torch.zeros(N, 2, device=dev, dtype=torch.int32)
    rounds = torch.zeros(B, device=dev, dtype=torch.int32)
    if N and B:
        lib = L.lib()
        od = offsets_dev(o, dev)
        status = torch.empty(B, device=dev, dtype=torch.int32)
        ws = _ragged.workspace(lib.sfmi_tangent_workspace_bytes(B, N), dev)
        L.check(lib.sfmi_tangent_forest_f32(L.ptr(nf), L.ptr(od), L.ptr(idx), B, N, k, _max_n(o), L.ptr(component), L.ptr(tree),
                                            L.ptr(parity), L.ptr(rounds), L.ptr(status), L.ptr(ws), L.stream_ptr()),
                "sfmi_tangent_forest_f32")
        L.check(lib.sfmi_tangent_apply_f32(L.ptr(xf), L.ptr(nf), L.ptr(od), L.ptr(component), L.ptr(parity), L.ptr(vd), B, N,
                                           L.ptr(votes), L.ptr(out), L.ptr(ws), L.stream_ptr()), "sfmi_tangent_apply_f32")
        bad = np.nonzero(status.cpu().numpy())[0]                  # the one read-back
        if bad.size:
            raise L.SfmiError(f"{what}: the walk to a tree's root reached its step cap in set(s) {bad.tolist()} (a cycle in the forest)")
    return {"normal": out, "component": component, "tree": tree, "parity": parity, "votes": votes, "rounds": rounds}


def orient_normals_dev(points, normals, off=None, k=16, idx=None, anchor="outward", viewpoint=None, details=False):
    """A consistent orientation for normals of arbitrary sign, set by set, without a camera: Hoppe et al.'s tangent-plane propagation
    (Open3D orient_normals_consistent_tangent_plane), exact and deterministic.

    points / normals (N,3) f32 HIP tensors with (B+1,) offsets (None: one set), or (B,M,3) batches.  idx: the (N,k) ((B,M,k)) int32
    neighbour table, local to each set, used as it is; None: knn_dev over k neighbours with the point itself included, the table of
    estimate_normals_dev.  -> the normals, each the input or its exact negation; with details=True also a dict: component, parity,
    tree, votes, rounds (B,), n_components (B,), on the device.
    Graph: points i != j of a set are joined when j is in row i or i in row j; a point whose normal is not finite or is (0,0,0) is
    dead: it joins nothing and passes through.  Weight w = max(0, 1 - |n_i . n_j|) in f64, flip = n_i . n_j < 0.  The minimum spanning
    forest under the strict order (bits of w, lo, hi) is unique; parity is the XOR of flip along the tree path to the tree's
    lowest-index point (component); tree (N,2) holds the forest's edges as local (lo, hi) rows, (-1,-1) elsewhere.
    anchor fixes one sign per tree by an integer vote over its points with m = the normal after parity: votes (N,2) int32 at the row
    of the tree's component = (#{m . d > 0}, #{m . d < 0}); the tree is negated when the second count is larger.  "outward":
    d = p - the set's centroid (of the SET, not of the tree: the sum of registration's frame-covariant rule); "viewpoint": d = v - p
    with viewpoint (B,3) ((3,) for one set), in f64.
    Trees are the connected pieces of the kNN graph: pieces that k neighbours do not join are oriented independently, each by its own
    vote (raise k to join them).  Bit-identical from run to run; a set's results depend on that set alone.  The (B,) status is read
    back: one synchronisation."""
    what = "orient_normals_dev"
    if idx is None:
        k = _check_k(k, what)
    if anchor not in ANCHORS:
        raise L.SfmiError(f"{what}: anchor must be one of {ANCHORS}, got {anchor!r}")
    x, o, shape = point_sets(points, off, what)
    B = len(o) - 1
    if not isinstance(normals, torch.Tensor) or tuple(normals.shape) != tuple(points.shape):
        raise L.SfmiError(f"{what}: normals must be a tensor of the points' shape {tuple(points.shape)}, got "
                          f"{tuple(normals.shape) if isinstance(normals, torch.Tensor) else type(normals).__name__}")
    if idx is not None:
        if not isinstance(idx, torch.Tensor) or idx.dtype != torch.int32:
            raise L.SfmiError(f"{what}: idx must be an int32 torch tensor on the HIP device")
        if idx.dim() != points.dim() or tuple(idx.shape[:-1]) != tuple(points.shape[:-1]):
            raise L.SfmiError(f"{what}: idx must be {tuple(points.shape[:-1])} + (k,), got {tuple(idx.shape)}")
        k = _check_k(int(idx.shape[-1]), what)
    if x.shape[0] >= 2 ** 31 or B > 65535:
        raise L.SfmiError(f"{what}: at most 65535 sets and fewer than 2^31 points")
    view = None
    if anchor == "viewpoint":
        if viewpoint is None:
            raise L.SfmiError(f"{what}: anchor='viewpoint' needs ({B},3) viewpoints")
        view = _viewpoints(viewpoint, B, what)
    elif viewpoint is not None:
        raise L.SfmiError(f"{what}: a viewpoint goes with anchor='viewpoint', not with 'outward'")
    dev = on_device(what, x, normals, *([idx] if idx is not None else []))
    xf, nf = x.float().contiguous(), normals.reshape(-1, 3).float().contiguous()
    table = _launch_knn(xf, xf, o, o, k, False)[1] if idx is None else idx.reshape(-1, k).contiguous()
    r = _orient_launch(what, xf, nf, o, table, torch.from_numpy(view).to(dev) if view is not None else None)
    out = r.pop("normal")
    out = out.reshape(*shape, 3) if shape else out
    if not details:
        return out
    N = xf.shape[0]
    if N:
        local = torch.arange(N, device=dev) - offsets_dev(o, dev)[set_ids(o, dev)]
        r["n_components"] = _counts((r["component"].long() == local).to(torch.uint8), o)
    else:
        r["n_components"] = torch.zeros(B, device=dev, dtype=torch.int32)
    return out, r


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


# ---- downsampling: farthest point sampling and a voxel grid (csrc/downsample.hip) ----------------------------------

FPS_RESIDENT_MAX = 16384          # sfmi_fps_resident_max(): the largest set sampled from registers; larger sets stream from memory
VOXEL_MAX_CELLS, VOXEL_MAX_SETS = 65536, 32768
VOXEL_PICKS = ("centroid", "first")
RESAMPLE_MODES = ("random", "fps")


def _aligned16(t):
    return t if t.data_ptr() % 16 == 0 else t.clone()


def farthest_point_sample_dev(points, off=None, n=None, start=None, valid=None):
    """Farthest point sampling, set by set, exact.

    points (N,3) f32 HIP tensor with (B+1,) exclusive offsets (None: one set), or a (B,M,3) batch.  -> idx (B,n) int32 local to the set,
    d2 (B,n) f32, count (B,) int32, status (B,) int32, all on the device; the call does not synchronise.
    Candidates of set b are its points, or those with valid != 0 (valid: (N,) uint8 HIP tensor, (B,M) for a batch);
    count[b] = min(n, candidates).  The first pick is start (an int or (B,) ints, local indices; not together with valid), by default
    the candidate of lowest index.  Every candidate starts at dist = +inf; after each pick s the remaining candidates take
    dist = min(dist, |p - s|^2) in the f32 direct form of nn_dist (the same bits) and s leaves the candidates, so indices in a row are
    distinct; the next pick is arg max dist, the lower index among equal f32 values.  d2[b,t] is the winner's dist when it was picked:
    d2[b,0] = +inf, the row is non-increasing, sqrt(d2[b,t]) is the covering radius of the first t picks.  Columns t >= count[b] hold
    (-1, 0.0).  status: 0 ok, 1 no candidate, 2 a non-finite coordinate among the candidates (1, 2: the row is all tail).
    Bit-identical from run to run; a set's row depends on that set only; a run with smaller n is a prefix of a run with larger n."""
    what = "farthest_point_sample_dev"
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or int(n) < 0 or int(n) >= 2 ** 31:
        raise L.SfmiError(f"{what}: n must be an integer in [0, 2^31), got {n!r}")
    n = int(n)
    x, o, shape = point_sets(points, off, what)
    B, sizes = len(o) - 1, np.diff(o)
    if (sizes >= 2 ** 31).any():
        raise L.SfmiError(f"{what}: a set has 2^31 points or more")
    if start is not None and valid is not None:
        raise L.SfmiError(f"{what}: start together with valid is refused (the first pick of a masked set is its lowest candidate)")
    st = None
    if start is not None:
        s = start.detach().cpu().numpy() if isinstance(start, torch.Tensor) else np.asarray(start)
        if s.dtype == np.bool_ or not np.issubdtype(s.dtype, np.integer):
            raise L.SfmiError(f"{what}: start must be an integer or a ({B},) integer array")
        if s.ndim == 0:
            s = np.full(B, s)
        if s.shape != (B,):
            raise L.SfmiError(f"{what}: start must be an integer or a ({B},) integer array, got shape {tuple(s.shape)}")
        if ((s < 0) | (s >= sizes)).any():
            raise L.SfmiError(f"{what}: start out of range for its set")
        st = s.astype(np.int32)
    if valid is not None:
        if not isinstance(valid, torch.Tensor) or valid.dtype != torch.uint8:
            raise L.SfmiError(f"{what}: valid must be a uint8 torch tensor on the HIP device")
        if tuple(valid.shape) != (shape if shape else (x.shape[0],)):
            raise L.SfmiError(f"{what}: valid must have one entry per point, got shape {tuple(valid.shape)}")
    dev = on_device(what, x, *([valid] if valid is not None else []))
    N = x.shape[0]
    idx = torch.empty(B, n, device=dev, dtype=torch.int32)
    d2 = torch.empty(B, n, device=dev, dtype=torch.float32)
    count = torch.empty(B, device=dev, dtype=torch.int32)
    status = torch.empty(B, device=dev, dtype=torch.int32)
    if B == 0:
        return idx, d2, count, status
    lib = L.lib()
    xf = _aligned16(x.float().contiguous())
    vd = valid.reshape(-1).contiguous() if valid is not None else None
    od = offsets_dev(o, dev)
    sd = torch.from_numpy(st).to(dev) if st is not None else None
    ws = _ragged.workspace(lib.sfmi_fps_workspace_bytes(B, N, n), dev)
    L.check(lib.sfmi_fps_f32(L.ptr(xf), L.ptr(od), L.ptr(vd), L.ptr(sd), B, N, n, L.ptr(idx), L.ptr(d2), L.ptr(count), L.ptr(status),
                             L.ptr(ws), L.stream_ptr()), "sfmi_fps_f32")
    return idx, d2, count, status


def _check_voxel(voxel, what):
    return check_number(voxel, what, "voxel", 0, float("inf"), lo_open=True)


def voxel_downsample_dev(points, off=None, voxel=None, pick="centroid"):
    """Voxel-grid downsampling, set by set: one output point per occupied cell of edge `voxel`.

    points (N,3) f32 HIP tensor with (B+1,) offsets (None: one set), or a (B,M,3) batch.  -> out (M,3) f32, out_off (B+1,) host int64
    (the result is ragged: the voxel counts are read back, one synchronisation), first (M,) int32, count (M,) int32.
    Per set lo is the componentwise f32 minimum of its points and the cell of a point is floor((double(x) - double(lo)) / voxel) per
    axis (a point on a cell face belongs to the upper cell).  The voxels of a set ascend in (cz, cy, cx).  count: the points in the
    voxel; first: the lowest local index among them.  pick="first": that input point, bit for bit.  pick="centroid" (PCL VoxelGrid,
    Open3D voxel_down_sample): their mean, summed in f64 in a fixed order and rounded to f32: bit-identical from run to run and
    independent of the batch around the set.  An empty set yields no voxels.
    Raises SfmiError after the read-back for a non-finite coordinate or a grid of 65 536 cells or more along an axis; a batch holds
    fewer than 32 768 sets."""
    what = "voxel_downsample_dev"
    voxel = _check_voxel(voxel, what)
    if pick not in VOXEL_PICKS:
        raise L.SfmiError(f"{what}: pick must be one of {VOXEL_PICKS}, got {pick!r}")
    x, o, _ = point_sets(points, off, what)
    B, N = len(o) - 1, x.shape[0]
    if B >= VOXEL_MAX_SETS:
        raise L.SfmiError(f"{what}: a batch holds fewer than {VOXEL_MAX_SETS} sets, got {B}")
    if N >= 2 ** 31:
        raise L.SfmiError(f"{what}: the batch has 2^31 points or more")
    dev = on_device(what, x)
    if N == 0:
        return (torch.empty(0, 3, device=dev, dtype=torch.float32), np.zeros(B + 1, np.int64),
                torch.empty(0, device=dev, dtype=torch.int32), torch.empty(0, device=dev, dtype=torch.int32))
    lib = L.lib()
    xf = x.float().contiguous()
    od = offsets_dev(o, dev)
    lo = torch.empty(B, 3, device=dev, dtype=torch.int32)
    keys = torch.empty(N, device=dev, dtype=torch.int64)
    status = torch.empty(1, device=dev, dtype=torch.int32)
    L.check(lib.sfmi_voxel_keys_f32(L.ptr(xf), L.ptr(od), B, N, voxel, L.ptr(lo), L.ptr(keys), L.ptr(status), L.stream_ptr()),
            "sfmi_voxel_keys_f32")
    order, is_start, rank = sorted_runs(keys)
    head = torch.cat([excl_at(rank, od), status.to(rank.dtype)]).cpu().numpy()          # the one read-back: voxels per set, status
    if head[-1]:
        raise L.SfmiError(f"{what}: " + ("a coordinate is not finite" if head[-1] & 1 else
                                         f"the grid has {VOXEL_MAX_CELLS} cells or more along an axis (voxel = {voxel!r})"))
    out_off = head[:-1].astype(np.int64)
    M = int(out_off[-1])
    starts = run_starts(is_start, rank, M)
    out = torch.empty(M, 3, device=dev, dtype=torch.float32)
    first = torch.empty(M, device=dev, dtype=torch.int32)
    count = torch.empty(M, device=dev, dtype=torch.int32)
    L.check(lib.sfmi_voxel_reduce_f32(L.ptr(xf), L.ptr(od), L.ptr(order), L.ptr(starts), B, N, M, int(pick == "centroid"), L.ptr(out),
                                      L.ptr(first), L.ptr(count), L.stream_ptr()), "sfmi_voxel_reduce_f32")
    return out, out_off, first, count


# ---- plane removal and Euclidean clustering (csrc/segment.hip) -----------------------------------------------------

def _mix64(x):
    """sfmi_mix64 of csrc/sfmi_ragged.h on a numpy uint64 array (wrapping arithmetic)"""
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def plane_hypotheses(sizes, H, seed=0):
    """The RANSAC draws of segment_plane_dev: (B,H,3) int32 on the host, index = sfmi_mix64((seed << 40) + 4 h + slot) mod n_b (uint64
    arithmetic): a function of (seed, h, slot, n) and not of b, so a batch draws what per-set calls draw.  Repeated indices are not
    redrawn: the kernel marks such a hypothesis invalid.  A set of no points gets index 0, which lies outside it."""
    H = check_count(H, "plane_hypotheses", "H")
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 2 ** 23:
        raise L.SfmiError(f"plane_hypotheses: seed must be an integer in [0, 2^23), got {seed!r}")
    n = np.asarray(sizes, np.int64).reshape(-1)
    if (n < 0).any():
        raise L.SfmiError("plane_hypotheses: sizes must be >= 0")
    ctr = np.uint64(int(seed) << 40) + np.uint64(4) * np.arange(H, dtype=np.uint64)[:, None] + np.arange(3, dtype=np.uint64)[None, :]
    r = _mix64(ctr)
    return (r[None] % np.maximum(n, 1).astype(np.uint64)[:, None, None]).astype(np.int32)


def _max_n(o):
    return int(np.diff(o).max()) if len(o) > 1 else 0


def _up_arg(up, B, what):
    if up is None:
        return None
    u = up.detach().cpu().numpy() if isinstance(up, torch.Tensor) else np.asarray(up)
    u = np.asarray(u, np.float64)
    if u.shape == (3,):
        u = np.broadcast_to(u, (B, 3))
    if u.shape != (B, 3) or not np.isfinite(u).all():
        raise L.SfmiError(f"{what}: up must be finite, (3,) or ({B},3), got shape {tuple(u.shape)}")
    return np.array(u, np.float64, order="C")          # a copy: broadcast_to gives a read-only view


def _triple_plane(xf, od, tr, best, upd):
    """refit=False: the plane of the winning triple, unit normal, in f64 by elementwise torch arithmetic (one rounding per operation)"""
    B = best.shape[0]
    nan = torch.full((B, 4), float("nan"), device=xf.device, dtype=torch.float64)
    if xf.shape[0] == 0:
        return nan
    t = tr[torch.arange(B, device=xf.device), best.clamp(min=0).long()].long() + od[:-1, None]
    p = xf[t.clamp(0, xf.shape[0] - 1)].double()                                          # (B,3,3): a set without a winner reads any row
    u, v, p0 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0], p[:, 0]
    n = torch.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], 1)
    n = n / torch.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])[:, None]
    if upd is not None:
        flip = ((n[:, 0] * upd[:, 0] + n[:, 1] * upd[:, 1]) + n[:, 2] * upd[:, 2]) < 0
    else:
        flip = n.gather(1, n.abs().argmax(1, keepdim=True))[:, 0] < 0
    n = torch.where(flip[:, None], -n, n)
    dd = -((n[:, 0] * p0[:, 0] + n[:, 1] * p0[:, 1]) + n[:, 2] * p0[:, 2])
    return torch.where((best >= 0)[:, None], torch.cat([n, dd[:, None]], 1), nan)


def segment_plane_dev(points, off=None, threshold=0.01, hypotheses=1024, seed=0, triples=None, up=None, refit=True):
    """The dominant plane of every set by RANSAC (PCL SACSegmentation, Open3D segment_plane), exact and deterministic.

    points (N,3) f32 HIP tensor with (B+1,) offsets (None: one set), or a (B,M,3) batch.  -> plane (B,4) f64 (nx, ny, nz, dd) with
    n.x + dd = 0 and |n| = 1, inlier (N,) uint8 ((B,M) for a batch), n_in (B,) int32, count (B,H) int32, best (B,) int32, status (B,)
    int32, all on the device; the call does not synchronise.
    Hypotheses are point triples: plane_hypotheses(sizes, hypotheses, seed), or `triples` (B,H,3) integers local to each set.  Scoring,
    in f64 with every product and sum rounded on its own: n = (p1 - p0) x (p2 - p0), nn = (nx nx + ny ny) + nz nz, d = (nx p0x + ny p0y)
    + nz p0z; x is an inlier iff s s <= threshold^2 nn with s = ((nx x + ny y) + nz z) - d.  count[b,h] = the inliers of hypothesis h over
    the set, -1 for an invalid one (an index repeats or lies outside the set, or nn > 0 is false: collinear points); best[b] = the valid
    hypothesis of largest count, the lowest h among equal counts, -1 without one; status: 0 ok, 1 no valid hypothesis (a set of fewer
    than 3 points has none), 2 a non-finite coordinate in the set (its row of count is all -1).
    refit=True (Open3D's last step): the least-squares plane of the winner's inliers - centroid and covariance in f64 summed in a fixed
    order, the eigenvector of the smallest eigenvalue, dd = -n.c - and inlier = fabs(n.x + dd) <= threshold in f64.  refit=False: the
    winner's own plane, normalised in f64, and its inliers by the scoring rule.  Sign: n.up >= 0 with up ((3,) or (B,3)), else the
    component of largest magnitude is positive.  A set without a winner, or whose winner has fewer than 3 inliers: plane NaN, mask 0,
    n_in 0.  Bit-identical from run to run; a set's results depend on that set alone."""
    what = "segment_plane_dev"
    thr = check_nonneg(threshold, what, "threshold")
    x, o, shape = point_sets(points, off, what)
    B, N = len(o) - 1, x.shape[0]
    if B > 65535 or (np.diff(o) >= 2 ** 31).any():
        raise L.SfmiError(f"{what}: at most 65535 sets, each below 2^31 points")
    if triples is None:
        tr = plane_hypotheses(np.diff(o), check_count(hypotheses, what, "hypotheses"), seed)
    else:
        tr = triples
        if not isinstance(tr, torch.Tensor):
            tr = np.asarray(tr)
            if tr.dtype == np.bool_ or not np.issubdtype(tr.dtype, np.integer):
                raise L.SfmiError(f"{what}: triples must be integers")
        elif tr.dtype.is_floating_point or tr.dtype == torch.bool:
            raise L.SfmiError(f"{what}: triples must be integers")
        if tr.ndim != 3 or tr.shape[0] != B or tr.shape[1] < 1 or tr.shape[2] != 3:
            raise L.SfmiError(f"{what}: triples must be ({B},H,3) with H >= 1, got {tuple(tr.shape)}")
    H = int(tr.shape[1])
    upa = _up_arg(up, B, what)
    dev = on_device(what, x, *([tr] if isinstance(tr, torch.Tensor) else []))
    xf = x.float().contiguous()
    trd = (tr if isinstance(tr, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(tr)).to(dev)).to(torch.int32).contiguous()
    od = offsets_dev(o, dev)
    upd = torch.from_numpy(upa).to(dev) if upa is not None else None
    count = torch.empty(B, H, device=dev, dtype=torch.int32)
    best = torch.empty(B, device=dev, dtype=torch.int32)
    status = torch.empty(B, device=dev, dtype=torch.int32)
    plane = torch.empty(B, 4, device=dev, dtype=torch.float64)
    inlier = torch.empty(N, device=dev, dtype=torch.uint8)
    n_in = torch.empty(B, device=dev, dtype=torch.int32)
    lib = L.lib()
    L.check(lib.sfmi_plane_score_f32(L.ptr(xf), L.ptr(od), L.ptr(trd), B, N, H, _max_n(o), thr * thr, L.ptr(count), L.ptr(best),
                                     L.ptr(status), L.stream_ptr()), "sfmi_plane_score_f32")
    L.check(lib.sfmi_plane_refit_f32(L.ptr(xf), L.ptr(od), L.ptr(trd), L.ptr(best), L.ptr(status), None, L.ptr(upd), B, N, H, thr,
                                     int(bool(refit)), L.ptr(plane), L.ptr(inlier), L.ptr(n_in), L.stream_ptr()), "sfmi_plane_refit_f32")
    if not refit:
        plane = _triple_plane(xf, od, trd, best, upd)
    return plane, (inlier.reshape(shape) if shape else inlier), n_in, count, best, status


def refit_plane_dev(points, off=None, plane=None, threshold=0.01, up=None):
    """The least-squares plane of a given plane's inliers, segment_plane_dev's refit seeded by any plane: plane (B,4) (or (4,) for one
    set) f64 (n, dd), n of any length > 0.  Its inliers are the points with s s <= threshold^2 nn, s = ((nx x + ny y) + nz z) + dd,
    nn = (nx nx + ny ny) + nz nz, in f64; centroid, covariance, eigenvector, sign and final mask as in segment_plane_dev.
    -> plane (B,4) f64, inlier (N,) uint8 ((B,M) for a batch), n_in (B,) int32.  A seed that is not finite or has n = 0, or fewer than
    3 seed inliers: plane NaN, mask 0, n_in 0.  Calling it on its own output iterates the fit."""
    what = "refit_plane_dev"
    thr = check_nonneg(threshold, what, "threshold")
    x, o, shape = point_sets(points, off, what)
    B, N = len(o) - 1, x.shape[0]
    if isinstance(plane, torch.Tensor):
        seed = plane.detach().to(torch.float64)
    else:
        seed = torch.from_numpy(np.array(plane, np.float64)) if plane is not None else None
    if seed is not None and tuple(seed.shape) == (4,) and B == 1:
        seed = seed[None]
    if seed is None or tuple(seed.shape) != (B, 4):
        raise L.SfmiError(f"{what}: plane must be ({B},4), got {None if seed is None else tuple(seed.shape)}")
    upa = _up_arg(up, B, what)
    dev = on_device(what, x)
    xf, seed = x.float().contiguous(), seed.to(dev).contiguous()
    od = offsets_dev(o, dev)
    upd = torch.from_numpy(upa).to(dev) if upa is not None else None
    out = torch.empty(B, 4, device=dev, dtype=torch.float64)
    inlier = torch.empty(N, device=dev, dtype=torch.uint8)
    n_in = torch.empty(B, device=dev, dtype=torch.int32)
    L.check(L.lib().sfmi_plane_refit_f32(L.ptr(xf), L.ptr(od), None, None, None, L.ptr(seed), L.ptr(upd), B, N, 0, thr, 1, L.ptr(out),
                                         L.ptr(inlier), L.ptr(n_in), L.stream_ptr()), "sfmi_plane_refit_f32")
    return out, (inlier.reshape(shape) if shape else inlier), n_in


def remove_planes_dev(points, off=None, threshold=0.01, max_planes=1, min_ratio=0.2, hypotheses=1024, seed=0, up=None, refit=True):
    """Up to max_planes dominant planes per set, one after the other: -> keep (N,) uint8 (0 on a removed plane; (B,M) for a batch), planes
    (B,max_planes,4) f64 (NaN rows where none was taken), taken (B,) int32, on the device.
    Round r runs segment_plane_dev with seed + r on what the earlier rounds left of each set, compacted.  A set takes the round's plane
    when its inliers (n_in) are at least 3 and at least min_ratio x the set's ORIGINAL point count; otherwise it stops for good.
    Between two rounds the per-set counts are read back (one synchronisation per round after the first) to cut the compacted batch;
    max_planes = 1 reads nothing back."""
    what = "remove_planes_dev"
    check_nonneg(threshold, what, "threshold")
    max_planes = check_count(max_planes, what, "max_planes")
    min_ratio = check_nonneg(min_ratio, what, "min_ratio")
    check_count(hypotheses, what, "hypotheses")
    x, o, shape = point_sets(points, off, what)
    B, N = len(o) - 1, x.shape[0]
    _up_arg(up, B, what)
    dev = on_device(what, x)
    cur, co = x.float().contiguous(), o
    idx = torch.arange(N, device=dev)
    keep = torch.ones(N, device=dev, dtype=torch.uint8)
    planes = torch.full((B, max_planes, 4), float("nan"), device=dev, dtype=torch.float64)
    taken = torch.zeros(B, device=dev, dtype=torch.int32)
    active = torch.ones(B, device=dev, dtype=torch.bool)
    need = min_ratio * torch.from_numpy(np.diff(o)).to(dev).double()
    for r in range(max_planes):
        plane, inl, n_in, _, _, _ = segment_plane_dev(cur, co, threshold, hypotheses, seed + r, None, up, refit)
        active = active & (n_in >= 3) & (n_in.double() >= need)
        planes[:, r] = torch.where(active[:, None], plane, planes[:, r])
        taken += active.to(torch.int32)
        sid = set_ids(co, dev)
        drop = inl.bool() & active[sid]
        keep[idx[drop]] = 0
        if r + 1 == max_planes:
            break
        rem = ~drop & active[sid]                                   # a set that has stopped brings no points to the next round
        head = _counts(rem.to(torch.uint8), co).cpu().numpy()      # the read-back of the round
        if not head.any():
            break
        cur, idx = cur[rem], idx[rem]
        co = np.concatenate([[0], np.cumsum(head)]).astype(np.int64)
    return (keep.reshape(shape) if shape else keep), planes, taken


def _cluster_roots(xf, o, r2):
    dev = xf.device
    root = torch.empty(xf.shape[0], device=dev, dtype=torch.int32)
    if xf.shape[0]:
        od = offsets_dev(o, dev)
        L.check(L.lib().sfmi_cluster_f32(L.ptr(xf), L.ptr(od), len(o) - 1, xf.shape[0], _max_n(o), r2, L.ptr(root), L.stream_ptr()),
                "sfmi_cluster_f32")
    return root


def euclidean_clusters_dev(points, off=None, radius=None, min_points=1, return_root=False):
    """Euclidean cluster extraction (PCL EuclideanClusterExtraction; Open3D cluster_dbscan with min_points = 1), exact.

    points (N,3) f32 HIP tensor with (B+1,) offsets (None: one set), or a (B,M,3) batch.  Two points of a set are joined iff
    fmaf(dz, dz, fmaf(dy, dy, dx dx)) <= radius^2 with the square rounded to f32 and the compare in f32 (knn_dev's d2 bits, the rule of
    radius_outlier_mask_dev); a cluster is a connected component of that graph; a point with a NaN coordinate is a cluster of its own.
    -> label (N,) int32 ((B,M) for a batch): the rank of the point's cluster in its set under (size descending, lowest member index
    ascending), -1 for clusters of fewer than min_points points; sizes: int32 on the device, the kept clusters' sizes set after set in
    rank order; c_off (B+1,) host int64 offsets into sizes (the cluster counts are read back: one synchronisation).
    return_root: also root (N,) int32, the lowest local index of each point's cluster, as the library returns it.
    Bit-identical from run to run (lock-free union-find whose result does not depend on the schedule); a set's labels depend on that
    set alone.  Brute force over N^2 / 2 pairs per set: meant to run after voxel_downsample_dev, not on 10^6 raw points."""
    what = "euclidean_clusters_dev"
    if radius is None or isinstance(radius, bool) or not float(radius) >= 0:
        raise L.SfmiError(f"{what}: radius must be >= 0, got {radius!r}")
    min_points = check_count(min_points, what, "min_points")
    x, o, shape = point_sets(points, off, what)
    B, N = len(o) - 1, x.shape[0]
    if B > 65535 or (np.diff(o) >= 2 ** 31).any():
        raise L.SfmiError(f"{what}: at most 65535 sets, each below 2^31 points")
    dev = on_device(what, x)
    xf = x.float().contiguous()
    root = _cluster_roots(xf, o, float(np.float32(float(radius) ** 2)))
    if N == 0:
        out = (root.clone(), torch.empty(0, device=dev, dtype=torch.int32), np.zeros(B + 1, np.int64))
        return out + (root,) if return_root else out
    od = offsets_dev(o, dev)
    sid = set_ids(o, dev)
    g = root.long() + od[sid]                                                   # the root as a batch index
    size_at = torch.bincount(g, minlength=N)                                    # at a root: its cluster's size; elsewhere 0
    roots = torch.nonzero(size_at >= min_points)[:, 0]                          # ascending: (set, root)
    by_size = torch.sort(-size_at[roots], stable=True).indices
    by_set = torch.sort(sid[roots][by_size], stable=True).indices
    ranked = roots[by_size[by_set]]                                             # (set, size descending, root ascending)
    c_off_d = torch.searchsorted(sid[ranked].contiguous(), torch.arange(B + 1, device=dev))
    rank_at = torch.full((N,), -1, device=dev, dtype=torch.int32)
    rank_at[ranked] = (torch.arange(ranked.shape[0], device=dev) - c_off_d[sid[ranked]]).to(torch.int32)
    label = rank_at[g]
    out = ((label.reshape(shape) if shape else label), size_at[ranked].to(torch.int32), c_off_d.cpu().numpy().astype(np.int64))
    return out + (root,) if return_root else out


def largest_cluster_mask_dev(points, off=None, radius=None, min_points=1):
    """-> keep (N,) uint8 ((B,M) for a batch): the points of each set's largest Euclidean cluster (euclidean_clusters_dev's rank 0: the
    one with the lowest member index among equally large ones), count (B,) int32 its size, 0 where no cluster reaches min_points."""
    label, _, _ = euclidean_clusters_dev(points, off, radius, min_points)
    keep = (label == 0).to(torch.uint8)
    _, o, _ = point_sets(points, off, "largest_cluster_mask_dev")
    return keep, _counts(keep.reshape(-1), o)


def upright_rotation(normal, up=(0, 1, 0)):
    """(B,3,3) f64 rotations that take each `normal` (B,3) or (3,) onto `up`: the reference's geoutil.rotation_v1tov2 (xgutils/
    geoutil.py:14-19), a turn of 180 degrees about the bisector a of the two unit vectors, R = 2 a a^T - I, in plain arithmetic.  For
    normal = -up the bisector vanishes: the turn is about the first coordinate axis not parallel to up.  numpy in -> numpy out, torch
    in -> torch out (on the tensor's device)."""
    is_t = isinstance(normal, torch.Tensor)
    xp = torch if is_t else np
    n = normal.to(torch.float64) if is_t else np.asarray(normal, np.float64)
    if n.shape[-1:] != (3,) or n.ndim not in (1, 2):
        raise L.SfmiError(f"upright_rotation: expected (3,) or (B,3) normals, got {tuple(n.shape)}")
    n = n.reshape(-1, 3)
    u = np.asarray(up.detach().cpu().numpy() if isinstance(up, torch.Tensor) else up, np.float64)
    if u.shape != (3,) or not np.isfinite(u).all() or not np.linalg.norm(u) > 0:
        raise L.SfmiError("upright_rotation: up must be a finite non-zero (3,) vector")
    u = u / np.linalg.norm(u)
    e = np.zeros(3)
    e[int(np.argmax(np.abs(np.cross(np.eye(3), u)).sum(1) > 1e-12))] = 1.0      # the first axis not parallel to up
    fb = e - (e @ u) * u
    fb = fb / np.linalg.norm(fb)                                                # its part orthogonal to up: the antiparallel case's axis
    if is_t:
        u, fb = torch.from_numpy(u).to(n.device), torch.from_numpy(fb).to(n.device)
    v = n / xp.sqrt((n * n).sum(-1))[:, None]
    a = v + u
    la = xp.sqrt((a * a).sum(-1))[:, None]
    a = xp.where(la > 1e-8, a / xp.where(la > 1e-8, la, xp.ones_like(la)), fb[None] + 0 * a)
    eye = torch.eye(3, dtype=torch.float64, device=n.device) if is_t else np.eye(3)
    return 2.0 * a[:, :, None] * a[:, None, :] - eye[None]


def _compact(xf, o, keep):
    """the kept points of a ragged batch, their host offsets (one read-back) and their indices into xf"""
    count = _counts(keep, o).cpu().numpy()
    idx = torch.nonzero(keep)[:, 0]
    return xf[idx], np.concatenate([[0], np.cumsum(count)]).astype(np.int64), idx


def isolate_object_dev(points, off=None, plane_threshold=0.01, cluster_radius=0.05, max_planes=1, min_ratio=0.2, min_points=1,
                       up=(0, 1, 0), normalize=None, scale=None, hypotheses=1024, seed=0):
    """The object of a raw scan without its floor and its surroundings: remove_planes_dev -> turn the first plane's normal onto `up`
    (upright_rotation) -> largest_cluster_mask_dev on what is left -> optionally normalize_scan(mode=normalize, scale) set by set.
    -> kept (M,3) f32 points, ragged; k_off (B+1,) host int64; mask (N,) uint8 over the input ((B,M) for a batch); planes
    (B,max_planes,4) f64; rotation (B,3,3) f64 (identity for a set that gave no plane).
    The first plane's normal is pointed at the side that holds the rest of the set (the mean signed distance of the points off the
    planes is >= 0) before it is turned onto up: an object stands ON its floor.  Points are rotated in f64 and rounded to f32 once;
    clustering runs on the points as they came.  Two read-backs (the compactions), plus remove_planes_dev's between rounds."""
    what = "isolate_object_dev"
    if normalize is not None and normalize not in NORMALIZE_MODES:
        raise L.SfmiError(f"{what}: normalize must be None or one of {NORMALIZE_MODES}, got {normalize!r}")
    if cluster_radius is None or isinstance(cluster_radius, bool) or not float(cluster_radius) >= 0:
        raise L.SfmiError(f"{what}: cluster_radius must be >= 0, got {cluster_radius!r}")
    check_count(min_points, what, "min_points")
    x, o, shape = point_sets(points, off, what)
    B = len(o) - 1
    up = np.asarray(up.detach().cpu().numpy() if isinstance(up, torch.Tensor) else up, np.float64)      # host or device, as upright_rotation takes it
    keep, planes, taken = remove_planes_dev(x, o, plane_threshold, max_planes, min_ratio, hypotheses, seed)
    dev = x.device
    xf = x.float().contiguous()
    rest, ro, ridx = _compact(xf, o, keep)
    plane0 = planes[:, 0].clone()
    if rest.shape[0]:
        sid = set_ids(ro, dev)
        sd = (rest.double() * plane0[sid, :3]).sum(1) + plane0[sid, 3]
        side = torch.zeros(B, device=dev, dtype=torch.float64).index_add_(0, sid, torch.nan_to_num(sd))
        plane0 = torch.where((side < 0)[:, None], -plane0, plane0)
        planes = planes.clone()
        planes[:, 0] = plane0
    has = taken > 0
    rot = upright_rotation(torch.where(has[:, None], plane0[:, :3], torch.from_numpy(np.asarray(up, np.float64)).to(dev)[None]), up)
    big, _ = largest_cluster_mask_dev(rest, ro, cluster_radius, min_points)
    kept, k_off, kidx = _compact(rest, ro, big)
    mask = torch.zeros(xf.shape[0], device=dev, dtype=torch.uint8)
    mask[ridx[kidx]] = 1
    if kept.shape[0]:
        kept = torch.einsum("nij,nj->ni", rot[set_ids(k_off, dev)], kept.double()).float()
    if normalize is not None:
        kw = {} if scale is None else {"scale": scale}
        kept = torch.cat([normalize_scan(kept[int(k_off[b]):int(k_off[b + 1])], normalize, **kw) if k_off[b + 1] > k_off[b]
                          else kept[:0] for b in range(B)]) if B else kept
    return kept, k_off, (mask.reshape(shape) if shape else mask), planes, rot


# ---- the cleaning front end --------------------------------------------------------------------------------------------------------

def clean_cloud_dev(X, k=16, std_ratio=2.0, out_N=None, seed=0, voxel=None, resample="random", remove_planes=None, keep_cluster=None):
    """Statistical outlier removal of a batch of clouds, back at a fixed size: X (B,N,3) HIP tensor -> (B, out_N or N, 3) f32, each row
    a uniformly drawn kept point of its cloud (hpr.resample_visible_dev with the mask as `visible`: a counter hash of (seed, cloud
    index, row), no global RNG), and count (B,) int32 kept points per cloud.  That function's fallback applies: a cloud with two or
    fewer kept points is resampled from all its points.
    voxel: each cloud is first reduced to one centroid per occupied voxel of that edge (voxel_downsample_dev), the outlier rule runs on
    the ragged result (a density test wants one density) and count is the number of kept voxels.
    resample="fps": the rows are the kept points in farthest-point order (farthest_point_sample_dev with the mask as `valid`); a cloud
    that keeps fewer than out_N points continues cyclically through that order (row r = order[r mod count]); two or fewer kept points:
    all the cloud's points, as above.
    remove_planes / keep_cluster: dicts of remove_planes_dev / largest_cluster_mask_dev keyword arguments (threshold, max_planes,
    min_ratio, ...; radius, min_points).  The order is voxel -> planes -> outlier rule -> largest cluster -> resample: each step runs on
    what the step before kept, compacted (one read-back each), and count is what is kept at the end.
    The defaults take exactly the path this function always took."""
    from .hpr import resample_visible_dev
    x = points_arg(X, "clean_cloud_dev")
    if x.dim() != 3:
        raise L.SfmiError(f"clean_cloud_dev: expected (B,N,3) points, got {tuple(x.shape)}")
    n_out = x.shape[1] if out_N is None else int(out_N)
    if n_out < 0:
        raise L.SfmiError("clean_cloud_dev: out_N must be >= 0")
    if resample not in RESAMPLE_MODES:
        raise L.SfmiError(f"clean_cloud_dev: resample must be one of {RESAMPLE_MODES}, got {resample!r}")
    if voxel is not None:
        voxel = _check_voxel(voxel, "clean_cloud_dev")
    for name, d in (("remove_planes", remove_planes), ("keep_cluster", keep_cluster)):
        if d is not None and not isinstance(d, dict):
            raise L.SfmiError(f"clean_cloud_dev: {name} must be None or a dict of keyword arguments, got {d!r}")
    B, n = x.shape[:2]
    if remove_planes is not None or keep_cluster is not None:
        _check_k(k, "clean_cloud_dev")
        if voxel is None:
            xf, o = x.reshape(B * n, 3).float().contiguous(), np.arange(B + 1, dtype=np.int64) * n
        else:
            xf, o, _, _ = voxel_downsample_dev(x, None, voxel, "centroid")
        cur, co, idx = xf, o, torch.arange(xf.shape[0], device=xf.device)
        if remove_planes is not None:
            cur, co, sub = _compact(cur, co, remove_planes_dev(cur, co, **remove_planes)[0])
            idx = idx[sub]
        cur, co, sub = _compact(cur, co, statistical_outlier_mask_dev(cur, co, k, std_ratio)[0])
        idx = idx[sub]
        if keep_cluster is not None:
            idx = idx[torch.nonzero(largest_cluster_mask_dev(cur, co, **keep_cluster)[0])[:, 0]]
        keep = torch.zeros(xf.shape[0], device=xf.device, dtype=torch.uint8)
        keep[idx] = 1
        count = _counts(keep, o)
    elif voxel is None:
        keep, count, _ = statistical_outlier_mask_dev(x, None, k, std_ratio)
        xf, o = x.reshape(B * n, 3).float().contiguous(), np.arange(B + 1, dtype=np.int64) * n
    else:
        _check_k(k, "clean_cloud_dev")
        xf, o, _, _ = voxel_downsample_dev(x, None, voxel, "centroid")
        keep, count, _ = statistical_outlier_mask_dev(xf, o, k, std_ratio)
    keep = keep.reshape(-1)
    if resample == "random":
        return resample_visible_dev(xf, o, keep, count, n_out, 0., seed), count
    dev = xf.device
    if B == 0 or xf.shape[0] == 0:
        return torch.zeros(B, n_out, 3, device=dev, dtype=torch.float32), count
    od = offsets_dev(o, dev)
    few = torch.repeat_interleave(count <= 2, od[1:] - od[:-1], output_size=xf.shape[0])        # the fallback: all the cloud's points
    idx, _, got, _ = farthest_point_sample_dev(xf, o, n_out, valid=keep | few.to(torch.uint8))
    r = torch.arange(n_out, device=dev)[None, :] % got.clamp(min=1).long()[:, None]
    rows = (idx.long().gather(1, r) + od[:-1, None]).clamp(min=0, max=xf.shape[0] - 1)          # an empty cloud has no order: any row
    return xf[rows.reshape(-1)].reshape(B, n_out, 3), count
