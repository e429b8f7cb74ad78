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
  farthest_point_sample_dev(points, off, n, start, valid) -> idx (B,n) int32, d2 (B,n) f32, count (B,), status (B,)   (csrc/downsample.hip,
  voxel_downsample_dev(points, off, voxel, pick)          -> out (M,3) f32, out_off (B+1,) host, first (M,), count (M,)       DESIGN.md §5.15)
  clean_cloud_dev(X, k, std_ratio, out_N, seed, voxel, resample) -> (B, out_N, 3) cleaned clouds of a fixed size, count (B,)

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
from ._ragged import excl_at, host_offsets, on_device, point_sets, points_arg, run_starts, sorted_runs

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
    od = torch.from_numpy(o).to(dev)
    sd = torch.from_numpy(st).to(dev) if st is not None else None
    ws = torch.empty(max(int(lib.sfmi_fps_workspace_bytes(B, N, n)), 16), device=dev, dtype=torch.uint8)
    L.check(lib.sfmi_fps_f32(L.ptr(xf), L.ptr(od), L.ptr(vd), L.ptr(sd), B, N, n, L.ptr(idx), L.ptr(d2), L.ptr(count), L.ptr(status),
                             L.ptr(ws), L.stream_ptr()), "sfmi_fps_f32")
    return idx, d2, count, status


def _check_voxel(voxel, what):
    if isinstance(voxel, bool) or not isinstance(voxel, (int, float, np.integer, np.floating)) or not 0 < float(voxel) < float("inf"):
        raise L.SfmiError(f"{what}: voxel must be a finite number > 0, got {voxel!r}")
    return float(voxel)


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
    od = torch.from_numpy(o).to(dev)
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


# ---- the cleaning front end --------------------------------------------------------------------------------------------------------

def clean_cloud_dev(X, k=16, std_ratio=2.0, out_N=None, seed=0, voxel=None, resample="random"):
    """Statistical outlier removal of a batch of clouds, back at a fixed size: X (B,N,3) HIP tensor -> (B, out_N or N, 3) f32, each row
    a uniformly drawn kept point of its cloud (hpr.resample_visible_dev with the mask as `visible`: a counter hash of (seed, cloud
    index, row), no global RNG), and count (B,) int32 kept points per cloud.  That function's fallback applies: a cloud with two or
    fewer kept points is resampled from all its points.
    voxel: each cloud is first reduced to one centroid per occupied voxel of that edge (voxel_downsample_dev), the outlier rule runs on
    the ragged result (a density test wants one density) and count is the number of kept voxels.
    resample="fps": the rows are the kept points in farthest-point order (farthest_point_sample_dev with the mask as `valid`); a cloud
    that keeps fewer than out_N points continues cyclically through that order (row r = order[r mod count]); two or fewer kept points:
    all the cloud's points, as above.  The defaults take exactly the path this function always took."""
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
    B, n = x.shape[:2]
    if voxel is None:
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
    od = torch.from_numpy(o).to(dev)
    few = torch.repeat_interleave(count <= 2, od[1:] - od[:-1], output_size=xf.shape[0])        # the fallback: all the cloud's points
    idx, _, got, _ = farthest_point_sample_dev(xf, o, n_out, valid=keep | few.to(torch.uint8))
    r = torch.arange(n_out, device=dev)[None, :] % got.clamp(min=1).long()[:, None]
    rows = (idx.long().gather(1, r) + od[:-1, None]).clamp(min=0, max=xf.shape[0] - 1)          # an empty cloud has no order: any row
    return xf[rows.reshape(-1)].reshape(B, n_out, 3), count
