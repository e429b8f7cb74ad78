"""Rigid registration of partial scans on the device: iterative closest point - host side of csrc/register.hip.

The real-scan front end (scan.py, poisson.py) takes one cloud in one frame; raw captures arrive as several partial scans, each in
its own frame.  This module brings ragged batches of (source, target) pairs into a common frame, as Open3D's registration_icp does
(point-to-point and point-to-plane), and merges scans:

  transform_points_dev(points, off, pose)                          -> (N,3) f32, set b moved by pose b
  evaluate_registration_dev(source, target, s_off, t_off, max_dist, pose) -> fitness (B,), rmse (B,), idx (N,) int32, d2 (N,) f32
  icp_step_dev(source, target, ..., pose)                          -> one Gauss-Newton step: pose (B,4,4), xi (B,6), sums (B,29), idx, d2
  icp_dev(source, target, s_off, t_off, max_dist, metric, ...)     -> pose (B,4,4) f64, fitness, rmse (B,) f64, iterations, status (B,) int32
  icp_multiscale_dev(..., voxels, max_dists)                       -> the same, coarse to fine over voxel_downsample_dev
  merge_scans_dev(clouds, offs, voxel, **icp)                      -> merged (K,3) f32, poses (S,4,4) f64, status (S,) host int32

The contract (pose, transform, correspondences, residuals, sums, step, loop, status) is stated in include/sfmi.h and restated in numpy
in tests/icp_ref.py.  In short: the pose is (B,12) f64 on the device and is always applied to the original f32 source; the
correspondences are nn_dist's bits on the transformed cloud; the sums are f64 in a fixed order, so a batch equals per-pair calls bit
for bit; a pair that has ended is frozen on the device, so the result does not depend on check_every - the host only reads the (B,)
states every check_every iterations to stop early.  Everything is refused with SfmiError on the host before a launch; there is no CPU
fallback.

Global registration (csrc/features.hip, csrc/global_register.hip) gives ICP its start when the scans are not roughly
aligned beforehand - Open3D's compute_fpfh_feature and registration_ransac_based_on_feature_matching for ragged batches:

  fpfh_dev(points, normals, off, k, radius)                        -> feature (N,33) f32, spfh (N,33) int32, m (N,) int32
  fpfh_from_spfh_dev(points, off, k, radius, spfh, m)              -> the second stage alone
  match_features_dev(fs, ft, s_off, t_off, mutual)                 -> corr (C,2) int32, c_off (B+1,) host, idx (N,), d2 (N,)
  correspondence_hypotheses(sizes, H, seed)                        -> (B,H,3) int32 draws on the host (scan.plane_hypotheses)
  hypothesis_poses_dev(..., corr, c_off, triples, similarity)      -> poses (B,H,12) f64, valid (B,H) int32
  score_poses_dev(..., corr, c_off, max_dist, poses)               -> count (B,H) int32
  ransac_correspondences_dev(..., corr, c_off, max_dist, ...)      -> pose (B,4,4) f64, fitness, inlier (C,), n_in, count (B,H), best, status
  global_registration_dev(source, target, ..., voxel, max_dist)    -> the same, from the clouds alone
  merge_scans_dev(..., global_init={...})                          -> the global pose is the init of the ICP that follows

Its contract is stated in include/sfmi.h and restated in numpy in tests/global_reg_ref.py; its status: 0 ok, 1 no valid hypothesis,
2 fewer than 3 inliers or a degenerate refit, 4 a non-finite value in the pair; with 1, 2, 4 the pose is the identity.

Multiway registration (csrc/posegraph.hip) is for captures in which not every scan overlaps scan 0 - a ring or a chain:
pairwise ICP along the edges of a pose graph, one information matrix per edge, and Open3D's global_optimization on the device:

  information_matrix_dev(source, target, ..., max_dist, pose)      -> info (B,6,6) f64, count (B,) int32, fitness, rmse (B,) f64
  pose_graph_optimize_dev(nodes, src, tgt, transforms, infos, ...) -> poses (S,4,4) f64, l (E,), cost, iterations, status (Bg,)
  global_optimization_dev(..., preference, max_dist, prune)        -> poses, kept (E,) bool, l of pass one, status of both passes
  multiway_registration_dev(clouds, offs, pairs, max_dists, ...)   -> poses (S,4,4) f64, status (S,) host int32, a dict of the edges
  merge_scans_dev(..., multiway={...})                             -> the poses come from multiway_registration_dev

Its contract is stated in include/sfmi.h and restated in numpy in tests/posegraph_ref.py; the optimiser's status: 0 converged, 1
max_iter reached, 2 a node that no alive edge joins to node 0, 3 the damped system is not positive definite, lambda overflowed or an edge
turned by more than 3.1 rad, 4 a non-finite input.

ICP's status: 0 converged, 1 max_iter reached, 2 fewer than 3 (point) / 6 (plane) inliers, 3 the normal equations are not positive definite,
4 a non-finite coordinate, normal or initial pose in the pair.  With 2, 3 and 4 the pose stays where it was.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L
from ._ragged import (check_count, check_nonneg, check_number, excl_at, host_offsets, i32_dev, nonfinite_sets, offsets_dev, on_device,
                      pair_offsets, pair_sets, point_sets, points_arg, set_ids)

METRICS = ("point", "plane")
N_SUMS = 29


def _identity_poses(B):
    return np.tile(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float64), (B, 1))


def _pose_arg(pose, B, what, name="pose"):
    """None (identity), (B,4,4), (B,3,4), (B,12) or, for one pair, (4,4) / (3,4) / (12,) -> (B,12) f64 numpy or torch tensor"""
    if pose is None:
        return _identity_poses(B)
    p = pose.detach().to(torch.float64) if isinstance(pose, torch.Tensor) else np.asarray(pose, np.float64)
    if B == 1 and tuple(p.shape) in ((4, 4), (3, 4), (12,)):
        p = p[None]
    if tuple(p.shape) == (B, 4, 4):
        p = p[:, :3, :]
    if tuple(p.shape) == (B, 3, 4):
        p = p.reshape(B, 12)
    if tuple(p.shape) != (B, 12):
        raise L.SfmiError(f"{what}: {name} must be ({B},4,4), ({B},3,4) or ({B},12), got {tuple(pose.shape) if hasattr(pose, 'shape') else pose!r}")
    return p


def _pose_dev(p, dev):
    t = p if isinstance(p, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(p))
    return t.to(dev).contiguous().clone()


def _pose44(pose12):
    B = pose12.shape[0]
    out = torch.zeros(B, 4, 4, device=pose12.device, dtype=torch.float64)
    out[:, :3, :] = pose12.reshape(B, 3, 4)
    out[:, 3, 3] = 1.0
    return out


def _per_pair(v, B, what, name, conv, expect):
    """one value for every pair, or a list / tuple of B values -> a list of B converted values"""
    vals = list(v) if isinstance(v, (list, tuple)) else [v] * B
    if len(vals) != B:
        raise L.SfmiError(f"{what}: {name} must be one value or one per pair ({B}), got {len(vals)}")
    out = [conv(x) for x in vals]
    if any(x is None for x in out):
        raise L.SfmiError(f"{what}: {name} must be {expect}, got {v!r}")
    return out


def _check_tol(v, what, name):
    return check_number(v, what, name, 0, float("inf"), allow_inf=True)


def _check_unit(v, what, name):
    return check_number(v, what, name, 0, 1)


def transform_points_dev(points, off=None, pose=None):
    """Set b of the points moved by pose b: x' = f32(((r00 x + r01 y) + r02 z) + t0) and likewise y', z', in f64 with every product and
    sum rounded on its own.  points (N,3) f32 HIP tensor with (B+1,) offsets (None: one set) or a (B,M,3) batch; pose (B,4,4) /
    (B,3,4) / (B,12) f64, host or device.  -> f32 points of the same shape."""
    what = "transform_points_dev"
    x, o, shape = point_sets(points, off, what)
    B, N = len(o) - 1, x.shape[0]
    p = _pose_arg(pose, B, what)
    dev = on_device(what, x)
    xf = x.float().contiguous()
    out = torch.empty_like(xf)
    if B > 0 and N > 0:
        pd, od = _pose_dev(p, dev), offsets_dev(o, dev)
        L.check(L.lib().sfmi_icp_transform_f32(L.ptr(xf), L.ptr(od), L.ptr(pd), B, N, L.ptr(out), L.stream_ptr()), "sfmi_icp_transform_f32")
    return out.reshape(*shape, 3) if shape else out


class _Icp:
    """The device state of one call: validated arguments, the pose and the per-pair outputs; `iterate` runs one iteration."""

    def __init__(self, what, source, target, s_off, t_off, max_dist, metric, target_normals, init, pose_name="init"):
        s, t, so, to, _ = pair_sets(source, target, s_off, t_off, what)
        B = len(so) - 1
        if B < 1:
            raise L.SfmiError(f"{what}: expected at least one pair")
        metrics = _per_pair(metric, B, what, "metric", lambda m: m if isinstance(m, str) and m in METRICS else None,
                            f"one of {METRICS}")
        dists = _per_pair(max_dist, B, what, "max_dist", lambda v: check_nonneg(v, what, "max_dist"), "a finite number >= 0")
        maxd2 = np.array([np.float32(d ** 2) for d in dists], np.float32)         # rounded as radius_outlier_mask_dev rounds its radius
        n = None
        if "plane" in metrics:
            if not isinstance(target_normals, torch.Tensor) or target_normals.reshape(-1, 3).shape != t.shape:
                raise L.SfmiError(f"{what}: the plane metric needs target_normals, one unit normal per target point")
            n = target_normals.reshape(-1, 3)
        elif target_normals is not None:
            raise L.SfmiError(f"{what}: target_normals go with metric='plane'")
        p = _pose_arg(init, B, what, pose_name)
        dev = on_device(what, s, t, *([n] if n is not None else []))
        self.B, self.N, self.M, self.dev = B, s.shape[0], t.shape[0], dev
        self.metric = torch.from_numpy(np.array([METRICS.index(m) for m in metrics], np.int32)).to(dev)
        self.maxd2 = torch.from_numpy(maxd2).to(dev)
        self.max_n, self.max_m = int(np.diff(so).max()), int(np.diff(to).max())
        self.src, self.tgt = s.float().contiguous(), t.float().contiguous()
        self.nrm = n.float().contiguous() if n is not None else None
        self.sod, self.tod = offsets_dev(so, dev), offsets_dev(to, dev)
        self.pose = _pose_dev(p, dev)
        lib = self.lib = L.lib()
        i32 = dict(device=dev, dtype=torch.int32)
        f64 = dict(device=dev, dtype=torch.float64)
        self.state, self.status, self.iterations = (torch.empty(B, **i32) for _ in range(3))
        self.fitness, self.rmse = torch.empty(B, **f64), torch.empty(B, **f64)
        self.idx = torch.full((self.N,), -1, **i32)
        self.d2 = torch.full((self.N,), float("inf"), device=dev, dtype=torch.float32)
        self.sums, self.xi = torch.zeros(B, N_SUMS, **f64), torch.zeros(B, 6, **f64)
        S = int(lib.sfmi_icp_splits(B, self.N, self.M))
        self.pd = torch.empty(S * self.N, device=dev, dtype=torch.float32) if S > 1 else None
        self.pi = torch.empty(S * self.N, **i32) if S > 1 else None
        chunks = max(-(-self.max_n // int(lib.sfmi_icp_chunk())), 1)
        self.part = torch.empty(B * chunks * N_SUMS, **f64)
        self.block_off = torch.empty(B + 1, device=dev, dtype=torch.int64)
        bad = torch.empty(B, **i32)
        L.check(lib.sfmi_icp_begin_f32(L.ptr(self.src), L.ptr(self.tgt), L.ptr(self.nrm), L.ptr(self.sod), L.ptr(self.tod), L.ptr(self.pose),
                                       L.ptr(self.metric), B, self.N, self.M, self.max_n, self.max_m, L.ptr(bad), L.ptr(self.block_off), L.ptr(self.state),
                                       L.ptr(self.status), L.ptr(self.iterations), L.ptr(self.fitness), L.ptr(self.rmse), L.stream_ptr()),
                "sfmi_icp_begin_f32")

    def iterate(self, k, last, rel_fitness=0.0, rel_rmse=0.0):
        L.check(self.lib.sfmi_icp_iterate_f32(
            L.ptr(self.src), L.ptr(self.tgt), L.ptr(self.nrm), L.ptr(self.sod), L.ptr(self.tod), L.ptr(self.block_off), self.B, self.N, self.M,
            self.max_n, L.ptr(self.metric), L.ptr(self.maxd2), int(k), int(bool(last)), rel_fitness, rel_rmse, L.ptr(self.pose), L.ptr(self.state),
            L.ptr(self.status), L.ptr(self.iterations), L.ptr(self.fitness), L.ptr(self.rmse), L.ptr(self.idx), L.ptr(self.d2), L.ptr(self.pd),
            L.ptr(self.pi), L.ptr(self.part), L.ptr(self.sums), L.ptr(self.xi), L.stream_ptr()), "sfmi_icp_iterate_f32")

    def run(self, max_iter, rel_fitness, rel_rmse, check_every):
        for k in range(max_iter + 1):
            self.iterate(k, k == max_iter, rel_fitness, rel_rmse)
            if k < max_iter and (k + 1) % check_every == 0 and bool((self.state != 0).all()):     # the one read-back: (B,) states
                break


def evaluate_registration_dev(source, target, s_off=None, t_off=None, max_dist=None, pose=None):
    """Open3D's evaluate_registration for a batch of pairs under the given poses (None: identity): exactly icp_dev(max_iter=0).
    -> fitness (B,) f64 = inliers / source points, rmse (B,) f64 over the inliers, idx (N,) int32 the nearest target point of every
    transformed source point (local to its set), d2 (N,) f32 - the bits of metrics.nn_dist on the transformed cloud.  A pair with a
    non-finite coordinate or pose keeps idx = -1, d2 = +inf.  An empty pair has fitness 0 and rmse 0."""
    st = _Icp("evaluate_registration_dev", source, target, s_off, t_off, max_dist, "point", None, pose, "pose")
    st.iterate(0, True)
    return st.fitness, st.rmse, st.idx, st.d2


def icp_step_dev(source, target, s_off=None, t_off=None, max_dist=None, metric="point", target_normals=None, pose=None):
    """One Gauss-Newton step of icp_dev from `pose`, with what it was made of: -> pose' (B,4,4) f64, xi (B,6) f64 = (w, v), sums (B,29)
    f64 (A's 21 upper entries row-major | sum J^T r | sum d2 | count), idx (N,), d2 (N,), status (B,) (1: the step was taken; 2, 3, 4:
    it was not and pose' = pose, xi = 0)."""
    st = _Icp("icp_step_dev", source, target, s_off, t_off, max_dist, metric, target_normals, pose, "pose")
    st.iterate(0, False)
    return _pose44(st.pose), st.xi, st.sums, st.idx, st.d2, st.status


def icp_dev(source, target, s_off=None, t_off=None, max_dist=None, metric="point", target_normals=None, init=None, max_iter=30,
            rel_fitness=1e-6, rel_rmse=1e-6, check_every=8):
    """Iterative closest point for a ragged batch of pairs: the rigid motion that takes set b of `source` onto set b of `target`.

    source (N,3) / target (M,3) f32 HIP tensors with (B+1,) offsets s_off / t_off (None: one pair), or (B,N,3) / (B,M,3) batches.
    max_dist: correspondences farther than this are not used (d2 <= f32(max_dist^2) in f32).  metric "point" (point-to-point) or
    "plane" (point-to-plane; target_normals (M,3): one UNIT normal per target point, used as given).  init: (B,4,4) starting poses
    (None: identity).  The loop follows Open3D: iteration k evaluates fitness and rmse under the current pose and stops when both
    changed by less than rel_fitness / rel_rmse (absolute differences) since the iteration before; after max_iter steps one more
    evaluation makes fitness and rmse describe the returned pose; max_iter = 0 is exactly an evaluation.
    -> pose (B,4,4) f64, fitness (B,) f64, rmse (B,) f64, iterations (B,) int32, status (B,) int32 (the module's table), all on the
    device.  The result is a function of the input: bit-identical from run to run, in any batch, for any check_every."""
    what = "icp_dev"
    max_iter = check_count(max_iter, what, "max_iter", 0)
    check_every = check_count(check_every, what, "check_every", 1)
    rel_fitness, rel_rmse = _check_tol(rel_fitness, what, "rel_fitness"), _check_tol(rel_rmse, what, "rel_rmse")
    st = _Icp(what, source, target, s_off, t_off, max_dist, metric, target_normals, init)
    st.run(max_iter, rel_fitness, rel_rmse, check_every)
    return _pose44(st.pose), st.fitness, st.rmse, st.iterations, st.status


def icp_multiscale_dev(source, target, s_off=None, t_off=None, voxels=(0.04, 0.02, 0.01), max_dists=None, metric="point", init=None,
                       max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6, check_every=8, normals_k=16):
    """icp_dev from coarse to fine: at every level both clouds are reduced by scan.voxel_downsample_dev(voxel=voxels[l]) (centroids), the
    plane metric takes its normals from scan.estimate_normals_dev(k=normals_k) on the reduced target, and the pose found is the next
    level's init.  max_dists: one per level, by default 2 x the voxel size.  -> icp_dev's results at the last level."""
    from .scan import estimate_normals_dev, voxel_downsample_dev
    what = "icp_multiscale_dev"
    if metric not in METRICS:
        raise L.SfmiError(f"{what}: metric must be one of {METRICS}, got {metric!r}")
    try:
        voxels = [float(v) for v in voxels]
    except (TypeError, ValueError):
        voxels = []
    if not voxels or not all(0 < v < float("inf") for v in voxels):
        raise L.SfmiError(f"{what}: voxels must be a non-empty sequence of finite numbers > 0")
    max_dists = [2.0 * v for v in voxels] if max_dists is None else list(max_dists)
    if len(max_dists) != len(voxels):
        raise L.SfmiError(f"{what}: max_dists must have one entry per level ({len(voxels)}), got {len(max_dists)}")
    for m in max_dists:
        check_nonneg(m, what, "max_dists")
    s, so, _ = point_sets(source, s_off, f"{what} source")
    t, to, _ = point_sets(target, t_off, f"{what} target")
    pair_offsets(so, s.shape[0], to, t.shape[0], what)
    pose = _pose_arg(init, len(so) - 1, what, "init")
    on_device(what, s, t)
    out = None
    for voxel, md in zip(voxels, max_dists):
        sv, svo, _, _ = voxel_downsample_dev(s, so, voxel)
        tv, tvo, _, _ = voxel_downsample_dev(t, to, voxel)
        nrm = estimate_normals_dev(tv, tvo, normals_k)[0] if metric == "plane" else None
        out = icp_dev(sv, tv, svo, tvo, md, metric, nrm, pose, max_iter, rel_fitness, rel_rmse, check_every)
        pose = out[0]
    return out


# ---- global registration: FPFH features and RANSAC over correspondences (csrc/features.hip, csrc/global_register.hip)

FPFH_BINS = 33
GREG_SUMS = 16


def _radius_arg(radius, what, name="radius"):
    """None, or a finite number > 0 -> (use_radius, f32(radius^2)) rounded as radius_outlier_mask_dev rounds its radius"""
    if radius is None:
        return 0, 0.0
    return 1, float(np.float32(check_number(radius, what, name, 0, float("inf"), lo_open=True) ** 2))


def _normals_arg(normals, x, what):
    if not isinstance(normals, torch.Tensor) or normals.shape[-1:] != (3,) or normals.reshape(-1, 3).shape != x.shape:
        raise L.SfmiError(f"{what}: normals must be a tensor with one (3,) normal per point")
    return normals.reshape(-1, 3)


def _fpfh_stage2(o, idx, d2, spfh, m, k, use, r2, dev):
    B, N = len(o) - 1, idx.shape[0]
    out = torch.empty(N, FPFH_BINS, device=dev, dtype=torch.float32)
    if N:
        od = offsets_dev(o, dev)
        L.check(L.lib().sfmi_fpfh_features_f32(L.ptr(od), L.ptr(idx), L.ptr(d2), L.ptr(spfh), L.ptr(m), B, N, k, use, r2, L.ptr(out),
                                               L.stream_ptr()), "sfmi_fpfh_features_f32")
    return out


def _fpfh_from_knn(xf, nf, o, idx, d2, k, use, r2):
    """both stages on given neighbour rows: xf / nf (N,3) f32 contiguous, idx / d2 (N,k) -> feature, spfh, m"""
    dev = xf.device
    B, N = len(o) - 1, xf.shape[0]
    spfh = torch.empty(N, FPFH_BINS, device=dev, dtype=torch.int32)
    m = torch.empty(N, device=dev, dtype=torch.int32)
    if N:
        od = offsets_dev(o, dev)
        L.check(L.lib().sfmi_fpfh_spfh_f32(L.ptr(xf), L.ptr(nf), L.ptr(od), L.ptr(idx), L.ptr(d2), B, N, k, use, r2, L.ptr(spfh), L.ptr(m),
                                           L.stream_ptr()), "sfmi_fpfh_spfh_f32")
    return _fpfh_stage2(o, idx, d2, spfh, m, k, use, r2, dev), spfh, m


def fpfh_dev(points, normals, off=None, k=32, radius=None):
    """Fast point feature histograms (Open3D's compute_fpfh_feature): 3 x 11 bins per point.

    points (N,3) f32 HIP tensor with (B+1,) offsets (None: one set) or a (B,M,3) batch; normals of the same shape, used as given.  The
    neighbourhood is scan.knn_dev(points, points, k, exclude_self=True), k <= 64; with `radius` a neighbour farther than it is dropped
    (d2 <= f32(radius^2) in f32: the hybrid search).  -> feature (N,33) f32, spfh (N,33) int32 the simplified histograms' counts, m (N,)
    int32 the counted pairs of every point ((B,M,..) for a batch).  The pair feature, the bins and the weighting are include/sfmi.h's;
    the counts are exact up to the bits of atan2 at a bin edge, bit-identical from run to run and independent of the batch."""
    from .scan import _check_k, _launch_knn
    what = "fpfh_dev"
    k = _check_k(k, what)
    use, r2 = _radius_arg(radius, what)
    x, o, shape = point_sets(points, off, what)
    n = _normals_arg(normals, x, what)
    dev = on_device(what, x, n)
    xf, nf = x.float().contiguous(), n.float().contiguous()
    d2, idx = _launch_knn(xf, xf, o, o, k, True)
    feat, spfh, m = _fpfh_from_knn(xf, nf, o, idx, d2, k, use, r2)
    return (feat.reshape(*shape, FPFH_BINS), spfh.reshape(*shape, FPFH_BINS), m.reshape(shape)) if shape else (feat, spfh, m)


def fpfh_from_spfh_dev(points, off=None, k=32, radius=None, spfh=None, m=None):
    """The second stage of fpfh_dev alone, on given counts: spfh (N,33) int32 and m (N,) int32 -> feature (N,33) f32."""
    from .scan import _check_k, _launch_knn
    what = "fpfh_from_spfh_dev"
    k = _check_k(k, what)
    use, r2 = _radius_arg(radius, what)
    x, o, shape = point_sets(points, off, what)
    N = x.shape[0]
    if not isinstance(spfh, torch.Tensor) or not isinstance(m, torch.Tensor) or spfh.numel() != N * FPFH_BINS or m.numel() != N:
        raise L.SfmiError(f"{what}: spfh must be (N,{FPFH_BINS}) and m (N,) integer tensors for the {N} points")
    dev = on_device(what, x, spfh, m)
    xf = x.float().contiguous()
    d2, idx = _launch_knn(xf, xf, o, o, k, True)
    feat = _fpfh_stage2(o, idx, d2, spfh.reshape(N, FPFH_BINS).to(torch.int32).contiguous(), m.reshape(N).to(torch.int32).contiguous(), k,
                        use, r2, dev)
    return feat.reshape(*shape, FPFH_BINS) if shape else feat


def _features_arg(f, what, name):
    if not isinstance(f, torch.Tensor) or f.dim() != 2 or f.shape[1] != FPFH_BINS or not f.dtype.is_floating_point:
        raise L.SfmiError(f"{what}: {name} must be an (N,{FPFH_BINS}) float tensor on the HIP device (no CPU fallback)")
    return f


def _feature_nn(fa, fb, ao, bo, splits, q):
    """rows of fa against their pair's set of fb -> idx (N,) int32 local, d2 (N,) f32"""
    dev, lib = fa.device, L.lib()
    B, N, M = len(ao) - 1, fa.shape[0], fb.shape[0]
    idx = torch.full((N,), -1, device=dev, dtype=torch.int32)
    d2 = torch.full((N,), float("inf"), device=dev, dtype=torch.float32)
    if N == 0:
        return idx, d2
    qb = int(lib.sfmi_fpfh_query_block(q))
    block_off = np.concatenate([[0], np.cumsum(-(-np.diff(ao) // qb))]).astype(np.int64)
    S = splits if splits else int(lib.sfmi_fpfh_nn_splits(B, N, M, q))
    pd = torch.empty(S * N, device=dev, dtype=torch.float32) if S > 1 else None
    pi = torch.empty(S * N, device=dev, dtype=torch.int32) if S > 1 else None
    aod, bod, kod = (offsets_dev(v, dev) for v in (ao, bo, block_off))
    L.check(lib.sfmi_fpfh_nn_f32(L.ptr(fa), L.ptr(fb), L.ptr(aod), L.ptr(bod), L.ptr(kod), B, N, M, int(block_off[-1]), S, q, L.ptr(idx),
                                 L.ptr(d2), L.ptr(pd), L.ptr(pi), L.stream_ptr()), "sfmi_fpfh_nn_f32")
    return idx, d2


def match_features_dev(fs, ft, s_off=None, t_off=None, mutual=True, splits=None, queries_per_lane=None):
    """Correspondences by nearest neighbours in feature space, pair by pair: for every source feature the nearest target feature of its
    pair (f32 fmaf distances over the 33 bins, the lowest index among equal distances; include/sfmi.h); with `mutual` it is kept only
    if the target feature's nearest source feature is that source feature again.
    fs (N,33) / ft (M,33) f32 HIP tensors with (B+1,) offsets.  -> corr (C,2) int32 (source index, target index) local to the sets, in
    source order (compacted by prefix counts); c_off (B+1,) host int64 (the counts are read back: one synchronisation); idx (N,) int32
    and d2 (N,) f32 of the source -> target search.  splits / queries_per_lane: how the library cuts the work (None: its own choice);
    the result does not depend on them."""
    what = "match_features_dev"
    fs, ft = _features_arg(fs, what, "fs"), _features_arg(ft, what, "ft")
    so, to = pair_offsets(s_off, fs.shape[0], t_off, ft.shape[0], what)
    if len(so) - 1 > 65535 or (np.diff(so) >= 2 ** 31).any() or (np.diff(to) >= 2 ** 31).any():
        raise L.SfmiError(f"{what}: at most 65535 pairs, every set below 2^31 rows")
    if splits is not None and (isinstance(splits, bool) or not isinstance(splits, (int, np.integer)) or not 1 <= int(splits) <= 64):
        raise L.SfmiError(f"{what}: splits must be None or an integer in [1, 64], got {splits!r}")
    if queries_per_lane not in (None, 2, 4) or isinstance(queries_per_lane, bool):
        raise L.SfmiError(f"{what}: queries_per_lane must be None, 2 or 4, got {queries_per_lane!r}")
    dev = on_device(what, fs, ft)
    S, q = int(splits or 0), int(queries_per_lane or 0)
    fs, ft = fs.float().contiguous(), ft.float().contiguous()
    idx, d2 = _feature_nn(fs, ft, so, to, S, q)
    N = fs.shape[0]
    sod, tod = offsets_dev(so, dev), offsets_dev(to, dev)
    sid = set_ids(so, dev)
    local = torch.arange(N, device=dev) - sod[sid]
    keep = idx >= 0
    if mutual and N and ft.shape[0]:
        back, _ = _feature_nn(ft, fs, to, so, S, q)
        keep &= back[(idx.long().clamp(min=0) + tod[sid]).clamp(max=ft.shape[0] - 1)].long() == local
    pre = torch.cumsum(keep, 0, dtype=torch.int64)
    c_off = torch.cat([pre.new_zeros(1), pre])[sod].cpu().numpy().astype(np.int64)          # the one read-back
    rows = torch.nonzero(keep)[:, 0]
    corr = torch.stack([local[rows], idx[rows].long()], 1).to(torch.int32).contiguous()
    return corr, c_off, idx, d2


def correspondence_hypotheses(sizes, H, seed=0):
    """The RANSAC draws of ransac_correspondences_dev: scan.plane_hypotheses' counter-hash draws over the correspondences of every pair,
    (B,H,3) int32 on the host.  Repeated indices are not redrawn: the kernel marks such a hypothesis invalid."""
    from .scan import plane_hypotheses
    return plane_hypotheses(sizes, H, seed)


class _Greg:
    """The validated arguments of one RANSAC call on the device"""

    def __init__(self, what, source, target, s_off, t_off, corr, c_off):
        s, t, so, to, _ = pair_sets(source, target, s_off, t_off, what)
        B = len(so) - 1
        if B < 1:
            raise L.SfmiError(f"{what}: expected at least one pair")
        if not isinstance(corr, torch.Tensor) or corr.dim() != 2 or corr.shape[1] != 2 or corr.dtype.is_floating_point or corr.dtype == torch.bool:
            raise L.SfmiError(f"{what}: corr must be a (C,2) integer tensor of (source index, target index)")
        co = host_offsets(c_off, corr.shape[0], f"{what} c_off")
        if len(co) != B + 1 or (np.diff(co) >= 2 ** 31).any():
            raise L.SfmiError(f"{what}: c_off must cut the correspondences into the {B} pairs")
        if corr.shape[0] and (s.numel() == 0 or t.numel() == 0):
            raise L.SfmiError(f"{what}: corr names points of empty clouds")
        self.B, self.so, self.to, self.co = B, so, to, co
        self.s, self.t, self.corr = s, t, corr

    def to_device(self, what, *more):
        dev = self.dev = on_device(what, self.s, self.t, self.corr, *more)
        self.s, self.t = self.s.float().contiguous(), self.t.float().contiguous()
        self.corr = self.corr.to(torch.int32).contiguous()
        self.sod, self.tod, self.cod = (offsets_dev(v, dev) for v in (self.so, self.to, self.co))
        self.max_c = int(np.diff(self.co).max())
        return dev

    def bad_pairs(self):
        """(B,) int32: a coordinate of the pair is not finite"""
        return nonfinite_sets(self.s, self.sod) | nonfinite_sets(self.t, self.tod)

    def poses(self, trd, similarity):
        H = trd.shape[1]
        poses = torch.empty(self.B, H, 12, device=self.dev, dtype=torch.float64)
        valid = torch.empty(self.B, H, device=self.dev, dtype=torch.int32)
        L.check(L.lib().sfmi_greg_poses_f32(L.ptr(self.s), L.ptr(self.t), L.ptr(self.sod), L.ptr(self.tod), L.ptr(self.corr), L.ptr(self.cod),
                                            L.ptr(trd), self.B, H, self.corr.shape[0], similarity, L.ptr(poses), L.ptr(valid), L.stream_ptr()),
                "sfmi_greg_poses_f32")
        return poses, valid

    def score(self, poses, valid, bad, maxd2):
        H = poses.shape[1]
        i32 = dict(device=self.dev, dtype=torch.int32)
        count, best, status = torch.empty(self.B, H, **i32), torch.empty(self.B, **i32), torch.empty(self.B, **i32)
        L.check(L.lib().sfmi_greg_score_f32(L.ptr(self.s), L.ptr(self.t), L.ptr(self.sod), L.ptr(self.tod), L.ptr(self.corr), L.ptr(self.cod),
                                            L.ptr(poses), L.ptr(valid), L.ptr(bad), self.B, H, self.max_c, maxd2, L.ptr(count), L.ptr(best),
                                            L.ptr(status), L.stream_ptr()), "sfmi_greg_score_f32")
        return count, best, status

    def refit(self, poses, best, status, maxd2, refit):
        H, C = poses.shape[1], self.corr.shape[0]
        pose = torch.empty(self.B, 12, device=self.dev, dtype=torch.float64)
        inlier = torch.zeros(C, device=self.dev, dtype=torch.uint8)
        n_in = torch.empty(self.B, device=self.dev, dtype=torch.int32)
        sums = torch.empty(self.B, GREG_SUMS, device=self.dev, dtype=torch.float64)
        L.check(L.lib().sfmi_greg_refit_f32(L.ptr(self.s), L.ptr(self.t), L.ptr(self.sod), L.ptr(self.tod), L.ptr(self.corr), L.ptr(self.cod),
                                            L.ptr(poses), L.ptr(best), self.B, H, C, maxd2, int(bool(refit)), L.ptr(status), L.ptr(pose),
                                            L.ptr(inlier), L.ptr(n_in), L.ptr(sums), L.stream_ptr()), "sfmi_greg_refit_f32")
        return pose, inlier, n_in, sums


def _triples_arg(tr, B, what):
    if not isinstance(tr, torch.Tensor):
        tr = np.asarray(tr)
        if tr.dtype == np.bool_ or not np.issubdtype(tr.dtype, np.integer):
            raise L.SfmiError(f"{what}: triples must be integers")
    elif tr.dtype.is_floating_point or tr.dtype == torch.bool:
        raise L.SfmiError(f"{what}: triples must be integers")
    if tr.ndim != 3 or tr.shape[0] != B or tr.shape[1] < 1 or tr.shape[2] != 3:
        raise L.SfmiError(f"{what}: triples must be ({B},H,3) with H >= 1, got {tuple(tr.shape)}")
    return tr


def _triples_dev(tr, dev):
    return (tr if isinstance(tr, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(tr)).to(dev)).to(torch.int32).contiguous()


def _maxd2(max_dist, what):
    return float(np.float32(check_nonneg(max_dist, what, "max_dist") ** 2))


def hypothesis_poses_dev(source, target, s_off=None, t_off=None, corr=None, c_off=None, triples=None, similarity=0.9):
    """The poses of RANSAC hypotheses: triples (B,H,3) of correspondence indices local to each pair -> poses (B,H,12) f64 row-major
    [R | t] (NaN for an invalid hypothesis), valid (B,H) int32.  The validity rules and the three-pair Kabsch are include/sfmi.h's."""
    what = "hypothesis_poses_dev"
    a = _Greg(what, source, target, s_off, t_off, corr, c_off)
    tr = _triples_arg(triples, a.B, what)
    sim = _check_unit(similarity, what, "similarity")
    dev = a.to_device(what, *([tr] if isinstance(tr, torch.Tensor) else []))
    return a.poses(_triples_dev(tr, dev), sim)


def score_poses_dev(source, target, s_off=None, t_off=None, corr=None, c_off=None, max_dist=None, poses=None):
    """count (B,H) int32: how many correspondences of pair b lie within max_dist under pose h of the pair - the transform of
    transform_points_dev, d2 by nn_dist's f32 rule, d2 <= f32(max_dist^2).  poses (B,H,12) / (B,H,3,4) / (B,H,4,4) f64."""
    what = "score_poses_dev"
    a = _Greg(what, source, target, s_off, t_off, corr, c_off)
    maxd2 = _maxd2(max_dist, what)
    p = poses.detach().to(torch.float64) if isinstance(poses, torch.Tensor) else torch.from_numpy(np.asarray(poses, np.float64))
    if p.dim() == 4 and p.shape[2:] == (4, 4):
        p = p[:, :, :3, :]
    if p.dim() < 3 or p.shape[0] != a.B or p.shape[1] < 1 or p[0, 0].numel() != 12:
        raise L.SfmiError(f"{what}: poses must be ({a.B},H,12), ({a.B},H,3,4) or ({a.B},H,4,4), got {tuple(poses.shape)}")
    dev = a.to_device(what)
    p = p.reshape(a.B, p.shape[1], 12).to(dev).contiguous()
    return a.score(p, None, None, maxd2)[0]


def _ransac(what, a, max_dist, hypotheses, seed, triples, similarity, refit, extra_bad=None):
    maxd2 = _maxd2(max_dist, what)
    sim = _check_unit(similarity, what, "similarity")
    tr = (correspondence_hypotheses(np.diff(a.co), check_count(hypotheses, what, "hypotheses"), seed) if triples is None
          else _triples_arg(triples, a.B, what))
    dev = a.to_device(what, *([tr] if isinstance(tr, torch.Tensor) else []))
    trd = _triples_dev(tr, dev)
    bad = a.bad_pairs()
    if extra_bad is not None:
        bad |= extra_bad.to(torch.int32)
    poses, valid = a.poses(trd, sim)
    count, best, status = a.score(poses, valid, bad, maxd2)
    pose, inlier, n_in, sums = a.refit(poses, best, status, maxd2, refit)
    C = torch.from_numpy(np.diff(a.co)).to(dev).double()
    fitness = torch.where(C > 0, n_in.double() / C.clamp(min=1), torch.zeros_like(C))
    return (_pose44(pose), fitness, inlier, n_in, count, best, status), dict(poses=poses, valid=valid, sums=sums)


def ransac_correspondences_dev(source, target, s_off=None, t_off=None, corr=None, c_off=None, max_dist=None, hypotheses=4096, seed=0,
                               triples=None, similarity=0.9, refit=True, details=False):
    """RANSAC over correspondences for a ragged batch of pairs (Open3D's registration_ransac_based_on_feature_matching with its edge
    length checker), exact in its counts and deterministic.

    source / target / offsets as icp_dev takes them; corr (C,2) integers (source index, target index) local to the pair's sets with
    (B+1,) offsets c_off, as match_features_dev returns them.  A hypothesis is a triple of correspondence indices of the pair:
    correspondence_hypotheses(sizes, hypotheses, seed), or `triples` (B,H,3).  Its pose is the least-squares rigid motion of the three
    pairs; it is invalid (count -1) when an index repeats or lies outside, two of its points coincide, an edge of the two triangles
    fails ls >= similarity lt and lt >= similarity ls, or the triangle is degenerate.  count[b,h] = the correspondences within max_dist
    under pose h (score_poses_dev's rule); best[b] = the valid hypothesis of largest count, the lowest h among equal counts.
    refit=True: the least-squares motion of the winner's inliers (f64 sums in a fixed order) and the inliers under it.
    -> pose (B,4,4) f64, fitness (B,) f64 = n_in / C, inlier (C,) uint8, n_in (B,) int32, count (B,H) int32, best (B,) int32, status (B,)
    int32, all on the device: 0 ok, 1 no valid hypothesis (fewer than 3 correspondences included), 2 the winner has fewer than 3
    inliers or the refit is degenerate, 4 a non-finite coordinate in the pair; with 1, 2 and 4 the pose is the identity.  With
    `details` a dict(poses (B,H,12), valid (B,H), sums (B,16)) follows.  Bit-identical from run to run; a pair's results depend on that
    pair alone."""
    what = "ransac_correspondences_dev"
    a = _Greg(what, source, target, s_off, t_off, corr, c_off)
    out, more = _ransac(what, a, max_dist, hypotheses, seed, triples, similarity, refit)
    return out + (more,) if details else out


def _oriented_normals(x, o, k, viewpoint):
    """estimate_normals_dev, turned towards the viewpoints or, without them, away from each set's centroid (a frame-covariant choice; the
    centroid is the set's own, summed in a fixed order on the device: a set's normals do not depend on the batch around it).  x: (N,3) f32
    contiguous"""
    from .scan import estimate_normals_dev
    if viewpoint is not None:
        return estimate_normals_dev(x, o, k, viewpoint)[0]
    n = estimate_normals_dev(x, o, k)[0].contiguous()
    if x.shape[0]:
        od = offsets_dev(o, x.device)
        L.check(L.lib().sfmi_fpfh_orient_f32(L.ptr(x), L.ptr(od), len(o) - 1, x.shape[0], L.ptr(n), L.stream_ptr()), "sfmi_fpfh_orient_f32")
    return n


def global_registration_dev(source, target, s_off=None, t_off=None, voxel=None, normals_k=16, feature_k=32, feature_radius=None,
                            max_dist=None, viewpoints=None, mutual=True, **ransac):
    """Coarse alignment of every (source, target) pair without a starting pose: both clouds are reduced by scan.voxel_downsample_dev
    (voxel=None: used as they are), get normals (scan.estimate_normals_dev with normals_k, turned towards `viewpoints` = (source (B,3),
    target (B,3)) or, with None, away from each set's centroid), FPFH features (fpfh_dev with feature_k, feature_radius), correspondences
    (match_features_dev) and a pose by ransac_correspondences_dev(max_dist, **ransac); max_dist defaults to 1.5 x voxel.
    -> ransac_correspondences_dev's results; the correspondences index the reduced clouds.  The pose is a start for icp_dev."""
    from .scan import _check_k, _check_voxel, voxel_downsample_dev
    what = "global_registration_dev"
    s, so, _ = point_sets(source, s_off, f"{what} source")
    t, to, _ = point_sets(target, t_off, f"{what} target")
    pair_offsets(so, s.shape[0], to, t.shape[0], what)
    if not 1 <= len(so) - 1 <= 65535:
        raise L.SfmiError(f"{what}: between 1 and 65535 pairs")
    if voxel is not None:
        voxel = _check_voxel(voxel, what)
    if max_dist is None:
        if voxel is None:
            raise L.SfmiError(f"{what}: max_dist is needed when voxel is None")
        max_dist = 1.5 * voxel
    check_nonneg(max_dist, what, "max_dist")
    _check_k(normals_k, what)
    _check_k(feature_k, what)
    _radius_arg(feature_radius, what, "feature_radius")
    bad_kw = set(ransac) - {"hypotheses", "seed", "triples", "similarity", "refit"}
    if bad_kw:
        raise L.SfmiError(f"{what}: unknown arguments {sorted(bad_kw)}")
    vs, vt = (None, None)
    if viewpoints is not None:
        if not isinstance(viewpoints, (tuple, list)) or len(viewpoints) != 2:
            raise L.SfmiError(f"{what}: viewpoints must be None or a pair (source viewpoints, target viewpoints)")
        vs, vt = viewpoints
    on_device(what, s, t)
    s, t = s.float().contiguous(), t.float().contiguous()
    if voxel is not None:
        s, so = voxel_downsample_dev(s, so, voxel)[:2]
        t, to = voxel_downsample_dev(t, to, voxel)[:2]
    ns, nt = _oriented_normals(s, so, normals_k, vs), _oriented_normals(t, to, normals_k, vt)
    fs, ft = fpfh_dev(s, ns, so, feature_k, feature_radius)[0], fpfh_dev(t, nt, to, feature_k, feature_radius)[0]
    corr, co, _, _ = match_features_dev(fs, ft, so, to, mutual)
    a = _Greg(what, s, t, so, to, corr, co)
    a.to_device(what)
    extra = nonfinite_sets(ns, a.sod) | nonfinite_sets(fs, a.sod) | nonfinite_sets(nt, a.tod) | nonfinite_sets(ft, a.tod)
    return _ransac(what, a, max_dist, ransac.get("hypotheses", 4096), ransac.get("seed", 0), ransac.get("triples"),
                   ransac.get("similarity", 0.9), ransac.get("refit", True), extra)[0]


def merge_scans_dev(clouds, offs=None, voxel=None, global_init=None, multiway=None, **icp):
    """Several partial scans of one object, each in its own frame, merged in the frame of scan 0.

    clouds: a list of (n_i,3) HIP tensors, or one (N,3) tensor with (S+1,) offsets `offs`.  Scans 1.. are registered onto scan 0 in one
    batch - icp_dev(**icp), or icp_multiscale_dev when `voxels` is among the keyword arguments - and transformed; the clouds are
    concatenated in scan order and, with `voxel`, reduced by scan.voxel_downsample_dev.  A scan whose status is >= 2 is left out and
    reported.  global_init: a dict of global_registration_dev's arguments; the pose it finds for a scan is the `init` of the ICP that
    follows, for scans that are not roughly aligned beforehand (a scan whose global status is >= 1 keeps the identity); None: the scans
    start from `init` or the identity.  -> merged (K,3) f32, poses (S,4,4) f64 (identity for scan 0), status (S,) host int32 (0 for
    scan 0).  The statuses are read back (one synchronisation).
    multiway: a dict of multiway_registration_dev's arguments (max_dists, pairs, global_init, ICP options ...): the poses come from the
    pose graph over all pairs instead of the star onto scan 0, for captures in which not every scan overlaps scan 0; every other
    registration argument then goes into that dict.  None: the star."""
    from .scan import _check_voxel, voxel_downsample_dev
    what = "merge_scans_dev"
    if multiway is not None and (not isinstance(multiway, dict) or global_init is not None or icp):
        raise L.SfmiError(f"{what}: multiway must be a dict of multiway_registration_dev arguments; global_init and the ICP options go inside it")
    if global_init is not None and (not isinstance(global_init, dict) or "init" in icp):
        raise L.SfmiError(f"{what}: global_init must be a dict of global_registration_dev arguments and replaces init")
    if voxel is not None:
        voxel = _check_voxel(voxel, what)
    parts, o = _scans_arg(clouds, offs, what)
    dev = on_device(what, *parts)
    x = (torch.cat([c.float() for c in parts]) if len(parts) > 1 else parts[0].float()).contiguous()
    S = len(o) - 1
    poses = torch.eye(4, device=dev, dtype=torch.float64).repeat(S, 1, 1)
    status = np.zeros(S, np.int32)
    first = x[:int(o[1])]
    if multiway is not None:
        poses, status, _ = multiway_registration_dev(x, o, **multiway)
        moved = transform_points_dev(x, o, poses)
        merged = torch.cat([moved[int(o[i]):int(o[i + 1])] for i in range(S) if status[i] < 2])
    elif S > 1:
        src, so = x[int(o[1]):], o[1:] - o[1]
        tgt, to = first.repeat(S - 1, 1), np.arange(S, dtype=np.int64) * first.shape[0]
        run = icp_multiscale_dev if "voxels" in icp else icp_dev
        if global_init is not None:
            g = global_registration_dev(src, tgt, so, to, **global_init)
            icp = dict(icp, init=torch.where((g[6] < 1)[:, None, None], g[0], poses[1:]))
        pose, _, _, _, st = run(src, tgt, so, to, **icp)
        poses[1:] = pose
        status[1:] = st.cpu().numpy()
        moved = transform_points_dev(src, so, pose)
        keep = [first] + [moved[int(so[i]):int(so[i + 1])] for i in range(S - 1) if status[i + 1] < 2]
        merged = torch.cat(keep)
    else:
        merged = first
    if voxel is not None and merged.shape[0]:
        merged = voxel_downsample_dev(merged, None, voxel)[0]
    return merged, poses, status


# ---- multiway registration: information matrices and pose-graph optimisation (csrc/posegraph.hip) -------------------

PG_MAX_NODES, PG_MAX_EDGES = 32, 496
PG_INFO_SUMS = 10


def _information(st):
    """the information matrices of the pairs of an evaluated _Icp state, from the correspondences it holds -> info, count, flag"""
    B, dev, lib = st.B, st.dev, st.lib
    chunks = max(-(-st.max_n // int(lib.sfmi_pg_chunk())), 1)
    part = torch.empty(B * chunks * PG_INFO_SUMS, device=dev, dtype=torch.float64)
    info = torch.empty(B, 6, 6, device=dev, dtype=torch.float64)
    count, flag, bad = (torch.empty(B, device=dev, dtype=torch.int32) for _ in range(3))
    L.check(lib.sfmi_pg_information_f32(L.ptr(st.src), L.ptr(st.tgt), L.ptr(st.sod), L.ptr(st.tod), L.ptr(st.pose), L.ptr(st.idx), L.ptr(st.d2),
                                        L.ptr(st.maxd2), B, st.N, st.M, st.max_n, st.max_m, L.ptr(bad), L.ptr(part), L.ptr(info), L.ptr(count),
                                        L.ptr(flag), L.stream_ptr()), "sfmi_pg_information_f32")
    return info, count, flag


def information_matrix_dev(source, target, s_off=None, t_off=None, max_dist=None, pose=None, details=False):
    """Open3D's get_information_matrix_from_point_clouds for a batch of pairs under the given poses (None: identity): the
    correspondences of evaluate_registration_dev, and over its inliers info = sum G^T G with G = [-[q]x | I], q the target point - the
    point metric's J^T J of icp_step_dev with q in place of the moved source point.  max_dist may differ from pair to pair.
    -> info (B,6,6) f64 symmetric, count (B,) int32 (= info[:,5,5]), fitness (B,) f64, rmse (B,) f64; with `details` also flag (B,) int32:
    1 for a pair with a non-finite coordinate or pose (info 0, count 0).  An empty pair has info 0, count 0 and flag 0.  f64 sums in
    icp_dev's fixed order: a batch equals per-pair calls bit for bit."""
    st = _Icp("information_matrix_dev", source, target, s_off, t_off, max_dist, "point", None, pose, "pose")
    st.iterate(0, True)
    info, count, flag = _information(st)
    return (info, count, st.fitness, st.rmse, flag) if details else (info, count, st.fitness, st.rmse)


def _edge_ints(v, E, what, name):
    a = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
    if a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer) or a.shape != (E,):
        raise L.SfmiError(f"{what}: {name} must be ({E},) integers, one per edge")
    return a.astype(np.int64)


def _edge_flags(v, E, what, name, default):
    """None, a host array or a tensor of E integers / booleans -> host int32 array or the tensor"""
    if v is None:
        return np.full(E, default, np.int32)
    if isinstance(v, torch.Tensor):
        if v.dtype.is_floating_point or tuple(v.shape) != (E,):
            raise L.SfmiError(f"{what}: {name} must be ({E},) integers or booleans, one per edge")
        return v
    a = np.asarray(v)
    if not (a.dtype == np.bool_ or np.issubdtype(a.dtype, np.integer)) or a.shape != (E,):
        raise L.SfmiError(f"{what}: {name} must be ({E},) integers or booleans, one per edge")
    return (a != 0).astype(np.int32)


class _Graph:
    """The validated arguments of one optimiser call: a ragged batch of pose graphs"""

    def __init__(self, what, nodes, src, tgt, transforms, infos, uncertain, alive, n_off, e_off):
        self.what = what
        if not hasattr(nodes, "shape") or len(nodes.shape) < 1:
            raise L.SfmiError(f"{what}: nodes must be (S,4,4), (S,3,4) or (S,12) poses")
        S = int(nodes.shape[0])
        self.X = _pose_arg(nodes, S, what, "nodes")
        E = len(src) if hasattr(src, "__len__") else -1
        if E < 0:
            raise L.SfmiError(f"{what}: src must be (E,) integers, one per edge")
        self.srch, self.tgth = _edge_ints(src, E, what, "src"), _edge_ints(tgt, E, what, "tgt")
        if not hasattr(transforms, "shape"):
            raise L.SfmiError(f"{what}: transforms must be ({E},4,4), ({E},3,4) or ({E},12)")
        self.T = _pose_arg(transforms, E, what, "transforms")
        if not hasattr(infos, "shape") or tuple(infos.shape) != (E, 6, 6):
            raise L.SfmiError(f"{what}: infos must be ({E},6,6), one information matrix per edge, got {tuple(getattr(infos, 'shape', ()))}")
        self.Lam = infos
        self.unc = _edge_flags(uncertain, E, what, "uncertain", 0)
        self.alive = _edge_flags(alive, E, what, "alive", 1)
        no, eo = host_offsets(n_off, S, f"{what} n_off"), host_offsets(e_off, E, f"{what} e_off")
        if len(no) != len(eo):
            raise L.SfmiError(f"{what}: n_off describes {len(no) - 1} graphs, e_off {len(eo) - 1}")
        ns, es = np.diff(no), np.diff(eo)
        if ns.min() < 1 or ns.max() > PG_MAX_NODES or es.max() > PG_MAX_EDGES:
            raise L.SfmiError(f"{what}: a graph has between 1 and {PG_MAX_NODES} nodes and at most {PG_MAX_EDGES} edges, got up to {ns.max()} "
                              f"nodes and {es.max()} edges")
        size = np.repeat(ns, es)
        if ((self.srch < 0) | (self.srch >= size) | (self.tgth < 0) | (self.tgth >= size) | (self.srch == self.tgth)).any():
            raise L.SfmiError(f"{what}: src / tgt must be node indices inside their own graph, and differ")
        self.S, self.E, self.Bg, self.no, self.eo, self.max_s = S, E, len(no) - 1, no, eo, int(ns.max())

    def to_device(self):
        t = [v for v in (self.T, self.Lam, self.X, self.unc, self.alive) if isinstance(v, torch.Tensor)]
        if not t:
            raise L.SfmiError(f"{self.what} needs HIP device tensors (no CPU fallback)")
        dev = self.dev = on_device(self.what, *t)
        f64 = lambda v: (v if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v, np.float64))).to(dev).to(torch.float64)
        i32 = lambda v: ((v != 0) if isinstance(v, torch.Tensor) else torch.from_numpy(v).to(dev)).to(dev).to(torch.int32).contiguous()
        self.X, self.T = f64(self.X).reshape(self.S, 12).contiguous(), f64(self.T).reshape(self.E, 12).contiguous()
        self.Lam = f64(self.Lam).reshape(self.E, 36).contiguous()
        self.unc, self.alive = i32(self.unc), i32(self.alive)
        self.src, self.tgt = i32_dev(self.srch, dev), i32_dev(self.tgth, dev)
        self.nod, self.eod = offsets_dev(self.no, dev), offsets_dev(self.eo, dev)
        return dev

    def run(self, X, alive, mu, max_iter, tol):
        """one launch -> X' (S,12), l, cost, iterations, status, details"""
        dev, Bg, E = self.dev, self.Bg, self.E
        nmax = 6 * (self.max_s - 1)
        f64 = dict(device=dev, dtype=torch.float64)
        X = X.clone()
        src, tgt, T, Lam, unc = self.src, self.tgt, self.T, self.Lam, self.unc
        if E == 0:                                             # no edge in the batch: one unused element each, so no pointer is NULL
            src = tgt = unc = alive = torch.zeros(1, device=dev, dtype=torch.int32)
            T = Lam = torch.zeros(36, **f64)
        l, ework = torch.zeros(max(E, 1), **f64), torch.empty(max(E, 1) * 27, **f64)
        cost, lam = torch.empty(Bg, **f64), torch.empty(Bg, **f64)
        it, status = torch.empty(Bg, device=dev, dtype=torch.int32), torch.empty(Bg, device=dev, dtype=torch.int32)
        H = torch.zeros(Bg, max(nmax * (nmax + 1) // 2, 1), **f64)
        g, delta = torch.zeros(Bg, max(nmax, 1), **f64), torch.zeros(Bg, max(nmax, 1), **f64)
        L.check(L.lib().sfmi_pg_optimize_f64(L.ptr(self.nod), L.ptr(self.eod), Bg, self.max_s, L.ptr(X), L.ptr(src), L.ptr(tgt),
                                             L.ptr(T), L.ptr(Lam), L.ptr(unc), L.ptr(alive), L.ptr(mu), max_iter, tol, L.ptr(l),
                                             L.ptr(cost), L.ptr(it), L.ptr(status), L.ptr(ework), L.ptr(H), L.ptr(g), L.ptr(delta), L.ptr(lam),
                                             L.stream_ptr()), "sfmi_pg_optimize_f64")
        return X, l[:E], cost, it, status, dict(H=H, g=g[:, :nmax], delta=delta[:, :nmax], lam=lam)


def _graph_opts(what, max_iter, tol):
    max_iter = check_count(max_iter, what, "max_iter", 0)
    return max_iter, check_nonneg(tol, what, "tol")


def pose_graph_optimize_dev(nodes, src, tgt, transforms, infos, uncertain=None, alive=None, n_off=None, e_off=None, mu=0.0, max_iter=100,
                            tol=1e-10, details=False):
    """Levenberg-Marquardt over a ragged batch of pose graphs, one workgroup per graph, the whole loop in one launch.

    nodes (S,4,4) / (S,3,4) / (S,12) f64: the starting poses, scan frame -> frame of the graph's node 0 (which is held fixed); src, tgt
    (E,) integers: node indices local to the edge's graph; transforms (E,4,4): p_tgt = T p_src; infos (E,6,6) f64 information matrices;
    uncertain (E,): loop closures, which the line process may switch off; alive (E,): None = all.  n_off / e_off: (Bg+1,) offsets of
    the graphs' nodes and edges (None: one graph); between 1 and 32 nodes and at most 496 edges per graph: a graph without nodes raises
    SfmiError (node 0 is the frame of the result), one node without edges comes back as given (0 iterations).  transforms and infos
    are HIP tensors; the rest may be host arrays.  mu: the line-process weight, one number, one per graph or a (Bg,) device tensor; <= 0: off.
    The residual, the Jacobians, the line process and the loop are include/sfmi.h's (numpy: tests/posegraph_ref.py).
    -> poses (S,4,4) f64, l (E,) f64 the line-process weights under them (1 for certain edges), cost (Bg,), iterations (Bg,), status
    (Bg,) int32 (the module's table), all on the device; with `details` a dict(H, g, delta, lam) of the last solve follows.  A graph's
    result depends on that graph alone and is bit-identical from run to run."""
    what = "pose_graph_optimize_dev"
    G = _Graph(what, nodes, src, tgt, transforms, infos, uncertain, alive, n_off, e_off)
    max_iter, tol = _graph_opts(what, max_iter, tol)
    if isinstance(mu, torch.Tensor):
        if tuple(mu.shape) != (G.Bg,):
            raise L.SfmiError(f"{what}: mu must be one number, one per graph or a ({G.Bg},) tensor")
    else:
        mu = np.asarray(_per_pair(mu, G.Bg, what, "mu", lambda v: float(v) if isinstance(v, (int, float, np.integer, np.floating)) and
                                  not isinstance(v, bool) and np.isfinite(v) else None, "a finite number"), np.float64)
    dev = G.to_device()
    mu = (mu if isinstance(mu, torch.Tensor) else torch.from_numpy(mu)).to(dev).to(torch.float64).contiguous()
    X, l, cost, it, status, more = G.run(G.X, G.alive, mu, max_iter, tol)
    out = (_pose44(X), l, cost, it, status)
    return out + (more,) if details else out


def global_optimization_dev(nodes, src, tgt, transforms, infos, uncertain=None, alive=None, n_off=None, e_off=None, preference=2.0,
                            max_dist=None, prune=0.25, max_iter=100, tol=1e-10):
    """Open3D's global_optimization in its two passes, on pose_graph_optimize_dev's arguments.  Pass one runs the line process with mu =
    preference x the mean over the graph's alive edges of infos[e,5,5] (the inlier count) x max_dist^2; then alive &= l >= prune on the
    uncertain edges; pass two runs without the line process from pass one's poses.
    -> poses (S,4,4) f64, kept (E,) bool, l (E,) f64 of pass one, status1 (Bg,), status2 (Bg,) int32, on the device."""
    what = "global_optimization_dev"
    G = _Graph(what, nodes, src, tgt, transforms, infos, uncertain, alive, n_off, e_off)
    max_iter, tol = _graph_opts(what, max_iter, tol)
    prune = _check_unit(prune, what, "prune")
    preference = check_nonneg(preference, what, "preference")
    md2 = check_nonneg(max_dist, what, "max_dist") ** 2
    G.to_device()
    w = torch.where(G.alive != 0, G.Lam[:, 35], torch.zeros_like(G.Lam[:, 35]))
    tot = excl_at(torch.cumsum(w, 0), G.eod)
    cnt = excl_at(torch.cumsum((G.alive != 0).to(torch.float64), 0), G.eod)
    tot, cnt = tot[1:] - tot[:-1], cnt[1:] - cnt[:-1]
    mu = torch.where(cnt > 0, preference * (tot / cnt.clamp(min=1)) * md2, torch.zeros_like(tot)).contiguous()
    X1, l1, _, _, st1, _ = G.run(G.X, G.alive, mu, max_iter, tol)
    kept = ((G.alive != 0) & ~((G.unc != 0) & (l1 < prune)))
    X2, _, _, _, st2, _ = G.run(X1, kept.to(torch.int32).contiguous(), torch.zeros_like(mu), max_iter, tol)
    return _pose44(X2), kept, l1, st1, st2


def _scans_arg(clouds, offs, what):
    """a list of (n_i,3) HIP tensors, or (N,3) points with (S+1,) offsets -> points (N,3) f32 contiguous, host offsets"""
    if isinstance(clouds, (list, tuple)):
        if offs is not None or not clouds:
            raise L.SfmiError(f"{what}: a non-empty list of clouds takes no offsets")
        parts = [points_arg(c, what) for c in clouds]
        if any(c.dim() != 2 for c in parts):
            raise L.SfmiError(f"{what}: every cloud must be (n,3)")
        return parts, np.concatenate([[0], np.cumsum([c.shape[0] for c in parts])]).astype(np.int64)
    x = points_arg(clouds, what)
    if x.dim() != 2:
        raise L.SfmiError(f"{what}: expected a list of (n,3) clouds or (N,3) points with offsets")
    return [x], host_offsets(offs, x.shape[0], f"{what} offs")


def _walk(S, edges, T):
    """node poses by walking the edges breadth-first from scan 0.  edges: (i, j) with T (12,) taking scan j's frame to scan i's
    -> X (S,12) f64, reached (S,) bool"""
    def mul(a, b):
        A, B = a.reshape(3, 4), b.reshape(3, 4)
        return np.concatenate([A[:, :3] @ B[:, :3], (A[:, :3] @ B[:, 3] + A[:, 3])[:, None]], 1).reshape(12)

    def inv(a):
        A = a.reshape(3, 4)
        return np.concatenate([A[:, :3].T, -(A[:, :3].T @ A[:, 3])[:, None]], 1).reshape(12)

    X = _identity_poses(S)
    seen, queue = np.zeros(S, bool), [0]
    seen[0] = True
    while queue:
        a = queue.pop(0)
        for k, (i, j) in enumerate(edges):
            if i == a and not seen[j]:
                X[j], seen[j] = mul(X[i], T[k]), True
                queue.append(j)
            elif j == a and not seen[i]:
                X[i], seen[i] = mul(X[j], inv(T[k])), True
                queue.append(i)
    return X, seen


def multiway_registration_dev(clouds, offs=None, pairs=None, max_dists=(0.05, 0.01), metric="point", min_fitness=0.1, preference=2.0,
                              prune=0.25, global_init=None, normals_k=16, graph_max_iter=100, graph_tol=1e-10, **icp):
    """Several partial scans of one object brought into the frame of scan 0 through a pose graph (Open3D's multiway registration), for
    captures in which not every scan overlaps scan 0.

    clouds: a list of (n_i,3) HIP tensors, or one (N,3) tensor with (S+1,) offsets `offs`; at most 32 scans.  Edges: all pairs i < j, or
    `pairs` (a list of (i, j), i < j); the source is scan j and the target scan i.  Every edge is registered in ONE batch by consecutive
    icp_dev(**icp) stages, one per entry of max_dists, each from the last stage's pose (the first from the identity or, with
    global_init = a dict of global_registration_dev's arguments, from the global pose of the pairs whose global status is 0); the plane
    metric takes its normals from scan.estimate_normals_dev(k=normals_k).  An edge is dropped if a stage ends with status >= 2 or its
    fitness under the last max_dist is below min_fitness.  Edges j = i + 1 are certain, the rest uncertain.  information_matrix_dev at the
    last max_dist weighs the edges; the node poses start from a breadth-first walk over the kept edges from scan 0 (on the host: the kept
    mask and the edges' (P,12) poses are read back) and are refined by global_optimization_dev(preference, max_dist = the last stage's,
    prune).  A scan that no kept edge reaches is reported with status 2 and keeps the identity.
    -> poses (S,4,4) f64 on the device, status (S,) host int32 (0, or 2, or the optimiser's status >= 2 for every reached scan), and a
    dict: edges (P,2) host, transforms (P,4,4), fitness (P,), information (P,6,6), l (P,) on the device, registered (P,) / kept (P,) host
    bool (the edge entered the graph / survived the pruning), icp_status (P,) host, graph_status (pass one, pass two), chain (S,4,4)
    the breadth-first start."""
    from .scan import estimate_normals_dev
    what = "multiway_registration_dev"
    parts, o = _scans_arg(clouds, offs, what)
    S = len(o) - 1
    if not 1 <= S <= PG_MAX_NODES:
        raise L.SfmiError(f"{what}: between 1 and {PG_MAX_NODES} scans, got {S}")
    if pairs is None:
        pairs = [(i, j) for i in range(S) for j in range(i + 1, S)]
    else:
        try:
            pairs = [(int(i), int(j)) for i, j in pairs]
        except (TypeError, ValueError):
            raise L.SfmiError(f"{what}: pairs must be a list of (i, j) scan indices") from None
        if any(not 0 <= i < j < S for i, j in pairs) or len(set(pairs)) != len(pairs):
            raise L.SfmiError(f"{what}: pairs must be distinct (i, j) with 0 <= i < j < {S}")
    if len(pairs) > PG_MAX_EDGES:
        raise L.SfmiError(f"{what}: at most {PG_MAX_EDGES} pairs")
    try:
        max_dists = list(max_dists)
    except TypeError:
        max_dists = []
    if not max_dists:
        raise L.SfmiError(f"{what}: max_dists must be a non-empty sequence, one max_dist per ICP stage")
    for m in max_dists:
        check_nonneg(m, what, "max_dists")
    if metric not in METRICS:
        raise L.SfmiError(f"{what}: metric must be one of {METRICS}, got {metric!r}")
    min_fitness = _check_unit(min_fitness, what, "min_fitness")
    prune = _check_unit(prune, what, "prune")
    preference = check_nonneg(preference, what, "preference")
    graph_max_iter, graph_tol = _graph_opts(what, graph_max_iter, graph_tol)
    bad_kw = set(icp) - {"max_iter", "rel_fitness", "rel_rmse", "check_every"}
    if bad_kw:
        raise L.SfmiError(f"{what}: unknown arguments {sorted(bad_kw)}")
    if global_init is not None and not isinstance(global_init, dict):
        raise L.SfmiError(f"{what}: global_init must be a dict of global_registration_dev arguments")
    dev = on_device(what, *parts)
    x = (torch.cat([c.float() for c in parts]) if len(parts) > 1 else parts[0].float()).contiguous()
    P = len(pairs)
    poses = torch.eye(4, device=dev, dtype=torch.float64).repeat(S, 1, 1)
    status = np.zeros(S, np.int32)
    edges = np.array(pairs, np.int64).reshape(P, 2)
    more = dict(edges=edges, transforms=poses[:0], fitness=poses.new_zeros(0), information=poses.new_zeros(0, 6, 6), l=poses.new_zeros(0),
                registered=np.zeros(P, bool), kept=np.zeros(P, bool), icp_status=np.zeros(P, np.int32), graph_status=(0, 0), chain=poses.clone())
    if P == 0:
        status[1:] = 2
        return poses, status, more
    scan = [x[int(o[i]):int(o[i + 1])] for i in range(S)]
    src, tgt = torch.cat([scan[j] for _, j in pairs]), torch.cat([scan[i] for i, _ in pairs])
    so = np.concatenate([[0], np.cumsum([scan[j].shape[0] for _, j in pairs])]).astype(np.int64)
    to = np.concatenate([[0], np.cumsum([scan[i].shape[0] for i, _ in pairs])]).astype(np.int64)
    nrm = None
    if metric == "plane":
        n_all = estimate_normals_dev(x, o, normals_k)[0]
        nrm = torch.cat([n_all[int(o[i]):int(o[i + 1])] for i, _ in pairs])
    pose = torch.eye(4, device=dev, dtype=torch.float64).repeat(P, 1, 1)
    if global_init is not None:
        g = global_registration_dev(src, tgt, so, to, **global_init)
        pose = torch.where((g[6] < 1)[:, None, None], g[0], pose)
    dead = torch.zeros(P, device=dev, dtype=torch.bool)
    st = None
    for md in max_dists:                                       # a pair that has failed keeps its pose: the stages that follow do not count
        new, _, _, _, st = icp_dev(src, tgt, so, to, md, metric, nrm, pose, **icp)
        pose = torch.where(dead[:, None, None], pose, new)
        dead |= st >= 2
    ev = _Icp(what, src, tgt, so, to, max_dists[-1], "point", None, pose, "pose")
    ev.iterate(0, True)
    info, _, _ = _information(ev)
    ok = (~dead) & (ev.fitness >= min_fitness)
    ok_h, st_h, T_h = ok.cpu().numpy(), st.cpu().numpy(), ev.pose.cpu().numpy()      # the read-back: (P,) masks and (P,12) poses
    reg = [k for k in range(P) if ok_h[k]]
    X0, seen = _walk(S, [pairs[k] for k in reg], T_h[reg])
    node = np.cumsum(seen) - 1
    keep = [k for k in reg if seen[pairs[k][0]] and seen[pairs[k][1]]]
    status[~seen] = 2
    chain = torch.from_numpy(X0).to(dev)
    poses = _pose44(chain)
    l_all, kept_h, gs = torch.zeros(P, device=dev, dtype=torch.float64), np.zeros(P, bool), (0, 0)
    if keep:
        kd = torch.from_numpy(np.array(keep, np.int64)).to(dev)
        gsrc, gtgt = np.array([node[pairs[k][1]] for k in keep]), np.array([node[pairs[k][0]] for k in keep])
        unc = np.array([pairs[k][1] != pairs[k][0] + 1 for k in keep], np.int32)
        sd = torch.from_numpy(np.nonzero(seen)[0]).to(dev)
        X, kept, l1, s1, s2 = global_optimization_dev(chain[sd], gsrc, gtgt, ev.pose[kd], info[kd], unc, None, None, None, preference,
                                                      max_dists[-1], prune, graph_max_iter, graph_tol)
        poses[sd] = X
        l_all[kd] = l1
        kept_h[keep] = kept.cpu().numpy()
        gs = (int(s1.cpu()[0]), int(s2.cpu()[0]))
        if gs[1] >= 2:
            status[seen] = gs[1]
    more.update(transforms=_pose44(ev.pose), fitness=ev.fitness, information=info, l=l_all, kept=kept_h, icp_status=st_h, graph_status=gs,
                chain=_pose44(chain))
    more["registered"][keep] = True
    return poses, status, more
