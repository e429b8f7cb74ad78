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

status: 0 converged, 1 max_iter reached, 2 fewer than 3 (point) / 6 (plane) inliers, 3 the normal equations are not positive definite,
4 a non-finite coordinate, normal or initial pose in the pair.  With 2, 3 and 4 the pose stays where it was.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L
from ._ragged import host_offsets, on_device, point_sets, points_arg

METRICS = ("point", "plane")
N_SUMS = 29


def _pose_arg(pose, B, what, name="pose"):
    """None (identity), (B,4,4), (B,3,4), (B,12) or, for one pair, (4,4) / (3,4) / (12,) -> (B,12) f64 numpy or torch tensor"""
    if pose is None:
        return np.tile(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float64), (B, 1))
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


def _check_max_dist(v, what, name="max_dist"):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not 0 <= float(v) < float("inf"):
        raise L.SfmiError(f"{what}: {name} must be a finite number >= 0, got {v!r}")
    return float(v)


def _per_pair(v, B, what, name, conv, expect):
    """one value for every pair, or a list / tuple of B values -> a list of B converted values"""
    vals = list(v) if isinstance(v, (list, tuple)) else [v] * B
    if len(vals) != B:
        raise L.SfmiError(f"{what}: {name} must be one value or one per pair ({B}), got {len(vals)}")
    out = [conv(x) for x in vals]
    if any(x is None for x in out):
        raise L.SfmiError(f"{what}: {name} must be {expect}, got {v!r}")
    return out


def _check_int(v, what, name, lo):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) < 2 ** 31:
        raise L.SfmiError(f"{what}: {name} must be an integer in [{lo}, 2^31), got {v!r}")
    return int(v)


def _check_tol(v, what, name):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not float(v) >= 0:
        raise L.SfmiError(f"{what}: {name} must be a number >= 0, got {v!r}")
    return float(v)


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
        pd, od = _pose_dev(p, dev), torch.from_numpy(o).to(dev)
        L.check(L.lib().sfmi_icp_transform_f32(L.ptr(xf), L.ptr(od), L.ptr(pd), B, N, L.ptr(out), L.stream_ptr()), "sfmi_icp_transform_f32")
    return out.reshape(*shape, 3) if shape else out


class _Icp:
    """The device state of one call: validated arguments, the pose and the per-pair outputs; `iterate` runs one iteration."""

    def __init__(self, what, source, target, s_off, t_off, max_dist, metric, target_normals, init, pose_name="init"):
        s, t = points_arg(source, f"{what} source"), points_arg(target, f"{what} target")
        if s.dim() == 3 or t.dim() == 3:
            if s.dim() != 3 or t.dim() != 3 or s.shape[0] != t.shape[0] or s_off is not None or t_off is not None:
                raise L.SfmiError(f"{what}: batched (B,N,3) sources need a (B,M,3) target of the same B and no offsets")
            B = s.shape[0]
            so, to = np.arange(B + 1, dtype=np.int64) * s.shape[1], np.arange(B + 1, dtype=np.int64) * t.shape[1]
        else:
            so, to = host_offsets(s_off, s.shape[0], f"{what} s_off"), host_offsets(t_off, t.shape[0], f"{what} t_off")
            if len(so) != len(to):
                raise L.SfmiError(f"{what}: source has {len(so) - 1} sets, target has {len(to) - 1}")
        B = len(so) - 1
        if B < 1:
            raise L.SfmiError(f"{what}: expected at least one pair")
        if B > 65535 or (np.diff(so) >= 2 ** 31).any() or (np.diff(to) >= 2 ** 31).any():
            raise L.SfmiError(f"{what}: at most 65535 pairs, every set below 2^31 points")
        s, t = s.reshape(-1, 3), t.reshape(-1, 3)
        metrics = _per_pair(metric, B, what, "metric", lambda m: m if isinstance(m, str) and m in METRICS else None,
                            f"one of {METRICS}")
        dists = _per_pair(max_dist, B, what, "max_dist", lambda v: _check_max_dist(v, what), "a finite number >= 0")
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
        self.sod, self.tod = torch.from_numpy(so).to(dev), torch.from_numpy(to).to(dev)
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
    non-finite coordinate or pose keeps idx = -1, d2 = +inf."""
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
    max_iter = _check_int(max_iter, what, "max_iter", 0)
    check_every = _check_int(check_every, what, "check_every", 1)
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
        _check_max_dist(m, what, "max_dists")
    s, so, _ = point_sets(source, s_off, f"{what} source")
    t, to, _ = point_sets(target, t_off, f"{what} target")
    if len(so) != len(to):
        raise L.SfmiError(f"{what}: source has {len(so) - 1} sets, target has {len(to) - 1}")
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


def merge_scans_dev(clouds, offs=None, voxel=None, **icp):
    """Several partial scans of one object, each in its own frame, merged in the frame of scan 0.

    clouds: a list of (n_i,3) HIP tensors, or one (N,3) tensor with (S+1,) offsets `offs`.  Scans 1.. are registered onto scan 0 in one
    batch - icp_dev(**icp), or icp_multiscale_dev when `voxels` is among the keyword arguments - and transformed; the clouds are
    concatenated in scan order and, with `voxel`, reduced by scan.voxel_downsample_dev.  A scan whose status is >= 2 is left out and
    reported.  -> merged (K,3) f32, poses (S,4,4) f64 (identity for scan 0), status (S,) host int32 (0 for scan 0).  The statuses are
    read back (one synchronisation)."""
    from .scan import voxel_downsample_dev
    what = "merge_scans_dev"
    if voxel is not None and not (isinstance(voxel, (int, float, np.integer, np.floating)) and not isinstance(voxel, bool) and 0 < float(voxel) < float("inf")):
        raise L.SfmiError(f"{what}: voxel must be a finite number > 0, got {voxel!r}")
    if isinstance(clouds, (list, tuple)):
        if offs is not None or not clouds:
            raise L.SfmiError(f"{what}: a non-empty list of clouds takes no offsets")
        parts = [points_arg(c, what) for c in clouds]
        if any(c.dim() != 2 for c in parts):
            raise L.SfmiError(f"{what}: every cloud must be (n,3)")
        o = np.concatenate([[0], np.cumsum([c.shape[0] for c in parts])]).astype(np.int64)
        on_device(what, *parts)
        x = torch.cat([c.float() for c in parts]).contiguous()
    else:
        x = points_arg(clouds, what)
        if x.dim() != 2:
            raise L.SfmiError(f"{what}: expected a list of (n,3) clouds or (N,3) points with offsets")
        o = host_offsets(offs, x.shape[0], f"{what} offs")
        on_device(what, x)
        x = x.float().contiguous()
    S, dev = len(o) - 1, x.device
    poses = torch.eye(4, device=dev, dtype=torch.float64).repeat(S, 1, 1)
    status = np.zeros(S, np.int32)
    first = x[:int(o[1])]
    if S > 1:
        src, so = x[int(o[1]):], o[1:] - o[1]
        tgt, to = first.repeat(S - 1, 1), np.arange(S, dtype=np.int64) * first.shape[0]
        run = icp_multiscale_dev if "voxels" in icp else icp_dev
        pose, _, _, _, st = run(src, tgt, so, to, **icp)
        poses[1:] = pose
        status[1:] = st.cpu().numpy()
        moved = transform_points_dev(src, so, pose)
        keep = [first] + [moved[int(so[i]):int(so[i + 1])] for i in range(S - 1) if status[i + 1] < 2]
        merged = torch.cat(keep)
    else:
        merged = first
    if voxel is not None and merged.shape[0]:
        merged = voxel_downsample_dev(merged, None, float(voxel))[0]
    return merged, poses, status
