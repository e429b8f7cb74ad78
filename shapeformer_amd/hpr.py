"""Hidden-point removal and virtual scans on the device — host side of csrc/hpr.hip.

The reference makes every partial cloud of its transformer training set with VirtualScanSelector (shapeformer/data/partial.py:
127-146): hidden-point removal (xgutils/geoutil.py:58-74, Katz et al.: flip the cloud about a huge sphere around the camera, keep the
vertices of the convex hull) with scipy's qhull on the host.  Here the same operator runs on the device, on the clouds the datasets
store: the flip in f64 in numpy's operation order, then hull-vertex membership of every point as a 2-D linear program (one wave per
point; this module hands the kernel a Morton order of the viewing directions to take the constraints in).  There is no CPU fallback.

  hidden_point_mask_dev(points, cams, off=None, param=pi) -> visible (uint8), count (B,), status (B,)
  hidden_point_removal(cloud, campos)                     -> the reference's signature: numpy rows, ascending index order
  virtual_scan_dev(X, context_N, radius, noise, seed, cams) -> Xct (B, context_N, 3) f32, cams (B,3) f64, count (B,)

Exact duplicate points: the lowest index of a class of bitwise-equal points represents it (qhull reports one arbitrary member).
status per shape: 0 ok, 1 fewer than 4 points, 2 a non-finite coordinate, 3 a point at the camera (mask all zero).
The resample and jitter draws are counter hashes of (seed, shape index, row): they touch no global RNG, and a batch equals per-shape
calls (`shape0` names the index of the first shape).  Ragged batches and their argument checks are _ragged.py's.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L
from . import _ragged
from ._ragged import on_device, point_sets


def _cams(cams, B, what):
    c = cams.detach().cpu().numpy() if isinstance(cams, torch.Tensor) else np.asarray(cams)
    c = np.asarray(c, np.float64)
    if c.shape == (3,) and B == 1:
        c = c[None]
    if c.shape != (B, 3):
        raise L.SfmiError(f"{what}: expected ({B},3) cameras, got {tuple(c.shape)}")
    return np.ascontiguousarray(c)


def _prepare(points, cams, off, what):
    """-> (flat (N,3) f32 / f64 contiguous device tensor, host offsets, host cameras (B,3) f64, batch shape or None)."""
    x, o, shape = point_sets(points, off, what)
    c = _cams(cams, len(o) - 1, what)
    on_device(what, x)
    if x.dtype not in (torch.float32, torch.float64):
        x = x.float()
    return x.contiguous(), o, c, shape


def _spread16(v):
    """the 16 low bits of an int64 tensor spread to the even bit positions (Morton interleave)"""
    v = (v | (v << 8)) & 0x00FF00FF
    v = (v | (v << 4)) & 0x0F0F0F0F
    v = (v | (v << 2)) & 0x33333333
    return (v | (v << 1)) & 0x55555555


def constraint_order_dev(x, o, c):
    """The order in which csrc/hpr.hip takes each point's constraints: per shape a permutation of its local indices (int32, (N,)) that
    sorts the points by the Morton code of their viewing direction (x - cam) / |x - cam|, taken in two tangent coordinates of the
    camera axis at 16 bits each, so that neighbours in the order lie on nearby view rays.  Stable, and a function of the shape and its
    camera only: the members of a class of equal points stay in index order and a batch orders a shape as a single call does.
    Performance only: visibility does not depend on it."""
    dev, B = x.device, len(o) - 1
    n = torch.from_numpy(np.diff(o)).to(dev)
    shape = torch.repeat_interleave(torch.arange(B, device=dev), n)
    axis = -c / np.maximum(np.linalg.norm(c, axis=1, keepdims=True), 1e-300)
    e = np.zeros_like(axis)
    e[np.arange(B), np.argmin(np.abs(axis), axis=1)] = 1.0
    t1 = np.cross(axis, e)
    t1 /= np.maximum(np.linalg.norm(t1, axis=1, keepdims=True), 1e-300)
    t2 = np.cross(axis, t1)
    cd, t1d, t2d = (torch.from_numpy(np.ascontiguousarray(a)).to(dev)[shape] for a in (c, t1, t2))
    d = x.double() - cd
    d = d / d.norm(dim=1, keepdim=True).clamp_min(1e-300)
    uv = [torch.nan_to_num((d * t).sum(1), nan=0.0).clamp(-1.0, 1.0) for t in (t1d, t2d)]
    lo = [torch.full((B,), 2.0, device=dev, dtype=torch.float64).scatter_reduce(0, shape, u, "amin") for u in uv]
    hi = [torch.full((B,), -2.0, device=dev, dtype=torch.float64).scatter_reduce(0, shape, u, "amax") for u in uv]
    span = torch.maximum(hi[0] - lo[0], hi[1] - lo[1]).clamp_min(1e-300)[shape]         # one scale for both: square cells
    key = shape.long() << 32
    for k in range(2):
        q = ((uv[k] - lo[k][shape]) / span * 65535.0).floor().clamp(0, 65535).long()
        key = key | (_spread16(q) << k)
    perm = torch.sort(key, stable=True).indices
    return (perm - torch.from_numpy(o[:-1]).to(dev)[shape]).to(torch.int32).contiguous()


def hidden_point_mask_dev(points, cams, off=None, param=np.pi, _evals=None, _index_order=False):
    """Which points each camera sees.  points: (B,N,3), or ragged (N,3) with (B+1,) exclusive offsets `off` (None: one shape), f32 or
    f64 HIP tensor; cams: (B,3) camera positions (numpy or tensor; used in f64).  -> visible uint8 (B,N) / (N,), count (B,) int32,
    status (B,) int32 on the device (include/sfmi.h; an empty shape has count 0).  A shape's mask depends on that shape and its camera
    alone.  A non-HIP tensor raises SfmiError before any launch."""
    x, o, c, shape = _prepare(points, cams, off, "hidden_point_mask_dev")
    dev, B, N = x.device, len(o) - 1, x.shape[0]
    lib = L.lib()
    vis = torch.empty(N, device=dev, dtype=torch.uint8)
    count = torch.empty(B, device=dev, dtype=torch.int32)
    status = torch.empty(B, device=dev, dtype=torch.int32)
    od, cd = torch.from_numpy(o).to(dev), torch.from_numpy(c).to(dev)
    order = constraint_order_dev(x, o, c) if N > 0 and not _index_order else None   # None: index order (tools/kbench_hpr.py's A/B)
    ws = _ragged.workspace(lib.sfmi_hpr_workspace_bytes(B, N), dev)
    if _evals is not None:
        _evals.append(torch.empty(N, 2, device=dev, dtype=torch.int32))
    L.check(lib.sfmi_hpr_visible(L.ptr(x), int(x.dtype == torch.float64), L.ptr(od), L.ptr(cd), L.ptr(order), B, N, float(param), L.ptr(vis),
                                 L.ptr(count), L.ptr(status), L.ptr(_evals[-1]) if _evals is not None else None, L.ptr(ws),
                                 L.stream_ptr()), "sfmi_hpr_visible")
    return (vis.reshape(shape) if shape else vis), count, status


def constraint_evaluations_dev(points, cams, off=None, param=np.pi, index_order=False):
    """(N,2) int32: how many constraints the kernel evaluated for each point, in the scan and in the re-solves (tools/kbench_hpr.py)."""
    ev = []
    hidden_point_mask_dev(points, cams, off, param, _evals=ev, _index_order=index_order)
    return ev[0]


def hidden_point_removal(cloud, campos, device="cuda"):
    """geoutil.hidden_point_removal(cloud, campos): numpy (N,3) in, the visible rows out, in ascending index order with one row per
    class of duplicate points (the reference returns hull.vertices order, which is ascending too)."""
    cloud = np.asarray(cloud)
    x = torch.from_numpy(np.ascontiguousarray(cloud if cloud.dtype in (np.float32, np.float64) else cloud.astype(np.float64)))
    vis, _, _ = hidden_point_mask_dev(x.to(device), np.asarray(campos, np.float64).reshape(1, 3))
    return cloud[vis.cpu().numpy().astype(bool)]


def sample_cameras(B, radius=10, seed=0, shape0=0):
    """Camera b = radius * a unit normal direction from np.random.RandomState([seed, shape0 + b]) (f64): shape b's camera depends on
    (seed, shape index) only."""
    v = np.stack([np.random.RandomState([int(seed) & 0xFFFFFFFF, shape0 + b]).randn(3) for b in range(B)])
    return v / np.linalg.norm(v, axis=1, keepdims=True) * radius


def resample_visible_dev(x, o, visible, count, context_N, noise=0., seed=0, shape0=0):
    """x (N,3) flat device tensor, o host offsets, visible (N,) uint8, count (B,) int32 -> (B, context_N, 3) f32 (csrc/hpr.hip).
    A shape without points gives NaN rows.  x: f32 or f64 of any layout (another dtype is read as f32), visible: N bytes, booleans or
    integers (non-zero: visible), count: B integers; tensors that already have the kernel's dtype and layout are used as they are."""
    what = "resample_visible_dev"
    x = _ragged.points_arg(x, what)
    if x.dim() != 2:
        raise L.SfmiError(f"{what}: expected flat (N,3) points, got {tuple(x.shape)}")
    o = _ragged.host_offsets(o, x.shape[0], f"{what} offsets", empty_ok=True)
    B, N = len(o) - 1, x.shape[0]
    if not isinstance(visible, torch.Tensor) or visible.numel() != N or visible.dtype.is_floating_point:
        raise L.SfmiError(f"{what}: visible must be a tensor of {N} bytes, one per point")
    if not isinstance(count, torch.Tensor) or count.numel() != B or count.dtype.is_floating_point or count.dtype == torch.bool:
        raise L.SfmiError(f"{what}: count must be a tensor of {B} integers, one per shape")
    if context_N < 0 or noise < 0:
        raise L.SfmiError("virtual_scan_dev: context_N and noise must be >= 0")
    dev = on_device(what, x, visible, count)
    x = (x if x.dtype in (torch.float32, torch.float64) else x.float()).contiguous()
    count = count.reshape(-1).to(torch.int32).contiguous()
    out = torch.empty(B, context_N, 3, device=dev, dtype=torch.float32)
    v = visible.reshape(-1)
    v = (v if v.dtype == torch.uint8 else (v != 0).to(torch.uint8)).contiguous()
    prefix = (torch.cumsum(v, 0, dtype=torch.int32) - v).to(torch.int32).contiguous()
    od = torch.from_numpy(o).to(dev)
    L.check(L.lib().sfmi_hpr_resample_f32(L.ptr(x), int(x.dtype == torch.float64), L.ptr(v), L.ptr(prefix), L.ptr(od), L.ptr(count),
                                          B, N, int(context_N), int(seed) & 0xFFFFFFFF, int(shape0), float(noise), L.ptr(out),
                                          L.stream_ptr()), "sfmi_hpr_resample_f32")
    return out


def virtual_scan_dev(X, context_N, radius=10, noise=0., seed=0, cams=None, off=None, shape0=0):
    """VirtualScanSelector on the device: X (B,N,3) (or ragged (N,3) + off) HIP tensor -> Xct (B, context_N, 3) f32 on the device, the
    cameras (B,3) f64 numpy, count (B,) int32 visible points per shape.  cams=None: sample_cameras(B, radius, seed, shape0).
    Row k of shape b is a uniformly drawn visible point of shape b (all points when two or fewer are visible, as the reference falls
    back), plus `noise` * normal jitter clipped to [-1, 1] when noise > 0.  Shape b is seeded by (seed, shape0 + b) only, so shape b of a
    batch equals a single-shape call with shape0 + b.  A shape without points has count 0 and NaN rows."""
    x, o, _, _ = _prepare(X, np.zeros((X.shape[0] if X.dim() == 3 else (1 if off is None else len(off) - 1), 3)), off, "virtual_scan_dev")
    B = len(o) - 1
    c = sample_cameras(B, radius, seed, shape0) if cams is None else _cams(cams, B, "virtual_scan_dev")
    visible, count, _ = hidden_point_mask_dev(x, c, o)
    return resample_visible_dev(x, o, visible, count, context_N, noise, seed, shape0), c, count
