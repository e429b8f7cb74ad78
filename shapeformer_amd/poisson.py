"""Poisson surface reconstruction of oriented point clouds on the device — host side of csrc/poisson.hip.

The step that follows normals: the reference's non-learned baseline mesh is xgutils/geoutil.py:297-342 Open3D_Toolbox.poisson_recon
(kNN normals, Poisson at an octree depth, a density-quantile trim).  Here the same call runs on a uniform lattice in HBM: this is the
interface of that call, not Open3D's octree output, and parity with Open3D is not claimed.

  poisson_splat_dev(points, normals, off, grid_dim, bbox)             -> Vx, Vy, Vz, W, outside
  poisson_rhs_dev(Vx, Vy, Vz)                                         -> rhs (B,R,R,R)
  poisson_solve_dev(rhs, tol, max_iter, check_every)                  -> chi (B,R,R,R), iterations (B,), residual (B,)
  poisson_field_dev(points, normals, off, grid_dim | depth, bbox, tol, max_iter) -> field, W, info
  poisson_sample_dev(lattice, points, off, bbox)                      -> (N,) f32 trilinear samples
  poisson_recon_dev(points, normals, off, depth, quantile, knn, viewpoint, keep_components, ..., orient) -> verts, faces, voff, toff, density
  Open3D_Toolbox().poisson_recon(cloud, normals, viewpoint, depth, quantile, knn, orient) -> (vert float64, face int) numpy

The discrete problem (its numpy statement is tests/poisson_ref.py): R nodes per axis over a cubic box, h = (hi - lo) / (R - 1), axes
those of marching_cubes_dev.  The normals are splatted with trilinear weights onto the lattice's EDGES (Vx (R-1,R,R) at ((i+½),j,k),
Vy, Vz likewise), a density W onto its nodes; every site's sum is taken in f64 in a fixed order (cells ascending, input index ascending
within a cell) and rounded to f32 once.  With G the forward difference from nodes to edges and zeros around the lattice, chi solves
G^T G chi = -G^T V by conjugate gradients (f32 vectors, f64 dot products over a fixed tree).  Normals point OUTWARD (what
estimate_normals_dev(viewpoint=...) and mesh face normals give), so chi is high inside; field = chi - iso with iso the mean of chi over
the set's in-box points is positive inside and marching_cubes_dev(field, 0.0, bbox) meshes it.  Everything is bit-identical from run to
run and a set's result does not depend on the batch around it.

Ragged batches and their checks are _ragged.py's: every refusal is an SfmiError raised on the host before the library
is loaded, where the tensors live is checked last, and there is no CPU fallback.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib as L
from . import _ragged
from ._ragged import host_offsets, offsets_dev, on_device, point_sets, points_arg

MIN_GRID, MAX_GRID = 5, 513
DEFAULT_BBOX = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))


# ---- host checks -----------------------------------------------------------------------------------------------------------

def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _check_grid(grid_dim, depth, what, default=129):
    if grid_dim is not None and depth is not None:
        raise L.SfmiError(f"{what}: give grid_dim or depth, not both")
    if depth is not None:
        if not _is_int(depth) or not 2 <= int(depth) <= 9:
            raise L.SfmiError(f"{what}: depth must be an integer in [2, 9] (grid_dim = 2^depth + 1), got {depth!r}")
        return 2 ** int(depth) + 1
    if grid_dim is None:
        return default
    if not _is_int(grid_dim) or not MIN_GRID <= int(grid_dim) <= MAX_GRID:
        raise L.SfmiError(f"{what}: grid_dim must be an integer in [{MIN_GRID}, {MAX_GRID}], got {grid_dim!r}")
    return int(grid_dim)


def _check_bbox(bbox, what):
    try:
        b = np.asarray(bbox, np.float64)
    except (TypeError, ValueError):
        b = np.zeros(0)
    if b.shape != (2, 3) or not np.isfinite(b).all():
        raise L.SfmiError(f"{what}: bbox must be ((lo x, y, z), (hi x, y, z)) finite numbers, got {bbox!r}")
    ext = b[1] - b[0]
    if not (ext > 0).all():
        raise L.SfmiError(f"{what}: bbox is degenerate (hi must exceed lo on every axis), got {bbox!r}")
    if ext.max() - ext.min() > 1e-9 * ext.max():
        raise L.SfmiError(f"{what}: bbox must be a cube (the lattice has one spacing), got sides {ext.tolist()}")
    return np.ascontiguousarray(b.reshape(6))


def _check_solver(tol, max_iter, check_every, what):
    if isinstance(tol, bool) or not isinstance(tol, (int, float, np.integer, np.floating)) or not 0 < float(tol) < float("inf"):
        raise L.SfmiError(f"{what}: tol must be a finite number > 0, got {tol!r}")
    if max_iter is not None and (not _is_int(max_iter) or int(max_iter) < 0):
        raise L.SfmiError(f"{what}: max_iter must be None or an integer >= 0, got {max_iter!r}")
    if not _is_int(check_every) or int(check_every) < 1:
        raise L.SfmiError(f"{what}: check_every must be an integer >= 1, got {check_every!r}")
    return float(tol), (None if max_iter is None else int(max_iter)), int(check_every)


def _check_quantile(q, what):
    if isinstance(q, bool) or not isinstance(q, (int, float, np.integer, np.floating)) or not 0 <= float(q) < 1:
        raise L.SfmiError(f"{what}: quantile must lie in [0, 1), got {q!r}")
    return float(q)


def _cloud_args(points, normals, off, what):
    """-> (points (N,3), normals (N,3) or None, host offsets); the normals have the points' shape"""
    x, o, _ = point_sets(points, off, what)
    n = None
    if normals is not None:
        nn = points_arg(normals, f"{what} normals")
        if tuple(nn.shape) != tuple(points.shape):
            raise L.SfmiError(f"{what}: normals {tuple(nn.shape)} must have the shape of the points {tuple(points.shape)}")
        n = nn.reshape(-1, 3)
    if x.shape[0] >= 2 ** 31:
        raise L.SfmiError(f"{what}: the batch has 2^31 points or more")
    return x, n, o


def _check_size(B, R, what):
    if B < 1 or B > 65535 or B * R ** 3 >= 2 ** 31:
        raise L.SfmiError(f"{what}: {B} lattices of {R}^3 nodes: the batch must hold 1 .. 65535 shapes and fewer than 2^31 nodes")


def _lattice_arg(t, what):
    if not isinstance(t, torch.Tensor) or t.dim() != 4 or not (t.shape[1] == t.shape[2] == t.shape[3]):
        raise L.SfmiError(f"{what}: expected a (B,R,R,R) torch tensor on the HIP device (no CPU fallback)")
    if not MIN_GRID <= t.shape[1] <= MAX_GRID:
        raise L.SfmiError(f"{what}: the lattice must have {MIN_GRID} .. {MAX_GRID} nodes per axis, got {t.shape[1]}")
    _check_size(t.shape[0], t.shape[1], what)
    return t


# ---- the stages ------------------------------------------------------------------------------------------------------------

def _splat(xf, nf, o, R, box):
    """checked, contiguous f32 device arrays -> Vx, Vy, Vz, W, outside"""
    lib, st, dev = L.lib(), L.stream_ptr, xf.device
    B, N, C = len(o) - 1, xf.shape[0], R - 1
    od = offsets_dev(o, dev)
    f32 = dict(device=dev, dtype=torch.float32)
    Vx, Vy, Vz = torch.empty(B, C, R, R, **f32), torch.empty(B, R, C, R, **f32), torch.empty(B, R, R, C, **f32)
    W = torch.empty(B, R, R, R, **f32)
    outside = torch.empty(B, device=dev, dtype=torch.int32)
    status = torch.empty(1, device=dev, dtype=torch.int32)
    keys = torch.empty(max(N, 1), device=dev, dtype=torch.int64)
    L.check(lib.sfmi_poisson_keys_f32(L.ptr(xf), L.ptr(nf), L.ptr(od), B, N, R, L.ptr(box), L.ptr(keys), L.ptr(outside), L.ptr(status),
                                      st()), "sfmi_poisson_keys_f32")
    if int(status.cpu()[0]):                                                   # the read-back
        raise L.SfmiError("poisson_splat_dev: a coordinate or a normal is not finite")
    s = torch.sort(keys[:N], stable=True)                                      # the order of every sum: cells, then input index
    order, cstart = s.indices, torch.empty(B * C ** 3 + 1, device=dev, dtype=torch.int32)
    L.check(lib.sfmi_poisson_cells_i32(L.ptr(s.values), B, N, R, L.ptr(cstart), st()), "sfmi_poisson_cells_i32")
    L.check(lib.sfmi_poisson_splat_f32(L.ptr(xf), L.ptr(nf), L.ptr(order), L.ptr(cstart), B, N, R, L.ptr(box), L.ptr(Vx), L.ptr(Vy),
                                       L.ptr(Vz), L.ptr(W), st()), "sfmi_poisson_splat_f32")
    return Vx, Vy, Vz, W, outside


def poisson_splat_dev(points, normals, off=None, grid_dim=129, bbox=DEFAULT_BBOX):
    """The staggered vector field and the density of a ragged batch of oriented clouds.

    points, normals (N,3) f32 HIP tensors with (B+1,) offsets (None: one set), or (B,M,3) batches.  -> Vx (B,R-1,R,R), Vy (B,R,R-1,R),
    Vz (B,R,R,R-1), W (B,R,R,R) f32 and outside (B,) int32 on the device.  Each point adds n_x w to the 8 Vx sites around it, w the
    trilinear weight on the lattice shifted by half a cell along x (Vy, Vz likewise), and the plain trilinear weights to the 8 nodes
    of W; weights on sites outside the arrays are dropped.  Weights are f64 from the f32 inputs; each site's sum is f64 in a fixed
    order (cells ascending, input index ascending within a cell), rounded to f32 once: bit-identical from run to run and independent
    of the batch around the set.  A point outside the closed box is ignored and counted in `outside`.
    Raises SfmiError after the read-back for a non-finite coordinate or normal."""
    what = "poisson_splat_dev"
    R = _check_grid(grid_dim, None, what)
    box = _check_bbox(bbox, what)
    if normals is None:
        raise L.SfmiError(f"{what}: normals are required")
    x, n, o = _cloud_args(points, normals, off, what)
    _check_size(len(o) - 1, R, what)
    on_device(what, x, n)
    return _splat(x.float().contiguous(), n.float().contiguous(), o, R, box)


def poisson_rhs_dev(Vx, Vy, Vz):
    """rhs (B,R,R,R) = -G^T V: ((Vx[i] - Vx[i-1]) + (Vy[j] - Vy[j-1])) + (Vz[k] - Vz[k-1]) in f64, sites outside the arrays zero."""
    what = "poisson_rhs_dev"
    if not all(isinstance(t, torch.Tensor) and t.dim() == 4 for t in (Vx, Vy, Vz)):
        raise L.SfmiError(f"{what}: expected three 4-D torch tensors on the HIP device (no CPU fallback)")
    B, R = Vy.shape[0], Vy.shape[1]
    if tuple(Vx.shape) != (B, R - 1, R, R) or tuple(Vy.shape) != (B, R, R - 1, R) or tuple(Vz.shape) != (B, R, R, R - 1):
        raise L.SfmiError(f"{what}: expected Vx (B,R-1,R,R), Vy (B,R,R-1,R), Vz (B,R,R,R-1), got {tuple(Vx.shape)}, {tuple(Vy.shape)}, "
                          f"{tuple(Vz.shape)}")
    if not MIN_GRID <= R <= MAX_GRID:
        raise L.SfmiError(f"{what}: the lattice must have {MIN_GRID} .. {MAX_GRID} nodes per axis, got {R}")
    _check_size(B, R, what)
    dev = on_device(what, Vx, Vy, Vz)
    Vx, Vy, Vz = (t.float().contiguous() for t in (Vx, Vy, Vz))
    rhs = torch.empty(B, R, R, R, device=dev, dtype=torch.float32)
    L.check(L.lib().sfmi_poisson_rhs_f32(L.ptr(Vx), L.ptr(Vy), L.ptr(Vz), B, R, L.ptr(rhs), L.stream_ptr()), "sfmi_poisson_rhs_f32")
    return rhs


def _solve(rhs, tol, max_iter, check_every):
    lib, st, dev = L.lib(), L.stream_ptr, rhs.device
    B, R = rhs.shape[0], rhs.shape[1]
    if max_iter is None:
        max_iter = 4 * R
    chi = torch.empty_like(rhs)
    ws = _ragged.workspace(lib.sfmi_poisson_cg_workspace_bytes(B, R), dev)
    iters = torch.empty(B, device=dev, dtype=torch.int32)
    done = torch.empty(B, device=dev, dtype=torch.int32)
    res = torch.empty(B, device=dev, dtype=torch.float64)
    L.check(lib.sfmi_poisson_cg_init_f32(L.ptr(rhs), B, R, tol, L.ptr(chi), L.ptr(ws), st()), "sfmi_poisson_cg_init_f32")

    def read(it):
        L.check(lib.sfmi_poisson_cg_read_i32(B, R, it, L.ptr(ws), L.ptr(iters), L.ptr(res), L.ptr(done), st()), "sfmi_poisson_cg_read_i32")

    it = 0
    read(0)
    while it < max_iter and not bool(done.cpu().all()):                        # the (B,) flags after each chunk
        n = min(check_every, max_iter - it)                                    # the last chunk is cut: exactly max_iter iterations
        L.check(lib.sfmi_poisson_cg_steps_f32(B, R, n, it, L.ptr(chi), L.ptr(ws), st()), "sfmi_poisson_cg_steps_f32")
        it += n
        read(it)
    return chi, iters, res


def poisson_solve_dev(rhs, tol=1e-4, max_iter=None, check_every=16):
    """Solve A chi = rhs per shape, A = G^T G the 7-point operator with 6 on every diagonal entry (zeros around the lattice), by
    conjugate gradients from 0.  rhs (B,R,R,R) f32 HIP tensor -> chi (B,R,R,R) f32, iterations (B,) int32, residual (B,) f64 (the
    recursive |r| / |rhs|).  A shape is frozen on the device at the first iteration with |r| <= tol |rhs|, so the result does not
    depend on check_every: the host only reads the (B,) flags after each chunk of check_every iterations and stops when all are set
    or max_iter (default 4 R) iterations have run.  f32 vectors, f64 dot products over a fixed tree: bit-identical from run to run,
    and a shape solved alone equals the same shape in a batch.  A zero rhs gives zeros and 0 iterations."""
    what = "poisson_solve_dev"
    tol, max_iter, check_every = _check_solver(tol, max_iter, check_every, what)
    rhs = _lattice_arg(rhs, what)
    on_device(what, rhs)
    return _solve(rhs.float().contiguous(), tol, max_iter, check_every)


def _sample(lat, xf, o, box):
    B, R, N = lat.shape[0], lat.shape[1], xf.shape[0]
    out = torch.empty(N, device=lat.device, dtype=torch.float32)
    od = offsets_dev(o, lat.device)
    L.check(L.lib().sfmi_poisson_sample_f32(L.ptr(lat), L.ptr(xf), L.ptr(od), B, N, R, L.ptr(box), L.ptr(out), L.stream_ptr()),
            "sfmi_poisson_sample_f32")
    return out


def poisson_sample_dev(lattice, points, off=None, bbox=DEFAULT_BBOX):
    """(N,) f32: the trilinear sample of shape b's lattice (B,R,R,R) at the points of set b (f64 weights, rounded once; a point outside
    the box is sampled where it is clamped to).  The vertex densities of poisson_recon_dev are poisson_sample_dev(W, verts, voff)."""
    what = "poisson_sample_dev"
    box = _check_bbox(bbox, what)
    lattice = _lattice_arg(lattice, what)
    x = points_arg(points, what)
    if x.dim() != 2:
        raise L.SfmiError(f"{what}: expected (N,3) points with offsets, got {tuple(x.shape)}")
    o = host_offsets(off, x.shape[0], f"{what} offsets")
    if len(o) - 1 != lattice.shape[0]:
        raise L.SfmiError(f"{what}: {len(o) - 1} point sets for {lattice.shape[0]} lattices")
    on_device(what, lattice, x)
    return _sample(lattice.float().contiguous(), x.float().contiguous(), o, box)


def _field(xf, nf, o, R, box, tol, max_iter):
    lib, dev = L.lib(), xf.device
    B, N = len(o) - 1, xf.shape[0]
    Vx, Vy, Vz, W, outside = _splat(xf, nf, o, R, box)
    rhs = torch.empty(B, R, R, R, device=dev, dtype=torch.float32)
    L.check(lib.sfmi_poisson_rhs_f32(L.ptr(Vx), L.ptr(Vy), L.ptr(Vz), B, R, L.ptr(rhs), L.stream_ptr()), "sfmi_poisson_rhs_f32")
    del Vx, Vy, Vz
    chi, iters, res = _solve(rhs, tol, max_iter, 16)
    iso = torch.empty(B, device=dev, dtype=torch.float64)
    od = offsets_dev(o, dev)
    L.check(lib.sfmi_poisson_iso_f32(L.ptr(chi), L.ptr(xf), L.ptr(od), B, N, R, L.ptr(box), L.ptr(iso), L.ptr(chi), L.stream_ptr()),
            "sfmi_poisson_iso_f32")
    return chi, W, dict(iterations=iters, residual=res, iso=iso, outside=outside)


def poisson_field_dev(points, normals, off=None, grid_dim=None, depth=None, bbox=DEFAULT_BBOX, tol=1e-4, max_iter=None):
    """Splat, solve, subtract the iso-value.  -> field (B,R,R,R) f32 = chi - iso (positive inside for outward normals: mesh it with
    marching_cubes_dev(field, 0.0, bbox)), W (B,R,R,R) the density, info = {iterations (B,) int32, residual (B,) f64, iso (B,) f64,
    outside (B,) int32} on the device.  grid_dim (default 129) or depth (grid_dim = 2^depth + 1).  iso[b] is the mean of the trilinear
    chi over the set's in-box points, an f64 sum in a fixed order; a set without an in-box point gives an all-zero field."""
    what = "poisson_field_dev"
    R = _check_grid(grid_dim, depth, what)
    box = _check_bbox(bbox, what)
    tol, max_iter, _ = _check_solver(tol, max_iter, 16, what)
    if normals is None:
        raise L.SfmiError(f"{what}: normals are required (poisson_recon_dev estimates them from a viewpoint)")
    x, n, o = _cloud_args(points, normals, off, what)
    _check_size(len(o) - 1, R, what)
    on_device(what, x, n)
    return _field(x.float().contiguous(), n.float().contiguous(), o, R, box, tol, max_iter)


def _np_quantile(sorted64, q):
    """np.quantile(..., q) of an ascending f64 device vector: numpy's default linear definition, operation for operation"""
    n = sorted64.shape[0]
    pos = (n - 1) * q
    lo = int(math.floor(pos))
    hi = min(lo + 1, n - 1)
    t = pos - lo
    a, b = sorted64[lo], sorted64[hi]
    d = b - a
    return b - d * (1 - t) if t >= 0.5 else a + d * t


def _trim(verts, faces, vo, to, density, q):
    """drop the vertices whose density lies below the shape's q-quantile, the faces that touch one, compact per shape"""
    dev, B = verts.device, len(vo) - 1
    d64 = density.double()
    thr = torch.full((B,), -math.inf, device=dev, dtype=torch.float64)
    for b in range(B):
        if vo[b + 1] > vo[b]:
            thr[b] = _np_quantile(torch.sort(d64[int(vo[b]):int(vo[b + 1])]).values, q)
    vod, tod = offsets_dev(vo, dev), offsets_dev(to, dev)
    vshape = torch.repeat_interleave(torch.arange(B, device=dev), vod[1:] - vod[:-1], output_size=verts.shape[0])
    fshape = torch.repeat_interleave(torch.arange(B, device=dev), tod[1:] - tod[:-1], output_size=faces.shape[0])
    keep = d64 >= thr[vshape]
    gf = faces.long() + vod[fshape][:, None]                                   # global vertex indices
    fkeep = keep[gf].all(1)
    vin = torch.cumsum(keep, 0)
    vex = torch.cat([vin.new_zeros(1), vin])                                   # kept vertices before each vertex
    fex = torch.cat([vin.new_zeros(1), torch.cumsum(fkeep, 0)])
    h = torch.cat([vex[vod], fex[tod]]).cpu().numpy()                          # the one read-back: sizes
    nvo, nto = h[:B + 1].astype(np.int64), h[B + 1:].astype(np.int64)
    nf = (vex[gf[fkeep]] - vex[vod][fshape[fkeep]][:, None]).to(torch.int32)
    return verts[keep], nf, nvo, nto, density[keep]


def poisson_recon_dev(points, normals=None, off=None, depth=None, quantile=0.0, knn=10, viewpoint=None, keep_components=None,
                      grid_dim=None, bbox=DEFAULT_BBOX, tol=1e-4, max_iter=None, orient=None):
    """geoutil.Open3D_Toolbox.poisson_recon on the device, for a ragged batch of clouds: normals (given, or estimate_normals_dev over
    knn neighbours oriented towards `viewpoint`), poisson_field_dev on a lattice of 2^depth + 1 nodes per axis (default depth 7; or
    grid_dim), marching_cubes_dev at 0, then the density trim: a vertex's density is the trilinear sample of W there, and with
    quantile = q > 0 the vertices below np.quantile(the shape's densities, q) (numpy's default linear definition, in f64) go, with
    every face that touches one; indices are compacted per shape.  q = 0 removes nothing.  keep_components (components.parse_keep's
    forms) filters the connected components after the trim.
    -> verts (V,3) f32, faces (T,3) int32 local per shape, voff, toff (B+1,) host, density (V,) f32.
    normals=None needs a viewpoint ((B,3), or (3,) for one set): the sign rule of estimate_normals_dev without one is not a consistent
    orientation, and Poisson needs one.  orient="tangent" (with normals=None) is the other way to one: the estimated normals are
    oriented by scan.orient_normals_dev on the same knn table, towards the viewpoint if one is given and outward otherwise."""
    from .components import parse_keep
    what = "poisson_recon_dev"
    if orient not in (None, "tangent"):
        raise L.SfmiError(f"{what}: orient must be None or 'tangent', got {orient!r}")
    if grid_dim is None and depth is None:
        depth = 7
    R = _check_grid(grid_dim, depth, what)
    box = _check_bbox(bbox, what)
    q = _check_quantile(quantile, what)
    tol, max_iter, _ = _check_solver(tol, max_iter, 16, what)
    keep = parse_keep(keep_components)
    x, n, o = _cloud_args(points, normals, off, what)
    _check_size(len(o) - 1, R, what)
    if n is None and viewpoint is None and orient is None:
        raise L.SfmiError(f"{what}: normals=None needs a viewpoint to orient the estimated normals (without one their signs are not "
                          "a consistent orientation)")
    if n is not None and orient is not None:
        raise L.SfmiError(f"{what}: orient goes with normals=None (given normals are used as they are; scan.orient_normals_dev "
                          "orients them)")
    on_device(what, x, *([n] if n is not None else []))
    xf = x.float().contiguous()
    if n is None:
        from .scan import estimate_normals_dev
        n = estimate_normals_dev(xf, o, knn, viewpoint, orient)[0]
    field, W, _ = _field(xf, n.float().contiguous(), o, R, box, tol, max_iter)
    from .mcubes import marching_cubes_dev
    lo_hi = (tuple(box[:3]), tuple(box[3:]))
    v, f, vo, to = marching_cubes_dev(field, 0.0, lo_hi)
    vo, to = np.asarray(vo, np.int64), np.asarray(to, np.int64)
    v, f = v.contiguous(), f.contiguous()
    density = _sample(W, v, vo, box)
    if q > 0 and v.shape[0]:
        v, f, vo, to, density = _trim(v, f, vo, to, density, q)
    if keep is not None and v.shape[0]:
        from .components import keep_components_dev
        v, f, vo, to = keep_components_dev(v, f, vo, to, **keep)[:4]
        vo, to = np.asarray(vo, np.int64), np.asarray(to, np.int64)
        density = _sample(W, v.contiguous(), vo, box)                          # the same vertices: the same samples
    return v, f, vo, to, density


class Open3D_Toolbox:
    """The reference's call for one numpy cloud (xgutils/geoutil.py:297-336), on the device."""

    def __init__(self, device="cuda:0"):
        self.device = device

    def poisson_recon(self, cloud, normals=None, viewpoint=None, depth=6, quantile=.3, knn=10, orient=None):
        """cloud (N,3) numpy, normals (N,3) or None (then estimated over knn neighbours and oriented towards viewpoint (3,), or with
        orient="tangent" by tangent-plane propagation, outward when no viewpoint is given)
        -> (vert (V,3) float64, face (T,3) int) numpy"""
        c = np.ascontiguousarray(np.asarray(cloud, np.float32))
        if c.ndim != 2 or c.shape[1] != 3:
            raise L.SfmiError(f"Open3D_Toolbox.poisson_recon: expected an (N,3) cloud, got {c.shape}")
        if normals is None and viewpoint is None and orient is None:
            raise L.SfmiError("Open3D_Toolbox.poisson_recon: normals=None needs a viewpoint to orient the estimated normals")
        dev = torch.device(self.device)
        x = torch.from_numpy(c).to(dev)
        n = None if normals is None else torch.from_numpy(np.ascontiguousarray(np.asarray(normals, np.float32))).to(dev)
        v, f = poisson_recon_dev(x, n, None, depth=depth, quantile=quantile, knn=knn, viewpoint=viewpoint, orient=orient)[:2]
        return v.cpu().numpy().astype(np.float64), f.cpu().numpy().astype(int)
