"""Smooth fields and smooth meshes from binary voxel grids on the device — host side of csrc/edt.hip.

`marching_cubes_dev` at 0.5 turns a binary grid (morph_voxelization_dev, mesh_occupancy_dev, the IMNet occupancy) into the staircase
surface of the voxels themselves.  The reference smooths first, inside the same call: xgutils/geoutil.py:194-197, array2mesh with
gaussian_sigma passes the grid through mcubes.smooth (a signed Euclidean distance transform, then a Gaussian filter or a constrained
solve in a narrow band: Lempitsky, CVPR 2010) on one core.  Here the three steps run where the grid is.  The contract is in
include/sfmi.h, its numpy / scipy statement in tests/voxfield_ref.py; it is this library's own, modelled on PyMCubes' smooth_gaussian /
smooth_constrained, and parity with PyMCubes' numbers is not claimed.  There is no CPU fallback.

  edt_sq_dev(vox, invert=False)                          -> d2 int32, status      scipy.ndimage.distance_transform_edt(vox)**2 (invert)
  signed_distance_dev(vox)                               -> d f64, status         positive inside, +-0.5 at the voxel faces
  gaussian_smooth_dev(vox, sigma=3.0)                    -> f64 field             scipy.ndimage.gaussian_filter(vox - 0.5, sigma)
  constrained_smooth_dev(vox, band_radius=4.0, iters=200) -> u f64, status        the projected biharmonic iteration on the band
  smooth_dev(vox, method="constrained" | "gaussian", **kw) -> f64 field
  voxels2mesh_dev(vox, method="constrained", bbox=..., **kw) -> verts, faces, voff, toff   smooth, cast to f32, marching cubes at 0

Grids are (B,G,G,G) or (G,G,G) uint8 / bool device tensors as in morph.py (non-zero = set; a (G,G,G) grid is a batch of one and comes
back without the batch axis), 1 <= G <= 513, B * G^3 < 2^31.  Every result is a function of the input bits: bit-identical from run to
run and between a batch and per-grid calls.  Arguments are checked on the host before anything is launched, the device last; the host
decides nothing from device data (voxels2mesh_dev reads the face counts back, as meshing does).
status (B,) int32 on the device: 0 ok; 1 the grid is all clear (edt_sq_dev: no voxel of the wanted kind) or all set: distances are then
sqrt(3) G, beyond any distance inside the lattice.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib as L
from . import _ragged
from . import morph as M
from ._ragged import on_device

MAX_GRID = 513              # sfmi_vox_max_grid()
MAX_RADIUS = 64             # sfmi_vox_gaussian_max_radius()
METHODS = ("constrained", "gaussian")
STATUS_OK, STATUS_UNIFORM = 0, 1


# ---- argument handling (host only: everything here runs before any launch) -------------------------------------------------

def _grid(vox, what):
    v4, B, G, squeeze = M._grid(vox, what)
    if G > MAX_GRID:
        raise L.SfmiError(f"{what}: G = {G} must be at most {MAX_GRID}")
    return v4, B, G, squeeze


def gaussian_weights(sigma, what="gaussian_smooth_dev"):
    """-> (radius, (2 radius + 1,) f64 weights) exactly as scipy.ndimage.gaussian_filter1d computes them with truncate = 4.0"""
    if isinstance(sigma, bool) or not isinstance(sigma, (int, float, np.integer, np.floating)) or not math.isfinite(sigma) or sigma <= 0:
        raise L.SfmiError(f"{what}: sigma = {sigma!r} must be a finite number > 0")
    sd = float(sigma)
    radius = int(4.0 * sd + 0.5)
    if radius > MAX_RADIUS:
        raise L.SfmiError(f"{what}: sigma = {sigma!r} gives a radius of {radius} taps, above {MAX_RADIUS}")
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sd * sd) * x ** 2)
    return radius, phi / phi.sum()


def _solve_args(band_radius, iters, what):
    if isinstance(band_radius, bool) or not isinstance(band_radius, (int, float, np.integer, np.floating)) or \
            not math.isfinite(band_radius) or band_radius < 0:
        raise L.SfmiError(f"{what}: band_radius = {band_radius!r} must be a finite number >= 0")
    if isinstance(iters, bool) or not isinstance(iters, (int, np.integer)) or iters < 0:
        raise L.SfmiError(f"{what}: iters = {iters!r} must be an int >= 0")
    return float(band_radius), int(iters)


def _method(method, kw, what):
    if method not in METHODS:
        raise L.SfmiError(f"{what}: method = {method!r} must be one of {METHODS}")
    allowed = ("band_radius", "iters") if method == "constrained" else ("sigma",)
    extra = sorted(set(kw) - set(allowed))
    if extra:
        raise L.SfmiError(f"{what}: method {method!r} takes {allowed}, not {extra}")


# ---- the launches on bit sets ----------------------------------------------------------------------------------------------

def _edt_sq(bits, B, G, invert):
    dev = bits.device
    d2 = torch.empty(B, G, G, G, device=dev, dtype=torch.int32)
    status = torch.empty(B, device=dev, dtype=torch.int32)
    ws = _ragged.workspace(L.lib().sfmi_edt_workspace_bytes(B, G, 0), dev)
    L.check(L.lib().sfmi_edt_sq_u32(L.ptr(bits), B, G, int(invert), L.ptr(d2), L.ptr(status), L.ptr(ws), L.stream_ptr()), "sfmi_edt_sq_u32")
    return d2, status


def _signed(bits, B, G):
    dev = bits.device
    d = torch.empty(B, G, G, G, device=dev, dtype=torch.float64)
    status = torch.empty(B, device=dev, dtype=torch.int32)
    ws = _ragged.workspace(L.lib().sfmi_edt_workspace_bytes(B, G, 1), dev)
    L.check(L.lib().sfmi_edt_signed_f64(L.ptr(bits), B, G, L.ptr(d), L.ptr(status), L.ptr(ws), L.stream_ptr()), "sfmi_edt_signed_f64")
    return d, status


def _gaussian(bits, B, G, radius, weights):
    dev = bits.device
    w = torch.from_numpy(np.ascontiguousarray(weights, dtype=np.float64)).to(dev)
    out = torch.empty(B, G, G, G, device=dev, dtype=torch.float64)
    ws = _ragged.workspace(L.lib().sfmi_vox_gaussian_workspace_bytes(B, G), dev)
    L.check(L.lib().sfmi_vox_gaussian_f64(L.ptr(bits), B, G, L.ptr(w), radius, L.ptr(out), L.ptr(ws), L.stream_ptr()), "sfmi_vox_gaussian_f64")
    return out


def _constrained(bits, d, B, G, band_radius, iters, return_ws=False):
    dev = bits.device
    u = torch.empty_like(d)
    ws = _ragged.workspace(L.lib().sfmi_vox_constrained_workspace_bytes(B, G), dev)
    L.check(L.lib().sfmi_vox_constrained_f64(L.ptr(bits), L.ptr(d), B, G, band_radius, iters, L.ptr(u), L.ptr(ws), L.stream_ptr()),
            "sfmi_vox_constrained_f64")
    return (u, ws) if return_ws else u


def _band_lists(ws, B, G):
    """the lists the solve left in its workspace -> band, support (int32 flat indices, ascending; the host reads the two counts)"""
    dev = ws.device
    band = torch.empty(B * G ** 3, device=dev, dtype=torch.int32)
    sup = torch.empty_like(band)
    n = torch.empty(2, device=dev, dtype=torch.int32)
    L.check(L.lib().sfmi_vox_constrained_lists_i32(L.ptr(ws), B, G, L.ptr(band), L.ptr(sup), L.ptr(n), L.stream_ptr()),
            "sfmi_vox_constrained_lists_i32")
    nb, ns = n.cpu().tolist()
    return band[:nb], sup[:ns]


def _smooth(v4, B, G, method, kw):
    """-> (field (B,G,G,G) f64, status or None) after every check"""
    bits = M._pack(v4, B, G)
    if method == "gaussian":
        return _gaussian(bits, B, G, *kw["weights"]), None
    d, status = _signed(bits, B, G)
    return _constrained(bits, d, B, G, kw["band_radius"], kw["iters"]), status


def _parse(method, kw, what):
    _method(method, kw, what)
    if method == "gaussian":
        return dict(weights=gaussian_weights(kw.get("sigma", 3.0), what))
    r, n = _solve_args(kw.get("band_radius", 4.0), kw.get("iters", 200), what)
    return dict(band_radius=r, iters=n)


# ---- public ----------------------------------------------------------------------------------------------------------------

def edt_sq_dev(vox, invert=False):
    """d2[v] = min |u - v|^2 in integers over the set voxels u of the same grid (invert: the clear ones); 0 on the set itself.  With
    invert=True this is scipy.ndimage.distance_transform_edt(vox)**2.  -> d2 int32 (vox's shape), status (B,) int32 (1: the set is
    empty and d2 = 3 G^2 everywhere)."""
    v4, B, G, squeeze = _grid(vox, "edt_sq_dev")
    on_device("edt_sq_dev", vox)
    d2, status = _edt_sq(M._pack(v4, B, G), B, G, bool(invert))
    return (d2[0] if squeeze else d2), status


def signed_distance_dev(vox):
    """The signed Euclidean distance to the voxel faces, positive inside: sqrt(d2 to the nearest clear voxel) - 0.5 on a set voxel,
    -sqrt(d2 to the nearest set voxel) + 0.5 on a clear one, in f64.  -> d f64 (vox's shape), status (B,) int32 (1: all set or all
    clear)."""
    v4, B, G, squeeze = _grid(vox, "signed_distance_dev")
    on_device("signed_distance_dev", vox)
    d, status = _signed(M._pack(v4, B, G), B, G)
    return (d[0] if squeeze else d), status


def gaussian_smooth_dev(vox, sigma=3.0):
    """scipy.ndimage.gaussian_filter(f64(vox != 0) - 0.5, sigma, mode="reflect") with scipy's truncate = 4.0 (its kernel, computed on
    the host as scipy computes it; radius = int(4 sigma + 0.5) <= 64).  -> f64 field, positive inside."""
    radius, w = gaussian_weights(sigma)
    v4, B, G, squeeze = _grid(vox, "gaussian_smooth_dev")
    on_device("gaussian_smooth_dev", vox)
    out = _gaussian(M._pack(v4, B, G), B, G, radius, w)
    return out[0] if squeeze else out


def constrained_smooth_dev(vox, band_radius=4.0, iters=200):
    """The smoothest field that keeps every voxel on its side of zero: u_0 = signed_distance_dev(vox); `iters` times, on the band
    |d| <= band_radius, u <- max(lo, min(hi, u - L(L u) / 84)) with L the Neumann Laplacian and [lo, hi] = [0, inf) on set voxels,
    (-inf, 0] on clear ones; off the band u stays d.  The iteration count is the argument: there is no convergence test.
    -> u f64 (vox's shape), status (B,) int32 (signed_distance_dev's)."""
    r, n = _solve_args(band_radius, iters, "constrained_smooth_dev")
    v4, B, G, squeeze = _grid(vox, "constrained_smooth_dev")
    on_device("constrained_smooth_dev", vox)
    u, status = _smooth(v4, B, G, "constrained", dict(band_radius=r, iters=n))
    return (u[0] if squeeze else u), status


def smooth_dev(vox, method="constrained", **kw):
    """constrained_smooth_dev's field (band_radius=, iters=) or gaussian_smooth_dev's (sigma=): an f64 field whose zero level is the
    smoothed surface, positive inside."""
    args = _parse(method, kw, "smooth_dev")
    v4, B, G, squeeze = _grid(vox, "smooth_dev")
    on_device("smooth_dev", vox)
    out = _smooth(v4, B, G, method, args)[0]
    return out[0] if squeeze else out


def voxels2mesh_dev(vox, method="constrained", bbox=((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)), **kw):
    """smooth_dev, cast to f32, marching_cubes_dev at level 0 over bbox -> verts (V,3) f32, faces (T,3) int32 local to each grid, host
    voff, toff (B+1,): the ragged mesh format of every mesh tool here."""
    from .mcubes import marching_cubes_dev
    args = _parse(method, kw, "voxels2mesh_dev")
    v4, B, G, _ = _grid(vox, "voxels2mesh_dev")
    if G < 2 or 3 * B * G ** 3 >= 2 ** 31:                 # marching_cubes_dev's own limits, checked before the smoothing is spent
        raise L.SfmiError(f"voxels2mesh_dev: marching cubes needs G >= 2 and 3 * B * G^3 < 2^31, got B = {B}, G = {G}")
    on_device("voxels2mesh_dev", vox)
    return marching_cubes_dev(_smooth(v4, B, G, method, args)[0].float(), 0.0, bbox)
