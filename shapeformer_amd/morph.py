"""Watertight voxelization of triangle soups on the device — host side of csrc/morph.hip.

`meshsdf.mesh_occupancy_dev` decides inside by the winding number, which needs closed, consistently oriented meshes.  ShapeNet .obj files
and raw scans are soups: open shells, interior partitions, doubled and flipped faces.  The reference's tool for them is
xgutils/geoutil.py:383-401 morph_voxelization (skimage, one core): sample the surface, voxelize the samples, dilate by a ball, flood the
outside from voxel (0,0,0), erode.  Here the same steps run where the mesh is.  The contract is in include/sfmi.h, its numpy / scipy
statement in tests/morph_ref.py.  There is no CPU fallback.

  point2voxel_dev(points, off=None, grid_dim=32)                  -> (B,G,G,G) uint8     ptutil.point2voxel
  ball_dilate_dev(vox, r) / ball_erode_dev(vox, r)                -> uint8 grids         binary_dilation / binary_erosion with ball(r)
  flood_dev(vox)                                                  -> region, status      flood(vox, (0,0,0))
  watertight_fill_dev(vox, selem_size=6)                          -> uint8 grids         geoutil.py:393-400
  morph_voxelization_dev(verts, faces, voff, toff, ...)           -> uint8 grids         the whole of morph_voxelization, ragged batches
  voxel_lookup_dev(vox, points, off=None)                         -> (N,) uint8          the voxel of the cell that holds each point

Grids are (B,G,G,G) uint8 device tensors ([i][j][k] = x, y, z; a (G,G,G) grid is taken as a batch of one and comes back as (G,G,G)).
Everything after the surface samples is exact: bit-identical to the reference's integer steps, from run to run, and between a batch and
per-shape calls.  Arguments are checked on the host before anything is launched (ragged batches: _ragged.py).
status (B,) int32 on the device: 0 ok; 3 the seed voxel (0,0,0) was set, so the flood ran over the set voxels as the reference's would
(morph_voxelization_dev: 1 a mesh without surface area).
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L
from . import _ragged
from ._ragged import i32_dev, mesh_args, on_device, point_sets

MAX_RADIUS = 16         # sfmi_morph_max_radius()
STATUS_OK, STATUS_NO_AREA, STATUS_SEED_SET = 0, 1, 3


# ---- argument handling (host only: everything here runs before any launch) -------------------------------------------------

def _grid_dim(grid_dim, what):
    if isinstance(grid_dim, bool) or not isinstance(grid_dim, (int, np.integer)) or grid_dim < 1:
        raise L.SfmiError(f"{what}: grid_dim = {grid_dim!r} must be an int >= 1")
    return int(grid_dim)


def _radius(r, what, name="r"):
    if isinstance(r, bool) or not isinstance(r, (int, np.integer)) or not 0 <= r <= MAX_RADIUS:
        raise L.SfmiError(f"{what}: {name} = {r!r} must be an int in [0, {MAX_RADIUS}]")
    return int(r)


def _sizes(B, G, what):
    if B < 1:
        raise L.SfmiError(f"{what}: an empty batch")
    if B * G ** 3 >= 2 ** 31:
        raise L.SfmiError(f"{what}: B * G^3 = {B} * {G}^3 needs 32-bit voxel indices (must be < 2^31)")


def _grid(vox, what):
    """-> (vox as (B,G,G,G), B, G, squeeze) after the shape checks (the device is checked by the caller, last)"""
    if not isinstance(vox, torch.Tensor):
        raise L.SfmiError(f"{what}: vox must be a torch tensor on the HIP device (no CPU fallback)")
    if vox.dim() not in (3, 4) or len(set(vox.shape[-3:])) != 1 or vox.shape[-1] < 1:
        raise L.SfmiError(f"{what}: vox must be (B,G,G,G) or (G,G,G), got {tuple(vox.shape)}")
    squeeze = vox.dim() == 3
    v4 = vox[None] if squeeze else vox
    _sizes(v4.shape[0], v4.shape[-1], what)
    return v4, v4.shape[0], v4.shape[-1], squeeze


def _points32(points, off, what):
    """-> (points as (N,3), host offsets (B+1,)); the kernels index the coordinates in 32 bits"""
    points, o, _ = point_sets(points, off, what)
    if 3 * points.shape[0] >= 2 ** 31:
        raise L.SfmiError(f"{what}: 2^31 / 3 points or more")
    return points, o


# ---- the launches on bit sets: (B,G,G,Wz) words held in int32 tensors ------------------------------------------------------

def _words(B, G, dev):
    return torch.empty(B, G, G, (G + 31) // 32, device=dev, dtype=torch.int32)


def _workspace(B, G, r, dev):
    return _ragged.workspace(L.lib().sfmi_morph_workspace_bytes(B, G, r), dev)


def _pack(v4, B, G):
    v8 = v4.contiguous() if v4.dtype == torch.uint8 else (v4 != 0).to(torch.uint8).contiguous()
    bits = _words(B, G, v4.device)
    L.check(L.lib().sfmi_morph_pack_u8(L.ptr(v8), B, G, L.ptr(bits), L.stream_ptr()), "sfmi_morph_pack_u8")
    return bits


def _unpack(bits, B, G, squeeze=False):
    vox = torch.empty(B, G, G, G, device=bits.device, dtype=torch.uint8)
    L.check(L.lib().sfmi_morph_unpack_u8(L.ptr(bits), B, G, L.ptr(vox), L.stream_ptr()), "sfmi_morph_unpack_u8")
    return vox[0] if squeeze else vox


def _dilate(bits, B, G, r, invert_in, invert_out, ws):
    out = torch.empty_like(bits)
    L.check(L.lib().sfmi_morph_dilate_u32(L.ptr(bits), B, G, r, int(invert_in), int(invert_out), L.ptr(out), L.ptr(ws), L.stream_ptr()),
            "sfmi_morph_dilate_u32")
    return out


def _flood(bits, B, G, ws):
    region = torch.empty_like(bits)
    status = torch.empty(B, device=bits.device, dtype=torch.int32)
    L.check(L.lib().sfmi_morph_flood_u32(L.ptr(bits), B, G, L.ptr(region), L.ptr(status), L.ptr(ws), L.stream_ptr()), "sfmi_morph_flood_u32")
    return region, status


def _voxelize(pts, o, B, G, dev):
    pf = pts.float().contiguous()
    od = i32_dev(o, dev)
    bits = _words(B, G, dev)
    L.check(L.lib().sfmi_voxelize_points_f32(L.ptr(pf), L.ptr(od), B, pf.shape[0], G, L.ptr(bits), L.stream_ptr()), "sfmi_voxelize_points_f32")
    return bits


def _fill(bits, B, G, r):
    """geoutil.py:393-400 on bit sets.  erode(1 - flood) = NOT dilate(flood): the complement costs no pass of its own"""
    ws = _workspace(B, G, r, bits.device)
    if r > 0:
        bits = _dilate(bits, B, G, r, False, False, ws)
    region, status = _flood(bits, B, G, ws)
    return _dilate(region, B, G, r, False, True, ws), status


# ---- public ----------------------------------------------------------------------------------------------------------------

def point2voxel_dev(points, off=None, grid_dim=32):
    """ptutil.point2voxel: the voxel clamp(round(((p + 1) / 2) * G - 0.5), 0, G - 1) of every point is set (f32, half to even, as torch
    evaluates the reference's expression); a point with a non-finite coordinate sets none.  points (N,3) with off (B+1,) exclusive offsets
    (None: one set) or (B,N,3).  -> (B,G,G,G) uint8."""
    G = _grid_dim(grid_dim, "point2voxel_dev")
    pts, o = _points32(points, off, "point2voxel_dev")
    B = len(o) - 1
    _sizes(B, G, "point2voxel_dev")
    dev = on_device("point2voxel_dev", points)
    return _unpack(_voxelize(pts, o, B, G, dev), B, G)


def voxel_lookup_dev(vox, points, off=None):
    """The voxel of the cell that holds each point (point2voxel_dev's index; 0 for a non-finite point): vox (B,G,G,G), points (N,3) with
    off (B+1,) or (B,N,3) -> (N,) / (B,N) uint8."""
    v4, B, G, _ = _grid(vox, "voxel_lookup_dev")
    pts, o = _points32(points, off, "voxel_lookup_dev")
    if len(o) - 1 != B:
        raise L.SfmiError(f"voxel_lookup_dev: {len(o) - 1} point sets for {B} grids")
    dev = on_device("voxel_lookup_dev", vox, points)
    pf, od = pts.float().contiguous(), i32_dev(o, dev)
    bits = _pack(v4, B, G)
    out = torch.empty(pf.shape[0], device=dev, dtype=torch.uint8)
    L.check(L.lib().sfmi_voxelize_lookup_f32(L.ptr(pf), L.ptr(od), B, pf.shape[0], G, L.ptr(bits), L.ptr(out), L.stream_ptr()),
            "sfmi_voxelize_lookup_f32")
    return out.reshape(points.shape[:-1])


def _morph(vox, r, erode, what):
    r = _radius(r, what)
    v4, B, G, squeeze = _grid(vox, what)
    dev = on_device(what, vox)
    out = _dilate(_pack(v4, B, G), B, G, r, erode, erode, _workspace(B, G, r, dev))
    return _unpack(out, B, G, squeeze)


def ball_dilate_dev(vox, r):
    """skimage binary_dilation(vox, ball(r)): a voxel is set iff a set voxel lies within r (integer squared distance <= r^2); outside the
    grid counts as empty.  0 <= r <= 16."""
    return _morph(vox, r, False, "ball_dilate_dev")


def ball_erode_dev(vox, r):
    """skimage binary_erosion(vox, ball(r)): a voxel stays iff every voxel within r is set; outside the grid counts as set."""
    return _morph(vox, r, True, "ball_erode_dev")


def flood_dev(vox):
    """skimage flood(vox, (0,0,0)): the voxels that carry voxel (0,0,0)'s value and are joined to it under 26-connectivity.
    -> region (uint8, vox's shape), status (B,) int32 (3: the seed voxel was set)."""
    v4, B, G, squeeze = _grid(vox, "flood_dev")
    dev = on_device("flood_dev", vox)
    region, status = _flood(_pack(v4, B, G), B, G, _workspace(B, G, 0, dev))
    return _unpack(region, B, G, squeeze), status


def watertight_fill_dev(vox, selem_size=6, return_status=False):
    """geoutil.py:393-400: selem_size == 0 -> 1 - flood(vox); else erode(1 - flood(dilate(vox))) with ball(selem_size).
    -> uint8 grid(s) (, status)."""
    r = _radius(selem_size, "watertight_fill_dev", "selem_size")
    v4, B, G, squeeze = _grid(vox, "watertight_fill_dev")
    on_device("watertight_fill_dev", vox)
    out, status = _fill(_pack(v4, B, G), B, G, r)
    out = _unpack(out, B, G, squeeze)
    return (out, status) if return_status else out


def index2point_dev(grid_dim, device):
    """ptutil.index2point of every cell of the grid: (idx + .5) / G * 2 - 1 -> (G^3, 3) f32, first axis slowest."""
    c = (torch.arange(grid_dim, device=device, dtype=torch.float32) + 0.5) / grid_dim * 2 - 1
    return torch.stack(torch.meshgrid(c, c, c, indexing="ij"), -1).reshape(-1, 3)


def morph_voxelization_dev(verts, faces, voff=None, toff=None, sampleN=1_000_000, grid_dim=128, selem_size=6, seed=0,
                           return_status=False, return_coords=False, return_samples=False):
    """geoutil.morph_voxelization for a ragged batch of meshes (verts (V,3) f32, faces (T,3) int local per shape, host voff / toff
    (B+1,), None: one mesh): sampleN area-weighted surface samples per shape (sample_mesh_dev: the reference's distribution, not its
    draws), their voxels, then watertight_fill_dev.  -> (B,G,G,G) uint8 (, coords (G^3,3) f32 cell centres) (, status (B,) int32: 1 a
    mesh without surface area, 3 the seed voxel was set) (, the samples (B,sampleN,3))."""
    from .metrics import sample_mesh_dev
    what = "morph_voxelization_dev"
    G, r = _grid_dim(grid_dim, what), _radius(selem_size, what, "selem_size")
    vf, ff, vo, to = mesh_args(verts, faces, voff, toff, what)
    if (np.diff(to) == 0).any():
        raise L.SfmiError(f"{what}: a shape has no faces")
    if isinstance(sampleN, bool) or not isinstance(sampleN, (int, np.integer)) or sampleN < 1:
        raise L.SfmiError(f"{what}: sampleN = {sampleN!r} must be an int >= 1")
    B, n = len(to) - 1, int(sampleN)
    _sizes(B, G, what)
    if 3 * B * n >= 2 ** 31:
        raise L.SfmiError(f"{what}: B * sampleN = {B} * {n} points is 2^31 / 3 or more")
    dev = on_device(what, verts, faces)
    pts, st = sample_mesh_dev(vf, ff, vo, to, n, seed=seed)
    out, st3 = _fill(_voxelize(pts, np.arange(B + 1, dtype=np.int64) * n, B, G, dev), B, G, r)
    res = [_unpack(out, B, G)]
    if return_coords:
        res.append(index2point_dev(G, dev))
    if return_status:
        res.append(torch.where(st != 0, torch.ones_like(st3), st3))
    if return_samples:
        res.append(pts.reshape(B, n, 3))
    return res[0] if len(res) == 1 else tuple(res)
