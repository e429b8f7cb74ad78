"""Mesh signed distance and occupancy on the device — host side of csrc/meshsdf.hip.

The way back in: a user's meshes (ShapeNet .obj, ModelNet .off, a completion's own .ply) become the surface samples and lattice
occupancy the VQDIF / transformer training reads (`make_dataset.py` writes the IMNet2-style store).  The reference does this on
the CPU with libigl (xgutils/geoutil.py:265-269 signed_distance, :282-291 mesh2sdf, :455-490 SDF_sampling; the dataset sampler
shapeformer/data/imnet_datasets/utils.py:33-70); here every query is exact brute force over its mesh's faces on the device.
There is no CPU fallback.

Contracts (include/sfmi.h):
  distance  exact f32 distance to the closest point of the mesh (degenerate faces: their segment or point); the lowest face
            index wins an f32 tie; I, C and |S| are bit-identical between a batch and per-shape calls and from run to run
  sign      S = -sqrt(d2) where |W| > 0.5 (inside), else +sqrt(d2); W = generalized winding number (sum of solid angles / 4 pi),
            libigl's winding-number sign type for closed, consistently oriented meshes; finite inputs never give NaN
  status    per shape: 0 ok, 1 no faces, 2 a vertex index outside the shape; its queries get S = NaN, I = -1, C = NaN, W = 0
            (its lattice occupancy is 0)
Ragged batches (_ragged.py): verts (V,3) f32 and faces (T,3) int32 local to each shape, host offsets voff / toff /
qoff (B+1,), validated before any launch.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L
from . import _ragged
from ._ragged import batch_meshes, f32_dev, host_offsets, mesh_args, on_device
from .metrics import sample_mesh_dev

STATUS_OK, STATUS_NO_FACES, STATUS_BAD_INDEX = 0, 1, 2


def _workspace(B, N, T, dev):
    return _ragged.workspace(L.lib().sfmi_mesh_sdf_workspace_bytes(B, N, T), dev)


def signed_distance_dev(queries, verts, faces, qoff=None, voff=None, toff=None, return_winding=False):
    """Signed distance of every query to the mesh of its set.

    queries (N,3), verts (V,3) f32 and faces (T,3) int HIP tensors; qoff / voff / toff (B+1,) exclusive offsets (None: one shape).
    -> S (N,) f32 signed distance (negative inside), I (N,) int32 closest face local to the shape, C (N,3) f32 closest point
    (, W (N,) f32 winding number), status (B,) int32: 0 ok, 1 the shape has no faces, 2 a face index outside the shape (its queries get
    S = NaN, I = -1, C = NaN, W = 0).  A shape with queries but no faces raises SfmiError; a shape with neither is admitted and gets
    status 1.  Bit-identical from run to run; a shape's results, W included, depend on that shape alone (include/sfmi.h)."""
    if not isinstance(queries, torch.Tensor) or queries.dim() != 2 or queries.shape[1] != 3:
        raise L.SfmiError("signed_distance_dev: queries must be an (N,3) torch tensor")
    vf, ff, vo, to = mesh_args(verts, faces, voff, toff, "signed_distance_dev")
    qo = host_offsets(qoff, queries.shape[0], "signed_distance_dev qoff")
    if len(qo) != len(to):
        raise L.SfmiError(f"signed_distance_dev: {len(qo) - 1} query sets for {len(to) - 1} meshes")
    if ((np.diff(to) == 0) & (np.diff(qo) > 0)).any():
        raise L.SfmiError("signed_distance_dev: a shape has queries but no faces")
    dev = on_device("signed_distance_dev", queries, verts, faces)
    B, N, T = len(to) - 1, queries.shape[0], faces.shape[0]
    qf = queries.float().contiguous()
    S = torch.empty(N, device=dev, dtype=torch.float32)
    I = torch.empty(N, device=dev, dtype=torch.int32)
    C = torch.empty(N, 3, device=dev, dtype=torch.float32)
    W = torch.empty(N, device=dev, dtype=torch.float32) if return_winding else None
    status = torch.empty(B, device=dev, dtype=torch.int32)
    qod, vod, tod = (torch.from_numpy(o).to(dev) for o in (qo, vo, to))
    ws = _workspace(B, N, T, dev)
    L.check(L.lib().sfmi_mesh_sdf_f32(L.ptr(qf), L.ptr(qod), L.ptr(vf), L.ptr(ff), L.ptr(vod), L.ptr(tod), B, N, T, L.ptr(S), L.ptr(I),
                                      L.ptr(C), L.ptr(W), L.ptr(status), L.ptr(ws), L.stream_ptr()), "sfmi_mesh_sdf_f32")
    return (S, I, C, W, status) if return_winding else (S, I, C, status)


def mesh_occupancy_dev(verts, faces, voff, toff, grid_dim=64, bbox=((-1.0,) * 3, (1.0,) * 3), return_status=False):
    """Inside test (|W| > 0.5) of every point of the makeGrid(bbox, [grid_dim]*3, mode="on", indexing="ij") lattice, generated in
    the kernel (no G^3 query array).  -> (B, G, G, G) uint8 in data.make_grid's order (first axis slowest) (, status (B,)).
    A shape without faces raises SfmiError.  A shape's lattice depends on that shape alone."""
    vf, ff, vo, to = mesh_args(verts, faces, voff, toff, "mesh_occupancy_dev")
    if (np.diff(to) == 0).any():
        raise L.SfmiError("mesh_occupancy_dev: a shape has no faces")
    G = int(grid_dim)
    if G < 1:
        raise L.SfmiError("mesh_occupancy_dev: grid_dim must be >= 1")
    lo, hi = (np.ascontiguousarray(np.asarray(x, np.float64).reshape(3)) for x in bbox)
    dev = on_device("mesh_occupancy_dev", verts, faces)
    B, T = len(to) - 1, faces.shape[0]
    occ = torch.empty(B, G, G, G, device=dev, dtype=torch.uint8)
    status = torch.empty(B, device=dev, dtype=torch.int32)
    vod, tod = torch.from_numpy(vo).to(dev), torch.from_numpy(to).to(dev)
    ws = _workspace(B, B * G ** 3, T, dev)
    L.check(L.lib().sfmi_mesh_occupancy_f32(L.ptr(vf), L.ptr(ff), L.ptr(vod), L.ptr(tod), B, T, G, lo.ctypes.data, hi.ctypes.data,
                                            L.ptr(occ), L.ptr(status), L.ptr(ws), L.stream_ptr()), "sfmi_mesh_occupancy_f32")
    return (occ, status) if return_status else occ


def sdf_sampling_dev(verts, faces, voff, toff, sample_N=64 ** 3, near_std=0.015, far_std=0.2, seed=0):
    """geoutil.SDF_sampling (IF-Net's recipe) for a batch of meshes: Xbd = sample_N area-weighted surface points per shape
    (sample_mesh_dev); Xtg = the first sample_N // 2 of them jittered by near_std, the rest by far_std, any coordinate outside
    +-0.99 replaced by a uniform draw in [-1, 1), then all clipped to +-0.99; Ytg = signed distance of Xtg (negative inside).
    The normals and uniforms come from a counter hash of (seed, k), not from numpy's global RNG: the draws match the reference
    in distribution, not draw for draw, and sample k of a shape does not depend on the batch around it.
    -> Xbd (B, sample_N, 3), Xtg (B, sample_N, 3), Ytg (B, sample_N) float16 (as the reference returns)."""
    vf, ff, vo, to = mesh_args(verts, faces, voff, toff, "sdf_sampling_dev")
    if (np.diff(to) == 0).any():
        raise L.SfmiError("sdf_sampling_dev: a shape has no faces")
    n = int(sample_N)
    if n < 1:
        raise L.SfmiError("sdf_sampling_dev: sample_N must be >= 1")
    dev = on_device("sdf_sampling_dev", verts, faces)
    B = len(to) - 1
    Xbd, st = sample_mesh_dev(vf, ff, vo, to, n, seed=seed)
    Xtg = torch.empty_like(Xbd)
    L.check(L.lib().sfmi_sdf_jitter_f32(L.ptr(Xbd), B, n, n // 2, float(near_std), float(far_std),
                                        (int(seed) * 0x9E3779B97F4A7C15 + 1) & (2 ** 64 - 1), L.ptr(Xtg), L.stream_ptr()),
            "sfmi_sdf_jitter_f32")
    S, _, _, st2 = signed_distance_dev(Xtg, vf, ff, np.arange(B + 1, dtype=np.int64) * n, vo, to)
    bad = ((st != 0) | (st2 != 0)).cpu().numpy()
    if bad.any():
        raise L.SfmiError(f"sdf_sampling_dev: shapes {np.nonzero(bad)[0].tolist()} have a bad vertex index or zero surface area")
    return Xbd.reshape(B, n, 3).half(), Xtg.reshape(B, n, 3).half(), S.reshape(B, n).half()


# ---- reference signatures (numpy in, numpy out) ------------------------------------------------------------------------------

def _one_mesh(vert, face):
    return batch_meshes([(np.asarray(vert).reshape(-1, 3), np.asarray(face).reshape(-1, 3))], torch.device("cuda"))


def _method(method, what):
    if method not in ("brute", "tree"):
        raise L.SfmiError(f"{what}: method must be 'brute' or 'tree', got {method!r}")
    return method


def signed_distance(queries, vert, face, method="brute"):
    """geoutil.signed_distance: (S f64 with NaN -> 0 as np.nan_to_num, I int64 closest face, C (N,3) f64 closest point).
    method "tree": through meshtree's bounding-volume tree: |S|, I and C the same bits, the sign from the tree-code winding number."""
    _method(method, "signed_distance")
    v, f, _, _ = _one_mesh(vert, face)
    q = f32_dev(np.asarray(queries, np.float32).reshape(-1, 3), v.device)
    if method == "tree":
        from . import meshtree
        S, I, C, _ = meshtree.signed_distance_tree_dev(q, meshtree.mesh_tree_dev(v, f))
    else:
        S, I, C, _ = signed_distance_dev(q, v, f)
    return (np.nan_to_num(S.cpu().numpy().astype(np.float64)), I.cpu().numpy().astype(np.int64),
            C.cpu().numpy().astype(np.float64))


def mesh2sdf(vert, face, gridDim=64, disturb=False, method="brute"):
    """geoutil.mesh2sdf: the makeGrid([-1]*3, [1]*3, [gridDim]*3, indexing="ij") lattice (+ U[0, 1/gridDim) per coordinate from
    numpy's global RNG when disturb) and its signed distance -> (gridDim^3, 4) f64 [x, y, z, S].  method "tree": the route for
    gridDim = 256 (geoutil.shape2sdf's high resolution)."""
    from .data import make_grid
    _method(method, "mesh2sdf")
    samples = make_grid([-1, -1, -1.], [1., 1, 1], [gridDim] * 3)
    if disturb:
        samples = samples + np.random.rand(samples.shape[0], 3) / gridDim
    S, _, _ = signed_distance(samples, vert, face, method=method)
    return np.concatenate([samples, S[:, None]], axis=-1)


def SDF_sampling(vert, face, sample_N=64 ** 3, near_std=0.015, far_std=0.2, seed=0):
    """geoutil.SDF_sampling for one mesh -> (Xbd, Xtg, Ytg) float16 numpy; see sdf_sampling_dev (counter-hash draws)."""
    Xbd, Xtg, Ytg = sdf_sampling_dev(*_one_mesh(vert, face), sample_N, near_std, far_std, seed=seed)
    return Xbd[0].cpu().numpy(), Xtg[0].cpu().numpy(), Ytg[0].cpu().numpy()


def normalize_point_set(vert, no_scale=False):
    """geoutil.normalizePointSet (host): centre the bounding box at the origin and, unless no_scale, scale its longest side
    to 2 (coordinates in [-1, 1])."""
    vert = np.asarray(vert)
    bbmax, bbmin = vert.max(axis=0), vert.min(axis=0)
    vert = vert - (bbmax + bbmin) / 2.
    if not no_scale:
        vert = vert / ((bbmax - bbmin).max() / 2.)
    return vert
