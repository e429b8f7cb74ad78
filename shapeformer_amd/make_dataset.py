"""Build an IMNet2-style training store from a user's meshes (the reference's dataset sampler,
shapeformer/data/imnet_datasets/utils.py:33-70, with the occupancy the IMNet2 stores carry).

    python -m shapeformer_amd.make_dataset MESH... --out ROOT --dataset NAME --split train [--grid 64] [--boundary-n 32768]
                                           [--cate NAME=GLOB ...] [--seed 0] [--batch K] [--scale 1.0]
                                           [--occupancy winding|morph|poisson] [--morph-grid 128] [--selem 6] [--morph-samples 1000000]
                                           [--poisson-grid m*(grid-1)+1] [--orient tangent] [--winding brute|tree] [--beta 2.0]

Each mesh (.obj / .off / .ply) is normalised with normalize_point_set (bounding box centred, longest side 2) and multiplied by
--scale, then batches of K meshes go through the device: lattice occupancy on the grid^3 makeGrid lattice of [-1, 1]^3 and
area-weighted surface samples (sample_mesh_dev).  --occupancy winding (the default) is mesh_occupancy_dev's inside test |W| > 0.5: for
closed, consistently oriented meshes; --winding tree takes it through meshtree's bounding-volume tree (|W_tree| > 0.5 with far-field
expansions beyond --beta radii), the route for --grid 256.  --occupancy morph is for triangle soups (open shells, interior partitions, doubled and flipped
faces): morph_voxelization_dev's watertight voxels on a --morph-grid^3 grid (closing with a ball of --selem cells over --morph-samples
surface samples), read at each lattice point from the cell that holds it; the outside is flooded from voxel (0,0,0), so a shape that
fills the box needs --scale 0.9 or so to keep that corner empty.  --occupancy poisson is for scans: the inputs are .ply point clouds
with nx/ny/nz normals (pointing outward) and no faces; a cloud is NOT normalised (a scan's bounding box is noise; normalise it upstream,
scan.normalize_scan), only multiplied by --scale; Xbd is the cloud resampled to --boundary-n points and the occupancy is
poisson_field_dev's field > 0 on a --poisson-grid^3 lattice of [-1, 1]^3, which must be m (grid - 1) + 1 nodes per axis so that the
store's lattice is every m-th Poisson node (default: the smallest such lattice of at least 129 nodes).  With --orient tangent a
cloud without normals is accepted: its normals are estimated over 16 neighbours and oriented outward by tangent-plane
propagation (scan.estimate_normals_dev(orient="tangent")); a cloud that has normals keeps them.  The store is what
data.Imnet2LowResDataset reads:

    ROOT/NAME/SPLIT/Xbd.npy          (n, boundary_n, 3) float32 surface samples
    ROOT/NAME/SPLIT/Ytg.npy          (n, grid^3 / 8) uint8 = np.packbits(occupancy.reshape(n, -1), axis=-1)
    ROOT/NAME/SPLIT/cate_<name>.npy  int64 indices of the meshes of each category (a mesh whose path matches GLOB)
"""
from __future__ import annotations

import argparse
import fnmatch
import os
import sys

import numpy as np


OCCUPANCY = ("winding", "morph", "poisson")
WINDING = ("brute", "tree")


def write_imnet_store(root, dataset, split, Xbd, occ, cates=None):
    """Host side of the store: Xbd (n, m, 3), occ (n, G, G, G) or (n, G^3) {0, 1}, cates {name: indices}.  -> the split's dir."""
    Xbd = np.asarray(Xbd, np.float32)
    occ = np.asarray(occ)
    n = Xbd.shape[0]
    if Xbd.ndim != 3 or Xbd.shape[2] != 3:
        raise ValueError(f"Xbd must be (n, m, 3), got {Xbd.shape}")
    if occ.shape[0] != n:
        raise ValueError(f"occ has {occ.shape[0]} shapes, Xbd {n}")
    flat = occ.reshape(n, -1)
    if flat.shape[1] % 8:
        raise ValueError(f"{flat.shape[1]} lattice points per shape: packbits needs a multiple of 8")
    d = os.path.join(root, dataset, split)
    os.makedirs(d, exist_ok=True)
    np.save(os.path.join(d, "Xbd.npy"), Xbd)
    np.save(os.path.join(d, "Ytg.npy"), np.packbits(flat != 0, axis=-1))
    for name, idx in (cates or {}).items():
        idx = np.asarray(idx, np.int64).reshape(-1)
        if idx.size and (idx.min() < 0 or idx.max() >= n):
            raise ValueError(f"cate {name}: index outside [0, {n})")
        np.save(os.path.join(d, f"cate_{name}.npy"), idx)
    return d


def _morph_occupancy(v, f, voff, toff, names, lattice, grid, morph_grid, selem, morph_samples, seed):
    """(B, grid, grid, grid) uint8: the watertight voxel of the cell that holds each lattice point; status (B,) on the device"""
    from . import morph
    vox, st = morph.morph_voxelization_dev(v, f, voff, toff, sampleN=morph_samples, grid_dim=morph_grid, selem_size=selem, seed=seed,
                                           return_status=True)
    seed_set = (st == morph.STATUS_SEED_SET).cpu().numpy()
    if seed_set.any():
        raise ValueError(f"{[names[i] for i in np.nonzero(seed_set)[0]]}: the closed shape reaches the corner voxel (0,0,0) that the "
                         "outside is flooded from; shrink it, e.g. --scale 0.9")
    B = len(names)
    o = morph.voxel_lookup_dev(vox, lattice[None].expand(B, -1, -1))
    return o.reshape(B, grid, grid, grid), st


def check_poisson_grid(grid, poisson_grid=None):
    """-> m with poisson_grid = m (grid - 1) + 1: the store's nodes are every m-th node of the Poisson lattice.  None: the smallest
    such lattice with at least 129 nodes per axis (129 itself for a store of 3, 5, 9, 17, 33, 65 or 129 nodes per axis)"""
    if poisson_grid is None:
        if grid < 2:
            raise ValueError(f"--grid {grid}: --occupancy poisson needs a lattice of at least 2 nodes per axis")
        return max(1, -(-128 // (grid - 1)))
    if grid < 2 or poisson_grid < grid or (poisson_grid - 1) % (grid - 1):
        raise ValueError(f"--poisson-grid {poisson_grid} must be m * (grid - 1) + 1 = m * {grid - 1} + 1 for an integer m >= 1")
    return (poisson_grid - 1) // (grid - 1)


def _poisson_batch(paths, grid, poisson_grid, boundary_n, scale, seed, dev, orient=None):
    """.ply clouds with normals (orient="tangent": or without) -> Xbd (B, boundary_n, 3), occupancy (B, grid, grid, grid) uint8, both on
    the device"""
    import torch
    from . import meshio, poisson
    from .hpr import resample_visible_dev
    m = check_poisson_grid(grid, poisson_grid)
    pts, nrm = [], []
    for p in paths:
        v, _, n = meshio.read_ply(p, with_normals=True)
        if n is None and orient is None:
            raise ValueError(f"{p}: the cloud has no normals (nx/ny/nz): --occupancy poisson needs oriented points")
        if len(v) == 0:
            raise ValueError(f"{p}: no points")
        pts.append(np.asarray(v * scale, np.float32))
        if n is None:                                              # estimated on the device, on the scaled points
            from .scan import estimate_normals_dev
            n = estimate_normals_dev(torch.from_numpy(pts[-1]).to(dev), orient=orient)[0].cpu().numpy()
        nrm.append(np.asarray(n, np.float32))
    off = np.concatenate([[0], np.cumsum([len(p) for p in pts])]).astype(np.int64)
    x, n = torch.from_numpy(np.concatenate(pts)).to(dev), torch.from_numpy(np.concatenate(nrm)).to(dev)
    field = poisson.poisson_field_dev(x, n, off, grid_dim=m * (grid - 1) + 1)[0]
    occ = (field[:, ::m, ::m, ::m] > 0).to(torch.uint8)
    ones = torch.ones(x.shape[0], device=dev, dtype=torch.uint8)
    count = torch.from_numpy(np.diff(off).astype(np.int32)).to(dev)
    return resample_visible_dev(x, off, ones, count, boundary_n, 0., seed), occ


def make_dataset(paths, out, dataset, split="train", grid=64, boundary_n=32768, cates=None, seed=0, batch=8, device="cuda:0",
                 log=None, occupancy="winding", morph_grid=128, selem=6, morph_samples=1_000_000, scale=1.0, poisson_grid=None,
                 orient=None, winding="brute", beta=2.0):
    """Read, normalise and sample every mesh of `paths`; write the store.  cates: {name: glob} matched against each path.
    occupancy: "winding" (mesh_occupancy_dev), "morph" (morph_voxelization_dev on a morph_grid^3 grid, ball of selem cells,
    morph_samples surface samples) or "poisson" (paths are .ply clouds with normals: poisson_field_dev on a poisson_grid^3 lattice);
    scale multiplies the normalised vertices (poisson: the cloud as it is) on every route.  orient="tangent" (poisson only): clouds
    without normals get normals over estimate_normals_dev's default neighbourhood, oriented outward by tangent-plane propagation.
    winding (the "winding" route only): "brute" (mesh_occupancy_dev) or "tree" (meshtree.mesh_occupancy_tree_dev at `beta`, for grids of
    256 and meshes of 10^5 faces)."""
    import torch
    from . import meshio, meshsdf
    from ._ragged import batch_meshes
    from .metrics import sample_mesh_dev
    if occupancy not in OCCUPANCY:
        raise ValueError(f"occupancy = {occupancy!r} must be one of {OCCUPANCY}")
    if not (np.isfinite(scale) and scale > 0):
        raise ValueError(f"scale = {scale!r} must be a positive number")
    if winding not in WINDING:
        raise ValueError(f"winding = {winding!r} must be one of {WINDING}")
    if not (np.isfinite(beta) and beta >= 0):
        raise ValueError(f"beta = {beta!r} must be a number >= 0")
    if occupancy == "poisson":
        check_poisson_grid(grid, poisson_grid)
    if orient not in (None, "tangent") or (orient is not None and occupancy != "poisson"):
        raise ValueError(f"orient = {orient!r} must be None or 'tangent', and goes with occupancy = 'poisson'")
    dev = torch.device(device)
    Xbd, occ = [], []
    lattice = None
    if occupancy == "morph":
        from .data import make_grid
        lattice = torch.from_numpy(make_grid([-1, -1, -1.], [1., 1, 1], [grid] * 3).astype(np.float32)).to(dev)
    for s in range(0, len(paths), batch):
        if occupancy == "poisson":
            x, o = _poisson_batch(paths[s:s + batch], grid, poisson_grid, boundary_n, scale, seed + s, dev, orient)
            occ.append(o.cpu().numpy())
            Xbd.append(x.cpu().numpy())
            if log:
                log(f"[make_dataset] {min(s + batch, len(paths))}/{len(paths)} clouds")
            continue
        meshes = []
        for p in paths[s:s + batch]:
            v, f = meshio.read_mesh(p)
            if len(f) == 0:
                raise ValueError(f"{p}: no faces")
            v = meshsdf.normalize_point_set(v)
            meshes.append((v if scale == 1.0 else v * scale, f))
        v, f, voff, toff = batch_meshes(meshes, dev)
        if occupancy == "morph":
            o, st = _morph_occupancy(v, f, voff, toff, paths[s:s + batch], lattice, grid, morph_grid, selem, morph_samples, seed + s)
        elif winding == "tree":
            from . import meshtree
            o, st = meshtree.mesh_occupancy_tree_dev(meshtree.mesh_tree_dev(v, f, voff, toff), grid_dim=grid, beta=float(beta), return_status=True)
        else:
            o, st = meshsdf.mesh_occupancy_dev(v, f, voff, toff, grid_dim=grid, return_status=True)
        x, st2 = sample_mesh_dev(v, f, voff, toff, boundary_n, seed=seed + s)
        bad = ((st != 0) | (st2 != 0)).cpu().numpy()
        if bad.any():
            raise ValueError(f"{[paths[s + i] for i in np.nonzero(bad)[0]]}: a vertex index outside the mesh or zero surface area")
        occ.append(o.cpu().numpy())
        Xbd.append(x.reshape(len(meshes), boundary_n, 3).cpu().numpy())
        if log:
            log(f"[make_dataset] {min(s + batch, len(paths))}/{len(paths)} meshes")
    ci = {name: [i for i, p in enumerate(paths) if fnmatch.fnmatch(p, g)] for name, g in (cates or {}).items()}
    return write_imnet_store(out, dataset, split, np.concatenate(Xbd), np.concatenate(occ), ci)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m shapeformer_amd.make_dataset", description=__doc__.split("\n\n")[0])
    ap.add_argument("meshes", nargs="+", help=".obj / .off / .ply files")
    ap.add_argument("--out", required=True, help="store root")
    ap.add_argument("--dataset", required=True)
    ap.add_argument("--split", default="train")
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--boundary-n", type=int, default=32768)
    ap.add_argument("--cate", action="append", default=[], metavar="NAME=GLOB")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--occupancy", choices=OCCUPANCY, default="winding",
                    help="winding: |W| > 0.5, for closed oriented meshes; morph: watertight voxelization, for triangle soups; "
                         "poisson: Poisson reconstruction of .ply point clouds with normals")
    ap.add_argument("--winding", choices=WINDING, default="brute",
                    help="winding: brute force over the faces, or the bounding-volume tree with far-field expansions (--grid 256, large meshes)")
    ap.add_argument("--beta", type=float, default=2.0, help="--winding tree: a node farther than beta radii is approximated")
    ap.add_argument("--poisson-grid", type=int, default=None,
                    help="poisson: nodes per axis of the Poisson lattice, m * (grid - 1) + 1 (default: the smallest such >= 129)")
    ap.add_argument("--orient", choices=("tangent",), default=None,
                    help="poisson: accept clouds without normals; estimate them and orient them outward by tangent-plane propagation")
    ap.add_argument("--morph-grid", type=int, default=128, help="morph: voxels per axis of the watertight grid")
    ap.add_argument("--selem", type=int, default=6, help="morph: radius in voxels of the closing's ball (0 .. 16)")
    ap.add_argument("--morph-samples", type=int, default=1_000_000, help="morph: surface samples per mesh")
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies the normalised vertices (both routes)")
    a = ap.parse_args(argv)
    if a.morph_grid < 1 or a.morph_samples < 1:
        ap.error("--morph-grid and --morph-samples must be >= 1")
    if not 0 <= a.selem <= 16:
        ap.error("--selem must lie in [0, 16]")
    if not (np.isfinite(a.scale) and a.scale > 0):
        ap.error("--scale must be a positive number")
    if not (np.isfinite(a.beta) and a.beta >= 0):
        ap.error("--beta must be a number >= 0")
    if a.occupancy == "poisson":
        try:
            check_poisson_grid(a.grid, a.poisson_grid)
        except ValueError as e:
            ap.error(str(e))
    if a.orient is not None and a.occupancy != "poisson":
        ap.error("--orient goes with --occupancy poisson")
    cates = {}
    for c in a.cate:
        name, sep, g = c.partition("=")
        if not sep or not name:
            ap.error(f"--cate {c!r}: expected NAME=GLOB")
        cates[name] = g
    a.cates = cates
    return a


def main(argv=None):
    a = parse_args(argv)
    d = make_dataset(a.meshes, a.out, a.dataset, a.split, a.grid, a.boundary_n, a.cates, a.seed, max(1, a.batch),
                     log=lambda m: print(m, file=sys.stderr), occupancy=a.occupancy, morph_grid=a.morph_grid, selem=a.selem,
                     morph_samples=a.morph_samples, scale=a.scale, poisson_grid=a.poisson_grid, orient=a.orient, winding=a.winding,
                     beta=a.beta)
    print(d)


if __name__ == "__main__":
    main()
