"""Build an IMNet2-style training store from a user's meshes (the reference's dataset sampler,
shapeformer/data/imnet_datasets/utils.py:33-70, with the occupancy the IMNet2 stores carry).

    python -m shapeformer_amd.make_dataset MESH... --out ROOT --dataset NAME --split train [--grid 64] [--boundary-n 32768]
                                           [--cate NAME=GLOB ...] [--seed 0] [--batch K]

Each mesh (.obj / .off / .ply) is normalised with normalize_point_set (bounding box centred, longest side 2), then batches of K
meshes go through the device: lattice occupancy (mesh_occupancy_dev on the grid^3 makeGrid lattice of [-1, 1]^3) and area-weighted
surface samples (sample_mesh_dev).  The store is what data.Imnet2LowResDataset reads:

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


def _batch(meshes, dev):
    import torch
    verts = torch.from_numpy(np.concatenate([v for v, _ in meshes]).astype(np.float32)).to(dev)
    faces = torch.from_numpy(np.concatenate([f for _, f in meshes]).astype(np.int32)).to(dev)
    voff = np.concatenate([[0], np.cumsum([len(v) for v, _ in meshes])]).astype(np.int64)
    toff = np.concatenate([[0], np.cumsum([len(f) for _, f in meshes])]).astype(np.int64)
    return verts, faces, voff, toff


def make_dataset(paths, out, dataset, split="train", grid=64, boundary_n=32768, cates=None, seed=0, batch=8, device="cuda:0",
                 log=None):
    """Read, normalise and sample every mesh of `paths`; write the store.  cates: {name: glob} matched against each path."""
    import torch
    from . import meshio, meshsdf
    from .metrics import sample_mesh_dev
    dev = torch.device(device)
    Xbd, occ = [], []
    for s in range(0, len(paths), batch):
        meshes = []
        for p in paths[s:s + batch]:
            v, f = meshio.read_mesh(p)
            if len(f) == 0:
                raise ValueError(f"{p}: no faces")
            meshes.append((meshsdf.normalize_point_set(v), f))
        v, f, voff, toff = _batch(meshes, dev)
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


def main(argv=None):
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
    a = ap.parse_args(argv)
    cates = {}
    for c in a.cate:
        name, sep, g = c.partition("=")
        if not sep or not name:
            ap.error(f"--cate {c!r}: expected NAME=GLOB")
        cates[name] = g
    d = make_dataset(a.meshes, a.out, a.dataset, a.split, a.grid, a.boundary_n, cates, a.seed, max(1, a.batch),
                     log=lambda m: print(m, file=sys.stderr))
    print(d)


if __name__ == "__main__":
    main()
