"""Micro-benchmark of the watertight voxelization (csrc/morph.hip, shapeformer_amd/morph.py; run on the GPU box).
One JSON line per measurement (device events around whole calls; 2 warm-up + 10 repetitions, 1 + 3 at 256^3 with 8 shapes):
  mesh: a cube as a triangle soup (every triangle its own vertices, half of them flipped, a square hole in one side, an interior
  partition), scaled differently per shape of a batch;
  settings: the reference's defaults (10^6 samples, 128^3, selem 6) and 256^3 with selem 6, each for one shape and for a batch of 8;
  per setting: the stages sample (sample_mesh_dev), voxelize, dilate, flood, erode (dilate of the flooded region, complemented on the
  way out), unpack to uint8, and the total of morph_voxelization_dev;
  the host route on one core for one shape of the same voxels: device-to-host copy + scipy.ndimage binary_dilation, label,
  binary_erosion with the same ball + the copy back (--no-host skips it), and whether the two routes return the same voxels.
No file dependency."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from shapeformer_amd import morph as M
from shapeformer_amd.metrics import sample_mesh_dev

torch.set_num_threads(1)                  # the host route runs on one core
dev = torch.device("cuda:0")


def line(**kw):
    print(json.dumps(kw), flush=True)


def gpu_ms(fn, n=10, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def soup_cube(n=8):
    """[-0.5, 0.5]^3: n x n quads per side, one quad of the +x side missing, a partition at x = 0, every second triangle flipped"""
    t = np.linspace(-0.5, 0.5, n + 1)
    tris = []
    for axis, x, skip in [(a, s, (n // 2, n // 2) if (a, s) == (0, 0.5) else None) for a in range(3) for s in (-0.5, 0.5)] + [(0, 0.0, None)]:
        u, w = [a for a in range(3) if a != axis]
        for a in range(n):
            for b in range(n):
                if skip == (a, b):
                    continue
                c = np.zeros((4, 3))
                c[:, axis] = x
                c[:, u] = [t[a], t[a + 1], t[a + 1], t[a]]
                c[:, w] = [t[b], t[b], t[b + 1], t[b + 1]]
                tris += [c[[0, 1, 2]], c[[0, 2, 3]]]
    tri = np.asarray(tris, np.float32)
    tri[1::2] = tri[1::2, ::-1]
    v = tri.reshape(-1, 3)
    return v, np.arange(len(v), dtype=np.int32).reshape(-1, 3)


def ball(r):
    a = np.arange(-r, r + 1)
    X, Y, Z = np.meshgrid(a, a, a, indexing="ij")
    return (X * X + Y * Y + Z * Z) <= r * r


def host_route(vox, r):
    """what a caller does today (geoutil.py:396-400 with scipy in skimage's place): copy, dilate, flood, erode, copy back"""
    from scipy import ndimage
    a = vox.cpu().numpy() != 0
    d = ndimage.binary_dilation(a, structure=ball(r))
    lab, _ = ndimage.label(d == d[0, 0, 0], structure=np.ones((3, 3, 3)))
    out = ndimage.binary_erosion(lab != lab[0, 0, 0], structure=ball(r), border_value=1)
    return torch.from_numpy(out.astype(np.uint8)).to(dev)


def report(B, G, r, n, host):
    v, f = soup_cube(24)                                        # the hole: 1/24 of a side, below 2 r cells on both grids
    scales = [1.0 + 0.08 * b for b in range(B)]                 # up to +-0.78: the dilated shell stays clear of the corner voxel
    verts = torch.from_numpy(np.concatenate([v * s for s in scales])).to(dev)
    faces = torch.from_numpy(np.concatenate([f] * B)).to(dev)
    voff, toff = np.arange(B + 1) * len(v), np.arange(B + 1) * len(f)
    reps = dict(n=3, warm=1) if B * G ** 3 > 2 ** 26 else dict(n=10, warm=2)
    pts, _ = sample_mesh_dev(verts, faces, voff, toff, n, seed=0)
    off = np.arange(B + 1, dtype=np.int64) * n
    ws = M._workspace(B, G, r, dev)
    bits = M._voxelize(pts, off, B, G, dev)
    dil = M._dilate(bits, B, G, r, False, False, ws)
    region, status = M._flood(dil, B, G, ws)
    out = M._dilate(region, B, G, r, False, True, ws)
    ms = dict(
        sample=gpu_ms(lambda: sample_mesh_dev(verts, faces, voff, toff, n, seed=0), **reps),
        voxelize=gpu_ms(lambda: M._voxelize(pts, off, B, G, dev), **reps),
        dilate=gpu_ms(lambda: M._dilate(bits, B, G, r, False, False, ws), **reps),
        flood=gpu_ms(lambda: M._flood(dil, B, G, ws), **reps),
        erode=gpu_ms(lambda: M._dilate(region, B, G, r, False, True, ws), **reps),
        unpack=gpu_ms(lambda: M._unpack(out, B, G), **reps),
        total=gpu_ms(lambda: M.morph_voxelization_dev(verts, faces, voff, toff, sampleN=n, grid_dim=G, selem_size=r, seed=0), **reps))
    vox = M.morph_voxelization_dev(verts, faces, voff, toff, sampleN=n, grid_dim=G, selem_size=r, seed=0)
    rec = dict(shapes=B, grid=G, selem=r, samples=n, faces=int(toff[-1]), status=status.cpu().tolist(), filled=[int(x) for x in vox.sum((1, 2, 3))],
               workspace_MiB=ws.numel() / 2 ** 20, ms=ms, ms_total_per_shape=ms["total"] / B)
    if host:
        first = M._unpack(bits, B, G)[0].contiguous()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h = host_route(first, r)
        torch.cuda.synchronize()
        ms_host = (time.perf_counter() - t0) * 1e3
        fill_dev = ms["dilate"] + ms["flood"] + ms["erode"] + ms["unpack"]
        rec.update(ms_host_route_one_core_one_shape=ms_host, same_voxels_as_host_route=bool(torch.equal(h, vox[0])),
                   ms_device_fill_per_shape=fill_dev / B, host_over_device_fill=ms_host / (fill_dev / B))
    line(**rec)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--samples", type=int, default=1_000_000)
    a = ap.parse_args()
    for G in (128, 256):
        for B in (1, 8):
            report(B, G, 6, a.samples, host=not a.no_host and B == 1)
            torch.cuda.empty_cache()
