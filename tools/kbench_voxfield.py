"""Micro-benchmark of the voxel fields (csrc/edt.hip, shapeformer_amd/voxfield.py; run on the GPU box).
One JSON line per measurement (device events around whole calls on bit sets that are already packed; 1 warm-up + 3 repetitions, 1 + 1
from 2^28 voxels on):
  grids: voxelised spheres of radius 0.30 G to 0.37 G, off centre, one per shape of a batch;
  sizes: 128^3, 256^3, 513^3, each for one grid and for a batch of 8;
  cases: the squared distance transform (to the set and to the clear voxels), the signed distance, the Gaussian with sigma 1 and 3,
  the constrained solve (compaction alone = 0 iterations, and ms per iteration from 20 iterations; band and support sizes), the whole
  voxels2mesh_dev with its defaults (200 iterations), and marching_cubes_dev alone on the binary grid at 0.5;
  the host route on the machine's cores as numpy / scipy use them, for ONE grid at 128^3 and 256^3 (--host-max): device-to-host copy, then
  scipy.ndimage.distance_transform_edt twice + the square roots, gaussian_filter with sigma 1 and 3, and the numpy iteration of
  tests/voxfield_ref.py (ms per iteration from 3), and whether the device's signed distance equals the host's."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

from shapeformer_amd import mcubes as MC
from shapeformer_amd import morph as M
from shapeformer_amd import voxfield as V

dev = torch.device("cuda:0")


def line(**kw):
    print(json.dumps(kw), flush=True)


def gpu_ms(fn, n=3, warm=1):
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


def spheres(B, G):
    a = torch.arange(G, device=dev, dtype=torch.float32)
    out = torch.empty(B, G, G, G, device=dev, dtype=torch.uint8)
    for b in range(B):
        r, c = (0.30 + 0.01 * b) * G, [(G - 1) / 2 + 0.3 + b, (G - 1) / 2 - 0.2, (G - 1) / 2 + 0.1 - b]
        out[b] = ((a[:, None, None] - c[0]) ** 2 + (a[None, :, None] - c[1]) ** 2 + (a[None, None, :] - c[2]) ** 2 <= r * r).to(torch.uint8)
    return out


def host_ms(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def report(B, G, host):
    from scipy import ndimage
    import voxfield_ref as R
    vox = spheres(B, G)
    NV = B * G ** 3
    reps = dict(n=1, warm=1) if NV >= 2 ** 28 else dict(n=3, warm=1)
    bits = M._pack(vox, B, G)
    d, status = V._signed(bits, B, G)
    u, ws = V._constrained(bits, d, B, G, 4.0, 0, return_ws=True)
    band, sup = V._band_lists(ws, B, G)
    n_band, n_sup = len(band), len(sup)
    del u, ws, band, sup
    w1, w3 = V.gaussian_weights(1.0), V.gaussian_weights(3.0)
    ms = dict(
        pack=gpu_ms(lambda: M._pack(vox, B, G), **reps),
        edt_to_set=gpu_ms(lambda: V._edt_sq(bits, B, G, 0), **reps),
        edt_to_clear=gpu_ms(lambda: V._edt_sq(bits, B, G, 1), **reps),
        signed=gpu_ms(lambda: V._signed(bits, B, G), **reps),
        gaussian_sigma1=gpu_ms(lambda: V._gaussian(bits, B, G, *w1), **reps),
        gaussian_sigma3=gpu_ms(lambda: V._gaussian(bits, B, G, *w3), **reps),
        compaction=gpu_ms(lambda: V._constrained(bits, d, B, G, 4.0, 0), **reps))
    ms["solve_per_iteration"] = (gpu_ms(lambda: V._constrained(bits, d, B, G, 4.0, 20), **reps) - ms["compaction"]) / 20
    # marching cubes indexes 3 B G^3 in 32 bits: a batch beyond that is meshed grid by grid
    parts = [vox] if 3 * NV < 2 ** 31 else [vox[b] for b in range(B)]
    ms["marching_cubes_binary"] = gpu_ms(lambda: [MC.marching_cubes_dev(p.reshape(-1, G, G, G).float(), 0.5) for p in parts], **reps)
    ms["voxels2mesh_constrained_200"] = gpu_ms(lambda: [V.voxels2mesh_dev(p) for p in parts], **reps)
    ms["voxels2mesh_gaussian_sigma1"] = gpu_ms(lambda: [V.voxels2mesh_dev(p, "gaussian", sigma=1.0) for p in parts], **reps)
    meshes = [V.voxels2mesh_dev(p) for p in parts]
    rec = dict(grids=B, grid=G, status=status.cpu().tolist(), band=n_band, support=n_sup, band_share=n_band / NV,
               mesh_calls=len(parts), verts=sum(int(m[2][-1]) for m in meshes), faces=sum(int(m[3][-1]) for m in meshes),
               ms={k: round(x, 4) for k, x in ms.items()}, ms_voxels2mesh_per_grid=ms["voxels2mesh_constrained_200"] / B)
    del meshes
    if host:
        torch.cuda.synchronize()
        t_copy, g = host_ms(lambda: vox[0].cpu().numpy() != 0)
        t_edt, hd = host_ms(lambda: R.signed_distance(g, np.rint(ndimage.distance_transform_edt(g) ** 2),
                                                      np.rint(ndimage.distance_transform_edt(~g) ** 2)))
        t_g1, _ = host_ms(lambda: R.gaussian(g, 1.0))
        t_g3, _ = host_ms(lambda: R.gaussian(g, 3.0))
        bandh = R.band_of(hd)

        def three():
            x = hd
            for _ in range(3):
                x = R.constrained_step(x, hd, g, bandh)
            return x
        t_it, _ = host_ms(three)
        hms = dict(copy=t_copy, signed=t_edt, gaussian_sigma1=t_g1, gaussian_sigma3=t_g3, solve_per_iteration=t_it / 3)
        per = {k: ms[k] / B for k in ("signed", "gaussian_sigma1", "gaussian_sigma3", "solve_per_iteration")}
        rec.update(host_threads=torch.get_num_threads(), ms_host_one_grid={k: round(x, 3) for k, x in hms.items()},
                   signed_equals_host=bool(np.array_equal(d[0].cpu().numpy(), hd)),
                   host_over_device_per_grid={k: round((hms[k] + (t_copy if k != "solve_per_iteration" else 0.0)) / per[k], 1) for k in per},
                   ms_host_route_constrained_200=round(t_copy + t_edt + 200 * t_it / 3, 1))
    line(**rec)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256, 513])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--host-max", type=int, default=256, help="the largest grid for which the host route is timed (0: never)")
    a = ap.parse_args()
    for G in a.sizes:
        for B in a.batches:
            report(B, G, host=B == 1 and G <= a.host_max)
            torch.cuda.empty_cache()
