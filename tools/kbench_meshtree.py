"""Micro-benchmark of the mesh tree (csrc/meshtree.hip; run on the GPU box) against the brute route (csrc/meshsdf.hip) at the same sizes:
  the tree build; lattice occupancy at 64^3, 128^3 and 256^3 of latitude-longitude spheres of 2 k, 20 k and 100 k faces, 1 and 8
  shapes, beta = 2 and 3, with the faces evaluated and the expansions taken per lattice point; 10^5 near-surface free queries; and the
  host route (numpy f64 brute force, tests/meshsdf_ref.py) on a slice, as pairs per second.
One JSON line per measurement.  HIP events; 2 timed calls after 1 warm-up, 1 cold call where a call takes seconds (`calls` says which).
A brute measurement that would take more than ~10 s is not run: its line carries `estimated_ms` from the measured pair rate."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

from shapeformer_amd import meshsdf as MS
from shapeformer_amd import meshtree as MT
from shapeformer_amd._ragged import batch_meshes

dev = torch.device("cuda:0")


def gpu_ms(fn, n=2, warm=1):
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


def uv_sphere(nu, nv, r=0.8):
    th = np.pi * np.arange(nv + 1) / nv
    ph = 2 * np.pi * np.arange(nu) / nu
    v = np.stack([r * np.sin(th)[:, None] * np.cos(ph)[None], r * np.sin(th)[:, None] * np.sin(ph)[None],
                  r * np.cos(th)[:, None] * np.ones(nu)[None]], -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(nv), np.arange(nu), indexing="ij")
    a, b, c, d = i * nu + j, (i + 1) * nu + j, (i + 1) * nu + (j + 1) % nu, i * nu + (j + 1) % nu
    f = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])
    return v.astype(np.float32), f.astype(np.int32)


def line(**kw):
    print(json.dumps(kw), flush=True)


SIZES = {2000: (50, 20), 20000: (200, 50), 100000: (500, 100)}
brute_rate = 385e9                                                       # pairs / s of the occupancy form, updated as it is measured
for T, (nu, nv) in SIZES.items():
    mesh = uv_sphere(nu, nv)
    for B in (1, 8):
        # B copies scaled a little apart: every shape has its own tree
        v, f, vo, to = batch_meshes([(mesh[0] * (1 - 0.01 * b), mesh[1]) for b in range(B)], dev)
        ms_build = gpu_ms(lambda: MT.mesh_tree_dev(v, f, vo, to))
        tree = MT.mesh_tree_dev(v, f, vo, to)
        line(kernel="mesh_tree_build", T=T, B=B, nodes=int(tree.noff[1]), ms=ms_build)
        for G in (64, 128, 256):
            pairs = B * G ** 3 * T
            est = pairs / brute_rate * 1e3
            if est > 10e3:
                line(kernel="mesh_occupancy_brute", G=G, T=T, B=B, estimated_ms=est, calls="not run: estimated from the measured pair rate")
                ms_brute = None
            else:
                cold = est > 500
                ms_brute = gpu_ms(lambda: MS.mesh_occupancy_dev(v, f, vo, to, grid_dim=G), n=1 if cold else 2, warm=0 if cold else 1)
                if pairs > 1e10:
                    brute_rate = pairs / (ms_brute * 1e-3)
                line(kernel="mesh_occupancy_brute", G=G, T=T, B=B, ms=ms_brute, Gpairs_s=pairs / ms_brute / 1e6, calls="1 cold" if cold else "2 after 1 warm-up")
            for beta in (2.0, 3.0):
                ms = gpu_ms(lambda: MT.mesh_occupancy_tree_dev(tree, grid_dim=G, beta=beta))
                cnt = torch.zeros(3, device=dev, dtype=torch.int64)
                occ = MT.mesh_occupancy_tree_dev(tree, grid_dim=G, beta=beta, counters=cnt)
                c = cnt.cpu().numpy()
                row = dict(kernel="mesh_occupancy_tree", G=G, T=T, B=B, beta=beta, ms=ms, ms_with_build=ms + ms_build,
                           faces_per_query=c[0] / c[2], expansions_per_query=c[1] / c[2], inside=float(occ.float().mean()))
                if ms_brute is not None:
                    row["brute_over_tree_with_build"] = ms_brute / (ms + ms_build)
                    if est <= 2000:
                        row["points_that_differ_from_brute"] = int((occ != MS.mesh_occupancy_dev(v, f, vo, to, grid_dim=G)).sum().item())
                else:
                    row["estimated_brute_over_tree_with_build"] = est / (ms + ms_build)
                line(**row)
        del tree

# free queries: 10^5 points near the surface
rs = np.random.RandomState(0)
for T in (20000, 100000):
    mv, mf = uv_sphere(*SIZES[T])
    v, f, vo, to = batch_meshes([(mv, mf)], dev)
    q = torch.from_numpy((mv[rs.randint(0, len(mv), 10 ** 5)] + rs.randn(10 ** 5, 3) * 0.01).astype(np.float32)).to(dev)
    tree = MT.mesh_tree_dev(v, f, vo, to)
    ms_brute = gpu_ms(lambda: MS.signed_distance_dev(q, v, f, None, vo, to))
    for beta in (2.0, 3.0):
        ms = gpu_ms(lambda: MT.signed_distance_tree_dev(q, tree, beta=beta))
        cnt = torch.zeros(3, device=dev, dtype=torch.int64)
        MT.signed_distance_tree_dev(q, tree, beta=beta, counters=cnt)
        c = cnt.cpu().numpy()
        line(kernel="signed_distance_tree", N=10 ** 5, T=T, beta=beta, ms=ms, ms_brute=ms_brute, faces_per_query=c[0] / c[2],
             expansions_per_query=c[1] / c[2], note="ms includes the host-side Morton sort of the queries and the permutation back")

# the host route: the copy of one 2 k mesh and numpy f64 brute force on 256 lattice points
import meshsdf_ref as R   # noqa: E402
mv, mf = uv_sphere(*SIZES[2000])
v, f, vo, to = batch_meshes([(mv, mf)], dev)
t0 = time.perf_counter()
hv, hf = v.cpu().numpy(), f.cpu().numpy()
R.brute(np.random.RandomState(1).uniform(-1, 1, (256, 3)), hv.astype(np.float64), hf)
dt = time.perf_counter() - t0
line(kernel="host_brute_f64", N=256, T=len(mf), s=dt, pairs_per_s=256 * len(mf) / dt, s_for_256cubed_100k=256 ** 3 * 1e5 / (256 * len(mf) / dt))
