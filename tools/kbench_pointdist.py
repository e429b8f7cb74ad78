"""Micro-benchmark of the completion-metric kernels (csrc/pointdist.hip; run on the GPU box):
  nn_dist on one 10^5 x 10^5 direction (B = 1, with indices), the 90-direction TMD batch of 10 x 10^5 points, sample_mesh_dev
  for 10 x 10^5 samples from a 128^3 marching-cubes batch, and scipy cKDTree.query (workers = 16) on the same data.
One JSON line per measurement.  FLOPs: 8 per pair (3 sub, 1 mul, 2 fma) against the 157.3 TF f32 peak; VALU lane-ops: 9 per pair
(the 6 arithmetic ops, a compare, 2 selects) against the issue rate of a SIMD-32 (a wave64 VALU instruction every 2 clocks):
256 CUs x 4 SIMDs x 32 lane-ops/clk x 2.4 GHz = 78.6e12 lane-ops/s.  Packed f32 (v_pk_*) moves two per lane but issues at half
the rate, so it does not raise that ceiling."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from scipy.spatial import cKDTree as cKDT

from shapeformer_amd import mcubes, metrics as M

dev = torch.device("cuda:0")
ISSUE = 256 * 4 * 32 * 2.4e9          # VALU lane-ops per second
PEAK_TF = 157.3


def gpu_ms(fn, n=10, warm=3):
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


def sphere(rs, n, r=0.5, jitter=0.002):
    u = rs.randn(n, 3)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    return (u * r + rs.randn(n, 3) * jitter).astype(np.float32)


def line(**kw):
    print(json.dumps(kw), flush=True)


rs = np.random.RandomState(0)
N = 10 ** 5
p, q = sphere(rs, N), sphere(rs, N)
pt, qt = torch.from_numpy(p).to(dev), torch.from_numpy(q).to(dev)
ms = gpu_ms(lambda: M.nn_dist(pt, qt, return_index=True))
pairs = N * N
line(kernel="nn_dist", B=1, N=N, M=N, ms=ms, Gpairs_s=pairs / ms / 1e6, TFLOPs=8 * pairs / ms / 1e9,
     frac_f32_peak=8 * pairs / ms / 1e9 / PEAK_TF, frac_valu_issue=9 * pairs / (ms * 1e-3) / ISSUE)

S = [torch.from_numpy(sphere(rs, N, r=0.45 + 0.01 * i, jitter=0.01)).to(dev) for i in range(10)]
ms = gpu_ms(lambda: M.tmd_directions(S), n=3, warm=1)
pairs = 90 * N * N
line(kernel="tmd_90_directions", k=10, n=N, ms=ms, Gpairs_s=pairs / ms / 1e6, TFLOPs=8 * pairs / ms / 1e9,
     frac_f32_peak=8 * pairs / ms / 1e9 / PEAK_TF, frac_valu_issue=9 * pairs / (ms * 1e-3) / ISSUE)
ms_t = gpu_ms(lambda: M.tmd(S), n=3, warm=1)
line(kernel="tmd_total", k=10, n=N, ms=ms_t)

Q = 128
ax = np.linspace(-1, 1, Q)
X, Y, Z = np.meshgrid(ax, ax, ax, indexing="ij")
occ = np.stack([1 / (1 + np.exp(10 * (np.sqrt(X ** 2 + Y ** 2 + Z ** 2) - (0.3 + 0.05 * i)))) for i in range(10)]).astype(np.float32)
v, f, voff, toff = mcubes.marching_cubes_dev(torch.from_numpy(occ).to(dev), 0.5)
ms = gpu_ms(lambda: M.sample_mesh_dev(v, f, voff, toff, N, seed=1))
line(kernel="sample_mesh_dev", B=10, Q=Q, faces=int(toff[-1]), n=N, ms=ms)

# the reference's method on this host (16 workers), same data
t0 = time.perf_counter()
tree = cKDT(q.astype(np.float64))
tree.query(p.astype(np.float64), k=1, workers=16)
line(kernel="ckdtree_query", N=N, M=N, workers=16, ms=(time.perf_counter() - t0) * 1e3)
Sn = [s.cpu().numpy().astype(np.float64) for s in S]
t0 = time.perf_counter()
trees = [cKDT(s) for s in Sn]
for i in range(10):
    for j in range(10):
        if i != j:
            trees[j].query(Sn[i], k=1, workers=16)
line(kernel="ckdtree_tmd_90_directions", k=10, n=N, workers=16, ms=(time.perf_counter() - t0) * 1e3)
