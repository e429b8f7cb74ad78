"""Micro-benchmark of the mesh signed-distance kernels (csrc/meshsdf.hip; run on the GPU box):
  the 64^3 and 128^3 lattice of one mesh of T = 2 k, 20 k and 100 k faces, as occupancy only (mesh_occupancy_dev: winding
  number, lattice generated in the kernel) and as the full S, I, C form (signed_distance_dev on the explicit lattice), and
  10^5 queries against 20 k faces (fewer query blocks than the chip holds: the faces are split into chunks and merged).
One JSON line per measurement.  The meshes are triangle soups on a sphere: the kernels are branch-free per pair, so the time
depends on the counts, not on the shape.  Rates: pairs / s, and the share of the VALU issue rate (a wave64 VALU instruction
every 2 clocks per SIMD: 256 CUs x 4 SIMDs x 32 lane-ops/clk x 2.4 GHz = 78.6e12 lane-ops/s) at the VALU instructions per pair
counted in the kernels' gfx950 ISA (OPS_FULL, OPS_OCC below: an estimate of the issue cost, not a measured count)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from shapeformer_amd import meshsdf as MS
from shapeformer_amd.data import make_grid

dev = torch.device("cuda:0")
ISSUE = 256 * 4 * 32 * 2.4e9          # VALU lane-ops per second
OPS_FULL, OPS_OCC = 188, 104         # VALU instructions per (query, face) pair in the inner loops (gfx950 ISA)


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


def soup(rs, T, r=0.6):
    c = rs.randn(T, 3)
    c = c / np.linalg.norm(c, axis=1, keepdims=True) * r
    v = (c[:, None, :] + rs.randn(T, 3, 3) * 0.02).reshape(-1, 3).astype(np.float32)
    return torch.from_numpy(v).to(dev), torch.arange(3 * T, dtype=torch.int32, device=dev).reshape(T, 3)


def line(**kw):
    print(json.dumps(kw), flush=True)


def rates(pairs, ms, ops):
    return dict(Gpairs_s=pairs / ms / 1e6, frac_valu_issue=ops * pairs / (ms * 1e-3) / ISSUE)


rs = np.random.RandomState(0)
for T in (2000, 20000, 100000):
    v, f = soup(rs, T)
    vo, to = np.array([0, v.shape[0]]), np.array([0, T])
    for G in (64, 128):
        pairs = G ** 3 * T
        ms = gpu_ms(lambda: MS.mesh_occupancy_dev(v, f, vo, to, grid_dim=G))
        line(kernel="mesh_occupancy", G=G, T=T, ms=ms, **rates(pairs, ms, OPS_OCC))
        X = torch.from_numpy(make_grid([-1, -1, -1.], [1., 1, 1], [G] * 3).astype(np.float32)).to(dev)
        ms = gpu_ms(lambda: MS.signed_distance_dev(X, v, f, None, vo, to))
        line(kernel="signed_distance_SIC", G=G, T=T, ms=ms, **rates(pairs, ms, OPS_FULL))
v, f = soup(rs, 20000)
vo, to = np.array([0, v.shape[0]]), np.array([0, 20000])
q = torch.from_numpy(rs.uniform(-1, 1, (10 ** 5, 3)).astype(np.float32)).to(dev)
ms = gpu_ms(lambda: MS.signed_distance_dev(q, v, f, None, vo, to), n=5)
qblocks = -(-10 ** 5 // 1024) + 1
line(kernel="signed_distance_SIC_split", N=10 ** 5, T=20000, splits=min(-(-2048 // qblocks), 20000 // 64, 64), ms=ms,
     **rates(10 ** 5 * 20000, ms, OPS_FULL))
