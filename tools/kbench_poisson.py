"""Micro-benchmark of the Poisson reconstruction (csrc/poisson.hip, shapeformer_amd/poisson.py; run on the GPU box):
lattices of 65 / 129 / 257 nodes, clouds of 16 384 and 10^6 points on a sphere, 1 and 8 shapes.  Per case three lines:
  splat   poisson_splat_dev (keys, the sort, the cell table, the gather) and poisson_rhs_dev
  solve   poisson_solve_dev to tol = 1e-4: iterations, ms per iteration, and the effective rate of an iteration's 44 bytes per node
          (apply: read p, write q; update: read p q x r, write x r; direction: read r p, write p) against the 6.3 TB/s an MI355X streams
  extract poisson iso-value and subtraction, and marching_cubes_dev on the same lattice (the yardstick: the step every mesh tool has)
Yardstick of splat and solve, the host route (one shape): the copy to the host, a numpy splat (np.add.at over the 8 sites of each of
the four arrays), and scipy.sparse.linalg.cg in f64 on the same system to the same tolerance.  The host route at 257 nodes takes
minutes and runs only with --host-257.
One JSON line per measurement: 1 warm-up + 3 repetitions, device events around whole calls (host work of the call included)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from shapeformer_amd import poisson as P
from shapeformer_amd.mcubes import marching_cubes_dev

dev = torch.device("cuda:0")
HBM_TBS = 6.3                 # measured streaming rate of the micro-architecture guide (8.0 TB/s spec)
BYTES_PER_NODE = 44


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


def line(**kw):
    print(json.dumps(kw), flush=True)


def sphere(rs, n, r=0.5, jitter=0.002):
    u = rs.randn(n, 3)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    return (u * r + rs.randn(n, 3) * jitter).astype(np.float32), u.astype(np.float32)


def host_splat(p, nrm, R):
    """numpy: f64 hat weights, np.add.at over the 8 sites of W, Vx, Vy, Vz"""
    t = (p.astype(np.float64) + 1.0) / (2.0 / (R - 1))
    C = R - 1
    out = [np.zeros((R, R, R)), np.zeros((C, R, R)), np.zeros((R, C, R)), np.zeros((R, R, C))]
    val = [np.ones(len(p)), nrm[:, 0].astype(np.float64), nrm[:, 1].astype(np.float64), nrm[:, 2].astype(np.float64)]
    for a, (o, v) in enumerate(zip(out, val)):
        shift = np.zeros(3)
        if a:
            shift[a - 1] = 0.5
        base = np.floor(t - shift).astype(np.int64)
        for d in range(8):
            s = base + np.array([d >> 2, (d >> 1) & 1, d & 1])
            w = np.maximum(0.0, 1.0 - np.abs(t - shift - s)).prod(1) * v
            ok = ((s >= 0) & (s < np.array(o.shape))).all(1)
            np.add.at(o, tuple(s[ok].T), w[ok])
    return out


def host_route(xt, nt, R, tol):
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    t0 = time.perf_counter()
    p, nrm = xt.cpu().numpy(), nt.cpu().numpy()
    W, Vx, Vy, Vz = host_splat(p, nrm, R)
    px, py, pz = np.pad(Vx, ((1, 1), (0, 0), (0, 0))), np.pad(Vy, ((0, 0), (1, 1), (0, 0))), np.pad(Vz, ((0, 0), (0, 0), (1, 1)))
    b = ((px[1:] - px[:-1]) + (py[:, 1:] - py[:, :-1])) + (pz[:, :, 1:] - pz[:, :, :-1])
    t1 = time.perf_counter()
    T = sp.diags([-np.ones(R - 1), 2.0 * np.ones(R), -np.ones(R - 1)], [-1, 0, 1])
    I = sp.identity(R)
    A = (sp.kron(sp.kron(T, I), I) + sp.kron(sp.kron(I, T), I) + sp.kron(sp.kron(I, I), T)).tocsr()
    t2 = time.perf_counter()
    its = [0]
    def count(_):
        its[0] += 1
    try:
        spla.cg(A, b.ravel(), rtol=tol, atol=0.0, callback=count)
    except TypeError:
        spla.cg(A, b.ravel(), tol=tol, callback=count)
    t3 = time.perf_counter()
    return dict(host_splat_ms=(t1 - t0) * 1e3, host_assemble_ms=(t2 - t1) * 1e3, host_cg_ms=(t3 - t2) * 1e3, host_cg_iterations=its[0])


def case(rs, R, n, B, host):
    pts, nrm = zip(*[sphere(rs, n) for _ in range(B)])
    xt, nt = torch.from_numpy(np.stack(pts)).to(dev), torch.from_numpy(np.stack(nrm)).to(dev)
    tag = dict(R=R, N=n, B=B)
    splat = lambda: P.poisson_rhs_dev(*P.poisson_splat_dev(xt, nt, None, grid_dim=R)[:3])
    ms_splat = gpu_ms(splat)
    rhs = splat()
    ms_solve = gpu_ms(lambda: P.poisson_solve_dev(rhs, tol=1e-4))
    chi, it, res = P.poisson_solve_dev(rhs, tol=1e-4)
    iters = int(it.max())
    per_it = ms_solve / max(iters, 1)
    bytes_it = BYTES_PER_NODE * B * R ** 3
    h = host_route(xt[0], nt[0], R, 1e-4) if host else {}
    line(kernel="poisson_splat_dev+rhs", **tag, ms=ms_splat, **({"host_numpy_ms": h["host_splat_ms"], "x_host": h["host_splat_ms"] * B / ms_splat} if h else {}))
    line(kernel="poisson_solve_dev", **tag, ms=ms_solve, iterations=iters, residual=float(res.max()), ms_per_iteration=per_it,
         GBs_per_iteration=bytes_it / per_it / 1e6, ms_per_iteration_at_hbm_rate=bytes_it / (HBM_TBS * 1e9),
         **({"host_scipy_cg_ms": h["host_cg_ms"], "host_assemble_ms": h["host_assemble_ms"], "host_cg_iterations": h["host_cg_iterations"],
             "x_host": h["host_cg_ms"] * B / ms_solve} if h else {}))
    field, _, _ = P.poisson_field_dev(xt, nt, None, grid_dim=R)
    ms_field = gpu_ms(lambda: P.poisson_field_dev(xt, nt, None, grid_dim=R))
    ms_mc = gpu_ms(lambda: marching_cubes_dev(field, 0.0))
    v, f, _, _ = marching_cubes_dev(field, 0.0)
    ms_recon = gpu_ms(lambda: P.poisson_recon_dev(xt, nt, None, grid_dim=R, quantile=0.1))
    line(kernel="extract", **tag, poisson_field_dev_ms=ms_field, marching_cubes_dev_ms=ms_mc, poisson_recon_dev_q01_ms=ms_recon,
         vertices=int(v.shape[0]), faces=int(f.shape[0]))


rs = np.random.RandomState(0)
for R in (65, 129, 257):
    for n in (16384, 10 ** 6):
        for B in (1, 8):
            case(rs, R, n, B, host=B == 1 and (R < 257 or (n == 16384 and "--host-257" in sys.argv)))
