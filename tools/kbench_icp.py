"""Micro-benchmark of iterative closest point (csrc/register.hip, shapeformer_amd/registration.py; run on the GPU box):
  1 and 8 pairs of 16 384 x 16 384 points and 1 pair of 65 536 x 65 536 (a sphere shell with noise, the source a disjoint sample of
  it moved by 5 degrees and 0.02), both metrics, the plane metric's normals from estimate_normals_dev on the target;
  ms per iteration = (a call of 9 iterations - a call of 1) / 8 with the stopping rule off; its split into search, sums and update is
  the kernel trace's (profiles/r22_icp_kernel_trace.txt); one evaluation (max_iter = 0) and a call on empty sources (begin, update and
  the host's share of a call) as whole calls;
  the search against metrics.nn_dist on the same sizes (the same tiled search without the pose);
  the whole call (max_iter = 30) against the host route: the copy to the host, scipy cKDTree with 16 workers for the
  correspondences, numpy for the sums and the solve (point metric), the same stopping rule.
One JSON line per measurement: 2 warm-ups + 5 repetitions, device events around whole calls (host work of the call included)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from shapeformer_amd import metrics, registration as G, scan

dev = torch.device("cuda:0")


def gpu_ms(fn, n=5, warm=2):
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


def rodrigues(w):
    t = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) + np.sin(t) / t * K + (1 - np.cos(t)) / t ** 2 * (K @ K)


def shell(rs, n):
    """points on a bumpy sphere shell"""
    u = rs.randn(n, 3)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    r = 0.5 + 0.08 * np.sin(7 * u[:, 0]) * np.cos(5 * u[:, 1]) + 0.05 * np.sin(9 * u[:, 2])
    return (u * r[:, None]).astype(np.float32)


def pair(rs, n):
    tgt, s = shell(rs, n), shell(rs, n)
    ax = rs.randn(3)
    R, t = rodrigues(ax / np.linalg.norm(ax) * np.deg2rad(5)), rs.randn(3) * 0.02
    return ((s.astype(np.float64) - t) @ R).astype(np.float32), tgt


def host_icp_ms(src, tgt, max_dist, max_iter=30, tol=1e-6):
    """the copy, cKDTree (16 workers) and numpy: point-to-point Gauss-Newton with the device's stopping rule"""
    from scipy.spatial import cKDTree
    t0 = time.perf_counter()
    s, q = src.cpu().numpy().astype(np.float64), tgt.cpu().numpy().astype(np.float64)
    tree = cKDTree(q)
    R, t = np.eye(3), np.zeros(3)
    pf = pr = None
    it = 0
    for it in range(max_iter + 1):
        a = s @ R.T + t
        d, j = tree.query(a, workers=16)
        inl = d <= max_dist
        fit, rm = inl.mean(), np.sqrt((d[inl] ** 2).mean()) if inl.any() else 0.0
        if it == max_iter or (it > 0 and abs(fit - pf) < tol and abs(rm - pr) < tol):
            break
        pf, pr = fit, rm
        a, r = a[inl], a[inl] - q[j[inl]]
        J = np.zeros((len(a), 3, 6))
        J[:, 0, 1], J[:, 0, 2], J[:, 1, 0], J[:, 1, 2], J[:, 2, 0], J[:, 2, 1] = a[:, 2], -a[:, 1], -a[:, 2], a[:, 0], a[:, 1], -a[:, 0]
        J[:, 0, 3] = J[:, 1, 4] = J[:, 2, 5] = 1.0
        xi = np.linalg.solve(np.einsum("nri,nrj->ij", J, J), -np.einsum("nri,nr->i", J, r))
        dR = rodrigues(xi[:3]) if np.linalg.norm(xi[:3]) > 0 else np.eye(3)
        R, t = dR @ R, dR @ t + xi[3:]
    return (time.perf_counter() - t0) * 1e3, it


def case(rs, B, n, max_dist=0.05):
    ps = [pair(rs, n) for _ in range(B)]
    src, tgt = (torch.from_numpy(np.stack([p[k] for p in ps])).to(dev) for k in range(2))
    nrm = scan.estimate_normals_dev(tgt)[0]
    nn_ms = gpu_ms(lambda: metrics.nn_dist(src, tgt, return_index=True))
    for metric in ("point", "plane"):
        kw = dict(metric=metric, target_normals=nrm if metric == "plane" else None)
        ev = gpu_ms(lambda: G.icp_dev(src, tgt, max_dist=max_dist, max_iter=0, **kw))       # search + sums + update
        empty = gpu_ms(lambda: G.icp_dev(src[:, :0], tgt, max_dist=max_dist, max_iter=0, **kw))  # begin + update + the host's share
        k = 8
        it1 = gpu_ms(lambda: G.icp_dev(src, tgt, max_dist=max_dist, max_iter=1, rel_fitness=0.0, rel_rmse=0.0, check_every=64, **kw))
        itk = gpu_ms(lambda: G.icp_dev(src, tgt, max_dist=max_dist, max_iter=1 + k, rel_fitness=0.0, rel_rmse=0.0, check_every=64, **kw))
        per_it = (itk - it1) / k
        full = gpu_ms(lambda: G.icp_dev(src, tgt, max_dist=max_dist, **kw))
        pose, fit, rmse, its, status = G.icp_dev(src, tgt, max_dist=max_dist, **kw)
        rec = dict(kernel="icp_dev", metric=metric, B=B, N=n, M=n, max_dist=max_dist, ms_per_iteration=per_it, nn_dist_ms=nn_ms,
                   evaluate_ms=ev, empty_call_ms=empty,
                   pair_tests_per_s=B * n * n / (per_it * 1e-3), icp_ms=full, iterations=its.tolist(), status=status.tolist(),
                   fitness=[round(float(f), 4) for f in fit], rmse=[round(float(r), 6) for r in rmse])
        if metric == "point":
            host, hit = host_icp_ms(src[0], tgt[0], max_dist)
            rec.update(host_ckdtree_ms_one_pair=host, host_iterations=hit, x_host=host * B / full)
        line(**rec)


rs = np.random.RandomState(0)
case(rs, 1, 16384)
case(rs, 8, 16384)
case(rs, 1, 65536)
