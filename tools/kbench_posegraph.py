"""Micro-benchmark of multiway registration (csrc/posegraph.hip, shapeformer_amd/registration.py; run on the GPU box):
  the information pass at 1 / 8 / 28 pairs of 16 384 x 16 384 points (kbench_icp's bumpy sphere shell): information_matrix_dev against
  the evaluate_registration_dev call it contains, the pass alone on an evaluated state (a memset and three launches), and
  the host route: the copy, cKDTree with 16 workers, numpy sums;
  the optimiser at S = 6, 16, 32 nodes with full graphs (15 / 120 / 496 edges; tests/posegraph_ref.synthetic with noisy edges and, below the
  edge cap, three false loop closures), 1 and 64 graphs per batch, with and without the line process, against the numpy reference on one graph;
  the whole multiway_registration_dev on 8 scans (sectors of the shell, each overlapping its neighbours by half; all 28 pairs, two
  ICP stages) against the host route: the copy, cKDTree ICP per pair and stage, numpy information matrices, the numpy optimiser.
One JSON line per measurement: 2 warm-ups + 5 repetitions, device events around whole calls (host work of the call included)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import posegraph_ref as P
from shapeformer_amd import registration as G

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
    u = rs.randn(n, 3)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    r = 0.5 + 0.08 * np.sin(7 * u[:, 0]) * np.cos(5 * u[:, 1]) + 0.05 * np.sin(9 * u[:, 2])
    return (u * r[:, None]).astype(np.float32)


def motion(rs, deg, trans):
    ax = rs.randn(3)
    return rodrigues(ax / np.linalg.norm(ax) * np.deg2rad(deg)), rs.randn(3) * trans


# ---- the information pass -------------------------------------------------------------------------------------------------------------

def info_of(p):
    """sum G^T G over the target points p (k,3), G = [-[q]x | I]"""
    L = np.zeros((6, 6))
    L[:3, :3] = (p * p).sum() * np.eye(3) - p.T @ p
    sx, sy, sz = p.sum(0)
    L[:3, 3:] = [[0, -sz, sy], [sz, 0, -sx], [-sy, sx, 0]]
    L[3:, :3] = L[:3, 3:].T
    L[3:, 3:] = len(p) * np.eye(3)
    return L


def host_information_ms(src, tgt, max_dist):
    from scipy.spatial import cKDTree
    t0 = time.perf_counter()
    s, q = src.cpu().numpy().astype(np.float64), tgt.cpu().numpy().astype(np.float64)
    d, j = cKDTree(q).query(s, workers=16)
    L = info_of(q[j[d <= max_dist]])
    return (time.perf_counter() - t0) * 1e3, L


def information_case(rs, B, n, max_dist=0.05):
    src = torch.from_numpy(np.stack([shell(rs, n) for _ in range(B)])).to(dev)
    tgt = torch.from_numpy(np.stack([shell(rs, n) for _ in range(B)])).to(dev)
    ev = gpu_ms(lambda: G.evaluate_registration_dev(src, tgt, max_dist=max_dist))
    full = gpu_ms(lambda: G.information_matrix_dev(src, tgt, max_dist=max_dist))
    info, count, _, _ = G.information_matrix_dev(src, tgt, max_dist=max_dist)
    st = G._Icp("kbench", src, tgt, None, None, max_dist, "point", None, None)
    st.iterate(0, True)
    alone = gpu_ms(lambda: G._information(st), n=20)
    host, L = host_information_ms(src[0], tgt[0], max_dist)
    rel = float(np.abs(info[0].cpu().numpy() - L).max() / np.abs(L).max())
    line(kernel="information_matrix_dev", B=B, N=n, M=n, evaluate_ms=ev, information_ms=full, pass_alone_us=alone * 1e3,
         count=count.tolist()[:4], host_ckdtree_ms_one_pair=host, x_host=host * B / full, rel_diff_to_host=rel)


# ---- the optimiser --------------------------------------------------------------------------------------------------------------------

def optimiser_case(S, Bg, mu):
    gs = [P.synthetic(S, seed=50 + b, noise=1e-3, outliers=3 if S < 32 else 0) for b in range(Bg)]
    no = np.concatenate([[0], np.cumsum([len(g["X0"]) for g in gs])]).astype(np.int64)
    eo = np.concatenate([[0], np.cumsum([len(g["src"]) for g in gs])]).astype(np.int64)
    cat = lambda k: np.concatenate([np.asarray(g[k]) for g in gs])
    X0, src, tgt, unc = cat("X0"), cat("src"), cat("tgt"), cat("unc")
    T, Lam = torch.from_numpy(cat("T")).to(dev), torch.from_numpy(cat("Lam")).to(dev)
    run = lambda **kw: G.pose_graph_optimize_dev(X0, src, tgt, T, Lam, unc, None, no, eo, mu, **kw)
    ms = gpu_ms(run)
    ms0 = gpu_ms(lambda: run(max_iter=0))                      # the checks, one evaluation and the host's share of a call
    _, l, cost, it, st = run()
    t0 = time.perf_counter()
    ref = P.optimize(gs[0]["X0"], gs[0]["src"], gs[0]["tgt"], gs[0]["T"], gs[0]["Lam"], gs[0]["unc"], mu=mu)
    host = (time.perf_counter() - t0) * 1e3
    its = it.cpu().numpy()
    line(kernel="pose_graph_optimize_dev", S=S, E=int(eo[1]), graphs=Bg, mu=mu, ms=ms, ms_max_iter_0=ms0,
         ms_per_iteration=(ms - ms0) / max(int(its.max()), 1), iterations=[int(its.min()), int(its.max())],
         status=sorted(set(st.tolist())), numpy_ms_one_graph=host, numpy_iterations=ref["iterations"], x_numpy=host * Bg / ms)


# ---- the whole pipeline -----------------------------------------------------------------------------------------------------------------

def sector_scans(rs, K, n):
    """K scans of the shell: scan i sees the azimuths [i, i + 2) x 360 / K degrees, in its own frame"""
    clouds, truth = [], []
    for i in range(K):
        p = shell(rs, 5 * n)
        az = (np.degrees(np.arctan2(p[:, 1], p[:, 0])) - i * 360.0 / K) % 360.0
        p = p[az < 2 * 360.0 / K][:n]
        R, t = (np.eye(3), np.zeros(3)) if i == 0 else motion(rs, 3, 0.01)
        clouds.append(((p.astype(np.float64) - t) @ R).astype(np.float32))
        truth.append(np.concatenate([R, t[:, None]], 1).reshape(12))
    return clouds, np.stack(truth)


def host_icp(s, q, tree, pose, max_dist, max_iter=30, tol=1e-6):
    """point-to-point Gauss-Newton on a cKDTree with the device's stopping rule -> pose (12,), fitness"""
    Rm, t = pose.reshape(3, 4)[:, :3], pose.reshape(3, 4)[:, 3]
    pf = pr = None
    fit = 0.0
    for it in range(max_iter + 1):
        a = s @ Rm.T + t
        d, j = tree.query(a, workers=16)
        inl = d <= max_dist
        fit, rm = inl.mean(), np.sqrt((d[inl] ** 2).mean()) if inl.any() else 0.0
        if it == max_iter or inl.sum() < 3 or (it > 0 and abs(fit - pf) < tol and abs(rm - pr) < tol):
            break
        pf, pr = fit, rm
        a, r = a[inl], a[inl] - q[j[inl]]
        J = np.zeros((len(a), 3, 6))
        J[:, 0, 1], J[:, 0, 2], J[:, 1, 0], J[:, 1, 2], J[:, 2, 0], J[:, 2, 1] = a[:, 2], -a[:, 1], -a[:, 2], a[:, 0], a[:, 1], -a[:, 0]
        J[:, 0, 3] = J[:, 1, 4] = J[:, 2, 5] = 1.0
        xi = np.linalg.solve(np.einsum("nri,nrj->ij", J, J), -np.einsum("nri,nr->i", J, r))
        dR = rodrigues(xi[:3]) if np.linalg.norm(xi[:3]) > 0 else np.eye(3)
        Rm, t = dR @ Rm, dR @ t + xi[3:]
    return np.concatenate([Rm, t[:, None]], 1).reshape(12), fit


def host_multiway_ms(clouds, max_dists, min_fitness):
    from scipy.spatial import cKDTree
    t0 = time.perf_counter()
    pts = [c.cpu().numpy().astype(np.float64) for c in clouds]
    trees = [cKDTree(p) for p in pts]
    S = len(pts)
    edges, T, info = [], [], []
    for i, j in P.all_pairs(S):
        pose = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0.0])
        for md in max_dists:
            pose, fit = host_icp(pts[j], pts[i], trees[i], pose, md)
        if fit < min_fitness:
            continue
        a = pts[j] @ pose.reshape(3, 4)[:, :3].T + pose.reshape(3, 4)[:, 3]
        d, k = trees[i].query(a, workers=16)
        info.append(info_of(pts[i][k[d <= max_dists[-1]]]))
        edges.append((i, j)), T.append(pose)
    X, seen = P.chain_poses(S, edges, T)
    g = P.global_optimization(X, [j for _, j in edges], [i for i, _ in edges], np.array(T), np.array(info),
                              [j != i + 1 for i, j in edges], max_dist=max_dists[-1])
    return (time.perf_counter() - t0) * 1e3, g["X"], len(edges)


def multiway_case(rs, K=8, n=8192, max_dists=(0.05, 0.01), min_fitness=0.3):
    clouds, truth = sector_scans(rs, K, n)
    dc = [torch.from_numpy(c).to(dev) for c in clouds]
    ms = gpu_ms(lambda: G.multiway_registration_dev(dc, max_dists=max_dists, min_fitness=min_fitness))
    poses, status, more = G.multiway_registration_dev(dc, max_dists=max_dists, min_fitness=min_fitness)
    err = P.graph_error(poses.cpu().numpy()[:, :3, :].reshape(-1, 12), truth)
    host, X, kept = host_multiway_ms(dc, max_dists, min_fitness)
    line(kernel="multiway_registration_dev", scans=K, points=[len(c) for c in clouds], pairs=len(more["edges"]),
         registered=int(more["registered"].sum()), kept=int(more["kept"].sum()), status=status.tolist(), graph_status=list(more["graph_status"]),
         ms=ms, error=[float(err[0]), float(err[1])], host_ms=host, host_edges=kept,
         host_error=[float(v) for v in P.graph_error(X, truth)], x_host=host / ms)


rs = np.random.RandomState(0)
for B in (1, 8, 28):
    information_case(rs, B, 16384)
for S in (6, 16, 32):
    for Bg in (1, 64):
        optimiser_case(S, Bg, 0.0)
    optimiser_case(S, 64, 40.0)
multiway_case(rs)
