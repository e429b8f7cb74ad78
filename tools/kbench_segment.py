"""Micro-benchmark of plane scoring, Euclidean clustering and isolate_object_dev (csrc/segment.hip, shapeformer_amd/scan.py; DESIGN.md
§5.17; run on the GPU box):
  plane scoring (segment_plane_dev, scoring + refit) with H = 1024 at 1 x 16 384, 8 x 16 384 and 1 x 10^6 points, H = 4096 at 10^6;
  clusters at 1 x 16 384 and 1 x 65 536 points: sparse (uniform points, about one neighbour each: many clusters), one blob (a ball
  whose points have 0.3 % of the set within the radius: one cluster, many edges) and, at 16 384, every pair within the radius (the
  most contended case for the union-find; no host figure: the pair list alone would be 2 GB);
  isolate_object_dev on a 10^6-point scan (floor, object, outliers) after voxel_downsample_dev(voxel=0.01).
Yardsticks, the host routes: scoring = the copy to the host plus the numpy statement of the contract (tests/segment_ref.py's
expression, vectorised over the points) on the first 64 hypotheses, scaled to H; clusters = the copy plus scipy cKDTree.query_pairs
plus scipy.sparse.csgraph.connected_components.
One JSON line per measurement: 2 warm-ups + 5 repetitions, device events around whole calls (host work of the call included)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from shapeformer_amd import scan

dev = torch.device("cuda:0")
HOST_H = 64


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


def room(rs, n, floor=0.6, outliers=0.01):
    """a floor at y = -0.4 (jitter 0.002), a sphere shell of radius 0.3 on the origin, uniform outliers"""
    n_f, n_o = int(n * floor), int(n * outliers)
    n_s = n - n_f - n_o
    fl = np.stack([rs.uniform(-0.8, 0.8, n_f), -0.4 + rs.randn(n_f) * 0.002, rs.uniform(-0.8, 0.8, n_f)], 1)
    u = rs.randn(n_s, 3)
    sp = 0.3 * u / np.linalg.norm(u, axis=1, keepdims=True) + rs.randn(n_s, 3) * 0.001
    p = np.concatenate([fl, sp, rs.uniform(-0.9, 0.9, (n_o, 3))]).astype(np.float32)
    return p[rs.permutation(n)]


def host_score_ms(xt, triples, thr, H):
    """the copy, then per set and hypothesis the contract's expression over all points; HOST_H hypotheses timed, scaled to H"""
    t0 = time.perf_counter()
    x = xt.cpu().numpy().astype(np.float64)
    for b in range(x.shape[0]):
        p = x[b]
        for t in triples[b, :HOST_H]:
            p0, u, v = p[t[0]], p[t[1]] - p[t[0]], p[t[2]] - p[t[0]]
            n = np.array([u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]])
            nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
            d = (n[0] * p0[0] + n[1] * p0[1]) + n[2] * p0[2]
            s = ((n[0] * p[:, 0] + n[1] * p[:, 1]) + n[2] * p[:, 2]) - d
            int((s * s <= thr * thr * nn).sum())
    return (time.perf_counter() - t0) * 1e3 * H / HOST_H


def score_case(rs, B, n, H, thr=0.01):
    xt = torch.from_numpy(np.stack([room(rs, n) for _ in range(B)])).to(dev)
    tr = scan.plane_hypotheses([n] * B, H, 0)
    trd = torch.from_numpy(tr).to(dev)
    ms = gpu_ms(lambda: scan.segment_plane_dev(xt, None, thr, triples=trd))
    host = host_score_ms(xt, tr, thr, H)
    n_in = scan.segment_plane_dev(xt, None, thr, triples=trd)[2]
    line(kernel="segment_plane_dev", B=B, N=n, H=H, ms=ms, pair_tests_per_s=B * n * H / (ms * 1e-3), host_numpy_ms=host, x_host=host / ms,
         host_hypotheses_timed=HOST_H, n_in=int(n_in[0]))


def host_cluster_ms(xt, radius):
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree
    t0 = time.perf_counter()
    p = xt.cpu().numpy().astype(np.float64)
    pairs = cKDTree(p).query_pairs(radius, output_type="ndarray")
    n = len(p)
    k, _ = connected_components(csr_matrix((np.ones(len(pairs), np.int8), (pairs[:, 0], pairs[:, 1])), shape=(n, n)), directed=False)
    return (time.perf_counter() - t0) * 1e3, k, len(pairs)


def cluster_case(rs, n, kind):
    if kind == "sparse":
        p, radius = rs.uniform(0, 1, (n, 3)), (3.0 / (4.0 * np.pi * n)) ** (1.0 / 3.0)
    else:
        u = rs.randn(n, 3)
        p = u / np.linalg.norm(u, axis=1, keepdims=True) * rs.uniform(0, 1, (n, 1)) ** (1.0 / 3.0)
        radius = 0.15 if kind == "blob" else 2.5
    xt = torch.from_numpy(p.astype(np.float32)).to(dev)
    ms = gpu_ms(lambda: scan.euclidean_clusters_dev(xt, None, radius))
    clusters = int(scan.euclidean_clusters_dev(xt, None, radius)[2][-1])
    if kind == "all_pairs":
        line(kernel="euclidean_clusters_dev", case=kind, N=n, radius=radius, clusters=clusters, ms=ms, pair_tests_per_s=n * n / 2 / (ms * 1e-3))
        return
    host, k, pairs = host_cluster_ms(xt, radius)
    line(kernel="euclidean_clusters_dev", case=kind, N=n, radius=radius, clusters=clusters, host_clusters=k, edges=pairs, ms=ms,
         pair_tests_per_s=n * n / 2 / (ms * 1e-3), host_ckdtree_ms=host, x_host=host / ms)


def isolate_case(rs, n=10 ** 6):
    xt = torch.from_numpy(room(rs, n)).to(dev)
    def f():
        v, vo, _, _ = scan.voxel_downsample_dev(xt, None, 0.01)
        return v, scan.isolate_object_dev(v, vo, 0.01, 0.03)
    ms = gpu_ms(f)
    vms = gpu_ms(lambda: scan.voxel_downsample_dev(xt, None, 0.01))
    v, (kept, k_off, _, planes, _) = f()
    line(kernel="voxel_downsample_dev + isolate_object_dev", N=n, voxel=0.01, voxels=int(v.shape[0]), kept=int(k_off[-1]), ms=ms,
         voxel_ms=vms, isolate_ms=ms - vms, plane=[round(float(c), 5) for c in planes[0, 0].cpu()])


rs = np.random.RandomState(0)
score_case(rs, 1, 16384, 1024)
score_case(rs, 8, 16384, 1024)
score_case(rs, 1, 10 ** 6, 1024)
score_case(rs, 1, 10 ** 6, 4096)
for n in (16384, 65536):
    cluster_case(rs, n, "sparse")
    cluster_case(rs, n, "blob")
cluster_case(rs, 16384, "all_pairs")
isolate_case(rs)
