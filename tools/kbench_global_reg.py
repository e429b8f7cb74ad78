"""Micro-benchmark of global registration (csrc/features.hip, csrc/global_register.hip, shapeformer_amd/registration.py; DESIGN.md §5.19;
run on the GPU box):
  1 and 8 pairs of 4096 and 16 384 points (a bumpy sphere shell, the source a disjoint sample of it moved by 90 degrees and 0.02);
  knn_dev (k = 32, the neighbourhood of the features), fpfh_dev (knn + SPFH + FPFH), the SPFH and FPFH launches alone on given
  neighbour rows, and the oriented normals (knn with k = 16, PCA, the turn away from the centroid); the feature search alone with 2
  and 4 queries per lane, in ms and pair tests / s, against metrics.nn_dist on the same sizes (the 3-D search: the same tiling with
  3 floats per row); hypothesis poses and scoring at H = 4096 and 65 536; the refit; the whole call (global_registration_dev without a voxel
  reduction, max_dist 0.03);
  the host route for one pair: the copy of the features to the host, scipy cKDTree in 33 dimensions with 16 workers both ways, the mutual
  filter, and a numpy RANSAC of 4096 hypotheses (batched SVD Kabsch, the edge-length check, vectorised scoring, the refit).
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
    R, t = rodrigues(ax / np.linalg.norm(ax) * np.deg2rad(90)), rs.randn(3) * 0.02
    return ((s.astype(np.float64) - t) @ R).astype(np.float32), tgt, R, t


def host_route_ms(src, tgt, fs, ft, max_dist, H=4096, sim=0.9):
    """one pair on the host from the device's features -> (ms of the matching, ms of RANSAC, correspondences)"""
    from scipy.spatial import cKDTree
    t0 = time.perf_counter()
    a, b = fs.cpu().numpy().astype(np.float64), ft.cpu().numpy().astype(np.float64)
    s, q = src.cpu().numpy().astype(np.float64), tgt.cpu().numpy().astype(np.float64)
    fwd = cKDTree(b).query(a, workers=16)[1]
    back = cKDTree(a).query(b, workers=16)[1]
    i = np.nonzero(back[fwd] == np.arange(len(a)))[0]
    cs, cq = s[i], q[fwd[i]]
    t1 = time.perf_counter()
    tr = np.random.RandomState(0).randint(0, len(i), (H, 3))
    ps, pq = cs[tr], cq[tr]
    ok = (tr[:, 0] != tr[:, 1]) & (tr[:, 0] != tr[:, 2]) & (tr[:, 1] != tr[:, 2])
    for x, y in ((0, 1), (1, 2), (2, 0)):
        ls, lt = np.linalg.norm(ps[:, x] - ps[:, y], axis=1), np.linalg.norm(pq[:, x] - pq[:, y], axis=1)
        ok &= (ls >= sim * lt) & (lt >= sim * ls)
    ps, pq = ps[ok], pq[ok]

    def kabsch(x, y):
        mx, my = x.mean(-2, keepdims=True), y.mean(-2, keepdims=True)
        U, _, Vt = np.linalg.svd(np.swapaxes(y - my, -1, -2) @ (x - mx))
        d = np.sign(np.linalg.det(U @ Vt))
        R = (U * np.stack([np.ones_like(d), np.ones_like(d), d], -1)[..., None, :]) @ Vt
        return R, my[..., 0, :] - (R @ mx[..., 0, :, None])[..., 0]

    R, t = kabsch(ps, pq)
    count = np.zeros(len(R), np.int64)
    for h0 in range(0, len(R), 256):
        d = np.einsum("hij,cj->hci", R[h0:h0 + 256], cs) + t[h0:h0 + 256, None] - cq[None]
        count[h0:h0 + 256] = ((d * d).sum(-1) <= max_dist ** 2).sum(1)
    w = int(np.argmax(count)) if len(count) else 0
    if len(count):
        inl = (((cs @ R[w].T + t[w] - cq) ** 2).sum(1) <= max_dist ** 2)
        if inl.sum() >= 3:
            kabsch(cs[inl], cq[inl])
    return (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3, len(i)


def case(rs, B, n, max_dist=0.03, k=32):
    ps = [pair(rs, n) for _ in range(B)]
    src, tgt = (torch.from_numpy(np.concatenate([p[j] for p in ps])).to(dev) for j in range(2))
    off = np.arange(B + 1, dtype=np.int64) * n
    base = dict(B=B, N=n, M=n)
    ns, nt = G._oriented_normals(src, off, 16, None), G._oriented_normals(tgt, off, 16, None)
    knn_ms = gpu_ms(lambda: scan.knn_dev(src, src, k, off, off, exclude_self=True))
    fpfh_ms = gpu_ms(lambda: G.fpfh_dev(src, ns, off, k))
    kd2, kidx = scan.knn_dev(src, src, k, off, off, exclude_self=True)
    stages_ms = gpu_ms(lambda: G._fpfh_from_knn(src, ns, off, kidx, kd2, k, 0, 0.0))       # the two launches on given neighbour rows
    orient_ms = gpu_ms(lambda: G._oriented_normals(src, off, 16, None))
    line(kernel="fpfh_dev", **base, k=k, knn_ms=knn_ms, fpfh_dev_ms=fpfh_ms, spfh_and_fpfh_ms=stages_ms, oriented_normals_ms=orient_ms)
    fs, ft = G.fpfh_dev(src, ns, off, k)[0], G.fpfh_dev(tgt, nt, off, k)[0]
    nn_ms = gpu_ms(lambda: metrics.nn_dist(src.reshape(B, n, 3), tgt.reshape(B, n, 3), return_index=True))
    for q in (2, 4):
        ms = gpu_ms(lambda: G._feature_nn(fs, ft, off, off, 0, q))
        line(kernel="feature_nn", **base, queries_per_lane=q, ms=ms, pair_tests_per_s=B * n * n / (ms * 1e-3), nn_dist_ms=nn_ms,
             nn_dist_pair_tests_per_s=B * n * n / (nn_ms * 1e-3), x_nn_dist=ms / nn_ms)
    match_ms = gpu_ms(lambda: G.match_features_dev(fs, ft, off, off))
    corr, co, _, _ = G.match_features_dev(fs, ft, off, off)
    line(kernel="match_features_dev", **base, ms=match_ms, correspondences=np.diff(co).tolist())
    a = G._Greg("kbench", src, tgt, off, off, corr, co)
    a.to_device("kbench")
    maxd2 = float(np.float32(max_dist ** 2))
    for H in (4096, 65536):
        trd = G._triples_dev(G.correspondence_hypotheses(np.diff(co), H, 0), dev)
        pose_ms = gpu_ms(lambda: a.poses(trd, 0.9))
        poses, valid = a.poses(trd, 0.9)
        score_ms = gpu_ms(lambda: a.score(poses, valid, None, maxd2))
        count, best, status = a.score(poses, valid, None, maxd2)
        refit_ms = gpu_ms(lambda: a.refit(poses, best, status.clone(), maxd2, True))
        line(kernel="ransac", **base, H=H, poses_ms=pose_ms, score_ms=score_ms, refit_ms=refit_ms, valid=valid.sum(1).tolist(),
             hypothesis_tests_per_s=float(valid.sum()) * float(np.diff(co).mean()) / (score_ms * 1e-3), best_count=count.max(1).values.tolist())
    whole = gpu_ms(lambda: G.global_registration_dev(src, tgt, off, off, max_dist=max_dist))
    out = G.global_registration_dev(src, tgt, off, off, max_dist=max_dist)
    errs = []
    for b, p in enumerate(ps):
        T = out[0][b].cpu().numpy()
        errs.append(round(float(np.linalg.norm(T[:3, :3] - p[2])), 5))
    m_ms, r_ms, c = host_route_ms(src[:n], tgt[:n], fs[:n], ft[:n], max_dist)
    line(kernel="global_registration_dev", **base, ms=whole, status=out[6].tolist(), n_in=out[3].tolist(), rotation_error=errs,
         host_match_ms_one_pair=m_ms, host_ransac_ms_one_pair=r_ms, host_correspondences=c, x_host=(m_ms + r_ms) * B / whole)


rs = np.random.RandomState(0)
for B, n in ((1, 4096), (8, 4096), (1, 16384), (8, 16384)):
    case(rs, B, n)
