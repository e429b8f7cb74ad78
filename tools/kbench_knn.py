"""Micro-benchmark of exact k-nearest neighbours and the scan-cleaning front end (csrc/knn.hip, shapeformer_amd/scan.py; run on the
GPU box):
  knn_dev at 16 384 x 16 384 for k = 8, 16, 32, 64 with 1 and with 64 sets, and at 10^5 x 10^5 for k = 16; the statistical outlier
  mask and the normals at 64 x 16 384.  Each case beside nn_dist (k = 1, csrc/pointdist.hip) on the same sets and beside the host
  route the reference takes: the copy to the host plus scipy cKDTree.query (workers = 16), tree build included.
  --million: also 10^6 x 10^6 at k = 16 as one timed step.
One JSON line per measurement.  The points are jittered sphere samples: surface-like data, as the clouds of the pipeline are.
Pairs are N x M per set; frac_valu_issue counts the 9 lane-ops per pair of the k = 1 kernel (tools/kbench_pointdist.py), so for
k > 1 it says how much of the issue rate the distance feed alone would take: the rest is list maintenance."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from scipy.spatial import cKDTree as cKDT

from shapeformer_amd import metrics as M
from shapeformer_amd import scan

dev = torch.device("cuda:0")
ISSUE = 256 * 4 * 32 * 2.4e9          # VALU lane-ops per second


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


def sphere(rs, n, r=0.5, jitter=0.002):
    u = rs.randn(n, 3)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    return (u * r + rs.randn(n, 3) * jitter).astype(np.float32)


def line(**kw):
    print(json.dumps(kw), flush=True)


def host_knn_ms(pt, qt, k):
    """the reference's route: both batches to the host, then per set a tree and a query with 16 workers"""
    t0 = time.perf_counter()
    p, q = pt.cpu().numpy().astype(np.float64), qt.cpu().numpy().astype(np.float64)
    for b in range(p.shape[0]):
        cKDT(q[b]).query(p[b], k=k, workers=16)
    return (time.perf_counter() - t0) * 1e3


def knn_case(rs, B, n, ks, host=True):
    pt = torch.from_numpy(np.stack([sphere(rs, n) for _ in range(B)])).to(dev)
    qt = torch.from_numpy(np.stack([sphere(rs, n) for _ in range(B)])).to(dev)
    pairs = B * n * n
    nn = gpu_ms(lambda: M.nn_dist(pt, qt, return_index=True))
    line(kernel="nn_dist", B=B, N=n, M=n, ms=nn, Gpairs_s=pairs / nn / 1e6, frac_valu_issue=9 * pairs / (nn * 1e-3) / ISSUE)
    for k in ks:
        ms = gpu_ms(lambda: scan.knn_dev(pt, qt, k))
        rec = dict(kernel="knn_dev", B=B, N=n, M=n, k=k, ms=ms, Gpairs_s=pairs / ms / 1e6, x_nn_dist=ms / nn,
                   frac_valu_issue=9 * pairs / (ms * 1e-3) / ISSUE)
        if host:
            rec["host_ckdtree_ms"] = host_knn_ms(pt, qt, k)
            rec["x_host"] = rec["host_ckdtree_ms"] / ms
        line(**rec)


rs = np.random.RandomState(0)
knn_case(rs, 1, 16384, (8, 16, 32, 64))
knn_case(rs, 64, 16384, (8, 16, 32, 64))
knn_case(rs, 1, 10 ** 5, (16,))

# the front end at the workload's shape: 64 clouds of 16 384 points, 1 % of them uniform outliers
B, n = 64, 16384
X = np.stack([sphere(rs, n) for _ in range(B)])
X[:, ::100] = rs.uniform(-1, 1, (B, len(range(0, n, 100)), 3)).astype(np.float32)
Xt = torch.from_numpy(X).to(dev)
ms = gpu_ms(lambda: scan.statistical_outlier_mask_dev(Xt, None, 16, 2.0), n=3, warm=1)
t0 = time.perf_counter()
Xh = Xt.cpu().numpy().astype(np.float64)
for b in range(B):
    m = cKDT(Xh[b]).query(Xh[b], k=17, workers=16)[0][:, 1:].mean(1)
    m <= m.mean() + 2.0 * m.std(ddof=1)
host = (time.perf_counter() - t0) * 1e3
line(kernel="statistical_outlier_mask_dev", B=B, N=n, k=16, ms=ms, host_ckdtree_ms=host, x_host=host / ms,
     kept=int(scan.statistical_outlier_mask_dev(Xt, None, 16, 2.0)[1].sum()))
ms = gpu_ms(lambda: scan.clean_cloud_dev(Xt, 16, 2.0), n=3, warm=1)
line(kernel="clean_cloud_dev", B=B, N=n, k=16, ms=ms)
ms = gpu_ms(lambda: scan.estimate_normals_dev(Xt, None, 16), n=3, warm=1)
t0 = time.perf_counter()
for b in range(B):
    nb = Xh[b][cKDT(Xh[b]).query(Xh[b], k=16, workers=16)[1]]
    y = nb - nb.mean(1, keepdims=True)
    np.linalg.eigh(np.einsum("nki,nkj->nij", y, y) / 16)
host = (time.perf_counter() - t0) * 1e3
line(kernel="estimate_normals_dev", B=B, N=n, k=16, ms=ms, host_ckdtree_eigh_ms=host, x_host=host / ms)
idx = scan.knn_dev(Xt, Xt, 16)[1].reshape(-1, 16)
from shapeformer_amd import _lib as L
xf, od = Xt.reshape(-1, 3), torch.arange(B + 1, device=dev, dtype=torch.int64) * n
normal, var = torch.empty(B * n, 3, device=dev), torch.empty(B * n, device=dev)
ms = gpu_ms(lambda: L.check(L.lib().sfmi_knn_normals_f32(L.ptr(xf), L.ptr(od), L.ptr(idx), B, B * n, 16, None, L.ptr(normal), L.ptr(var),
                                                         L.stream_ptr()), "sfmi_knn_normals_f32"))
line(kernel="knn_normals_kernel", B=B, N=n, k=16, ms=ms)

if "--million" in sys.argv:
    n = 10 ** 6
    pt, qt = torch.from_numpy(sphere(rs, n)).to(dev), torch.from_numpy(sphere(rs, n)).to(dev)
    scan.knn_dev(pt[:1000], qt[:1000], 16)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    scan.knn_dev(pt, qt, 16)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    line(kernel="knn_dev", B=1, N=n, M=n, k=16, ms=ms, Gpairs_s=n * n / ms / 1e6, steps=1)
