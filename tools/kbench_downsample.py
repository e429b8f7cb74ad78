"""Micro-benchmark of farthest point sampling, voxel-grid downsampling and the voxel-first cleaning front end (csrc/downsample.hip,
shapeformer_amd/scan.py; run on the GPU box):
  FPS 16 384 -> 2 048 with 1 and with 64 sets, 16 384 -> 16 384 (a full ordering), 10^5 -> 16 384 (the streaming form), and full
  orderings of 1 024 and 4 096 points (the smaller resident instances);
  the voxel pass at 10^5 and 10^6 points, voxel = 1/64 of the extent;
  clean_cloud_dev on one 10^6-point scan of two densities, with voxel= and on the raw cloud.
Yardsticks, the host routes: FPS = the copy to the host plus a vectorised numpy FPS; voxel = the copy plus np.unique on the keys plus
np.add.at.  --clean-only runs the last case alone; a tree whose clean_cloud_dev has no `voxel` argument (the parent commit) then gives
the raw-cloud time only: run this file from both trees in one session for the voxel-then-clean comparison.
One JSON line per measurement: 2 warm-ups + 5 repetitions, device events around whole calls (host work of the call included)."""
import inspect
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from shapeformer_amd import scan

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


def sphere(rs, n, r=0.5, jitter=0.002):
    u = rs.randn(n, 3)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    return (u * r + rs.randn(n, 3) * jitter).astype(np.float32)


def line(**kw):
    print(json.dumps(kw), flush=True)


def host_fps_ms(xt, n):
    """the host route: the batch to the host, then per set the greedy loop with one vectorised distance update per pick"""
    t0 = time.perf_counter()
    x = xt.cpu().numpy()
    for p in x:
        dist = np.full(len(p), np.inf, np.float32)
        s = 0
        for _ in range(n):
            d = p - p[s]
            np.minimum(dist, (d * d).sum(1), out=dist)
            dist[s] = -1
            s = int(np.argmax(dist))
    return (time.perf_counter() - t0) * 1e3


def host_voxel_ms(xt, voxel):
    """the host route: the copy, f64 cells, np.unique on the packed keys, np.add.at for the sums"""
    t0 = time.perf_counter()
    p = xt.cpu().numpy()
    c = np.floor((p.astype(np.float64) - p.min(0).astype(np.float64)) / voxel).astype(np.int64)
    _, inv, cnt = np.unique((c[:, 2] * 65536 + c[:, 1]) * 65536 + c[:, 0], return_inverse=True, return_counts=True)
    acc = np.zeros((len(cnt), 3))
    np.add.at(acc, inv.reshape(-1), p)
    (acc / cnt[:, None]).astype(np.float32)
    return (time.perf_counter() - t0) * 1e3, len(cnt)


def fps_case(rs, B, m, n):
    xt = torch.from_numpy(np.stack([sphere(rs, m) for _ in range(B)])).to(dev)
    ms = gpu_ms(lambda: scan.farthest_point_sample_dev(xt, None, n))
    host = host_fps_ms(xt, n)
    line(kernel="farthest_point_sample_dev", form="resident" if m <= scan.FPS_RESIDENT_MAX else "streaming", B=B, M=m, n=n, ms=ms,
         us_per_pick=ms * 1e3 / n, host_numpy_ms=host, x_host=host / ms)


def voxel_case(rs, m):
    xt = torch.from_numpy(sphere(rs, m)).to(dev)
    voxel = float((xt.max() - xt.min()).item()) / 64
    for pick in scan.VOXEL_PICKS:
        ms = gpu_ms(lambda: scan.voxel_downsample_dev(xt, None, voxel, pick))
        host, cells = host_voxel_ms(xt, voxel)
        line(kernel="voxel_downsample_dev", pick=pick, N=m, voxel=voxel, voxels=cells, ms=ms, host_numpy_ms=host, x_host=host / ms)


def two_density(rs, n=10 ** 6):
    """a sphere scanned at two densities, 20 : 1, and 0.04 % outliers at radius 0.8 - 1.0 (the 12 620-point scan of the tests, scaled)"""
    n_out = n // 2500
    n_sparse = (n - n_out) // 21
    n_dense = n - n_out - n_sparse
    def half(k, positive):
        u = rs.randn(int(k * 2.2) + 64, 3)
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        return u[(u[:, 0] > 0) == positive][:k]
    s = np.concatenate([half(n_dense, True), half(n_sparse, False)]) * 0.5 + rs.randn(n_dense + n_sparse, 3) * 0.002
    u = rs.randn(n_out, 3)
    out = u / np.linalg.norm(u, axis=1, keepdims=True) * rs.uniform(0.8, 1.0, (n_out, 1))
    p = np.concatenate([s, out]).astype(np.float32)
    assert p.shape == (n, 3)
    return p


def clean_case(rs):
    xt = torch.from_numpy(two_density(rs)).to(dev)[None]
    has_voxel = "voxel" in inspect.signature(scan.clean_cloud_dev).parameters
    tree = "this" if has_voxel else "parent"
    ms = gpu_ms(lambda: scan.clean_cloud_dev(xt, 16, 2.0, out_N=16384))
    line(kernel="clean_cloud_dev", tree=tree, cloud="raw", N=xt.shape[1], out_N=16384, ms=ms, kept=int(scan.clean_cloud_dev(xt, 16, 2.0, out_N=16384)[1][0]))
    if has_voxel:
        for resample in scan.RESAMPLE_MODES:
            f = lambda: scan.clean_cloud_dev(xt, 16, 2.0, out_N=16384, voxel=0.01, resample=resample)
            vms = gpu_ms(f)
            line(kernel="clean_cloud_dev", tree=tree, cloud="voxel=0.01", resample=resample, N=xt.shape[1], out_N=16384, ms=vms, x_raw=ms / vms,
                 kept=int(f()[1][0]))


rs = np.random.RandomState(0)
if "--clean-only" not in sys.argv:
    fps_case(rs, 1, 16384, 2048)
    fps_case(rs, 64, 16384, 2048)
    fps_case(rs, 1, 16384, 16384)
    fps_case(rs, 1, 10 ** 5, 16384)
    fps_case(rs, 1, 1024, 1024)               # the smaller resident instances: one and four points per lane
    fps_case(rs, 1, 4096, 4096)
    voxel_case(rs, 10 ** 5)
    voxel_case(rs, 10 ** 6)
clean_case(np.random.RandomState(1))          # a generator of its own: the same scan with and without --clean-only
