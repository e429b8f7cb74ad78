"""Micro-benchmark of hidden-point removal on the device (csrc/hpr.hip; run on the GPU box) against the scipy path it replaces
(data.hidden_point_removal: numpy flip + qhull), timed in the same process on the same clouds.  One JSON line per measurement:
  hidden_point_mask_dev at B = 8 and B = 1, N = 32768, camera radius 10 (device events, warm-up, >= 10 repetitions);
  virtual_scan_dev at B = 8, context_N = 16384 (mask + prefix sum + resample);
  the scipy path per shape on one core, and the row-set difference of its visible rows against the device mask;
  the bar of the feature: device time per shape at B = 8 below the host's single-core time per shape / 16.
The clouds are seeded synthetic surface samples (boxes and spheres, f32) with the duplicate share of the stored clouds (~22 % of the
rows repeat an earlier row), no file dependency.  VALU share: constraint evaluations counted by the kernel itself (scan and
re-solve separately) times the instructions per evaluation in the gfx950 ISA of the two inner loops (an estimate of the issue cost,
not a measured count), against 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz = 3.93e13 lane-ops/s: once with the f64 instructions alone
(arithmetic, compares and the f32 <-> f64 conversions: F64_SCAN, F64_RESOLVE) and once with every VALU instruction (VALU_*)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from shapeformer_amd import data as D, hpr

dev = torch.device("cuda:0")
F64_ISSUE = 256 * 4 * 16 * 2.4e9
F64_SCAN, F64_RESOLVE = 19, 32          # f64 instructions per constraint evaluation, scan / re-solve loop
VALU_SCAN, VALU_RESOLVE = 38, 50        # all VALU instructions per constraint evaluation
N, B, CTX, RADIUS = 32768, 8, 16384, 10.


def line(**kw):
    print(json.dumps(kw), flush=True)


def gpu_ms(fn, n=10, warm=2):
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


def cloud(rs, n, distinct_share=0.784):
    """n surface points of a few boxes and spheres inside [-.5, .5]^3, f32; (1 - distinct_share) n rows repeat an earlier row."""
    nd = int(n * distinct_share)
    parts = []
    for k in range(5):
        m = nd // 5 if k < 4 else nd - 4 * (nd // 5)
        c, h = rs.uniform(-.2, .2, 3), rs.uniform(.08, .28, 3)
        if k < 3:                                                     # box surface: a random face, uniform on it
            p = rs.uniform(-1, 1, (m, 3))
            ax = rs.randint(0, 3, m)
            p[np.arange(m), ax] = rs.choice([-1., 1.], m)
            parts.append(c + p * h)
        else:                                                         # ellipsoid surface
            v = rs.randn(m, 3)
            parts.append(c + v / np.linalg.norm(v, axis=1, keepdims=True) * h)
    x = np.concatenate(parts).astype(np.float32)
    x = np.concatenate([x, x[rs.choice(nd, n - nd)]])
    return x[rs.permutation(n)]


def rows(a):
    return {r.tobytes() for r in np.ascontiguousarray(a)}


rs = np.random.RandomState(0)
clouds = np.stack([cloud(rs, N) for _ in range(B)])
cams = hpr.sample_cameras(B, RADIUS, seed=0)
X = torch.from_numpy(clouds).to(dev)
line(inputs="synthetic surface clouds", B=B, N=N, distinct_rows=[len(rows(c)) for c in clouds], radius=RADIUS)

ms8 = gpu_ms(lambda: hpr.hidden_point_mask_dev(X, cams))
vis, count, status = hpr.hidden_point_mask_dev(X, cams)
ev = hpr.constraint_evaluations_dev(X, cams).cpu().numpy().astype(np.float64).sum(0)
share = (ev[0] * F64_SCAN + ev[1] * F64_RESOLVE) / (ms8 * 1e-3) / F64_ISSUE
share_all = (ev[0] * VALU_SCAN + ev[1] * VALU_RESOLVE) / (ms8 * 1e-3) / F64_ISSUE
line(kernel="hidden_point_mask_dev", B=B, N=N, ms=ms8, ms_per_shape=ms8 / B, visible=count.cpu().tolist(), status=status.cpu().tolist(),
     scan_evals_per_N2=ev[0] / (B * N * N), resolve_evals_per_N2=ev[1] / (B * N * N), frac_f64_valu_issue=share,
     frac_all_valu_issue=share_all)
x_flat, o_host, c_host, _ = hpr._prepare(X, cams, None, "kbench")
ms_order = gpu_ms(lambda: hpr.constraint_order_dev(x_flat, o_host, c_host))
line(step="constraint_order_dev (torch: Morton keys + stable sort; included in every hidden_point_mask_dev time)", B=B, N=N, ms=ms_order)
ms8i = gpu_ms(lambda: hpr.hidden_point_mask_dev(X, cams, _index_order=True), n=3, warm=1)
visi, _, _ = hpr.hidden_point_mask_dev(X, cams, _index_order=True)
evi = hpr.constraint_evaluations_dev(X, cams, index_order=True).cpu().numpy().astype(np.float64).sum(0)
line(kernel="hidden_point_mask_dev, constraints in index order (A/B)", B=B, N=N, ms=ms8i, ms_per_shape=ms8i / B,
     scan_evals_per_N2=evi[0] / (B * N * N), resolve_evals_per_N2=evi[1] / (B * N * N), mask_equal_to_morton_order=bool(torch.equal(visi, vis)))
ms1 = gpu_ms(lambda: hpr.hidden_point_mask_dev(X[:1], cams[:1]))
line(kernel="hidden_point_mask_dev", B=1, N=N, ms=ms1, ms_per_shape=ms1)
msv = gpu_ms(lambda: hpr.virtual_scan_dev(X, CTX, radius=RADIUS, seed=0, cams=cams))
line(kernel="virtual_scan_dev", B=B, N=N, context_N=CTX, ms=msv, ms_per_shape=msv / B)

# the host path on the same clouds, one core (numpy's elementwise flip and qhull are single-threaded); one untimed call first:
# the first qhull call of a process pays for scipy's import
vis = vis.cpu().numpy().astype(bool)
D.hidden_point_removal(clouds[0], cams[0])
host, diffs = [], []
for b in range(B):
    t0 = time.perf_counter()
    want = D.hidden_point_removal(clouds[b], cams[b])
    host.append((time.perf_counter() - t0) * 1e3)
    diffs.append(len(rows(want) ^ rows(clouds[b][vis[b]])))
host_ms = float(np.mean(host))
line(host="data.hidden_point_removal (scipy qhull, one core)", N=N, ms_per_shape=host_ms, ms_each=host, rows_differing_from_device=diffs)
line(bar="device ms/shape at B=8 < host single-core ms/shape / 16", device_ms_per_shape=ms8 / B, host_ms_per_shape_over_16=host_ms / 16,
     ratio_host_over_device=host_ms / (ms8 / B), met=bool(ms8 / B < host_ms / 16))
