"""Micro-benchmark of the consistent normal orientation (csrc/tangent.hip, shapeformer_amd/scan.py orient_normals_dev; DESIGN.md §5.21;
run on the GPU box):
  the forest (sfmi_tangent_forest_f32: all Boruvka rounds, component, parity) with its round count,
  the anchor (sfmi_tangent_apply_f32: centroid, vote, apply),
  the whole orient_normals_dev with the table given and with its own self-kNN,
at 1 and 8 sets of 16 384 points and one set of 10^6 points reduced by voxel_downsample_dev(voxel=0.01), k = 8 / 16 / 32, each next to
the knn + knn_normals time it follows (estimate_normals_dev).  The clouds are noisy sphere shells of radius 0.5.  The forest is also
timed with its round cap lowered to the rounds the input needs (what the empty rounds past the last useful one cost) next to one
read-back of a device flag (what checking on the host would cost instead).  Offers issued against offers skipped by the pre-check
are not counted: that needs a counter in the kernel, i.e. another kernel than the one measured.
Yardstick, the host route: the copy of points, normals and nothing else, scipy cKDTree.query with 16 workers, the weights in numpy,
scipy.sparse.csgraph.minimum_spanning_tree and breadth_first_order (time only: scipy breaks ties its own way and drops zero weights,
which get 1e-12 added here; tests/orient_ref.py is the statement of the result).
One JSON line per measurement: 2 warm-ups + 5 repetitions, device events around whole calls (host work of the call included)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from shapeformer_amd import _lib as L
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


def line(**kw):
    print(json.dumps(kw), flush=True)


def shell(rs, n):
    u = rs.randn(n, 3)
    return (0.5 * u / np.linalg.norm(u, axis=1, keepdims=True) + rs.randn(n, 3) * 0.001).astype(np.float32)


def host_ms(x, nrm, k):
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import breadth_first_order, minimum_spanning_tree
    from scipy.spatial import cKDTree
    t0 = time.perf_counter()
    p, n = x.cpu().numpy().astype(np.float64), nrm.cpu().numpy().astype(np.float64)
    N = len(p)
    idx = cKDTree(p).query(p, k=k, workers=16)[1]
    i = np.repeat(np.arange(N), k)
    j = idx.reshape(-1)
    w = np.maximum(0.0, 1.0 - np.abs((n[i] * n[j]).sum(1))) + 1e-12
    keep = i != j
    mst = minimum_spanning_tree(csr_matrix((w[keep], (i[keep], j[keep])), shape=(N, N)))
    order, pred = breadth_first_order(mst, 0, directed=False)
    return (time.perf_counter() - t0) * 1e3, len(order)


def case(x, o, k, what):
    lib = L.lib()
    B, N = len(o) - 1, x.shape[0]
    od = torch.from_numpy(o).to(dev)
    max_n = int(np.diff(o).max())
    normals_ms = gpu_ms(lambda: scan.estimate_normals_dev(x, o, k))
    nrm = scan.estimate_normals_dev(x, o, k)[0]
    idx = scan.knn_dev(x, x, k, o, o)[1]
    component = torch.empty(N, device=dev, dtype=torch.int32)
    tree = torch.empty(N, 2, device=dev, dtype=torch.int32)
    parity = torch.empty(N, device=dev, dtype=torch.uint8)
    votes = torch.empty(N, 2, device=dev, dtype=torch.int32)
    rounds = torch.empty(B, device=dev, dtype=torch.int32)
    status = torch.empty(B, device=dev, dtype=torch.int32)
    out = torch.empty_like(nrm)
    ws = torch.empty(int(lib.sfmi_tangent_workspace_bytes(B, N)), device=dev, dtype=torch.uint8)
    forest = lambda: L.check(lib.sfmi_tangent_forest_f32(L.ptr(nrm), L.ptr(od), L.ptr(idx), B, N, k, max_n, L.ptr(component), L.ptr(tree),
                                                         L.ptr(parity), L.ptr(rounds), L.ptr(status), L.ptr(ws), L.stream_ptr()), "forest")
    apply = lambda: L.check(lib.sfmi_tangent_apply_f32(L.ptr(x), L.ptr(nrm), L.ptr(od), L.ptr(component), L.ptr(parity), None, B, N,
                                                       L.ptr(votes), L.ptr(out), L.ptr(ws), L.stream_ptr()), "apply")
    forest_ms = gpu_ms(forest)
    # the price of the rounds past the last useful one (five launches that return at once, each): the same call told a max_n that
    # makes the cap equal to the rounds this input needs
    need = int(rounds.max())
    exact = lambda: L.check(lib.sfmi_tangent_forest_f32(L.ptr(nrm), L.ptr(od), L.ptr(idx), B, N, k, min(max_n, 2 ** need), L.ptr(component),
                                                        L.ptr(tree), L.ptr(parity), L.ptr(rounds), L.ptr(status), L.ptr(ws), L.stream_ptr()),
                            "forest")
    exact_ms = gpu_ms(exact)
    flag = torch.zeros(1, device=dev, dtype=torch.int32)
    readback_ms = gpu_ms(lambda: flag.cpu())               # what one read-back of a flag would cost instead
    apply_ms = gpu_ms(apply)
    given_ms = gpu_ms(lambda: scan.orient_normals_dev(x, nrm, o, idx=idx))
    whole_ms = gpu_ms(lambda: scan.orient_normals_dev(x, nrm, o, k=k))
    _, d = scan.orient_normals_dev(x, nrm, o, idx=idx, details=True)
    s = slice(int(o[0]), int(o[1]))
    h_ms, reached = host_ms(x[s], nrm[s], k)
    h_ms *= B                                              # the host route runs set after set; the first one is timed
    launches = 1 + 5 * int(np.ceil(np.log2(max_n))) + 2
    line(kernel="orient_normals_dev", case=what, B=B, N=N, k=k, knn_normals_ms=normals_ms, forest_ms=forest_ms,
         forest_without_empty_rounds_ms=exact_ms, flag_readback_ms=readback_ms, anchor_ms=apply_ms,
         orient_given_idx_ms=given_ms, orient_ms=whole_ms, rounds=d["rounds"].cpu().tolist(), round_cap=int(np.ceil(np.log2(max_n))),
         forest_launches=launches, components=d["n_components"].cpu().tolist(), host_ms=h_ms, host_reached=reached,
         x_host_given_idx=h_ms / given_ms, forest_over_knn_normals=forest_ms / normals_ms)


rs = np.random.RandomState(0)
for k in (8, 16, 32):
    x1 = torch.from_numpy(shell(rs, 16384)).to(dev)
    case(x1, np.array([0, 16384], np.int64), k, "1 x 16384")
    x8 = torch.from_numpy(shell(rs, 8 * 16384)).to(dev)
    case(x8, np.arange(9, dtype=np.int64) * 16384, k, "8 x 16384")
    big = torch.from_numpy(shell(rs, 10 ** 6)).to(dev)
    v, vo, _, _ = scan.voxel_downsample_dev(big, None, 0.01)
    case(v, vo, k, "1 x 10^6 -> voxel 0.01")
