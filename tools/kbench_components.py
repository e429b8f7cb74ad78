"""Micro-benchmark of the device mesh connected components (csrc/components.hip, shapeformer_amd/components.py; run on
the GPU box).  One JSON line per measurement (device events around whole calls, their size read-backs included; 2 warm-up + 10
repetitions):
  meshes: an analytic field of one large (r = 0.3) and 64 small (r = 0.04) spheres at 129^3 and 257^3 through the dense route, and
  the res16 hash-weight VQDIF's mesh at 129^3, one shape each;
  per mesh: marching_cubes_dev of that grid, mesh_components_dev (the labelling and statistics alone), keep_components_dev(top=1), the
  size read-backs per call of each, and the host route on one core: device-to-host copy + scipy.sparse.csgraph.connected_components +
  a numpy filter (largest piece by area, mask and renumber) + the copy back; whether the two routes return the same mesh; the ratio of
  keep_components_dev to the extraction time.  The bar: keep_components_dev takes less than the host route on every input.
No file dependency."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from shapeformer_amd import components as CC, mcubes, synthetic, weights as W
from shapeformer_amd.vqdif import VQDIF

torch.set_num_threads(1)                  # the host route runs on one core
dev = torch.device("cuda:0")


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


def spheres_field(Q):
    """occupancy of one large sphere at the origin and 64 small ones on a 4^3 grid around it, none touching another"""
    x = torch.linspace(-1, 1, Q, device=dev, dtype=torch.float32)
    g = (-0.85, -0.28, 0.28, 0.85)
    balls = [((0.0, 0.0, 0.0), 0.3)] + [((a, b, c), 0.04) for a in g for b in g for c in g]
    occ = torch.zeros(Q, Q, Q, device=dev)
    for (a, b, c), r in balls:
        d = ((x[:, None, None] - a) ** 2 + (x[None, :, None] - b) ** 2 + (x[None, None, :] - c) ** 2).sqrt()
        occ = torch.maximum(occ, torch.sigmoid(40.0 * (r - d)))
    return occ[None].contiguous()


def host_route(v, f):
    """what a caller does today: copy, scipy's connected components, keep the largest piece by area with numpy, copy back"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    hv, hf = v.cpu().numpy(), f.cpu().numpy().astype(np.int64)
    i, j = np.concatenate([hf[:, 0], hf[:, 0]]), np.concatenate([hf[:, 1], hf[:, 2]])
    n, lab = connected_components(coo_matrix((np.ones(len(i), np.int8), (i, j)), shape=(len(hv), len(hv))), directed=False)
    p = hv.astype(np.float64)
    a, b, c = p[hf[:, 0]], p[hf[:, 1]], p[hf[:, 2]]
    fl = lab[hf[:, 0]]
    area = np.bincount(fl, weights=0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1), minlength=n)
    big = int(np.argmax(area))
    fk = fl == big
    vk = np.zeros(len(hv), bool)
    vk[hf[fk].reshape(-1)] = True
    new = np.cumsum(vk) - 1
    return torch.from_numpy(hv[vk]).to(dev), torch.from_numpy(new[hf[fk]].astype(np.int32)).to(dev), n


def report(name, Q, mesh_fn):
    ms_mesh = gpu_ms(mesh_fn, n=5, warm=1)
    v, f, voff, toff = mesh_fn()
    ms_label = gpu_ms(lambda: CC.mesh_components_dev(v, f, voff, toff))
    ms_keep = gpu_ms(lambda: CC.keep_components_dev(v, f, voff, toff, top=1))
    rb = CC.read_backs
    vl, fl, coff, stats, status = CC.mesh_components_dev(v, f, voff, toff)
    rb_label = CC.read_backs - rb
    rb = CC.read_backs
    kv, kf, kvo, kto, _, kept, _ = CC.keep_components_dev(v, f, voff, toff, top=1)
    rb_keep = CC.read_backs - rb
    torch.cuda.synchronize()
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        hv, hf, n_host = host_route(v, f)
        torch.cuda.synchronize()
        host.append((time.perf_counter() - t0) * 1e3)
    ms_host = min(host)
    line(mesh=name, Q=Q, verts=int(voff[-1]), faces=int(toff[-1]), components=int(coff[-1]), components_scipy=int(n_host),
         largest_faces=int(stats["n_face"].max()) if coff[-1] else 0, status=status.cpu().tolist(), ms_meshing=ms_mesh,
         ms_mesh_components=ms_label, ms_keep_top1=ms_keep, read_backs_per_mesh_components=rb_label, read_backs_per_keep=rb_keep,
         kept_verts=int(kvo[-1]), kept_faces=int(kto[-1]), ms_host_route_one_core=ms_host, host_route_runs_ms=host,
         same_mesh_as_host_route=bool(torch.equal(kv, hv) and torch.equal(kf, hf)), keep_over_meshing=ms_keep / ms_mesh,
         keep_faster_than_host_route=bool(ms_keep < ms_host))


for Q in (129, 257):
    F = spheres_field(Q)
    report("analytic field: one large and 64 small spheres, dense marching cubes", Q, lambda: mcubes.marching_cubes_dev(F, 0.5))
    del F
    torch.cuda.empty_cache()

vq = VQDIF(W.make_state_dict(W.vqdif_spec(16)), res=16, device=dev)
cloud = torch.from_numpy(synthetic.make_batch(2024, 1, n_full=8192, n_partial=4096)["Xbd"]).to(dev)
q = vq.quantize_cloud_dev(cloud)[0].clone()
iso = float(vq.decode_index(q, grid_Q=33, sigmoid=True)["logits"].median())
occ129 = vq.decode_index(q, grid_Q=129, sigmoid=True)["logits"].reshape(1, 129, 129, 129).clone()
report("res16 hash-weight VQDIF at its median level, marching cubes of the decoded grid", 129, lambda: mcubes.marching_cubes_dev(occ129, iso))
