"""Micro-benchmark of the edge-collapse decimation (csrc/collapse.hip, shapeformer_amd/collapse.py; run on the GPU box).
One JSON line per mesh (device events around whole calls, their read-backs included):
  meshes: those of tools/kbench_simplify.py - an analytic sphere (r = 0.6) at 129^3 and 257^3 through the dense route, the 257^3 sphere
  as a batch of 8, and the res16 hash-weight VQDIF's mesh at 129^3 (dense route) and 257^3 (sparse route, margin 1);
  per mesh, to 4096 faces: pure collapse (rounds per shape, ms per call and per round, read-backs, faces and status), the hybrid route
  with precluster 4 and 16, and `simplify.decimate_dev` as the yardstick; the output's topology (mesh_topology_dev) for each route; on
  the sphere the one-sided vertex-to-surface error max / mean | |v| - 0.6 | of each route's output.
  Argument: `small` leaves the 257^3 meshes out.
No file dependency."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from shapeformer_amd import collapse as CD, mcubes, simplify as SD, synthetic, weights as W
from shapeformer_amd.vqdif import VQDIF

dev = torch.device("cuda:0")
BUDGET, RADIUS = 4096, 0.6


def line(**kw):
    print(json.dumps(kw), flush=True)


def gpu_ms(fn, n, warm=1):
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


def sphere_field(Q, B):
    x = torch.linspace(-1, 1, Q, device=dev, dtype=torch.float64)
    d = (x[:, None, None] ** 2 + x[None, :, None] ** 2 + x[None, None, :] ** 2).sqrt()
    return (1 / (1 + torch.exp(10 * (d - RADIUS)))).float()[None].expand(B, -1, -1, -1).contiguous()


def describe(out, sphere):
    v, f, voff, toff, status = out[:5]
    counts, _ = CD.mesh_topology_dev(v, f, voff, toff)
    d = dict(faces=[int(x) for x in np.diff(toff)], status=status.cpu().tolist(),
             topology={k: counts[:, i].cpu().tolist() for i, k in enumerate(CD.TOPOLOGY)})
    if sphere and len(v):
        e = (v.double().norm(dim=1) - RADIUS).abs()
        d.update(sphere_err_max=float(e.max()), sphere_err_mean=float(e.mean()))
    return d


def report(name, Q, B, mesh, sphere=False):
    v, f, voff, toff = mesh
    T = int(toff[-1])
    n = 3 if T < 1_000_000 else 1
    res = dict(mesh=name, Q=Q, B=B, verts=int(voff[-1]), faces=T, budget=BUDGET)
    rb = CD.read_backs
    out = CD.collapse_dev(v, f, voff, toff, BUDGET, details=True)
    rb = CD.read_backs - rb
    ms = gpu_ms(lambda: CD.collapse_dev(v, f, voff, toff, BUDGET), n, warm=0)
    rounds = [int(r) for r in out[5]]
    res["collapse"] = dict(ms=ms, rounds=rounds, ms_per_round=ms / max(max(rounds), 1), read_backs=rb, **describe(out, sphere))
    for k in (4, 16):
        run = lambda: CD.decimate_collapse_dev(v, f, voff, toff, BUDGET, precluster=k)
        res[f"precluster{k}"] = dict(ms=gpu_ms(run, 3), **describe(run(), sphere))
    run = lambda: SD.decimate_dev(v, f, voff, toff, BUDGET)
    res["decimate_dev"] = dict(ms=gpu_ms(run, 5), G=[int(g) for g in run()[5]], **describe(run(), sphere))
    line(**res)


small = "small" in sys.argv[1:]
for Q, B in ((129, 1),) if small else ((129, 1), (257, 1), (257, 8)):
    F = sphere_field(Q, B)
    report("analytic sphere r=0.6, dense marching cubes", Q, B, mcubes.marching_cubes_dev(F, 0.5), sphere=True)
    del F
    torch.cuda.empty_cache()

vq = VQDIF(W.make_state_dict(W.vqdif_spec(16)), res=16, device=dev)
cloud = torch.from_numpy(synthetic.make_batch(2024, 1, n_full=8192, n_partial=4096)["Xbd"]).to(dev)
q = vq.quantize_cloud_dev(cloud)[0].clone()
iso = float(vq.decode_index(q, grid_Q=33, sigmoid=True)["logits"].median())
occ = vq.decode_index(q, grid_Q=129, sigmoid=True)["logits"]
report("res16 hash-weight VQDIF, decode_index + marching cubes", 129, 1, mcubes.marching_cubes_dev(occ.reshape(1, 129, 129, 129), iso))
del occ
torch.cuda.empty_cache()
if not small:
    report("res16 hash-weight VQDIF, decode_index_mesh (sparse, margin 1)", 257, 1,
           vq.decode_index_mesh(q, 257, coarse=33, margin=1, thresh=iso, sigmoid=True))
