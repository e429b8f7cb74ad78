"""Micro-benchmark of the device mesh decimation (csrc/simplify.hip, shapeformer_amd/simplify.py; run on the GPU box).
One JSON line per measurement (device events around whole calls, their size read-backs included; 2 warm-up + 10 repetitions):
  meshes: an analytic sphere (r = 0.6) at 129^3 and 257^3 through the dense route, and the res16 hash-weight VQDIF's mesh at 129^3
  (dense route) and 257^3 (sparse route, margin 1), one shape each, plus the 257^3 sphere as a batch of 8;
  per mesh: the meshing time of that mesh, the counting pass at G = 64, cluster_simplify_dev at G = 64, decimate_dev to 4096 faces with
  the G it found and its host read-backs, the bytes the decimated mesh saves in the copy to the host (12 V + 12 T) and in the
  double-precision PLY (24 V + 13 T), and the host time of tests/simplify_ref.py (numpy) for the counting pass and one clustering
  on the same mesh - the comparison figure: there is no earlier device path and igl is not installed.
No file dependency."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import simplify_ref as S
from shapeformer_amd import mcubes, simplify as SD, synthetic, weights as W
from shapeformer_amd.vqdif import VQDIF

dev = torch.device("cuda:0")
G_FIXED, BUDGET = 64, 4096


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


def sphere_field(Q, B):
    x = torch.linspace(-1, 1, Q, device=dev, dtype=torch.float64)
    d = (x[:, None, None] ** 2 + x[None, :, None] ** 2 + x[None, None, :] ** 2).sqrt()
    return (1 / (1 + torch.exp(10 * (d - 0.6)))).float()[None].expand(B, -1, -1, -1).contiguous()


def mesh_bytes(V, T):
    return dict(copy=12 * int(V) + 12 * int(T), ply=24 * int(V) + 13 * int(T))


def report(name, Q, B, mesh_fn):
    ms_mesh = gpu_ms(mesh_fn, n=5, warm=1)
    v, f, voff, toff = mesh_fn()
    V, T = int(voff[-1]), int(toff[-1])
    ms_count = gpu_ms(lambda: SD.cluster_faces_dev(v, f, voff, toff, G_FIXED))
    ms_cluster = gpu_ms(lambda: SD.cluster_simplify_dev(v, f, voff, toff, G_FIXED))
    cv, cf, cvo, cto, _ = SD.cluster_simplify_dev(v, f, voff, toff, G_FIXED)
    ms_dec = gpu_ms(lambda: SD.decimate_dev(v, f, voff, toff, BUDGET))
    rb = SD.read_backs
    dv, df, dvo, dto, status, G = SD.decimate_dev(v, f, voff, toff, BUDGET)
    rb = SD.read_backs - rb
    full, small = mesh_bytes(V, T), mesh_bytes(dvo[-1], dto[-1])
    hv, hf = v[:voff[1]].cpu().numpy(), f[:toff[1]].cpu().numpy()          # the reference on the first shape
    t0 = time.perf_counter()
    ref_count = S.count(hv, hf, G_FIXED)
    t1 = time.perf_counter()
    same = err = ref_cluster_ms = None
    if len(hf) <= 3_000_000:               # the numpy clustering of a larger mesh takes minutes (np.add.at over 9 terms per corner)
        rv, rf, _ = S.cluster(hv, hf, G_FIXED)
        ref_cluster_ms = (time.perf_counter() - t1) * 1e3
        same = bool(np.array_equal(rf, cf[:cto[1]].cpu().numpy()))
        err = float(np.abs(rv.astype(np.float64) - cv[:cvo[1]].cpu().numpy()).max()) if len(rv) == cvo[1] else None
    line(mesh=name, Q=Q, B=B, verts=V, faces=T, ms_meshing=ms_mesh, G_fixed=G_FIXED, ms_counting_pass=ms_count, ms_cluster_simplify=ms_cluster,
         cluster_verts=int(cvo[-1]), cluster_faces=int(cto[-1]), budget=BUDGET, ms_decimate=ms_dec, decimate_G=[int(g) for g in G],
         decimate_faces=[int(x) for x in np.diff(dto)], decimate_status=status.cpu().tolist(), read_backs_per_decimate=rb,
         bytes_copy_full=full["copy"], bytes_copy_decimated=small["copy"], bytes_ply_full=full["ply"], bytes_ply_decimated=small["ply"],
         ref_host_ms_counting_pass_one_shape=(t1 - t0) * 1e3, ref_host_ms_cluster_one_shape=ref_cluster_ms,
         ref_counts_equal=bool(ref_count == (int(cto[1]), int(cvo[1]))), ref_faces_equal=same, ref_max_abs_position_diff=err)


for Q, B in ((129, 1), (257, 1), (257, 8)):
    F = sphere_field(Q, B)
    report("analytic sphere r=0.6, dense marching cubes", Q, B, lambda: mcubes.marching_cubes_dev(F, 0.5))
    del F
    torch.cuda.empty_cache()

vq = VQDIF(W.make_state_dict(W.vqdif_spec(16)), res=16, device=dev)
cloud = torch.from_numpy(synthetic.make_batch(2024, 1, n_full=8192, n_partial=4096)["Xbd"]).to(dev)
q = vq.quantize_cloud_dev(cloud)[0].clone()
iso = float(vq.decode_index(q, grid_Q=33, sigmoid=True)["logits"].median())


def dense129():
    occ = vq.decode_index(q, grid_Q=129, sigmoid=True)["logits"]
    return mcubes.marching_cubes_dev(occ.reshape(1, 129, 129, 129), iso)


report("res16 hash-weight VQDIF, decode_index + marching cubes", 129, 1, dense129)
torch.cuda.empty_cache()
report("res16 hash-weight VQDIF, decode_index_mesh (sparse, margin 1)", 257, 1,
       lambda: vq.decode_index_mesh(q, 257, coarse=33, margin=1, thresh=iso, sigmoid=True))
