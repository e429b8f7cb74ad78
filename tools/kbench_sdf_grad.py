"""Micro-benchmark of the gradient kernel (csrc/sdf_query.hip sdf_grad_kernel; run on the GPU box).  One JSON line per
measurement (device events, warm-up, >= 10 repetitions):
  the value kernel (ops.sdf_query) against the gradient kernel (ops.sdf_query_grad, and its two epilogue forms) at 2^20 points;
  VQDIF.refine_mesh_dev(steps=2) + vertex_normals_dev on the fixture mesh at 129^3 against the extraction that produced it
  (decode_index_mesh, decoder grid included), and against decode_index_mesh at 257^3 - what the refinement is an alternative to.
The model is the res16 hash-weight VQDIF on a seeded synthetic shape; iso is the median of the coarse-lattice occupancy, a level the
hash-weight field is sure to cross.  No file dependency."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from shapeformer_amd import ops, synthetic, weights as W
from shapeformer_amd.vqdif import VQDIF

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


vq = VQDIF(W.make_state_dict(W.vqdif_spec(16)), res=16, device=dev)
cloud = torch.from_numpy(synthetic.make_shape(3, 8192, 4096)["Xbd"])[None].to(dev)
q = vq.quantize_cloud_dev(cloud)[0].clone()
grid = vq.decoder_grid_cl(vq.get_code_cl(q)).clone()

# ---- kernel against kernel
N = 1 << 20
x = (torch.rand(1, N, 3, generator=torch.Generator().manual_seed(0)) * 2.2 - 1.1).to(dev)
out = torch.empty(1, N, 1, device=dev)
ms_v = gpu_ms(lambda: ops.sdf_query(x, grid, vq.sdf_w, out=out), n=20)
ms_g = gpu_ms(lambda: ops.sdf_query_grad(x, grid, vq.sdf_w_grad), n=20)
ms_s = gpu_ms(lambda: ops.sdf_refine_step(x, grid, vq.sdf_w_grad, 0.0, 0.01), n=20)
ms_n = gpu_ms(lambda: ops.sdf_normals(x, grid, vq.sdf_w_grad), n=20)
line(points=N, ms_value=ms_v, ms_value_and_grad=ms_g, ratio=ms_g / ms_v, ms_with_step_epilogue=ms_s, ms_with_normal_epilogue=ms_n,
     value_gpts_per_s=N / ms_v * 1e-6, grad_gpts_per_s=N / ms_g * 1e-6, note="the gradient launches include their output allocations")

# ---- refinement against the extraction, and against the finer lattice
iso = float(vq.decode_index(q, grid_Q=33, sigmoid=True)["logits"].median())
level = float(np.log(iso / (1 - iso)))
res = lambda g, p: float((ops.sdf_query(p[None], g, vq.sdf_w)[0, :, 0] - level).abs().median()) if len(p) else None
for Q in (129, 257):
    ms_x = gpu_ms(lambda: vq.decode_index_mesh(q, Q, thresh=iso))
    v, f, voff, toff = vq.decode_index_mesh(q, Q, thresh=iso)
    g = vq.decoder_grid_cl(vq.get_code_cl(q))
    rec = dict(Q=Q, ms_extract=ms_x, verts=int(voff[-1]), faces=int(toff[-1]), median_residual=res(g, v))
    if Q == 129:
        ms_r = gpu_ms(lambda: vq.refine_mesh_dev(g, v, voff, thresh=iso, steps=2, max_step=1.0 / (Q - 1)))
        v2 = vq.refine_mesh_dev(g, v, voff, thresh=iso, steps=2, max_step=1.0 / (Q - 1))
        ms_nrm = gpu_ms(lambda: vq.vertex_normals_dev(g, v2, voff))
        ms_all = gpu_ms(lambda: vq.decode_index_mesh(q, Q, thresh=iso, refine_steps=2, normals=True))
        rec.update(ms_refine_2_steps=ms_r, ms_normals=ms_nrm, refine_plus_normals_over_extract=(ms_r + ms_nrm) / ms_x,
                   ms_extract_refine_normals=ms_all, median_residual_refined=res(g, v2))
    line(**rec)
