"""Micro-benchmark of the coarse-to-fine sparse iso-surface extraction (csrc/iso_sparse.hip + the keyed form of csrc/sdf_query.hip; run on
the GPU box) against the dense route it replaces, VQDIF.decode_index(grid_Q=Q, sigmoid=True) + marching_cubes_dev, timed in the same
process on the same shapes.  One JSON line per measurement (device events, warm-up, >= 10 repetitions):
  Q = 129, 257 at B = 8: sparse (margin 0 and 1, coarse 33) and dense, ms per shape; whether the two meshes are equal;
  Q = 513: sparse at B = 8, dense once at B = 1 as the comparator;
  per level the cells (S_l), cut cells (M_l) and points evaluated, points evaluated / Q^3, the split between the keyed decoder queries
  and the structure (the same extraction with the recorded field values replayed), and the peak device memory of one call;
  the bar of the feature: sparse device time per shape at Q = 257 below the dense route's.
The model is the res16 hash-weight VQDIF on seeded synthetic shapes; iso is the median of the coarse-lattice occupancy, a level the
hash-weight field is sure to cross.  No file dependency."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from shapeformer_amd import iso_sparse, mcubes, ops, synthetic, weights as W
from shapeformer_amd.vqdif import VQDIF

dev = torch.device("cuda:0")
B, COARSE = 8, 33


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


def peak_bytes(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


vq = VQDIF(W.make_state_dict(W.vqdif_spec(16)), res=16, device=dev)
cloud = torch.from_numpy(synthetic.make_batch(2024, B, n_full=8192, n_partial=4096)["Xbd"]).to(dev)
q = vq.quantize_cloud_dev(cloud)[0].clone()
iso = float(vq.decode_index(q, grid_Q=COARSE, sigmoid=True)["logits"].median())
line(inputs="res16 hash-weight VQDIF, synthetic.make_batch(2024)", B=B, coarse=COARSE, iso=iso)


def dense(qq, Q):
    occ = vq.decode_index(qq, grid_Q=Q, sigmoid=True)["logits"]
    return mcubes.marching_cubes_dev(occ.reshape(qq.shape[0], Q, Q, Q), iso)


for Q in (129, 257, 513):
    nl = iso_sparse.lattice_levels(Q, COARSE)
    dense_mesh = None
    if Q < 513:
        ms_d = gpu_ms(lambda: dense(q, Q))
        dense_mesh = dense(q, Q)
        line(route="dense", Q=Q, B=B, ms=ms_d, ms_per_shape=ms_d / B, faces=int(dense_mesh[3][-1]), peak_bytes=peak_bytes(lambda: dense(q, Q)))
        ms_d /= B
    else:
        ms_d = gpu_ms(lambda: dense(q[:1], Q), n=10, warm=1)
        line(route="dense", Q=Q, B=1, ms=ms_d, ms_per_shape=ms_d, faces=int(dense(q[:1], Q)[3][-1]), peak_bytes=peak_bytes(lambda: dense(q[:1], Q)))
    for margin in (0, 1):
        run = lambda: vq.decode_index_mesh(q, Q, coarse=COARSE, margin=margin, thresh=iso, sigmoid=True)
        ms_s = gpu_ms(run)
        v, f, voff, toff, info = vq.decode_index_mesh(q, Q, coarse=COARSE, margin=margin, thresh=iso, sigmoid=True, return_levels=True)
        # the split: the keyed queries alone on the recorded key lists, and the structure alone with their values replayed
        grid = vq.decoder_grid_cl(vq.get_code_cl(q), final_affine=True).clone()
        axis = torch.from_numpy(np.linspace(-1.0, 1.0, Q).astype(np.float32)).to(dev)
        rec = []

        def recording(keys, koff):
            val = ops.sdf_query_keys(axis, keys, koff, grid, vq.sdf_w, sigmoid=True)
            rec.append((keys, koff, val))
            return val
        iso_sparse.extract_sparse_dev(recording, B, COARSE, nl, thresh=iso, margin=margin, device=dev)
        calls = list(rec)
        ms_q = gpu_ms(lambda: [ops.sdf_query_keys(axis, k, o, grid, vq.sdf_w, sigmoid=True) for k, o, _ in calls])
        it = [None]

        def replay(keys, koff):
            return next(it[0])
        def structure():
            it[0] = iter([c[2] for c in calls])
            iso_sparse.extract_sparse_dev(replay, B, COARSE, nl, thresh=iso, margin=margin, device=dev)
        ms_st = gpu_ms(structure)
        ms_grid = gpu_ms(lambda: vq.decoder_grid_cl(vq.get_code_cl(q), final_affine=True))
        pts = info["points"]
        eq = None
        if dense_mesh is not None:
            eq = bool(np.array_equal(voff, dense_mesh[2]) and np.array_equal(toff, dense_mesh[3]) and torch.equal(v, dense_mesh[0])
                      and torch.equal(f, dense_mesh[1]))
        line(route="sparse", Q=Q, B=B, margin=margin, levels=nl, ms=ms_s, ms_per_shape=ms_s / B, faces=int(toff[-1]),
             equal_to_dense_mesh=eq, cells_S=[int(o[-1]) for _, o in info["S"]], cells_M=[int(o[-1]) for _, o in info["M"]],
             points=[int(p.sum()) for p in pts], points_over_Q3=float(pts.sum()) / (B * Q ** 3),
             ms_keyed_queries=ms_q, ms_structure=ms_st, ms_decoder_grid=ms_grid, peak_bytes=peak_bytes(run),
             workspace_bytes=int(iso_sparse.L.lib().sfmi_iso_sparse_workspace_bytes(B, Q)))
        if Q == 257:
            line(bar="sparse device ms/shape at Q=257 < dense ms/shape", margin=margin, sparse_ms_per_shape=ms_s / B, dense_ms_per_shape=ms_d,
                 ratio_dense_over_sparse=ms_d / (ms_s / B), met=bool(ms_s / B < ms_d))
        del rec, calls, grid
    # the structure alone on a field whose surface is a surface: two analytic spheres (the `two` input of the tests), computed from the
    # keys by torch ops - what a trained model's shapes look like to the hierarchy; the hash-weight field above crosses iso almost everywhere
    axd = torch.from_numpy(np.linspace(-1.0, 1.0, Q)).to(dev)

    def spheres(keys, koff):
        k = keys.long()
        x, y, z = axd[k // (Q * Q)], axd[(k // Q) % Q], axd[k % Q]
        d1 = ((x + .4) ** 2 + (y - .1) ** 2 + (z - .05) ** 2).sqrt()
        d2 = ((x - .55) ** 2 + (y + .5) ** 2 + (z - .45) ** 2).sqrt()
        return torch.maximum(1 / (1 + torch.exp(10 * (d1 - .35))), 1 / (1 + torch.exp(10 * (d2 - .12)))).float()
    for margin in (0, 1):
        ms_a = gpu_ms(lambda: iso_sparse.extract_sparse_dev(spheres, B, COARSE, nl, margin=margin, device=dev))
        v, f, voff, toff, info = iso_sparse.extract_sparse_dev(spheres, B, COARSE, nl, margin=margin, return_levels=True, device=dev)
        line(route="sparse structure + torch-op analytic field (two spheres)", Q=Q, B=B, margin=margin, ms=ms_a, ms_per_shape=ms_a / B,
             faces=int(toff[-1]), cells_S=[int(o[-1]) for _, o in info["S"]], cells_M=[int(o[-1]) for _, o in info["M"]],
             points=[int(p.sum()) for p in info["points"]], points_over_Q3=float(info["points"].sum()) / (B * Q ** 3))
    dense_mesh = None
    torch.cuda.empty_cache()
