"""Mesh decimation on the device — host side of csrc/simplify.hip.

The reference decimates in the call that meshes: xgutils/geoutil.py:175-233 array2mesh(..., if_decimate=False, decimate_face=4096) runs
igl.decimate(verts, faces, decimate_face) when the mesh has more faces than the budget (xgutils/vis/npfvis.py:88-116 turns it on).
Here the ragged meshes of `marching_cubes_dev` / `extract_sparse_dev` are decimated where they are, in HBM, by vertex clustering with
quadric error metrics on a G^3 grid over the box, G bisected per shape to the face budget.  What is kept of the reference is its
interface - a face budget, and a mesh at or below it returned unchanged - NOT igl.decimate's output (edge collapse; its order is
not reproducible).  The contract is in include/sfmi.h, its numpy statement in tests/simplify_ref.py.  There is no CPU fallback.

  cluster_faces_dev(verts, faces, voff, toff, grid, bbox)            -> surviving faces, occupied cells per shape (the counting pass)
  cluster_simplify_dev(verts, faces, voff, toff, grid, bbox, reg)    -> verts, faces, voff, toff, status
  decimate_dev(verts, faces, voff, toff, decimate_face, bbox, reg)   -> verts, faces, voff, toff, status, G

verts (V,3) f32 and faces (T,3) int32 (indices local per shape) are device tensors, voff / toff (B+1) host offsets, as
`marching_cubes_dev` returns them (the argument checks are _ragged.py's).  status (B) int32 on the device: 0 ok, 1 no vertices, 2 a face index outside the shape, 3 a
non-finite vertex (such a shape comes back empty).  Results are bit-identical from run to run and a batch equals per-shape calls.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L
from ._ragged import i32_dev, mesh_args, on_device, runs

GRID_MAX = 512
UNIT_BOX = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
read_backs = 0          # device -> host size read-backs so far (tools/kbench_simplify.py reports the number per call)


# how this module calls mesh_args: 32-bit batch-wide indices, offsets of any array shape
_MESH = dict(index32=True, flatten_offsets=True)


def _nshapes(off):
    if off is None:
        return 1
    return (off.numel() if isinstance(off, torch.Tensor) else np.asarray(off).size) - 1


def _grid(grid, B):
    """an int or one per shape -> (B,) int32, every entry in [1, 512]; checked before anything touches the device"""
    g = np.asarray(grid)
    g = np.full(B, g) if g.ndim == 0 else g
    if g.shape != (B,) or not np.all(np.mod(g, 1) == 0):
        raise L.SfmiError(f"simplify: grid must be an int or {B} ints (one per shape), got {grid!r}")
    if len(g) and (g.min() < 1 or g.max() > GRID_MAX):
        raise L.SfmiError(f"simplify: grid = {g.tolist()} must lie in [1, {GRID_MAX}]")
    return np.ascontiguousarray(g.astype(np.int32))


def _box(bbox):
    lo, hi = (np.ascontiguousarray(np.asarray(x, np.float64).reshape(3)) for x in bbox)
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (lo < hi).all()):
        raise L.SfmiError(f"simplify: bbox needs finite lo < hi, got {lo.tolist()}, {hi.tolist()}")
    return lo, hi


def _cluster(verts, faces, vo, to, g, lo, hi, reg=None):
    """The passes of csrc/simplify.hip on a checked batch; reg None: the counting pass alone.  One read-back (sizes)."""
    global read_backs
    lib, st, dev = L.lib(), L.stream_ptr, verts.device
    B, V, T = len(g), verts.shape[0], faces.shape[0]
    nW = int(lib.sfmi_simplify_words(L.ptr(g), B))
    if nW < 0:
        raise L.SfmiError("sfmi_simplify_words: invalid grid")
    gq = g.astype(np.int64) ** 3
    woff, gd, voff, toff = (i32_dev(a, dev) for a in (np.concatenate([[0], np.cumsum((gq + 31) // 32)]), g, vo, to))
    bits, rank = torch.empty(nW, device=dev, dtype=torch.int32), torch.empty(nW, device=dev, dtype=torch.int32)
    vkey, vslot = torch.empty(max(V, 1), device=dev, dtype=torch.int32), torch.empty(max(V, 1), device=dev, dtype=torch.int32)
    flags, status, count = (torch.empty(B, device=dev, dtype=torch.int32) for _ in range(3))
    surv = torch.empty(max(T, 1), device=dev, dtype=torch.uint8)
    cslot = torch.empty(max(3 * T, 1), device=dev, dtype=torch.int32) if reg is not None else None
    L.check(lib.sfmi_simplify_cells_f32(L.ptr(verts), L.ptr(faces), L.ptr(voff), L.ptr(toff), L.ptr(g), L.ptr(gd), L.ptr(woff), B, V, T,
                                        L.ptr(lo), L.ptr(hi), L.ptr(vkey), L.ptr(bits), L.ptr(flags), st()), "sfmi_simplify_cells_f32")
    L.check(lib.sfmi_simplify_popc_i32(L.ptr(bits), L.ptr(flags), L.ptr(woff), L.ptr(g), B, L.ptr(rank), L.ptr(status), st()),
            "sfmi_simplify_popc_i32")
    rank.cumsum_(0)
    coff = torch.cat([rank.new_zeros(1), rank[(woff[1:] - 1).long()]]).contiguous()
    L.check(lib.sfmi_simplify_slots_i32(L.ptr(vkey), L.ptr(voff), L.ptr(woff), L.ptr(bits), L.ptr(rank), L.ptr(flags), L.ptr(g), B, V,
                                        L.ptr(vslot), st()), "sfmi_simplify_slots_i32")
    L.check(lib.sfmi_simplify_faces_i32(L.ptr(faces), L.ptr(voff), L.ptr(toff), L.ptr(vslot), L.ptr(flags), B, T, L.ptr(cslot), L.ptr(surv),
                                        L.ptr(count), st()), "sfmi_simplify_faces_i32")
    h = torch.cat([coff, count]).cpu().numpy().astype(np.int64)             # the one read-back: sizes
    read_backs += 1
    hc, hs = h[:B + 1], h[B + 1:]
    if reg is None:
        return hs, np.diff(hc)
    nC, nS = int(hc[-1]), int(hs.sum())
    out_v = torch.empty(max(nC, 1), 3, device=dev, dtype=torch.float32)
    out_f = torch.empty(max(nS, 1), 3, device=dev, dtype=torch.int32)
    if nC:
        vorder, vseg = runs(vslot[:V], nC)
        corder, cseg = runs(cslot[:3 * T], nC)
        L.check(lib.sfmi_simplify_solve_f32(L.ptr(verts), L.ptr(faces), L.ptr(voff), L.ptr(vkey), L.ptr(g), L.ptr(gd), L.ptr(vorder),
                                            L.ptr(vseg), L.ptr(corder), L.ptr(cseg), B, nC, L.ptr(lo), L.ptr(hi), float(reg), L.ptr(out_v),
                                            st()), "sfmi_simplify_solve_f32")
    if nS:
        sincl = torch.cumsum(surv[:T], 0, dtype=torch.int32)
        L.check(lib.sfmi_simplify_emit_i32(L.ptr(faces), L.ptr(voff), L.ptr(toff), L.ptr(vslot), L.ptr(surv), L.ptr(sincl), L.ptr(coff), B, T,
                                           nS, L.ptr(out_f), st()), "sfmi_simplify_emit_i32")
    return out_v[:nC], out_f[:nS], hc, np.concatenate([[0], np.cumsum(hs)]), status


def cluster_faces_dev(verts, faces, voff, toff, grid, bbox=UNIT_BOX):
    """The counting pass: per shape the faces that survive clustering on a grid^3 lattice over bbox and the occupied cells, as two
    (B,) host int arrays ((0, 0) for a shape whose status is not 0).  grid: an int or one per shape, in [1, 512]."""
    g = _grid(grid, _nshapes(voff))
    verts, faces, vo, to = mesh_args(verts, faces, voff, toff, "cluster_faces_dev", **_MESH)
    on_device("cluster_faces_dev", verts, faces)
    return _cluster(verts, faces, vo, to, g, *_box(bbox))


def cluster_simplify_dev(verts, faces, voff, toff, grid, bbox=UNIT_BOX, reg=1e-3):
    """One vertex per occupied cell of the grid^3 lattice over bbox (ascending cell key per shape), placed by the regularised quadric
    of the planes of the faces at its vertices; the faces whose three cells differ, in input order.
    -> verts (C,3) f32, faces (S,3) int32 local per shape (device), voff, toff (B+1) host arrays, status (B) int32 (device)."""
    g = _grid(grid, _nshapes(voff))
    if not (np.isfinite(reg) and reg > 0):
        raise L.SfmiError(f"simplify: reg = {reg} must be > 0")
    verts, faces, vo, to = mesh_args(verts, faces, voff, toff, "cluster_simplify_dev", **_MESH)
    on_device("cluster_simplify_dev", verts, faces)
    return _cluster(verts, faces, vo, to, g, *_box(bbox), reg=float(reg))


def _take(verts, faces, vo, to, shapes):
    """the sub-batch of the listed shapes"""
    v = torch.cat([verts[vo[b]:vo[b + 1]] for b in shapes])
    f = torch.cat([faces[to[b]:to[b + 1]] for b in shapes])
    return (v, f, np.concatenate([[0], np.cumsum([vo[b + 1] - vo[b] for b in shapes])]),
            np.concatenate([[0], np.cumsum([to[b + 1] - to[b] for b in shapes])]))


def decimate_dev(verts, faces, voff, toff, decimate_face=4096, bbox=UNIT_BOX, reg=1e-3):
    """array2mesh's `if_decimate` step for a ragged batch: a shape with at most `decimate_face` faces comes back unchanged, bit for
    bit (it is not inspected: status 0, or 1 without vertices; G = 0); every other one is clustered at the G the bisection of
    include/sfmi.h finds, so that it keeps at most `decimate_face` faces (and more than that at G+1 while G < 512).  The shapes over
    the budget bisect together: one counting pass and one read-back per step, at most 10 steps, then one clustering pass.
    -> verts, faces (device), voff, toff (host), status (B) int32 (device), G (B) host ints."""
    target = int(decimate_face)
    if target < 0:
        raise L.SfmiError(f"decimate_dev: decimate_face = {decimate_face} must be >= 0")
    if not (np.isfinite(reg) and reg > 0):
        raise L.SfmiError(f"simplify: reg = {reg} must be > 0")
    lo, hi = _box(bbox)
    verts, faces, vo, to = mesh_args(verts, faces, voff, toff, "decimate_dev", **_MESH)
    on_device("decimate_dev", verts, faces)
    B = len(vo) - 1
    status = torch.from_numpy((np.diff(vo) == 0).astype(np.int32)).to(verts.device)
    G = np.zeros(B, np.int64)
    over = [b for b in range(B) if to[b + 1] - to[b] > target]
    if not over:
        return verts, faces, vo, to, status, G
    sub = (verts, faces, vo, to) if len(over) == B else _take(verts, faces, vo, to, over)
    n = len(over)
    done = _cluster(*sub, np.full(n, GRID_MAX, np.int32), lo, hi)[0] <= target
    glo, ghi = np.ones(n, np.int64), np.full(n, GRID_MAX, np.int64)
    while True:
        act = ~done & (ghi - glo > 1)
        if not act.any():
            break
        mid = np.where(act, (glo + ghi) // 2, glo)
        ok = _cluster(*sub, mid.astype(np.int32), lo, hi)[0] <= target
        glo, ghi = np.where(act & ok, mid, glo), np.where(act & ~ok, mid, ghi)
    gs = np.where(done, GRID_MAX, glo)
    sv, sf, svo, sto, sst = _cluster(*sub, gs.astype(np.int32), lo, hi, reg=float(reg))
    G[over] = gs
    status[torch.as_tensor(over, device=verts.device)] = sst
    if len(over) == B:
        return sv, sf, svo, sto, status, G
    pv, pf, nv, nt = [], [], [], []
    where = {b: k for k, b in enumerate(over)}
    for b in range(B):
        if b in where:
            k = where[b]
            pv.append(sv[svo[k]:svo[k + 1]]), pf.append(sf[sto[k]:sto[k + 1]])
        else:
            pv.append(verts[vo[b]:vo[b + 1]]), pf.append(faces[to[b]:to[b + 1]])
        nv.append(pv[-1].shape[0]), nt.append(pf[-1].shape[0])
    return (torch.cat(pv), torch.cat(pf), np.concatenate([[0], np.cumsum(nv)]).astype(np.int64),
            np.concatenate([[0], np.cumsum(nt)]).astype(np.int64), status, G)
