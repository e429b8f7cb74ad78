"""Mesh queries through a bounding-volume tree — host side of csrc/meshtree.hip.

The hierarchical route next to meshsdf's brute force, for 256^3 lattices and meshes of 10^5 faces, where O(G^3 T) takes seconds per
mesh (the reference's high-resolution path: xgutils/geoutil.py:270,345 shape2sdf / shapes2sdfs at gridDim = 256).  There is no CPU
fallback.

  mesh_tree_dev               the tree of every mesh of a ragged batch -> MeshTree, queried any number of times
  signed_distance_tree_dev    |S|, I, C bit-identical to meshsdf.signed_distance_dev (exact, pruned by the tree); the sign and W come
                              from the tree-code winding number, so the sign can differ only where |W| is near 0.5
  mesh_occupancy_tree_dev     |W_tree| > 0.5 on mesh_occupancy_dev's lattice, no workspace beyond the output
  volumetric_iou_dev          vqdif/common.py:8-36 compute_iou of two occupancy batches
  mesh_iou_dev                the IoU of two batches of meshes on one lattice (a completion against its ground truth)

W_tree (include/sfmi.h): a node whose centroid is farther from the query than beta times its radius adds its third-order expansion
(Barill et al. 2018), a leaf that is not adds its faces' exact solid angles.  beta = 2 errs by at most 2.5e-3 on the test fixtures,
beta = 3 by 3.2e-4; W_tree is a function of (query, mesh, beta) alone, so a batch equals per-shape calls bitwise.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L
from . import _ragged
from ._ragged import check_count, check_number, host_offsets, mesh_args, offsets_dev, on_device, set_ids

UNIT_BOX = ((-1.0,) * 3, (1.0,) * 3)
LEAF = 64                                        # faces per leaf (sfmi_meshtree_leaf_faces)
NODE, MOM = 9, 36                                # float4 per node, doubles of f64 sums per node (include/sfmi.h)


def level_nodes(T):
    """the node count of every level of a shape with T faces, leaves first ([] without faces): the implicit 8-ary tree"""
    if T <= 0:
        return []
    out = [(int(T) + LEAF - 1) // LEAF]
    while out[-1] > 1:
        out.append((out[-1] + 7) // 8)
    return out


class MeshTree:
    """The trees of a ragged batch of meshes (mesh_tree_dev).  Device tensors: rec (5 T, 4) f32 packed face records in sorted order,
    orig (T,) int32 the original face index (local to the shape) of every sorted face, nodes (9 NN, 4) f32 the node table, mom (NN, 36)
    f64 the sums before rounding, bbox (B, 6) f32, status (B,) int32; host offsets voff, toff, noff (B+1,) int64."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def B(self):
        return len(self.toff) - 1


def mesh_tree_dev(verts, faces, voff=None, toff=None):
    """verts (V,3) f32 and faces (T,3) int HIP tensors with indices local to each shape, voff / toff (B+1,) exclusive offsets (None:
    one shape) -> MeshTree.  status (B,) int32: 0 ok, 1 no faces, 2 a face index outside the shape, 3 a non-finite vertex (queries of
    such a shape get S = NaN, I = -1, C = NaN, W = 0, occupancy 0).  A shape's tree depends on that shape alone."""
    what = "mesh_tree_dev"
    vf, ff, vo, to = mesh_args(verts, faces, voff, toff, what)
    dev = on_device(what, verts, faces)
    B, T = len(to) - 1, int(ff.shape[0])
    nn = np.array([sum(level_nodes(t)) for t in np.diff(to)], np.int64)
    no = np.concatenate([[0], np.cumsum(nn)]).astype(np.int64)
    NN = int(no[-1])
    vod, tod, nod = (offsets_dev(o, dev) for o in (vo, to, no))
    lib, st = L.lib(), L.stream_ptr
    bbox = torch.empty(B, 6, device=dev, dtype=torch.float32)
    keys = torch.empty(T, device=dev, dtype=torch.int64)
    flags, status = (torch.empty(B, device=dev, dtype=torch.int32) for _ in range(2))
    L.check(lib.sfmi_meshtree_keys_f32(L.ptr(vf), L.ptr(ff), L.ptr(vod), L.ptr(tod), B, T, L.ptr(bbox), L.ptr(keys), L.ptr(flags), st()),
            "sfmi_meshtree_keys_f32")
    order = torch.sort(keys, stable=True).indices if T else keys          # (shape, key, face index)
    rec = torch.empty(5 * T, 4, device=dev, dtype=torch.float32)
    orig = torch.empty(T, device=dev, dtype=torch.int32)
    nodes = torch.empty(NODE * NN, 4, device=dev, dtype=torch.float32)
    mom = torch.empty(NN, MOM, device=dev, dtype=torch.float64)
    L.check(lib.sfmi_meshtree_build_f32(L.ptr(vf), L.ptr(ff), L.ptr(vod), L.ptr(tod), L.ptr(nod), L.ptr(order), L.ptr(flags), B, T,
                                        int(np.diff(to).max()), L.ptr(rec) if T else None, L.ptr(orig) if T else None,
                                        L.ptr(nodes) if T else None, L.ptr(mom) if T else None, L.ptr(status), st()),
            "sfmi_meshtree_build_f32")
    return MeshTree(rec=rec, orig=orig, nodes=nodes, mom=mom, bbox=bbox, keys=keys, order=order, status=status, voff=vo, toff=to, noff=no,
                    toff_dev=tod, noff_dev=nod, device=dev)


def _tree_arg(tree, what):
    if not isinstance(tree, MeshTree):
        raise L.SfmiError(f"{what}: tree must be a MeshTree (mesh_tree_dev)")
    return tree


def _beta(beta, what):
    return check_number(beta, what, "beta", 0.0, float("inf"))


def _spread10(u):
    u = (u | (u << 16)) & 0x030000FF
    u = (u | (u << 8)) & 0x0300F00F
    u = (u | (u << 4)) & 0x030C30C3
    return (u | (u << 2)) & 0x09249249


def _query_order(q, qo):
    """the order the device takes the queries in: by (set, 30-bit Morton code in the queries' bounding box), so that the 64 queries of
    a wave are neighbours.  Performance only: a query's results do not depend on its wave-mates."""
    x = torch.nan_to_num(q, nan=0.0, posinf=0.0, neginf=0.0)
    lo, hi = x.min(0).values, x.max(0).values
    u = ((x - lo) / (hi - lo).clamp_min(1e-30) * 1024.0).long().clamp_(0, 1023)
    key = (set_ids(qo, q.device) << 30) | (_spread10(u[:, 0]) << 2) | (_spread10(u[:, 1]) << 1) | _spread10(u[:, 2])
    return torch.sort(key, stable=True).indices


def signed_distance_tree_dev(queries, tree, qoff=None, beta=2.0, return_winding=False, counters=None):
    """Signed distance of every query to the mesh of its set, through the tree.  Outputs as meshsdf.signed_distance_dev:
    -> S (N,) f32, I (N,) int32 ORIGINAL face index local to the shape, C (N,3) f32 (, W (N,) f32 the tree-code winding number),
    status (B,) int32.  sqrt(d2), I and C are bit for bit the brute route's; S = -sqrt(d2) where |W_tree| > 0.5.  counters: None, or a
    (3,) int64 HIP tensor that gains (faces evaluated, expansions taken, queries)."""
    what = "signed_distance_tree_dev"
    if not isinstance(queries, torch.Tensor) or queries.dim() != 2 or queries.shape[1] != 3:
        raise L.SfmiError(f"{what}: queries must be an (N,3) torch tensor")
    tree = _tree_arg(tree, what)
    beta = _beta(beta, what)
    qo = host_offsets(qoff, queries.shape[0], f"{what} qoff")
    if len(qo) != len(tree.toff):
        raise L.SfmiError(f"{what}: {len(qo) - 1} query sets for a tree of {tree.B} meshes")
    if ((np.diff(tree.toff) == 0) & (np.diff(qo) > 0)).any():
        raise L.SfmiError(f"{what}: a shape has queries but no faces")
    dev = on_device(what, queries, tree.rec)
    B, N = tree.B, int(queries.shape[0])
    S = torch.empty(N, device=dev, dtype=torch.float32)
    I = torch.empty(N, device=dev, dtype=torch.int32)
    C = torch.empty(N, 3, device=dev, dtype=torch.float32)
    W = torch.empty(N, device=dev, dtype=torch.float32)
    if N:
        qf = queries.float().contiguous()
        order = _query_order(qf, qo)
        qs = qf[order].contiguous()
        bo = np.concatenate([[0], np.cumsum((np.diff(qo) + LEAF - 1) // LEAF)]).astype(np.int64)
        qod, bod = offsets_dev(qo, dev), offsets_dev(bo, dev)
        Ss, Is, Cs, Ws = (torch.empty_like(x) for x in (S, I, C, W))
        L.check(L.lib().sfmi_meshtree_query_f32(L.ptr(qs), L.ptr(qod), L.ptr(bod), int(bo[-1]), L.ptr(tree.toff_dev), L.ptr(tree.noff_dev),
                                                L.ptr(tree.rec), L.ptr(tree.orig), L.ptr(tree.nodes), L.ptr(tree.status), B, N, beta,
                                                L.ptr(Ss), L.ptr(Is), L.ptr(Cs), L.ptr(Ws), L.ptr(counters), L.stream_ptr()),
                "sfmi_meshtree_query_f32")
        S[order], I[order], C[order], W[order] = Ss, Is, Cs, Ws
    return (S, I, C, W, tree.status) if return_winding else (S, I, C, tree.status)


def _lattice(grid_dim, bbox, what):
    G = check_count(grid_dim, what, "grid_dim")
    lo, hi = (np.ascontiguousarray(np.asarray(x, np.float64).reshape(3)) for x in bbox)
    if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
        raise L.SfmiError(f"{what}: bbox must be finite")
    return G, lo, hi


def mesh_occupancy_tree_dev(tree, grid_dim=256, bbox=UNIT_BOX, beta=2.0, return_status=False, counters=None):
    """Inside test |W_tree| > 0.5 at every point of meshsdf.mesh_occupancy_dev's lattice (makeGrid(bbox, [grid_dim]*3, mode="on",
    indexing="ij"), generated in the kernel) -> (B, G, G, G) uint8 (, status (B,)).  One wave per 4 x 4 x 4 block of lattice points
    writes its 64 results: there is no workspace.  A shape without faces raises SfmiError."""
    what = "mesh_occupancy_tree_dev"
    tree = _tree_arg(tree, what)
    if (np.diff(tree.toff) == 0).any():
        raise L.SfmiError(f"{what}: a shape has no faces")
    G, lo, hi = _lattice(grid_dim, bbox, what)
    beta = _beta(beta, what)
    B = tree.B
    if ((G + 3) // 4) ** 3 * B >= 2 ** 31:
        raise L.SfmiError(f"{what}: {B} lattices of {G}^3 are too many blocks for one launch")
    dev = on_device(what, tree.rec)
    occ = torch.empty(B, G, G, G, device=dev, dtype=torch.uint8)
    L.check(L.lib().sfmi_meshtree_occupancy_f32(L.ptr(tree.toff_dev), L.ptr(tree.noff_dev), L.ptr(tree.rec), L.ptr(tree.nodes),
                                                L.ptr(tree.status), B, G, lo.ctypes.data, hi.ctypes.data, beta, L.ptr(occ), L.ptr(counters),
                                                L.stream_ptr()), "sfmi_meshtree_occupancy_f32")
    return (occ, tree.status) if return_status else occ


def volumetric_iou_dev(occ_a, occ_b, thresh=0.5):
    """vqdif/common.py:8-36 compute_iou: occ_a, occ_b (B, ...) tensors of one shape on one device -> (B,) f64 = |a & b| / |a | b| with
    a = occ_a >= thresh, flattened per item; the counts are int64 and an empty union gives NaN (the reference's 0 / 0)."""
    what = "volumetric_iou_dev"
    if not isinstance(occ_a, torch.Tensor) or not isinstance(occ_b, torch.Tensor):
        raise L.SfmiError(f"{what}: occ_a / occ_b must be torch tensors")
    if occ_a.dim() < 1 or occ_a.shape != occ_b.shape or occ_a.device != occ_b.device:
        raise L.SfmiError(f"{what}: occ_a and occ_b must have one shape (B, ...) and one device, got {tuple(occ_a.shape)} and "
                          f"{tuple(occ_b.shape)}")
    thresh = check_number(thresh, what, "thresh", -float("inf"), float("inf"))
    a, b = ((x >= thresh).reshape(x.shape[0], -1) for x in (occ_a, occ_b))
    inter, union = (a & b).sum(1, dtype=torch.int64), (a | b).sum(1, dtype=torch.int64)
    return inter.double() / union.double()


def mesh_iou_dev(verts_a, faces_a, voff_a, toff_a, verts_b, faces_b, voff_b, toff_b, grid_dim=128, bbox=UNIT_BOX, method="tree", beta=2.0):
    """The volumetric IoU of mesh i of batch a against mesh i of batch b on the grid_dim^3 lattice of bbox -> (B,) f64.  method "tree"
    (mesh_occupancy_tree_dev at beta) or "brute" (meshsdf.mesh_occupancy_dev)."""
    from . import meshsdf
    what = "mesh_iou_dev"
    if method not in ("tree", "brute"):
        raise L.SfmiError(f"{what}: method must be 'tree' or 'brute', got {method!r}")
    a, b = mesh_args(verts_a, faces_a, voff_a, toff_a, f"{what} a"), mesh_args(verts_b, faces_b, voff_b, toff_b, f"{what} b")
    if len(a[3]) != len(b[3]):
        raise L.SfmiError(f"{what}: {len(a[3]) - 1} meshes against {len(b[3]) - 1}")
    _lattice(grid_dim, bbox, what)
    _beta(beta, what)
    on_device(what, verts_a, faces_a, verts_b, faces_b)
    if method == "tree":
        oa, ob = (mesh_occupancy_tree_dev(mesh_tree_dev(*m), grid_dim, bbox, beta) for m in (a, b))
    else:
        oa, ob = (meshsdf.mesh_occupancy_dev(*m, grid_dim=grid_dim, bbox=bbox) for m in (a, b))
    return volumetric_iou_dev(oa, ob)
