"""Edge-collapse mesh decimation on the device — host side of csrc/collapse.hip.

The reference's array2mesh(..., if_decimate=True) runs igl.decimate, an edge collapse (xgutils/geoutil.py:175-233).  `simplify.decimate_dev`
keeps that interface by vertex clustering: fast, but the budget is only an upper bound, detail is spread evenly whatever the curvature,
and thin parts leave duplicate and non-manifold faces.  Here the ragged meshes of `marching_cubes_dev` / `extract_sparse_dev` are
decimated where they are by rounds of independent quadric edge collapses: the face count lands on the budget (or one below), the
Euler characteristic, the boundary and every non-manifold edge are kept, and no two faces share their three vertices.  The contract is in
include/sfmi.h, its plain Python statement in tests/collapse_ref.py; the results are equal bit for bit.  There is no CPU fallback.

  collapse_dev(verts, faces, voff, toff, target, reg, max_rounds, details)          -> verts, faces, voff, toff, status[, rounds]
  decimate_collapse_dev(verts, faces, voff, toff, decimate_face, precluster, ...)  -> verts, faces, voff, toff, status
  mesh_topology_dev(verts, faces, voff, toff)                                      -> counts (B,6), status

verts (V,3) f32 and faces (T,3) int32 (indices local per shape) are device tensors, voff / toff (B+1) host offsets (None: one shape;
the argument checks are _ragged.py's).  status (B) int32 on the device: 0 done, 1 no vertices, 2 a face index outside
the shape, 3 a non-finite vertex (such a shape comes back empty), 4 stalled (no edge may collapse any more: the shape comes back as far
as it got), 5 the round cap.  Results are bit-identical from run to run, a batch equals per-shape calls, and neither depends on
`rounds_per_sync`.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L
from . import _ragged
from ._ragged import check_count, check_number, excl, i32_dev, mesh_args, on_device, runs

MAX_ROUNDS = 1024       # the default round cap: DESIGN.md §5.25 (the measured meshes stop within 141 rounds)
ROUNDS_PER_SYNC = 8     # rounds between two read-backs of the number of shapes that go on
TOPOLOGY = ("verts", "edges", "faces", "boundary", "nonmanifold", "euler")   # the columns of mesh_topology_dev
read_backs = 0          # device -> host read-backs so far (tools/kbench_collapse.py reports the number per call)

# how this module calls mesh_args: 32-bit batch-wide indices, offsets of any array shape
_MESH = dict(index32=True, flatten_offsets=True)


class _State:
    """the workspace of one call and the arrays the sorts between the passes go through"""

    def __init__(self, verts, faces, vo, to, target, max_rounds):
        self.lib, self.dev = L.lib(), verts.device
        self.B, self.V, self.T = len(vo) - 1, verts.shape[0], faces.shape[0]
        self.dims = (self.B, self.V, self.T)
        self.target, self.max_rounds = target, max_rounds
        nbytes = int(self.lib.sfmi_collapse_workspace_bytes(*self.dims))
        if nbytes <= 0:
            raise L.SfmiError("sfmi_collapse_workspace_bytes: the batch is too large for 32-bit indices")
        self.ws = _ragged.workspace(nbytes, self.dev)
        self.voff, self.toff = i32_dev(vo, self.dev), i32_dev(to, self.dev)
        n = max(3 * self.T, 1)
        i32, i64 = dict(device=self.dev, dtype=torch.int32), dict(device=self.dev, dtype=torch.int64)
        self.ekey, self.cand, self.wkey = (torch.empty(n, **i64) for _ in range(3))
        self.ckey, self.ecnt, self.wshape = (torch.empty(n, **i32) for _ in range(3))
        self.xs = torch.empty(n, 3, device=self.dev, dtype=torch.float32)
        self.shapes = torch.arange(self.B, **i32)
        L.check(self.lib.sfmi_collapse_init_f32(L.ptr(verts), L.ptr(faces), L.ptr(self.voff), L.ptr(self.toff), *self.dims, target,
                                                max_rounds, L.ptr(self.ws), L.stream_ptr()), "sfmi_collapse_init_f32")

    def edge_table(self):
        """records, the two sorts, the run lengths: what a round and mesh_topology_dev share"""
        lib, st, n = self.lib, L.stream_ptr, 3 * self.T
        L.check(lib.sfmi_collapse_records_i32(*self.dims, L.ptr(self.ekey), L.ptr(self.ckey), L.ptr(self.ws), st()), "sfmi_collapse_records_i32")
        self.skey, self.sidx = torch.sort(self.ekey[:n])
        self.corder, self.cseg = runs(self.ckey[:n], self.V)
        L.check(lib.sfmi_collapse_runs_i32(L.ptr(self.skey), *self.dims, L.ptr(self.ecnt), L.ptr(self.ws), st()), "sfmi_collapse_runs_i32")

    def quadrics(self):
        L.check(self.lib.sfmi_collapse_quadrics_f64(L.ptr(self.corder), L.ptr(self.cseg), *self.dims, L.ptr(self.ws), L.stream_ptr()),
                "sfmi_collapse_quadrics_f64")

    def round(self, reg):
        lib, st, n, B = self.lib, L.stream_ptr, 3 * self.T, self.B
        erank = torch.cumsum(self.ecnt[:n] > 0, 0, dtype=torch.int32) - 1
        L.check(lib.sfmi_collapse_eval_f64(L.ptr(self.skey), L.ptr(self.ecnt), L.ptr(erank), L.ptr(self.corder), L.ptr(self.cseg), *self.dims,
                                           reg, L.ptr(self.cand), L.ptr(self.xs), L.ptr(self.ws), st()), "sfmi_collapse_eval_f64")
        L.check(lib.sfmi_collapse_win_i32(L.ptr(self.skey), L.ptr(self.sidx), L.ptr(self.cand), L.ptr(self.corder), L.ptr(self.cseg),
                                          *self.dims, L.ptr(self.wkey), L.ptr(self.wshape), L.ptr(self.ws), st()), "sfmi_collapse_win_i32")
        # the budget's order: by key, then (stably) by shape; one shape: the winners are in front already
        order = torch.sort(self.wkey[:n]).indices
        sshape = self.wshape[:n][order]
        if B > 1:
            s = torch.sort(sshape, stable=True)
            order, sshape = order[s.indices], s.values
        order, sshape = order.contiguous(), sshape.contiguous()
        sstart = torch.searchsorted(sshape, self.shapes).to(torch.int32)
        L.check(lib.sfmi_collapse_apply_f32(L.ptr(self.skey), L.ptr(order), L.ptr(sshape), L.ptr(sstart), L.ptr(self.xs), L.ptr(self.corder),
                                            L.ptr(self.cseg), *self.dims, self.target, self.max_rounds, L.ptr(self.ws), st()),
                "sfmi_collapse_apply_f32")

    def report(self):
        """-> status, rounds, nalive (B each), nactive (1): int32 views of one device tensor"""
        B = self.B
        out = torch.empty(3 * B + 1, device=self.dev, dtype=torch.int32)
        L.check(self.lib.sfmi_collapse_report_i32(*self.dims, L.ptr(self.ws), L.ptr(out[:B]), L.ptr(out[B:2 * B]), L.ptr(out[2 * B:3 * B]),
                                                  L.ptr(out[3 * B:]), L.stream_ptr()), "sfmi_collapse_report_i32")
        return out


def _collapse(verts, faces, vo, to, target, reg, max_rounds, rounds_per_sync):
    """The rounds of csrc/collapse.hip on a checked batch of B >= 1 shapes -> verts, faces (device), voff, toff, status (device), rounds
    (host).  One read-back per `rounds_per_sync` rounds (a counter) and one at the end (sizes)."""
    global read_backs
    s = _State(verts, faces, vo, to, target, max_rounds)
    lib, st, dev, B, V, T = s.lib, L.stream_ptr, s.dev, s.B, s.V, s.T
    first = True
    while T > 0:
        go = int(s.report()[3 * B:].item())                                   # a read-back: shapes that go on
        read_backs += 1
        if go == 0:
            break
        for _ in range(rounds_per_sync):                                      # a round of a batch whose shapes have all stopped changes nothing
            s.edge_table()
            if first:
                s.quadrics()
                first = False
            s.round(reg)
    out_v, out_f = torch.empty(max(V, 1), 3, device=dev, dtype=torch.float32), torch.empty(max(T, 1), 3, device=dev, dtype=torch.int32)
    vkeep, fkeep = torch.empty(max(V, 1), device=dev, dtype=torch.uint8), torch.empty(max(T, 1), device=dev, dtype=torch.uint8)
    L.check(lib.sfmi_collapse_finish_f32(L.ptr(s.voff), B, V, T, L.ptr(s.ws), L.ptr(out_v), L.ptr(out_f), L.ptr(vkeep), L.ptr(fkeep), st()),
            "sfmi_collapse_finish_f32")
    # compaction: the prefix counts and the emit pass of components
    vex, fex = excl(vkeep[:V]), excl(fkeep[:T])
    nvoff, ntoff = vex[s.voff.long()].contiguous(), fex[s.toff.long()].contiguous()
    rep = s.report()
    h = torch.cat([nvoff, ntoff, rep[:2 * B]]).cpu().numpy().astype(np.int64)  # the last read-back: sizes, rounds
    read_backs += 1
    nvo, nto, rounds = h[:B + 1], h[B + 1:2 * B + 2], h[3 * B + 2:]
    nV, nT = int(nvo[-1]), int(nto[-1])
    res_v, res_f = torch.empty(max(nV, 1), 3, device=dev, dtype=torch.float32), torch.empty(max(nT, 1), 3, device=dev, dtype=torch.int32)
    vincl, fincl = vex[1:].contiguous(), fex[1:].contiguous()
    L.check(lib.sfmi_cc_emit_f32(L.ptr(out_v), L.ptr(out_f), L.ptr(s.voff), L.ptr(s.toff), L.ptr(vkeep), L.ptr(fkeep), L.ptr(vincl), L.ptr(fincl),
                                 L.ptr(nvoff), B, V, T, nV, nT, L.ptr(res_v), L.ptr(res_f), st()), "sfmi_cc_emit_f32")
    return res_v[:nV], res_f[:nT], nvo, nto, rep[:B].clone(), rounds


def _take(verts, faces, vo, to, shapes):
    """the sub-batch of the listed shapes"""
    v = torch.cat([verts[vo[b]:vo[b + 1]] for b in shapes])
    f = torch.cat([faces[to[b]:to[b + 1]] for b in shapes])
    return (v, f, np.concatenate([[0], np.cumsum([vo[b + 1] - vo[b] for b in shapes])]).astype(np.int64),
            np.concatenate([[0], np.cumsum([to[b + 1] - to[b] for b in shapes])]).astype(np.int64))


def collapse_dev(verts, faces, voff, toff, target, reg=1e-3, max_rounds=MAX_ROUNDS, details=False, rounds_per_sync=ROUNDS_PER_SYNC):
    """Edge-collapse every shape with more than `target` faces down to `target` faces (or target - 1: a collapse removes two); a shape
    at or under the budget comes back unchanged, bit for bit, and uninspected (status 0, or 1 without vertices).  reg > 0 pulls an
    edge's new vertex towards its midpoint where the quadric leaves it free (§5.10's regulariser).
    -> verts, faces (device), voff, toff (host), status (B) int32 (device); with details also rounds (B) host ints."""
    what = "collapse_dev"
    target = check_count(target, what, "target", lo=0)
    reg = check_number(reg, what, "reg", 0.0, float("inf"), lo_open=True)
    max_rounds = check_count(max_rounds, what, "max_rounds", lo=0)
    rounds_per_sync = check_count(rounds_per_sync, what, "rounds_per_sync", lo=1)
    verts, faces, vo, to = mesh_args(verts, faces, voff, toff, what, **_MESH)
    on_device(what, verts, faces)
    B = len(vo) - 1
    status = torch.from_numpy((np.diff(vo) == 0).astype(np.int32)).to(verts.device)
    rounds = np.zeros(B, np.int64)
    over = [b for b in range(B) if to[b + 1] - to[b] > target]
    if not over:
        return (verts, faces, vo, to, status) + ((rounds,) if details else ())
    sub = (verts, faces, vo, to) if len(over) == B else _take(verts, faces, vo, to, over)
    sv, sf, svo, sto, sst, srounds = _collapse(*sub, target, reg, max_rounds, rounds_per_sync)
    rounds[over] = srounds
    if len(over) == B:
        return (sv, sf, svo, sto, sst) + ((rounds,) if details else ())
    status[torch.as_tensor(over, device=verts.device)] = sst
    pv, pf, where = [], [], {b: k for k, b in enumerate(over)}
    for b in range(B):
        if b in where:
            k = where[b]
            pv.append(sv[svo[k]:svo[k + 1]]), pf.append(sf[sto[k]:sto[k + 1]])
        else:
            pv.append(verts[vo[b]:vo[b + 1]]), pf.append(faces[to[b]:to[b + 1]])
    nvo = np.concatenate([[0], np.cumsum([p.shape[0] for p in pv])]).astype(np.int64)
    nto = np.concatenate([[0], np.cumsum([p.shape[0] for p in pf])]).astype(np.int64)
    return (torch.cat(pv), torch.cat(pf), nvo, nto, status) + ((rounds,) if details else ())


def decimate_collapse_dev(verts, faces, voff, toff, decimate_face=4096, precluster=None, bbox=None, reg=1e-3, max_rounds=MAX_ROUNDS):
    """array2mesh's `if_decimate` step by edge collapse.  precluster = k: a shape is first clustered by `simplify.decimate_dev` to at
    most k * decimate_face faces over `bbox` (default: simplify's unit box) and then collapsed - the hybrid route for meshes of millions
    of faces; None: pure collapse.  A shape the clustering refuses (status 1..3) keeps that status.
    -> verts, faces (device), voff, toff (host), status (B) int32 (device)."""
    what = "decimate_collapse_dev"
    target = check_count(decimate_face, what, "decimate_face", lo=0)
    if precluster is None:
        return collapse_dev(verts, faces, voff, toff, target, reg, max_rounds)
    k = check_count(precluster, what, "precluster", lo=1)
    if k * target >= 2 ** 31:
        raise L.SfmiError(f"{what}: precluster * decimate_face must stay below 2^31")
    from . import simplify
    v, f, vo, to, st0 = simplify.decimate_dev(verts, faces, voff, toff, k * target, simplify.UNIT_BOX if bbox is None else bbox, reg)[:5]
    v, f, vo, to, st1 = collapse_dev(v, f, vo, to, target, reg, max_rounds)
    return v, f, vo, to, torch.where(st0 != 0, st0, st1)


def mesh_topology_dev(verts, faces, voff, toff):
    """The edge table on its own: per shape the vertices that a face names, the distinct undirected edges, the faces, the boundary edges
    (in one face), the non-manifold edges (in more than two) and the Euler characteristic V - E + F.  A closed manifold surface has no
    boundary and no non-manifold edge; each of its components of genus g adds 2 - 2g to the characteristic.  A face with a repeated index
    counts as a face and names its vertices but has no edges.
    -> counts (B,6) int32 in the order of TOPOLOGY (zeros where status is not 0), status (B) int32: 0, or 1..3 as above (device)."""
    what = "mesh_topology_dev"
    verts, faces, vo, to = mesh_args(verts, faces, voff, toff, what, **_MESH)
    dev = on_device(what, verts, faces)
    s = _State(verts, faces, vo, to, 0, 1)
    B, V, T = s.dims
    ref, cnt = torch.zeros(max(V, 1), device=dev, dtype=torch.uint8), torch.zeros(3, B, device=dev, dtype=torch.int32)
    if T > 0:
        s.edge_table()
        L.check(s.lib.sfmi_collapse_topology_i32(L.ptr(s.skey), L.ptr(s.sidx), L.ptr(s.ecnt), B, V, T, L.ptr(s.ws), L.ptr(ref), L.ptr(cnt),
                                                 L.stream_ptr()), "sfmi_collapse_topology_i32")
    rep = s.report()
    status, nface = rep[:B].clone(), rep[2 * B:3 * B]
    nref = torch.diff(excl(ref[:V])[s.voff.long()])
    return torch.stack([nref, cnt[0], nface, cnt[1], cnt[2], nref - cnt[0] + nface], 1).to(torch.int32).contiguous(), status
