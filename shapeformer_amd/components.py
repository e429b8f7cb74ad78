"""Mesh connected components on the device — host side of csrc/components.hip.

A completion sampled token by token is not one surface: a wrong (pos, val) tuple leaves a blob of occupancy in an empty cell and
marching cubes turns it into a floater.  The reference has a stub for the step that would drop it: xgutils/geoutil.py:151-163
filterMesh, a vertex-mask filter with `# TODO filterF`.  Here the ragged meshes of `marching_cubes_dev` / `extract_sparse_dev` /
`decimate_dev` are labelled, measured and filtered where they are, in HBM.  The contract is in include/sfmi.h, its numpy statement in
tests/components_ref.py.  There is no CPU fallback.

  mesh_components_dev(verts, faces, voff, toff)                                   -> vlabel, flabel, coff, stats, status
  keep_components_dev(verts, faces, voff, toff, top=None, min_share=0.0, by="area") -> verts, faces, voff, toff, status, kept, coff
  filter_components_dev(verts, faces, voff, toff, spec)                           -> verts, faces, voff, toff, status, report

verts (V,3) f32 and faces (T,3) int32 (indices local per shape) are device tensors, voff / toff (B+1) host offsets (None: one shape;
the argument checks are _ragged.py's).  Labels are local per shape, -1 for a vertex no face names; the components of a
shape are numbered by their smallest vertex index.  status (B) int32 on the device: 0 ok, 1 no vertices, 2 a face index outside the
shape, 3 a non-finite vertex (such a shape has no components and comes back empty).  Results are bit-identical from run to run and a
batch equals per-shape calls.  Each call reads sizes back once.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib as L
from ._ragged import excl, i32_dev, mesh_args, on_device, runs

MEASURES = ("area", "faces", "volume")
read_backs = 0          # device -> host size read-backs so far (tools/kbench_components.py reports the number per call)


# how this module calls mesh_args: 32-bit batch-wide indices; B = 0 is a batch (it comes back empty); offsets of any array shape
_MESH = dict(index32=True, empty_ok=True, flatten_offsets=True)


def _selection(top, min_share, by):
    if by not in MEASURES:
        raise L.SfmiError(f"components: by = {by!r} must be one of {MEASURES}")
    if top is not None:
        if isinstance(top, bool) or not isinstance(top, (int, np.integer)) or top < 1:
            raise L.SfmiError(f"components: top = {top!r} must be None or an int >= 1")
        top = int(top)
    try:
        share = float(min_share)
    except (TypeError, ValueError):
        share = math.nan
    if not (math.isfinite(share) and 0.0 <= share <= 1.0):
        raise L.SfmiError(f"components: min_share = {min_share!r} must lie in [0, 1]")
    return top, share, by


def parse_keep(spec):
    """The `keep_components` option of the callbacks and of array2mesh -> keyword arguments of keep_components_dev, or None (off).
    "largest": top=1; an int k: top=k; a float in (0, 1]: min_share (by area); a dict: the keyword arguments themselves."""
    if spec is None:
        return None
    if isinstance(spec, dict):
        extra = set(spec) - {"top", "min_share", "by"}
        if extra:
            raise L.SfmiError(f"keep_components: unknown keys {sorted(extra)}")
        kw = dict(spec)
    elif isinstance(spec, str):
        if spec != "largest":
            raise L.SfmiError(f"keep_components = {spec!r}: the only name is 'largest'")
        kw = dict(top=1)
    elif isinstance(spec, bool):
        raise L.SfmiError(f"keep_components = {spec!r}: expected None, 'largest', an int, a float in (0, 1] or a dict")
    elif isinstance(spec, (int, np.integer)):
        kw = dict(top=int(spec))
    elif isinstance(spec, (float, np.floating)):
        if not 0.0 < float(spec) <= 1.0:
            raise L.SfmiError(f"keep_components = {spec!r}: a float must lie in (0, 1]")
        kw = dict(min_share=float(spec), by="area")
    else:
        raise L.SfmiError(f"keep_components = {spec!r}: expected None, 'largest', an int, a float in (0, 1] or a dict")
    _selection(kw.get("top"), kw.get("min_share", 0.0), kw.get("by", "area"))
    return kw


def _label(verts, faces, vo, to):
    """The labelling and statistics passes of csrc/components.hip on a checked batch of B >= 1 shapes.  No read-back: the component
    tables have the capacity nC = min(V, T) + 1; the entries from coff[B] on are empty (no vertices, no faces, zero sums)."""
    lib, st, dev = L.lib(), L.stream_ptr, verts.device
    B, V, T = len(vo) - 1, verts.shape[0], faces.shape[0]
    nC = min(V, T) + 1
    i32 = dict(device=dev, dtype=torch.int32)
    voff, toff = i32_dev(vo, dev), i32_dev(to, dev)
    parent, root, isroot, vlabel, vkey = (torch.empty(max(V, 1), **i32) for _ in range(5))
    flabel, fkey = (torch.empty(max(T, 1), **i32) for _ in range(2))
    ref = torch.empty(max(V, 1), device=dev, dtype=torch.uint8)
    flags, status = torch.empty(B, **i32), torch.empty(B, **i32)
    L.check(lib.sfmi_cc_init_f32(L.ptr(verts), L.ptr(faces), L.ptr(voff), L.ptr(toff), B, V, T, L.ptr(parent), L.ptr(ref), L.ptr(flags),
                                 st()), "sfmi_cc_init_f32")
    L.check(lib.sfmi_cc_hook_i32(L.ptr(faces), L.ptr(voff), L.ptr(toff), L.ptr(flags), B, V, T, L.ptr(parent), L.ptr(ref), st()),
            "sfmi_cc_hook_i32")
    L.check(lib.sfmi_cc_flatten_i32(L.ptr(parent), L.ptr(ref), V, L.ptr(root), L.ptr(isroot), st()), "sfmi_cc_flatten_i32")
    rank = torch.cumsum(isroot[:V], 0, dtype=torch.int32)
    coff = excl(isroot[:V])[voff.long()].contiguous()                       # (B+1): the roots before each shape
    L.check(lib.sfmi_cc_number_i32(L.ptr(faces), L.ptr(voff), L.ptr(toff), L.ptr(flags), L.ptr(root), L.ptr(ref), L.ptr(rank), L.ptr(coff),
                                   B, V, T, L.ptr(vlabel), L.ptr(flabel), L.ptr(vkey), L.ptr(fkey), L.ptr(status), st()), "sfmi_cc_number_i32")
    # the runs of the sorted keys: where each component's faces start (the order of the sums) and how many vertices / faces it has
    forder, seg = runs(fkey[:T], nC)
    n_face, n_vert = torch.diff(seg), torch.diff(runs(vkey[:V], nC)[1])
    K = int(lib.sfmi_cc_chunk())
    nW = T // K + min(nC, T)                                                 # sum of ceil(n_c / K) <= T / K + components with faces
    choff = excl((n_face + (K - 1)) // K)
    part = torch.empty(2 * max(nW, 1), device=dev, dtype=torch.float64)
    area, volume = torch.empty(nC, device=dev, dtype=torch.float64), torch.empty(nC, device=dev, dtype=torch.float64)
    L.check(lib.sfmi_cc_stats_f64(L.ptr(verts), L.ptr(faces), L.ptr(voff), L.ptr(toff), L.ptr(forder), L.ptr(seg), L.ptr(choff), B, V, T,
                                  nC, nW, L.ptr(part), L.ptr(area), L.ptr(volume), st()), "sfmi_cc_stats_f64")
    return dict(B=B, V=V, T=T, nC=nC, voff=voff, toff=toff, coff=coff, vlabel=vlabel[:V], flabel=flabel[:T], status=status,
                n_vert=n_vert, n_face=n_face, area=area, volume=volume)


def _empty_batch(verts, faces):
    dev = verts.device
    z = lambda dt: torch.empty(0, device=dev, dtype=dt)
    return z(torch.int32), dict(n_vert=z(torch.int32), n_face=z(torch.int32), area=z(torch.float64), volume=z(torch.float64))


def mesh_components_dev(verts, faces, voff, toff):
    """-> vlabel (V) int32, flabel (T) int32 (device; ids local per shape, -1 = unreferenced / a shape whose status is not 0),
    coff (B+1) host offsets into the component table, stats: dict of device tensors over the component table (n_vert, n_face int32,
    area, volume f64), status (B) int32 (device)."""
    global read_backs
    verts, faces, vo, to = mesh_args(verts, faces, voff, toff, "mesh_components_dev", **_MESH)
    on_device("mesh_components_dev", verts, faces)
    if len(vo) == 1:
        e, stats = _empty_batch(verts, faces)
        return e, e.clone(), np.zeros(1, np.int64), stats, e.clone()
    r = _label(verts, faces, vo, to)
    coff = r["coff"].cpu().numpy().astype(np.int64)                          # the one read-back: sizes
    read_backs += 1
    C = int(coff[-1])
    return r["vlabel"], r["flabel"], coff, {k: r[k][:C] for k in ("n_vert", "n_face", "area", "volume")}, r["status"]


def _measure(r, by):
    return r["area"] if by == "area" else (r["n_face"].double() if by == "faces" else r["volume"].abs())


def _select(r, top, share, by):
    """keep flags over the component table (capacity nC) by the selection rule, on the device"""
    B, nC, coff = r["B"], r["nC"], r["coff"]
    dev = coff.device
    ids = torch.arange(nC, device=dev, dtype=torch.int32)
    cshape = torch.searchsorted(coff[1:].contiguous(), ids, right=True)      # B for the empty entries behind the last component
    m = _measure(r, by)
    # the largest measure per shape, then 0 for the empty tail.  The table is ordered by shape: a segmented maximum (a scatter with
    # atomic maxima would have every entry hit B addresses); one shape: the maximum (the tail's measures are 0, none is negative)
    if B == 1:
        mmax = torch.cat([m.max().reshape(1), m.new_zeros(1)])
    else:
        ends = torch.cat([coff.long(), coff.new_full((1,), nC, dtype=torch.int64)])
        mmax = torch.segment_reduce(m, "max", offsets=ends, unsafe=True, initial=0.0)
    keep = (cshape < B) & (m >= share * mmax[cshape])
    if top is not None:
        order = torch.sort(m, descending=True, stable=True).indices          # equal measures stay in id order
        if B > 1:
            order = order[torch.sort(cshape[order], stable=True).indices]    # by shape, then measure descending, then id
        pos = torch.empty(nC, device=dev, dtype=torch.int64)
        pos[order] = torch.arange(nC, device=dev, dtype=torch.int64)
        keep &= (pos - coff.long()[cshape]) < top
    return keep


def _keep(verts, faces, vo, to, top, share, by):
    global read_backs
    dev = verts.device
    if len(vo) == 1:
        z = np.zeros(1, np.int64)
        return dict(verts=verts[:0], faces=faces[:0], voff=z, toff=z.copy(), status=torch.empty(0, device=dev, dtype=torch.int32),
                    kept=torch.empty(0, device=dev, dtype=torch.bool), coff=z.copy(), area=torch.empty(0, device=dev, dtype=torch.float64))
    lib, st = L.lib(), L.stream_ptr
    r = _label(verts, faces, vo, to)
    B, V, T, nC = r["B"], r["V"], r["T"], r["nC"]
    keep = _select(r, top, share, by)
    k8 = keep.to(torch.uint8)
    vkeep, fkeep = torch.empty(max(V, 1), device=dev, dtype=torch.uint8), torch.empty(max(T, 1), device=dev, dtype=torch.uint8)
    L.check(lib.sfmi_cc_mark_i32(L.ptr(r["vlabel"]), L.ptr(r["flabel"]), L.ptr(r["voff"]), L.ptr(r["toff"]), L.ptr(r["coff"]), L.ptr(k8),
                                 B, V, T, nC, L.ptr(vkeep), L.ptr(fkeep), st()), "sfmi_cc_mark_i32")
    vex, fex = excl(vkeep[:V]), excl(fkeep[:T])
    nvoff, ntoff = vex[r["voff"].long()].contiguous(), fex[r["toff"].long()].contiguous()
    h = torch.cat([r["coff"], nvoff, ntoff]).cpu().numpy().astype(np.int64)  # the one read-back: sizes
    read_backs += 1
    coff, nvo, nto = h[:B + 1], h[B + 1:2 * B + 2], h[2 * B + 2:]
    nV, nT, C = int(nvo[-1]), int(nto[-1]), int(coff[-1])
    out_v = torch.empty(max(nV, 1), 3, device=dev, dtype=torch.float32)
    out_f = torch.empty(max(nT, 1), 3, device=dev, dtype=torch.int32)
    vincl, fincl = vex[1:].contiguous(), fex[1:].contiguous()
    L.check(lib.sfmi_cc_emit_f32(L.ptr(verts), L.ptr(faces), L.ptr(r["voff"]), L.ptr(r["toff"]), L.ptr(vkeep), L.ptr(fkeep), L.ptr(vincl),
                                 L.ptr(fincl), L.ptr(nvoff), B, V, T, nV, nT, L.ptr(out_v), L.ptr(out_f), st()), "sfmi_cc_emit_f32")
    return dict(verts=out_v[:nV], faces=out_f[:nT], voff=nvo, toff=nto, status=r["status"], kept=keep[:C], coff=coff, area=r["area"][:C])


def keep_components_dev(verts, faces, voff, toff, top=None, min_share=0.0, by="area"):
    """Drop components.  by: "area", "faces" or "volume" (|volume|).  A shape's components are ranked by that measure, descending,
    equal measures by ascending id; a component is kept if its rank is below `top` (when top is not None) and its measure is at least
    min_share times the shape's largest (in f64).  The kept vertices and faces keep the input order, faces are re-indexed, vertices that
    no face names are dropped; a shape whose components are all kept and that has no such vertex comes back bit for bit.
    -> verts, faces (device), voff, toff (host), status (B) int32 (device), kept (C_total) bool (device), coff (B+1) host."""
    top, share, by = _selection(top, min_share, by)
    verts, faces, vo, to = mesh_args(verts, faces, voff, toff, "keep_components_dev", **_MESH)
    on_device("keep_components_dev", verts, faces)
    o = _keep(verts, faces, vo, to, top, share, by)
    return o["verts"], o["faces"], o["voff"], o["toff"], o["status"], o["kept"], o["coff"]


def filter_components_dev(verts, faces, voff, toff, spec):
    """keep_components_dev with the option forms of `parse_keep`, plus what it removed: report[b] = {"count": components before
    filtering, "kept": components kept, "area_removed": share of the shape's area in the dropped components}.  The report costs one
    more small copy (the component table's areas and keep flags)."""
    kw = parse_keep(spec)
    if kw is None:
        raise L.SfmiError("filter_components_dev: keep_components is None (off)")
    top, share, by = _selection(kw.get("top"), kw.get("min_share", 0.0), kw.get("by", "area"))
    verts, faces, vo, to = mesh_args(verts, faces, voff, toff, "filter_components_dev", **_MESH)
    on_device("filter_components_dev", verts, faces)
    o = _keep(verts, faces, vo, to, top, share, by)
    area, kept, coff = o["area"].cpu().numpy(), o["kept"].cpu().numpy(), o["coff"]
    report = []
    for b in range(len(coff) - 1):
        a, k = area[coff[b]:coff[b + 1]], kept[coff[b]:coff[b + 1]]
        tot = float(a.sum())
        report.append({"count": int(len(a)), "kept": int(k.sum()), "area_removed": float(a[~k].sum() / tot) if tot > 0 else 0.0})
    return o["verts"], o["faces"], o["voff"], o["toff"], o["status"], report
