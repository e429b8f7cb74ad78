"""Coarse-to-fine sparse iso-surface extraction on the device — host side of csrc/iso_sparse.hip.

The reference meshes a dense lattice only (xgutils/geoutil.py:175-233 array2mesh over the Q^3 occupancy of shapeformer.py:382-391 /
vqdif.py:60-76).  Here the field is evaluated on a coarse lattice first and only around the cells the surface passes through at
each finer level, so a mesh at 257^3 or 513^3 costs what its surface costs.  The contract (lattice, hierarchy, mesh order) is in
include/sfmi.h; the result equals `marching_cubes_dev` on the dense Q^3 grid restricted to the cut cells that were reached, bit for
bit, and the whole dense mesh where every cut cell was reached.  There is no CPU fallback.  The ragged-batch idioms (prefix sums at
offsets) are _ragged.py's.

  extract_sparse_dev(field, B, coarse_Q, levels, ...) -> verts, faces, voff, toff [, info]
  table_field(F)                                      -> a field that gathers from a dense (B,Q,Q,Q) device tensor
  lattice_levels(res, coarse)                         -> L with res = (coarse-1) 2^L + 1, or SfmiError naming the nearest valid res
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L
from . import _ragged
from ._ragged import excl_at


def lattice_levels(res, coarse):
    """The L >= 1 with res == (coarse-1) * 2**L + 1; SfmiError (naming the nearest valid res) when there is none or res^3 >= 2^31."""
    res, coarse = int(res), int(coarse)
    if coarse < 2:
        raise L.SfmiError(f"sparse iso-surface: coarse = {coarse} must be >= 2")
    valid = [(coarse - 1) * 2 ** l + 1 for l in range(1, 31) if ((coarse - 1) * 2 ** l + 1) ** 3 < 2 ** 31]
    if res in valid:
        return valid.index(res) + 1
    if not valid:
        raise L.SfmiError(f"sparse iso-surface: coarse = {coarse} leaves no res = (coarse-1)*2^L+1 with res^3 < 2^31")
    near = min(valid, key=lambda v: (abs(v - res), v))
    raise L.SfmiError(f"sparse iso-surface: res = {res} is not (coarse-1)*2^L+1 for coarse = {coarse}, L >= 1 with res^3 < 2^31; "
                      f"nearest valid res = {near}")


def _check(coarse_Q, levels, margin):
    if margin not in (0, 1):
        raise L.SfmiError(f"sparse iso-surface: margin = {margin} must be 0 or 1")
    if int(levels) < 1:
        raise L.SfmiError(f"sparse iso-surface: levels = {levels} must be >= 1")
    Q = (int(coarse_Q) - 1) * 2 ** int(levels) + 1
    if lattice_levels(Q, coarse_Q) != int(levels):
        raise L.SfmiError("sparse iso-surface: inconsistent lattice")
    return Q


def table_field(F):
    """field(keys, koff) for a dense (B,Q,Q,Q) f32 device tensor: values F[b].flatten()[key] of every shape's keys."""
    if not isinstance(F, torch.Tensor) or F.dim() != 4 or F.device.type != "cuda":
        raise L.SfmiError("table_field: F must be a (B,Q,Q,Q) torch tensor on the HIP device (no CPU fallback)")
    F = F.contiguous().float()
    B, n3 = F.shape[0], F[0].numel()
    flat = F.reshape(-1)

    def field(keys, koff):
        j = torch.arange(keys.numel(), device=keys.device, dtype=torch.int32)
        shape = torch.bucketize(j, koff[1:B].contiguous(), right=True) if B > 1 else torch.zeros_like(j)
        return flat[shape.long() * n3 + keys.long()]
    return field


class _BitSet:
    """bits / rank halves of one bit set of the workspace (include/sfmi.h)."""

    def __init__(self, ws, k, quarter, B, W):
        self.bits = ws[2 * k * quarter:][:B * W * 4].view(torch.int32)
        self.rank = ws[(2 * k + 1) * quarter:][:B * W * 4].view(torch.int32)
        self.starts = torch.arange(1, B + 1, device=ws.device) * W - 1

    def scan(self, lib, lat):
        """rank table from the bits; -> (B+1) int32 device offsets of the shapes in the ascending key list"""
        L.check(lib.sfmi_iso_popc_i32(L.ptr(self.bits), L.ptr(self.rank), *lat, L.stream_ptr()), "sfmi_iso_popc_i32")
        self.rank.cumsum_(0)
        return torch.cat([self.rank.new_zeros(1), self.rank[self.starts]])

    def keys(self, lib, lat, n):
        k = torch.empty(max(n, 1), device=self.bits.device, dtype=torch.int32)
        L.check(lib.sfmi_iso_compact_i32(L.ptr(self.bits), L.ptr(self.rank), *lat, L.ptr(k), n, L.stream_ptr()), "sfmi_iso_compact_i32")
        return k[:n]


def extract_sparse_dev(field, B, coarse_Q, levels, thresh=0.5, margin=1, bbox=((-1.0,) * 3, (1.0,) * 3), return_levels=False, device="cuda"):
    """Mesh of the iso-surface `thresh` of `field` on the lattice of Q = (coarse_Q-1) 2^levels + 1 points per axis, coarse to fine.

    field(keys, koff) -> values: a device callable; keys int32 (n) shape-local fine lattice indices (i0 Q + i1) Q + i2, ascending per
    shape, koff (B+1) int32 device offsets; returns the (n) f32 field values (any trailing unit dimension is dropped).
    -> verts (V,3) f32, faces (T,3) int32 local per shape (device), voff, toff (B+1) host arrays - the format of marching_cubes_dev;
    return_levels=True adds a dict: S / M (per level: ascending cell keys and (B+1) host offsets) and points (levels+1, B) evaluated
    (a corner that the level before evaluated keeps its value).
    One host read-back per refinement for sizes, one for the output sizes."""
    Q = _check(coarse_Q, levels, margin)
    Q0, nl, B, margin = int(coarse_Q), int(levels), int(B), int(margin)
    if B <= 0:
        raise L.SfmiError("sparse iso-surface: B must be >= 1")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise L.SfmiError("extract_sparse_dev needs a HIP device (no CPU fallback)")
    lib = L.lib()
    nbytes = int(lib.sfmi_iso_sparse_workspace_bytes(B, Q))
    if nbytes == 0:
        raise L.SfmiError("sfmi_iso_sparse_workspace_bytes: invalid lattice")
    ws = _ragged.workspace(nbytes, dev)
    W = (Q ** 3 + 31) // 32
    lat = (B, Q0, nl, Q)
    pts, cel = _BitSet(ws, 0, nbytes // 4, B, W), _BitSet(ws, 1, nbytes // 4, B, W)
    st = L.stream_ptr
    iso = float(thresh)
    info = dict(S=[], M=[], points=[])

    L.check(lib.sfmi_iso_seed_i32(*lat, L.ptr(pts.bits), L.ptr(cel.bits), st()), "sfmi_iso_seed_i32")
    poff, coff = pts.scan(lib, lat), cel.scan(lib, lat)
    hp, hc = np.arange(B + 1, dtype=np.int64) * Q0 ** 3, np.arange(B + 1, dtype=np.int64) * (Q0 - 1) ** 3    # level 0 is known
    prev = None
    for l in range(nl + 1):
        nP, nC = int(hp[-1]), int(hc[-1])
        pkeys, cells = pts.keys(lib, lat, nP), cel.keys(lib, lat, nC)
        if prev is None:
            ekeys, eoff, he, sel = pkeys, poff, hp, None
            vals = torch.empty(max(nP, 1), device=dev)
        else:
            # the corners the level before already evaluated keep their values (dst: their slots here); the others, nE of them (known
            # on the host since the read-back), are selected in ascending order: no second read-back
            dst, old = prev
            vals, known = torch.empty(max(nP, 1), device=dev), torch.zeros(max(nP, 1), device=dev, dtype=torch.uint8)
            L.check(lib.sfmi_iso_carry_apply_f32(L.ptr(dst), L.ptr(old), dst.numel(), L.ptr(vals), L.ptr(known), nP, st()), "sfmi_iso_carry_apply_f32")
            he = hp - hh
            nE = int(he[-1])
            sel = torch.empty(max(nE, 1), device=dev, dtype=torch.int32)
            L.check(lib.sfmi_iso_select_i32(L.ptr(known), L.ptr(torch.cumsum(known[:nP] == 0, 0, dtype=torch.int32)), nP, L.ptr(sel), nE, st()),
                    "sfmi_iso_select_i32")
            sel = sel[:nE].long()
            ekeys, eoff = pkeys[sel], torch.from_numpy(he.astype(np.int32)).to(dev)
        if ekeys.numel():
            ev = field(ekeys, eoff).reshape(-1).float()
            if ev.numel() != ekeys.numel():
                raise L.SfmiError(f"sparse iso-surface: the field returned {ev.numel()} values for {ekeys.numel()} keys")
            if sel is None:
                vals[:nP] = ev
            else:
                vals[sel] = ev
        flag = torch.zeros(max(nC, 1), device=dev, dtype=torch.uint8)
        L.check(lib.sfmi_iso_classify_f32(L.ptr(cells), L.ptr(coff), nC, l, L.ptr(pts.bits), L.ptr(pts.rank), L.ptr(vals), nP, iso, *lat,
                                          L.ptr(flag), st()), "sfmi_iso_classify_f32")
        info["points"].append(np.diff(he))
        if return_levels:
            mincl = torch.cumsum(flag[:nC] != 0, 0, dtype=torch.int32)
            moff = excl_at(mincl, coff)
            info["S"].append((cells, hc.copy()))
        else:
            moff = coff.new_zeros(B + 1)
        if l < nl:
            L.check(lib.sfmi_iso_refine_i32(L.ptr(cells), L.ptr(coff), L.ptr(flag), nC, l, margin, *lat, L.ptr(pts.bits), L.ptr(cel.bits), st()),
                    "sfmi_iso_refine_i32")
            old_poff, poff, coff = poff, pts.scan(lib, lat), cel.scan(lib, lat)
            dst = torch.full((max(nP, 1),), -1, device=dev, dtype=torch.int32)
            L.check(lib.sfmi_iso_carry_i32(L.ptr(pkeys), L.ptr(old_poff), nP, L.ptr(pts.bits), L.ptr(pts.rank), *lat, L.ptr(dst), st()),
                    "sfmi_iso_carry_i32")
            hoff = excl_at(torch.cumsum(dst[:nP] >= 0, 0, dtype=torch.int32), old_poff)
            h = torch.cat([poff, coff, moff, hoff]).cpu().numpy().astype(np.int64).reshape(4, B + 1)       # the level's one read-back: sizes
            hp, hc, hm, hh = h
            prev = (dst[:nP], vals)
        else:
            emask = torch.empty(max(nP, 1), device=dev, dtype=torch.int32)
            ntri = torch.zeros(max(nC, 1), device=dev, dtype=torch.int32)
            L.check(lib.sfmi_iso_mc_count_i32(L.ptr(cells), L.ptr(coff), L.ptr(flag), nC, L.ptr(pts.bits), L.ptr(pts.rank), nP, *lat,
                                              L.ptr(emask), L.ptr(ntri), st()), "sfmi_iso_mc_count_i32")
            m = emask[:nP]
            vincl = torch.cumsum((m & 1) + ((m >> 1) & 1) + ((m >> 2) & 1), 0, dtype=torch.int32)
            tincl = torch.cumsum(ntri[:nC], 0, dtype=torch.int32)
            voff_d, toff_d = excl_at(vincl, poff).contiguous(), excl_at(tincl, coff)
            voff, toff, hm = torch.cat([voff_d, toff_d, moff]).cpu().numpy().astype(np.int64).reshape(3, B + 1)   # the output sizes
            verts = torch.empty(max(int(voff[-1]), 1), 3, device=dev, dtype=torch.float32)
            faces = torch.empty(max(int(toff[-1]), 1), 3, device=dev, dtype=torch.int32)
            lo, hi = bbox
            L.check(lib.sfmi_iso_mc_emit_f32(L.ptr(cells), L.ptr(coff), L.ptr(flag), nC, L.ptr(pkeys), L.ptr(poff), nP, L.ptr(pts.bits),
                                             L.ptr(pts.rank), L.ptr(vals), iso, L.ptr(emask), L.ptr(vincl), L.ptr(tincl), L.ptr(voff_d), *lat,
                                             float(lo[0]), float(lo[1]), float(lo[2]), float(hi[0]), float(hi[1]), float(hi[2]),
                                             L.ptr(verts), L.ptr(faces), st()), "sfmi_iso_mc_emit_f32")
        if return_levels:
            nM = int(hm[-1])        # known on the host since the read-back: the cut cells are selected without a second one
            sel = torch.empty(max(nM, 1), device=dev, dtype=torch.int32)
            L.check(lib.sfmi_iso_select_i32(L.ptr((flag[:nC] == 0).to(torch.uint8)), L.ptr(mincl), nC, L.ptr(sel), nM, st()), "sfmi_iso_select_i32")
            info["M"].append((cells[sel[:nM].long()], hm.copy()))
    out = (verts[:int(voff[-1])], faces[:int(toff[-1])], voff, toff)
    if return_levels:
        info["points"] = np.stack(info["points"])
        return out + (info,)
    return out
