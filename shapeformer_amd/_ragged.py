"""Shared pieces of the mesh and scan tools, host side (the device side is csrc/sfmi_ragged.h).

Argument handling and small tensor idioms of metrics / meshsdf / hpr / iso_sparse / simplify / components / morph / make_dataset and of
scan / poisson / registration.

A ragged batch is B sets stored back to back with (B+1,) exclusive offsets: off[0] = 0, nondecreasing, off[B] = the row count; None
means one set.  Every check here runs on the host and raises SfmiError before the library is loaded, so a refused call launches
nothing.  Where the tensors live is NOT part of `mesh_args` / `point_sets`: a caller finishes its own host checks and then calls
`on_device`, last, so a CPU tensor reports the first wrong argument and not the device.

What a caller's tensor may look like is one contract for every public entry point (stated in tests/input_forms.py, held by
tests/test_input_forms_cpu.py / _gpu.py): a strided view, a float64 cloud, int64 faces or offsets in any integer form give the bits of
the canonical call - `mesh_args`, `.float().contiguous()` after `point_sets`, `i32_dev` are how - or are refused here on the host; a
caller's output buffer of another dtype or layout is always refused.  A new public function gets a row in that table.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L


# ---- argument handling (host only: everything here runs before any launch) -------------------------------------------------

def host_offsets(off, n, what, empty_ok=False, flatten=False):
    """-> (B+1,) int64 numpy exclusive offsets, validated against the n rows they cut.  None: one set.  empty_ok admits the
    one-element [0] (B = 0); flatten takes an array of any shape as its elements in order (components / simplify always did)."""
    if off is None:
        return np.array([0, n], np.int64)
    o = off.detach().cpu().numpy() if isinstance(off, torch.Tensor) else np.asarray(off)
    if flatten:
        o = o.reshape(-1)
    if o.ndim != 1 or o.shape[0] < (1 if empty_ok else 2) or not np.issubdtype(o.dtype, np.integer):
        raise L.SfmiError(f"{what}: offsets must be a 1-D integer array of length B+1")
    o = o.astype(np.int64)
    if o[0] != 0 or o[-1] != n or (np.diff(o) < 0).any():
        raise L.SfmiError(f"{what}: offsets must start at 0, be nondecreasing and end at {n}")
    return o


def check_count(v, what, name, lo=1):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) < 2 ** 31:
        raise L.SfmiError(f"{what}: {name} must be an integer in [{lo}, 2^31), got {v!r}")
    return int(v)


def check_number(v, what, name, lo, hi, lo_open=False, hi_open=False, allow_inf=False):
    """-> float(v) for an int or a float, not a bool and not NaN, between lo and hi (each end closed unless *_open).  hi = inf: no upper
    bound, and +inf itself passes only with allow_inf."""
    inf = float("inf")
    ok = not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating))
    if ok:
        x = float(v)
        ok = (x > lo if lo_open else x >= lo) and (x < hi if hi_open else x <= hi) and (allow_inf or x != inf)
    if not ok:
        want = (f"a {'' if allow_inf else 'finite '}number {'>' if lo_open else '>='} {lo:g}" if hi == inf else
                f"a number in {'(' if lo_open else '['}{lo:g}, {hi:g}{')' if hi_open else ']'}")
        raise L.SfmiError(f"{what}: {name} must be {want}, got {v!r}")
    return x


def check_nonneg(v, what, name):
    return check_number(v, what, name, 0, float("inf"))


def on_device(what, *tensors):
    """-> the one HIP device all the tensors are on.  Every caller's last check."""
    dev = tensors[0].device
    for t in tensors:
        if t.device.type != "cuda":
            raise L.SfmiError(f"{what} needs HIP device tensors (no CPU fallback)")
        if t.device != dev:
            raise L.SfmiError(f"{what}: all tensors must be on one device")
    return dev


def points_arg(x, what):
    if not isinstance(x, torch.Tensor):
        raise L.SfmiError(f"{what}: expected a torch tensor on the HIP device (no CPU fallback)")
    if x.shape[-1:] != (3,) or x.dim() not in (2, 3):
        raise L.SfmiError(f"{what}: expected (N,3) or (B,N,3) points, got {tuple(x.shape)}")
    return x


def point_sets(points, off, what):
    """(B,N,3) points (off must be None), or (N,3) points with offsets -> (points as (N,3), host offsets (B+1,), (B,N) or None)."""
    x = points_arg(points, what)
    if x.dim() == 3:
        if off is not None:
            raise L.SfmiError(f"{what}: offsets go with (N,3) points, not with (B,N,3)")
        B, n = x.shape[:2]
        return x.reshape(B * n, 3), np.arange(B + 1, dtype=np.int64) * n, (B, n)
    return x, host_offsets(off, x.shape[0], f"{what} offsets"), None


def pair_offsets(a_off, n, b_off, m, what, names=("source", "target")):
    """the offsets of two clouds of n and m rows that are cut into the same number of sets -> two host offset arrays of equal length.
    names: what the caller calls the two clouds; their initials name the offsets (s_off / t_off, p_off / q_off)"""
    ao, bo = host_offsets(a_off, n, f"{what} {names[0][0]}_off"), host_offsets(b_off, m, f"{what} {names[1][0]}_off")
    if len(ao) != len(bo):
        raise L.SfmiError(f"{what}: {names[0]} has {len(ao) - 1} sets, {names[1]} has {len(bo) - 1}")
    return ao, bo


def pair_sets(a, b, a_off, b_off, what, names=("source", "target"), max_sets=65535):
    """Set i of a against set i of b: (N,3) / (M,3) clouds with offsets (pair_offsets), or (B,N,3) / (B,M,3) batches of equal B with both
    offsets None -> (a as (N,3), b as (M,3), host offsets of a, of b, (B,N) or None).  max_sets: the launch bounds of the registration
    kernels, at most that many pairs (a grid's y limit) and every set below 2^31 points; None: neither bound."""
    a, b = points_arg(a, f"{what} {names[0]}"), points_arg(b, f"{what} {names[1]}")
    shape = None
    if a.dim() == 3 or b.dim() == 3:
        if a.dim() != b.dim() or a.shape[0] != b.shape[0] or a_off is not None or b_off is not None:
            raise L.SfmiError(f"{what}: a batched (B,N,3) {names[0]} needs a (B,M,3) {names[1]} of the same B and no offsets; "
                              f"an (N,3) {names[0]} needs an (M,3) {names[1]}")
        shape = tuple(a.shape[:2])
        ao, bo = (np.arange(shape[0] + 1, dtype=np.int64) * x.shape[1] for x in (a, b))
    else:
        ao, bo = pair_offsets(a_off, a.shape[0], b_off, b.shape[0], what, names)
    if max_sets is not None and (len(ao) - 1 > max_sets or (np.diff(ao) >= 2 ** 31).any() or (np.diff(bo) >= 2 ** 31).any()):
        raise L.SfmiError(f"{what}: at most {max_sets} pairs, every set below 2^31 points")
    return a.reshape(-1, 3), b.reshape(-1, 3), ao, bo, shape


def mesh_args(verts, faces, voff, toff, what, index32=False, empty_ok=False, flatten_offsets=False):
    """A ragged batch of indexed meshes -> (verts f32 contiguous, faces int32 contiguous, host voff, host toff) after the host checks:
    tensors, (V,3) / (T,3), integer faces, offsets (host_offsets), equal shape counts, and the size bound - with index32 the whole batch
    in 32-bit indices (components, simplify), else each shape's faces (meshsdf, morph).  A tensor that already has the dtype and
    layout comes back as it is."""
    if not isinstance(verts, torch.Tensor) or not isinstance(faces, torch.Tensor):
        raise L.SfmiError(f"{what}: verts / faces must be torch tensors on the HIP device (no CPU fallback)")
    if verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise L.SfmiError(f"{what}: expected verts (V,3) and faces (T,3), got {tuple(verts.shape)} and {tuple(faces.shape)}")
    if faces.dtype.is_floating_point or faces.dtype == torch.bool:
        raise L.SfmiError(f"{what}: faces must be an integer tensor")
    vo = host_offsets(voff, verts.shape[0], f"{what} voff", empty_ok, flatten_offsets)
    to = host_offsets(toff, faces.shape[0], f"{what} toff", empty_ok, flatten_offsets)
    if len(vo) != len(to):
        raise L.SfmiError(f"{what}: voff and toff describe different batch sizes ({len(vo) - 1} and {len(to) - 1} shapes)")
    if index32:
        if verts.shape[0] + faces.shape[0] + len(vo) >= 2 ** 31 or 3 * faces.shape[0] >= 2 ** 31:
            raise L.SfmiError(f"{what}: the batch is too large for 32-bit indices")
    elif (np.diff(to) >= 2 ** 31).any():
        raise L.SfmiError(f"{what}: a shape has 2^31 faces or more")
    return verts.float().contiguous(), faces.to(torch.int32).contiguous(), vo, to


# ---- host arrays -> device tensors -----------------------------------------------------------------------------------------

def offsets_dev(o, dev):
    """host offsets -> (B+1,) int64 on dev"""
    return torch.from_numpy(np.asarray(o, np.int64)).to(dev)


def i32_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(np.int32))).to(dev)


def f32_dev(x, dev=None):
    """a tensor as it is; anything else as a contiguous f32 array on dev (None: the current HIP device)"""
    if isinstance(x, torch.Tensor):
        return x
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32))).to(dev or torch.device("cuda"))


def workspace(nbytes, dev):
    """-> the uint8 buffer a `void* workspace` argument points at: what the tool's sfmi_*_workspace_bytes reported, at least 256 bytes
    (never an empty tensor, whose pointer is null).  Every tool allocates through here, called as `_ragged.workspace`, so a test can
    put guard bands around every workspace by replacing this one function."""
    return torch.empty(max(int(nbytes), 256), device=dev, dtype=torch.uint8)


def batch_meshes(meshes, dev):
    """[(verts (n_i,3), faces (t_i,3)) numpy, indices local] -> verts f32, faces int32 on dev, host voff, toff (B+1,)"""
    verts = torch.from_numpy(np.concatenate([v for v, _ in meshes]).astype(np.float32)).to(dev)
    faces = torch.from_numpy(np.concatenate([f for _, f in meshes]).astype(np.int32)).to(dev)
    voff = np.concatenate([[0], np.cumsum([len(v) for v, _ in meshes])]).astype(np.int64)
    toff = np.concatenate([[0], np.cumsum([len(f) for _, f in meshes])]).astype(np.int64)
    return verts, faces, voff, toff


# ---- prefix sums and sorted runs (any device) ------------------------------------------------------------------------------

def set_ids(o, dev):
    """host offsets (B+1,) -> (N,) int64 on dev: the set of every row"""
    return torch.repeat_interleave(torch.arange(len(o) - 1, device=dev), torch.from_numpy(np.diff(o)).to(dev), output_size=int(o[-1]))


def excl(x):
    """(n,) counts -> (n+1,) int32 exclusive prefix sums"""
    return torch.cat([x.new_zeros(1, dtype=torch.int32), torch.cumsum(x, 0, dtype=torch.int32)])


def excl_at(incl, off):
    """exclusive prefix at the (B+1) offsets `off` of an inclusive prefix sum (its total at off[B])"""
    return torch.cat([incl.new_zeros(1), incl])[off.long()]


def nonfinite_sets(x, od):
    """x (N,C) rows cut by the offsets od (B+1,) on x's device -> (B,) int32: 1 for a set with a row that is not finite"""
    z = excl_at(torch.cumsum((~torch.isfinite(x).all(1)).to(torch.int32), 0, dtype=torch.int32), od)
    return ((z[1:] - z[:-1]) > 0).to(torch.int32)


def runs(keys, n):
    """stable sort of the records by key -> (order int32, (n+1) int32 run starts: the records of key k are order[seg[k]:seg[k+1]];
    keys >= n sort behind every run)"""
    s = torch.sort(keys, stable=True)
    seg = torch.searchsorted(s.values, torch.arange(n + 1, device=keys.device, dtype=torch.int32))
    return s.indices.to(torch.int32), seg.to(torch.int32)


def sorted_runs(keys):
    """`runs` for sparse keys (any int64 values): stable sort of the n >= 1 records by key -> (order int64, is_start bool: sorted record
    i begins a run of equal keys, rank int64: the runs begun up to and including i).  Nothing is read back."""
    s = torch.sort(keys, stable=True)
    is_start = torch.ones_like(s.values, dtype=torch.bool)
    is_start[1:] = s.values[1:] != s.values[:-1]
    return s.indices, is_start, torch.cumsum(is_start, 0)


def run_starts(is_start, rank, m):
    """-> (m+1,) int64: where each of the m runs of `sorted_runs` begins, the record count at [m] (m read back by the caller)"""
    n = is_start.shape[0]
    starts = torch.empty(m + 2, device=rank.device, dtype=torch.int64)
    starts.scatter_(0, torch.where(is_start, rank - 1, m + 1), torch.arange(n, device=rank.device))   # the rest land in the spare slot
    starts[m] = n
    return starts[:m + 1]
