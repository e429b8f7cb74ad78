"""The forms in which a caller's tensors may reach the device entry points: the case table of test_input_forms_cpu.py / _gpu.py.

THE CONTRACT (cross-referenced from shapeformer_amd/_ragged.py).  Every public function of the 13 tool and op modules (scan,
registration, metrics, meshsdf, hpr, poisson, morph, components, simplify, iso_sparse, mcubes, tokens, ops) and the listed VQDIF
methods hand kernels the raw address of the caller's tensors.  For every such function and every tensor argument, each admissible form
of the SAME VALUES - a strided view, another dtype that holds the values exactly, offsets as a list / numpy array / tensor - must either

  give outputs that are bit-identical to the canonical call (contiguous tensors of the documented dtype), or
  be refused with SfmiError on the host, before the library is touched and before any output tensor changes.

A silently different result is never allowed.  A caller-provided output buffer of another dtype or layout is always refused: converting
it would lose the result.  The caller's tensors, the parts of a parent buffer that a view skips included, hold the same bytes after the
call as before it.  A tensor that must live on the device and does not is refused with SfmiError before the library is loaded.

THE TABLE.  CASES maps "module.function" (or "module.function#form" for a second set of arguments, "VQDIF.method" for the model) to a
Case: a builder of canonical keyword arguments at the smallest shape at which the function's kernels all run, and the role of each
tensor argument.  The variants of an argument come from its role, never from the function:

  FLOAT    f32 points / normals / vertices / features / lattices: `strided` (columns 0:3 of an (..,6) buffer, 0:33 of (..,40), else a
           [..., ::2] view of twice the last extent; the skipped entries are NaN), `f64` (a float64 copy: exact)
  INT      int32 tables (faces, idx, corr, triples, keys, token grids and rows): `strided` (the same, skipped entries 0: a valid value
           of every table here), `retyped` (int64 for int32, the high halves zero; for a table whose canonical form is int64, int32 as a
           [..., ::2] view of a zeroed buffer of the canonical byte size)
  BYTE     uint8 masks / voxels: `strided`, `bool`
  F64      f64 tensors that must be on the device (edge transforms, information matrices): `strided`, `f32` (the values are exact in
           f32; a [..., ::2] view of a buffer of the canonical byte size)
  HOST64   f64 poses / viewpoints / cameras / planes, host or device: numpy canonical; `cpu_tensor`, `dev_tensor`, `dev_strided`, `f32`
  HOSTINT  offsets and other integers the host reads: a list canonical; `np32`, `np64`, `cpu_tensor`, `dev_i32` (a [::2] view of a
           zeroed buffer, so that its bytes read as int64 are the same values), `dev_i64`
  OUT      caller-provided outputs: `strided` (a view of a buffer twice as large) and `retyped` (f64 / int64) - both refused
  every role that must live on the device also has `cpu` (that one argument as its CPU copy): refused

Every variant is "same" unless the Arg says "refuse" (the function chooses to refuse it) or "own" (a documented path that keeps the
dtype - hpr's f64 clouds, chamfer_distance's means in points1's dtype: equal to the function's own result from a contiguous f64 tensor).

What keeps a wrong wrapper harmless.  Every DEVICE tensor of a variant lies in a buffer of at least the canonical tensor's bytes, with
in-range values wherever a kernel that ignored the strides or the dtype would look, so such a wrapper computes a wrong answer from
addresses inside the tensors built here.  That argument does not cover a host pointer: every call that must be REFUSED (the `cpu`
variants above all) therefore runs with the library's loader replaced by one that fails the test, on the GPU as on the CPU, so a
wrapper that stopped refusing fails at `L.lib()` and launches nothing.  Host arrays (HOST64, HOSTINT as numpy or CPU tensors) reach a
kernel only through the function's own conversion; `hpr.resample_visible_dev` is why they are in the table.  HOST_ONLY names the
public functions that bind no tensor to a kernel.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

FLOAT, INT, BYTE, F64, HOST64, HOSTINT, OUT = "float", "int", "byte", "f64", "host64", "hostint", "out"
DEVICE_ROLES = (FLOAT, INT, BYTE, F64, OUT)

MODULES = ("scan", "registration", "metrics", "meshsdf", "hpr", "poisson", "morph", "components", "simplify", "iso_sparse", "mcubes",
           "tokens", "ops")
VQDIF_METHODS = ("quantize_cloud_dev", "quantize_cloud", "mode_of", "decode_index", "decode_index_grad", "refine_mesh_dev")

HOST_ONLY = {
    "scan.plane_hypotheses": "counter-hash draws on the host from set sizes; no tensor",
    "scan.normalize_scan": "plain numpy / torch array arithmetic on the array's own device; launches nothing",
    "scan.upright_rotation": "plain numpy / torch arithmetic on (B,3) normals; launches nothing",
    "registration.correspondence_hypotheses": "scan.plane_hypotheses under another name",
    "metrics.metrics_from_matrices": "small torch arithmetic on distance matrices; launches nothing",
    "meshsdf.signed_distance": "numpy in, numpy out: builds its own device tensors and calls signed_distance_dev",
    "meshsdf.mesh2sdf": "numpy in, numpy out: the lattice on the host, then signed_distance",
    "meshsdf.SDF_sampling": "numpy in, numpy out: builds its own device tensors and calls sdf_sampling_dev",
    "meshsdf.normalize_point_set": "numpy arithmetic on the host",
    "hpr.constraint_order_dev": "torch sort of Morton keys (performance only); binds nothing to a kernel",
    "hpr.hidden_point_removal": "numpy in, numpy out: builds its own device tensor and calls hidden_point_mask_dev",
    "hpr.sample_cameras": "numpy random directions on the host",
    "morph.index2point_dev": "torch.arange / meshgrid from an int; no tensor argument",
    "components.parse_keep": "parses an option on the host",
    "iso_sparse.lattice_levels": "integer arithmetic on the host",
    "iso_sparse.table_field": "returns a torch gather closure; extract_sparse_dev's entry feeds it every form of the table",
    "mcubes.array2mesh": "host or device array in, numpy out: moves the array itself, then marching_cubes_dev / keep_components_dev / decimate_dev",
    "ops.sdf_pack_weights": "packs numpy weights on the host",
    "ops.sdf_pack_weights_grad": "packs numpy weights on the host",
}


# parameters that share a name with a tensor role elsewhere but are not tensors here: function -> names
NOT_TENSORS = {}


class Arg:
    """the role of one tensor argument; expect: variant name -> "refuse" / "own" where it is not "same"; host_ok: a CPU tensor is
    admitted (moved by the function), so `cpu` is "same" """

    def __init__(self, role, host_ok=False, **expect):
        self.role, self.host_ok, self.expect = role, host_ok, expect


class Case:
    def __init__(self, build, roles, call=None, refuses_cpu=True):
        self.build, self.roles, self.call, self.refuses_cpu = build, roles, call, refuses_cpu


# ---- variants ---------------------------------------------------------------------------------------------------------------

def _strided(t, fill):
    """-> (a view with t's values and shape, its parent buffer: at least twice t's bytes, the skipped entries = fill)"""
    last = t.shape[-1] if t.dim() else 1
    if t.dim() >= 2 and last in (3, 33):
        parent = torch.full(t.shape[:-1] + ({3: 6, 33: 40}[last],), fill, dtype=t.dtype, device=t.device)
        view = parent[..., :last]
    else:
        t1 = t.reshape(1) if t.dim() == 0 else t
        parent = torch.full(t1.shape[:-1] + (2 * t1.shape[-1],), fill, dtype=t.dtype, device=t.device)
        view = parent[..., ::2]
        if t.dim() == 0:
            view = view[0]
    view.copy_(t)
    assert t.numel() == 0 or not view.is_contiguous()
    return view, parent


def _fill(t):
    return float("nan") if t.dtype.is_floating_point else 0


def variant_names(arg):
    names = {FLOAT: ["strided", "f64"], INT: ["strided", "retyped"], BYTE: ["strided", "bool"], F64: ["strided", "f32"],
             HOST64: ["cpu_tensor", "dev_tensor", "dev_strided", "f32"], HOSTINT: ["np32", "np64", "cpu_tensor", "dev_i32", "dev_i64"],
             OUT: ["strided", "retyped"]}[arg.role]
    if arg.role == FLOAT and arg.expect.get("f64") == "own":
        names = ["strided", "f64_strided"]             # the contiguous f64 tensor is what f64_strided is held against
    return names + (["cpu"] if arg.role in DEVICE_ROLES else [])


def expectation(arg, name):
    if name in arg.expect:
        return arg.expect[name]
    if name == "f64_strided":
        return "own"
    if arg.role == OUT:
        return "refuse"
    if name == "cpu":
        return "same" if arg.host_ok else "refuse"
    return "same"


def _one(role, name, v, dev):
    """one tensor / array in the named form -> (value, [parent buffers])"""
    if role in (HOST64, HOSTINT):
        a = np.asarray(v, np.float64 if role == HOST64 else np.int64)
        if name == "np32":
            return a.astype(np.int32), []
        if name == "np64":
            return a.astype(np.int64), []
        if name == "f32":
            assert np.array_equal(a.astype(np.float32).astype(np.float64), a)       # the builders keep these exact in f32
            return a.astype(np.float32), []
        t = torch.from_numpy(np.ascontiguousarray(a))
        if name == "cpu_tensor":
            return t, [t]
        t = t.to(dev, torch.int32 if name == "dev_i32" else t.dtype)
        if name == "dev_strided":
            return _strided(t, float("nan"))
        if name == "dev_i32":
            return _strided(t, 0)
        return t, [t]
    if name == "cpu":
        t = v.cpu()
        return t, [t]
    if name in ("strided", "f64_strided"):
        view, parent = _strided(v.double() if name == "f64_strided" else v, _fill(v))
        return view, [parent]
    if name == "retyped" and role == OUT:
        t = v.to(torch.float64 if v.dtype.is_floating_point else torch.int64)
    elif name == "retyped":
        t = v.to(torch.int64 if v.dtype == torch.int32 else torch.int32)
    else:
        t = v.to({"f64": torch.float64, "f32": torch.float32, "bool": torch.bool}[name])
        assert torch.equal(t.to(v.dtype), v)
    if t.element_size() < v.element_size():             # a narrower dtype: no fewer bytes than the canonical tensor behind the view
        view, parent = _strided(t, 0)
        assert parent.numel() * parent.element_size() >= v.numel() * v.element_size()
        return view, [parent]
    return t, [t]


def make_variant(arg, name, value, dev):
    """the argument's canonical value (a tensor, an array, or a list / tuple of them) in the named form -> (value, parent buffers)"""
    if isinstance(value, (list, tuple)) and value and all(isinstance(e, (np.ndarray, torch.Tensor)) for e in value):
        made = [_one(arg.role, name, v, dev) for v in value]
        return type(value)(m[0] for m in made), [p for m in made for p in m[1]]
    return _one(arg.role, name, value, dev)


def canonical_f64(value):
    """the contiguous f64 form that hpr's own f64 path is compared against"""
    return value.double().contiguous()


def flatten(out):
    """every tensor, array and number of a result, in a fixed order, as tensors (test_workspace_gpu._tensors, plus host values)"""
    if isinstance(out, torch.Tensor):
        return [out]
    if isinstance(out, np.ndarray):
        return [torch.from_numpy(np.ascontiguousarray(out))]
    if isinstance(out, (bool, int, float, np.integer, np.floating)):
        return [torch.tensor(float(out), dtype=torch.float64)]
    if isinstance(out, dict):
        out = [out[k] for k in sorted(out)]
    if isinstance(out, (tuple, list)):
        return [t for o in out for t in flatten(o)]
    return []


def raw_bytes(t):
    """the bytes of a contiguous buffer, as a CPU copy (NaN and bool compare by their bits)"""
    assert t.is_contiguous()
    t = t.reshape(-1)
    return (t.view(torch.uint8) if t.dtype != torch.bool else t.to(torch.uint8)).cpu().clone()


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(raw_bytes(a.contiguous()), raw_bytes(b.contiguous()))


# ---- canonical data (numpy, deterministic; every builder is device-agnostic) ----------------------------------------------------

def _t(a, dev, dt=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.to(dev) if dt is None else t.to(dev, dt)


@functools.lru_cache(None)
def _cloud(seed, n):
    return np.random.RandomState(seed).rand(n, 3).astype(np.float32) * 2 - 1


@functools.lru_cache(None)
def _sphere(seed, n, r=1.0):
    x = np.random.RandomState(seed).randn(n, 3)
    return (x / np.linalg.norm(x, axis=1, keepdims=True) * r).astype(np.float32)


CUBE_V = np.array([[x, y, z] for x in (-0.5, 0.5) for y in (-0.5, 0.5) for z in (-0.5, 0.5)], np.float32)
CUBE_F = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
                   [1, 5, 7], [1, 7, 3]], np.int32)
OFF2 = [0, 300, 500]
VIEW2 = np.array([[0.0, 0.0, 5.0], [5.0, 0.0, 0.0]])
Q = 8


def _two_sets():
    return np.concatenate([_sphere(1, 300), _sphere(2, 200, 0.75)])


def _rot(deg, axis, t):
    a = math.radians(deg)
    c, s = np.float32(math.cos(a)).astype(np.float64), np.float32(math.sin(a)).astype(np.float64)     # entries exact in f32
    R = {0: [[1, 0, 0], [0, c, -s], [0, s, c]], 1: [[c, 0, s], [0, 1, 0], [-s, 0, c]], 2: [[c, -s, 0], [s, c, 0], [0, 0, 1]]}[axis]
    P = np.eye(4)
    P[:3, :3], P[:3, 3] = np.array(R, np.float64), np.asarray(t, np.float64)
    return P


POSE2 = np.stack([_rot(5, 2, [0.0625, 0.0, -0.03125]), _rot(-4, 0, [0.0, 0.03125, 0.0625])])


def _moved(x, P):
    return (x.astype(np.float64) @ P[:3, :3].T + P[:3, 3]).astype(np.float32)


def _pair():
    """two (source, target) pairs: the targets are the sources under POSE2, rounded to f32"""
    s = _two_sets()
    t = np.concatenate([_moved(s[:300], POSE2[0]), _moved(s[300:], POSE2[1])])
    return s, t


def _mesh2(dev):
    return dict(verts=_t(np.concatenate([CUBE_V, CUBE_V * 1.5]), dev), faces=_t(np.concatenate([CUBE_F, CUBE_F]), dev, torch.int32),
                voff=[0, 8, 16], toff=[0, 12, 24])


MESH = dict(verts=Arg(FLOAT), faces=Arg(INT), voff=Arg(HOSTINT), toff=Arg(HOSTINT))


@functools.lru_cache(None)
def _occ():
    g = np.stack(np.meshgrid(*[np.linspace(-1, 1, Q)] * 3, indexing="ij"), -1)
    return np.stack([(np.linalg.norm(g, axis=-1) < 0.8), (np.abs(g).max(-1) < 0.6)]).astype(np.float32)


@functools.lru_cache(None)
def _knn_table(k):
    """a (500,k) int32 neighbour table of _two_sets, local to each set, the point itself included (numpy brute force)"""
    x, rows = _two_sets().astype(np.float64), []
    for lo, hi in zip(OFF2[:-1], OFF2[1:]):
        d = ((x[lo:hi, None] - x[None, lo:hi]) ** 2).sum(-1)
        rows.append(np.argsort(d, axis=1, kind="stable")[:, :k])
    return np.concatenate(rows).astype(np.int32)


def _pts(dev, **kw):
    return dict(points=_t(_two_sets(), dev), off=list(OFF2), **kw)


PTS = dict(points=Arg(FLOAT), off=Arg(HOSTINT))


def _flipped_normals():
    p = _two_sets()
    n = p / np.linalg.norm(p, axis=1, keepdims=True)
    return (n * np.where(np.random.RandomState(10).rand(500, 1) < 0.5, -1.0, 1.0)).astype(np.float32)


# ---- the cases --------------------------------------------------------------------------------------------------------------

CASES = {}


def case(name, roles, call=None, refuses_cpu=True):
    def deco(build):
        CASES[name] = Case(build, roles, call, refuses_cpu)
        return build
    return deco


# scan
@case("scan.knn_dev", dict(p=Arg(FLOAT), q=Arg(FLOAT), p_off=Arg(HOSTINT), q_off=Arg(HOSTINT)))
def _(dev):
    return dict(p=_t(_cloud(3, 100), dev), q=_t(_cloud(4, 40000), dev), k=16, p_off=[0, 100], q_off=[0, 40000])       # the split search


case("scan.knn_mean_dist_dev", PTS)(lambda dev: _pts(dev, k=8))
case("scan.statistical_outlier_mask_dev", PTS)(lambda dev: _pts(dev, k=8, std_ratio=1.0))
case("scan.radius_outlier_mask_dev", PTS)(lambda dev: _pts(dev, radius=0.25, min_neighbors=4))
case("scan.estimate_normals_dev", dict(PTS, viewpoint=Arg(HOST64)))(lambda dev: _pts(dev, k=8, viewpoint=VIEW2))
case("scan.estimate_normals_dev#tangent", PTS)(lambda dev: _pts(dev, k=8, orient="tangent"))


@case("scan.orient_normals_dev", dict(PTS, normals=Arg(FLOAT), idx=Arg(INT, retyped="refuse"), viewpoint=Arg(HOST64)))
def _(dev):
    return _pts(dev, normals=_t(_flipped_normals(), dev), idx=_t(_knn_table(8), dev), anchor="viewpoint", viewpoint=VIEW2, details=True)


case("scan.orient_normals_dev#knn", dict(PTS, normals=Arg(FLOAT)))(lambda dev: _pts(dev, normals=_t(_flipped_normals(), dev), k=8))


@case("scan.farthest_point_sample_dev", dict(PTS, valid=Arg(BYTE, bool="refuse")))
def _(dev):
    return _pts(dev, n=16, valid=_t((np.random.RandomState(11).rand(500) < 0.7).astype(np.uint8), dev))


case("scan.farthest_point_sample_dev#start", dict(PTS, start=Arg(HOSTINT)))(lambda dev: _pts(dev, n=16, start=[7, 5]))
case("scan.voxel_downsample_dev", PTS)(lambda dev: _pts(dev, voxel=0.25))


def _triples(sizes, H, seed):
    from shapeformer_amd.scan import plane_hypotheses
    return plane_hypotheses(sizes, H, seed)


case("scan.segment_plane_dev", dict(PTS, triples=Arg(INT), up=Arg(HOST64)))(
    lambda dev: _pts(dev, threshold=0.05, triples=_t(_triples([300, 200], 64, 1), dev), up=np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0]])))
case("scan.refit_plane_dev", dict(PTS, plane=Arg(HOST64), up=Arg(HOST64)))(
    lambda dev: _pts(dev, plane=np.array([[0.0, 0.0, 1.0, -0.5], [1.0, 0.0, 0.0, 0.25]]), threshold=0.1, up=np.array([0.0, 0.0, 1.0])))
case("scan.remove_planes_dev", dict(PTS, up=Arg(HOST64)))(
    lambda dev: _pts(dev, threshold=0.05, max_planes=2, min_ratio=0.05, hypotheses=64, up=np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0]])))
case("scan.euclidean_clusters_dev", PTS)(lambda dev: _pts(dev, radius=0.25, min_points=2, return_root=True))
case("scan.largest_cluster_mask_dev", PTS)(lambda dev: _pts(dev, radius=0.25))
case("scan.isolate_object_dev", dict(PTS, up=Arg(HOST64)))(
    lambda dev: _pts(dev, plane_threshold=0.05, cluster_radius=0.25, hypotheses=64, normalize="bbox", up=np.array([0.0, 0.0, 1.0])))
case("scan.clean_cloud_dev", dict(X=Arg(FLOAT)))(
    lambda dev: dict(X=_t(np.stack([_sphere(1, 300), _sphere(5, 300, 0.75)]), dev), k=8, out_N=64, resample="fps"))
case("scan.clean_cloud_dev#voxel", dict(X=Arg(FLOAT)))(
    lambda dev: dict(X=_t(np.stack([_sphere(1, 300), _sphere(5, 300, 0.75)]), dev), k=4, out_N=64, voxel=0.125))


# registration
def _reg(dev, **kw):
    s, t = _pair()
    return dict(source=_t(s, dev), target=_t(t, dev), s_off=list(OFF2), t_off=list(OFF2), **kw)


REG = dict(source=Arg(FLOAT), target=Arg(FLOAT), s_off=Arg(HOSTINT), t_off=Arg(HOSTINT))
START2 = np.stack([_rot(1, 2, [0.0, 0.0, 0.0]), _rot(1, 0, [0.0, 0.0, 0.0])])


def _target_normals():
    t = _pair()[1]
    c = np.concatenate([np.tile(t[:300].mean(0), (300, 1)), np.tile(t[300:].mean(0), (200, 1))])
    n = t - c
    return (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)


case("registration.transform_points_dev", dict(PTS, pose=Arg(HOST64)))(lambda dev: _pts(dev, pose=POSE2))
case("registration.evaluate_registration_dev", dict(REG, pose=Arg(HOST64)))(lambda dev: _reg(dev, max_dist=0.3, pose=START2))
case("registration.icp_step_dev", dict(REG, target_normals=Arg(FLOAT), pose=Arg(HOST64)))(
    lambda dev: _reg(dev, max_dist=0.3, metric="plane", target_normals=_t(_target_normals(), dev), pose=START2))
case("registration.icp_dev", dict(REG, target_normals=Arg(FLOAT), init=Arg(HOST64)))(
    lambda dev: _reg(dev, max_dist=0.3, metric=["plane", "point"], target_normals=_t(_target_normals(), dev), init=START2, max_iter=4))
case("registration.icp_multiscale_dev", dict(REG, init=Arg(HOST64)))(
    lambda dev: _reg(dev, voxels=(0.25, 0.125), metric="plane", init=START2, max_iter=3, normals_k=8))
case("registration.fpfh_dev", dict(PTS, normals=Arg(FLOAT)))(lambda dev: _pts(dev, normals=_t(_flipped_normals(), dev), k=8, radius=0.5))


@case("registration.fpfh_from_spfh_dev", dict(PTS, spfh=Arg(INT), m=Arg(INT)))
def _(dev):
    rs = np.random.RandomState(12)
    return _pts(dev, k=8, spfh=_t(rs.randint(0, 8, (500, 33)).astype(np.int32), dev), m=_t(rs.randint(1, 8, 500).astype(np.int32), dev))


@case("registration.match_features_dev", dict(fs=Arg(FLOAT), ft=Arg(FLOAT), s_off=Arg(HOSTINT), t_off=Arg(HOSTINT)))
def _(dev):
    rs = np.random.RandomState(13)
    f = rs.rand(500, 33).astype(np.float32)
    g = np.concatenate([f[:300][::-1], f[300:][::-1]]) + (rs.rand(500, 33) * 0.01).astype(np.float32)
    return dict(fs=_t(f, dev), ft=_t(g, dev), s_off=list(OFF2), t_off=list(OFF2))


def _corr():
    """50 true correspondences per pair (source i <-> target i: the targets are the moved sources)"""
    rs = np.random.RandomState(14)
    a, b = np.sort(rs.choice(300, 50, replace=False)), np.sort(rs.choice(200, 50, replace=False))
    return np.concatenate([np.stack([a, a], 1), np.stack([b, b], 1)]).astype(np.int32), [0, 50, 100]


def _greg(dev, **kw):
    corr, c_off = _corr()
    return _reg(dev, corr=_t(corr, dev), c_off=c_off, **kw)


GREG = dict(REG, corr=Arg(INT), c_off=Arg(HOSTINT))
case("registration.hypothesis_poses_dev", dict(GREG, triples=Arg(INT)))(
    lambda dev: _greg(dev, triples=_t(_triples([50, 50], 32, 2), dev), similarity=0.5))
case("registration.score_poses_dev", dict(GREG, poses=Arg(HOST64)))(
    lambda dev: _greg(dev, max_dist=0.1, poses=np.stack([POSE2, START2], 1)))
case("registration.ransac_correspondences_dev", dict(GREG, triples=Arg(INT)))(
    lambda dev: _greg(dev, max_dist=0.1, triples=_t(_triples([50, 50], 32, 2), dev), similarity=0.5, details=True))
case("registration.global_registration_dev", dict(REG, viewpoints=Arg(HOST64)))(
    lambda dev: _reg(dev, voxel=None, normals_k=8, feature_k=8, max_dist=0.2, hypotheses=64, viewpoints=(VIEW2, VIEW2[::-1].copy())))


def _scans(dev):
    x = _sphere(1, 300)
    return [_t(x, dev), _t(_moved(x[:250], POSE2[0]), dev), _t(_moved(x[50:], POSE2[1]), dev)]


case("registration.merge_scans_dev", dict(clouds=Arg(FLOAT)))(lambda dev: dict(clouds=_scans(dev), voxel=0.125, max_dist=0.3, max_iter=3))
case("registration.merge_scans_dev#offs", dict(clouds=Arg(FLOAT), offs=Arg(HOSTINT)))(
    lambda dev: dict(clouds=torch.cat(_scans(dev)), offs=[0, 300, 550, 800], max_dist=0.3, max_iter=3))
case("registration.merge_scans_dev#global_init", dict(clouds=Arg(FLOAT)))(          # global_init: a dict of numbers, no tensor of its own
    lambda dev: dict(clouds=_scans(dev), global_init=dict(max_dist=0.2, normals_k=8, feature_k=8, hypotheses=64), max_dist=0.3, max_iter=3))
case("registration.information_matrix_dev", dict(REG, pose=Arg(HOST64)))(lambda dev: _reg(dev, max_dist=0.3, pose=START2, details=True))


def _graph(dev, **kw):
    """one graph of three nodes and three edges (the last a loop closure); every pose entry is exact in f32"""
    X = np.stack([np.eye(4), _rot(5, 2, [0.25, 0.0, 0.0]), _rot(10, 2, [0.5, 0.0, 0.0])])
    T = np.stack([_rot(5, 2, [0.25, 0.0, 0.0]), _rot(5, 2, [0.25, 0.0, 0.0]), _rot(10, 2, [0.5, 0.0625, 0.0])])
    info = np.tile(np.diag([64.0, 64.0, 64.0, 128.0, 128.0, 128.0]), (3, 1, 1))
    return dict(nodes=X, src=[1, 2, 2], tgt=[0, 1, 0], transforms=_t(T, dev), infos=_t(info, dev), uncertain=[0, 0, 1], alive=[1, 1, 1],
                n_off=[0, 3], e_off=[0, 3], max_iter=5, **kw)


GRAPH = dict(nodes=Arg(HOST64, cpu_tensor="refuse"), src=Arg(HOSTINT), tgt=Arg(HOSTINT), transforms=Arg(F64), infos=Arg(F64),
             uncertain=Arg(HOSTINT, cpu_tensor="refuse"), alive=Arg(HOSTINT, cpu_tensor="refuse"), n_off=Arg(HOSTINT), e_off=Arg(HOSTINT))
case("registration.pose_graph_optimize_dev", GRAPH)(lambda dev: _graph(dev, mu=1.0, details=True))
case("registration.global_optimization_dev", GRAPH)(lambda dev: _graph(dev, max_dist=0.125))
case("registration.multiway_registration_dev", dict(clouds=Arg(FLOAT)))(
    lambda dev: dict(clouds=_scans(dev), max_dists=(0.3,), max_iter=3, graph_max_iter=5))
case("registration.multiway_registration_dev#offs", dict(clouds=Arg(FLOAT), offs=Arg(HOSTINT), pairs=Arg(HOSTINT)))(
    lambda dev: dict(clouds=torch.cat(_scans(dev)), offs=[0, 300, 550, 800], pairs=[[0, 1], [1, 2]], max_dists=(0.3,), max_iter=3,
                     graph_max_iter=5))


# metrics
def _sets(dev, k, n, seed=20):
    return [_t(_sphere(seed + i, n, 1.0 - 0.125 * i), dev) for i in range(k)]


AB = dict(a=Arg(FLOAT), b=Arg(FLOAT))
case("metrics.nn_dist", dict(p=Arg(FLOAT), q=Arg(FLOAT), p_off=Arg(HOSTINT), q_off=Arg(HOSTINT)))(
    lambda dev: dict(p=_t(_cloud(1, 100), dev), q=_t(_cloud(2, 40000), dev), p_off=[0, 100], q_off=[0, 40000], return_index=True))
case("metrics.chamfer", AB)(lambda dev: dict(a=_t(_sphere(1, 300), dev), b=_t(_sphere(2, 200, 0.75), dev)))
case("metrics.fscore", dict(pred=Arg(FLOAT), gt=Arg(FLOAT)))(
    lambda dev: dict(pred=_t(_sphere(1, 300), dev), gt=_t(_sphere(2, 200), dev), tau=0.125, return_pr=True))
case("metrics.uhd", dict(partial=Arg(FLOAT), completions=Arg(FLOAT)))(lambda dev: dict(partial=_t(_sphere(1, 300), dev), completions=_sets(dev, 2, 100)))
case("metrics.tmd_directions", dict(completions=Arg(FLOAT)))(lambda dev: dict(completions=torch.stack(_sets(dev, 3, 100))))
case("metrics.tmd", dict(completions=Arg(FLOAT)))(lambda dev: dict(completions=_sets(dev, 3, 100)))
case("metrics.evaluate", dict(Xct=Arg(FLOAT), completions=Arg(FLOAT), Xbd=Arg(FLOAT)))(
    lambda dev: dict(Xct=_t(_sphere(1, 300)[:100], dev), completions=_sets(dev, 2, 100), Xbd=_t(_sphere(1, 300), dev), tau=0.125, emd_n=64))


@case("metrics.emd_dev", AB)
def _(dev):
    res = 2048                                      # sfmi_emd_resident_max(): one resident pair, one that streams; the rounds are capped
    return dict(a=[_t(_cloud(11, 255), dev), _t(_cloud(12, res + 1), dev)], b=[_t(_cloud(13, 255), dev), _t(_cloud(14, res + 1), dev)],
                max_rounds=200, details=True)


case("metrics.emd_dev#pairs", dict(AB, a_off=Arg(HOSTINT), b_off=Arg(HOSTINT), pairs=Arg(HOSTINT)))(
    lambda dev: dict(a=_t(_cloud(15, 192), dev), b=_t(_cloud(16, 128), dev), a_off=[0, 64, 128, 192], b_off=[0, 64, 128],
                     pairs=[[0, 1], [2, 0], [1, 1]], eps_rel=0.01))
case("metrics.emd", AB)(lambda dev: dict(a=_t(_cloud(15, 64), dev), b=_t(_cloud(16, 64), dev), eps_rel=0.01))
case("metrics.pairwise_chamfer_dev", dict(X=Arg(FLOAT), Y=Arg(FLOAT)))(lambda dev: dict(X=_sets(dev, 3, 100), Y=_sets(dev, 2, 80, 30)))
case("metrics.pairwise_emd_dev", dict(X=Arg(FLOAT), Y=Arg(FLOAT)))(
    lambda dev: dict(X=torch.stack(_sets(dev, 3, 64)), Y=torch.stack(_sets(dev, 2, 64, 30)), eps_rel=0.01))
case("metrics.set_metrics", dict(gen=Arg(FLOAT), ref=Arg(FLOAT)))(
    lambda dev: dict(gen=torch.stack(_sets(dev, 3, 64)), ref=torch.stack(_sets(dev, 2, 64, 30)), metric="cd"))
case("metrics.sample_mesh_dev", MESH)(lambda dev: dict(_mesh2(dev), n=64, seed=3, return_face=True))
case("metrics.points_dist", dict(p1=Arg(FLOAT), p2=Arg(FLOAT)))(
    lambda dev: dict(p1=_t(_sphere(1, 300), dev), p2=_t(_sphere(2, 200), dev), return_ind=True))
case("metrics.points_dist#k", dict(p1=Arg(FLOAT), p2=Arg(FLOAT)))(
    lambda dev: dict(p1=_t(_sphere(1, 300), dev), p2=_t(_sphere(2, 200), dev), k=4, return_ind=True))
case("metrics.chamfer_dist", dict(p1=Arg(FLOAT), p2=Arg(FLOAT)))(lambda dev: dict(p1=_t(_sphere(1, 300), dev), p2=_t(_sphere(2, 200), dev)))
case("metrics.chamfer_distance", dict(points1=Arg(FLOAT, f64="own"), points2=Arg(FLOAT)))(      # the means take points1's dtype
    lambda dev: dict(points1=torch.stack(_sets(dev, 2, 100)), points2=torch.stack(_sets(dev, 2, 80, 30)), give_id=True))


# meshsdf
case("meshsdf.signed_distance_dev", dict(queries=Arg(FLOAT), verts=Arg(FLOAT), faces=Arg(INT), qoff=Arg(HOSTINT), voff=Arg(HOSTINT),
                                         toff=Arg(HOSTINT)))(
    lambda dev: dict(queries=_t(_cloud(5, 300), dev), verts=_t(CUBE_V, dev), faces=_t(CUBE_F, dev), qoff=[0, 300, 300], voff=[0, 8, 8],
                     toff=[0, 12, 12], return_winding=True))
case("meshsdf.mesh_occupancy_dev", MESH)(lambda dev: dict(_mesh2(dev), grid_dim=Q, return_status=True))
case("meshsdf.sdf_sampling_dev", MESH)(lambda dev: dict(_mesh2(dev), sample_N=64, seed=2))


# hpr: "f32 or f64" - the f64 forms are held against the function's own result from a contiguous f64 tensor
def _spheres2(dev):
    return _t(np.stack([_sphere(6, 300), _sphere(7, 300)]), dev)


CAMS = np.array([[0.0, 0.0, 10.0], [10.0, 0.0, 0.0]])
OWN = dict(f64="own")
case("hpr.hidden_point_mask_dev", dict(points=Arg(FLOAT, **OWN), cams=Arg(HOST64)))(lambda dev: dict(points=_spheres2(dev), cams=CAMS))
case("hpr.hidden_point_mask_dev#ragged", dict(points=Arg(FLOAT, **OWN), cams=Arg(HOST64), off=Arg(HOSTINT)))(
    lambda dev: dict(points=_t(_two_sets(), dev), cams=CAMS, off=list(OFF2)))
case("hpr.constraint_evaluations_dev", dict(points=Arg(FLOAT, **OWN), cams=Arg(HOST64)))(lambda dev: dict(points=_spheres2(dev), cams=CAMS))


@case("hpr.resample_visible_dev", dict(x=Arg(FLOAT, **OWN), o=Arg(HOSTINT), visible=Arg(BYTE), count=Arg(INT)))
def _(dev):
    vis = (np.random.RandomState(17).rand(500) < 0.5).astype(np.uint8)
    count = np.array([vis[:300].sum(), vis[300:].sum()], np.int32)
    return dict(x=_t(_two_sets(), dev), o=list(OFF2), visible=_t(vis, dev), count=_t(count, dev), context_N=32, noise=0.01, seed=3)


case("hpr.virtual_scan_dev", dict(X=Arg(FLOAT, **OWN), cams=Arg(HOST64)))(lambda dev: dict(X=_spheres2(dev), context_N=32, noise=0.01, cams=CAMS))
case("hpr.virtual_scan_dev#ragged", dict(X=Arg(FLOAT, **OWN), off=Arg(HOSTINT)))(
    lambda dev: dict(X=_t(_two_sets(), dev), context_N=32, off=list(OFF2), seed=5))
case("hpr.constraint_evaluations_dev#ragged", dict(points=Arg(FLOAT, **OWN), off=Arg(HOSTINT)))(
    lambda dev: dict(points=_t(_two_sets(), dev), cams=CAMS, off=list(OFF2), index_order=True))


# poisson
def _oriented(dev, **kw):
    p = _two_sets()
    return dict(points=_t(p * np.float32(0.75), dev), normals=_t(p / np.linalg.norm(p, axis=1, keepdims=True), dev), off=list(OFF2), **kw)


ORIENTED = dict(PTS, normals=Arg(FLOAT))
R = 9


def _lat(seed, *shape):
    return np.random.RandomState(seed).randn(*shape).astype(np.float32)


case("poisson.poisson_splat_dev", ORIENTED)(lambda dev: _oriented(dev, grid_dim=R))
case("poisson.poisson_rhs_dev", dict(Vx=Arg(FLOAT), Vy=Arg(FLOAT), Vz=Arg(FLOAT)))(
    lambda dev: dict(Vx=_t(_lat(1, 2, R - 1, R, R), dev), Vy=_t(_lat(2, 2, R, R - 1, R), dev), Vz=_t(_lat(3, 2, R, R, R - 1), dev)))
case("poisson.poisson_solve_dev", dict(rhs=Arg(FLOAT)))(lambda dev: dict(rhs=_t(_lat(15, 2, 8, 8, 8), dev), tol=1e-4))
case("poisson.poisson_sample_dev", dict(lattice=Arg(FLOAT), points=Arg(FLOAT), off=Arg(HOSTINT)))(
    lambda dev: dict(lattice=_t(_lat(4, 2, R, R, R), dev), points=_t(_two_sets(), dev), off=list(OFF2)))
case("poisson.poisson_field_dev", ORIENTED)(lambda dev: _oriented(dev, grid_dim=R, max_iter=8))
case("poisson.poisson_recon_dev", ORIENTED)(lambda dev: _oriented(dev, grid_dim=R, max_iter=8, quantile=0.125, keep_components="largest"))
case("poisson.poisson_recon_dev#estimated", dict(PTS, viewpoint=Arg(HOST64)))(
    lambda dev: dict(points=_t(_two_sets() * np.float32(0.75), dev), off=list(OFF2), grid_dim=R, max_iter=8, knn=8, viewpoint=VIEW2))


# morph
def _vox(dev):
    return _t(_occ().astype(np.uint8), dev)


VOX = dict(vox=Arg(BYTE))
case("morph.point2voxel_dev", PTS)(lambda dev: _pts(dev, grid_dim=Q))
case("morph.voxel_lookup_dev", dict(PTS, vox=Arg(BYTE)))(lambda dev: _pts(dev, vox=_vox(dev)))
case("morph.ball_dilate_dev", VOX)(lambda dev: dict(vox=_vox(dev), r=1))
case("morph.ball_erode_dev", VOX)(lambda dev: dict(vox=_vox(dev), r=1))
case("morph.flood_dev", VOX)(lambda dev: dict(vox=_vox(dev)))
case("morph.watertight_fill_dev", VOX)(lambda dev: dict(vox=_vox(dev), selem_size=1, return_status=True))
case("morph.morph_voxelization_dev", MESH)(
    lambda dev: dict(_mesh2(dev), sampleN=256, grid_dim=Q, selem_size=1, seed=1, return_status=True, return_samples=True))

# components, simplify, mcubes
case("components.mesh_components_dev", MESH)(lambda dev: _mesh2(dev))
case("components.keep_components_dev", MESH)(lambda dev: dict(_mesh2(dev), top=1))
case("components.filter_components_dev", MESH)(lambda dev: dict(_mesh2(dev), spec="largest"))
case("simplify.cluster_faces_dev", MESH)(lambda dev: dict(_mesh2(dev), grid=[2, 3]))
case("simplify.cluster_simplify_dev", MESH)(lambda dev: dict(_mesh2(dev), grid=[2, 3]))
case("simplify.decimate_dev", MESH)(lambda dev: dict(_mesh2(dev), decimate_face=8))
case("mcubes.marching_cubes_dev", dict(occ=Arg(FLOAT)))(lambda dev: dict(occ=_t(_occ(), dev), thresh=0.5))


# iso_sparse: the one tensor a caller brings is the table behind the field
def _extract(F, dev, return_levels=False):
    from shapeformer_amd import iso_sparse
    return iso_sparse.extract_sparse_dev(iso_sparse.table_field(F), F.shape[0], 3, 2, thresh=0.5, return_levels=return_levels, device=dev)


@case("iso_sparse.extract_sparse_dev", dict(F=Arg(FLOAT)), call=_extract)
def _(dev):
    g = np.stack(np.meshgrid(*[np.linspace(-1, 1, R)] * 3, indexing="ij"), -1)           # R = (3-1) 2^2 + 1
    F = np.stack([1.0 - np.linalg.norm(g, axis=-1), 0.9 - np.abs(g).max(-1)]).astype(np.float32)
    return dict(F=_t(F, dev), dev=dev, return_levels=True)


# tokens: 4^3 grids over a vocabulary of 17 (16 = the empty code); the end tokens lie outside both
END, VOCAB, LPAD = (64, 17), 17, 40


@functools.lru_cache(None)
def _grid4():
    rs = np.random.RandomState(18)
    q = np.full((2, 4, 4, 4), 16, np.int32)
    q.reshape(2, -1)[0, rs.choice(64, 20, replace=False)] = rs.randint(0, 16, 20)
    q.reshape(2, -1)[1, rs.choice(64, 30, replace=False)] = rs.randint(0, 16, 30)
    return q


@functools.lru_cache(None)
def _rows4():
    """the (2,LPAD,2) rows and lengths that dense2sparse makes of _grid4 (numpy)"""
    tok, ln = np.tile(np.array(END, np.int32), (2, LPAD, 1)), np.zeros(2, np.int32)
    for b in range(2):
        pos = np.nonzero(_grid4()[b].reshape(-1) != 16)[0]
        tok[b, :len(pos), 0], tok[b, :len(pos), 1], ln[b] = pos, _grid4()[b].reshape(-1)[pos], len(pos) + 1
    return tok, ln


CONTROL = dict(strided="refuse", retyped="refuse")              # small control tensors go to the kernel as they are
case("tokens.mode_i32", dict(idx=Arg(INT)))(lambda dev: dict(idx=_t(_grid4(), dev), vocab=VOCAB, rows=2))
case("tokens.dense2sparse_dev", dict(q=Arg(INT), mode=Arg(INT, **CONTROL), tokens=Arg(OUT), length=Arg(OUT)))(
    lambda dev: dict(q=_t(_grid4(), dev), mode=_t(np.array([16, 16], np.int32), dev), max_length=LPAD, end_tokens=END, Lpad=LPAD,
                     tokens=torch.zeros(2, LPAD, 2, dtype=torch.int32, device=dev), length=torch.zeros(2, dtype=torch.int32, device=dev)))
case("tokens.sparse2dense_dev", dict(tokens=Arg(INT), length=Arg(INT, **CONTROL), empty=Arg(INT, **CONTROL), start=Arg(INT, **CONTROL),
                                     out=Arg(OUT)))(
    lambda dev: dict(tokens=_t(_rows4()[0], dev), length=_t(_rows4()[1], dev), empty=_t(np.array([16, 3], np.int32), dev), dense_res=4,
                     end_tokens=END, out=torch.zeros(2, 4, 4, 4, dtype=torch.int32, device=dev), start=_t(np.array([0, 2], np.int32), dev)))
case("tokens.batch_dense2sparse", dict(indices=Arg(INT)))(
    lambda dev: dict(indices=_t(_grid4(), dev, torch.int64), max_length=LPAD, end_tokens=END, vocab=VOCAB))
case("tokens.batch_sparse2dense_padded", dict(sparse=Arg(INT)))(
    lambda dev: dict(sparse=_t(_rows4()[0], dev, torch.int64), empty_ind=16, dense_res=4, end_tokens=END))


# ops: every dtype but the kernel's own is refused
G = 4
OPF, OPI = dict(f64="refuse"), dict(retyped="refuse")


@functools.lru_cache(None)
def _packs():
    from shapeformer_amd import ops, weights as W
    sd = W.make_state_dict(W.vqdif_spec(16))
    return ops.sdf_pack_weights(sd), ops.sdf_pack_weights_grad(sd)


def _grid_cl(dev, B=2):
    return _t(np.random.RandomState(19).randn(B, G, G, G, 32).astype(np.float32), dev)


def _xyz(dev):
    return _t(np.stack([_cloud(21, 100), _cloud(22, 100)]) * np.float32(1.25), dev)


def _axis(n):
    return np.linspace(-1.0, 1.0, n).astype(np.float32)


case("ops.sdf_query", dict(xyz=Arg(FLOAT, **OPF), grid_cl=Arg(FLOAT, **OPF), wpack=Arg(FLOAT, **OPF), out=Arg(OUT)))(
    lambda dev: dict(xyz=_xyz(dev), grid_cl=_grid_cl(dev), wpack=_t(_packs()[0], dev), sigmoid=True, out=torch.zeros(2, 100, 1, device=dev)))
case("ops.sdf_query_keys", dict(axis=Arg(FLOAT, **OPF), keys=Arg(INT, **OPI), koff=Arg(INT, **OPI), grid_cl=Arg(FLOAT, **OPF),
                                wpack=Arg(FLOAT, **OPF)))(
    lambda dev: dict(axis=_t(_axis(R), dev), keys=_t(np.concatenate([np.arange(0, R ** 3, 7), np.arange(3, R ** 3, 11)]).astype(np.int32), dev),
                     koff=_t(np.array([0, len(range(0, R ** 3, 7)), len(range(0, R ** 3, 7)) + len(range(3, R ** 3, 11))], np.int32), dev),
                     grid_cl=_grid_cl(dev), wpack=_t(_packs()[0], dev)))
case("ops.sigmoid", dict(x=Arg(FLOAT, **OPF), out=Arg(OUT)))(
    lambda dev: dict(x=_t(_lat(23, 1000), dev), out=torch.zeros(1000, device=dev)))
case("ops.sdf_query_grid", dict(axis=Arg(FLOAT, **OPF), grid_cl=Arg(FLOAT, **OPF), wpack=Arg(FLOAT, **OPF), out=Arg(OUT),
                                affine=Arg(FLOAT, **OPF)))(
    lambda dev: dict(axis=_t(_axis(Q), dev), grid_cl=_grid_cl(dev), wpack=_t(_packs()[0], dev), out=torch.zeros(2, 4 * Q * Q, 1, device=dev),
                     x_range=(1, 5), affine=(_t(_lat(24, 2, 32), dev), _t(_lat(25, 2, 32), dev))))


def _grad(dev, **kw):
    return dict(xyz=_t(_two_sets(), dev), grid_cl=_grid_cl(dev), wpack_grad=_t(_packs()[1], dev), off=_t(np.array(OFF2, np.int32), dev), **kw)


GRAD = dict(xyz=Arg(FLOAT, **OPF), grid_cl=Arg(FLOAT, **OPF), wpack_grad=Arg(FLOAT, **OPF), off=Arg(INT, **OPI))
case("ops.sdf_query_grad", GRAD)(lambda dev: _grad(dev))
case("ops.sdf_query_grad#batch", dict(xyz=Arg(FLOAT, **OPF)))(
    lambda dev: dict(xyz=_xyz(dev), grid_cl=_grid_cl(dev), wpack_grad=_t(_packs()[1], dev)))
case("ops.sdf_refine_step", GRAD)(lambda dev: _grad(dev, level=0.0, max_step=0.0625))
case("ops.sdf_normals", GRAD)(lambda dev: _grad(dev))


# the VQDIF methods: the model moves host tensors to its device itself, so the CPU copy of an argument is one more admissible form
HOSTF, HOSTI = dict(host_ok=True), dict(host_ok=True)


def _model_cloud(dev):
    return _t(np.stack([_sphere(1, 300)[:256], _sphere(2, 300)[:256] * np.float32(0.75)]), dev)


def _codes(dev):
    return _t(np.random.RandomState(26).randint(0, 4096, (2, 16, 16, 16)).astype(np.int32), dev)


case("VQDIF.quantize_cloud_dev", dict(cloud=Arg(FLOAT, **HOSTF)), refuses_cpu=False)(lambda dev: dict(cloud=_model_cloud(dev), per_shape_mode=True))
case("VQDIF.quantize_cloud", dict(cloud=Arg(FLOAT, **HOSTF)), refuses_cpu=False)(lambda dev: dict(cloud=_model_cloud(dev)))
case("VQDIF.mode_of", dict(idx=Arg(INT)))(lambda dev: dict(idx=_codes(dev), name="mode_forms", rows=2))
case("VQDIF.decode_index", dict(code_ind=Arg(INT, **HOSTI), Xtg=Arg(FLOAT, **HOSTF)), refuses_cpu=False)(
    lambda dev: dict(code_ind=_codes(dev), Xtg=_xyz(dev)))
case("VQDIF.decode_index_grad", dict(code_ind=Arg(INT, **HOSTI), Xtg=Arg(FLOAT, **HOSTF)), refuses_cpu=False)(
    lambda dev: dict(code_ind=_codes(dev), Xtg=_xyz(dev)))
case("VQDIF.refine_mesh_dev", dict(grid_cl=Arg(FLOAT, **OPF), verts=Arg(FLOAT, **HOSTF), voff=Arg(HOSTINT)))(
    lambda dev: dict(grid_cl=_t(np.random.RandomState(27).randn(2, 8, 8, 8, 32).astype(np.float32), dev), verts=_t(_two_sets(), dev),
                     voff=list(OFF2), thresh=0.5, steps=2, max_step=0.0625))


# ---- resolving and calling ----------------------------------------------------------------------------------------------------

def base_name(key):
    return key.split("#")[0]


def resolve(key, model=None):
    """the callable behind a table key: a module's public function, or the model's bound method"""
    import importlib
    mod, fn = base_name(key).split(".")
    if mod == "VQDIF":
        return getattr(model, fn) if model is not None else None
    return getattr(importlib.import_module("shapeformer_amd." + mod), fn)


def invoke(key, kw, model=None):
    c = CASES[key]
    if c.call is not None:
        return c.call(**kw)
    return resolve(key, model)(**kw)


def tensor_args(key):
    """[(argument, Arg)] of a case, in the table's order"""
    return list(CASES[key].roles.items())


def gpu_params():
    """every (case, argument, variant) of the table"""
    return [(k, a, v) for k in CASES for a, arg in tensor_args(k) for v in variant_names(arg)]
