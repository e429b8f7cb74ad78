"""GPU: nothing writes past its workspace.  Every tool whose layout is stated through csrc/sfmi_ragged.h's SfmiCarver
allocates its `void* workspace` through `_ragged.workspace`; here that one function is replaced by one that puts a band of a byte
pattern in front of and behind every buffer it hands out.  Each tool runs through its public Python function at the smallest shape at
which every section of its layout exists, the bands must still hold the pattern afterwards, and the results must equal, bit for bit,
those of the same call without the guard.  Only ordinary, valid calls."""
import numpy as np
import pytest
import torch

from shapeformer_amd import _lib as L
from shapeformer_amd import _ragged, hpr, mcubes, meshsdf, metrics, poisson, scan

pytestmark = pytest.mark.gpu

BAND, PAT = 4096, 0xA5


class _Guard:
    """the replacement of _ragged.workspace: nbytes + 2 BAND bytes of PAT, the middle handed out, every buffer remembered"""

    def __init__(self):
        self.handed = []                                     # (whole buffer, bytes handed out)

    def __call__(self, nbytes, dev):
        n = max(int(nbytes), 256)
        whole = torch.full((n + 2 * BAND,), PAT, device=dev, dtype=torch.uint8)
        ws = whole[BAND:BAND + n]
        assert ws.data_ptr() % 256 == 0                      # sections start on 256 bytes: so must the buffer
        self.handed.append((whole, n))
        return ws

    def check(self):
        torch.cuda.synchronize()
        assert self.handed, "the tool allocated no workspace through _ragged.workspace"
        for whole, n in self.handed:
            assert bool((whole[:BAND] == PAT).all()), f"a write in front of a {n}-byte workspace"
            assert bool((whole[BAND + n:] == PAT).all()), f"a write behind a {n}-byte workspace"


def _tensors(out):
    if isinstance(out, torch.Tensor):
        return [out]
    if isinstance(out, dict):
        out = [out[k] for k in sorted(out)]
    if isinstance(out, (tuple, list)):
        return [t for o in out for t in _tensors(o)]
    return []


def _same_bits(a, b):
    if a.dtype.is_floating_point:                            # NaN rows (a capped auction) compare by their bits
        a, b = (t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64) for t in (a, b))
    return a.shape == b.shape and torch.equal(a, b)


def _guarded(monkeypatch, call, n_ws=None):
    """call() with guard bands, then without: the bands are whole and the two results are the same bits"""
    plain = _tensors(call())
    guard = _Guard()
    with monkeypatch.context() as m:
        m.setattr(_ragged, "workspace", guard)
        got = _tensors(call())
        guard.check()
    assert n_ws is None or len(guard.handed) == n_ws
    assert len(got) == len(plain) > 0 and all(_same_bits(a, b) for a, b in zip(got, plain))
    return guard


def _t(a, dev, dt=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)


def _cloud(seed, n):
    return np.random.RandomState(seed).rand(n, 3).astype(np.float32) * 2 - 1


def _sphere(seed, n):
    x = np.random.RandomState(seed).randn(n, 3)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


CUBE_V = np.array([[x, y, z] for x in (-0.5, 0.5) for y in (-0.5, 0.5) for z in (-0.5, 0.5)], np.float32)
CUBE_F = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
                   [1, 5, 7], [1, 7, 3]], np.int32)


def test_nn_dist(dev, monkeypatch):
    N, M = 100, 40000
    assert L.lib().sfmi_nn_dist_workspace_bytes(1, N, M) > 256 + N * 8          # this shape takes partial lists: every section exists
    p, q = _t(_cloud(1, N), dev), _t(_cloud(2, M), dev)
    _guarded(monkeypatch, lambda: metrics.nn_dist(p, q, return_index=True), n_ws=1)


def test_knn(dev, monkeypatch):
    N, M, k = 100, 40000, 16
    assert L.lib().sfmi_knn_workspace_bytes(1, N, M, k) > 256 + N * k * 8
    p, q = _t(_cloud(3, N), dev), _t(_cloud(4, M), dev)
    _guarded(monkeypatch, lambda: scan.knn_dev(p, q, k), n_ws=1)


def test_mesh_sdf_and_occupancy(dev, monkeypatch):
    v, f, q = _t(CUBE_V, dev), _t(CUBE_F, dev, torch.int32), _t(_cloud(5, 300), dev)
    # two shapes, the second without vertices, faces or queries
    _guarded(monkeypatch, lambda: meshsdf.signed_distance_dev(q, v, f, [0, 300, 300], [0, 8, 8], [0, 12, 12], return_winding=True), n_ws=1)
    # no faces at all: the record section is clamped to one record
    e = _t(np.zeros((0, 3), np.float32), dev)
    _guarded(monkeypatch, lambda: meshsdf.signed_distance_dev(e, e, e.to(torch.int32), [0, 0, 0], [0, 0, 0], [0, 0, 0]), n_ws=1)
    v2, f2 = _t(np.concatenate([CUBE_V, CUBE_V * 1.5]), dev), _t(np.concatenate([CUBE_F, CUBE_F]), dev, torch.int32)
    _guarded(monkeypatch, lambda: meshsdf.mesh_occupancy_dev(v2, f2, [0, 8, 16], [0, 12, 24], grid_dim=8, return_status=True), n_ws=1)


def test_hpr(dev, monkeypatch):
    x = _t(np.stack([_sphere(6, 300), _sphere(7, 300)]), dev)
    cams = np.array([[0.0, 0.0, 10.0], [10.0, 0.0, 0.0]])
    _guarded(monkeypatch, lambda: hpr.hidden_point_mask_dev(x, cams), n_ws=1)


@pytest.mark.parametrize("anchor", ["outward", "viewpoint"])
def test_orient(dev, monkeypatch, anchor):
    """both uses of tangent's buffer: the forest, then (outward) the centroids at its start"""
    p = np.concatenate([_sphere(8, 300), _sphere(9, 200)])
    rs = np.random.RandomState(10)
    n = p * np.where(rs.rand(500, 1) < 0.5, -1.0, 1.0).astype(np.float32)
    pt, nt = _t(p, dev), _t(n, dev)
    kw = dict(anchor="viewpoint", viewpoint=np.array([[0.0, 0.0, 5.0], [5.0, 0.0, 0.0]])) if anchor == "viewpoint" else {}
    _guarded(monkeypatch, lambda: scan.orient_normals_dev(pt, nt, [0, 300, 500], k=8, details=True, **kw), n_ws=2)   # knn's and tangent's


def test_emd(dev, monkeypatch):
    """one pair of the resident form and one just above it, which streams B from the workspace's last three sections; the rounds are
    capped, so the larger pair ends at its cap (status 1, emd NaN) after exactly the same rounds in both runs"""
    res = L.lib().sfmi_emd_resident_max()
    a = [_t(_cloud(11, 255), dev), _t(_cloud(12, res + 1), dev)]
    b = [_t(_cloud(13, 255), dev), _t(_cloud(14, res + 1), dev)]
    _guarded(monkeypatch, lambda: metrics.emd_dev(a, b, max_rounds=200, details=True), n_ws=1)


def test_mcubes(dev, monkeypatch):
    Q = 8
    g = np.stack(np.meshgrid(*[np.linspace(-1, 1, Q)] * 3, indexing="ij"), -1)
    occ = np.stack([(np.linalg.norm(g, axis=-1) < 0.8), (np.abs(g).max(-1) < 0.6)]).astype(np.float32)
    ot = _t(occ, dev)

    def call():
        v, f, voff, toff = mcubes.marching_cubes_dev(ot, 0.5)
        return v, f, torch.from_numpy(np.concatenate([voff, toff]))
    _guarded(monkeypatch, call, n_ws=1)


def test_poisson_solve(dev, monkeypatch):
    rhs = _t(np.random.RandomState(15).randn(2, 8, 8, 8).astype(np.float32), dev)
    _guarded(monkeypatch, lambda: poisson.poisson_solve_dev(rhs, tol=1e-4), n_ws=1)
