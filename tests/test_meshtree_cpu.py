"""Mesh tree, CPU side: the numpy statement of the tree (tests/meshtree_ref.py) on hand-checkable meshes, the tree code's approximation
error against the exact f64 winding number, the band condition the GPU occupancy test rests on, volumetric IoU on CPU tensors, and
meshtree's argument checks (they raise before the library is touched).

The exact winding numbers of the two fixtures on the 17^3 lattice are tests/golden/meshtree_wbrute_{sphere,bowl}.npy, written once by
meshtree_ref.brute_winding (4 913 x 9 216 solid angles in f64 take 13 s); a sample of them is recomputed here.

Measured with meshtree_ref's own traversal, 17^3 lattice of [-1, 1]^3.  The expansion is of the third order because the numbers ask
for it: the dipole alone errs by 1.601e-2 (sphere) / 1.289e-2 (bowl) at beta = 2, which puts 1.81 % of the bowl's lattice points inside
tau (the z = 0 plane lies 0.0371 under the rim, |W| - 0.5 >= 0.0232 there); the second order alone is worse (3.6e-2 / 2.1e-2).

    fixture  beta  max |W_tree - W|   tau = 4 x   share of lattice points with ||W| - 0.5| <= tau
    sphere   2     2.236e-3           8.94e-3     0
    sphere   3     3.189e-4           1.28e-3     0
    bowl     2     2.421e-3           9.68e-3     0
    bowl     3     2.581e-4           1.03e-3     0
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import meshtree_ref as M   # noqa: E402

FIXTURES = {"sphere": M.sphere, "bowl": M.bowl}
CLOSED = {"sphere": True, "bowl": False}
# the maximum error of W_ref(tree) against the exact winding number, as measured above and rounded up in the third digit
RECORDED = {("sphere", 2.0): 2.24e-3, ("sphere", 3.0): 3.19e-4, ("bowl", 2.0): 2.43e-3, ("bowl", 3.0): 2.59e-4}
_cache = {}


def _fixture(name):
    if name not in _cache:
        v, f = FIXTURES[name]()
        _cache[name] = (v, f, M.build(v, f), np.load(os.path.join(HERE, "golden", f"meshtree_wbrute_{name}.npy")))
    return _cache[name]


def _interleave(ux, uy, uz):
    k = 0
    for b in range(10):
        k |= ((ux >> b) & 1) << (3 * b + 2) | ((uy >> b) & 1) << (3 * b + 1) | ((uz >> b) & 1) << (3 * b)
    return k


@pytest.mark.parametrize("T", [1, 63, 64, 65, 512, 513, 4100])
def test_keys_order_and_topology_on_a_strip(T):
    v, f = M.strip_mesh(T)
    # face t of the strip has its centroid at x = (t + 1) / 2 of [0, (T + 1) / 2] and y = 1/3 (even t) or 2/3; z is flat
    want = [_interleave(min(1024 * (t + 1) // (T + 1), 1023), 341 if t % 2 == 0 else 682, 0) for t in range(T)]
    keys = M.morton_keys(v, f)
    assert keys.tolist() == want
    order = M.face_order(v, f)
    assert order.tolist() == sorted(range(T), key=lambda t: (want[t], t))
    levels = M.level_nodes(T)
    assert levels == {1: [1], 63: [1], 64: [1], 65: [2, 1], 512: [8, 1], 513: [9, 2, 1], 4100: [65, 9, 2, 1]}[T]
    L0 = levels[0]
    for l, n in enumerate(levels):
        r = [M.leaf_range(l, j, L0) for j in range(n)]
        assert r[0][0] == 0 and r[-1][1] == L0 and all(a[1] == b[0] for a, b in zip(r, r[1:])) and all(a < b for a, b in r)
        if l:                                                            # a node covers exactly its (at most 8) children
            for j in range(n):
                kids = [M.leaf_range(l - 1, c, L0) for c in range(8 * j, min(8 * j + 8, levels[l - 1]))]
                assert (kids[0][0], kids[-1][1]) == r[j] and 1 <= len(kids) <= 8
    tr = M.build(v, f)
    P = tr["P"].astype(np.float64)
    for l, n in enumerate(levels):
        for j in range(n):
            a0, a1 = M.leaf_range(l, j, L0)
            pts = P[a0 * 64:min(a1 * 64, T)].reshape(-1, 3)
            k = M.level_base(levels, l) + j
            d = np.sqrt(((pts - tr["p"][k].astype(np.float64)) ** 2).sum(1)).max()
            assert float(tr["r"][k]) >= d and float(tr["r"][k]) <= d * (1 + 3e-7) + 1e-30          # bounds its vertices, within 2 ulp
            assert (pts >= tr["lo"][k]).all() and (pts <= tr["hi"][k]).all()
    # the root's sums are the mesh's: its area, and one orientation
    area = 0.5 * np.linalg.norm(np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]), axis=1).sum()
    assert abs(tr["mom"][-1, 0] - area) <= 1e-12 * area and tr["mom"][-1, 6] * np.sign(tr["mom"][0, 6]) > 0
    assert abs(abs(tr["mom"][-1, 6]) - area) <= 1e-12 * area                                        # a flat strip: |dipole| = area


def test_golden_winding_is_the_brute_force():
    rs = np.random.RandomState(0)
    q = M.lattice(17)
    for name in FIXTURES:
        v, f, _, Wb = _fixture(name)
        k = rs.choice(len(q), 64, replace=False)
        assert np.abs(M.brute_winding(q[k], v, f) - Wb[k]).max() < 1e-12


@pytest.mark.parametrize("name,beta", sorted(RECORDED))
def test_tree_code_error_is_the_recorded_one(name, beta):
    v, f, tr, Wb = _fixture(name)
    W = M.winding(M.lattice(17), tr["P"], tr["wt"], tr["levels"], tr["p"], tr["r"], tr["dip"], tr["coef"], beta)
    err = np.abs(W - Wb).max()
    print(f"{name} beta {beta}: max |W_tree - W| = {err:.3e} (recorded {RECORDED[name, beta]:.3e})")
    assert 0.9 * RECORDED[name, beta] <= err <= RECORDED[name, beta]
    assert np.array_equal(np.abs(W) > 0.5, np.abs(Wb) > 0.5)             # occupancy identical at all 4 913 points


@pytest.mark.parametrize("name,beta", sorted(RECORDED))
def test_band_condition(name, beta):
    """by the brute force alone: with tau = 4 x the recorded error, no lattice point of a closed fixture and at most 1 % of the bowl's
    has ||W| - 0.5| <= tau"""
    Wb = _fixture(name)[3]
    share = (np.abs(np.abs(Wb) - 0.5) <= 4 * RECORDED[name, beta]).mean()
    print(f"{name} beta {beta}: share in the band {share:.4f}")
    assert share == 0 if CLOSED[name] else share <= 0.01


def test_volumetric_iou_on_cpu_tensors():
    from shapeformer_amd import meshtree as MT
    from shapeformer_amd._lib import SfmiError
    rs = np.random.RandomState(1)
    a, b = rs.rand(4, 5, 6, 7).astype(np.float32), rs.rand(4, 5, 6, 7).astype(np.float32)
    a[3], b[3] = 0.0, 0.25                                               # an empty union
    a[2] = b[2]
    got = MT.volumetric_iou_dev(torch.from_numpy(a), torch.from_numpy(b))
    A, Bm = a.reshape(4, -1) >= 0.5, b.reshape(4, -1) >= 0.5             # vqdif/common.py:8-36
    with np.errstate(invalid="ignore"):
        want = (A & Bm).astype(np.float32).sum(-1) / (A | Bm).astype(np.float32).sum(-1)
    assert got.dtype == torch.float64 and got.shape == (4,)
    assert np.array_equal(got.numpy()[:3].astype(np.float32), want[:3]) and float(got[2]) == 1.0 and np.isnan(float(got[3])) and np.isnan(want[3])
    u8 = MT.volumetric_iou_dev(torch.from_numpy((a >= 0.5).astype(np.uint8)), torch.from_numpy((b >= 0.5).astype(np.uint8)))
    assert np.array_equal(u8.numpy()[:3], got.numpy()[:3])
    assert MT.volumetric_iou_dev(torch.from_numpy(a), torch.from_numpy(b), thresh=0.0).tolist() == [1.0] * 4
    with pytest.raises(SfmiError, match="one shape"):
        MT.volumetric_iou_dev(torch.zeros(2, 3), torch.zeros(2, 4))
    with pytest.raises(SfmiError, match="tensors"):
        MT.volumetric_iou_dev(a, b)


def test_refusals_come_before_the_library(monkeypatch):
    from shapeformer_amd import _lib as L
    from shapeformer_amd import meshsdf as MS
    from shapeformer_amd import meshtree as MT
    E = L.SfmiError

    def no_lib():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(L, "lib", no_lib)
    v, f, q = torch.zeros(8, 3), torch.zeros(4, 3, dtype=torch.int32), torch.zeros(10, 3)
    with pytest.raises(E, match="HIP device"):                           # a CPU tensor: every host check passes, the device is last
        MT.mesh_tree_dev(v, f)
    with pytest.raises(E, match="HIP device"):                           # strided and retyped inputs are admitted, then the device
        MT.mesh_tree_dev(torch.zeros(8, 6, dtype=torch.float64)[:, ::2], torch.zeros(4, 6, dtype=torch.int64)[:, ::2], [0, 8], np.array([0, 4], np.int32))
    with pytest.raises(E, match="integer"):
        MT.mesh_tree_dev(v, f.float())
    with pytest.raises(E, match=r"verts \(V,3\)"):
        MT.mesh_tree_dev(torch.zeros(8, 4), f)
    with pytest.raises(E, match="different batch sizes"):
        MT.mesh_tree_dev(v, f, [0, 4, 8], [0, 1, 2, 4])
    with pytest.raises(E, match="offsets"):
        MT.mesh_tree_dev(v, f, [0.0, 8.0], [0, 4])
    z = lambda n, dt=torch.float32: torch.zeros(n, 4, dtype=dt)
    tree = MT.MeshTree(rec=z(20), orig=torch.zeros(4, dtype=torch.int32), nodes=z(4), mom=torch.zeros(1, 8, dtype=torch.float64),
                       status=torch.zeros(1, dtype=torch.int32), voff=np.array([0, 8]), toff=np.array([0, 4]), noff=np.array([0, 1]),
                       toff_dev=None, noff_dev=None)
    with pytest.raises(E, match="queries"):
        MT.signed_distance_tree_dev(torch.zeros(10, 2), tree)
    with pytest.raises(E, match="MeshTree"):
        MT.signed_distance_tree_dev(q, (v, f))
    with pytest.raises(E, match="beta"):
        MT.signed_distance_tree_dev(q, tree, beta=-1.0)
    with pytest.raises(E, match="beta"):
        MT.signed_distance_tree_dev(q, tree, beta=float("nan"))
    with pytest.raises(E, match="a tree of 1 meshes"):                   # a MeshTree of another batch
        MT.signed_distance_tree_dev(q, tree, qoff=[0, 5, 10])
    with pytest.raises(E, match="end at 10"):
        MT.signed_distance_tree_dev(q, tree, qoff=[0, 9])
    with pytest.raises(E, match="HIP device"):
        MT.signed_distance_tree_dev(q.double()[::1], tree)
    empty = MT.MeshTree(**{**tree.__dict__, "toff": np.array([0, 4, 4]), "voff": np.array([0, 8, 8]), "noff": np.array([0, 1, 1])})
    with pytest.raises(E, match="no faces"):
        MT.signed_distance_tree_dev(q, empty, qoff=[0, 5, 10])
    with pytest.raises(E, match="no faces"):
        MT.mesh_occupancy_tree_dev(empty)
    with pytest.raises(E, match="grid_dim"):
        MT.mesh_occupancy_tree_dev(tree, grid_dim=0)
    with pytest.raises(E, match="bbox"):
        MT.mesh_occupancy_tree_dev(tree, bbox=((0, 0, 0), (1, 1, float("inf"))))
    with pytest.raises(E, match="too many blocks"):
        MT.mesh_occupancy_tree_dev(tree, grid_dim=8192)
    with pytest.raises(E, match="HIP device"):
        MT.mesh_occupancy_tree_dev(tree, grid_dim=8)
    with pytest.raises(E, match="method"):
        MT.mesh_iou_dev(v, f, None, None, v, f, None, None, method="exact")
    with pytest.raises(E, match="1 meshes against 2"):
        MT.mesh_iou_dev(v, f, None, None, v, f, [0, 4, 8], [0, 2, 4])
    with pytest.raises(E, match="HIP device"):
        MT.mesh_iou_dev(v, f, None, None, v, f, None, None)
    with pytest.raises(E, match="method"):
        MS.signed_distance(np.zeros((3, 3)), np.zeros((3, 3)), np.zeros((1, 3), int), method="bvh")
    with pytest.raises(E, match="method"):
        MS.mesh2sdf(np.zeros((3, 3)), np.zeros((1, 3), int), method="bvh")


def test_make_dataset_takes_winding_and_beta():
    from shapeformer_amd import make_dataset as MD
    a = MD.parse_args(["m.obj", "--out", "o", "--dataset", "d"])
    assert (a.winding, a.beta) == ("brute", 2.0)
    a = MD.parse_args(["m.obj", "--out", "o", "--dataset", "d", "--winding", "tree", "--beta", "3"])
    assert (a.winding, a.beta) == ("tree", 3.0)
    with pytest.raises(SystemExit):
        MD.parse_args(["m.obj", "--out", "o", "--dataset", "d", "--winding", "fast"])
    with pytest.raises(ValueError, match="winding"):
        MD.make_dataset(["m.obj"], "o", "d", winding="fast")
