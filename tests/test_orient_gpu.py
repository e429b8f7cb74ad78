"""GPU tests of the consistent normal orientation (shapeformer_amd/scan.py orient_normals_dev, csrc/tangent.hip)
against tests/orient_ref.py.  Everything is compared with ==: the forest as a set of pairs, component, parity, votes, the output's bits.
The contract starts at (normal, idx): the device's own neighbour table and PCA normals are downloaded and handed to the reference.
Scenes are a few thousand points at most; the reference of the three scenes that several tests use is computed once."""

import os

import numpy as np
import pytest
import torch

import orient_ref as OR
from shapeformer_amd import make_dataset as MD
from shapeformer_amd import meshio, poisson, scan

pytestmark = pytest.mark.gpu


def _off(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _device_inputs(p, off, k, dev):
    """the device's self-kNN table (the point itself included) and its PCA normals without a viewpoint, downloaded"""
    x = _t(p, dev)
    o = None if off is None else off
    idx = scan.knn_dev(x, x, k, o, o, exclude_self=False)[1].cpu().numpy()
    nrm = scan.estimate_normals_dev(x, o, k)[0].cpu().numpy()
    return idx, nrm


def _run(p, nrm, dev, off=None, **kw):
    out, d = scan.orient_normals_dev(_t(p, dev), _t(nrm, dev), off, details=True, **kw)
    r = {name: v.cpu().numpy() for name, v in d.items()}
    r["normal"] = out.cpu().numpy()
    return r


def _tree_sets(tree, off):
    sets = []
    for b in range(len(off) - 1):
        rows = tree[int(off[b]):int(off[b + 1])]
        real = rows[rows[:, 0] >= 0]
        assert (rows[rows[:, 0] < 0] == -1).all() and (real[:, 0] < real[:, 1]).all()
        pairs = set(map(tuple, real.tolist()))
        assert len(pairs) == len(real)                                        # no edge twice
        sets.append(pairs)
    return sets


def _check(got, ref, nrm, off=None):
    """every output of the device equals the reference's; the output normal is the input or its negation, bit for bit"""
    off = np.array([0, len(nrm)], np.int64) if off is None else off
    assert np.array_equal(got["component"], ref["component"])
    assert np.array_equal(got["parity"], ref["parity"])
    assert np.array_equal(got["n_components"], ref["n_components"])
    trees = _tree_sets(got["tree"], off)
    assert trees == ref["tree"]
    for b, t in enumerate(trees):                                             # exactly n_b - components_b rows per set
        assert len(t) == int(off[b + 1] - off[b]) - int(ref["n_components"][b])
    assert np.array_equal(got["votes"], ref["votes"])
    assert np.array_equal(got["rounds"], ref["rounds"])                       # the same rounds did work
    assert np.array_equal(got["normal"].view(np.uint32), ref["normal"].view(np.uint32))
    bits, inb = got["normal"].view(np.uint32), np.ascontiguousarray(nrm).view(np.uint32)
    same, neg = (bits == inb).all(1), (bits == (inb ^ np.uint32(0x80000000))).all(1)
    assert (same | neg).all()


SCENES = {"torus": (lambda: OR.torus(2048, 0.5, 0.2, seed=3), 12),
          "box": (lambda: (OR.thin_box(2048, seed=7), None), 16),
          "spheres": (lambda: OR.two_spheres(1024, 512), 10)}


@pytest.fixture(scope="module")
def scenes(dev):
    """name -> (points, outward or None, k, device table, device normals, reference, device result)"""
    out = {}
    for name, (make, k) in SCENES.items():
        p, outward = make()
        idx, nrm = _device_inputs(p, None, k, dev)
        ref = OR.orient(p, nrm, idx, with_boruvka=True)
        out[name] = (p, outward, k, idx, nrm, ref, _run(p, nrm, dev, k=k))
    return out


# ---- 1. a closed surface with a hole through it

def test_torus(scenes):
    p, outward, k, idx, nrm, ref, got = scenes["torus"]
    _check(got, ref, nrm)
    assert ref["n_components"].tolist() == [1] and ref["margin"] >= 1e-9
    assert ((ref["normal"].astype(np.float64) * outward).sum(1) > 0).all()    # and so the device's: they are equal


# ---- 2. the tie-break case: thousands of edges of one weight

def test_thin_box_ties(scenes):
    p, _, k, idx, nrm, ref, got = scenes["box"]
    lo, hi, bits, _ = OR.graph_edges(nrm, idx)
    ties = int(np.bincount(np.unique(bits, return_inverse=True)[1]).max())
    print(f"thin box: {len(bits)} edges, {ties} of one weight, rounds {ref['rounds'].tolist()}")
    assert ties > 5000                                                        # PCA normals of a face are exact axes: w = 0 exactly
    assert ref["margin"] >= 1e-9
    _check(got, ref, nrm)


# ---- 3. all weights equal: (lo, hi) alone decides, one round, one long chain

def test_lattice_all_weights_equal(dev):
    p, nrm = OR.lattice(32, seed=11)
    idx = scan.knn_dev(_t(p, dev), _t(p, dev), 9)[1].cpu().numpy()
    ref = OR.orient(p, nrm, idx, with_boruvka=True)
    lo, hi, bits, _ = OR.graph_edges(nrm, idx)
    assert (bits == 0).all() and ref["n_components"].tolist() == [1]
    print(f"lattice: rounds {ref['rounds'].tolist()}, longest hook chain {ref['chain'].tolist()}")
    # the resolve walk's worst case: one round, every vertex hooks towards its lowest neighbour.  The 9 nearest of a lattice point lie at
    # most 2 rows and 2 columns away (at a corner), so a hook lowers the index by at most 66 and the walk from 1023 takes >= 16 steps
    assert ref["rounds"].tolist() == [1] and ref["chain"][0] >= 16
    got = _run(p, nrm, dev, k=9)
    _check(got, ref, nrm)
    assert (got["normal"][:, 2] == got["normal"][0, 2]).all()                 # parity undid every random sign
    assert (got["votes"] == 0).all()                                          # d lies in the plane: m . d = 0, nobody votes


# ---- 4. a hand-made chain through idx=

def test_chain_through_idx(dev):
    p, nrm, idx, sign = OR.chain(1000, seed=13)
    ref = OR.orient(p, nrm, idx, with_boruvka=True)
    assert ref["rounds"].tolist() == [1] and ref["chain"].tolist() == [999] and ref["margin"] >= 1e-9
    assert 400 < int((sign < 0).sum()) < 600
    got = _run(p, nrm, dev, idx=_t(idx, dev))
    _check(got, ref, nrm)
    assert np.array_equal(got["parity"], (sign != sign[0]).astype(np.uint8))
    assert ((got["normal"].astype(np.float64) * p).sum(1) > 0).all()          # outward on the circle


# ---- 5. two pieces in one set, each by its own vote against the set's centroid

def test_two_spheres(scenes):
    p, outward, k, idx, nrm, ref, got = scenes["spheres"]
    assert ref["n_components"].tolist() == [2] and ref["margin"] >= 1e-9
    comps = np.unique(ref["component"])
    assert comps.tolist() == [0, 1024]
    v = ref["votes"][comps]
    print(f"two spheres: votes {v.tolist()}")
    assert (v.min(1) > 0).all() and v[0].sum() == 1024 and v[1].sum() == 512  # neither vote is unanimous: the centroid lies outside
    assert ((ref["normal"].astype(np.float64) * outward).sum(1) > 0).all()
    _check(got, ref, nrm)


# ---- 6. the edges of the contract

def test_contract_edges(dev):
    rs = np.random.RandomState(17)
    sizes = [0, 1, 2, 3, 7, 0, 60]
    off = _off(sizes)
    N = int(off[-1])
    p = (rs.rand(N, 3) - 0.5).astype(np.float32)
    nrm = rs.randn(N, 3)
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    s = int(off[6])
    p[s + 20:s + 24] = p[s + 19]                                              # duplicate points
    nrm[s + 30:s + 33] = 0                                                    # dead vertices mid-set
    nrm[s + 40, 1] = np.nan
    nrm[s + 41, 0] = np.inf
    k = 10                                                                    # k > n - 1 in the small sets: rows end in -1
    idx = scan.knn_dev(_t(p, dev), _t(p, dev), k, off, off)[1].cpu().numpy()
    assert (idx[int(off[4]):int(off[5])] == -1).any()
    ref = OR.orient(p, nrm, idx, off, with_boruvka=True)
    assert ref["margin"] >= 1e-9
    dead = [s + 30, s + 31, s + 32, s + 40, s + 41]
    assert (ref["component"][dead] == np.array(dead) - s).all()               # a dead vertex is its own component
    got = _run(p, nrm, dev, off, k=k)
    _check(got, ref, nrm, off)
    assert np.array_equal(got["normal"][dead].view(np.uint32), nrm[dead].view(np.uint32))
    # a directed-only graph, entries outside the set, a repeated pair: row i names i + 1 and nothing names i back
    n = 9
    p2 = (rs.rand(n, 3) - 0.5).astype(np.float32)
    n2 = rs.randn(n, 3)
    n2 = (n2 / np.linalg.norm(n2, axis=1, keepdims=True)).astype(np.float32)
    idx2 = np.stack([np.arange(n) + 1, np.arange(n) + 1, np.full(n, n + 5), np.arange(n)], 1).astype(np.int32)
    idx2[5, :2] = -7                                                          # the chain is cut between 5 and 6
    ref2 = OR.orient(p2, n2, idx2, with_boruvka=True)
    assert ref2["n_components"].tolist() == [2] and ref2["tree"][0] == {(i, i + 1) for i in range(8) if i != 5}
    got2 = _run(p2, n2, dev, idx=_t(idx2, dev))
    _check(got2, ref2, n2)
    # the same table as a (B,M,k) batch of one
    got3 = scan.orient_normals_dev(_t(p2, dev)[None], _t(n2, dev)[None], idx=_t(idx2, dev)[None])
    assert got3.shape == (1, n, 3) and np.array_equal(got3[0].cpu().numpy().view(np.uint32), got2["normal"].view(np.uint32))


# ---- 7. a set's result is that set's alone; two runs give the same bytes

def test_batch_independence_and_repeatability(scenes, dev):
    names = ["torus", "box", "spheres"]
    k = 12
    singles = []
    for name in names:
        p, _, _, _, _, _, _ = scenes[name]
        idx, nrm = _device_inputs(p, None, k, dev)
        singles.append((p, nrm, _run(p, nrm, dev, k=k)))
    P = np.concatenate([s[0] for s in singles])
    Nn = np.concatenate([s[1] for s in singles])
    off = _off([len(s[0]) for s in singles])
    a = _run(P, Nn, dev, off, k=k)
    b = _run(P, Nn, dev, off, k=k)
    for name in ("normal", "component", "parity", "tree", "votes", "rounds", "n_components"):
        assert a[name].tobytes() == b[name].tobytes(), name
    for i, (_, _, one) in enumerate(singles):
        s = slice(int(off[i]), int(off[i + 1]))
        for name in ("normal", "component", "parity", "tree", "votes"):
            assert a[name][s].tobytes() == one[name].tobytes(), (names[i], name)
        assert a["rounds"][i] == one["rounds"][0] and a["n_components"][i] == one["n_components"][0]


# ---- 8. anchor="viewpoint"

def test_viewpoint_anchor(dev):
    view = np.array([0.0, 0.0, 2.0])
    p, outward = OR.hemisphere(4096, 0.5, view, seed=19)
    assert 1000 < len(p) < 2500
    k = 12
    idx, nrm = _device_inputs(p, None, k, dev)
    ref = OR.orient(p, nrm, idx, anchor="viewpoint", viewpoint=view[None], with_boruvka=True)
    assert ref["n_components"].tolist() == [1] and ref["margin"] >= 1e-9
    got = _run(p, nrm, dev, k=k, anchor="viewpoint", viewpoint=view)
    _check(got, ref, nrm)
    assert ((got["normal"].astype(np.float64) * (view[None] - p.astype(np.float64))).sum(1) > 0).all()
    assert ((got["normal"].astype(np.float64) * outward).sum(1) > 0).all()
    # estimate_normals_dev takes the viewpoint anchor when it has a viewpoint
    est = scan.estimate_normals_dev(_t(p, dev), None, k, viewpoint=view, orient="tangent")[0].cpu().numpy()
    assert np.array_equal(np.abs(est), np.abs(got["normal"])) and ((est.astype(np.float64) * outward).sum(1) > 0).all()


# ---- 9. the wiring: estimate_normals_dev, poisson_recon_dev, make_dataset

def test_wiring(dev, tmp_path):
    p, outward = OR.sphere(4096, 0.5, seed=23)
    x = _t(p, dev)
    n, var = scan.estimate_normals_dev(x, None, 10, orient="tangent")
    plain, var0 = scan.estimate_normals_dev(x, None, 10)
    assert torch.equal(var, var0) and torch.equal(n.abs(), plain.abs())
    idx = scan.knn_dev(x, x, 10)[1].cpu().numpy()
    ref = OR.orient(p, plain.cpu().numpy(), idx)
    assert ref["margin"] >= 1e-9 and ((ref["normal"].astype(np.float64) * outward).sum(1) > 0).all()   # every sign is right
    assert np.array_equal(n.cpu().numpy().view(np.uint32), ref["normal"].view(np.uint32))
    inward = scan.estimate_normals_dev(x, None, 10, viewpoint=(0.0, 0.0, 0.0))[0]   # a camera at the centre: the consistent inward field
    assert np.array_equal(n.cpu().numpy().view(np.uint32), (-inward).cpu().numpy().view(np.uint32))
    a = poisson.poisson_recon_dev(x, None, grid_dim=33, orient="tangent", knn=10)
    b = poisson.poisson_recon_dev(x, n, grid_dim=33)
    assert a[0].shape[0] > 100 and a[1].shape[0] > 100
    for u, v in zip(a, b):
        u, v = (u.cpu().numpy(), v.cpu().numpy()) if isinstance(u, torch.Tensor) else (np.asarray(u), np.asarray(v))
        assert u.tobytes() == v.tobytes()
    # make_dataset --occupancy poisson --orient tangent: a store from a .ply without normals
    path = str(tmp_path / "sphere.ply")
    meshio.write_ply(path, p, np.zeros((0, 3), np.int64))
    MD.main([path, "--out", str(tmp_path / "store"), "--dataset", "d", "--grid", "16", "--poisson-grid", "31", "--boundary-n", "64",
             "--occupancy", "poisson", "--orient", "tangent"])
    d = os.path.join(str(tmp_path / "store"), "d", "train")
    Xbd = np.load(os.path.join(d, "Xbd.npy"))
    occ = np.unpackbits(np.load(os.path.join(d, "Ytg.npy"))[0]).reshape(16, 16, 16)
    assert Xbd.shape == (1, 64, 3) and np.abs(np.linalg.norm(Xbd[0], axis=1) - 0.5).max() < 1e-6
    X = np.stack(np.meshgrid(*[np.linspace(-1, 1, 16)] * 3, indexing="ij"), -1)
    r = np.linalg.norm(X, axis=-1)
    wrong = (occ != 0) != (r < 0.5)                                            # inside the sphere, to within a node: outward normals
    assert (occ != 0).sum() > 10 and np.all(np.abs(r[wrong] - 0.5) < 2.0 / 15)
    with pytest.raises(ValueError, match="the cloud has no normals"):
        MD.make_dataset([path], str(tmp_path / "store2"), "d", grid=16, boundary_n=64, occupancy="poisson", poisson_grid=31)
