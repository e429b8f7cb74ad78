"""Multiway registration: the numpy reference - its Jacobians against central differences, its rotation vector against
scipy, its optimiser on synthetic graphs with and without false loop closures, the whole pipeline on the ring and chain scenes cut
from the armchair fixture - the host-side refusals of shapeformer_amd.registration, and the C entry points the header declares.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

import icp_ref as R
import posegraph_ref as P
from shapeformer_amd import _lib, registration as G
from shapeformer_amd._lib import SfmiError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_jacobians_against_central_differences():
    rs = np.random.RandomState(0)
    worst, thetas = 0.0, []
    for _ in range(40):
        xs, xt, T = (P.random_pose(rs, 57, 0.5) for _ in range(3))               # theta of the residual up to about 1 rad and beyond
        J, Js, Jt = P.jacobian(xs, xt, T), np.zeros((6, 6)), np.zeros((6, 6))
        for c in range(6):
            d = np.zeros(6)
            d[c] = 1e-6
            Js[:, c] = (P.residual(R.apply_step(xs, d), xt, T)[0] - P.residual(R.apply_step(xs, -d), xt, T)[0]) / 2e-6
            Jt[:, c] = (P.residual(xs, R.apply_step(xt, d), T)[0] - P.residual(xs, R.apply_step(xt, -d), T)[0]) / 2e-6
        thetas.append(P.residual(xs, xt, T)[1])
        worst = max(worst, np.abs(J - Js).max() / np.abs(Js).max(), np.abs(-J - Jt).max() / np.abs(Jt).max())
    assert min(thetas) < 0.3 and max(thetas) > 1.0
    assert worst < 1e-6                                                           # measured 3e-10: the differences' own truncation


def test_rotation_vector_against_scipy():
    from scipy.spatial.transform import Rotation
    rs = np.random.RandomState(0)
    for scale in (0.0, 1e-9, 5e-5, 0.99e-4, 1.01e-4, 1e-2, 1.0, 3.0):
        for _ in range(4):
            ax = rs.randn(3)
            w = ax / np.linalg.norm(ax) * scale
            M = R.rodrigues(w)
            got, th = P.rotvec(M)
            # vee(R - R^T) carries the few eps of R's entries; the factor theta / (2 sin theta) enlarges them near pi
            tol = 8 * np.finfo(np.float64).eps * max(1.0, scale / max(np.sin(scale), 1e-300) if scale else 1.0)
            assert abs(th - scale) <= tol and np.abs(got - w).max() <= tol
            assert np.abs(got - Rotation.from_matrix(M).as_rotvec()).max() <= tol + 4e-16
            Ji = P.jl_inv(w, scale)                                               # Jl^-1 inverts the left Jacobian of SO(3)
            if scale:
                K = P.skew(w)
                Jl = np.eye(3) + (1 - np.cos(scale)) / scale ** 2 * K + (scale - np.sin(scale)) / scale ** 3 * (K @ K)
                if scale > 1e-3:
                    assert np.abs(Ji @ Jl - np.eye(3)).max() < 1e-12


@pytest.mark.parametrize("S", [2, 3, 6, 12])
def test_reference_recovers_synthetic_graphs(S):
    g = P.synthetic(S, seed=S)
    o = P.optimize(g["X0"], g["src"], g["tgt"], g["T"], g["Lam"], g["unc"])
    eR, et = P.graph_error(o["X"], g["X_true"])
    assert o["status"] == 0 and 2 <= o["iterations"] <= 7
    assert eR <= 1e-9 and et <= 1e-9                           # 10 x tol; measured 1e-16 .. 5e-16
    again = P.optimize(o["X"], g["src"], g["tgt"], g["T"], g["Lam"], g["unc"])
    assert again["status"] == 0 and again["iterations"] == 1   # a fixed point ends at once, not in the lambda overflow


def test_reference_prunes_false_loop_closures():
    g = P.synthetic(8, seed=1, outliers=3)
    o = P.global_optimization(g["X0"], g["src"], g["tgt"], g["T"], g["Lam"], g["unc"], max_dist=0.01, prune=0.25)
    assert o["status1"] == 0 and o["status2"] == 0
    assert (o["l"][-3:] < 0.25).all() and (o["l"][:-3] > 0.9).all()
    assert not o["kept"][-3:].any() and o["kept"][:-3].all()
    eR, et = P.graph_error(o["X"], g["X_true"])
    assert eR <= 1e-9 and et <= 1e-9
    plain = P.optimize(g["X0"], g["src"], g["tgt"], g["T"], g["Lam"], g["unc"])
    assert P.graph_error(plain["X"], g["X_true"])[0] > 1e-3    # without the line process the false edges pull the graph away


def test_reference_statuses():
    g = P.synthetic(4, seed=3)
    run = lambda **kw: P.optimize(**{**dict(X=g["X0"], src=g["src"], tgt=g["tgt"], T=g["T"], Lam=g["Lam"], unc=g["unc"]), **kw})
    assert run(max_iter=0)["status"] == 1 and run(max_iter=0)["iterations"] == 0
    alive = np.ones(6, bool)
    alive[(g["src"] == 3) | (g["tgt"] == 3)] = False
    assert run(alive=alive)["status"] == 2 and np.array_equal(run(alive=alive)["X"], g["X0"])
    T = g["T"].copy()
    T[0, 3] = np.nan
    assert run(T=T)["status"] == 4
    assert run(src=np.array([1, 2, 4, 2, 3, 3]))["status"] == 4
    Lam = g["Lam"].copy()
    Lam[0] *= -1e3
    assert run(Lam=Lam)["status"] == 3
    T = g["T"].copy()
    T[1] = P.mul12(T[1], R.pose12(R.rodrigues(np.array([0, 0, 3.12])), np.zeros(3)))
    assert run(T=T, X=g["X_true"])["status"] == 3


@pytest.fixture(scope="module")
def ring():
    sc = P.ring_scene()
    return sc, P.multiway(sc["clouds"])


def test_ring_scene_needs_the_graph(ring):
    sc, m = ring
    assert m["edges"] == [(0, 1), (0, 5), (1, 2), (2, 3), (3, 4), (4, 5)]          # min_fitness = 0.1 keeps the six neighbouring pairs
    assert m["kept"].all() and m["status"].tolist() == [0] * 6 and (m["status1"], m["status2"]) == (0, 0)
    assert abs(m["l"][1] - 0.99998) < 1e-5 and (np.delete(m["l"], 1) == 1).all()   # the loop closure (0, 5) stays
    cR, ct = P.graph_error(m["chain"], sc["X_true"])
    oR, ot = P.graph_error(m["poses"], sc["X_true"])
    assert max(oR, ot) < max(cR, ct) and oR < cR and ot < ct                      # 3.3e-4 / 2.1e-4 -> 2.1e-4 / 1.1e-4
    merged, poses, st = R.merge(sc["clouds"], 0.05)                              # the star: scans 2, 3, 4 share nothing with scan 0
    for i in (2, 3, 4):
        Xt = sc["X_true"][i].reshape(3, 4)
        assert st[i] >= 2 or R.pose_error(poses[i], Xt[:, :3], Xt[:, 3])[0] > 1e-2
    graph = np.concatenate([R.transform(c, p) for c, p in zip(sc["clouds"], m["poses"])])
    assert R.chamfer(merged, sc["fixture"]) >= P.STAR_FACTOR * R.chamfer(graph, sc["fixture"])      # 4.0e-3 against 3.4e-8


def test_chain_scene_false_edges_are_pruned():
    """min_fitness = 0.01 admits the false edges (0,2) (fitness 0.025) and (1,3) (0.137) but not (2,4) (0.0088, 6 correspondences).  The
    reference prunes both: l = 0.145 and 0.0148 against prune = 0.25.  (At min_fitness = 0, (2,4) survives with l = 0.56.)"""
    sc = P.chain_scene()
    m = P.multiway(sc["clouds"], min_fitness=0.01)
    assert m["edges"] == [(0, 1), (0, 2), (1, 2), (1, 3), (2, 3), (3, 4)]
    assert m["kept"].tolist() == [True, False, True, False, True, True]
    assert abs(m["l"][1] - 0.145) < 1e-3 and abs(m["l"][3] - 0.01475) < 1e-4
    cR, ct = P.graph_error(m["chain"], sc["X_true"])           # the breadth-first start walks the false edge (0,2): 0.11 / 0.067
    oR, ot = P.graph_error(m["poses"], sc["X_true"])
    assert cR > 0.05 and oR < 1e-3 and ot < 1e-3               # 2.1e-4 / 1.2e-4: the chain's ICP accuracy


def test_host_side_refusals():
    eye = np.tile(np.eye(4), (3, 1, 1))
    T, Lam = torch.zeros(2, 4, 4, dtype=torch.float64), torch.zeros(2, 6, 6, dtype=torch.float64)   # CPU tensors: the device check is last
    ok = dict(nodes=eye, src=[1, 2], tgt=[0, 1], transforms=T, infos=Lam, uncertain=[0, 0])
    for f in (G.pose_graph_optimize_dev, lambda **kw: G.global_optimization_dev(max_dist=0.01, **kw)):
        with pytest.raises(SfmiError, match="32 nodes"):
            f(**{**ok, "nodes": np.tile(np.eye(4), (33, 1, 1))})
        for src in ([1, 3], [-1, 2], [1, 1]):
            with pytest.raises(SfmiError, match="inside their own graph"):
                f(**{**ok, "src": src})
        with pytest.raises(SfmiError, match="inside their own graph"):           # node 2 exists, but not in the edge's own graph
            f(**{**ok, "src": [1, 2], "tgt": [0, 0], "n_off": [0, 2, 3], "e_off": [0, 2, 2]})
        for bad in (torch.zeros(2, 36, dtype=torch.float64), torch.zeros(3, 6, 6, dtype=torch.float64), np.zeros((2, 6))):
            with pytest.raises(SfmiError, match="infos"):
                f(**{**ok, "infos": bad})
        with pytest.raises(SfmiError, match="transforms"):
            f(**{**ok, "transforms": torch.zeros(3, 4, 4, dtype=torch.float64)})
        with pytest.raises(SfmiError, match="src"):
            f(**{**ok, "src": [1.0, 2.0]})
        with pytest.raises(SfmiError, match="uncertain"):
            f(**{**ok, "uncertain": [0, 0, 1]})
        with pytest.raises(SfmiError, match="offsets"):
            f(**{**ok, "n_off": [0, 2, 4]})
        with pytest.raises(SfmiError, match="max_iter"):
            f(**{**ok, "max_iter": -1})
        with pytest.raises(SfmiError, match="tol"):
            f(**{**ok, "tol": float("nan")})
        with pytest.raises(SfmiError, match="no CPU fallback"):
            f(**ok)
    with pytest.raises(SfmiError, match="mu"):
        G.pose_graph_optimize_dev(**ok, mu=[1.0, 2.0])
    for prune in (-0.1, 1.5, None, True):
        with pytest.raises(SfmiError, match="prune"):
            G.global_optimization_dev(**ok, max_dist=0.01, prune=prune)
    with pytest.raises(SfmiError, match="max_dist"):
        G.global_optimization_dev(**ok)
    p, q = torch.zeros(10, 3), torch.zeros(12, 3)
    for md in ((), [], None):
        with pytest.raises(SfmiError, match="max_dists"):
            G.multiway_registration_dev([p, q], max_dists=md)
    with pytest.raises(SfmiError, match="max_dists"):
        G.multiway_registration_dev([p, q], max_dists=(0.05, -0.01))
    with pytest.raises(SfmiError, match="prune"):
        G.multiway_registration_dev([p, q], prune=2)
    with pytest.raises(SfmiError, match="min_fitness"):
        G.multiway_registration_dev([p, q], min_fitness=-1)
    with pytest.raises(SfmiError, match="32 scans"):
        G.multiway_registration_dev(torch.zeros(33, 3), offs=np.arange(34))
    for pairs in ([(1, 0)], [(0, 2)], [(0, 1), (0, 1)], [3]):
        with pytest.raises(SfmiError, match="pairs"):
            G.multiway_registration_dev([p, q], pairs=pairs)
    with pytest.raises(SfmiError, match="metric"):
        G.multiway_registration_dev([p, q], metric="colour")
    with pytest.raises(SfmiError, match="unknown arguments"):
        G.multiway_registration_dev([p, q], voxels=(0.02,))
    with pytest.raises(SfmiError, match="global_init"):
        G.multiway_registration_dev([p, q], global_init="yes")
    for kw in (dict(multiway="yes"), dict(multiway={}, global_init={}), dict(multiway={}, max_dist=0.1), dict(multiway={}, init=np.eye(4)[None])):
        with pytest.raises(SfmiError, match="multiway"):
            G.merge_scans_dev([p, q], **kw)
    with pytest.raises(SfmiError, match="max_dist"):
        G.information_matrix_dev(p, q)
    for call in (lambda: G.multiway_registration_dev([p, q]), lambda: G.merge_scans_dev([p, q], multiway={}),
                 lambda: G.information_matrix_dev(p, q, max_dist=0.1)):
        with pytest.raises(SfmiError, match="no CPU fallback"):
            call()


def test_library_exports_every_pg_entry_of_the_header():
    names = sorted(set(re.findall(r"\b(sfmi_pg_\w+)\s*\(", open(os.path.join(ROOT, "include", "sfmi.h")).read())))
    assert names == ["sfmi_pg_chunk", "sfmi_pg_information_f32", "sfmi_pg_max_edges", "sfmi_pg_max_nodes", "sfmi_pg_optimize_f64"]
    lib = _lib.lib()
    for n in names:
        assert hasattr(lib, n), f"libsfmi.so does not export {n}"
        assert n in _lib.PROTOTYPES, f"_lib.PROTOTYPES does not bind {n}"
    assert sorted(n for n in _lib.PROTOTYPES if n.startswith("sfmi_pg_")) == names
    assert lib.sfmi_pg_chunk() == lib.sfmi_icp_chunk() and lib.sfmi_pg_max_nodes() == G.PG_MAX_NODES == P.MAX_NODES
    assert lib.sfmi_pg_max_edges() == G.PG_MAX_EDGES == P.MAX_EDGES == 32 * 31 // 2
