"""Edge-collapse decimation on the device (csrc/collapse.hip) against the plain Python statement of its contract
(tests/collapse_ref.py).  The claim is bit equality - faces, positions, status and rounds - so nothing here has a tolerance but the
one sanity bound on the sphere's radius, which is twice what the reference itself gives."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import collapse_ref as R   # noqa: E402

pytestmark = pytest.mark.gpu

BATCH_TARGET = 80


def _batch(meshes, dev):
    from shapeformer_amd._ragged import batch_meshes
    return batch_meshes([(np.asarray(v, np.float32).reshape(-1, 3), np.asarray(f, np.int32).reshape(-1, 3)) for v, f in meshes], dev)


def _split(v, f, voff, toff):
    v, f = v.cpu().numpy(), f.cpu().numpy()
    return [(v[voff[b]:voff[b + 1]], f[toff[b]:toff[b + 1]]) for b in range(len(voff) - 1)]


def _run(meshes, target, dev, **kw):
    """collapse_dev on a batch -> [(verts, faces, status, rounds)] per shape, host"""
    from shapeformer_amd.collapse import collapse_dev
    v, f, voff, toff, status, rounds = collapse_dev(*_batch(meshes, dev), target, details=True, **kw)
    assert len(voff) == len(toff) == len(meshes) + 1 and v.shape[0] == voff[-1] and f.shape[0] == toff[-1]
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and status.dtype == torch.int32
    st = status.cpu().numpy()
    return [(ov, of, int(st[b]), int(rounds[b])) for b, (ov, of) in enumerate(_split(v, f, voff, toff))]


def _same(got, want, what=""):
    """bit equality of one shape's (verts, faces, status, rounds)"""
    assert got[2:] == tuple(want[2:]), f"{what}: status / rounds {got[2:]} != {tuple(want[2:])}"
    assert np.array_equal(got[1], want[1]), f"{what}: faces differ"
    assert got[0].shape == want[0].shape and got[0].tobytes() == np.ascontiguousarray(want[0]).tobytes(), f"{what}: positions differ"


def _topology(meshes, dev):
    from shapeformer_amd.collapse import mesh_topology_dev
    counts, status = mesh_topology_dev(*_batch(meshes, dev))
    return counts.cpu().numpy(), status.cpu().numpy()


@pytest.fixture(scope="module")
def mc_sphere(dev):
    """a marching-cubes sphere on a 17^3 lattice (made once, downloaded: the reference and the device see the same bits)"""
    from shapeformer_amd.mcubes import marching_cubes_dev
    g = np.linspace(-1.0, 1.0, 17, dtype=np.float32)
    x, y, z = np.meshgrid(g, g, g, indexing="ij")
    occ = (1.3 - np.sqrt((x - 0.03) ** 2 + (y + 0.02) ** 2 + (z - 0.01) ** 2)).astype(np.float32)     # radius 0.8 at level 0.5
    v, f, voff, toff = marching_cubes_dev(torch.from_numpy(occ)[None].to(dev), 0.5)
    v, f = v.cpu().numpy(), f.cpu().numpy()
    assert len(f) > 600
    return occ, v, f, R.collapse_ref(v, f, 300)


@pytest.fixture(scope="module")
def planted():
    """an icosphere with a fin: three faces on one edge"""
    v, f = R.icosphere(2)
    a, b = int(f[0, 0]), int(f[0, 1])
    v2 = np.concatenate([v, (1.5 * (v[a] + v[b]))[None]]).astype(np.float32)
    f2 = np.concatenate([f, [[a, b, len(v)]]]).astype(np.int32)
    return v2, f2, (a, b, len(v)), R.collapse_ref(v2, f2, 101)


@pytest.fixture(scope="module")
def cut_torus():
    v, f = R.torus_grid(16, 8, open_ring=True)
    return v, f, R.collapse_ref(v, f, 60)


@pytest.mark.parametrize("name", list(R.CASES))
def test_parity_with_the_reference(name, dev):
    v, f, target, want = R.case(name)
    got = _run([(v, f)], target, dev)[0]
    print(f"{name}: {len(f)} -> {len(got[1])} faces, status {got[2]}, rounds {got[3]}")
    _same(got, want, name)
    tin, tout = _topology([(v, f), got[:2]], dev)[0]
    assert tuple(tin) == R.topology_ref(v, f) and tuple(tout) == R.topology_ref(*want[:2])
    assert tout[5] == tin[5] and tuple(tout[3:5]) == tuple(tin[3:5]) and R.duplicate_faces(got[1]) == 0


def test_parity_on_a_marching_cubes_sphere(mc_sphere, dev):
    _, v, f, want = mc_sphere
    got = _run([(v, f)], 300, dev)[0]
    print(f"mc sphere: {len(f)} -> {len(got[1])} faces, status {got[2]}, rounds {got[3]}")
    _same(got, want, "mc sphere")
    assert want[2] == 0 and 299 <= len(got[1]) <= 300
    tin, tout = _topology([(v, f), got[:2]], dev)[0]
    assert tuple(tin) == R.topology_ref(v, f) and tuple(tout) == R.topology_ref(*want[:2]) and tout[5] == tin[5] == 2


def test_planted_non_manifold_edge_does_not_move(planted, dev):
    v, f, fin, want = planted
    got = _run([(v, f)], 101, dev)[0]
    _same(got, want, "planted")
    kept = {p.tobytes() for p in got[0]}
    assert all(v[i].tobytes() in kept for i in fin)
    tin, tout = _topology([(v, f), got[:2]], dev)[0]
    assert tin[4] == tout[4] == 1 and tin[3] == tout[3] == 2 and tuple(tout) == R.topology_ref(*want[:2])


def test_cut_torus_keeps_its_boundary(cut_torus, dev):
    v, f, want = cut_torus
    got = _run([(v, f)], 60, dev)[0]
    _same(got, want, "cut torus")
    before = {v[i].tobytes() for i in R.boundary_vertices(f)}
    assert len(before) == 16 and {got[0][i].tobytes() for i in R.boundary_vertices(got[1])} == before
    tin, tout = _topology([(v, f), got[:2]], dev)[0]
    assert tin[3] == tout[3] == 16 and tin[5] == tout[5] and tuple(tout) == R.topology_ref(*want[:2])


def _mixed(mc_sphere, planted, cut_torus):
    bad = R.icosphere(2)[1].copy()
    bad[7, 2] = 162                                                          # one index outside the shape: status 2
    nan = R.icosphere(2)[0].copy()
    nan[11, 0] = np.inf
    meshes = [R.case(n)[:2] for n in R.CASES]
    meshes += [(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)), R.icosphere(1), (R.icosphere(2)[0], bad),
               (nan, R.icosphere(2)[1]), mc_sphere[1:3], planted[:2], cut_torus[:2]]
    return meshes


def test_mixed_batch_equals_per_shape_calls_and_the_reference(mc_sphere, planted, cut_torus, dev):
    meshes = _mixed(mc_sphere, planted, cut_torus)
    got = _run(meshes, BATCH_TARGET, dev)
    again = _run(meshes, BATCH_TARGET, dev)
    other = _run(meshes, BATCH_TARGET, dev, rounds_per_sync=3)
    for b, (v, f) in enumerate(meshes):
        _same(got[b], _run([(v, f)], BATCH_TARGET, dev)[0], f"shape {b} alone")
        _same(again[b], got[b], f"shape {b}, second run")
        _same(other[b], got[b], f"shape {b}, three rounds per read-back")
        _same(got[b], R.collapse_ref(v, f, BATCH_TARGET), f"shape {b} against the reference")
    st = [g[2] for g in got]
    assert st[5:10] == [0, 1, 0, 2, 3] and [len(g[1]) for g in got[5:10]] == [4, 0, 80, 0, 0] and len(got[8][0]) == len(got[9][0]) == 0
    assert got[7][0].tobytes() == R.icosphere(1)[0].tobytes()               # at the budget: unchanged
    counts, status = _topology([g[:2] for g in got], dev)
    for b, g in enumerate(got):
        assert tuple(counts[b]) == (R.topology_ref(*g[:2]) if status[b] == 0 else (0,) * 6)
    assert list(status[[6, 8, 9]]) == [1, 1, 1]                             # what came back empty has no vertices


def test_topology_statuses(dev):
    v, f = R.icosphere(1)
    bad = f.copy()
    bad[0, 0] = -1
    nan = v.copy()
    nan[0, 0] = np.nan
    deg = np.concatenate([f, [[3, 3, 5]]]).astype(np.int32)                 # a repeated index: a face without edges
    counts, status = _topology([(v, f), (v, bad), (nan, f), (v[:0], f[:0]), (v, f[:0]), (v, deg)], dev)
    assert list(status) == [0, 2, 3, 1, 0, 0]
    assert tuple(counts[0]) == R.topology_ref(v, f) == (42, 120, 80, 0, 0, 2)
    assert not counts[1:4].any() and tuple(counts[4]) == (0,) * 6
    assert tuple(counts[5]) == R.topology_ref(v, deg) == (42, 120, 81, 0, 0, 3)


def test_wide_batch_equals_per_shape_calls(dev):
    """261 shapes, four kinds at three sizes, runs of empty shapes between them: more shapes than some of them have faces"""
    kinds = {}
    for name, (v, f) in (("tetra", R.tetrahedron()), ("octa", R.octahedron()), ("ico0", R.icosphere(0)), ("ico1", R.icosphere(1))):
        for s in (1.0, 0.37, 1.9):
            kinds[(name, s)] = ((v * np.float32(s)).astype(np.float32), f)
    kinds["empty"] = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    keys, order = list(kinds), []
    rng = np.random.default_rng(5)
    while len(order) < 261:
        if len(order) % 29 == 7:
            order += ["empty"] * 5
        order.append(keys[int(rng.integers(len(keys)))])
    order = order[:261]
    target = 6
    alone = {k: _run([kinds[k]], target, dev)[0] for k in keys}
    got = _run([kinds[k] for k in order], target, dev)
    for b, k in enumerate(order):
        _same(got[b], alone[k], f"shape {b} ({k})")
    for k in keys:
        if k != "empty":
            _same(alone[k], R.collapse_ref(*kinds[k], target), str(k))
    assert {alone[(n, 1.0)][2] for n in ("ico0", "ico1")} <= {0, 4} and alone["empty"][2] == 1


def test_input_forms(dev):
    """_ragged.py's conventions: a strided view, int64 faces, offsets as tensors of either integer type give the canonical bits"""
    from shapeformer_amd.collapse import collapse_dev, mesh_topology_dev
    meshes = [R.case("ico2")[:2], R.icosphere(1), R.case("grid12")[:2]]
    v, f, voff, toff = _batch(meshes, dev)
    want = collapse_dev(v, f, voff, toff, 60, details=True)
    wide = torch.zeros(v.shape[0], 6, device=dev)
    wide[:, ::2] = v
    forms = [(wide[:, ::2], f, voff, toff), (v, f.long(), voff, toff), (v, f, torch.from_numpy(voff), torch.from_numpy(toff).to(torch.int32)),
             (v.double(), f.to(torch.int16), list(voff), toff.reshape(1, -1))]
    assert not forms[0][0].is_contiguous()
    for k, args in enumerate(forms):
        got = collapse_dev(*args, 60, details=True)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[4], want[4]), f"form {k}"
        assert all(np.array_equal(got[i], want[i]) for i in (2, 3, 5)), f"form {k}"
        assert torch.equal(mesh_topology_dev(*args)[0], mesh_topology_dev(v, f, voff, toff)[0])
    one = collapse_dev(*_batch(meshes[:1], dev)[:2], None, None, 60)          # None offsets: one shape
    assert torch.equal(one[0], want[0][:want[2][1]]) and torch.equal(one[1], want[1][:want[3][1]])


def test_under_budget_comes_back_as_it_is(dev):
    from shapeformer_amd.collapse import collapse_dev
    v, f, voff, toff = _batch([R.icosphere(1), R.tetrahedron()], dev)
    f[3, 0] = 1000                                                           # not inspected
    ov, of, ovo, oto, status, rounds = collapse_dev(v, f, voff, toff, 80, details=True)
    assert torch.equal(ov, v) and torch.equal(of, f) and np.array_equal(ovo, voff) and np.array_equal(oto, toff)
    assert status.tolist() == [0, 0] and list(rounds) == [0, 0]


def test_round_cap(dev):
    v, f = R.icosphere(2)
    for cap in (0, 3):
        got = _run([(v, f)], 40, dev, max_rounds=cap)[0]
        _same(got, R.collapse_ref(v, f, 40, max_rounds=cap), f"cap {cap}")
        assert got[2:] == (5, cap)


def test_sphere_radius_sanity(dev):
    """320 -> 80 faces on the icosphere of radius 0.5: no output vertex leaves the sphere by more than twice what the reference's do
    (the prototype of the issue gave 0.0198; the factor two is slack for a future change of reg, nothing else)"""
    v, f, target, want = R.case("ico2")
    ref = np.abs(np.linalg.norm(want[0].astype(np.float64), axis=1) - 0.5).max()
    got = _run([(v, f)], target, dev)[0]
    err = np.abs(np.linalg.norm(got[0].astype(np.float64), axis=1) - 0.5).max()
    print(f"max | |v| - 0.5 |: device {err:.4f}, reference {ref:.4f}")
    assert 0.0 < ref < 0.05 and err <= 2.0 * ref


def test_hybrid_route(mc_sphere, dev):
    """precluster = 4: clustered to at most 4 x 100 faces, then collapsed to the budget"""
    from shapeformer_amd.collapse import decimate_collapse_dev
    _, v, f, _ = mc_sphere
    ov, of, ovo, oto, status = decimate_collapse_dev(*_batch([(v, f), R.icosphere(1)], dev), decimate_face=100, precluster=4)
    st = status.tolist()
    print(f"hybrid: {len(f)} -> {oto[1]} faces, status {st}")
    assert st[0] in (0, 4) and st[1] == 0
    assert oto[1] - oto[0] <= 100 and oto[2] - oto[1] == 80
    pure = decimate_collapse_dev(*_batch([(v, f)], dev), decimate_face=100)
    assert pure[4].tolist() == [0] and 99 <= pure[3][1] <= 100


def test_array2mesh_wiring(mc_sphere, dev):
    from shapeformer_amd import mcubes
    from shapeformer_amd.collapse import decimate_collapse_dev
    from shapeformer_amd.simplify import decimate_dev
    occ = mc_sphere[0]
    raw = mcubes.marching_cubes_dev(torch.from_numpy(occ)[None].to(dev), 0.5)
    v, f = mcubes.array2mesh(occ, device=dev, if_decimate=True, decimate_face=300, decimate_method="collapse")
    dv, df = decimate_collapse_dev(*raw, 300)[:2]
    assert v.dtype == np.float64 and np.array_equal(v, dv.cpu().numpy().astype(np.float64)) and np.array_equal(f, df.cpu().numpy())
    assert 299 <= len(f) <= 300
    v0, f0 = mcubes.array2mesh(occ, device=dev, if_decimate=True, decimate_face=300)          # omitted: the clustering, as before
    cv, cf = decimate_dev(*raw, 300, ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)))[:2]
    assert np.array_equal(v0, cv.cpu().numpy().astype(np.float64)) and np.array_equal(f0, cf.cpu().numpy())
    v1, f1 = mcubes.array2mesh(occ, device=dev, if_decimate=True, decimate_face=300, decimate_method="cluster")
    assert np.array_equal(v1, v0) and np.array_equal(f1, f0)
