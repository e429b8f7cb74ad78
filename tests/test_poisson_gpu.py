"""GPU tests of the Poisson reconstruction (shapeformer_amd/poisson.py, csrc/poisson.hip) against the f64 statement
of tests/poisson_ref.py.  The shapes are small on purpose: lattices of 8, 9, 17 and 33 nodes (33 = 16 + 16 + 1 and 17 = 16 + 1: every
tile of the stencil kernel has a ragged edge, 33 spans more than one tile and more than one chunk of planes), a batch of three."""
import numpy as np
import pytest
import torch

import meshsdf_ref as MR
import poisson_ref as PR
from shapeformer_amd import components as CC
from shapeformer_amd import make_dataset as MD
from shapeformer_amd import meshio
from shapeformer_amd import poisson as P
from shapeformer_amd._lib import SfmiError

pytestmark = pytest.mark.gpu

VIEW = (0.0, 0.0, 3.0)


def _off(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(*ts):
    return [t.cpu().numpy() if isinstance(t, torch.Tensor) else t for t in ts]


# ---- 5. splat parity

@pytest.fixture(scope="module")
def cloud():
    """600 points and normals: random ones (a fifth outside the box), 8 exactly on nodes of the 9- and 17-lattice, 8 on box faces (the
    upper ones included), 25 copies of one point and 25 more points in the same cell of both lattices"""
    rs = np.random.RandomState(5)
    p = (rs.rand(600, 3) * 2.3 - 1.15).astype(np.float32)
    p[:8] = np.linspace(-1, 1, 9)[rs.randint(0, 9, (8, 3))]
    p[8:16] = np.clip(p[8:16], -1, 1)
    for r, (a, v) in enumerate([(0, 1.0), (0, -1.0), (1, 1.0), (1, -1.0), (2, 1.0), (2, -1.0), (0, 1.0)]):
        p[8 + r, a] = v                                                         # one coordinate on a face of the box
    p[15] = [1.0, 1.0, 1.0]                                                     # the upper corner
    p[16:41] = np.float32([0.3, -0.45, 0.7])                                    # 25 duplicates
    p[41:66] = np.float32([0.26, -0.49, 0.63]) + rs.rand(25, 3).astype(np.float32) * 0.11   # the same cell at h = 0.25 and h = 0.125
    n = rs.randn(600, 3).astype(np.float32)
    return p, n


@pytest.fixture(scope="module")
def sets(cloud):
    """four ragged sets: none, one point, the 600, the 600 in reverse order"""
    p, n = cloud
    return np.concatenate([p[100:101], p, p[::-1]]), np.concatenate([n[100:101], n, n[::-1]]), _off([0, 1, 600, 600])


@pytest.fixture(scope="module")
def splat_refs(sets):
    p, n, off = sets
    return {R: [PR.splat(p[off[b]:off[b + 1]], n[off[b]:off[b + 1]], R) for b in range(4)] for R in (9, 17)}


@pytest.mark.parametrize("R", [9, 17])
def test_splat_matches_the_f64_reference(dev, sets, splat_refs, R):
    p, n, off = sets
    out = P.poisson_splat_dev(_t(p, dev), _t(n, dev), off, grid_dim=R)
    Vx, Vy, Vz, W, outside = _np(*out)
    assert Vx.shape == (4, R - 1, R, R) and Vy.shape == (4, R, R - 1, R) and Vz.shape == (4, R, R, R - 1) and W.shape == (4, R, R, R)
    assert all(a.dtype == np.float32 for a in (Vx, Vy, Vz, W)) and outside.dtype == np.int32
    worst = 0.0
    for b in range(4):
        ref, cnt = splat_refs[R][b], off[b + 1] - off[b]
        assert outside[b] == ref[4]
        for got, want in zip((Vx[b], Vy[b], Vz[b], W[b]), ref[:4]):
            err = np.abs(got.astype(np.float64) - want)
            bound = 2.0 ** -23 * np.abs(want) + 1e-12 * cnt                      # one f32 rounding of an f64 sum + the order of that sum
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()) if cnt else float(err.max()))
            assert np.all(err <= bound)
    print(f"R = {R}: worst error / bound = {worst:.3f}; outside = {outside.tolist()}")
    assert outside[0] == 0 and outside[2] == outside[3] > 50 and not Vx[0].any() and not W[0].any()
    again = P.poisson_splat_dev(_t(p, dev), _t(n, dev), off, grid_dim=R)
    assert all(torch.equal(a, b) for a, b in zip(out, again))                   # bit-identical from run to run
    for b in range(4):                                                          # and each set alone
        solo = P.poisson_splat_dev(_t(p[off[b]:off[b + 1]], dev), _t(n[off[b]:off[b + 1]], dev), None, grid_dim=R)
        assert all(torch.equal(s[0], o[b]) for s, o in zip(solo, out))


def test_splat_refuses_non_finite_input(dev, cloud):
    p, n = cloud
    for arr in (0, 1):
        q = [p.copy(), n.copy()]
        q[arr][77, 1] = np.nan if arr else np.inf
        with pytest.raises(SfmiError, match="not finite"):
            P.poisson_splat_dev(_t(q[0], dev), _t(q[1], dev), None, grid_dim=9)


# ---- 6. the solver

@pytest.fixture(scope="module")
def systems(dev, cloud):
    """per R: the right-hand sides of three shapes (the 600 points, no points: b = 0, the first 300 points) on the device and in f64"""
    p, n = cloud
    pts, nrm, off = np.concatenate([p, p[:300]]), np.concatenate([n, n[:300]]), _off([600, 0, 300])
    out = {}
    for R in (8, 17, 33):
        Vx, Vy, Vz, _, _ = P.poisson_splat_dev(_t(pts, dev), _t(nrm, dev), off, grid_dim=R)
        rhs = P.poisson_rhs_dev(Vx, Vy, Vz)
        want = np.stack([PR.rhs(*[a[b].astype(np.float64) for a in _np(Vx, Vy, Vz)]) for b in range(3)])
        got = rhs.cpu().numpy()
        assert np.all(np.abs(got - want) <= 2.0 ** -23 * np.abs(want))           # the f64 difference of f32 values, rounded once
        assert not got[1].any() and got[0].any() and got[2].any()
        out[R] = rhs
    return out


@pytest.mark.parametrize("R", [8, 17, 33])
def test_solve(dev, systems, R):
    rhs, tol = systems[R], 1e-4
    chi, it, res = P.poisson_solve_dev(rhs, tol=tol)
    assert chi.shape == rhs.shape and chi.dtype == torch.float32 and it.dtype == torch.int32 and res.dtype == torch.float64
    x, b, it_h, res_h = chi.cpu().numpy(), rhs.cpu().numpy(), it.cpu().numpy(), res.cpu().numpy()
    assert np.isfinite(x).all()
    true = [PR.true_residual(x[s], b[s]) for s in (0, 2)]
    print(f"R = {R}: iterations {it_h.tolist()}, recursive residual {res_h.tolist()}, true residual {true}")
    assert np.all(res_h <= tol) and np.all(it_h <= 4 * R) and np.all(it_h[[0, 2]] > 0)
    assert max(true) <= 2 * tol
    assert it_h[1] == 0 and res_h[1] == 0 and not x[1].any()                     # b = 0: zeros, no iteration
    if R == 17:
        import scipy.sparse.linalg as spla
        A = PR.laplacian(R).tocsc()
        for s, tr in zip((0, 2), true):
            star = spla.spsolve(A, b[s].astype(np.float64).ravel())
            rel = np.linalg.norm(x[s].ravel() - star) / np.linalg.norm(star)
            print(f"  shape {s}: |chi - chi*| / |chi*| = {rel:.3e}, kappa * true residual = {PR.kappa(R) * tr:.3e}")
            assert rel <= PR.kappa(R) * tr
    # exactly max_iter iterations, whatever the chunking
    c5, it5, _ = P.poisson_solve_dev(rhs, tol=tol, max_iter=5)
    assert it5.cpu().tolist() == [5, 0, 5]
    c5b, it5b, _ = P.poisson_solve_dev(rhs, tol=tol, max_iter=5, check_every=2)
    assert torch.equal(c5, c5b) and torch.equal(it5, it5b) and not torch.equal(c5, chi)
    c0, it0, res0 = P.poisson_solve_dev(rhs, tol=tol, max_iter=0)
    assert not c0.any() and it0.cpu().tolist() == [0, 0, 0] and res0.cpu().tolist() == [1.0, 0.0, 1.0]
    # the result does not depend on check_every: shapes are frozen on the device
    c1, it1, res1 = P.poisson_solve_dev(rhs, tol=tol, check_every=1)
    assert torch.equal(c1, chi) and torch.equal(it1, it) and torch.equal(res1, res)
    # a shape alone equals the same shape in the batch
    for s in range(3):
        cs, its, rs_ = P.poisson_solve_dev(rhs[s:s + 1].clone(), tol=tol)
        assert torch.equal(cs[0], chi[s]) and its[0] == it[s] and rs_[0] == res[s]


def test_solve_largest_lattice_one_step(dev):
    """R = 513 (the third instance of the plane march and of the element-wise span; node indices up to 1.35e8): from b = a unit impulse
    one CG step is known in closed form: alpha = |b|^2 / <b, A b> = 1/6, chi = b / 6, r = b - A b / 6 = 1/6 on the neighbours - five of
    them for an impulse on a face, the sixth being a zero outside the lattice - so |r| / |b| = sqrt(5) / 6 up to the f32 rounding of
    alpha.  Two steps are compared with f64 CG on an 11^3 box that holds the same impulse on the same face."""
    R = 513
    rhs = torch.zeros(1, R, R, R, device=dev)
    i, j, k = R - 7, R - 8, R - 1                                               # on the upper z face, five nodes from the other faces
    rhs[0, i, j, k] = 1.0
    chi, it, res = P.poisson_solve_dev(rhs, max_iter=1)
    assert it.cpu().tolist() == [1] and int(chi.count_nonzero()) == 1 and float(chi[0, i, j, k]) == float(np.float32(1.0 / 6.0))
    assert abs(float(res[0]) - np.sqrt(5.0) / 6.0) < 1e-7
    chi2, it2, _ = P.poisson_solve_dev(rhs, max_iter=2)
    want = PR.cg64(np.pad(np.ones((1, 1, 1)), ((5, 5), (5, 5), (10, 0))), tol=1e-30, max_iter=2)
    got = chi2[0, i - 5:i + 6, j - 5:j + 6, k - 10:].cpu().numpy()
    assert it2.cpu().tolist() == [2] and int(chi2.count_nonzero()) == 6 and np.count_nonzero(want) == 6
    assert got.shape == want.shape == (11, 11, 11) and np.allclose(got, want, rtol=1e-6, atol=0)


# ---- 7. end to end

@pytest.fixture(scope="module")
def sphere():
    return PR.sphere_cloud(4000, 0.5, seed=33)


@pytest.fixture(scope="module")
def sphere_mesh(dev, sphere):
    p, n = sphere
    return P.poisson_recon_dev(_t(p, dev), _t(n, dev), depth=5)


def _euler(faces):
    e = np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]), axis=1)
    return len(np.unique(faces)) - len(np.unique(e, axis=0)) + len(faces)


def test_sphere_end_to_end(dev, sphere, sphere_mesh):
    v, f, voff, toff, density = sphere_mesh
    h = 2.0 / 32
    r = np.linalg.norm(v.cpu().numpy().astype(np.float64), axis=1)
    print(f"{len(v)} vertices, {len(f)} faces, |r - 0.5| / h max {np.abs(r - 0.5).max() / h:.3f}")
    assert len(v) > 500 and voff.tolist() == [0, len(v)] and toff.tolist() == [0, len(f)] and density.shape == (len(v),)
    assert np.abs(r - 0.5).max() <= 0.5 * h
    coff = CC.mesh_components_dev(v, f, voff, toff)[2]
    assert coff[-1] == 1
    assert _euler(f.cpu().numpy()) == 2
    assert torch.isfinite(density).all() and density.min() > 0


def test_batch_equals_solo_and_an_empty_set_gives_nothing(dev, sphere, sphere_mesh):
    p, n = sphere
    q, m = PR.sphere_cloud(1500, 0.6, seed=7)
    far = np.float32([[3, 3, 3], [-2, 0, 0]])                                   # a set without an in-box point
    pts, nrm, off = np.concatenate([p, far, q]), np.concatenate([n, far, m]), _off([4000, 2, 1500])
    v, f, voff, toff, d = P.poisson_recon_dev(_t(pts, dev), _t(nrm, dev), off, depth=5)
    solo2 = P.poisson_recon_dev(_t(q, dev), _t(m, dev), depth=5)
    assert voff[2] == voff[1] and toff[2] == toff[1]                            # no in-box point: an empty mesh
    for b, solo in ((0, sphere_mesh), (2, solo2)):
        assert torch.equal(v[voff[b]:voff[b + 1]], solo[0]) and torch.equal(f[toff[b]:toff[b + 1]], solo[1])
        assert torch.equal(d[voff[b]:voff[b + 1]], solo[4])
    field, W, info = P.poisson_field_dev(_t(pts, dev), _t(nrm, dev), off, depth=5)
    assert torch.isfinite(field).all() and not field[1].any() and not W[1].any()
    assert info["outside"].cpu().tolist() == [0, 2, 0] and info["iso"][1] == 0 and info["iterations"][1] == 0
    c = 16
    assert field[0, c, c, c] > 0 and field[0, 0, 0, 0] < 0 and field[2, c, c, c] > 0 and field[2, -1, -1, -1] < 0
    count, radius = PR.ray_crossings(field[0].cpu().numpy().astype(np.float64), 500)   # the device field, measured as the f64 one is
    print(f"device field: crossings {count.min()} .. {count.max()}, |r - 0.5| / h max {np.abs(radius - 0.5).max() * 16:.3f}")
    assert np.all(count == 1) and np.abs(radius - 0.5).max() <= 0.5 / 16


@pytest.fixture(scope="module")
def hemisphere(dev):
    p, _ = PR.sphere_cloud(6000, 0.5, seed=11)
    p = p[p[:, 2] > 0.1][:2300]                                                 # what VIEW sees of the sphere: n . (VIEW - p) > 0 from z > 1/12
    x = _t(p, dev)
    return x, P.poisson_recon_dev(x, None, depth=5, viewpoint=VIEW, knn=10)


def test_estimated_normals_from_a_viewpoint(dev, hemisphere):
    x, (v, f, voff, toff, d) = hemisphere
    assert len(v) > 100 and len(f) > 100 and torch.isfinite(v).all() and torch.isfinite(d).all()
    assert int(f.min()) >= 0 and int(f.max()) < len(v)
    from shapeformer_amd.scan import estimate_normals_dev
    nrm = estimate_normals_dev(x, None, 10, VIEW)[0]
    field, _, info = P.poisson_field_dev(x, nrm, depth=5)
    assert torch.isfinite(field).all() and info["outside"].cpu().tolist() == [0] and bool(torch.isfinite(info["iso"]).all())
    with pytest.raises(SfmiError, match="needs a viewpoint"):
        P.poisson_recon_dev(x, None, depth=5)


# ---- 8. the trim

def test_quantile_trim(dev, hemisphere):
    x, (v, f, voff, toff, d) = hemisphere
    same = P.poisson_recon_dev(x, None, depth=5, viewpoint=VIEW, knn=10, quantile=0.0)
    assert all(torch.equal(a, b) for a, b in zip((v, f, d), (same[0], same[1], same[4])))
    d_h = d.cpu().numpy().astype(np.float64)
    # the surface that closes the open side lies where no point is: its vertices have density 0, and they are more than 30 % of all, so
    # the 0.3-quantile is 0 and nothing lies below it; 0.7 cuts into the scanned side
    for q in (0.3, 0.7):
        tv, tf, tvo, tto, td = P.poisson_recon_dev(x, None, depth=5, viewpoint=VIEW, knn=10, quantile=q)
        td_h, tf_h = td.cpu().numpy().astype(np.float64), tf.cpu().numpy()
        thr = np.quantile(d_h, q)
        keep, want_f = PR.quantile_trim(d_h, f.cpu().numpy(), q)
        print(f"trim {q}: {len(v)} -> {len(tv)} vertices, {len(f)} -> {len(tf)} faces, threshold {thr:.4f}")
        assert np.all(td_h >= thr) and len(tv) == int((d_h >= thr).sum()) == tvo[-1] and len(tv) > 0
        assert tto[-1] == len(tf) and tf_h.min() >= 0 and tf_h.max() < len(tv)
        assert torch.equal(tv, v[_t(keep, dev)]) and np.array_equal(td_h, d_h[keep]) and np.array_equal(tf_h, want_f)
    assert thr > 0 and len(tv) < len(v) and len(tf) < len(f)
    kv, kf, kvo, kto, kd = P.poisson_recon_dev(x, None, depth=5, viewpoint=VIEW, knn=10, quantile=0.7, keep_components="largest")
    assert CC.mesh_components_dev(kv, kf, kvo, kto)[2][-1] == 1 and len(kd) == len(kv) <= len(tv)


# ---- 9. make_dataset --occupancy poisson

def _occupancy_check(occ, grid):
    X = np.stack(np.meshgrid(*[np.linspace(-1, 1, grid)] * 3, indexing="ij"), -1)
    r = np.linalg.norm(X, axis=-1)
    wrong = (occ != 0) != (r < 0.5)
    h = 2.0 / (grid - 1)
    print(f"grid {grid}: {int(wrong.sum())} nodes differ, the farthest {np.abs(r[wrong] - 0.5).max() / h if wrong.any() else 0:.3f} h away")
    assert occ.shape == (grid, grid, grid) and np.all(np.abs(r[wrong] - 0.5) < h) and (occ != 0).sum() > 10


def test_make_dataset_poisson(dev, tmp_path, sphere):
    """The issue's case is a store of 17 nodes per axis from a Poisson lattice of 33.  write_imnet_store packs bits and refuses a
    lattice whose node count is no multiple of 8 (17^3 is odd), so that case runs through make_dataset's per-batch function, and the
    command line end to end runs at 16 nodes from a lattice of 31, with the same bound."""
    p, n = sphere
    path = str(tmp_path / "sphere.ply")
    meshio.write_ply(path, p, np.zeros((0, 3), np.int32), normal=n)
    x, occ = MD._poisson_batch([path], 17, 33, 256, 1.0, 0, dev)
    assert x.shape == (1, 256, 3) and np.abs(np.linalg.norm(x[0].cpu().numpy(), axis=1) - 0.5).max() < 1e-6
    _occupancy_check(occ[0].cpu().numpy(), 17)
    MD.main([path, "--out", str(tmp_path / "root"), "--dataset", "scan", "--grid", "16", "--boundary-n", "256", "--occupancy", "poisson",
             "--poisson-grid", "31"])
    d = tmp_path / "root" / "scan" / "train"
    Xbd, Ytg = np.load(d / "Xbd.npy"), np.load(d / "Ytg.npy")
    assert Xbd.shape == (1, 256, 3) and Xbd.dtype == np.float32 and Ytg.shape == (1, 16 ** 3 // 8)
    _occupancy_check(np.unpackbits(Ytg[0]).reshape(16, 16, 16), 16)
    bare = str(tmp_path / "bare.ply")
    meshio.write_ply(bare, p, np.zeros((0, 3), np.int32))
    with pytest.raises(ValueError, match="bare.ply.*no normals"):
        MD.main([bare, "--out", str(tmp_path / "root"), "--dataset", "bare", "--grid", "16", "--occupancy", "poisson", "--poisson-grid", "31"])
    # the toolbox call of the reference, for the same cloud
    vert, face = P.Open3D_Toolbox().poisson_recon(p, normals=n, depth=5, quantile=.3)
    assert vert.dtype == np.float64 and vert.shape[1] == 3 and np.issubdtype(face.dtype, np.integer) and face.shape[1] == 3
    assert len(vert) > 100 and face.min() >= 0 and face.max() < len(vert) and np.abs(np.linalg.norm(vert, axis=1) - 0.5).max() < 2.0 / 32


def test_make_dataset_winding_route_is_unchanged(dev, tmp_path):
    from shapeformer_amd import meshsdf
    from shapeformer_amd._ragged import batch_meshes
    from shapeformer_amd.metrics import sample_mesh_dev
    v, f = MR.icosphere(2, r=3.0)
    path = str(tmp_path / "a.obj")
    with open(path, "w") as fh:
        fh.write("".join(f"v {x} {y} {z}\n" for x, y, z in v) + "".join(f"f {a + 1} {b + 1} {c + 1}\n" for a, b, c in f))
    MD.main([path, "--out", str(tmp_path / "root"), "--dataset", "mesh", "--grid", "16", "--boundary-n", "512", "--seed", "3"])
    d = tmp_path / "root" / "mesh" / "train"
    rv, rf = meshio.read_mesh(path)                                             # the untouched code path, call by call
    bv, bf, voff, toff = batch_meshes([(meshsdf.normalize_point_set(rv), rf)], dev)
    occ, st = meshsdf.mesh_occupancy_dev(bv, bf, voff, toff, grid_dim=16, return_status=True)
    x, st2 = sample_mesh_dev(bv, bf, voff, toff, 512, seed=3)
    assert int(st[0]) == 0 and int(st2[0]) == 0
    assert np.array_equal(np.load(d / "Ytg.npy"), np.packbits(occ.cpu().numpy().reshape(1, -1) != 0, axis=-1))
    assert np.array_equal(np.load(d / "Xbd.npy"), x.reshape(1, 512, 3).cpu().numpy())
