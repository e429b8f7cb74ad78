"""CPU tests of the Poisson reconstruction (shapeformer_amd/poisson.py, csrc/poisson.hip): the C-ABI surface, the
workspace helper through ctypes, every host-side refusal (raised before the library is loaded), and the numpy statement of the
contract (tests/poisson_ref.py) against brute-force definitions and against the geometry it is meant to recover."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import poisson_ref as PR
from shapeformer_amd import _lib as L
from shapeformer_amd import make_dataset as MD
from shapeformer_amd import poisson as P
from shapeformer_amd._lib import SfmiError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("sfmi_poisson_keys_f32", "sfmi_poisson_cells_i32", "sfmi_poisson_splat_f32", "sfmi_poisson_rhs_f32", "sfmi_poisson_cg_workspace_bytes",
           "sfmi_poisson_cg_init_f32", "sfmi_poisson_cg_steps_f32", "sfmi_poisson_cg_read_i32", "sfmi_poisson_iso_f32",
           "sfmi_poisson_sample_f32")


@pytest.fixture()
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(L, "lib", refuse)


def test_symbols_are_exported_declared_and_bound():
    from shapeformer_amd import build as B
    B.build(verbose=False)
    lib = ctypes.CDLL(L.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "sfmi.h")).read()
    for name in ENTRIES:
        assert hasattr(lib, name) and re.search(r"\b%s\s*\(" % name, hdr) and name in L.PROTOTYPES, name
    for name in ("poisson_splat_dev", "poisson_solve_dev", "poisson_field_dev", "poisson_recon_dev", "poisson_sample_dev", "Open3D_Toolbox"):
        assert callable(getattr(P, name))
    src = open(os.path.join(ROOT, "shapeformer_amd", "csrc", "poisson.hip")).read()
    assert '#include "sfmi_ragged.h"' in src and "wave_sum_f64" in src and "getenv" not in src
    assert "atomicAdd(float" not in src and "unsafeAtomicAdd" not in src           # the splat is a gather


def test_workspace_bytes():
    from shapeformer_amd import build as B
    B.build(verbose=False)
    ws = ctypes.CDLL(L.LIB_PATH).sfmi_poisson_cg_workspace_bytes
    ws.restype, ws.argtypes = L.PROTOTYPES["sfmi_poisson_cg_workspace_bytes"]
    for B_, R in ((0, 17), (-1, 17), (1, 0), (1, -5), (1, 4), (1, 514), (17, 513)):  # the last: 2^31 nodes or more
        assert ws(B_, R) == 0, (B_, R)
    for B_, R in ((1, 5), (1, 17), (3, 33), (1, 129), (8, 257), (1, 513)):
        n = B_ * R ** 3
        assert 12 * n <= ws(B_, R) <= 12 * n + n // 8 + 65536, (B_, R)              # three f32 lattices; partials and state are small
    assert 12 * 129 ** 3 <= ws(2, 129) - ws(1, 129) <= 12.1 * 129 ** 3              # linear in B
    assert abs((ws(8, 129) - ws(7, 129)) - (ws(2, 129) - ws(1, 129))) <= 16 * 256  # up to the 256-byte alignment of each section


def _cloud(n=10):
    return torch.zeros(n, 3), torch.ones(n, 3)


def test_shape_refusals(no_library):
    p, n = _cloud()
    for call in (P.poisson_splat_dev, P.poisson_field_dev, P.poisson_recon_dev):
        with pytest.raises(SfmiError, match=r"\(N,3\)"):
            call(torch.zeros(10, 2), torch.zeros(10, 2))
        with pytest.raises(SfmiError, match="must have the shape of the points"):
            call(p, torch.ones(9, 3))
        with pytest.raises(SfmiError, match="must have the shape of the points"):
            call(p, torch.ones(1, 10, 3))
        with pytest.raises(SfmiError, match="end at 10"):
            call(p, n, [0, 4, 9])
        with pytest.raises(SfmiError, match="offsets go with"):
            call(p[None], n[None], [0, 10])
        with pytest.raises(SfmiError, match="torch tensor"):
            call(np.zeros((10, 3), np.float32), n)
    with pytest.raises(SfmiError, match="normals are required"):
        P.poisson_splat_dev(p, None)
    with pytest.raises(SfmiError, match="normals are required"):
        P.poisson_field_dev(p, None)
    for rhs in (torch.zeros(17, 17, 17), torch.zeros(1, 17, 17, 16), np.zeros((1, 17, 17, 17)), torch.zeros(1, 4, 4, 4), torch.zeros(1, 17, 17, 17, 1)):
        with pytest.raises(SfmiError, match="poisson_solve_dev"):
            P.poisson_solve_dev(rhs)
    with pytest.raises(SfmiError, match="expected Vx"):
        P.poisson_rhs_dev(torch.zeros(1, 8, 9, 9), torch.zeros(1, 9, 8, 9), torch.zeros(1, 9, 9, 9))
    with pytest.raises(SfmiError, match="point sets for"):
        P.poisson_sample_dev(torch.zeros(2, 9, 9, 9), p, None)


@pytest.mark.parametrize("grid_dim", [4, 514, 0, -17, 17.0, "17", True])
def test_grid_dim_refused(no_library, grid_dim):
    p, n = _cloud()
    for call in (P.poisson_splat_dev, P.poisson_field_dev, P.poisson_recon_dev):
        with pytest.raises(SfmiError, match="grid_dim must be an integer"):
            call(p, n, grid_dim=grid_dim)


def test_grid_and_bbox_refusals(no_library):
    p, n = _cloud()
    for call in (P.poisson_field_dev, P.poisson_recon_dev):
        with pytest.raises(SfmiError, match="not both"):
            call(p, n, grid_dim=17, depth=4)
        for depth in (1, 10, 4.0, "4", True):
            with pytest.raises(SfmiError, match="depth must be an integer"):
                call(p, n, depth=depth)
    for call in (P.poisson_splat_dev, P.poisson_field_dev, P.poisson_recon_dev):
        for bbox in (((0, 0, 0), (0, 1, 1)), ((1, 1, 1), (-1, -1, -1)), ((0, 0, 0), (0, 0, 0))):
            with pytest.raises(SfmiError, match="degenerate"):
                call(p, n, bbox=bbox)
        for bbox in (((0, 0, 0), (1, 1, 2)), ((-1, -1, -1), (1, 1.001, 1))):
            with pytest.raises(SfmiError, match="must be a cube"):
                call(p, n, bbox=bbox)
        for bbox in (None, (0, 1), ((0, 0), (1, 1)), ((0, 0, 0), (1, 1, float("nan"))), ((0, 0, 0), (1, 1, float("inf"))), "box"):
            with pytest.raises(SfmiError, match="bbox must be"):
                call(p, n, bbox=bbox)
    with pytest.raises(SfmiError, match="fewer than 2\\^31 nodes"):
        P.poisson_field_dev(torch.zeros(17, 4, 3), torch.zeros(17, 4, 3), grid_dim=513)


def test_solver_and_trim_refusals(no_library):
    p, n = _cloud()
    rhs = torch.zeros(1, 17, 17, 17)
    for tol in (0, 0.0, -1e-4, float("nan"), float("inf"), None, "1e-4", True):
        with pytest.raises(SfmiError, match="tol must be"):
            P.poisson_solve_dev(rhs, tol=tol)
        with pytest.raises(SfmiError, match="tol must be"):
            P.poisson_field_dev(p, n, tol=tol)
        with pytest.raises(SfmiError, match="tol must be"):
            P.poisson_recon_dev(p, n, tol=tol)
    for max_iter in (-1, 2.0, "5", True):
        with pytest.raises(SfmiError, match="max_iter must be"):
            P.poisson_solve_dev(rhs, max_iter=max_iter)
        with pytest.raises(SfmiError, match="max_iter must be"):
            P.poisson_recon_dev(p, n, max_iter=max_iter)
    for check_every in (0, -1, 1.0, None, True):
        with pytest.raises(SfmiError, match="check_every must be"):
            P.poisson_solve_dev(rhs, check_every=check_every)
    for q in (1, 1.0, -0.1, 1.5, float("nan"), None, "0.3", True):
        with pytest.raises(SfmiError, match="quantile must lie"):
            P.poisson_recon_dev(p, n, quantile=q)
    with pytest.raises(SfmiError, match="needs a viewpoint"):
        P.poisson_recon_dev(p, None)
    with pytest.raises(SfmiError, match="needs a viewpoint"):
        P.poisson_recon_dev(p, None, knn=10, quantile=0.3)
    with pytest.raises(SfmiError, match="needs a viewpoint"):
        P.Open3D_Toolbox().poisson_recon(np.zeros((10, 3)))
    with pytest.raises(SfmiError, match="keep_components"):
        P.poisson_recon_dev(p, n, keep_components="biggest")


def test_cpu_tensors_are_refused_last(no_library):
    p, n = _cloud()
    calls = (lambda: P.poisson_splat_dev(p, n), lambda: P.poisson_splat_dev(p[None], n[None], grid_dim=9),
             lambda: P.poisson_field_dev(p, n, [0, 4, 10], depth=4), lambda: P.poisson_recon_dev(p, n, quantile=0.3, keep_components="largest"),
             lambda: P.poisson_recon_dev(p, None, viewpoint=(0, 0, 2.0)), lambda: P.poisson_solve_dev(torch.zeros(2, 8, 8, 8), max_iter=0),
             lambda: P.poisson_rhs_dev(torch.zeros(1, 8, 9, 9), torch.zeros(1, 9, 8, 9), torch.zeros(1, 9, 9, 8)),
             lambda: P.poisson_sample_dev(torch.zeros(1, 9, 9, 9), p))
    for call in calls:
        with pytest.raises(SfmiError, match="HIP device.*no CPU fallback"):
            call()


def test_make_dataset_poisson_grid(tmp_path):
    assert "poisson" in MD.OCCUPANCY and MD.check_poisson_grid(17, 33) == 2 and MD.check_poisson_grid(17, 17) == 1
    assert MD.check_poisson_grid(64, 127) == 2 and MD.check_poisson_grid(65, 129) == 2
    for grid, pg in ((17, 34), (17, 32), (17, 16), (17, 9), (64, 129), (17, 0)):
        with pytest.raises(ValueError, match="poisson-grid"):
            MD.check_poisson_grid(grid, pg)
        with pytest.raises(ValueError, match="poisson-grid"):                    # before any file is read or any device is touched
            MD.make_dataset([str(tmp_path / "missing.ply")], str(tmp_path), "d", grid=grid, occupancy="poisson", poisson_grid=pg)
        with pytest.raises(SystemExit):
            MD.parse_args(["a.ply", "--out", "o", "--dataset", "d", "--grid", str(grid), "--occupancy", "poisson", "--poisson-grid", str(pg)])
    a = MD.parse_args(["a.ply", "--out", "o", "--dataset", "d", "--grid", "17", "--occupancy", "poisson", "--poisson-grid", "33"])
    assert a.occupancy == "poisson" and a.poisson_grid == 33
    a = MD.parse_args(["a.obj", "--out", "o", "--dataset", "d"])                  # winding stays the default; its route never looks at the grid
    assert a.occupancy == "winding" and a.poisson_grid is None
    # no --poisson-grid: the smallest m (grid - 1) + 1 >= 129
    assert [MD.check_poisson_grid(g) for g in (64, 65, 17, 16, 129, 200)] == [3, 2, 8, 9, 1, 1]


def test_make_dataset_refuses_a_cloud_without_normals(tmp_path):
    from shapeformer_amd import meshio
    path = str(tmp_path / "bare.ply")
    meshio.write_ply(path, np.random.RandomState(0).rand(20, 3), np.zeros((0, 3), np.int32))
    with pytest.raises(ValueError, match="bare.ply.*no normals"):
        MD._poisson_batch([path], 17, 33, 64, 1.0, 0, torch.device("cpu"))


# ---- the numpy statement against brute-force definitions, R = 5

def _random_cloud(rs, n, R):
    p = (rs.rand(n, 3) * 2.4 - 1.2).astype(np.float32)                           # some outside the box
    node = np.linspace(-1, 1, R)
    p[:6] = node[rs.randint(0, R, (6, 3))]                                       # exactly on nodes
    p[6:10, 0] = [1.0, -1.0, 1.0, -1.0]                                          # on box faces
    p[6:10, 1:] = np.clip(p[6:10, 1:], -1, 1)
    nrm = rs.randn(n, 3).astype(np.float32)
    return p, nrm


def test_splat_equals_the_per_point_loop():
    rs = np.random.RandomState(0)
    p, nrm = _random_cloud(rs, 80, 5)
    fast, slow = PR.splat(p, nrm, 5), PR.splat_loop(p, nrm, 5)
    assert fast[4] == slow[4] and 0 < fast[4] < 80
    for a, b in zip(fast[:4], slow[:4]):
        assert a.shape == b.shape and np.allclose(a, b, rtol=1e-13, atol=1e-14)
    inside = PR.coords(p, 5)[1]
    assert np.isclose(fast[3].sum(), inside.sum())                               # the node weights of an inside point sum to 1
    one = PR.splat(np.float32([[0.25, -0.5, 1.0]]), np.float32([[2.0, 3.0, 5.0]]), 5)   # t = (2.5, 1, 4): between two nodes along x only
    assert np.isclose(one[3][2, 1, 4], 0.5) and np.isclose(one[3][3, 1, 4], 0.5) and np.isclose(one[3].sum(), 1.0)
    assert np.isclose(one[0][2, 1, 4], 2.0) and np.isclose(one[0].sum(), 2.0)    # exactly on the Vx site (2.5, 1, 4)
    assert np.isclose(one[1][2, 0, 4] + one[1][2, 1, 4] + one[1][3, 0, 4] + one[1][3, 1, 4], 3.0)
    assert np.isclose(one[2].sum(), 2.5)                                         # z = hi face: half of Vz's weight falls outside the array


def test_operator_and_rhs_equal_the_explicit_gradient():
    R = 5
    G, A = PR.gradient(R), PR.laplacian(R)
    assert G.shape == (3 * (R + 1) * R * R, R ** 3)
    GtG = (G.T @ G).toarray()
    assert np.array_equal(GtG, A.toarray()) and np.all(np.diag(GtG) == 6.0) and np.array_equal(GtG, GtG.T)
    assert np.linalg.eigvalsh(GtG).min() > 0                                     # symmetric positive definite
    ev = np.linalg.eigvalsh(GtG)
    assert np.isclose(ev.max() / ev.min(), PR.kappa(R))
    rs = np.random.RandomState(1)
    x = rs.randn(R, R, R)
    assert np.allclose(PR.apply_A(x).ravel(), A @ x.ravel())
    p, nrm = _random_cloud(rs, 60, R)
    Vx, Vy, Vz, _, _ = PR.splat(p, nrm, R)
    b = PR.rhs(Vx, Vy, Vz)
    assert np.allclose(b.ravel(), -(G.T @ PR.pad_edges(Vx, Vy, Vz)), rtol=1e-13, atol=1e-14)
    chi = PR.cg64(b)
    assert PR.true_residual(chi, b) < 1e-10
    assert np.allclose(chi.ravel(), np.linalg.solve(GtG, b.ravel()))            # the minimiser of |G chi + V|^2
    keep, nf = PR.quantile_trim(np.float32([5, 1, 3, 4, 2]), np.array([[0, 2, 3], [0, 1, 2], [2, 3, 4]]), 0.5)
    assert keep.tolist() == [True, False, True, True, False] and nf.tolist() == [[0, 1, 2]]


# ---- the formulation's geometry, on the reference alone

@pytest.mark.parametrize("R,n", [(17, 2000), (33, 4000)])
def test_sphere_is_recovered_within_half_a_cell(R, n):
    p, nrm = PR.sphere_cloud(n, 0.5, seed=R)
    fld, W = PR.field(p, nrm, R)
    h = 2.0 / (R - 1)
    count, radius = PR.ray_crossings(fld, 500)
    err = np.abs(radius - 0.5) / h
    print(f"R = {R}: crossings {count.min()} .. {count.max()}, |r - 0.5| / h max {err.max():.3f} mean {err.mean():.3f}")
    assert np.all(count == 1)
    assert err.max() <= 0.5
    c = (R - 1) // 2
    assert fld[c, c, c] > 0
    corners = fld[[0, 0, 0, 0, -1, -1, -1, -1], [0, 0, -1, -1, 0, 0, -1, -1], [0, -1, 0, -1, 0, -1, 0, -1]]
    assert np.all(corners < 0)
    assert np.isclose(W.sum(), n)
