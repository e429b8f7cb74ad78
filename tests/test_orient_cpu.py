"""CPU tests of the consistent normal orientation (shapeformer_amd/scan.py orient_normals_dev, csrc/tangent.hip): the
numpy statement of the contract (tests/orient_ref.py) against analytic truth with its own cKDTree table and numpy PCA normals, its
Boruvka restatement against Kruskal on the tie-break scene, the C-ABI surface, and every host-side refusal (raised before the library
is loaded, the device check last)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import orient_ref as OR
from shapeformer_amd import _lib as L
from shapeformer_amd import make_dataset as MD
from shapeformer_amd import poisson as P
from shapeformer_amd import scan as S
from shapeformer_amd._lib import SfmiError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("sfmi_tangent_workspace_bytes", "sfmi_tangent_forest_f32", "sfmi_tangent_apply_f32")


@pytest.fixture()
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(L, "lib", refuse)


# ---- the reference against analytic truth ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scene", ["sphere", "torus"])
def test_reference_orients_closed_surfaces_outward(scene):
    p, outward = OR.sphere(2048, 0.5, seed=3) if scene == "sphere" else OR.torus(2048, 0.5, 0.2, seed=3)
    idx = OR.knn_table(p, 12)
    nrm = OR.pca_normals(p, idx)
    rng = np.random.default_rng(5)
    nrm = nrm * np.where(rng.random(len(p)) < 0.5, -1.0, 1.0).astype(np.float32)[:, None]      # arbitrary signs in
    r = OR.orient(p, nrm, idx, with_boruvka=True)
    assert r["n_components"].tolist() == [1] and len(r["tree"][0]) == len(p) - 1
    assert r["margin"] >= 1e-9
    assert ((r["normal"].astype(np.float64) * outward).sum(1) > 0).all()
    same = (r["normal"] == nrm).all(1) | (r["normal"] == -nrm).all(1)
    assert same.all()                                                                           # the input or its exact negation
    assert 1 <= r["rounds"][0] <= int(np.ceil(np.log2(len(p))))


def test_reference_boruvka_equals_kruskal_on_the_tie_break_scene():
    p = OR.thin_box(2048, seed=7)
    idx = OR.knn_table(p, 16)
    nrm = OR.pca_normals(p, idx)
    lo, hi, bits, flip = OR.graph_edges(nrm, idx)
    assert len(bits) > 10000 and (np.bincount(np.unique(bits, return_inverse=True)[1]).max() > 5000)    # one weight, thousands of edges
    key = np.stack([bits, lo.astype(np.uint64), hi.astype(np.uint64)], 1)
    assert (np.lexsort((hi, lo, bits)) == np.arange(len(bits))).all() and len(np.unique(key, axis=0)) == len(key)   # strict order
    take_k = OR.kruskal(len(p), lo, hi)
    take_b, rounds, _ = OR.boruvka(len(p), lo, hi)
    assert np.array_equal(take_k, take_b) and rounds >= 1
    comp, par = OR.forest_outputs(len(p), lo, hi, flip, take_k)
    assert take_k.sum() == len(p) - len(np.unique(comp))


def test_reference_small_cases():
    # a triangle with one heavy edge, a dead vertex, a directed-only entry and a repeated pair
    nrm = np.array([[0, 0, 1], [0, 0, -1], [0, 0.6, 0.8], [0, 0, 0], [1, 0, 0]], np.float32)
    idx = np.array([[1, 1, 3], [0, 2, -1], [0, 9, 2], [0, 1, 2], [-1, -1, 2]], np.int32)
    lo, hi, bits, flip = OR.graph_edges(nrm, idx)
    assert list(zip(lo.tolist(), hi.tolist())) == [(0, 1), (0, 2), (1, 2), (2, 4)]             # w = 0, 0.2, 0.2, 1; the dead 3 has no edge
    assert flip.tolist() == [True, False, True, False]
    r = OR.orient(np.zeros((5, 3), np.float32), nrm, idx)
    assert r["tree"][0] == {(0, 1), (0, 2), (2, 4)}
    assert r["component"].tolist() == [0, 0, 0, 3, 0] and r["parity"].tolist() == [0, 1, 0, 0, 0]
    assert r["n_components"].tolist() == [2]
    p, nrm, idx, sign = OR.chain(1000)
    r = OR.orient(p, nrm, idx, with_boruvka=True)
    assert r["rounds"].tolist() == [1] and r["chain"].tolist() == [999]
    assert np.array_equal(r["parity"], (sign != sign[0]).astype(np.uint8))


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------

def test_symbols_are_exported_declared_and_bound():
    from shapeformer_amd import build as B
    B.build(verbose=False)
    lib = ctypes.CDLL(L.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "sfmi.h")).read()
    for name in ENTRIES:
        assert hasattr(lib, name) and re.search(r"\b%s\s*\(" % name, hdr) and name in L.PROTOTYPES, name
    assert sorted(n for n in L.PROTOTYPES if n.startswith("sfmi_tangent_")) == sorted(ENTRIES)
    assert len(L.PROTOTYPES["sfmi_tangent_forest_f32"][1]) == 14 and len(L.PROTOTYPES["sfmi_tangent_apply_f32"][1]) == 12
    ws = lib.sfmi_tangent_workspace_bytes
    ws.restype, ws.argtypes = L.PROTOTYPES["sfmi_tangent_workspace_bytes"]
    for B_, N in ((0, 10), (-1, 10), (1, -1), (1, 2 ** 31)):
        assert ws(B_, N) == 0, (B_, N)
    for B_, N in ((1, 1), (3, 1000), (1, 10 ** 6)):
        assert 36 * N <= ws(B_, N) <= 36 * N + 11 * 256, (B_, N)                               # 4 int32, 2 uint64 and 4 bytes per vertex
    assert ws(65535, 0) >= 24 * 65535                                                          # the centroids
    src = open(os.path.join(ROOT, "shapeformer_amd", "csrc", "tangent.hip")).read()
    assert '#include "sfmi_ragged.h"' in src and "sfmi_centroid_f64" in src and "getenv" not in src
    assert "atomicAdd(float" not in src and "unsafeAtomicAdd" not in src and "atomicCAS" not in src
    feat = open(os.path.join(ROOT, "shapeformer_amd", "csrc", "features.hip")).read()
    assert "sfmi_centroid_f64" in feat                                                          # one copy of the centroid's sum


# ---- refusals -------------------------------------------------------------------------------------------------------------------------

def test_refusals_come_before_the_library(no_library):
    p, n = torch.zeros(10, 3), torch.ones(10, 3)
    for k in (0, 65, -1, 2.0, "8", True, None):
        with pytest.raises(SfmiError, match="k must be an integer"):
            S.orient_normals_dev(p, n, k=k)
    for k in (0, 65):
        with pytest.raises(SfmiError, match="k must be an integer"):
            S.orient_normals_dev(p, n, idx=torch.zeros(10, k, dtype=torch.int32))
    for anchor in ("inward", None, 0, "Outward"):
        with pytest.raises(SfmiError, match="anchor must be one of"):
            S.orient_normals_dev(p, n, anchor=anchor)
    with pytest.raises(SfmiError, match="anchor='viewpoint' needs"):
        S.orient_normals_dev(p, n, anchor="viewpoint")
    with pytest.raises(SfmiError, match=r"expected \(2,3\) viewpoints"):
        S.orient_normals_dev(p, n, [0, 4, 10], anchor="viewpoint", viewpoint=(0, 0, 1.0))
    with pytest.raises(SfmiError, match=r"expected \(1,3\) viewpoints"):
        S.orient_normals_dev(p, n, anchor="viewpoint", viewpoint=np.zeros((2, 3)))
    with pytest.raises(SfmiError, match="goes with anchor='viewpoint'"):
        S.orient_normals_dev(p, n, viewpoint=(0, 0, 1.0))
    with pytest.raises(SfmiError, match="normals must be a tensor of the points' shape"):
        S.orient_normals_dev(p, n[:9])
    with pytest.raises(SfmiError, match="normals must be a tensor of the points' shape"):
        S.orient_normals_dev(p, n.numpy())
    with pytest.raises(SfmiError, match="normals must be a tensor of the points' shape"):
        S.orient_normals_dev(p[None], n)
    with pytest.raises(SfmiError, match="idx must be an int32"):
        S.orient_normals_dev(p, n, idx=torch.zeros(10, 4, dtype=torch.int64))
    with pytest.raises(SfmiError, match="idx must be"):
        S.orient_normals_dev(p, n, idx=torch.zeros(9, 4, dtype=torch.int32))
    with pytest.raises(SfmiError, match="idx must be"):
        S.orient_normals_dev(p[None], n[None], idx=torch.zeros(10, 4, dtype=torch.int32))
    with pytest.raises(SfmiError, match=r"expected \(N,3\) or \(B,N,3\) points"):
        S.orient_normals_dev(torch.zeros(10, 2), torch.zeros(10, 2))
    with pytest.raises(SfmiError, match="offsets must start at 0"):
        S.orient_normals_dev(p, n, [0, 4, 9])
    for orient in ("mst", "outward", 1, True):
        with pytest.raises(SfmiError, match="orient must be"):
            S.estimate_normals_dev(p, None, 8, orient=orient)
        with pytest.raises(SfmiError, match="orient must be"):
            P.poisson_recon_dev(p, None, orient=orient)
    with pytest.raises(SfmiError, match="orient goes with normals=None"):
        P.poisson_recon_dev(p, n, orient="tangent")


def test_cpu_tensors_are_refused_last(no_library):
    p, n = torch.zeros(10, 3), torch.ones(10, 3)
    calls = (lambda: S.orient_normals_dev(p, n), lambda: S.orient_normals_dev(p[None], n[None], k=4, details=True),
             lambda: S.orient_normals_dev(p, n, [0, 4, 10], anchor="viewpoint", viewpoint=np.zeros((2, 3))),
             lambda: S.orient_normals_dev(p, n, idx=torch.zeros(10, 4, dtype=torch.int32)),
             lambda: S.estimate_normals_dev(p, None, 8, orient="tangent"),
             lambda: S.estimate_normals_dev(p, None, 8, viewpoint=(0, 0, 1.0), orient="tangent"),
             lambda: P.poisson_recon_dev(p, None, orient="tangent", knn=10, grid_dim=17),
             lambda: P.poisson_recon_dev(p, None, orient="tangent", viewpoint=(0, 0, 2.0)))
    for call in calls:
        with pytest.raises(SfmiError, match="HIP device.*no CPU fallback"):
            call()


def test_the_viewpoint_errors_stand(no_library, tmp_path):
    p = torch.zeros(10, 3)
    with pytest.raises(SfmiError, match="needs a viewpoint"):
        P.poisson_recon_dev(p, None)
    with pytest.raises(SfmiError, match="needs a viewpoint"):
        P.poisson_recon_dev(p, None, knn=10, quantile=0.3, orient=None)
    with pytest.raises(SfmiError, match="needs a viewpoint"):
        P.Open3D_Toolbox().poisson_recon(np.zeros((10, 3)))
    # make_dataset: without the flag a cloud without normals is refused as before; the flag belongs to the poisson route
    from shapeformer_amd import meshio
    path = str(tmp_path / "bare.ply")
    meshio.write_ply(path, np.random.default_rng(0).random((20, 3)), np.zeros((0, 3), np.int64))
    with pytest.raises(ValueError, match="the cloud has no normals"):
        MD.make_dataset([path], str(tmp_path / "out"), "d", grid=8, boundary_n=16, occupancy="poisson", device="cpu")
    with pytest.raises(ValueError, match="goes with occupancy = 'poisson'"):
        MD.make_dataset([path], str(tmp_path / "out"), "d", grid=8, boundary_n=16, orient="tangent", device="cpu")
    with pytest.raises(ValueError, match="must be None or 'tangent'"):
        MD.make_dataset([path], str(tmp_path / "out"), "d", grid=8, boundary_n=16, occupancy="poisson", orient="mst", device="cpu")
    assert MD.parse_args([path, "--out", "o", "--dataset", "d", "--occupancy", "poisson", "--orient", "tangent"]).orient == "tangent"
    assert MD.parse_args([path, "--out", "o", "--dataset", "d"]).orient is None
    for bad in (["--orient", "tangent"], ["--occupancy", "poisson", "--orient", "mst"]):
        with pytest.raises(SystemExit):
            MD.parse_args([path, "--out", "o", "--dataset", "d"] + bad)
