"""CPU tests of the k-nearest-neighbour front end (shapeformer_amd/scan.py, csrc/knn.hip): the C-ABI surface, the
workspace rule, every host-side refusal (raised before the library is loaded), the four scan normalisations of the reference written
out, the raw-scan dataset under its four dotted names, and the point readers."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from shapeformer_amd import _lib as L
from shapeformer_amd import data as D
from shapeformer_amd import meshio, scan
from shapeformer_amd._lib import SfmiError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("sfmi_knn_workspace_bytes", "sfmi_knn_f32", "sfmi_knn_mean_dist_f64", "sfmi_knn_normals_f32")


@pytest.fixture()
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(L, "lib", refuse)


def test_symbols_are_exported_declared_and_bound():
    for name in ("knn_dev", "knn_mean_dist_dev", "statistical_outlier_mask_dev", "radius_outlier_mask_dev", "estimate_normals_dev",
                 "normalize_scan", "clean_cloud_dev"):
        assert callable(getattr(scan, name))
    hdr = open(os.path.join(ROOT, "include", "sfmi.h")).read()
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in L.PROTOTYPES
    assert len(L.PROTOTYPES["sfmi_knn_f32"][1]) == 13 and len(L.PROTOTYPES["sfmi_knn_normals_f32"][1]) == 10
    assert callable(meshio.read_points) and inspect.isclass(D.ScanDataset)
    from shapeformer_amd import callbacks as CB
    assert inspect.signature(CB.VisShapeFormer.__init__).parameters["clean_context"].default is None
    assert CB.VisShapeFormer(end_tokens=(4096, 4096)).clean_context is None
    with pytest.raises(ValueError, match="clean_context"):
        CB.VisShapeFormer(end_tokens=(4096, 4096), clean_context={"out_N": 5})


def test_workspace_bytes():
    """pure host arithmetic of the built library: finite for N = 0, larger than the result on a split shape and growing with k there,
    and no partial lists where the query blocks alone fill the chip"""
    from shapeformer_amd import build as B
    B.build(verbose=False)
    lib = ctypes.CDLL(L.LIB_PATH)
    f = lib.sfmi_knn_workspace_bytes
    f.restype, f.argtypes = L.PROTOTYPES["sfmi_knn_workspace_bytes"]
    assert 0 < f(1, 0, 0, 8) < 4096 and 0 < f(3, 0, 100, 64) < 4096
    split = [f(1, 100, 40000, k) for k in (8, 16, 32, 64)]
    assert all(a < b for a, b in zip(split, split[1:]))
    for k, w in zip((8, 16, 32, 64), split):
        assert w > 100 * k * 8
    assert f(1, 100, 40000, 9) == split[1] and f(1, 100, 40000, 33) == split[3]            # the instance that serves k
    assert f(64, 64 * 16384, 64 * 16384, 16) < 4096                                          # 4160 query blocks: no split
    assert f(1, 100, 100, 0) == 0 and f(1, 100, 100, 65) == 0 and f(0, 1, 1, 8) == 0 and f(1, -1, 1, 8) == 0


@pytest.mark.parametrize("k", [0, -1, 65, 1000, 2.0, "8", None, True])
def test_k_out_of_range(no_library, k):
    p = torch.zeros(10, 3)
    with pytest.raises(SfmiError, match=r"k must be an integer in \[1, 64\]"):
        scan.knn_dev(p, p, k)
    with pytest.raises(SfmiError, match=r"k must be"):
        scan.knn_mean_dist_dev(p, None, k)
    with pytest.raises(SfmiError, match=r"k must be"):
        scan.statistical_outlier_mask_dev(p, None, k)
    with pytest.raises(SfmiError, match=r"k must be"):
        scan.radius_outlier_mask_dev(p, None, 0.1, k)
    with pytest.raises(SfmiError, match=r"k must be"):
        scan.estimate_normals_dev(p, None, k)
    with pytest.raises(SfmiError, match=r"k must be"):
        scan.clean_cloud_dev(p[None], k=k)


def test_points_dist_k_range(no_library):
    from shapeformer_amd import metrics as M
    p = torch.zeros(10, 3)
    for k in (0, 65):
        with pytest.raises(SfmiError, match="k must be"):
            M.points_dist(p, p, k)


def test_knn_dev_refusals(no_library):
    p, q = torch.zeros(10, 3), torch.zeros(12, 3)
    with pytest.raises(SfmiError, match="exclude_self"):                                     # unequal sizes
        scan.knn_dev(p, q, 4, exclude_self=True)
    with pytest.raises(SfmiError, match="exclude_self"):                                     # equal sizes, unequal sets
        scan.knn_dev(p, p, 4, [0, 4, 10], [0, 5, 10], exclude_self=True)
    with pytest.raises(SfmiError, match="exclude_self"):
        scan.knn_dev(torch.zeros(2, 5, 3), torch.zeros(2, 6, 3), 4, exclude_self=True)
    with pytest.raises(SfmiError, match="reference set is empty"):
        scan.knn_dev(p, q, 4, [0, 4, 10], [0, 0, 12])
    with pytest.raises(SfmiError, match="reference set is empty"):
        scan.knn_dev(p, q[:0], 4)
    with pytest.raises(SfmiError, match="reference set is empty"):
        scan.knn_dev(torch.zeros(2, 5, 3), torch.zeros(2, 0, 3), 4)
    with pytest.raises(SfmiError, match="integer"):                                          # float offsets
        scan.knn_dev(p, q, 4, [0.0, 4.0, 10.0], [0, 6, 12])
    with pytest.raises(SfmiError, match="q_off.*integer"):
        scan.knn_dev(p, q, 4, [0, 4, 10], torch.tensor([0.0, 6.0, 12.0]))
    with pytest.raises(SfmiError, match="end at 12"):
        scan.knn_dev(p, q, 4, [0, 4, 10], [0, 6, 11])
    with pytest.raises(SfmiError, match="p has 2 sets, q has 1"):
        scan.knn_dev(p, q, 4, [0, 4, 10], None)
    with pytest.raises(SfmiError, match="same B and no offsets"):
        scan.knn_dev(torch.zeros(2, 5, 3), torch.zeros(3, 5, 3), 4)
    with pytest.raises(SfmiError, match="same B and no offsets"):
        scan.knn_dev(torch.zeros(2, 5, 3), torch.zeros(2, 5, 3), 4, p_off=[0, 5, 10])
    with pytest.raises(SfmiError, match=r"needs an \(M,3\) q"):
        scan.knn_dev(p, torch.zeros(2, 6, 3), 4)
    for bad, word in ((np.zeros((5, 3)), "torch tensor"), (torch.zeros(5, 2), r"\(N,3\)")):
        with pytest.raises(SfmiError, match=word):
            scan.knn_dev(bad, q, 4)
        with pytest.raises(SfmiError, match=word):
            scan.knn_dev(p, bad, 4)
    # where the tensors live is reported last: valid arguments on the CPU
    for call in (lambda: scan.knn_dev(p, q, 4), lambda: scan.knn_dev(p, p, 4, exclude_self=True),
                 lambda: scan.knn_dev(torch.zeros(2, 5, 3), torch.zeros(2, 6, 3), 64),
                 lambda: scan.knn_mean_dist_dev(p, [0, 4, 10], 3), lambda: scan.statistical_outlier_mask_dev(p),
                 lambda: scan.radius_outlier_mask_dev(p, None, 0.1, 2), lambda: scan.estimate_normals_dev(p, viewpoint=[0, 0, 0]),
                 lambda: scan.clean_cloud_dev(p[None])):
        with pytest.raises(SfmiError, match="HIP device.*no CPU fallback"):
            call()


def test_front_end_refusals(no_library):
    p = torch.zeros(10, 3)
    with pytest.raises(SfmiError, match="integer"):
        scan.statistical_outlier_mask_dev(p, [0.0, 10.0])
    with pytest.raises(SfmiError, match="offsets go with"):
        scan.statistical_outlier_mask_dev(p[None], [0, 10])
    with pytest.raises(SfmiError, match="radius must be >= 0"):
        scan.radius_outlier_mask_dev(p, None, -1.0, 2)
    with pytest.raises(SfmiError, match="radius must be >= 0"):
        scan.radius_outlier_mask_dev(p, None, float("nan"), 2)
    with pytest.raises(SfmiError, match=r"expected \(2,3\) viewpoints"):
        scan.estimate_normals_dev(p, [0, 4, 10], 8, viewpoint=np.zeros(3))
    with pytest.raises(SfmiError, match=r"\(B,N,3\)"):
        scan.clean_cloud_dev(p)
    with pytest.raises(SfmiError, match="out_N"):
        scan.clean_cloud_dev(p[None], out_N=-1)
    with pytest.raises(SfmiError, match="mode must be one of"):
        scan.normalize_scan(np.zeros((4, 3)), "unit_sphere", 1.0)


def _cloud(seed=0, n=500, cols=3):
    rs = np.random.RandomState(seed)
    return rs.randn(n, cols) * np.array([3.0, 0.5, 1.5] + [1.0] * (cols - 3)) + np.array([10.0, -4.0, 2.5] + [0.0] * (cols - 3))


def test_normalize_scan_is_the_four_reference_recipes():
    raw = _cloud(cols=6)                                    # as np.loadtxt returns a .pts with normals: f64, six columns
    # redwood.py:53-58 (Redwood, 0.7) and realtest.py:55-62 (RealTest_dataset, 0.8)
    for s in (0.7, 0.8):
        points = raw[:, :3].astype(np.float32)
        points[:, 0] -= np.mean(points[:, 0])
        points[:, 1] -= np.mean(points[:, 1])
        points[:, 2] -= np.mean(points[:, 2])
        points /= points.max()
        points = points * s
        got = scan.normalize_scan(raw, "mean_max", s)
        assert got.dtype == np.float32 and got.shape == (500, 3) and np.array_equal(got, points)
    # redwood.py:99-102 (Redwood2, 0.9) and realtest.py:105-109 (RealTest2_dataset, 0.85)
    for s in (0.9, 0.85):
        points = raw[:, :3].astype(np.float32)
        points -= (points.max(axis=0) + points.min(axis=0)) / 2
        points /= np.abs(points).max()
        points = points * s
        got = scan.normalize_scan(raw, "bbox", s)
        assert got.dtype == np.float32 and np.array_equal(got, points)
        assert np.isclose(np.abs(got).max(), s, rtol=1e-6)
    assert raw.dtype == np.float64 and np.array_equal(raw, _cloud(cols=6))                 # the input is not written to
    # torch in, torch out: the same recipe in torch's f32 (its mean sums in another order than numpy's: a few ulps)
    for mode, s in (("mean_max", 0.7), ("bbox", 0.9)):
        t = scan.normalize_scan(torch.from_numpy(raw), mode, s)
        assert isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.shape == (500, 3)
        assert np.allclose(t.numpy(), scan.normalize_scan(raw, mode, s), rtol=0, atol=1e-6)


def test_read_points_round_trips(tmp_path):
    raw = _cloud(cols=6)
    np.savetxt(tmp_path / "a.pts", raw)
    np.savetxt(tmp_path / "a.xyz", raw[:, :3])
    np.save(tmp_path / "a.npy", raw.astype(np.float32))
    meshio.write_ply(str(tmp_path / "a.ply"), raw[:, :3], np.zeros((0, 3), np.int32))
    np.savetxt(tmp_path / "one.pts", raw[:1])
    for name, want in (("a.pts", raw[:, :3]), ("a.xyz", raw[:, :3]), ("a.npy", raw[:, :3].astype(np.float32)), ("a.ply", raw[:, :3]),
                       ("one.pts", raw[:1, :3])):
        got = meshio.read_points(str(tmp_path / name))
        assert got.dtype == np.float64 and got.shape == want.shape and np.array_equal(got, want.astype(np.float64))
    assert np.array_equal(meshio.read_points(str(tmp_path / "a.pts")), np.loadtxt(tmp_path / "a.pts")[:, :3])
    np.savetxt(tmp_path / "flat.pts", raw[:, :2])
    with pytest.raises(ValueError, match="three coordinates"):
        meshio.read_points(str(tmp_path / "flat.pts"))
    with pytest.raises(ValueError, match="unknown point format"):
        meshio.read_points(str(tmp_path / "a.obj"))


NAMES = {"shapeformer.data.imnet_datasets.redwood.Redwood": ("mean_max", 0.7),
         "shapeformer.data.imnet_datasets.redwood.Redwood2": ("bbox", 0.9),
         "shapeformer.data.imnet_datasets.realtest.RealTest_dataset": ("mean_max", 0.8),
         "shapeformer.data.imnet_datasets.realtest.RealTest2_dataset": ("bbox", 0.85)}


@pytest.fixture()
def scans(tmp_path):
    clouds = {}
    for name, seed in (("b.pts", 1), ("a.pts", 2), ("c.pts", 3)):
        clouds[name] = _cloud(seed, n=300, cols=6)
        np.savetxt(tmp_path / name, clouds[name])
    np.savetxt(tmp_path / "ignored.xyz", clouds["a.pts"])
    return tmp_path, clouds


def test_scan_dataset(scans, monkeypatch):
    path, clouds = scans
    monkeypatch.setattr(torch.cuda, "is_available", lambda: (_ for _ in ()).throw(AssertionError("the dataset touched the device")))
    ds = D.ScanDataset(str(path), context_N=128)
    assert len(ds) == 3 and [os.path.basename(f) for f in ds.files] == ["a.pts", "b.pts", "c.pts"]          # sorted
    assert isinstance(ds.partial_selector, D.VirtualScanSelector)
    assert ds.partial_selector.radius == 10 and ds.partial_selector.context_N == 128
    for i, name in enumerate(("a.pts", "b.pts", "c.pts")):
        np.random.seed(5 + i)
        item = ds[i]
        want = scan.normalize_scan(np.loadtxt(path / name)[:, :3], "mean_max", 0.7)
        assert set(item) == {"Xbd", "Xct"} and item["Xbd"].dtype == np.float32 and np.array_equal(item["Xbd"], want)
        np.random.seed(5 + i)
        assert np.array_equal(item["Xct"], D.VirtualScanSelector(radius=10, context_N=128)(want))
        assert item["Xct"].shape == (128, 3)
        rows = {r.tobytes() for r in want}
        assert all(r.tobytes() in rows for r in item["Xct"])                                                 # a partial view of Xbd
    # the selector and the file pattern are the caller's to replace
    ds = D.ScanDataset(str(path), pattern="*.xyz", normalize="bbox", scale=0.9,
                       partial_opt={"class": "shapeformer.data.partial.AllSelector", "kwargs": {}})
    assert len(ds) == 1 and np.array_equal(ds[0]["Xct"], ds[0]["Xbd"])
    assert np.array_equal(ds[0]["Xbd"], scan.normalize_scan(clouds["a.pts"], "bbox", 0.9))
    with pytest.raises(ValueError, match="normalize"):
        D.ScanDataset(str(path), normalize="unit")


@pytest.mark.parametrize("name", sorted(NAMES))
def test_scan_dataset_reference_names(scans, name):
    path, clouds = scans
    mode, scale = NAMES[name]
    # the reference's kwargs travel through: split / samples_per_cate / evalseed are accepted and unused
    ds = D.instantiate({"class": name, "kwargs": dict(scan_path=str(path), split="test", samples_per_cate=100, context_N=64, camR=5,
                                                      evalseed=314)})
    assert isinstance(ds, D.ScanDataset) and (ds.normalize, ds.scale) == (mode, scale) and len(ds) == 3
    assert ds.partial_selector.radius == 5 and ds.partial_selector.context_N == 64
    np.random.seed(0)
    item = ds[1]
    assert np.array_equal(item["Xbd"], scan.normalize_scan(clouds["b.pts"], mode, scale)) and item["Xct"].shape == (64, 3)
    assert np.isclose(item["Xbd"].max() if mode == "mean_max" else np.abs(item["Xbd"]).max(), scale, rtol=1e-6)
