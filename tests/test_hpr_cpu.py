"""Hidden-point removal, CPU side: the f64 restatement (tests/hpr_ref.py: hull-vertex membership as a 2-D linear program) against the
project's scipy path and the rows the real reference recorded, hpr's argument checks (they raise before any launch), and the
data-side opt-in: the default path is unchanged, partial="device" hands the stored cloud and an f64 camera to virtual_scan_dev."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hpr_ref as R   # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
G = np.load(os.path.join(GOLD, "data_side.npz"))


@pytest.mark.parametrize("name,seed", [("car", 0), ("armchair", 3)])
def test_restatement_equals_scipy_on_the_demo_clouds(name, seed):
    from shapeformer_amd import data as D
    X = np.load(os.path.join(GOLD, "demo_ds", name, "Xbd.npy"))
    np.random.seed(seed)
    cam = D.sample_sphere(1)[0] * 10
    vis = R.visible_mask(X, cam)
    assert R.rows_differing(X[vis], D.hidden_point_removal(X, cam)) == 0
    idx = np.nonzero(vis)[0]
    assert len(R.row_set(X[idx])) == len(idx)                     # one row per class of duplicate points


def test_restatement_equals_the_recorded_reference():
    X = G["cloud"]
    vis = R.visible_mask(X, G["hpr_cam"])
    assert R.rows_differing(X[vis], G["hpr"]) == 0


def test_argument_checks_raise_before_launch():
    from shapeformer_amd import hpr
    from shapeformer_amd._lib import SfmiError
    x = torch.zeros(2, 10, 3)
    with pytest.raises(SfmiError):                                # a CPU tensor: no fallback
        hpr.hidden_point_mask_dev(x, np.zeros((2, 3)))
    with pytest.raises(SfmiError):                                # one camera per shape
        hpr.hidden_point_mask_dev(x, np.zeros((3, 3)))
    with pytest.raises(SfmiError):
        hpr.hidden_point_mask_dev(x[0], np.zeros((2, 3)), off=np.array([0, 4, 11]))     # offsets do not end at N
    with pytest.raises(SfmiError):
        hpr.hidden_point_mask_dev(x[0], np.zeros((2, 3)), off=np.array([0, 7, 5, 10]))  # decreasing, and B mismatch
    with pytest.raises(SfmiError):
        hpr.hidden_point_mask_dev(x, np.zeros((2, 3)), off=np.array([0, 10, 20]))       # a batch takes no offsets
    with pytest.raises(SfmiError):
        hpr.hidden_point_mask_dev(torch.zeros(10, 2), np.zeros((1, 3)))
    with pytest.raises(SfmiError):
        hpr.virtual_scan_dev(x, 16)
    with pytest.raises(SfmiError):
        hpr.hidden_point_removal(np.zeros((10, 3)), np.ones(3), device="cpu")


def test_sample_cameras_depend_on_seed_and_shape_index_only():
    from shapeformer_amd import hpr
    c = hpr.sample_cameras(3, radius=2.5, seed=4)
    assert c.dtype == np.float64 and np.allclose(np.linalg.norm(c, axis=1), 2.5)
    assert np.array_equal(hpr.sample_cameras(1, radius=2.5, seed=4, shape0=2)[0], c[2])
    assert not np.array_equal(hpr.sample_cameras(3, radius=2.5, seed=5), c)


def _store(tmp_path, dtype=np.float64):
    rs = np.random.RandomState(0)
    d = tmp_path / "datasets" / "IMNet2_64" / "train"
    d.mkdir(parents=True)
    clouds = np.stack([G["cloud"][rs.choice(3000, 2000)] * s for s in (1.0, 0.8, 0.6)]).astype(dtype)
    np.save(d / "Xbd.npy", clouds)
    np.save(d / "Ytg.npy", np.packbits(rs.rand(3, 512) > 0.5, axis=-1))
    kw = dict(dataset="IMNet2_64", split="train", boundary_N=256, target_N=64, grid_dim=8, root=str(tmp_path / "datasets"), cate="all",
              partial_opt={"class": "shapeformer.data.partial.VirtualScanSelector", "kwargs": {"context_N": 128, "radius": 4, "noise": 0.01}})
    return clouds, {"class": "shapeformer.data.imnet_datasets.imnet_datasets.Imnet2LowResDataset", "kwargs": kw}


def test_default_batches_are_unchanged(tmp_path):
    from shapeformer_amd import data as D
    _, opt = _store(tmp_path)
    dm = D.DataModule(batch_size=2, num_workers=0, trainset_opt=opt, testset_opt=opt)
    dm.setup()
    np.random.seed(7)
    want = [dm.train_set[i] for i in range(3)]
    np.random.seed(7)
    got = list(dm.batches("train", "cpu"))
    np.random.seed(7)
    got_kw = list(dm.batches("train", "cpu", partial="host"))
    assert [b["Xct"].shape[0] for b in got] == [2, 1]
    for bs in (got, got_kw):
        for bi, b in enumerate(bs):
            assert set(b) == {"Xct", "Xbd", "Xtg", "Ytg"}
            for k, v in b.items():
                assert np.array_equal(v.numpy(), np.stack([want[2 * bi + j][k] for j in range(v.shape[0])]))
    # the selector's camera draw is the first draw of its call
    sel = dm.train_set.partial_selector
    np.random.seed(5)
    cam = sel.draw_camera()
    np.random.seed(5)
    assert np.array_equal(cam, D.sample_sphere(1)[0] * 4)
    assert dm.train_set.defer_partial is False
    with pytest.raises(ValueError):
        next(dm.batches("train", "cpu", partial="gpu"))


class _Recorder:
    def __init__(self):
        self.calls = []

    def __call__(self, X, context_N, radius=10, noise=0., seed=0, cams=None, off=None, shape0=0):
        self.calls.append(dict(X=X.clone(), context_N=context_N, radius=radius, noise=noise, seed=seed, cams=np.array(cams), shape0=shape0))
        return X[:, :context_N].float().contiguous(), cams, torch.full((X.shape[0],), context_N, dtype=torch.int32)


def test_partial_device_hands_stored_cloud_and_f64_camera_to_the_device_path(tmp_path, monkeypatch):
    from shapeformer_amd import data as D, hpr
    clouds, opt = _store(tmp_path)
    rec = _Recorder()
    monkeypatch.setattr(hpr, "virtual_scan_dev", rec)
    dm = D.DataModule(batch_size=2, num_workers=0, trainset_opt=opt, testset_opt=opt)
    dm.setup()
    np.random.seed(7)
    got = list(dm.batches("train", "cpu", partial="device", seed=9))
    assert len(got) == 2 and len(rec.calls) == 2 and dm.train_set.defer_partial is False
    item = 0
    for b, c in zip(got, rec.calls):
        assert set(b) == {"Xct", "Xbd", "Xtg", "Ytg"}                                  # no Xsrc, no cam
        assert b["Xct"].shape[1:] == (128, 3) and b["Xbd"].shape[1:] == (256, 3)
        assert c["context_N"] == 128 and c["noise"] == 0.01 and c["seed"] == 9 and c["shape0"] == item
        assert c["cams"].dtype == np.float64 and c["cams"].shape == (c["X"].shape[0], 3)
        assert np.allclose(np.linalg.norm(c["cams"], axis=1), 4, rtol=0, atol=1e-12)   # f64 cameras of norm `radius`
        assert not np.array_equal(c["cams"], c["cams"].astype(np.float32))             # and not rounded through f32
        for x in c["X"].numpy():                                                       # Xsrc: the stored cloud, whole, as f32
            assert x.shape == (2000, 3) and np.array_equal(x, clouds[item].astype(np.float32))
            item += 1
    # the cameras are the selector's numpy draws: the first one under the seed is the host path's first draw
    np.random.seed(7)
    assert np.array_equal(rec.calls[0]["cams"][0], D.sample_sphere(1)[0] * 4)
    # Xct_as_Xbd is honoured where Xct is made
    opt2 = {"class": opt["class"], "kwargs": dict(opt["kwargs"], Xct_as_Xbd=True)}
    dm2 = D.DataModule(batch_size=3, num_workers=0, trainset_opt=opt2, testset_opt=opt2)
    dm2.setup()
    b = next(dm2.batches("train", "cpu", partial="device"))
    assert b["Xbd"] is b["Xct"] and set(b) == {"Xct", "Xbd", "Xtg", "Ytg"}
    # a selector that is no virtual scan: an error, not a quiet host path
    opt3 = {"class": opt["class"], "kwargs": dict(opt["kwargs"], partial_opt=None)}
    dm3 = D.DataModule(batch_size=3, num_workers=0, trainset_opt=opt3, testset_opt=opt3)
    dm3.setup()
    with pytest.raises(ValueError):
        next(dm3.batches("train", "cpu", partial="device"))


def test_partial_device_through_a_transform_dataset_moves_the_camera_with_the_cloud(tmp_path, monkeypatch):
    from shapeformer_amd import data as D, hpr
    clouds, opt = _store(tmp_path)
    rec = _Recorder()
    monkeypatch.setattr(hpr, "virtual_scan_dev", rec)
    topt = {"class": "shapeformer.data.paper_datasets.transform_dataset.TransformDataset",
            "kwargs": dict(max_voxels=512, voxel_dim=16, mode=["rot_axis_y", "scale", "shift"], dset_opt=opt)}
    dm = D.DataModule(batch_size=3, num_workers=0, trainset_opt=topt, testset_opt=topt)
    dm.setup()
    np.random.seed(11)
    b = next(dm.batches("train", "cpu", partial="device"))
    assert set(b) == {"Xct", "Xbd", "Xtg", "Ytg"} and dm.train_set.dset.defer_partial is False
    c = rec.calls[0]
    assert c["cams"].dtype == np.float64
    for j in range(3):
        # recover the similarity y = s Q x + t from the stored cloud and what the stub received, then apply it to a camera of norm
        # `radius`: Q orthogonal, s > 0, and |Q^T (cam' - t) / s| = radius
        x, y = clouds[j], c["X"][j].numpy().astype(np.float64)
        xc, yc = x - x.mean(0), y - y.mean(0)
        s = np.sqrt((yc ** 2).sum() / (xc ** 2).sum())
        U, _, Vt = np.linalg.svd(yc.T @ xc)
        Q = U @ Vt
        t = y.mean(0) - s * Q @ x.mean(0)
        assert np.abs(s * x @ Q.T + t - y).max() < 1e-5 and abs(np.linalg.det(Q) - 1) < 1e-6
        cam0 = Q.T @ (c["cams"][j] - t) / s
        assert abs(np.linalg.norm(cam0) - 4) < 1e-4
