"""Plane removal and Euclidean clustering: the numpy reference against hand-made cases, and everything of
shapeformer_amd.scan that runs on the host - the hypothesis draws, the upright rotation, the argument refusals.  No GPU."""
import numpy as np
import pytest
import torch

import segment_ref as R
from shapeformer_amd import scan
from shapeformer_amd._lib import SfmiError


def _grid_cloud():
    """a 5 x 5 lattice on z = 0 (indices 0..24) and points above it at z = 0.005, 0.01, 0.0100001, 0.02, -0.01, -0.03"""
    g = np.stack(np.meshgrid(np.arange(5.), np.arange(5.), indexing="ij"), -1).reshape(-1, 2)
    flat = np.concatenate([g, np.zeros((25, 1))], 1)
    extra = np.array([[0.5, 0.5, z] for z in (0.005, 0.01, 0.0100001, 0.02, -0.01, -0.03)])
    return np.concatenate([flat, extra]).astype(np.float32)


def test_reference_counts_the_points_within_the_threshold():
    p = _grid_cloud()
    thr = 0.01
    expect = int((np.abs(p[:, 2].astype(np.float64)) <= thr).sum())
    assert expect == 25 + 3                                     # 0.005 and +-0.01 (f32(0.01) is below 0.01); f32(0.0100001) is above
    count, best, status = R.plane_score_set(p, np.array([[0, 1, 5], [0, 6, 23], [3, 20, 9]]), thr)
    assert count.tolist() == [expect] * 3 and best == 0 and status == 0       # ties go to the lower h


def test_reference_invalid_hypotheses_and_status():
    p = _grid_cloud()
    tr = np.array([[0, 1, 2],        # collinear
                   [0, 0, 5],        # repeated
                   [0, 1, 31],       # out of range
                   [-1, 1, 5],       # negative
                   [0, 1, 5]])
    count, best, status = R.plane_score_set(p, tr, 0.01)
    assert count[:4].tolist() == [-1] * 4 and count[4] > 0 and best == 4 and status == 0
    count, best, status = R.plane_score_set(p, tr[:4], 0.01)
    assert count.tolist() == [-1] * 4 and best == -1 and status == 1
    for n in (0, 1, 2):
        count, best, status = R.plane_score_set(p[:n], np.array([[0, 1, 2], [0, 1, 1]]), 0.01)
        assert count.tolist() == [-1, -1] and best == -1 and status == 1
    q = p.copy()
    q[7, 1] = np.nan
    count, best, status = R.plane_score_set(q, tr, 0.01)
    assert count.tolist() == [-1] * 5 and best == -1 and status == 2


def test_reference_ties_go_to_the_lower_h():
    p = _grid_cloud()
    tr = np.array([[0, 1, 25], [0, 1, 5], [0, 6, 23], [0, 1, 5]])             # h = 0 tilts out of the lattice: fewer inliers
    count, best, _ = R.plane_score_set(p, tr, 0.01)
    assert count[0] < count[1] == count[2] == count[3] and best == 1


def test_reference_refit_and_clusters_by_hand():
    p = _grid_cloud()
    plane, mask, n_in, dist, gap = R.plane_refit_set(p, [0, 1, 5], 0.01)
    assert abs(plane[2] - 1) < 1e-4 and plane[2] > 0 and abs(plane[3]) < 1e-2 and n_in == mask.sum() >= 25
    assert R.plane_refit_set(p, [0, 1, 5], 0.01, up=(0, 0, -1))[0][2] < 0
    assert np.isnan(R.plane_refit_set(p, [0, 1, 2], 0.01)[0]).all()
    q = np.array([[0, 0, 0], [0.5, 0, 0], [2, 0, 0], [2, 0.4, 0], [1.0, 0, 0], [9, 9, 9]], np.float32)
    root = R.cluster_roots(q, 0.5)
    assert root.tolist() == [0, 0, 2, 2, 0, 5]
    label, sizes = R.cluster_labels(root)
    assert label.tolist() == [0, 0, 1, 1, 0, 2] and sizes.tolist() == [3, 2, 1]
    label, sizes = R.cluster_labels(root, min_points=2)
    assert label.tolist() == [0, 0, 1, 1, 0, -1] and sizes.tolist() == [3, 2]
    q[3, 0] = np.nan
    assert R.cluster_roots(q, 0.5).tolist() == [0, 0, 2, 3, 0, 5]             # a NaN point joins nothing


def test_plane_hypotheses_match_the_reference_and_ignore_b():
    sizes = [4100, 7, 4100, 1, 0, 3]
    for seed in (0, 1, 12345):
        t = scan.plane_hypotheses(sizes, 65, seed)
        assert t.dtype == np.int32 and t.shape == (6, 65, 3)
        assert np.array_equal(t, R.plane_hypotheses(sizes, 65, seed))
        assert np.array_equal(t[0], t[2])                                     # a function of (seed, h, slot, n), not of b
        for b, n in enumerate(sizes):
            assert np.array_equal(t[b], scan.plane_hypotheses([n], 65, seed)[0])
            assert (t[b] >= 0).all() and (t[b] < max(n, 1)).all()
    assert not np.array_equal(scan.plane_hypotheses([4100], 65, 0), scan.plane_hypotheses([4100], 65, 1))
    assert np.array_equal(scan.plane_hypotheses([4100], 65, 0)[:, :10], scan.plane_hypotheses([4100], 10, 0))


@pytest.mark.parametrize("up", [(0, 1, 0), (0, 0, 1), (1, 2, -2)])
def test_upright_rotation(up):
    rng = np.random.default_rng(0)
    n = rng.normal(size=(16, 3))
    u = np.asarray(up, np.float64) / np.linalg.norm(up)
    n[0] = -u * 3                                                             # the antiparallel case
    n[1] = u * 0.5
    Rm = scan.upright_rotation(n, up)
    assert Rm.shape == (16, 3, 3) and Rm.dtype == np.float64
    unit = n / np.linalg.norm(n, axis=1, keepdims=True)
    for k in range(16):
        assert np.abs(Rm[k] @ Rm[k].T - np.eye(3)).max() < 1e-14
        assert abs(np.linalg.det(Rm[k]) - 1) < 1e-14
        assert np.abs(Rm[k] @ unit[k] - u).max() < 1e-14
        assert np.abs(Rm[k] - R.upright_rotation(n[k], up)).max() < 1e-14
    Rt = scan.upright_rotation(torch.from_numpy(n), up)
    assert isinstance(Rt, torch.Tensor) and np.abs(Rt.numpy() - Rm).max() < 1e-15
    assert scan.upright_rotation(n[3], up).shape == (1, 3, 3)


def test_upright_rotation_antiparallel_axis():
    assert np.array_equal(scan.upright_rotation([0, -1, 0], (0, 1, 0))[0], np.diag([1., -1., -1.]))     # about x
    assert np.array_equal(scan.upright_rotation([-1, 0, 0], (1, 0, 0))[0], np.diag([-1., 1., -1.]))     # x is parallel to up: about y


def test_host_side_refusals():
    p = torch.zeros(10, 3)                                                    # a CPU tensor: every refusal below comes before the device check
    for h in (0, -1, 1.5, True):
        with pytest.raises(SfmiError, match="hypotheses"):
            scan.segment_plane_dev(p, hypotheses=h)
    for thr in (-0.01, float("nan"), float("inf"), None):
        with pytest.raises(SfmiError, match="threshold"):
            scan.segment_plane_dev(p, threshold=thr)
        with pytest.raises(SfmiError, match="threshold"):
            scan.remove_planes_dev(p, threshold=thr)
    for tr in (np.zeros((1, 4, 2), np.int32), np.zeros((2, 4, 3), np.int32), np.zeros((4, 3), np.int32), np.zeros((1, 0, 3), np.int32),
               np.zeros((1, 4, 3), np.float32)):
        with pytest.raises(SfmiError, match="triples"):
            scan.segment_plane_dev(p, triples=tr)
    with pytest.raises(SfmiError, match="up"):
        scan.segment_plane_dev(p, up=np.zeros((2, 3)))
    for plane in (None, np.zeros(3), np.zeros((2, 4))):
        with pytest.raises(SfmiError, match="plane must be"):
            scan.refit_plane_dev(p, None, plane)
    with pytest.raises(SfmiError, match="no CPU fallback"):
        scan.refit_plane_dev(p, None, [0, 1, 0, 0.4])
    for r in (-1.0, float("nan"), None):
        with pytest.raises(SfmiError, match="radius"):
            scan.euclidean_clusters_dev(p, radius=r)
        with pytest.raises(SfmiError, match="radius"):
            scan.largest_cluster_mask_dev(p, radius=r)
        with pytest.raises(SfmiError, match="cluster_radius"):
            scan.isolate_object_dev(p, cluster_radius=r)
    with pytest.raises(SfmiError, match="min_points"):
        scan.euclidean_clusters_dev(p, radius=0.1, min_points=0)
    with pytest.raises(SfmiError, match="max_planes"):
        scan.remove_planes_dev(p, max_planes=0)
    with pytest.raises(SfmiError, match="min_ratio"):
        scan.remove_planes_dev(p, min_ratio=-0.5)
    with pytest.raises(SfmiError, match="normalize"):
        scan.isolate_object_dev(p, normalize="unit")
    with pytest.raises(SfmiError, match="remove_planes"):
        scan.clean_cloud_dev(torch.zeros(1, 10, 3), remove_planes=0.01)
    with pytest.raises(SfmiError, match="no CPU fallback"):                   # all arguments fine: the device check is the last one
        scan.segment_plane_dev(p)
    with pytest.raises(SfmiError, match="no CPU fallback"):
        scan.euclidean_clusters_dev(p, radius=0.1)
