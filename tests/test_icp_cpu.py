"""Iterative closest point: the numpy reference against scenes with a known motion, its Rodrigues formula against
scipy, the host-side refusals of shapeformer_amd.registration, and the C entry points the header declares.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

import icp_ref as R
from shapeformer_amd import _lib, registration as G
from shapeformer_amd._lib import SfmiError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("metric,seed,deg,max_dist", [("point", 0, 5, 0.05), ("plane", 0, 5, 0.05), ("point", 2, 15, 0.1), ("plane", 1, 10, 0.05)])
def test_reference_recovers_scene_S(metric, seed, deg, max_dist):
    s = R.scene("S", seed, deg)
    pose, fitness, rmse, it, status = R.icp(s["src"], s["tgt"], max_dist, metric, s["nrm"])
    eR, et = R.pose_error(pose, s["R"], s["t"])
    assert status == 0 and 0 < it < 30 and fitness == 1.0 and rmse < 5e-8
    assert eR <= 1e-8 and et <= 1e-8                           # the source is the target's subset moved and rounded to f32


def test_reference_loop_edges():
    s = R.scene("S", 0, 5)
    pose, fitness, rmse, it, status = R.icp(s["src"], s["tgt"], 0.05, max_iter=0)
    e = R.evaluate(s["src"], s["tgt"], None, R.IDENTITY, 0.05)
    assert status == 1 and it == 0 and np.array_equal(pose, R.IDENTITY) and fitness == e["fitness"] and rmse == e["rmse"]
    assert R.icp(s["src"][:0], s["tgt"], 0.05)[4] == 2 and R.icp(s["src"], s["tgt"][:0], 0.05)[4] == 2
    assert R.icp(s["src"] + 10, s["tgt"], 0.05)[4] == 2        # nothing within max_dist
    g = np.stack(np.meshgrid(np.arange(4.), np.arange(4.), [0.0], indexing="ij"), -1).reshape(-1, 3).astype(np.float32) / 4
    pose, _, _, _, status = R.icp(g + np.float32([0, 0, 0.125]), g, 1.0, "plane", np.tile(np.float32([0, 0, 1]), (16, 1)))
    assert status == 3 and np.array_equal(pose, R.IDENTITY)    # a coplanar target: three columns of J vanish
    bad = s["src"].copy()
    bad[3, 1] = np.nan
    assert R.icp(bad, s["tgt"], 0.05)[1:] == (0.0, 0.0, 0, 4)


def test_rodrigues_against_scipy():
    from scipy.spatial.transform import Rotation
    rs = np.random.RandomState(0)
    for scale in (0.0, 1e-9, 5e-5, 0.99e-4, 1.01e-4, 1e-2, 1.0, 3.0):
        for _ in range(4):
            w = rs.randn(3) * scale
            M = R.rodrigues(w)
            assert np.abs(M - Rotation.from_rotvec(w).as_matrix()).max() < 1e-15
            assert np.abs(M @ M.T - np.eye(3)).max() < 1e-15


def test_transform_statement_by_hand():
    p = np.float32([[1, 2, 3], [0.5, -0.25, 4]])
    pose = R.pose12([[0, -1, 0], [1, 0, 0], [0, 0, 1]], [0.5, 0.25, -1])
    assert np.array_equal(R.transform(p, pose), np.float32([[-1.5, 1.25, 2], [0.75, 0.75, 3]]))
    assert np.array_equal(R.transform(p, R.IDENTITY), p)


def test_nn_statement_ties_and_empty():
    q = np.float32([[1, 0, 0], [0, 1, 0], [1, 0, 0], [-1, 0, 0]])
    idx, d2 = R.nn(np.float32([[0, 0, 0], [1, 0, 0.5]]), q)
    assert idx.tolist() == [0, 0] and d2.tolist() == [1.0, 0.25]          # the lowest index among equal distances
    idx, d2 = R.nn(np.float32([[0, 0, 0]]), q[:0])
    assert idx.tolist() == [-1] and np.isinf(d2).all()


def test_host_side_refusals():
    p, q = torch.zeros(10, 3), torch.zeros(12, 3)              # CPU tensors: every refusal below comes before the device check
    for md in (None, -1.0, float("nan"), float("inf"), True, [0.1, 0.2]):
        with pytest.raises(SfmiError, match="max_dist"):
            G.icp_dev(p, q, max_dist=md)
    for m in ("colour", None, 1, ["point", "plane"]):
        with pytest.raises(SfmiError, match="metric"):
            G.icp_dev(p, q, max_dist=0.1, metric=m)
    with pytest.raises(SfmiError, match="target_normals"):
        G.icp_dev(p, q, max_dist=0.1, metric="plane")
    with pytest.raises(SfmiError, match="target_normals"):
        G.icp_dev(p, q, max_dist=0.1, metric="plane", target_normals=torch.zeros(11, 3))
    with pytest.raises(SfmiError, match="target_normals"):
        G.icp_dev(p, q, max_dist=0.1, target_normals=torch.zeros(12, 3))
    for init in (np.zeros((3, 3)), np.zeros((2, 4, 4)), np.zeros(11)):
        with pytest.raises(SfmiError, match="init"):
            G.icp_dev(p, q, max_dist=0.1, init=init)
    for mi in (-1, 1.5, True):
        with pytest.raises(SfmiError, match="max_iter"):
            G.icp_dev(p, q, max_dist=0.1, max_iter=mi)
    for ce in (0, -3, 2.0):
        with pytest.raises(SfmiError, match="check_every"):
            G.icp_dev(p, q, max_dist=0.1, check_every=ce)
    with pytest.raises(SfmiError, match="rel_rmse"):
        G.icp_dev(p, q, max_dist=0.1, rel_rmse=-1e-6)
    with pytest.raises(SfmiError, match="rel_fitness"):
        G.icp_dev(p, q, max_dist=0.1, rel_fitness=float("nan"))
    with pytest.raises(SfmiError, match="sets"):
        G.icp_dev(p, q, [0, 4, 10], [0, 12], max_dist=0.1)
    with pytest.raises(SfmiError, match="offsets"):
        G.icp_dev(p, q, [0, 4, 11], [0, 6, 12], max_dist=0.1)
    with pytest.raises(SfmiError, match="batched"):
        G.icp_dev(torch.zeros(2, 5, 3), q, max_dist=0.1)
    with pytest.raises(SfmiError, match="pose"):
        G.transform_points_dev(p, None, np.zeros((2, 4, 4)))
    with pytest.raises(SfmiError, match="pose"):
        G.evaluate_registration_dev(p, q, max_dist=0.1, pose=np.zeros(5))
    with pytest.raises(SfmiError, match="voxels"):
        G.icp_multiscale_dev(p, q, voxels=())
    with pytest.raises(SfmiError, match="voxels"):
        G.icp_multiscale_dev(p, q, voxels=(0.02, -0.01))
    with pytest.raises(SfmiError, match="max_dists"):
        G.icp_multiscale_dev(p, q, voxels=(0.02, 0.01), max_dists=(0.04,))
    with pytest.raises(SfmiError, match="merge_scans_dev"):
        G.merge_scans_dev([])
    with pytest.raises(SfmiError, match="offsets"):
        G.merge_scans_dev([p, q], offs=[0, 10, 22])
    with pytest.raises(SfmiError, match="voxel"):
        G.merge_scans_dev([p, q], voxel=0.0, max_dist=0.1)
    for call in (lambda: G.icp_dev(p, q, max_dist=0.1), lambda: G.transform_points_dev(p, None, np.eye(4)),
                 lambda: G.evaluate_registration_dev(p, q, max_dist=0.1), lambda: G.icp_multiscale_dev(p, q),
                 lambda: G.merge_scans_dev([p, q], max_dist=0.1)):
        with pytest.raises(SfmiError, match="no CPU fallback"):                   # all arguments fine: the device check is the last one
            call()


def test_library_exports_every_icp_entry_of_the_header():
    names = sorted(set(re.findall(r"\b(sfmi_icp_\w+)\s*\(", open(os.path.join(ROOT, "include", "sfmi.h")).read())))
    assert len(names) >= 6 and "sfmi_icp_iterate_f32" in names and "sfmi_icp_transform_f32" in names
    lib = _lib.lib()
    for n in names:
        assert hasattr(lib, n), f"libsfmi.so does not export {n}"
        assert n in _lib.PROTOTYPES, f"_lib.PROTOTYPES does not bind {n}"
    assert sorted(n for n in _lib.PROTOTYPES if n.startswith("sfmi_icp_")) == names
