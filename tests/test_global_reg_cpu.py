"""Global registration by FPFH and RANSAC: the numpy reference against scenes with a known motion that ICP alone does
not recover, its exact fmaf against fractions, the pair feature by hand, the bin-edge cap of the test scenes, the host-side refusals
of shapeformer_amd.registration, and the C entry points the header declares.  No GPU.

The reference's own errors on the five scenes (|| R - R_true ||_F, max |t - t_true|), the yardstick of tests/test_global_reg_gpu.py:
  H (0, 90) 5.07e-3 / 9.2e-4   H (1, 170) 5.07e-3 / 8.1e-4   H (2, 60) 5.07e-3 / 7.5e-4   (219 correspondences, 100 inliers)
  S (0, 90) 2.70e-2 / 5.3e-3   S (1, 170) 2.70e-2 / 5.8e-3                                 (184 correspondences, 20 inliers)
icp_ref.icp (point metric, max_dist 0.05) from there ends 6.2e-4 from the truth with fitness 0.68 on H (the scene's fixed point) and
1.1e-9 with fitness 1 on S; from the identity it ends 1.93, 2.82, 0.22 (H) and 1.96, 2.82 (S) away."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import global_reg_ref as G
import icp_ref as R
from shapeformer_amd import _lib, registration as D, scan
from shapeformer_amd._lib import SfmiError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = [("H", 0, 90), ("H", 1, 170), ("H", 2, 60), ("S", 0, 90), ("S", 1, 170)]
# the reference's measured errors with room for another BLAS: (rotation, translation, ICP's end from there)
LIMITS = {"H": (1e-2, 2e-3, 1e-3), "S": (5e-2, 1e-2, 1e-8)}


@pytest.fixture(scope="module")
def refs():
    out = {}
    for key in SCENES:
        sc = R.scene(*key)
        out[key] = (sc, G.global_registration(sc["src"], sc["tgt"]))
    return out


@pytest.mark.parametrize("key", SCENES)
def test_reference_recovers_what_icp_alone_does_not(refs, key):
    sc, g = refs[key]
    eR, et = R.pose_error(g["pose"], sc["R"], sc["t"])
    pose, fitness, _, _, status = R.icp(sc["src"], sc["tgt"], 0.05, init=g["pose"])
    fR, ft = R.pose_error(pose, sc["R"], sc["t"])
    lone = R.icp(sc["src"], sc["tgt"], 0.05)
    lR, _ = R.pose_error(lone[0], sc["R"], sc["t"])
    print(key, "C", len(g["corr"]), "inliers", g["n_in"], "global", eR, et, "then icp", fR, ft, fitness, "icp alone", lR, lone[1])
    lim = LIMITS[key[0]]
    assert g["status"] == 0 and g["n_in"] >= 15 and eR <= lim[0] and et <= lim[1]
    assert status == 0 and fR <= lim[2] and fitness >= (1.0 if key[0] == "S" else 0.65)
    assert lR > 0.1                                            # what makes the feature necessary


@pytest.mark.parametrize("key", SCENES)
def test_bin_edge_cap(refs, key):
    """at most 1 % of the points of a test scene have a counted pair within 1e-9 of a bin edge of atan2's feature (the ends +-pi
    included): the only points whose counts may differ between two correct implementations"""
    ms, mt = refs[key][1]["marginal"]
    print(key, "marginal", ms.sum(), "of", len(ms), mt.sum(), "of", len(mt))
    assert ms.mean() <= 0.01 and mt.mean() <= 0.01


def test_bin_edge_cap_of_the_fpfh_inputs():
    """the same cap for the inputs of the exact SPFH tests on the device: the fixture cloud at every k and radius (one zero normal up to
    k = 32) and the ragged batch of small sets"""
    cloud = G.fixture_cloud()
    X, d2, idx = cloud[0], cloud[3], cloud[4]
    assert len(X) - len(np.unique(X, axis=0)) == 106
    for k, radius in G.FPFH_CASES:
        frac = G.marginal_fraction(X, G.fixture_normals(cloud, k), np.array([0, len(X)]), k, radius, (d2, idx))
        print("k", k, "radius", radius, "marginal fraction", frac)
        assert frac <= 0.01
    zero64 = G.marginal_fraction(X, cloud[2], np.array([0, len(X)]), 64, None, (d2, idx))
    assert zero64 > 0.01                                       # why k = 64 runs without the zero normal: 39 of 2048 points
    off = np.concatenate([[0], np.cumsum(G.RAGGED_SIZES)])
    for radius in G.RAGGED_RADII:
        assert G.marginal_fraction(X[:off[-1]], cloud[1][:off[-1]], off, G.RAGGED_K, radius) <= 0.01


def _round_f32(x):
    """a Fraction rounded to the nearest f32, ties to even, by integer arithmetic (normal range)"""
    if x == 0:
        return 0.0
    sign, x = (-1 if x < 0 else 1), abs(x)
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fraction(2) ** e > x:
        e -= 1
    q = x / Fraction(2) ** (e - 23)
    n = q.numerator // q.denominator
    rem = q - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2 == 1):
        n += 1
    return sign * float(Fraction(n) * Fraction(2) ** (e - 23))


def test_fmaf_is_exact():
    # a product just below a tie of the f32 grid at c: through f64 the sum rounds onto the tie, and the tie rounds the wrong way
    a, b, c = np.float32(0.25 * (1 + 2.0 ** -23)), np.float32(0.25 - 2.0 ** -25), np.float32(2.0 ** 20 + 2.0 ** -3)
    through = np.float32(np.float64(a) * np.float64(b) + np.float64(c))
    assert G.fmaf(a, b, c) == c and through != c
    # the mirror image: c - p lies just past the tie 2^20 + 2^-4, through f64 it sits on it and goes to the even neighbour 2^20
    assert G.fmaf(-a, b, c) == c and np.float32(np.float64(-a) * np.float64(b) + np.float64(c)) == np.float32(2.0 ** 20)
    rs = np.random.RandomState(0)
    n = 400
    a, b = rs.randn(n).astype(np.float32), rs.randn(n).astype(np.float32)
    c = (rs.randn(n) * 2.0 ** rs.randint(-30, 30, n)).astype(np.float32)
    # a quarter of the cases sit on a tie: c = r + half an ulp of the result's grid is not an f32, so put the half ulp into the product
    r = rs.randn(n // 4).astype(np.float32)
    half = (np.spacing(np.abs(r)) / 2).astype(np.float32)
    a[:n // 4], b[:n // 4], c[:n // 4] = half * np.float32(1 + 2.0 ** -23), np.float32(1 - 2.0 ** -23) * np.sign(r), r
    got = G.fmaf(a, b, c)
    for i in range(n):
        want = _round_f32(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i])))
        assert float(got[i]) == want, (i, a[i], b[i], c[i])
    d = rs.rand(5, 33).astype(np.float32) * 100
    chain = G.feature_d2(d[:2], d[2:])                         # the chain of 33 terms against fractions
    for i in range(2):
        for j in range(3):
            acc = Fraction(float(np.float32(d[i, 0] - d[2 + j, 0]) * np.float32(d[i, 0] - d[2 + j, 0])))
            for k in range(1, 33):
                t = Fraction(float(np.float32(d[i, k] - d[2 + j, k])))
                acc = Fraction(_round_f32(t * t + acc))
            assert float(chain[i, j]) == float(acc)


def test_pair_feature_by_hand():
    z, x = np.float32([0, 0, 1]), np.float32([1, 0, 0])
    o = np.float32([0, 0, 0])
    flat = G.pair_feature(o, z, x, z)                          # a flat patch: f0 = 0, f1 = 0, f2 = 0, the middle bins
    assert flat["ok"] and not flat["swap"] and flat["bins"].tolist() == [5, 5, 5] and flat["f"].tolist() == [0, 0, 0]
    n2 = np.float32([0.6, 0, 0.8])
    sw = G.pair_feature(o, z, x, n2)                           # a1 = 0, a2 = 0.6: the roles swap, f2 = -a2
    a2 = np.float64(n2[0])
    assert sw["ok"] and sw["swap"] and sw["f"][2] == -a2 and sw["bins"][2] == int(np.floor(11 * (1 - a2) * 0.5))
    # the swapped frame: dp = (-1, 0, 0), na = n2, nb = z; v = dp x na = (0, 0.8, 0), w = na x v = (-0.8, 0, 0.6)
    assert sw["f"][1] == 0 and sw["f"][0] == np.arctan2(np.float64(n2[0]), np.float64(n2[2]))
    tie = G.pair_feature(o, np.float32([0.6, 0, 0.8]), x, np.float32([-0.6, 0, 0.8]))
    assert tie["ok"] and not tie["swap"]                       # |a1| == |a2|: strict, no swap
    assert not G.pair_feature(o, z, o, z)["ok"]                # d = 0
    assert not G.pair_feature(o, x, x, x)["ok"]                # vn = 0: the normal along the line between the points
    zero = G.pair_feature(o, o, x, z)                          # a zero normal at p1: a1 = 0 < a2 = 0 is false, v = dp x 0 = 0
    assert not zero["ok"]
    p = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 0, 0]])        # a duplicate is a neighbour by index and skipped by d > 0
    nrm = np.tile(z, (4, 1))
    d2, idx = G.knn(p, 3)
    assert idx[1].tolist() == [3, 0, 2] and d2[1].tolist() == [0, 1, 2] and idx[3].tolist() == [1, 0, 2]
    counts, m, marg = G.spfh(p, nrm, idx, d2)
    assert m.tolist() == [3, 2, 3, 2] and counts[:, 5].tolist() == m.tolist() and not marg.any()
    near, mn, _ = G.spfh(p, nrm, idx, d2, radius=1.0)          # the hybrid search: d2 <= 1
    assert mn.tolist() == [3, 1, 1, 1] and near.sum() == 3 * mn.sum()
    f = G.fpfh_from_spfh(counts, m, idx, d2)
    assert f.dtype == np.float32 and f[:, 5].tolist() == [200, 200, 200, 200] and f.sum() == 4 * 600


def test_reference_statuses_and_ties():
    sc = R.scene("S", 0, 90)
    src, tgt = sc["src"][:40], sc["tgt"]
    true = R.pose12(sc["R"], sc["t"])
    near = G.feature_nn(np.zeros((3, 33), np.float32), np.zeros((0, 33), np.float32))
    assert near[0].tolist() == [-1] * 3 and np.isinf(near[1]).all()
    f = np.random.RandomState(0).rand(6, 33).astype(np.float32)
    idx, d2 = G.feature_nn(f[:2], np.concatenate([f, f]))
    assert idx.tolist() == [0, 1] and d2.tolist() == [0, 0]    # the lowest index among equal distances
    bad = f.copy()
    bad[1, 7] = np.nan
    assert G.feature_nn(bad[:2], f)[0].tolist() == [0, -1] and G.feature_nn(f[:2], bad[1:2])[0].tolist() == [-1, -1]
    # correspondences by construction: source i is target j of the subset scene
    j = G.d2_3(R.transform(src, true)[:, None], tgt[None]).argmin(1)
    corr = np.stack([np.arange(40), j], 1).astype(np.int32)
    out = G.ransac(src, tgt, corr, 0.01, hypotheses=64)
    assert out["status"] == 0 and out["n_in"] == 40 and out["fitness"] == 1.0 and max(R.pose_error(out["pose"], sc["R"], sc["t"])) < 1e-6
    assert out["best"] == int(np.argmax(out["count"])) and (out["count"][:out["best"]] < 40).all()
    assert G.ransac(src, tgt, corr[:2], 0.01, hypotheses=64)["status"] == 1
    wrong = np.stack([np.arange(40), j[::-1]], 1).astype(np.int32)            # wrong partners: no triple fits to 1e-6
    lost = G.ransac(src, tgt, wrong, 1e-6, hypotheses=64, similarity=0.0)
    assert lost["status"] == 2 and lost["best"] >= 0 and lost["n_in"] == 0 and np.array_equal(lost["pose"], G.IDENTITY)
    nan = src.copy()
    nan[3, 0] = np.nan
    assert G.ransac(nan, tgt, corr, 0.01, hypotheses=64)["status"] == 4
    tr = [[0, 0, 1], [0, 1, 40], [0, 1, 2]]
    ok, _, _ = G.hypothesis_poses(src, tgt, corr, tr)
    assert ok.tolist() == [False, False, True]
    assert np.array_equal(D.correspondence_hypotheses([40, 7], 16, 3), scan.plane_hypotheses([40, 7], 16, 3))


def test_host_side_refusals():
    p, q, n = torch.zeros(10, 3), torch.zeros(12, 3), torch.zeros(10, 3)   # CPU tensors: every refusal below comes before the device check
    for k in (0, 65, 2.0, True):
        with pytest.raises(SfmiError, match="k must"):
            D.fpfh_dev(p, n, k=k)
    for r in (0, -1.0, float("inf"), True):
        with pytest.raises(SfmiError, match="radius"):
            D.fpfh_dev(p, n, radius=r)
    with pytest.raises(SfmiError, match="normals"):
        D.fpfh_dev(p, q)
    with pytest.raises(SfmiError, match="spfh"):
        D.fpfh_from_spfh_dev(p, None, 8, None, torch.zeros(9, 33, dtype=torch.int32), torch.zeros(10, dtype=torch.int32))
    fs, ft = torch.zeros(10, 33), torch.zeros(12, 33)
    with pytest.raises(SfmiError, match="fs"):
        D.match_features_dev(torch.zeros(10, 32), ft)
    with pytest.raises(SfmiError, match="sets"):
        D.match_features_dev(fs, ft, [0, 4, 10], [0, 12])
    for s in (0, 65, 1.5):
        with pytest.raises(SfmiError, match="splits"):
            D.match_features_dev(fs, ft, splits=s)
    with pytest.raises(SfmiError, match="queries_per_lane"):
        D.match_features_dev(fs, ft, queries_per_lane=3)
    corr = torch.zeros(4, 2, dtype=torch.int32)
    with pytest.raises(SfmiError, match="corr"):
        D.ransac_correspondences_dev(p, q, corr=corr.float(), max_dist=0.1)
    with pytest.raises(SfmiError, match="c_off"):
        D.ransac_correspondences_dev(p, q, [0, 4, 10], [0, 6, 12], corr, None, 0.1)
    for md in (None, -1.0, float("nan")):
        with pytest.raises(SfmiError, match="max_dist"):
            D.ransac_correspondences_dev(p, q, corr=corr, max_dist=md)
    for sim in (-0.1, 1.5, None):
        with pytest.raises(SfmiError, match="similarity"):
            D.ransac_correspondences_dev(p, q, corr=corr, max_dist=0.1, similarity=sim)
    with pytest.raises(SfmiError, match="hypotheses"):
        D.ransac_correspondences_dev(p, q, corr=corr, max_dist=0.1, hypotheses=0)
    for tr in (np.zeros((1, 4, 3)), np.zeros((2, 4, 3), np.int32), np.zeros((1, 4, 2), np.int32)):
        with pytest.raises(SfmiError, match="triples"):
            D.ransac_correspondences_dev(p, q, corr=corr, max_dist=0.1, triples=tr)
    with pytest.raises(SfmiError, match="triples"):
        D.hypothesis_poses_dev(p, q, corr=corr, triples=np.zeros((1, 4, 3)))
    with pytest.raises(SfmiError, match="poses"):
        D.score_poses_dev(p, q, corr=corr, max_dist=0.1, poses=np.zeros((1, 4, 11)))
    with pytest.raises(SfmiError, match="max_dist"):
        D.global_registration_dev(p, q)
    with pytest.raises(SfmiError, match="voxel"):
        D.global_registration_dev(p, q, voxel=0.0)
    with pytest.raises(SfmiError, match="unknown"):
        D.global_registration_dev(p, q, voxel=0.05, metric="point")
    with pytest.raises(SfmiError, match="viewpoints"):
        D.global_registration_dev(p, q, voxel=0.05, viewpoints=np.zeros(3))
    with pytest.raises(SfmiError, match="global_init"):
        D.merge_scans_dev([p, q], max_dist=0.1, global_init=0.05)
    with pytest.raises(SfmiError, match="global_init"):
        D.merge_scans_dev([p, q], max_dist=0.1, global_init=dict(voxel=0.05), init=np.eye(4))
    tr = np.zeros((1, 4, 3), np.int32)
    for call in (lambda: D.fpfh_dev(p, n), lambda: D.fpfh_from_spfh_dev(p, None, 8, None, torch.zeros(10, 33, dtype=torch.int32), torch.zeros(10, dtype=torch.int32)),
                 lambda: D.match_features_dev(fs, ft), lambda: D.ransac_correspondences_dev(p, q, corr=corr, max_dist=0.1),
                 lambda: D.hypothesis_poses_dev(p, q, corr=corr, triples=tr),
                 lambda: D.score_poses_dev(p, q, corr=corr, max_dist=0.1, poses=np.zeros((1, 4, 12))),
                 lambda: D.global_registration_dev(p, q, voxel=0.05), lambda: D.merge_scans_dev([p, q], max_dist=0.1, global_init=dict(voxel=0.05))):
        with pytest.raises(SfmiError, match="no CPU fallback"):                   # all arguments fine: the device check is the last one
            call()


def test_library_exports_every_global_registration_entry_of_the_header():
    text = open(os.path.join(ROOT, "include", "sfmi.h")).read()
    names = sorted(set(re.findall(r"\b(sfmi_(?:fpfh|greg)_\w+)\s*\(", text)))
    assert len(names) == 10 and "sfmi_fpfh_nn_f32" in names and "sfmi_greg_refit_f32" in names
    lib = _lib.lib()
    for n in names:
        assert hasattr(lib, n), f"libsfmi.so does not export {n}"
        assert n in _lib.PROTOTYPES, f"_lib.PROTOTYPES does not bind {n}"
    assert sorted(n for n in _lib.PROTOTYPES if n.startswith(("sfmi_fpfh_", "sfmi_greg_"))) == names
