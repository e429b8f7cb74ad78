"""Global registration on the device (csrc/features.hip, csrc/global_register.hip, shapeformer_amd/registration.py)
against tests/global_reg_ref.py.

What is exact is compared with `==`: the SPFH counts on every point that has no pair within 1e-9 of a bin edge of atan2's feature (at
most 1 % of the points, asserted), the feature search (idx and d2, split or not, 2 or 4 queries per lane), the mutual filter and its
compaction, the valid flags, the inlier counts of given poses, the winner, the final mask under the device's own refit pose, a batch
against per-pair calls, two runs.  What is not has a derived bound:
  fpfh    the second stage on the device's own counts: within 1 f32 ulp of the reference's (the terms are non-negative and both f64
          paths err by about k eps, so only the final rounding can move);
  poses   a hypothesis against numpy's SVD Kabsch: 64 eps x sigma_1 / sigma_2 of the centred cross-covariance (the polar factor of a
          rank-2 matrix is conditioned by that ratio; it is asserted below 1e4);
  sums    the refit sums: 4 n eps sum |term|; the refit pose from the device's own sums: the poses' bound;
  scenes  global_registration_dev ends no farther from the truth than 3 x the reference's own error on that scene (measured: 5.07e-3 /
          9.2e-4 on H, 2.70e-2 / 5.8e-3 on S; tests/test_global_reg_cpu.py): one count may differ where a pose differs in its last
          bits, and the device's normals are its own; ICP from there reaches what the reference reaches.
The scenes are icp_ref.scene on tests/golden/demo_ds/armchair/Xbd.npy; the normals of the exact tests are the same host arrays for the
device and the reference."""
import numpy as np
import pytest
import torch

import global_reg_ref as G
import icp_ref as R
from shapeformer_amd import _lib, registration as D, scan

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
SCENES = [("H", 0, 90), ("H", 1, 170), ("H", 2, 60), ("S", 0, 90), ("S", 1, 170)]


def _off(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(*ts):
    return [t.cpu().numpy() if isinstance(t, torch.Tensor) else t for t in ts]


@pytest.fixture(scope="module")
def refs():
    """the reference's run of the five scenes, once"""
    out = {}
    for key in SCENES:
        sc = R.scene(*key)
        out[key] = (sc, G.global_registration(sc["src"], sc["tgt"]))
    return out


@pytest.fixture(scope="module")
def cloud():
    """the fixture cloud of global_reg_ref: points, host normals, the same with one zero normal, the 64 neighbours"""
    return G.fixture_cloud()


# ---- 1. SPFH and FPFH -----------------------------------------------------------------------------------------------------------------

def _ulp_close(a, b):
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.maximum(np.abs(a), np.abs(b)))


def _check_fpfh(dev, p, nrm, off, k, radius, knn=None):
    """the device on a ragged batch against the reference set by set -> the fraction of marginal points"""
    feat, spfh, m = _np(*D.fpfh_dev(_t(p, dev), _t(nrm, dev), off, k, radius))
    again = D.fpfh_from_spfh_dev(_t(p, dev), off, k, radius, _t(spfh, dev), _t(m, dev)).cpu().numpy()
    assert feat.dtype == np.float32 and spfh.dtype == np.int32 and np.array_equal(feat, again)
    marginal = 0
    for b in range(len(off) - 1):
        sl = slice(off[b], off[b + 1])
        d2, idx = G.knn(p[sl], k) if knn is None else (knn[0][:, :k], knn[1][:, :k])
        counts, rm, marg = G.spfh(p[sl], nrm[sl], idx, d2, radius)
        assert np.array_equal(spfh[sl][~marg], counts[~marg]) and np.array_equal(m[sl][~marg], rm[~marg])
        assert (spfh[sl].sum(1) == 3 * m[sl]).all()
        want = G.fpfh_from_spfh(spfh[sl], m[sl], idx, d2, radius)          # the second stage on the device's own counts
        assert _ulp_close(feat[sl], want).all()
        marginal += marg.sum()
    return marginal / max(len(p), 1)


@pytest.mark.parametrize("k,radius", G.FPFH_CASES)
def test_fpfh_on_the_fixture(dev, cloud, k, radius):
    """the cap on the marginal points of these inputs is also asserted without a GPU, in tests/test_global_reg_cpu.py"""
    X, _, _, d2, idx = cloud
    nrm = G.fixture_normals(cloud, k)
    if k == 64 and radius is None:                             # the neighbourhood is knn_dev's, bit for bit
        kd2, kidx = _np(*scan.knn_dev(_t(X, dev), _t(X, dev), 64, exclude_self=True))
        assert np.array_equal(kidx, idx) and np.array_equal(kd2, d2)
    frac = _check_fpfh(dev, X, nrm, _off([len(X)]), k, radius, (d2, idx))
    print("k", k, "radius", radius, "marginal fraction", frac)
    assert frac <= 0.01
    if radius is not None and k >= 32:                         # the radius cuts into the neighbourhoods
        assert (d2[:, :k] > np.float32(radius ** 2)).any() and (d2[:, :k] <= np.float32(radius ** 2)).any()


def test_fpfh_ragged_small_sets(dev, cloud):
    X, nrm, _, _, _ = cloud
    k = G.RAGGED_K
    off = _off(G.RAGGED_SIZES)
    assert G.RAGGED_SIZES[:5] == [0, 1, 2, k, k + 1]
    p, n = X[:off[-1]].copy(), nrm[:off[-1]].copy()
    for radius in G.RAGGED_RADII:
        assert _check_fpfh(dev, p, n, off, k, radius) <= 0.01
    feat, spfh, m = _np(*D.fpfh_dev(_t(p, dev), _t(n, dev), off, k))
    assert m[0] == 0 and (feat[0] == 0).all() and (m[1:3] <= 1).all()            # a set of one point has no pair
    batch = D.fpfh_dev(_t(p[off[6]:].reshape(1, 300, 3), dev), _t(n[off[6]:].reshape(1, 300, 3), dev), None, k)
    assert batch[0].shape == (1, 300, 33) and np.array_equal(batch[0][0].cpu().numpy(), feat[off[6]:])


# ---- 2. the feature search ------------------------------------------------------------------------------------------------------------

def _check_nn(dev, fs, ft, so, to, **kw):
    corr, co, idx, d2 = _np(*D.match_features_dev(_t(fs, dev), _t(ft, dev), so, to, mutual=False, **kw))
    for b in range(len(so) - 1):
        ridx, rd2 = G.feature_nn(fs[so[b]:so[b + 1]], ft[to[b]:to[b + 1]])
        assert np.array_equal(idx[so[b]:so[b + 1]], ridx) and np.array_equal(d2[so[b]:so[b + 1]], rd2)
        keep = np.nonzero(ridx >= 0)[0]
        assert co[b + 1] - co[b] == len(keep) and np.array_equal(corr[co[b]:co[b + 1]], np.stack([keep, ridx[keep]], 1))
    return idx, d2


def test_feature_nn_edges(dev):
    lib = _lib.lib()
    tile, qb = lib.sfmi_fpfh_tile(), lib.sfmi_fpfh_query_block(0)
    assert tile == 64 and qb == 512 and lib.sfmi_fpfh_query_block(4) == 1024
    rs = np.random.RandomState(0)
    ns, nt = [qb - 1, qb, qb + 1, 5, 2 * qb + 3, 7], [0, 1, tile - 1, tile, tile + 1, 3 * tile + 5]
    fs = (rs.rand(sum(ns), 33) * 100).astype(np.float32)
    ft = (rs.rand(sum(nt), 33) * 100).astype(np.float32)
    so, to = _off(ns), _off(nt)
    base = _check_nn(dev, fs, ft, so, to)
    assert (base[0][:ns[0]] == -1).all() and np.isinf(base[1][:ns[0]]).all()      # an empty target set
    for kw in (dict(splits=1), dict(splits=3), dict(splits=64), dict(queries_per_lane=4), dict(queries_per_lane=4, splits=5)):
        other = _check_nn(dev, fs, ft, so, to, **kw)
        assert np.array_equal(other[0], base[0]) and np.array_equal(other[1], base[1])


def test_feature_nn_duplicates_nan_and_scene(dev, refs):
    rs = np.random.RandomState(1)
    f = (rs.rand(150, 33) * 100).astype(np.float32)
    q = (rs.rand(40, 33) * 100).astype(np.float32)
    q[:20] = f[rs.permutation(150)[:20]]                                       # exact matches: distance 0, twice in the target
    idx, d2 = _check_nn(dev, q, np.concatenate([f, f]), _off([40]), _off([300]), splits=2)
    assert (idx < 150).all() and (d2[:20] == 0).all()                           # the lower index wins
    bad_t, bad_s = np.concatenate([f, f]), q.copy()
    bad_t[idx[3], 4] = np.nan                                                  # the winner of query 3 drops out: its copy takes over
    bad_s[7, 0] = np.nan
    idx2, d22 = _check_nn(dev, bad_s, bad_t, _off([40]), _off([300]))
    assert idx2[3] == idx[3] + 150 and idx2[7] == -1 and np.isinf(d22[7])
    sc, g = refs[("S", 0, 90)]
    fs, ft = g["features"]
    assert _lib.lib().sfmi_fpfh_nn_splits(1, len(fs), len(ft), 0) > 1         # the scene alone: the target is cut and merged
    _check_nn(dev, fs, ft, _off([len(fs)]), _off([len(ft)]))
    _check_nn(dev, fs, ft, _off([len(fs)]), _off([len(ft)]), splits=1)


def test_mutual_filter_and_compaction(dev, refs):
    keys = [("H", 0, 90), ("S", 0, 90)]
    fs = np.concatenate([refs[k][1]["features"][0] for k in keys] + [np.zeros((3, 33), np.float32)])
    ft = np.concatenate([refs[k][1]["features"][1] for k in keys])
    so = _off([len(refs[k][1]["features"][0]) for k in keys] + [3])
    to = _off([len(refs[k][1]["features"][1]) for k in keys] + [0])
    corr, co, idx, d2 = _np(*D.match_features_dev(_t(fs, dev), _t(ft, dev), so, to))
    for b, k in enumerate(keys):
        want = refs[k][1]["corr"]
        assert np.array_equal(corr[co[b]:co[b + 1]], want) and len(want) in (219, 184)
    assert co[3] == co[2] and corr.dtype == np.int32


# ---- 3. hypotheses ----------------------------------------------------------------------------------------------------------------------

def test_valid_flags(dev):
    base = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [2, 0, 0], [3, 0, 0]])
    src = np.concatenate([base, base[:1]])                                     # point 6 repeats point 0
    tgt = np.concatenate([2 * base, 2 * base[:1], np.float32([[0.25, 0.25, 0.125]])])   # the target triangles are twice as large
    corr = np.int32([[0, 0], [1, 1], [2, 2], [3, 3], [4, 4], [5, 5], [6, 6], [6, 0], [3, 7]])
    tr = np.int32([[[0, 1, 2], [0, 0, 1], [0, 1, 9], [-1, 1, 2], [0, 1, 6], [1, 2, 7], [0, 4, 5], [1, 2, 3], [0, 1, 8]]])
    half_up = float(np.nextafter(0.5, 1.0))
    for sim, want in ((0.5, [1, 0, 0, 0, 0, 1, 0, 1, 0]), (half_up, [0] * 9), (0.0, [1, 0, 0, 0, 0, 1, 0, 1, 1])):
        args = (_t(src, dev), _t(tgt, dev), None, None, _t(corr, dev), None, tr, sim)
        poses, valid = _np(*D.hypothesis_poses_dev(*args))
        ok, rp, _ = G.hypothesis_poses(src, tgt, corr, tr[0], sim)
        assert valid[0].tolist() == want and ok.tolist() == [bool(v) for v in want]
        assert np.isnan(poses[0][~ok]).all() and (not ok.any() or np.abs(poses[0][ok] - rp[ok]).max() < 1e-14)
        rev = _np(*D.hypothesis_poses_dev(_t(tgt, dev), _t(src, dev), None, None, _t(corr[:, ::-1].copy(), dev), None, tr, sim))
        assert rev[1][0].tolist() == want                                      # the other boundary: the source twice as large
    # [0 1 2] ok at sim = 1/2 exactly (ls = lt / 2); [0 0 1] repeats; [0 1 9], [-1 1 2] outside; [0 1 6] two source points coincide;
    # [1 2 7] ok (source 6 = source 0, target 0); [0 4 5] collinear; [0 1 8]: the edge (0,0,1)-(0,0,0) against 0.375 fails until sim = 0


def test_hypothesis_poses_against_numpy(dev, refs):
    sc, g = refs[("H", 1, 170)]
    corr = g["corr"]
    tr = D.correspondence_hypotheses([len(corr)], 2048, 5)
    poses, valid = _np(*D.hypothesis_poses_dev(_t(sc["src"], dev), _t(sc["tgt"], dev), None, None, _t(corr, dev), None, tr, 0.9))
    ok, rp, S = G.hypothesis_poses(sc["src"], sc["tgt"], corr, tr[0], 0.9)
    assert np.array_equal(valid[0].astype(bool), ok) and 20 < ok.sum() < 2048
    ratio = S[ok, 0] / S[ok, 1]
    assert ratio.max() < 1e4
    err = np.abs(poses[0][ok] - rp[ok]).max(1)
    print("valid", ok.sum(), "max ratio", ratio.max(), "max err / bound", (err / (64 * EPS * ratio)).max())
    assert (err <= 64 * EPS * ratio).all()
    Rm = poses[0][ok].reshape(-1, 3, 4)[:, :, :3]
    assert np.abs(np.linalg.det(Rm) - 1).max() < 1e-12 and np.abs(Rm @ Rm.transpose(0, 2, 1) - np.eye(3)).max() < 1e-12 * ratio.max()


# ---- 4. scoring -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H", [1, 255, 256, 257])
def test_score_counts(dev, refs, H):
    rs = np.random.RandomState(H)
    pairs = [refs[("H", 0, 90)], refs[("S", 1, 170)]]
    src, tgt = np.concatenate([p[0]["src"] for p in pairs] * 2), np.concatenate([p[0]["tgt"] for p in pairs] * 2)
    so, to = _off([len(p[0]["src"]) for p in pairs] * 2), _off([len(p[0]["tgt"]) for p in pairs] * 2)
    corrs = [pairs[0][1]["corr"], pairs[1][1]["corr"], pairs[0][1]["corr"][:3], pairs[1][1]["corr"][:0]]
    corrs[2] = corrs[2][:2] if H == 255 else corrs[2]                           # C = 0, 2 and 3 among the pairs
    co = _off([len(c) for c in corrs])
    poses = np.empty((4, H, 12))
    for b in range(4):
        sc = pairs[b % 2][0]
        for h in range(H):                                                      # the truth, turned by up to a few degrees
            poses[b, h] = R.pose12(R.rodrigues(rs.randn(3) * 0.02 * (h % 5)) @ sc["R"], sc["t"] + rs.randn(3) * 0.002 * (h % 3))
    if H > 1:
        poses[0, 1, 3] = np.nan
    count = D.score_poses_dev(_t(src, dev), _t(tgt, dev), so, to, _t(np.concatenate(corrs), dev), co, 0.03, poses).cpu().numpy()
    for b in range(4):
        want = G.score(src[so[b]:so[b + 1]], tgt[to[b]:to[b + 1]], corrs[b], poses[b], 0.03)
        assert np.array_equal(count[b], want)
    assert count[:2].max() >= 15 and (count[3] == 0).all() and (H == 1 or count[0, 1] == 0)


def test_score_at_exactly_max_dist(dev):
    s, t = np.float32([[0, 0, 0], [1, 1, 1], [2, 0, 0]]), np.float32([[0.5, 0, 0], [1, 1, 1.75], [2, 0.25, 0]])
    corr = np.int32([[0, 0], [1, 1], [2, 2]])
    args = (_t(s, dev), _t(t, dev), None, None, _t(corr, dev), None)
    ident = G.IDENTITY.reshape(1, 1, 12)
    assert D.score_poses_dev(*args, 0.5, ident).item() == 2                    # d2 = 0.25 <= 0.25: an inlier at exactly max_dist
    assert D.score_poses_dev(*args, float(np.nextafter(np.float32(0.5), np.float32(0))), ident).item() == 1
    assert D.score_poses_dev(*args, 0.75, ident).item() == 3 and D.score_poses_dev(*args, 0.0, ident).item() == 0


# ---- 5. RANSAC: the winner, the refit, batches --------------------------------------------------------------------------------------------

def _ransac(dev, sc, corr, max_dist=0.03, **kw):
    return D.ransac_correspondences_dev(_t(sc["src"], dev), _t(sc["tgt"], dev), None, None, _t(corr, dev), None, max_dist, **kw)


def _check_counts(sc, corr, count, poses, valid, max_dist=0.03):
    """count (H,) against the reference's count of the device's own poses (H,12); -> the first of the largest"""
    ok = valid.astype(bool)
    want = np.full(len(count), -1, np.int32)
    if ok.any():
        want[ok] = G.score(sc["src"], sc["tgt"], corr, poses[ok], max_dist)
    assert np.array_equal(count, want)
    return int(np.argmax(want)) if ok.any() else -1


def test_best_with_tied_counts(dev, refs):
    sc, g = refs[("H", 2, 60)]
    corr = g["corr"]
    tr = D.correspondence_hypotheses([len(corr)], 300, 0)
    ref = G.ransac(sc["src"], sc["tgt"], corr, 0.03, triples=tr[0])
    w = ref["best"]
    assert w > 6 and ref["count"][w] >= 20
    tr[0, 290], tr[0, 6], tr[0, 3] = tr[0, w], tr[0, w], [0, 0, 1]              # the winner three times: the lowest h takes it
    out = _ransac(dev, sc, corr, triples=tr, details=True)
    pose, fit, inl, n_in, count, best, status = _np(*out[:7])
    first = _check_counts(sc, corr, count[0], *_np(out[7]["poses"][0], out[7]["valid"][0]))
    assert best[0] == 6 == first and count[0, 6] == count[0, w] == count[0, 290] and count[0, 3] == -1 and status[0] == 0


def test_refit_sums_and_pose(dev, refs):
    for key in (("H", 0, 90), ("S", 0, 90)):
        sc, g = refs[key]
        corr = g["corr"]
        out = _ransac(dev, sc, corr, details=True)
        pose, fit, inl, n_in, count, best, status = _np(*out[:7])
        poses, valid, sums = _np(out[7]["poses"], out[7]["valid"], out[7]["sums"])
        assert status[0] == 0 and best[0] == _check_counts(sc, corr, count[0], poses[0], valid[0])
        winner = poses[0, best[0]]
        mask = G.inliers(sc["src"], sc["tgt"], corr, winner, 0.03)
        s, q = G.refit_terms(sc["src"], sc["tgt"], corr, mask)
        n = len(s)
        assert sums[0, 0] == n == count[0, best[0]] and n >= 15
        for got, terms in ((sums[0, 1:4], s), (sums[0, 4:7], q)):
            assert (np.abs(got - terms.sum(0)) <= 4 * n * EPS * np.abs(terms).sum(0)).all()
        cs, cq = sums[0, 1:4] / n, sums[0, 4:7] / n                             # the device's own centroids
        cross = (q - cq)[:, :, None] * (s - cs)[:, None, :]
        M = sums[0, 7:].reshape(3, 3)
        assert (np.abs(M - cross.sum(0)) <= 4 * n * EPS * np.abs(cross).sum(0)).all()
        U, S, Vt = np.linalg.svd(M)
        Rm = U @ np.diag([1, 1, np.sign(np.linalg.det(U @ Vt))]) @ Vt
        want = R.pose12(Rm, cq - Rm @ cs)
        bound = 64 * EPS * S[0] / S[1]
        print(key, "inliers", n, "sigma", S, "pose err / bound", np.abs(pose[0, :3].reshape(12) - want).max() / bound)
        assert S[0] / S[1] < 1e4 and np.abs(pose[0, :3].reshape(12) - want).max() <= bound
        final = G.inliers(sc["src"], sc["tgt"], corr, pose[0, :3].reshape(12), 0.03)
        assert np.array_equal(inl.astype(bool), final) and n_in[0] == final.sum() and fit[0] == final.sum() / len(corr)
        norefit = _np(*_ransac(dev, sc, corr, refit=False))
        assert np.array_equal(norefit[0][0, :3].reshape(12), winner) and np.array_equal(norefit[2].astype(bool), mask) and norefit[3][0] == n


def test_mixed_batch_equals_per_pair_calls_and_two_runs(dev, refs):
    a, b = refs[("H", 1, 170)], refs[("S", 0, 90)]
    nan = dict(a[0], src=a[0]["src"].copy())
    nan["src"][11, 2] = np.nan
    pairs = [(a[0], a[1]["corr"]), (b[0], b[1]["corr"]), (a[0], a[1]["corr"][:0]), (b[0], b[1]["corr"][:2]), (nan, a[1]["corr"]),
             (b[0], b[1]["corr"][::-1][:60].copy())]
    src, tgt = np.concatenate([p[0]["src"] for p in pairs]), np.concatenate([p[0]["tgt"] for p in pairs])
    so, to, co = _off([len(p[0]["src"]) for p in pairs]), _off([len(p[0]["tgt"]) for p in pairs]), _off([len(p[1]) for p in pairs])
    corr = np.concatenate([p[1] for p in pairs])
    def call():
        out = D.ransac_correspondences_dev(_t(src, dev), _t(tgt, dev), so, to, _t(corr, dev), co, 0.03, hypotheses=1024, seed=2, details=True)
        return _np(*out[:7]), _np(out[7]["poses"], out[7]["valid"])
    base, (hp, hv) = call()
    pose, fit, inl, n_in, count, best, status = base
    assert status.tolist()[:5] == [0, 0, 1, 1, 4] and (count[2:5] == -1).all() and (best[2:5] == -1).all()
    for x in (2, 3, 4):
        assert np.array_equal(pose[x], np.eye(4)) and n_in[x] == 0 and fit[x] == 0
    for x, y in zip(base, call()[0]):                                           # two runs: the same bits
        assert np.array_equal(x, y, equal_nan=True)
    for i, (sc, c) in enumerate(pairs):                                         # a pair alone: the same bits
        one = _np(*_ransac(dev, sc, c, hypotheses=1024, seed=2))
        for x, y in zip((pose, fit, n_in, count, best, status), (one[0], one[1], one[3], one[4], one[5], one[6])):
            assert np.array_equal(x[i:i + 1], y)
        assert np.array_equal(inl[co[i]:co[i + 1]], one[2])
        if status[i] == 0:
            assert best[i] == _check_counts(sc, c, count[i], hp[i], hv[i])
    wrong = np.stack([b[1]["corr"][:, 0], b[1]["corr"][::-1, 1]], 1)            # wrong partners: a winner without three inliers
    lost = _np(*_ransac(dev, b[0], wrong, max_dist=1e-6, hypotheses=256, similarity=0.0))
    assert lost[6][0] == 2 and lost[5][0] >= 0 and np.array_equal(lost[0][0], np.eye(4)) and lost[3][0] == 0 and not lost[2].any()


# ---- 6. end to end ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def global_poses(dev, refs):
    """global_registration_dev on the five scenes in one batch"""
    scs = [refs[k][0] for k in SCENES]
    src, tgt = np.concatenate([s["src"] for s in scs]), np.concatenate([s["tgt"] for s in scs])
    so, to = _off([len(s["src"]) for s in scs]), _off([len(s["tgt"]) for s in scs])
    out = _np(*D.global_registration_dev(_t(src, dev), _t(tgt, dev), so, to, max_dist=0.03))
    return (src, tgt, so, to), out


def test_global_registration_on_the_scenes(refs, global_poses):
    _, (pose, fit, inl, n_in, count, best, status) = global_poses
    for b, key in enumerate(SCENES):
        sc, g = refs[key]
        eR, et = R.pose_error(pose[b, :3].reshape(12), sc["R"], sc["t"])
        rR, rt = R.pose_error(g["pose"], sc["R"], sc["t"])                     # measured: 5.07e-3 / 9.2e-4 (H), 2.70e-2 / 5.8e-3 (S)
        print(key, "device", eR, et, "inliers", n_in[b], "reference", rR, rt, "inliers", g["n_in"])
        assert status[b] == 0 and eR <= 3 * rR and et <= 3 * rt


def test_icp_from_the_global_pose(dev, refs, global_poses):
    """ICP (point metric, max_dist 0.05) from the device's global pose reaches what the reference's ICP reaches from the reference's
    global pose: the truth to 1e-6 on S (the margin of tests/test_icp_gpu.py); on H the scene's fixed point, within 10 x the spread of
    the reference's own runs from its three global poses and from the three true motions (the margin's construction in
    tests/test_icp_gpu.py).  From the identity it does not: it ends more than 0.1 away."""
    (src, tgt, so, to), out = global_poses
    s, t = _t(src, dev), _t(tgt, dev)
    pose, fitness, rmse, it, status = _np(*D.icp_dev(s, t, so, to, 0.05, init=_t(out[0], dev)))
    lone = _np(*D.icp_dev(s, t, so, to, 0.05))
    rel = lambda p44, sc: np.concatenate([(p44[:3, :3] @ sc["R"].T).ravel(), p44[:3, 3] - p44[:3, :3] @ sc["R"].T @ sc["t"]])
    runs = []
    for key in SCENES[:3]:
        sc, g = refs[key]
        for init in (g["pose"], R.pose12(sc["R"], sc["t"])):
            r = R.icp(sc["src"], sc["tgt"], 0.05, init=init)
            assert r[4] == 0
            runs.append(rel(R.pose44(r[0]), sc))
    runs = np.stack(runs)
    spread = max(np.abs(x - y).max() for x in runs for y in runs)
    for b, key in enumerate(SCENES):
        sc = refs[key][0]
        eR, et = R.pose_error(pose[b, :3].reshape(12), sc["R"], sc["t"])
        lR, _ = R.pose_error(lone[0][b, :3].reshape(12), sc["R"], sc["t"])
        dist = np.abs(rel(pose[b], sc) - runs.mean(0)).max()
        print(key, "icp from global", eR, et, "fitness", fitness[b], "from identity", lR, "H spread", spread, "dist", dist)
        assert status[b] == 0 and lR > 0.1
        if key[0] == "S":
            assert eR <= 1e-6 and et <= 1e-6 and fitness[b] == 1.0
        else:
            assert dist <= 10 * spread


def test_a_nan_in_one_pair_leaves_the_other_pairs_alone(dev, refs):
    """global_registration_dev on [a pair with a NaN coordinate, two healthy scenes]: the bad pair reports status 4 and the identity,
    and every healthy pair has the bits of its own per-pair call - normals, features, correspondences and pose depend on the pair alone
    (the centroid that orients the normals is the set's own)"""
    keys = [("H", 0, 90), ("S", 1, 170)]
    bad = dict(refs[("S", 0, 90)][0])
    bad["src"], bad["tgt"] = bad["src"].copy(), bad["tgt"].copy()
    bad["src"][17, 1], bad["tgt"][3, 0] = np.nan, np.inf
    scs = [bad] + [refs[k][0] for k in keys]
    src, tgt = np.concatenate([s["src"] for s in scs]), np.concatenate([s["tgt"] for s in scs])
    so, to = _off([len(s["src"]) for s in scs]), _off([len(s["tgt"]) for s in scs])
    pose, fit, inl, n_in, count, best, status = _np(*D.global_registration_dev(_t(src, dev), _t(tgt, dev), so, to, max_dist=0.03))
    assert status.tolist() == [4, 0, 0] and np.array_equal(pose[0], np.eye(4)) and n_in[0] == 0 and best[0] == -1 and (count[0] == -1).all()
    end = len(inl)
    for b in (2, 1):                                                            # the healthy pairs, from the back of the inlier mask
        sc = scs[b]
        one = _np(*D.global_registration_dev(_t(sc["src"], dev), _t(sc["tgt"], dev), max_dist=0.03))
        for x, y in zip((pose, fit, n_in, count, best, status), (one[0], one[1], one[3], one[4], one[5], one[6])):
            assert np.array_equal(x[b:b + 1], y)
        assert np.array_equal(inl[end - len(one[2]):end], one[2]) and n_in[b] >= 15
        end -= len(one[2])
    swapped = _np(*D.global_registration_dev(_t(tgt, dev), _t(src, dev), to, so, max_dist=0.03))      # the NaN pair's target leads the batch
    assert swapped[6].tolist() == [4, 0, 0]


def test_global_registration_with_a_voxel_reduction(dev, refs):
    """voxel = 0.02 in front of the features, max_dist at its default of 1.5 x voxel: against the reference on the clouds reduced by
    tests/downsample_ref.py (measured there: 8.6e-2 / 2.5e-2 on H at 90 degrees with 39 inliers of 158 correspondences, 2.4e-2 / 5.9e-3
    on S at 170 degrees with 21 of 159), the same 3 x margin; the pose is in the frame of the full clouds, and ICP on them reaches the
    truth on S from it"""
    import downsample_ref as DS
    keys = [("H", 0, 90), ("S", 1, 170)]
    scs = [refs[k][0] for k in keys]
    src, tgt = np.concatenate([s["src"] for s in scs]), np.concatenate([s["tgt"] for s in scs])
    so, to = _off([len(s["src"]) for s in scs]), _off([len(s["tgt"]) for s in scs])
    out = _np(*D.global_registration_dev(_t(src, dev), _t(tgt, dev), so, to, voxel=0.02))
    same = _np(*D.global_registration_dev(_t(src, dev), _t(tgt, dev), so, to, voxel=0.02, max_dist=1.5 * 0.02))
    for x, y in zip(out, same):
        assert np.array_equal(x, y)
    for b, sc in enumerate(scs):
        g = G.global_registration(DS.voxel_down(sc["src"], 0.02)[0], DS.voxel_down(sc["tgt"], 0.02)[0], max_dist=1.5 * 0.02)
        eR, et = R.pose_error(out[0][b, :3].reshape(12), sc["R"], sc["t"])
        rR, rt = R.pose_error(g["pose"], sc["R"], sc["t"])
        print(keys[b], "device", eR, et, "inliers", out[3][b], "reference", rR, rt, "inliers", g["n_in"], "of", len(g["corr"]))
        assert g["status"] == 0 and out[6][b] == 0 and eR <= 3 * rR and et <= 3 * rt
    pose, fitness, _, _, status = _np(*D.icp_dev(_t(src, dev), _t(tgt, dev), so, to, 0.05, init=_t(out[0], dev)))
    eR, et = R.pose_error(pose[1, :3].reshape(12), scs[1]["R"], scs[1]["t"])
    assert status[1] == 0 and fitness[1] == 1.0 and eR <= 1e-6 and et <= 1e-6


def test_merge_scans_with_global_init(dev):
    """Three 60 % subsets of the fixture, two of them moved by 60 and 170 degrees.  The reference merge starts ICP from the reference's
    global pose; the device's merged cloud has its Chamfer distance to the fixture within the 1e-3 relative margin that
    tests/test_icp_gpu.py gives merges.  Without global_init the merge is at least 10 x farther."""
    X = R.fixture()
    rs = np.random.RandomState(11)
    subs = [X[rs.permutation(len(X))[:1229]] for _ in range(3)]
    clouds = [subs[0], R.moved(subs[1], *R.motion(1, 60)), R.moved(subs[2], *R.motion(2, 170))]
    parts = [clouds[0]]
    for c in clouds[1:]:
        g = G.global_registration(c, clouds[0])
        r = R.icp(c, clouds[0], 0.05, init=g["pose"], max_iter=60)
        assert g["status"] == 0 and r[4] == 0
        parts.append(R.transform(c, r[0]))
    c_ref, c_raw = R.chamfer(np.concatenate(parts), X), R.chamfer(np.concatenate(clouds), X)
    merged, poses, status = D.merge_scans_dev([_t(c, dev) for c in clouds], max_dist=0.05, max_iter=60, global_init=dict(max_dist=0.03))
    c_dev = R.chamfer(merged.cpu().numpy(), X)
    plain, _, st0 = D.merge_scans_dev([_t(c, dev) for c in clouds], max_dist=0.05, max_iter=60)
    c_plain = R.chamfer(plain.cpu().numpy(), X)
    print("chamfer device", c_dev, "reference", c_ref, "unregistered", c_raw, "without global_init", c_plain, "poses", poses[1:, :3, 3])
    assert status.tolist() == [0, 0, 0] and merged.shape == (3 * 1229, 3) and np.array_equal(poses[0].cpu().numpy(), np.eye(4))
    assert c_dev <= c_ref * (1 + 1e-3) and c_raw >= 10 * c_dev
    assert c_plain >= 10 * c_dev
