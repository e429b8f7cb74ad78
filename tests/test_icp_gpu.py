"""Iterative closest point on the device (csrc/register.hip, shapeformer_amd/registration.py) against tests/icp_ref.py.

What is exact is compared with `==`: the transform, the correspondences (against the numpy statement and against the project's own
nn_dist on the reference-transformed cloud), the inlier count, a batch against per-pair calls, two runs, any check_every.
What is not has a derived bound:
  sums   |device - numpy| <= 4 n eps sum |term| per entry, n the inlier count: any two summation orders of n terms differ by at most
         2 (n - 1) eps sum |term|, and the terms themselves agree to a few eps;
  step   xi against numpy.linalg.solve on the device's own sums: cond(A) x 64 eps relative (both solvers are backward stable to a few
         eps on a 6 x 6 system; cond(A) < 100 is asserted); the pose likewise, relative to its largest entry;
  loop   scene S ends within 1e-6 of the true motion: the 6e-8 spacing of the f32 inputs x cond <= 17, with room (the reference
         alone reaches 8e-9).
The scenes are cut from tests/golden/demo_ds/armchair/Xbd.npy by icp_ref.scene; the target normals are icp_ref.pca_normals (host PCA),
the same arrays for the device and the reference."""
import numpy as np
import pytest
import torch

import icp_ref as R
from shapeformer_amd import _lib, metrics, registration as G

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
S_STARTS = [(0, 5, 0.05), (1, 10, 0.05), (2, 15, 0.1)]                       # (seed, degrees, max_dist) of scene S
H_STARTS = [(seed, deg) for seed in range(3) for deg in (5, 10)]


def _off(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(*ts):
    return [t.cpu().numpy() for t in ts]


def _pack(pairs, dev):
    """[scene dict] -> source, target, normals tensors and host offsets"""
    src, tgt, nrm = (np.concatenate([p[k] for p in pairs]) for k in ("src", "tgt", "nrm"))
    return _t(src, dev), _t(tgt, dev), _t(nrm, dev), _off([len(p["src"]) for p in pairs]), _off([len(p["tgt"]) for p in pairs])


def _run(dev, pairs, metric, max_dist, **kw):
    s, t, n, so, to = _pack(pairs, dev)
    plane = "plane" in (metric if isinstance(metric, list) else [metric])
    return _np(*G.icp_dev(s, t, so, to, max_dist, metric, n if plane else None, **kw))


def _rel(pose44, sc):
    """the pose against the scene's true motion: (R Rt^T, t - R Rt^T tt) as 12 numbers, the identity for a perfect result"""
    Rr = pose44[:3, :3] @ sc["R"].T
    return np.concatenate([Rr.ravel(), pose44[:3, 3] - Rr @ sc["t"]])


def _mid_pose(sc, frac=0.5):
    """a pose part of the way from the identity to the truth"""
    from scipy.spatial.transform import Rotation
    return R.pose12(R.rodrigues(Rotation.from_matrix(sc["R"]).as_rotvec() * frac), sc["t"] * frac)


@pytest.fixture(scope="module")
def scenes_S():
    return [R.scene("S", seed, deg) for seed, deg, _ in S_STARTS]


@pytest.fixture(scope="module")
def scenes_H():
    return [R.scene("H", seed, deg) for seed, deg in H_STARTS]


@pytest.fixture(scope="module")
def scene_D():
    return R.scene("D", 0, 5)


# ---- 1. transform ---------------------------------------------------------------------------------------------------------------------

def test_transform_bits(dev):
    rs = np.random.RandomState(0)
    sizes = [0, 1, 257, 0, 300]
    p = rs.uniform(-0.8, 0.8, (sum(sizes), 3)).astype(np.float32)
    ax = np.array([1.0, -2.0, 0.5]) / np.linalg.norm([1.0, -2.0, 0.5])
    poses = np.stack([R.IDENTITY, R.IDENTITY, R.pose12(R.rodrigues(ax * np.deg2rad(170)), [0.3, -0.2, 0.1]),
                      R.IDENTITY, R.pose12(R.rodrigues(rs.randn(3)), rs.randn(3))])
    off = _off(sizes)
    out = G.transform_points_dev(_t(p, dev), off, poses).cpu().numpy()
    ref = np.concatenate([R.transform(p[off[b]:off[b + 1]], poses[b]) for b in range(len(sizes))])
    assert out.dtype == np.float32 and np.array_equal(out, ref)
    assert np.array_equal(out[:1], p[:1])                                       # the identity returns the bits it was given
    assert not np.array_equal(out[1:258], p[1:258])
    p44 = np.stack([R.pose44(q) for q in poses])                                # the three pose layouts are one pose
    assert np.array_equal(G.transform_points_dev(_t(p, dev), off, _t(p44, dev)).cpu().numpy(), out)
    one = G.transform_points_dev(_t(p[1:258].reshape(1, 257, 3), dev), None, poses[2]).cpu().numpy()
    assert one.shape == (1, 257, 3) and np.array_equal(one[0], out[1:258])


# ---- 2. correspondences at a given pose ---------------------------------------------------------------------------------------------

def _check_corr(dev, src, tgt, so, to, poses, max_dist=0.1):
    fit, rmse, idx, d2 = _np(*G.evaluate_registration_dev(_t(src, dev), _t(tgt, dev), so, to, max_dist, poses))
    moved = np.concatenate([R.transform(src[so[b]:so[b + 1]], poses[b]) for b in range(len(so) - 1)])
    nd2, nidx = _np(*metrics.nn_dist(_t(moved, dev), _t(tgt, dev), so, to, return_index=True))
    assert np.array_equal(idx, nidx) and np.array_equal(d2, nd2)                # the project's nn_dist on the reference-transformed cloud
    for b in range(len(so) - 1):
        ridx, rd2 = R.nn(moved[so[b]:so[b + 1]], tgt[to[b]:to[b + 1]])
        assert np.array_equal(idx[so[b]:so[b + 1]], ridx) and np.array_equal(d2[so[b]:so[b + 1]], rd2)
        inl = rd2 <= R.maxd2_of(max_dist)
        assert fit[b] == (inl.sum() / len(ridx) if len(ridx) else 0.0)
        want = np.sqrt(rd2[inl].astype(np.float64).sum() / inl.sum()) if inl.any() else 0.0
        assert rmse[b] == pytest.approx(want, rel=1e-13)
    return idx, d2


@pytest.mark.parametrize("nt", [1, 255, 256, 257])
@pytest.mark.parametrize("ns", [2047, 2048, 2049])
def test_correspondences_at_the_block_and_tile_edges(dev, ns, nt):
    lib = _lib.lib()
    assert lib.sfmi_icp_query_block() == 2048 and lib.sfmi_icp_splits(1, ns, nt) == 1
    rs = np.random.RandomState(ns * 1000 + nt)
    src = rs.uniform(-0.8, 0.8, (ns, 3)).astype(np.float32)
    tgt = rs.uniform(-0.8, 0.8, (nt, 3)).astype(np.float32)
    pose = R.pose12(R.rodrigues(rs.randn(3) * 0.3), rs.randn(3) * 0.05)
    _check_corr(dev, src, tgt, _off([ns]), _off([nt]), pose[None])


def test_correspondences_split_target_and_ragged_batch(dev, scenes_S):
    lib = _lib.lib()
    sc = scenes_S[0]
    assert lib.sfmi_icp_splits(1, 700, 1400) > 1                                # scene S alone: the target is cut and merged
    _check_corr(dev, sc["src"], sc["tgt"], _off([700]), _off([1400]), _mid_pose(sc)[None])
    rs = np.random.RandomState(5)
    sizes_s, sizes_t = [700, 0, 2049, 3], [1400, 5, 600, 0]
    assert lib.sfmi_icp_splits(4, sum(sizes_s), sum(sizes_t)) == 1 and lib.sfmi_icp_splits(2, 2752, 4000) > 1
    src = np.concatenate([sc["src"], rs.uniform(-0.8, 0.8, (2052, 3)).astype(np.float32)])
    tgt = np.concatenate([sc["tgt"], rs.uniform(-0.8, 0.8, (605, 3)).astype(np.float32)])
    poses = np.stack([_mid_pose(sc), R.IDENTITY, R.pose12(R.rodrigues([0.1, 0.2, -0.1]), [0.01, 0, 0.02]), R.IDENTITY])
    so, to = _off(sizes_s), _off(sizes_t)
    s, t = _t(src, dev), _t(tgt, dev)
    fit, rmse, idx, d2 = _np(*G.evaluate_registration_dev(s, t, so, to, 0.1, poses))
    for b in range(3):                                                          # an empty target: (-1, +inf), fitness 0
        m = R.transform(src[so[b]:so[b + 1]], poses[b])
        ridx, rd2 = R.nn(m, tgt[to[b]:to[b + 1]])
        assert np.array_equal(idx[so[b]:so[b + 1]], ridx) and np.array_equal(d2[so[b]:so[b + 1]], rd2)
    assert (idx[so[3]:] == -1).all() and np.isinf(d2[so[3]:]).all() and fit[3] == 0 and rmse[3] == 0 and fit[1] == 0
    two_s, two_t = np.concatenate([src[:700], src[700:2752]]), np.concatenate([tgt[:1400], np.tile(tgt[1400:2000], (5, 1))[:2600]])
    _check_corr(dev, two_s, two_t, _off([700, 2052]), _off([1400, 2600]), poses[[0, 2]])   # two pairs, split targets


def test_correspondences_duplicates_and_the_exact_bound(dev):
    rs = np.random.RandomState(3)
    q = rs.uniform(-0.5, 0.5, (300, 3)).astype(np.float32)
    src = rs.uniform(-0.5, 0.5, (500, 3)).astype(np.float32)
    idx, _ = _check_corr(dev, src, np.concatenate([q, q]), _off([500]), _off([600]), R.IDENTITY[None])
    assert (idx < 300).all()                                                    # every target point is there twice: the lower index wins
    # dyadic coordinates, a pair at exactly max_dist: an inlier; one f32 step closer in max_dist and it is not
    s1, t1 = np.float32([[0, 0, 0], [1, 1, 1]]), np.float32([[0.5, 0, 0], [1, 1, 1.75]])
    fit, _, idx, d2 = _np(*G.evaluate_registration_dev(_t(s1, dev), _t(t1, dev), None, None, 0.5))
    assert idx.tolist() == [0, 1] and d2.tolist() == [0.25, 0.5625] and fit[0] == 0.5
    assert G.evaluate_registration_dev(_t(s1, dev), _t(t1, dev), None, None, float(np.nextafter(np.float32(0.5), np.float32(0))))[0].item() == 0
    assert G.evaluate_registration_dev(_t(s1, dev), _t(t1, dev), None, None, 0.75)[0].item() == 1.0


# ---- 3. sums, 4. step ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def mid_step(dev, scenes_S):
    """scene S (seed 0) at a mid pose: the device's step for both metrics and the reference's evaluation"""
    sc = scenes_S[0]
    pose = _mid_pose(sc)
    out = {}
    for metric in ("point", "plane"):
        d = _np(*G.icp_step_dev(_t(sc["src"], dev), _t(sc["tgt"], dev), None, None, 0.05, metric,
                                _t(sc["nrm"], dev) if metric == "plane" else None, pose))
        out[metric] = dict(dev=d, ref=R.evaluate(sc["src"], sc["tgt"], sc["nrm"], pose, 0.05, metric), pose=pose)
    return out


@pytest.mark.parametrize("metric", ["point", "plane"])
def test_sums_against_numpy(mid_step, metric):
    (pose1, xi, sums, idx, d2, status), ref = mid_step[metric]["dev"], mid_step[metric]["ref"]
    assert np.array_equal(idx, ref["idx"]) and np.array_equal(d2, ref["d2"])
    n = ref["sums"][R.CNT]
    assert sums[0, R.CNT] == n and 300 < n <= 700                               # the count is exact
    bound = 4 * n * EPS * ref["abs"]
    err = np.abs(sums[0] - ref["sums"])
    print(metric, "n", n, "max err / bound", (err / np.maximum(bound, 1e-300)).max())
    assert (err <= bound).all()                                                 # an entry whose terms are all zero must be exactly 0


@pytest.mark.parametrize("metric", ["point", "plane"])
def test_step_against_numpy_solve(mid_step, metric):
    (pose1, xi, sums, idx, d2, status), pose = mid_step[metric]["dev"], mid_step[metric]["pose"]
    A, g = R.system(sums[0])
    cond = np.linalg.cond(A)
    assert cond < 100 and status[0] == 1
    want = np.linalg.solve(A, g)
    bound = cond * 64 * EPS
    print(metric, "cond", cond, "xi err", np.linalg.norm(xi[0] - want) / np.linalg.norm(want), "bound", bound)
    assert np.linalg.norm(want) > 1e-3 and np.linalg.norm(xi[0] - want) <= bound * np.linalg.norm(want)
    p_ref = R.apply_step(pose, want)
    assert np.abs(pose1[0, :3].reshape(12) - p_ref).max() <= bound * np.abs(p_ref).max()
    assert np.array_equal(pose1[0, 3], [0, 0, 0, 1])


# ---- 5. lockstep --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("metric", ["point", "plane"])
def test_lockstep_with_the_reference(dev, scenes_S, metric):
    """12 single steps, each from the device's own previous pose: the correspondences equal the reference's at that pose and the new
    pose is one reference step from it, within the step test's bound - without asking two trajectories to agree"""
    sc = scenes_S[1]
    s, t, n = _t(sc["src"], dev), _t(sc["tgt"], dev), _t(sc["nrm"], dev) if metric == "plane" else None
    pose = R.IDENTITY.copy()
    for k in range(12):
        pose1, xi, sums, idx, d2, status = _np(*G.icp_step_dev(s, t, None, None, 0.05, metric, n, pose))
        e = R.evaluate(sc["src"], sc["tgt"], sc["nrm"], pose, 0.05, metric)
        assert np.array_equal(idx, e["idx"]) and np.array_equal(d2, e["d2"]) and sums[0, R.CNT] == e["sums"][R.CNT]
        want, _, st = R.step(pose, e["sums"], metric)
        cond = np.linalg.cond(R.system(e["sums"])[0])
        assert st == -1 and status[0] == 1 and cond < 100
        got = pose1[0, :3].reshape(12)
        assert np.abs(got - want).max() <= cond * 64 * EPS * np.abs(want).max(), (k, np.abs(got - want).max())
        one = _np(*G.icp_dev(s, t, None, None, 0.05, metric, n, init=pose, max_iter=1))
        assert np.array_equal(one[0][0], pose1[0]) and one[3][0] == 1 and one[4][0] == 1     # max_iter = 1 takes this very step
        pose = got
    eR, et = R.pose_error(pose, sc["R"], sc["t"])
    assert eR < 1e-4 and et < 1e-4                                              # and the steps went somewhere


# ---- 6. the full loop on scene S ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("metric", ["point", "plane"])
def test_full_loop_recovers_scene_S(dev, scenes_S, metric):
    pose, fitness, rmse, it, status = _run(dev, scenes_S, metric, [d for _, _, d in S_STARTS])
    for b, sc in enumerate(scenes_S):
        eR, et = R.pose_error(pose[b, :3].reshape(12), sc["R"], sc["t"])
        print(metric, S_STARTS[b], "iterations", it[b], "errR", eR, "errt", et, "rmse", rmse[b])
        assert status[b] == 0 and fitness[b] == 1.0 and rmse[b] < 1e-6
        assert eR <= 1e-6 and et <= 1e-6


# ---- 7. scenes H and D --------------------------------------------------------------------------------------------------------------

def test_scene_H_reaches_the_reference_fixed_point(dev, scenes_H):
    """Plane metric, max_dist = 0.05, six starts.  Every start of the reference reaches one fixed point (3.58e-3 from the true motion in
    R: the halves share 667 points): against the true motion the six results differ pairwise by at most 3.4e-8 (measured on the
    reference alone).  The device must end within 10 x that spread, computed here from the reference's six runs, of their mean; the
    margin allows the device another path into the same basin."""
    ref = [R.icp(sc["src"], sc["tgt"], 0.05, "plane", sc["nrm"]) for sc in scenes_H]
    assert all(r[4] == 0 for r in ref)
    rel = np.stack([_rel(R.pose44(r[0]), sc) for r, sc in zip(ref, scenes_H)])
    spread = max(np.abs(a - b).max() for a in rel for b in rel)
    assert 1e-9 < spread < 1e-7
    pose, fitness, rmse, it, status = _run(dev, scenes_H, "plane", 0.05)
    for b, sc in enumerate(scenes_H):
        dist = np.abs(_rel(pose[b], sc) - rel.mean(0)).max()
        print(H_STARTS[b], "iterations", it[b], "ref", ref[b][3], "dist", dist, "bound", 10 * spread)
        assert status[b] == 0 and dist <= 10 * spread


def test_scene_D_rmse(dev, scene_D):
    """Disjoint samples: the optimum is sampling-limited (rmse 1.87e-2, the pose about 1e-2 from the truth), so no pose is asserted.
    The reference's runs with rel_rmse = 1e-6 and 1e-9 end 4.2e-6 apart in rmse; the device's rmse must lie within twice that spread,
    computed here, of the 1e-6 run."""
    a = R.icp(scene_D["src"], scene_D["tgt"], 0.05, "point", max_iter=100)
    b = R.icp(scene_D["src"], scene_D["tgt"], 0.05, "point", max_iter=100, rel_fitness=1e-9, rel_rmse=1e-9)
    spread = abs(a[2] - b[2])
    assert a[4] == 0 and b[4] == 0 and 1e-7 < spread < 1e-4
    pose, fitness, rmse, it, status = _run(dev, [scene_D], "point", 0.05, max_iter=100)
    print("rmse", rmse[0], "ref", a[2], b[2], "iterations", it[0], a[3])
    assert status[0] == 0 and abs(rmse[0] - a[2]) <= 2 * spread


# ---- 8. determinism and freezing ----------------------------------------------------------------------------------------------------

def test_batch_equals_per_pair_calls_and_freezing(dev, scenes_S, scenes_H, scene_D):
    pairs = [scenes_S[0], scenes_S[2], scene_D, scenes_H[1]]
    metric, dist = ["plane", "point", "point", "plane"], [0.05, 0.1, 0.05, 0.05]
    base = _run(dev, pairs, metric, dist, max_iter=30)
    pose, fitness, rmse, it, status = base
    print("iterations", it, "status", status)
    assert len(set(it.tolist())) >= 3 and (status == 0).all()                   # the pairs end at different iterations
    for other in (_run(dev, pairs, metric, dist, max_iter=30), _run(dev, pairs, metric, dist, max_iter=30, check_every=1),
                  _run(dev, pairs, metric, dist, max_iter=30, check_every=30), _run(dev, pairs, metric, dist, max_iter=40)):
        for x, y in zip(base, other):
            assert np.array_equal(x, y)
    for b, sc in enumerate(pairs):                                              # a pair alone: the same bits
        for x, y in zip(base, _run(dev, [sc], metric[b], dist[b], max_iter=30)):
            assert np.array_equal(x[b:b + 1], y)
    short = _run(dev, pairs, metric, dist, max_iter=int(it.min()) + 1)          # some pairs run out of iterations, the first does not
    assert short[4][np.argmin(it)] == 0 and (short[4] == 1).sum() >= 2
    assert np.array_equal(short[0][np.argmin(it)], pose[np.argmin(it)])


# ---- 9. statuses --------------------------------------------------------------------------------------------------------------------

def test_statuses_and_unaffected_neighbours(dev, scenes_S):
    ok = scenes_S[0]
    g = np.stack(np.meshgrid(np.arange(4.), np.arange(4.), [0.0], indexing="ij"), -1).reshape(-1, 3).astype(np.float32) / 4
    up = np.tile(np.float32([0, 0, 1]), (16, 1))
    nan = lambda a, i: np.where(np.arange(a.size).reshape(a.shape) == i, np.float32(np.nan), a)
    small = dict(src=ok["src"][:50], tgt=ok["tgt"][:200], nrm=ok["nrm"][:200])
    pairs = [ok,
             dict(small, src=small["src"][:0]),                                 # 1: empty source
             dict(small, tgt=small["tgt"][:0], nrm=small["nrm"][:0]),           # 2: empty target
             dict(small, src=small["src"] + np.float32(10)),                    # 3: nothing within max_dist
             dict(src=g + np.float32([0, 0, 0.125]), tgt=g, nrm=up),            # 4: a coplanar dyadic target under the plane metric
             dict(small, src=nan(small["src"], 7)),                             # 5 - 8: a NaN in the source, target, normals, init
             dict(small, tgt=nan(small["tgt"], 301)),
             dict(small, nrm=nan(small["nrm"], 5)),
             dict(small),
             ok]
    B = len(pairs)
    init = np.tile(R.IDENTITY, (B, 1))
    init[4] = R.pose12(np.eye(3), [0.125, 0.25, 0])
    init[8, 5] = np.nan
    dist = [0.05] * B
    dist[4] = 1.0
    pose, fitness, rmse, it, status = _run(dev, pairs, "plane", dist, init=init)
    assert status.tolist() == [0, 2, 2, 2, 3, 4, 4, 4, 4, 0]
    for b in (1, 2, 3, 4, 5, 6, 7):                                             # the pose stays where it was
        assert np.array_equal(pose[b, :3].reshape(12), init[b])
    assert np.isnan(pose[8, 1, 1]) and fitness[4] == 1.0 and it[4] == 0
    assert (fitness[[1, 2, 3, 5, 6, 7, 8]] == 0).all() and (rmse[[1, 2, 3, 5, 6, 7, 8]] == 0).all()
    alone = _run(dev, [ok], "plane", 0.05)
    for x, y in zip((pose, fitness, rmse, it, status), alone):                  # the neighbours are unaffected
        assert np.array_equal(x[0:1], y) and np.array_equal(x[B - 1:B], y)
    assert _run(dev, [pairs[7]], "point", 0.05)[4][0] != 4                      # normals do not matter to a point pair


# ---- 10. wiring ---------------------------------------------------------------------------------------------------------------------

def test_evaluate_is_icp_without_iterations(dev, scenes_S):
    s, t, n, so, to = _pack(scenes_S, dev)
    init = np.stack([_mid_pose(sc, 0.9) for sc in scenes_S])
    fit, rmse, idx, d2 = _np(*G.evaluate_registration_dev(s, t, so, to, 0.05, init))
    pose, fit0, rmse0, it, status = _np(*G.icp_dev(s, t, so, to, 0.05, init=init, max_iter=0))
    assert np.array_equal(fit, fit0) and np.array_equal(rmse, rmse0) and (it == 0).all() and (status == 1).all()
    assert np.array_equal(pose[:, :3].reshape(3, 12), init) and (fit > 0).all() and (idx >= 0).all()


def test_multiscale_recovers_scene_S(dev, scenes_S):
    """three levels, the last with a voxel so small (1e-4) that it keeps every distinct point of both clouds"""
    s, t, _, so, to = _pack(scenes_S[:2], dev)
    for metric in ("point", "plane"):
        pose, fitness, rmse, it, status = _np(*G.icp_multiscale_dev(s, t, so, to, voxels=(0.08, 0.04, 1e-4), max_dists=(0.16, 0.08, 0.03),
                                                                    metric=metric))
        for b, sc in enumerate(scenes_S[:2]):
            eR, et = R.pose_error(pose[b, :3].reshape(12), sc["R"], sc["t"])
            print(metric, b, "errR", eR, "errt", et, "iterations", it[b])
            assert status[b] == 0 and eR <= 1e-6 and et <= 1e-6


def test_merge_scans(dev):
    """Three random 60 % subsets of the fixture, two of them moved by 5 and 10 degrees.  By the reference alone: the merged cloud is
    1.90e-5 from the fixture in Chamfer distance, the unregistered one 1.98e-3 (104 x); the reference's own runs with rel_rmse = 1e-5
    and 1e-6 end 8.7e-4 apart in relative Chamfer distance, which is the margin given to the device: 1e-3."""
    X = R.fixture()
    rs = np.random.RandomState(11)
    subs = [X[rs.permutation(len(X))[:1229]] for _ in range(3)]
    clouds = [subs[0]] + [R.moved(subs[i], *R.motion(i, 5 * i)) for i in (1, 2)]
    ref, ref_poses, ref_status = R.merge(clouds, 0.05, max_iter=60)
    c_ref, c_raw = R.chamfer(ref, X), R.chamfer(np.concatenate(clouds), X)
    assert ref_status.tolist() == [0, 0, 0] and c_raw >= 10 * c_ref
    merged, poses, status = G.merge_scans_dev([_t(c, dev) for c in clouds], max_dist=0.05, max_iter=60)
    merged, poses = merged.cpu().numpy(), poses.cpu().numpy()
    c_dev = R.chamfer(merged, X)
    print("chamfer device", c_dev, "reference", c_ref, "unregistered", c_raw)
    assert status.tolist() == [0, 0, 0] and merged.shape == (3 * 1229, 3) and np.array_equal(merged[:1229], clouds[0])
    assert np.array_equal(poses[0], np.eye(4))
    assert c_dev <= c_ref * (1 + 1e-3) and c_raw >= 10 * c_dev
    packed = G.merge_scans_dev(_t(np.concatenate(clouds), dev), _off([1229] * 3), voxel=0.02, max_dist=0.05, max_iter=60)
    assert np.array_equal(packed[1].cpu().numpy(), poses) and 0 < packed[0].shape[0] < 3 * 1229
    far = [clouds[0], clouds[1] + np.float32(10)]                               # a scan that cannot be registered is left out and reported
    m2, _, st2 = G.merge_scans_dev([_t(c, dev) for c in far], max_dist=0.05)
    assert st2.tolist() == [0, 2] and np.array_equal(m2.cpu().numpy(), clouds[0])
