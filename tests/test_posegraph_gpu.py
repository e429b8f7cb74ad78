"""Multiway registration on the device (csrc/posegraph.hip, shapeformer_amd/registration.py) against
tests/posegraph_ref.py.

What is exact is compared with `==`: the inlier count, a batch against per-pair / per-graph calls, two runs, the statuses, the kept
mask.  What is not has a derived bound:
  Lambda  |device - numpy| <= 4 n eps sum |term| per entry, n the inlier count (§5.18's bound: any two summation orders of n terms
          differ by at most 2 (n - 1) eps sum |term|);
  H, g    the same kind of bound over the edges: 4 (k + 100) eps sum_e l_e |J|^T |Lambda| |J| per entry, k the alive edges - the
          summation order, plus the ~40 products and sums inside one edge's block and the few eps of sin, cos, atan2 in J; for g the
          residual itself carries an absolute error of 32 eps (1 + the largest translation), which enters unscaled;
  delta   against numpy.linalg.solve on the device's own H + lambda I and g: cond x 64 eps relative (both solvers are backward stable);
  cost    c F plus what the residuals' absolute error can move it by (posegraph_ref.cost_slack);
  loop    the device's fixed point against the reference's on the same graph: 10 x the reference's own distance from the truth, the
          issue's margin; on graphs with exact edges both must reach the truth within 10 x tol (an accepted step below tol ends them).
"""
import numpy as np
import pytest
import torch

import icp_ref as R
import posegraph_ref as P
from shapeformer_amd import registration as G

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


def _off(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(*ts):
    return [t.cpu().numpy() for t in ts]


def _same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- 1. information matrices --------------------------------------------------------------------------------------------------------

def _info_pairs():
    """(src, tgt, pose, max_dist): the chunk edges, scene S, no inlier, one inlier at exactly max_dist and one just outside"""
    rs = np.random.RandomState(3)
    tgt = rs.uniform(-0.5, 0.5, (600, 3)).astype(np.float32)
    pairs = []
    for n in (1023, 1024, 1025, 4097):
        pose = P.random_pose(rs, 20, 0.1)
        want = tgt[rs.randint(0, 600, n)] + (rs.randn(n, 3) * 0.006).astype(np.float32)
        Tm = np.asarray(pose).reshape(3, 4)
        pairs.append((R.moved(want, Tm[:, :3], Tm[:, 3]), tgt, pose, 0.01))
    s = R.scene("S", 0, 5)
    pairs.append((s["src"], s["tgt"], R.pose12(s["R"], s["t"]), 0.05))
    pairs.append((tgt[:300] + np.float32(10), tgt, R.IDENTITY, 0.05))
    two = np.float32([[0, 0, 0], [5, 5, 5]])
    pairs.append((np.float32([[0.25, 0, 0]]), two, R.IDENTITY, 0.25))
    pairs.append((np.float32([[0.25, 0, 0]]), two, R.IDENTITY, float(np.nextafter(np.float32(0.25), np.float32(0)))))
    return pairs


def _info(dev, pairs):
    src, tgt = np.concatenate([p[0] for p in pairs]), np.concatenate([p[1] for p in pairs])
    so, to = _off([len(p[0]) for p in pairs]), _off([len(p[1]) for p in pairs])
    return _np(*G.information_matrix_dev(_t(src, dev), _t(tgt, dev), so, to, [p[3] for p in pairs], np.stack([p[2] for p in pairs]),
                                         details=True))


def test_information_counts_bounds_batch_and_runs(dev):
    pairs = _info_pairs()
    info, count, fit, rmse, flag = _info(dev, pairs)
    assert info.shape == (len(pairs), 6, 6) and count.dtype == np.int32 and not flag.any()
    worst = 0.0
    for b, (s, t, pose, md) in enumerate(pairs):
        ref, ab, n, rfit, _ = P.information(s, t, pose, md)
        assert count[b] == n and info[b, 5, 5] == n and info[b, 3, 3] == n and fit[b] == rfit
        assert np.array_equal(info[b], info[b].T)
        bound = 4 * n * EPS * ab
        assert (np.abs(info[b] - ref) <= bound).all()
        worst = max(worst, (np.abs(info[b] - ref) / np.where(bound > 0, bound, 1)).max())
        one = _info(dev, [pairs[b]])
        assert _same(one[0][0], info[b]) and one[1][0] == count[b]                 # a batch equals per-pair calls bit for bit
    print(f"information: worst |device - numpy| / bound = {worst:.4f}")
    assert count[:4].min() > 100 and count[4] == 700 and count[5] == 0 and count[6] == 1 and count[7] == 0
    assert not info[5].any() and np.array_equal(info[6], np.diag([0, 0, 0, 1.0, 1, 1]))
    again = _info(dev, pairs)
    assert all(_same(a, b) for a, b in zip(again, (info, count, fit, rmse, flag)))


def test_information_bad_pair_keeps_its_neighbours(dev):
    pairs = _info_pairs()[:3]
    good = _info(dev, pairs)
    src = pairs[1][0].copy()
    src[7, 2] = np.nan
    tgt = pairs[1][1].copy()
    tgt[599, 0] = np.inf
    pose = np.array(pairs[1][2])
    pose[5] = np.nan
    for bad in ((src, pairs[1][1], pairs[1][2], 0.01), (pairs[1][0], tgt, pairs[1][2], 0.01), (pairs[1][0], pairs[1][1], pose, 0.01)):
        info, count, fit, rmse, flag = _info(dev, [pairs[0], bad, pairs[2]])
        assert flag.tolist() == [0, 1, 0] and count[1] == 0 and not info[1].any() and fit[1] == 0
        for b in (0, 2):
            assert _same(info[b], good[0][b]) and count[b] == good[1][b]


# ---- 2. the optimiser ------------------------------------------------------------------------------------------------------------------

def _opt(dev, graphs, mu=0.0, alive=None, **kw):
    """a ragged batch of posegraph_ref.synthetic dicts -> numpy (X (S,12), l, cost, iterations, status, details)"""
    no, eo = _off([len(g["X0"]) for g in graphs]), _off([len(g["src"]) for g in graphs])
    cat = lambda k: np.concatenate([np.asarray(g[k]) for g in graphs])
    al = None if alive is None else np.concatenate([np.asarray(a) for a in alive]).astype(np.int32)
    out = G.pose_graph_optimize_dev(cat("X0"), cat("src"), cat("tgt"), _t(cat("T"), dev), _t(cat("Lam"), dev), cat("unc"), al, no, eo, mu,
                                    details=True, **kw)
    X, l, cost, it, st = _np(*out[:5])
    return X[:, :3, :].reshape(-1, 12), l, cost, it, st, {k: v.cpu().numpy() for k, v in out[5].items()}, no, eo


def _full(Hp, n):
    H = np.zeros((n, n))
    H[np.tril_indices(n)] = Hp[:n * (n + 1) // 2]
    return H + np.tril(H, -1).T


@pytest.mark.parametrize("S,mu,outliers", [(2, 0.0, 0), (3, 0.0, 0), (6, 0.0, 0), (6, 40.0, 3), (32, 0.0, 0)])
def test_one_iteration_against_the_reference(dev, S, mu, outliers):
    g = P.synthetic(S, seed=S, outliers=outliers)
    X, l, cost, it, st, d, _, _ = _opt(dev, [g], mu, max_iter=1)
    n, E = 6 * (S - 1), len(g["src"])
    assert st[0] in (0, 1) and it[0] == 1 and E == (496 if S == 32 else E)
    alive = np.ones(E, bool)
    _, _, lr, _ = P.evaluate(g["X0"], g["src"], g["tgt"], g["T"], g["Lam"], g["unc"] != 0, alive, mu)
    H, gv, Ha, Ga, Gr = P.normal_equations(g["X0"], g["src"], g["tgt"], g["T"], g["Lam"], alive, lr)
    Hd, gd, delta, lam = _full(d["H"][0], n), d["g"][0], d["delta"][0], d["lam"][0]
    c = 4 * (E + 100) * EPS
    assert (Ha > 0).all() and not d["H"][0][n * (n + 1) // 2:].any()              # a full graph: every block has an edge
    rH, rg = (np.abs(Hd - H) / (c * Ha)).max(), (np.abs(gd - gv) / (c * Ga + Gr)).max()
    print(f"S={S} mu={mu}: |H - ref| / bound = {rH:.4f}, |g - ref| / bound = {rg:.4f}")
    assert rH <= 1 and rg <= 1
    ratio = lam / (1e-5 * Hd.diagonal().max())                  # lambda: the start, doubled by every rejected try
    assert ratio >= 1 and np.log2(ratio) == np.round(np.log2(ratio))
    A = Hd + lam * np.eye(n)
    x, cond = np.linalg.solve(A, gd), np.linalg.cond(A)
    rd = np.abs(delta - x).max() / (cond * 64 * EPS * np.abs(x).max())
    print(f"S={S}: cond = {cond:.3g}, |delta - solve| / bound = {rd:.4f}")
    assert rd <= 1
    want = np.stack([g["X0"][0]] + [R.apply_step(g["X0"][k], delta[6 * (k - 1):6 * k]) for k in range(1, S)])
    assert np.abs(X - want).max() <= 32 * EPS * (1 + np.abs(want).max())          # the step is §5.18's, on the device's own delta
    if mu == 0:                                                 # the cost under the returned poses, on the device's own poses
        Fn, _, _, _ = P.evaluate(X, g["src"], g["tgt"], g["T"], g["Lam"], g["unc"] != 0, alive, mu)
        assert (l == 1).all() and abs(cost[0] - Fn) <= c * Fn + P.cost_slack(X, g["src"], g["tgt"], g["T"], g["Lam"], alive)


@pytest.mark.parametrize("S,noise", [(3, 1e-3), (6, 1e-3), (32, 1e-3), (6, 0.0), (32, 0.0)])
def test_full_loop_reaches_the_reference_fixed_point(dev, S, noise):
    g = P.synthetic(S, seed=10 + S, noise=noise)
    X, l, cost, it, st, _, _, _ = _opt(dev, [g])
    ref = P.optimize(g["X0"], g["src"], g["tgt"], g["T"], g["Lam"], g["unc"])
    assert st[0] == 0 and ref["status"] == 0 and 1 < it[0] < 30
    eR, et = P.graph_error(ref["X"], g["X_true"])
    dR, dt = P.graph_error(X, ref["X"])
    print(f"S={S} noise={noise}: iterations {it[0]} / {ref['iterations']}, reference from truth ({eR:.3g}, {et:.3g}), "
          f"device from reference ({dR:.3g}, {dt:.3g})")
    if noise:
        assert dR <= 10 * eR and dt <= 10 * et
    else:
        tR, tt = P.graph_error(X, g["X_true"])
        assert max(tR, tt, eR, et) <= 1e-9                      # 10 x tol: the accepted step that ended either loop was below tol


def _batch_graphs():
    """healthy | status 4 (a NaN transform) | healthy | status 2 (alive cuts node 2 off) | status 3 (an edge turned by 3.12 rad) |
    status 3 (an indefinite information matrix) | healthy | status 4 (a NaN pose)"""
    gs = [P.synthetic(6, seed=1, noise=1e-3), P.synthetic(4, seed=2), P.synthetic(3, seed=3, noise=1e-3), P.synthetic(5, seed=4),
          P.synthetic(4, seed=5), P.synthetic(3, seed=6), P.synthetic(2, seed=7, noise=1e-3), P.synthetic(3, seed=8)]
    alive = [np.ones(len(g["src"]), np.int32) for g in gs]
    gs[1]["T"][2, 7] = np.nan
    alive[3][(gs[3]["src"] == 2) | (gs[3]["tgt"] == 2)] = 0
    gs[4]["T"][1] = P.mul12(gs[4]["T"][1], R.pose12(R.rodrigues(np.array([0, 0, 3.12])), np.zeros(3)))
    gs[4]["X0"] = gs[4]["X_true"].copy()
    gs[5]["Lam"][0] = -gs[5]["Lam"][0] * 1e3
    gs[7]["X0"][1, 3] = np.inf
    return gs, alive, [0, 4, 0, 2, 3, 3, 0, 4]


def test_batch_equals_per_graph_calls_statuses_and_runs(dev):
    gs, alive, want = _batch_graphs()
    X, l, cost, it, st, d, no, eo = _opt(dev, gs, 0.0, alive)
    assert st.tolist() == want
    for b, g in enumerate(gs):
        ref = P.optimize(g["X0"], g["src"], g["tgt"], g["T"], g["Lam"], g["unc"], alive[b])
        assert ref["status"] == want[b]
        one = _opt(dev, [g], 0.0, [alive[b]])
        assert _same(one[0], X[no[b]:no[b + 1]]) and _same(one[1], l[eo[b]:eo[b + 1]])     # the bits of the graph's own call
        assert one[2][0].tobytes() == cost[b].tobytes() and one[3][0] == it[b] and one[4][0] == st[b]
        if want[b] in (2, 4):
            assert _same(X[no[b]:no[b + 1]], np.asarray(g["X0"], np.float64))               # the poses stay as given
        if want[b] == 4:
            assert not l[eo[b]:eo[b + 1]].any() and cost[b] == 0 and it[b] == 0
        if want[b] == 2:
            assert it[b] == 0 and (l[eo[b]:eo[b + 1]] == alive[b]).all()
    again = _opt(dev, gs, 0.0, alive)
    assert all(_same(a, b) for a, b in zip(again[:5], (X, l, cost, it, st)))


def test_single_node_and_max_iter_zero(dev):
    g = P.synthetic(1, seed=0)
    X, l, cost, it, st, _, _, _ = _opt(dev, [g])
    assert st.tolist() == [0] and it.tolist() == [0] and cost[0] == 0 and len(l) == 0 and _same(X, g["X0"])
    g = P.synthetic(4, seed=1)
    X, l, cost, it, st, _, _, _ = _opt(dev, [g, P.synthetic(1, seed=0)], max_iter=0)
    assert st.tolist() == [1, 0] and it.tolist() == [0, 0] and _same(X[:4], g["X0"])
    F, _, _, _ = P.evaluate(g["X0"], g["src"], g["tgt"], g["T"], g["Lam"], g["unc"] != 0, np.ones(6, bool), 0.0)
    assert abs(cost[0] - F) <= 4 * 106 * EPS * F + P.cost_slack(g["X0"], g["src"], g["tgt"], g["T"], g["Lam"], np.ones(6, bool))


def test_outlier_edges_are_pruned_as_the_reference_prunes(dev):
    gs = [P.synthetic(8, seed=1, outliers=3), P.synthetic(6, seed=2, outliers=3, noise=1e-3)]
    no, eo = _off([len(g["X0"]) for g in gs]), _off([len(g["src"]) for g in gs])
    cat = lambda k: np.concatenate([np.asarray(g[k]) for g in gs])
    poses, kept, l, s1, s2 = _np(*G.global_optimization_dev(cat("X0"), cat("src"), cat("tgt"), _t(cat("T"), dev), _t(cat("Lam"), dev),
                                                            cat("unc"), None, no, eo, max_dist=0.01))
    assert s1.tolist() == [0, 0] and s2.tolist() == [0, 0]
    for b, g in enumerate(gs):
        ref = P.global_optimization(g["X0"], g["src"], g["tgt"], g["T"], g["Lam"], g["unc"], max_dist=0.01)
        e = slice(eo[b], eo[b + 1])
        assert np.array_equal(kept[e], ref["kept"]) and not kept[e][-3:].any() and kept[e][:-3].all()
        assert (l[e][-3:] < 0.25).all() and (l[e][:-3] > 0.9).all() 
        eR, et = P.graph_error(ref["X"], g["X_true"])
        dR, dt = P.graph_error(poses[no[b]:no[b + 1], :3, :].reshape(-1, 12), ref["X"])
        print(f"pruned graph {b}: reference from truth ({eR:.3g}, {et:.3g}), device from reference ({dR:.3g}, {dt:.3g})")
        assert dR <= max(10 * eR, 1e-9) and dt <= max(10 * et, 1e-9)


# ---- 3. end to end on the ring scene -------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ring():
    sc = P.ring_scene()
    return sc, P.multiway(sc["clouds"])


def test_ring_scene_multiway_registration(dev, ring):
    sc, ref = ring
    clouds = [_t(c, dev) for c in sc["clouds"]]
    poses, status, more = G.multiway_registration_dev(clouds)
    assert status.tolist() == [0] * 6 and more["graph_status"] == (0, 0)
    reg = [tuple(e) for e, r in zip(more["edges"].tolist(), more["registered"]) if r]
    assert reg == ref["edges"] == [(0, 1), (0, 5), (1, 2), (2, 3), (3, 4), (4, 5)]
    assert more["kept"][more["registered"]].tolist() == ref["kept"].tolist() and more["kept"].sum() == 6
    eR, et = P.graph_error(ref["poses"], sc["X_true"])
    dR, dt = P.graph_error(poses.cpu().numpy()[:, :3, :].reshape(-1, 12), sc["X_true"])
    print(f"ring: reference from truth ({eR:.3g}, {et:.3g}), device from truth ({dR:.3g}, {dt:.3g})")
    assert dR <= 10 * eR and dt <= 10 * et


def test_ring_scene_merge_beats_the_star(dev, ring):
    sc, ref = ring
    clouds = [_t(c, dev) for c in sc["clouds"]]
    merged, poses, status = G.merge_scans_dev(clouds, multiway=dict(max_dists=(0.05, 0.01)))
    assert status.tolist() == [0] * 6 and merged.shape[0] == sum(len(c) for c in sc["clouds"])
    cd = R.chamfer(merged.cpu().numpy(), sc["fixture"])
    cd_ref = R.chamfer(np.concatenate([R.transform(c, p) for c, p in zip(sc["clouds"], ref["poses"])]), sc["fixture"])
    eR, et = P.graph_error(ref["poses"], sc["X_true"])
    reach = np.abs(sc["fixture"]).max() * np.sqrt(3)
    bound = 2 * (10 * (eR * reach + et)) ** 2                   # every merged point within 10 x the reference's pose error of its own
    print(f"ring merge: chamfer {cd:.3g}, reference merge {cd_ref:.3g}, bound {bound:.3g}")
    assert cd <= bound and cd_ref <= bound
    star, _, st = G.merge_scans_dev(clouds, max_dist=0.05)
    cd_star = R.chamfer(star.cpu().numpy(), sc["fixture"])
    print(f"ring merge: the star's chamfer {cd_star:.3g}, status {st.tolist()}")
    assert cd_star >= P.STAR_FACTOR * cd


def test_ring_scene_pairs_global_init_and_plane_metric(dev, ring, monkeypatch):
    """The options of multiway_registration_dev on the ring scene.  `pairs`: the six neighbouring pairs and (0,3), which shares nothing.
    `global_init`: the global registration is replaced by one that knows the true relative pose of every other pair (status 0) and
    reports status 1 with a useless pose for the rest, so the wiring is what is tested: both kinds of pairs must end where the plain
    call ends.  The plane metric has no reference run: a pose within 1e-2 of the truth is what the CPU test calls registered."""
    sc, ref = ring
    clouds = [_t(c, dev) for c in sc["clouds"]]
    pairs = [(0, 1), (0, 3), (0, 5), (1, 2), (2, 3), (3, 4), (4, 5)]
    eR, et = P.graph_error(ref["poses"], sc["X_true"])

    def fake(src, tgt, so, to, **kw):
        assert kw == dict(voxel=0.05) and len(so) == len(pairs) + 1
        pose = np.stack([R.pose44(P.mul12(P.inv12(sc["X_true"][i]), sc["X_true"][j])) for i, j in pairs])
        st = np.arange(len(pairs)) % 2
        pose[st == 1, :3, 3] += 5.0
        return (_t(pose, dev), None, None, None, None, None, _t(st.astype(np.int32), dev))

    monkeypatch.setattr(G, "global_registration_dev", fake)
    for kw in (dict(), dict(global_init=dict(voxel=0.05))):
        poses, status, more = G.multiway_registration_dev(clouds, pairs=pairs, **kw)
        assert status.tolist() == [0] * 6 and more["edges"].tolist() == [list(p) for p in pairs]
        assert more["registered"].tolist() == [True, False, True, True, True, True, True] == more["kept"].tolist()
        dR, dt = P.graph_error(poses.cpu().numpy()[:, :3, :].reshape(-1, 12), sc["X_true"])
        assert dR <= 10 * eR and dt <= 10 * et
    poses, status, more = G.multiway_registration_dev(clouds, pairs=pairs, metric="plane")
    dR, dt = P.graph_error(poses.cpu().numpy()[:, :3, :].reshape(-1, 12), sc["X_true"])
    print(f"ring, plane metric: device from truth ({dR:.3g}, {dt:.3g}), registered {more['registered'].tolist()}")
    assert status.tolist() == [0] * 6 and not more["registered"][1] and dR < 1e-2 and dt < 1e-2
    cut = G.multiway_registration_dev(clouds, pairs=[(0, 1), (1, 2), (4, 5)])                 # scans 3, 4, 5: no kept edge reaches them
    assert cut[1].tolist() == [0, 0, 0, 2, 2, 2] and _same(cut[0][3:].cpu().numpy(), np.tile(np.eye(4), (3, 1, 1)))
