"""GPU: every ragged-batch tool on the wide batches of tests/wide_batch.py (B = 261 sets, runs of empty sets, more sets than items)
against calls on each member alone.

For each tool and layout: one call on the batch, one call per distinct member, one call on a single empty set.  Every per-item slice and
every per-set value of the batch is compared BIT FOR BIT with the member-alone result - the tools promise it, so there is no tolerance
anywhere in that comparison.  The empty sets must equal the single-empty-set call, have zero-length ragged outputs, and hold the values
the docstrings name.  Then each tool's existing reference checker, with its existing bound, runs once per member on that member's slice
of the BATCH result, so a wrong-owner bug that is self-consistent still fails.

A runner takes the list of members a call holds (None: an empty set) and returns (items, sets): items {name: (array, (B+1,) offsets)}
are per-item or ragged outputs, sets {name: (B, ...) array} per-set outputs.  Inputs that a wrapper would draw per set on the host
(triples, cameras, viewpoints, poses) are fixed per MEMBER here and reach every call through the explicit argument.
"""
import numpy as np
import pytest
import torch
from scipy.spatial import cKDTree

import downsample_ref as DR
import knn_ref as KR
import segment_ref as SR
import wide_batch as W
from shapeformer_amd import hpr, meshsdf as MS, metrics as M, registration as G, scan

pytestmark = pytest.mark.gpu

E3 = np.zeros((0, 3), np.float32)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(v):
    return v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


def _off(parts):
    return np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)


def _cat(ms, pick=None, empty=E3):
    """the members' arrays (pick(m) of each, the member itself by default) back to back -> (array, offsets)"""
    parts = [empty if m is None else (m if pick is None else pick(m)) for m in ms]
    return np.concatenate(parts), _off(parts)


def _rows(ms, pick, empty):
    """one row per set: pick(m), `empty` for an empty set -> (B, ...) array"""
    return np.stack([np.asarray(empty) if m is None else np.asarray(pick(m)) for m in ms])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _host(res):
    items, sets = res
    return {k: (_np(v), np.asarray(o, np.int64)) for k, (v, o) in items.items()}, {k: _np(v) for k, v in sets.items()}


def _view(res, b):
    """everything the result holds for set b: {name: array}"""
    items, sets = res
    out = {k: v[o[b]:o[b + 1]] for k, (v, o) in items.items()}
    out.update({k: v[b] for k, v in sets.items()})
    return out


def run_case(dev, name, layout, run, members, literal=None, check=None, empty_alone=True):
    """the six steps of the module docstring for one tool and one layout"""
    row, lay = W.TOOLS[name], W.LAYOUTS[layout]
    sub = W.substitute_of(row, layout)
    which = lay.members(sub)
    assert len(members) == len(W.sizes_of(row, layout))
    batch = _host(run(dev, [members[m] if m >= 0 else None for m in which]))
    for k, (v, o) in batch[0].items():
        assert o.shape == (W.B + 1,) and o[0] == 0 and o[-1] == len(v) and (np.diff(o) >= 0).all(), k
    for k, v in batch[1].items():
        assert len(v) == W.B, k
    alone = {m: _host(run(dev, [members[m]])) for m in sorted(set(which[which >= 0].tolist()))}
    empty = _host(run(dev, [None])) if empty_alone and (which < 0).any() else None
    for b in range(W.B):
        got = _view(batch, b)
        if which[b] < 0:
            for k, (v, o) in batch[0].items():
                assert o[b + 1] == o[b], (name, b, k)
            if empty is not None:
                want = _view(empty, 0)
                for k in got:
                    assert same_bits(got[k], want[k]), (name, "empty set", b, k)
            if literal is not None:
                literal(got)
        else:
            want = _view(alone[which[b]], 0)
            assert sorted(got) == sorted(want)
            for k in got:
                assert same_bits(got[k], want[k]), (name, layout, "set", b, "member", int(which[b]), k)
    if check is not None:
        for m in alone:
            occ = lay.occurrences(m, sub)
            b = int(occ[occ >= 255][0]) if (occ >= 255).any() else int(occ[-1])      # members 3, 4, 5: the sets astride lane 256
            check(members[m], _view(batch, b))
    return batch


LAYOUT_NAMES = ["wide", "sparse"]


def _points(layout, name):
    return W.point_members(W.TOOLS[name].wide if layout == "wide" else W.TOOLS[name].sparse)


def _pairs(layout, name):
    return W.pair_members(W.TOOLS[name].wide if layout == "wide" else W.TOOLS[name].sparse)


# ---- metrics.nn_dist, scan.knn_dev -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", LAYOUT_NAMES)
@pytest.mark.parametrize("index", [False, True])
def test_nn_dist(dev, layout, index):
    from test_metrics_gpu import RTOL, ATOL, _truth
    name = "nn_dist_index" if index else "nn_dist"

    def run(dev, ms):
        (p, po), (q, qo) = _cat(ms, lambda m: m[0]), _cat(ms, lambda m: m[1])
        out = M.nn_dist(_t(p, dev), _t(q, dev), po, qo, return_index=index)
        return ({"d2": (out[0], po), "idx": (out[1], po)} if index else {"d2": (out, po)}), {}

    def check(m, got):
        t, ind = _truth(*m)
        d2 = got["d2"].astype(np.float64)
        assert (np.abs(d2 - t) <= RTOL * t + ATOL).all()
        if index:
            mine = ((m[0].astype(np.float64) - m[1].astype(np.float64)[got["idx"]]) ** 2).sum(1)
            assert ((got["idx"] == ind) | (np.abs(mine - t) <= RTOL * t + ATOL)).all()

    run_case(dev, name, layout, run, _pairs(layout, name), check=check)


@pytest.mark.parametrize("layout", LAYOUT_NAMES)
@pytest.mark.parametrize("k", [8, 33])
@pytest.mark.parametrize("exclude_self", [False, True])
def test_knn(dev, layout, k, exclude_self):
    name = f"knn_k{k}" + ("_exclude_self" if exclude_self else "")

    def run(dev, ms):
        if exclude_self:
            p, po = _cat(ms)
            pt = _t(p, dev)
            d2, idx = scan.knn_dev(pt, pt, k, po, po, exclude_self=True)
        else:
            (p, po), (q, qo) = _cat(ms, lambda m: m[0]), _cat(ms, lambda m: m[1])
            d2, idx = scan.knn_dev(_t(p, dev), _t(q, dev), k, po, qo)
        return {"d2": (d2, po), "idx": (idx, po)}, {}

    def check(m, got):
        KR.check_order(got["d2"], got["idx"])
        p, q = (m, m) if exclude_self else m
        KR.check_ranks(got["d2"], got["idx"], p, q, k, exclude_self=exclude_self)      # includes the (+inf, -1) tails of small sets

    run_case(dev, name, layout, run, _points(layout, name) if exclude_self else _pairs(layout, name), check=check)


# ---- scan: statistics over the neighbour table ---------------------------------------------------------------------------------------

def _self_d2(dev, m, k):
    """the device's own neighbour distances of one member (the rows the reference restatements of test_scan_gpu.py start from)"""
    pt = _t(m, dev)
    return scan.knn_dev(pt, pt, k, exclude_self=True)[0].cpu().numpy()


@pytest.mark.parametrize("layout", LAYOUT_NAMES)
def test_knn_mean_dist(dev, layout):
    def run(dev, ms):
        p, po = _cat(ms)
        return {"m": (scan.knn_mean_dist_dev(_t(p, dev), po, 8), po)}, {}

    def check(m, got):
        want = KR.mean_dist(_self_d2(dev, m, 8))
        fin = np.isfinite(want)
        assert np.array_equal(np.isposinf(got["m"]), ~fin) and np.allclose(got["m"][fin], want[fin], rtol=1e-13, atol=0)
        assert fin.all() == (len(m) >= 9)                                         # fewer than k + 1 points: +inf

    run_case(dev, "knn_mean_dist", layout, run, _points(layout, "knn_mean_dist"), check=check)


@pytest.mark.parametrize("layout", LAYOUT_NAMES)
def test_statistical_outlier_mask(dev, layout):
    from test_scan_gpu import _band_compare
    k, ratio = 16, 1.0

    def run(dev, ms):
        p, po = _cat(ms)
        keep, count, stat = scan.statistical_outlier_mask_dev(_t(p, dev), po, k=k, std_ratio=ratio)
        return {"keep": (keep, po), "stat": (stat, po)}, {"count": count}

    def literal(got):
        assert got["count"] == 0

    def check(m, got):
        want = KR.mean_dist(_self_d2(dev, m, k))
        fin = np.isfinite(want)
        assert np.array_equal(np.isposinf(got["stat"]), ~fin) and np.allclose(got["stat"][fin], want[fin], rtol=1e-13, atol=0)
        o = np.array([0, len(m)])
        _band_compare(got["keep"], want, KR.sor_threshold(want, o, k, ratio), "statistical")
        assert got["count"] == got["keep"].sum()
        if len(m) < k + 1:
            assert got["keep"].all()

    run_case(dev, "statistical_outlier_mask", layout, run, _points(layout, "statistical_outlier_mask"), literal, check)


@pytest.mark.parametrize("layout", LAYOUT_NAMES)
def test_radius_outlier_mask(dev, layout):
    radius, mn = 0.12, 4

    def run(dev, ms):
        p, po = _cat(ms)
        keep, count = scan.radius_outlier_mask_dev(_t(p, dev), po, radius, mn)
        return {"keep": (keep, po)}, {"count": count}

    def literal(got):
        assert got["count"] == 0

    def check(m, got):
        x = m.astype(np.float64)
        n = cKDTree(x).query_ball_point(x, radius, return_length=True) - 1
        t_mn = KR.tree_knn(x, x, mn + 1)[0][:, mn]
        r2 = radius ** 2
        band = np.abs(t_mn - r2) <= 1e-9 * r2
        assert band.mean() <= 1e-3
        assert np.array_equal(got["keep"][~band].astype(bool), (n >= mn)[~band]) and got["count"] == got["keep"].sum()

    run_case(dev, "radius_outlier_mask", layout, run, _points(layout, "radius_outlier_mask"), literal, check)


VIEW, CAMS = W.VIEW, W.CAMS


@pytest.mark.parametrize("layout", LAYOUT_NAMES)
@pytest.mark.parametrize("viewpoint", [False, True])
def test_estimate_normals(dev, layout, viewpoint):
    name = "estimate_normals_viewpoint" if viewpoint else "estimate_normals"
    k = 16
    members = [(x, VIEW[i]) for i, x in enumerate(_points(layout, name))]

    def run(dev, ms):
        p, po = _cat(ms, lambda m: m[0])
        view = _rows(ms, lambda m: m[1], np.zeros(3)) if viewpoint else None
        normal, var = scan.estimate_normals_dev(_t(p, dev), po, k, viewpoint=view)
        return {"normal": (normal, po), "variation": (var, po)}, {}

    def check(m, got):
        x, v = m
        n, var = got["normal"].astype(np.float64), got["variation"].astype(np.float64)
        if len(x) < 3:                                                            # fewer than 3 neighbours: (0,0,0) and NaN
            assert np.all(n == 0) and np.isnan(var).all()
            return
        xt = _t(x, dev)
        tab = scan.knn_dev(xt, xt, k)[1].cpu().numpy()
        vec, lam = KR.pca_normals(x, tab)
        ok = (lam[:, 1] - lam[:, 0]) / lam[:, 2] >= 0.05
        assert (~ok).mean() <= 0.01 and np.all(KR.angle(n, vec)[ok] <= 1e-5)
        assert np.all(np.abs(np.linalg.norm(n, axis=1) - 1) <= 1e-6)
        want = lam[:, 0] / lam.sum(1)
        assert np.all(np.abs(var - want) <= 1e-5 * want + 1e-9)
        if viewpoint:
            assert np.all((n * (v[None] - x.astype(np.float64))).sum(1) >= 0)
        else:
            assert np.all(np.abs(n).max(1) == n.max(1))

    run_case(dev, name, layout, run, members, check=check)


@pytest.mark.parametrize("layout", LAYOUT_NAMES)
@pytest.mark.parametrize("anchor", ["outward", "viewpoint"])
def test_orient_normals(dev, layout, anchor):
    import orient_ref as OR
    name = f"orient_normals_{anchor}"
    k = 8
    row = W.TOOLS[name]
    members = W.orient_members(row.wide if layout == "wide" else row.sparse)

    def run(dev, ms):
        p, po = _cat(ms, lambda m: m[0])
        n, _ = _cat(ms, lambda m: m[1])
        view = _rows(ms, lambda m: m[2], np.zeros(3)) if anchor == "viewpoint" else None
        out, r = scan.orient_normals_dev(_t(p, dev), _t(n, dev), po, k=k, anchor=anchor, viewpoint=view, details=True)
        items = {"normal": (out, po)}
        items.update({key: (r[key], po) for key in ("component", "tree", "parity", "votes")})
        return items, {"rounds": r["rounds"], "n_components": r["n_components"]}

    def literal(got):
        assert got["rounds"] == 0 and got["n_components"] == 0

    def check(m, got):
        """tests/orient_ref.py on the device's own neighbour table: forest, parity, votes and normals exactly, as test_orient_gpu.py"""
        x, n, v = m
        xt = _t(x, dev)
        tab = scan.knn_dev(xt, xt, k)[1].cpu().numpy()
        want = OR.orient(x, n, tab, anchor=anchor, viewpoint=v if anchor == "viewpoint" else None)
        assert want["margin"] >= 1e-9                    # no vote hangs on the last bits of the centroid
        for key in ("normal", "component", "parity", "votes"):
            assert np.array_equal(got[key], want[key]), key
        assert got["n_components"] == want["n_components"][0]
        tree = got["tree"][got["tree"][:, 0] >= 0]
        assert {(int(a), int(b)) for a, b in tree} == want["tree"][0] and len(tree) == len(want["tree"][0])
        assert np.all(got["tree"][got["tree"][:, 0] < 0] == -1)

    run_case(dev, name, layout, run, members, literal, check)


# ---- scan: downsampling ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", LAYOUT_NAMES)
def test_farthest_point_sample(dev, layout):
    n = 16

    def run(dev, ms):
        p, po = _cat(ms)
        idx, d2, count, status = scan.farthest_point_sample_dev(_t(p, dev), po, n)
        return {}, {"idx": idx, "d2": d2, "count": count, "status": status}

    def literal(got):                                                             # status 1: no candidate, the row is all tail (-1, 0.0)
        assert got["status"] == 1 and got["count"] == 0 and np.all(got["idx"] == -1) and np.all(got["d2"] == 0)

    def check(m, got):
        assert got["status"] == 0
        DR.check_greedy(m, got["idx"], got["d2"], got["count"])

    run_case(dev, "farthest_point_sample", layout, run, _points(layout, "farthest_point_sample"), literal, check)


@pytest.mark.parametrize("layout", LAYOUT_NAMES)
@pytest.mark.parametrize("pick", ["centroid", "first"])
def test_voxel_downsample(dev, layout, pick):
    name, voxel = f"voxel_downsample_{pick}", 0.11

    def run(dev, ms):
        p, po = _cat(ms)
        out, out_off, first, count = scan.voxel_downsample_dev(_t(p, dev), po, voxel, pick)
        return {"out": (out, out_off), "first": (first, out_off), "count": (count, out_off)}, {"voxels": np.diff(out_off)}

    def check(m, got):
        want, wfirst, wcount = DR.voxel_down(m, voxel, pick)
        assert got["voxels"] == len(want) and np.array_equal(got["first"], wfirst) and np.array_equal(got["count"], wcount)
        if pick == "first":
            assert np.array_equal(got["out"], m[wfirst])
        else:
            assert DR.ulps(got["out"], want).max(initial=0) <= 1

    run_case(dev, name, layout, run, _points(layout, name), check=check)             # an empty set yields no voxels: run_case's zero length


# ---- scan: planes and clusters -------------------------------------------------------------------------------------------------------------

H_PLANE, THR = 32, 0.02


@pytest.mark.parametrize("layout", LAYOUT_NAMES)
def test_segment_plane(dev, layout):
    members = [(x, scan.plane_hypotheses([len(x)], H_PLANE, seed=i)[0]) for i, x in enumerate(_points(layout, "segment_plane"))]

    def run(dev, ms):
        p, po = _cat(ms, lambda m: m[0])
        triples = _rows(ms, lambda m: m[1], np.zeros((H_PLANE, 3), np.int32))
        plane, inlier, n_in, count, best, status = scan.segment_plane_dev(_t(p, dev), po, THR, triples=triples)
        return {"inlier": (inlier, po)}, {"plane": plane, "n_in": n_in, "count": count, "best": best, "status": status}

    def literal(got):                                    # no valid hypothesis: status 1, best -1, count -1; no winner: plane NaN, n_in 0
        assert got["status"] == 1 and got["best"] == -1 and np.all(got["count"] == -1) and np.isnan(got["plane"]).all() and got["n_in"] == 0

    def check(m, got):
        x, tr = m
        count, best, status = SR.plane_score_set(x, tr, THR)
        assert np.array_equal(got["count"], count) and got["best"] == best and got["status"] == status
        if best >= 0:
            plane, mask, n_in, dist, gap = SR.plane_refit_set(x, tr[best], THR)
            if n_in >= 3 and gap > 0.05:                  # test_segment_gpu.py's bound on the refit: 1e-9 per coefficient
                assert np.all(np.abs(got["plane"] - plane) <= 1e-9)
                near = np.abs(np.abs(dist) - THR) <= 1e-9
                assert np.array_equal(got["inlier"][~near].astype(bool), mask[~near]) and abs(int(got["n_in"]) - n_in) <= near.sum()
        else:
            assert np.isnan(got["plane"]).all() and got["n_in"] == 0 and not got["inlier"].any()

    run_case(dev, "segment_plane", layout, run, members, literal, check)


@pytest.mark.parametrize("layout", LAYOUT_NAMES)
def test_refit_plane(dev, layout):
    seeds = np.array([[0, 1, 0, 0.0], [0, 0, 2, 0.1], [1, 1, 0, 0.0], [0, 1, 0, -0.3], [1, 0, 0, 0.0], [0, 0, 1, 0.4]], np.float64)
    members = [(x, seeds[i]) for i, x in enumerate(_points(layout, "refit_plane"))]
    thr = 0.05

    def run(dev, ms):
        p, po = _cat(ms, lambda m: m[0])
        plane, inlier, n_in = scan.refit_plane_dev(_t(p, dev), po, _rows(ms, lambda m: m[1], seeds[0]), thr)
        return {"inlier": (inlier, po)}, {"plane": plane, "n_in": n_in}

    def literal(got):                                    # fewer than 3 seed inliers: plane NaN, n_in 0
        assert np.isnan(got["plane"]).all() and got["n_in"] == 0

    def check(m, got):
        x, s = m
        nn = (s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]
        plane, mask, n_in, dist, gap = SR.plane_refit_seed(x, s[:3], -s[3], nn, thr)
        if n_in >= 3 and gap > 0.05:
            assert np.all(np.abs(got["plane"] - plane) <= 1e-9)
            near = np.abs(np.abs(dist) - thr) <= 1e-9
            assert np.array_equal(got["inlier"][~near].astype(bool), mask[~near])
        elif n_in < 3:
            assert np.isnan(got["plane"]).all() and got["n_in"] == 0 and not got["inlier"].any()

    run_case(dev, "refit_plane", layout, run, members, literal, check)


@pytest.mark.parametrize("layout", LAYOUT_NAMES)
def test_euclidean_clusters(dev, layout):
    radius = 0.09

    def run(dev, ms):
        p, po = _cat(ms)
        label, sizes, c_off, root = scan.euclidean_clusters_dev(_t(p, dev), po, radius, min_points=2, return_root=True)
        return {"label": (label, po), "root": (root, po), "sizes": (sizes, c_off)}, {"clusters": np.diff(c_off)}

    def check(m, got):
        root = SR.cluster_roots(m, radius)
        assert np.array_equal(got["root"], root)
        label, sizes = SR.cluster_labels(root, 2)
        assert np.array_equal(got["label"], label) and np.array_equal(got["sizes"], sizes) and got["clusters"] == len(sizes)

    run_case(dev, "euclidean_clusters", layout, run, _points(layout, "euclidean_clusters"), check=check)


# ---- registration: ICP and its parts -------------------------------------------------------------------------------------------------------

IDENTITY = np.eye(4)
MAX_DIST = 0.08


def _poses(n, seed=400, **kw):
    return [W.rigid(seed + i, **kw) for i in range(n)]


@pytest.mark.parametrize("layout", LAYOUT_NAMES)
def test_transform_points(dev, layout):
    import icp_ref as IR
    members = [(x, T) for x, T in zip(_points(layout, "transform_points"), _poses(6, angle=0.7, shift=0.3))]

    def run(dev, ms):
        p, po = _cat(ms, lambda m: m[0])
        return {"out": (G.transform_points_dev(_t(p, dev), po, _rows(ms, lambda m: m[1], IDENTITY)), po)}, {}

    def check(m, got):
        assert np.array_equal(got["out"], IR.transform(m[0], IR.pose12(m[1][:3, :3], m[1][:3, 3])))

    run_case(dev, "transform_points", layout, run, members, check=check)


def _pair_batch(dev, ms):
    (s, so), (t, to) = _cat(ms, lambda m: m[0]), _cat(ms, lambda m: m[1])
    return _t(s, dev), _t(t, dev), so, to


@pytest.mark.parametrize("layout", LAYOUT_NAMES)
def test_evaluate_registration(dev, layout):
    import icp_ref as IR
    members = [p + (T,) for p, T in zip(_pairs(layout, "evaluate_registration"), _poses(6, angle=0.02, shift=0.005))]

    def run(dev, ms):
        s, t, so, to = _pair_batch(dev, ms)
        fitness, rmse, idx, d2 = G.evaluate_registration_dev(s, t, so, to, MAX_DIST, _rows(ms, lambda m: m[2], IDENTITY))
        return {"idx": (idx, so), "d2": (d2, so)}, {"fitness": fitness, "rmse": rmse}

    def literal(got):
        assert got["fitness"] == 0 and got["rmse"] == 0

    def check(m, got):
        s, t, T = m
        ridx, rd2 = IR.nn(IR.transform(s, IR.pose12(T[:3, :3], T[:3, 3])), t)       # test_icp_gpu.py's _check_corr for one pair
        assert np.array_equal(got["idx"], ridx) and np.array_equal(got["d2"], rd2)
        inl = rd2 <= IR.maxd2_of(MAX_DIST)
        assert got["fitness"] == inl.sum() / len(ridx)
        want = np.sqrt(rd2[inl].astype(np.float64).sum() / inl.sum()) if inl.any() else 0.0
        assert got["rmse"] == pytest.approx(want, rel=1e-13)

    run_case(dev, "evaluate_registration", layout, run, members, literal, check)


@pytest.mark.parametrize("layout", LAYOUT_NAMES)
@pytest.mark.parametrize("metric", ["point", "plane"])
def test_icp(dev, layout, metric):
    import icp_ref as IR
    name = f"icp_{metric}"
    members = []
    for i, ((s, t), T) in enumerate(zip(_pairs(layout, name), _poses(6, angle=0.01, shift=0.003))):
        # unit normals "used as given": random ones, so that the plane metric's 6 x 6 system is well conditioned (radial normals of a
        # sphere leave the turn about its centre unobservable)
        n = np.random.RandomState(500 + i).randn(len(t), 3)
        members.append((s, t, T, (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)))

    def run(dev, ms):
        s, t, so, to = _pair_batch(dev, ms)
        nrm = _t(_cat(ms, lambda m: m[3])[0], dev) if metric == "plane" else None
        pose, fitness, rmse, it, status = G.icp_dev(s, t, so, to, MAX_DIST, metric, nrm, _rows(ms, lambda m: m[2], IDENTITY), max_iter=3)
        return {}, {"pose": pose, "fitness": fitness, "rmse": rmse, "iterations": it, "status": status}

    def literal(got):                                    # fewer than 3 / 6 inliers: status 2, the pose stays where it was
        assert got["status"] == 2 and np.array_equal(got["pose"], IDENTITY) and got["fitness"] == 0

    def check(m, got):
        s, t, T, n = m
        want = IR.icp(s, t, MAX_DIST, metric, n if metric == "plane" else None, IR.pose12(T[:3, :3], T[:3, 3]), max_iter=3)
        _icp_compare(IR, want, got)

    run_case(dev, name, layout, run, members, literal, check)


def _icp_compare(IR, want, got):
    """icp_dev against icp_ref.icp for one pair after at most 3 steps.  Status, iterations and fitness (a count over the source
    points) exactly.  Pose and rmse to 1e-9: both sides solve the same 6 x 6 system in f64 from sums of at most 300 terms taken in
    different orders (relative 300 eps = 3e-14 of sum |term|); with the condition of these members' systems below 1e4 a step moves
    by at most 1e-9 of the pose's size, and three steps stay inside 1e-9 absolute on entries of size <= 1."""
    pose, fitness, rmse, it, status = want[:5]
    assert got["status"] == status and got["iterations"] == it and got["fitness"] == fitness
    assert np.all(np.abs(got["pose"] - IR.pose44(np.asarray(pose))) <= 1e-9) and abs(got["rmse"] - rmse) <= 1e-9


@pytest.mark.parametrize("layout", LAYOUT_NAMES)
def test_information_matrix(dev, layout):
    members = [p + (T,) for p, T in zip(_pairs(layout, "information_matrix"), _poses(6, angle=0.02, shift=0.005))]

    def run(dev, ms):
        s, t, so, to = _pair_batch(dev, ms)
        info, count, fitness, rmse, flag = G.information_matrix_dev(s, t, so, to, MAX_DIST, _rows(ms, lambda m: m[2], IDENTITY), details=True)
        return {}, {"info": info, "count": count, "fitness": fitness, "rmse": rmse, "flag": flag}

    def literal(got):
        assert got["count"] == 0 and np.all(got["info"] == 0) and got["flag"] == 0

    def check(m, got):
        import icp_ref as IR
        import posegraph_ref as PR
        s, t, T = m
        ref, ab, n, rfit, _ = PR.information(s, t, IR.pose12(T[:3, :3], T[:3, 3]), MAX_DIST)      # test_posegraph_gpu.py's comparison
        assert got["count"] == n and got["info"][5, 5] == n and got["info"][3, 3] == n and got["fitness"] == rfit
        assert np.array_equal(got["info"], got["info"].T)
        assert (np.abs(got["info"] - ref) <= 4 * n * np.finfo(np.float64).eps * ab).all()

    run_case(dev, "information_matrix", layout, run, members, literal, check)


# ---- hidden point removal ----------------------------------------------------------------------------------------------------------------



@pytest.mark.parametrize("layout", LAYOUT_NAMES)
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_hidden_point_mask(dev, layout, dtype):
    from test_hpr_gpu import check_against_scipy
    name = f"hidden_point_mask_{dtype}"
    members = [(x.astype(np.float64) if dtype == "f64" else x, CAMS[i]) for i, x in enumerate(_points(layout, name))]

    def run(dev, ms):
        p, po = _cat(ms, lambda m: m[0], members[0][0][:0])
        vis, count, status = hpr.hidden_point_mask_dev(_t(p, dev), _rows(ms, lambda m: m[1], CAMS[0]), po)
        return {"visible": (vis, po)}, {"count": count, "status": status}

    def literal(got):
        assert got["count"] == 0

    def check(m, got):
        x, cam = m
        assert got["count"] == got["visible"].sum()
        if len(x) >= 4:                                   # qhull needs a simplex: 4 flipped points and the viewpoint
            check_against_scipy(x, cam, got["visible"], name)                       # its cap: ceil(0.001 n) rows may differ

    run_case(dev, name, layout, run, members, literal, check)


@pytest.mark.parametrize("layout", LAYOUT_NAMES)
def test_resample_visible(dev, layout):
    """virtual_scan_dev = hidden_point_mask_dev + resample_visible_dev.  Shape b is seeded by (seed, shape0 + b), so the alone call of a
    member is made for ONE of its sets with shape0 = that set's index, and the draw is compared there; the visible counts are compared
    at every set."""
    ctx, noise = 8, 0.01
    lay, row = W.LAYOUTS[layout], W.TOOLS["resample_visible"]
    members = [(x, CAMS[i]) for i, x in enumerate(_points(layout, "resample_visible"))]
    which = lay.members()
    p, po = _cat([members[m] if m >= 0 else None for m in which], lambda m: m[0])
    cams = _rows([members[m] if m >= 0 else None for m in which], lambda m: m[1], CAMS[0])
    out, c, count = hpr.virtual_scan_dev(_t(p, dev), ctx, noise=noise, seed=5, cams=cams, off=po)
    assert out.shape == (W.B, ctx, 3) and np.array_equal(c, cams)
    out, count = out.cpu().numpy(), count.cpu().numpy()
    for m in sorted(set(which[which >= 0].tolist())):
        occ = lay.occurrences(m)
        b = int(occ[occ >= 255][0]) if (occ >= 255).any() else int(occ[-1])
        x, cam = members[m]
        o1, _, c1 = hpr.virtual_scan_dev(_t(x, dev), ctx, noise=noise, seed=5, cams=cam[None], off=[0, len(x)], shape0=b)
        assert same_bits(o1.cpu().numpy()[0], out[b]), (m, b)
        assert np.all(count[occ] == int(c1[0]))
        rows = out[b].astype(np.float64)
        assert np.isfinite(rows).all() and np.abs(rows).max() <= 1.0
        d = np.sqrt(((rows[:, None, :] - x.astype(np.float64)[None]) ** 2).sum(-1)).min(1)
        assert d.max() <= 6 * noise * np.sqrt(3)          # every row is a point of the shape plus the jitter (6 sigma per axis)
    for b in lay.empty:                                   # an empty shape has nothing to draw from: NaN rows, count 0
        assert np.isnan(out[b]).all() and count[b] == 0
    o0, _, c0 = hpr.virtual_scan_dev(_t(E3, dev), ctx, noise=noise, seed=5, cams=CAMS[:1], off=[0, 0], shape0=lay.empty[0])
    assert np.isnan(o0.cpu().numpy()).all() and int(c0[0]) == 0


# ---- registration: features and RANSAC over correspondences --------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", LAYOUT_NAMES)
def test_fpfh(dev, layout):
    import global_reg_ref as GR
    from test_global_reg_gpu import _ulp_close
    k = 16
    members = W.orient_members(W.sizes_of(W.TOOLS["fpfh"], layout))

    def run(dev, ms):
        p, po = _cat(ms, lambda m: m[0])
        n, _ = _cat(ms, lambda m: m[1])
        feat, spfh, m = G.fpfh_dev(_t(p, dev), _t(n, dev), po, k)
        return {"feature": (feat, po), "spfh": (spfh, po), "m": (m, po)}, {}

    def check(mem, got):                                  # test_global_reg_gpu.py's _check_fpfh for one set; the 1 % cap on marginal
        x, n, _ = mem                                     # points holds with 0 by the reference alone (test_wide_batch_cpu.py)
        d2, idx = GR.knn(x, k)
        counts, rm, marg = GR.spfh(x, n, idx, d2, None)
        assert marg.mean() <= 0.01
        assert np.array_equal(got["spfh"][~marg], counts[~marg]) and np.array_equal(got["m"][~marg], rm[~marg])
        assert (got["spfh"].sum(1) == 3 * got["m"]).all()
        assert _ulp_close(got["feature"], GR.fpfh_from_spfh(got["spfh"], got["m"], idx, d2, None)).all()

    run_case(dev, "fpfh", layout, run, members, check=check)


@pytest.mark.parametrize("layout", LAYOUT_NAMES)
@pytest.mark.parametrize("splits,q", [(1, 2), (3, 4)])
def test_match_features(dev, layout, splits, q):
    import global_reg_ref as GR
    name = f"match_features_s{splits}_q{q}"
    members = W.feature_members(W.sizes_of(W.TOOLS[name], layout))
    E33 = np.zeros((0, 33), np.float32)

    def run(dev, ms):
        (fs, so), (ft, to) = _cat(ms, lambda m: m[0], E33), _cat(ms, lambda m: m[1], E33)
        corr, c_off, idx, d2 = G.match_features_dev(_t(fs, dev), _t(ft, dev), so, to, mutual=True, splits=splits, queries_per_lane=q)
        return {"corr": (corr, c_off), "idx": (idx, so), "d2": (d2, so)}, {"matches": np.diff(c_off)}

    def check(m, got):
        ridx, rd2 = GR.feature_nn(*m)
        assert np.array_equal(got["idx"], ridx) and np.array_equal(got["d2"], rd2)
        back, _ = GR.feature_nn(m[1], m[0])
        keep = np.nonzero((ridx >= 0) & (back[np.maximum(ridx, 0)] == np.arange(len(ridx))))[0]
        assert np.array_equal(got["corr"], np.stack([keep, ridx[keep]], 1)) and got["matches"] == len(keep)
        assert len(keep) >= min(len(m[0]), len(m[1])) // 2                           # the planted mutual matches

    run_case(dev, name, layout, run, members, check=check)


EC = np.zeros((0, 2), np.int32)
H_CORR = 16


def _corr_batch(dev, ms):
    (s, so), (t, to), (c, co) = _cat(ms, lambda m: m[0]), _cat(ms, lambda m: m[1]), _cat(ms, lambda m: m[2], EC)
    triples = _rows(ms, lambda m: m[3], np.zeros((H_CORR, 3), np.int32))
    return (_t(s, dev), _t(t, dev), so, to, _t(c, dev), co), triples, co


@pytest.mark.parametrize("layout", LAYOUT_NAMES)
def test_hypothesis_poses(dev, layout):
    import global_reg_ref as GR
    members = W.corr_members(W.sizes_of(W.TOOLS["hypothesis_poses"], layout), H=H_CORR)

    def run(dev, ms):
        args, triples, _ = _corr_batch(dev, ms)
        poses, valid = G.hypothesis_poses_dev(*args, triples=triples, similarity=0.9)
        return {}, {"poses": poses, "valid": valid}

    def literal(got):                                     # no correspondence: every index lies outside, every hypothesis is invalid
        assert not got["valid"].any() and np.isnan(got["poses"]).all()

    def check(m, got):
        s, t, corr, tr = m
        ok, rp, S = GR.hypothesis_poses(s, t, corr, tr, 0.9)
        assert np.array_equal(got["valid"].astype(bool), ok) and np.isnan(got["poses"][~ok]).all()
        if ok.any():                                      # test_global_reg_gpu.py's bound: 64 eps x the ratio of the singular values
            ratio = S[ok, 0] / S[ok, 1]
            assert (np.abs(got["poses"][ok] - rp[ok]).max(1) <= 64 * np.finfo(np.float64).eps * ratio).all()

    run_case(dev, "hypothesis_poses", layout, run, members, literal, check)


@pytest.mark.parametrize("layout", LAYOUT_NAMES)
def test_score_poses(dev, layout):
    import global_reg_ref as GR
    import icp_ref as IR
    members = []
    for i, (s, t, corr, tr) in enumerate(W.corr_members(W.sizes_of(W.TOOLS["score_poses"], layout), H=H_CORR)):
        truth = W.rigid(700 + i, angle=0.4, shift=0.2)     # corr_members' motion, and three others
        poses = np.stack([IR.pose12(T[:3, :3], T[:3, 3]) for T in [truth] + _poses(3, 800 + 10 * i, angle=0.3, shift=0.1)])
        members.append((s, t, corr, tr, poses))

    def run(dev, ms):
        args, _, _ = _corr_batch(dev, ms)
        poses = _rows(ms, lambda m: m[4], np.tile(IR.IDENTITY, (4, 1)))
        return {}, {"count": G.score_poses_dev(*args, max_dist=0.03, poses=poses)}

    def literal(got):
        assert np.all(got["count"] == 0)

    def check(m, got):
        s, t, corr, _, poses = m
        assert np.array_equal(got["count"], GR.score(s, t, corr, poses, 0.03))
        assert len(corr) < 3 or got["count"][0] >= 0.7 * len(corr)                   # the true motion keeps the unscrambled ones

    run_case(dev, "score_poses", layout, run, members, literal, check)


@pytest.mark.parametrize("layout", LAYOUT_NAMES)
def test_ransac_correspondences(dev, layout):
    import global_reg_ref as GR
    import icp_ref as IR
    members = W.corr_members(W.sizes_of(W.TOOLS["ransac_correspondences"], layout), H=H_CORR)

    def run(dev, ms):
        args, triples, co = _corr_batch(dev, ms)
        pose, fitness, inlier, n_in, count, best, status = G.ransac_correspondences_dev(*args, max_dist=0.03, triples=triples)
        return {"inlier": (inlier, co)}, {"pose": pose, "fitness": fitness, "n_in": n_in, "count": count, "best": best, "status": status}

    def literal(got):                                     # fewer than 3 correspondences: status 1, the pose is the identity
        assert got["status"] == 1 and np.array_equal(got["pose"], IDENTITY) and got["best"] == -1 and np.all(got["count"] == -1)
        assert got["fitness"] == 0 and got["n_in"] == 0

    def check(m, got):
        s, t, corr, tr = m
        ref = GR.ransac(s, t, corr, 0.03, triples=tr)
        assert got["status"] == ref["status"] and got["best"] == ref["best"] and np.array_equal(got["count"], ref["count"])
        assert np.array_equal(got["inlier"].astype(bool), ref["inlier"]) and got["n_in"] == ref["n_in"] and got["fitness"] == ref["fitness"]
        # the refit is a Kabsch fit over the inliers in f64 on both sides: test_global_reg_gpu.py allows it 1e-12
        assert np.abs(got["pose"] - IR.pose44(ref["pose"])).max() <= 1e-12

    run_case(dev, "ransac_correspondences", layout, run, members, literal, check)


@pytest.mark.parametrize("layout", LAYOUT_NAMES)
def test_pose_graph_optimize(dev, layout):
    """An empty graph is refused (node 0 is the frame of the result), so the one-node graph without edges stands in the empty slots."""
    import posegraph_ref as P
    members = W.graph_members(W.GRAPH_NODES if layout == "wide" else W.SPARSE_GRAPH_NODES)

    def run(dev, ms):
        cat = lambda key, width: np.concatenate([np.asarray(g[key]).reshape((-1,) + width) for g in ms])
        no, eo = _off([g["X0"] for g in ms]), _off([g["src"] for g in ms])
        poses, l, cost, it, status = G.pose_graph_optimize_dev(cat("X0", (12,)), cat("src", ()), cat("tgt", ()), _t(cat("T", (12,)), dev),
                                                               _t(cat("Lam", (6, 6)), dev), cat("unc", ()), None, no, eo)
        return {"poses": (poses, no), "l": (l, eo)}, {"cost": cost, "iterations": it, "status": status}

    def check(g, got):
        assert got["status"] == 0 and (got["l"] == 1).all()
        if len(g["X0"]) == 1:                             # nothing to optimise: the pose of node 0 as given, no iteration
            assert got["iterations"] == 0 and got["cost"] == 0 and np.array_equal(got["poses"][0, :3].reshape(12), g["X0"][0])
        else:                                             # test_posegraph_gpu.py: without noise both loops end within 1e-9 of the truth
            assert max(P.graph_error(got["poses"][:, :3, :].reshape(-1, 12), g["X_true"])) <= 1e-9

    run_case(dev, "pose_graph_optimize", layout, run, members, check=check)


# ---- meshes ------------------------------------------------------------------------------------------------------------------------------

EF = np.zeros((0, 3), np.int32)


def _mesh_batch(dev, ms):
    (v, vo), (f, to) = _cat(ms, lambda m: m[0]), _cat(ms, lambda m: m[1], EF)
    return _t(v, dev), _t(f, dev), vo, to


def _meshes(layout, degenerate=False):
    return W.mesh_members(degenerate) if layout == "wide" else W.sparse_mesh_members(degenerate)


@pytest.mark.parametrize("layout", LAYOUT_NAMES)
def test_sample_mesh(dev, layout):
    """A shape without faces is refused, so the one-face zero-area triangle (status 1, NaN points) stands in the empty slots."""
    from test_metrics_gpu import _check_on_faces
    n = 5

    def run(dev, ms):
        v, f, vo, to = _mesh_batch(dev, ms)
        pts, status, face = M.sample_mesh_dev(v, f, vo, to, n, seed=9, return_face=True)
        return {}, {"points": pts.reshape(len(ms), n, 3), "face": face.reshape(len(ms), n), "status": status}

    def check(m, got):
        if len(m[1]) == 1:                                # the zero-area triangle
            assert got["status"] == 1 and np.isnan(got["points"]).all()
        else:
            assert got["status"] == 0
            _check_on_faces(got["points"], got["face"], *m)

    run_case(dev, "sample_mesh", layout, run, _meshes(layout, True), check=check)


def _queries(v, seed, n=24):
    rs = np.random.RandomState(seed)
    near = v[rs.randint(0, len(v), n // 2)] + rs.randn(n // 2, 3).astype(np.float32) * 0.05
    return np.concatenate([near, rs.uniform(-1, 1, (n - n // 2, 3)).astype(np.float32)]).astype(np.float32)


@pytest.mark.parametrize("layout", LAYOUT_NAMES)
def test_signed_distance(dev, layout):
    from test_meshsdf_gpu import _check_against_oracle
    members = [(v, f, _queries(v, 900 + i)) for i, (v, f) in enumerate(_meshes(layout))]

    def run(dev, ms):
        v, f, vo, to = _mesh_batch(dev, ms)
        q, qo = _cat(ms, lambda m: m[2])
        S, I, C, Wn, status = MS.signed_distance_dev(_t(q, dev), v, f, qo, vo, to, return_winding=True)
        return {"S": (S, qo), "I": (I, qo), "C": (C, qo), "W": (Wn, qo)}, {"status": status}

    def literal(got):
        assert got["status"] == MS.STATUS_NO_FACES

    def check(m, got):
        v, f, q = m
        assert got["status"] == 0
        o = _check_against_oracle(q, v, f, got["S"], got["I"], got["C"], got["W"])
        far = np.abs(o["S"]) > 1e-4
        assert (np.sign(got["S"][far]) == np.sign(o["S"][far])).all()

    run_case(dev, "signed_distance", layout, run, members, literal, check)


@pytest.mark.parametrize("layout", LAYOUT_NAMES)
def test_mesh_occupancy(dev, layout):
    """A shape without faces is refused, so the tetrahedron stands in the empty slots."""
    import meshsdf_ref as MR
    from shapeformer_amd.data import make_grid
    Gd = 8
    X = make_grid([-1, -1, -1.], [1., 1, 1], [Gd] * 3)

    def run(dev, ms):
        v, f, vo, to = _mesh_batch(dev, ms)
        occ, status = MS.mesh_occupancy_dev(v, f, vo, to, grid_dim=Gd, return_status=True)
        return {}, {"occ": occ, "status": status}

    def check(m, got):
        v, f = m
        wn = np.abs(MR.brute(X.astype(np.float32), v.astype(np.float64), f)["W"])
        sure = np.abs(wn - 0.5) > 1e-4                    # test_meshsdf_gpu.py's bound on the winding number
        assert got["status"] == 0 and np.array_equal(got["occ"].reshape(-1)[sure].astype(bool), (wn > 0.5)[sure]) and sure.all()
        assert 0 < got["occ"].sum() < Gd ** 3

    run_case(dev, "mesh_occupancy", layout, run, _meshes(layout), check=check)


@pytest.mark.parametrize("layout", LAYOUT_NAMES)
def test_mesh_components(dev, layout):
    import components_ref as CR
    from shapeformer_amd.components import mesh_components_dev
    EPS = 2.0 ** -52

    def run(dev, ms):
        v, f, vo, to = _mesh_batch(dev, ms)
        vl, fl, coff, stats, status = mesh_components_dev(v, f, vo, to)
        items = {"vlabel": (vl, vo), "flabel": (fl, to)}
        items.update({k: (t, coff) for k, t in stats.items()})
        return items, {"status": status, "components": np.diff(coff)}

    def literal(got):
        assert got["components"] == 0

    def check(m, got):                                    # test_components_gpu.py's _check_labels for one shape
        rvl, rfl, rst, rs = CR.components(*m)
        assert got["status"] == rs and np.array_equal(got["vlabel"], rvl) and np.array_equal(got["flabel"], rfl)
        assert got["components"] == len(rst["area"]) == 1
        assert np.array_equal(got["n_vert"], rst["n_vert"]) and np.array_equal(got["n_face"], rst["n_face"])
        for key in ("area", "volume"):
            assert (np.abs(got[key] - rst[key]) <= (rst["n_face"] + 8) * EPS * rst["abs_" + key]).all()

    run_case(dev, "mesh_components", layout, run, _meshes(layout), literal, check)


@pytest.mark.parametrize("layout", LAYOUT_NAMES)
def test_cluster_simplify(dev, layout):
    import simplify_ref as SRf
    from shapeformer_amd.simplify import cluster_simplify_dev
    grid = 4

    def run(dev, ms):
        v, f, vo, to = _mesh_batch(dev, ms)
        ov, of, ovo, oto, status = cluster_simplify_dev(v, f, vo, to, grid)
        return {"verts": (ov, ovo), "faces": (of, oto)}, {"status": status}

    def check(m, got):
        rv, rf, rs = SRf.cluster(m[0], m[1], grid)
        assert got["status"] == rs == 0 and np.array_equal(got["faces"], rf) and len(got["verts"]) == len(rv)
        assert np.abs(got["verts"].astype(np.float64) - rv).max() <= 2.0 ** -22     # test_simplify_gpu.py: 2^-22 x the box's largest coordinate

    run_case(dev, "cluster_simplify", layout, run, _meshes(layout), check=check)


@pytest.mark.parametrize("layout", LAYOUT_NAMES)
def test_marching_cubes(dev, layout):
    """A dense (261, 8, 8, 8) batch whose grids follow the layout; the empty sets are all-zero grids, the ragged side is the output."""
    from oracle import mc_oracle as MO
    from shapeformer_amd import mcubes
    from test_mcubes_cpu import _sphere, _torus
    fields = [_sphere(8, 0.6), _sphere(8, 0.35, (0.2, 0, 0)), _torus(8, 0.5, 0.3), _sphere(8, 0.8), _sphere(8, 0.5, (-0.3, 0.2, 0.1)),
              np.maximum(_sphere(8, 0.3, (-0.5, 0, 0)), _sphere(8, 0.3, (0.5, 0, 0)))]
    members = [f.astype(np.float32) for f in fields][:len(W.sizes_of(W.TOOLS["marching_cubes"], layout))]
    zero = np.zeros((8, 8, 8), np.float32)

    def run(dev, ms):
        v, f, voff, toff = mcubes.marching_cubes_dev(_t(_rows(ms, lambda m: m, zero), dev), 0.5)
        return {"verts": (v, voff), "faces": (f, toff)}, {"n_verts": np.diff(voff), "n_faces": np.diff(toff)}

    def literal(got):
        assert got["n_verts"] == 0 and got["n_faces"] == 0

    def check(m, got):
        vo, fo = MO.marching_cubes(m, 0.5)
        assert len(fo) > 0 and np.array_equal(got["faces"], fo) and np.abs(got["verts"] - vo).max() < 1e-6      # test_mcubes_gpu.py's

    run_case(dev, "marching_cubes", layout, run, members, literal, check)


# ---- lattices: poisson and morph -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", LAYOUT_NAMES)
def test_poisson_splat(dev, layout):
    import poisson_ref as PR
    from shapeformer_amd import poisson
    R = 9
    members = W.orient_members(W.sizes_of(W.TOOLS["poisson_splat"], layout))

    def run(dev, ms):
        p, po = _cat(ms, lambda m: m[0])
        n, _ = _cat(ms, lambda m: m[1])
        Vx, Vy, Vz, Wd, outside = poisson.poisson_splat_dev(_t(p, dev), _t(n, dev), po, grid_dim=R)
        return {}, {"Vx": Vx, "Vy": Vy, "Vz": Vz, "W": Wd, "outside": outside}

    def literal(got):
        assert got["outside"] == 0 and not any(got[k].any() for k in ("Vx", "Vy", "Vz", "W"))

    def check(m, got):                                    # test_poisson_gpu.py: one f32 rounding of an f64 sum + the order of that sum
        ref = PR.splat(m[0], m[1], R)
        assert got["outside"] == ref[4] == 0
        for key, want in zip(("Vx", "Vy", "Vz", "W"), ref[:4]):
            assert np.all(np.abs(got[key].astype(np.float64) - want) <= 2.0 ** -23 * np.abs(want) + 1e-12 * len(m[0]))

    run_case(dev, "poisson_splat", layout, run, members, literal, check)


@pytest.mark.parametrize("layout", LAYOUT_NAMES)
def test_poisson_sample(dev, layout):
    import poisson_ref as PR
    from shapeformer_amd import poisson
    R = 9
    members = [(x, np.random.RandomState(950 + i).randn(R, R, R).astype(np.float32))
               for i, x in enumerate(_points(layout, "poisson_sample"))]
    zero = np.zeros((R, R, R), np.float32)

    def run(dev, ms):
        p, po = _cat(ms, lambda m: m[0])
        return {"value": (poisson.poisson_sample_dev(_t(_rows(ms, lambda m: m[1], zero), dev), _t(p, dev), po), po)}, {}

    def check(m, got):
        """"f64 weights, rounded once": the trilinear sum of 8 products in f64, then one rounding to f32 - poisson_splat's bound"""
        want = PR.sample(m[1].astype(np.float64), m[0])
        assert np.all(np.abs(got["value"].astype(np.float64) - want) <= 2.0 ** -23 * np.abs(want) + 1e-12)

    run_case(dev, "poisson_sample", layout, run, members, check=check)


@pytest.mark.parametrize("layout", LAYOUT_NAMES)
def test_point2voxel(dev, layout):
    import morph_ref as MRf
    from shapeformer_amd import morph
    Gd = 8

    def run(dev, ms):
        p, po = _cat(ms)
        return {}, {"vox": morph.point2voxel_dev(_t(p, dev), po, grid_dim=Gd)}

    def literal(got):
        assert not got["vox"].any()

    def check(m, got):
        assert np.array_equal(got["vox"], MRf.point2voxel(m, Gd)) and got["vox"].any()

    run_case(dev, "point2voxel", layout, run, _points(layout, "point2voxel"), literal, check)


@pytest.mark.parametrize("layout", LAYOUT_NAMES)
def test_voxel_lookup(dev, layout):
    import morph_ref as MRf
    from shapeformer_amd import morph
    Gd = 8
    members = [(x, (np.random.RandomState(970 + i).rand(Gd, Gd, Gd) < 0.5).astype(np.uint8))
               for i, x in enumerate(_points(layout, "voxel_lookup"))]
    zero = np.zeros((Gd, Gd, Gd), np.uint8)

    def run(dev, ms):
        p, po = _cat(ms, lambda m: m[0])
        return {"value": (morph.voxel_lookup_dev(_t(_rows(ms, lambda m: m[1], zero), dev), _t(p, dev), po), po)}, {}

    def check(m, got):
        i = MRf.point2index(m[0], Gd).numpy()
        assert np.array_equal(got["value"], m[1][i[:, 0], i[:, 1], i[:, 2]])

    run_case(dev, "voxel_lookup", layout, run, members, check=check)


def test_every_tool_of_the_table_has_its_test():
    """a new ragged tool adds a row to wide_batch.TOOLS and a test here: the names the tests above pass to run_case, spelled out"""
    names = {"nn_dist", "nn_dist_index", "knn_mean_dist", "statistical_outlier_mask", "radius_outlier_mask", "estimate_normals",
             "estimate_normals_viewpoint", "orient_normals_outward", "orient_normals_viewpoint", "farthest_point_sample",
             "voxel_downsample_centroid", "voxel_downsample_first", "segment_plane", "refit_plane", "euclidean_clusters",
             "transform_points", "evaluate_registration", "icp_point", "icp_plane", "fpfh", "match_features_s1_q2", "match_features_s3_q4",
             "hypothesis_poses", "score_poses", "ransac_correspondences", "information_matrix", "pose_graph_optimize",
             "hidden_point_mask_f32", "hidden_point_mask_f64", "resample_visible", "poisson_splat", "poisson_sample", "point2voxel",
             "voxel_lookup", "sample_mesh", "signed_distance", "mesh_occupancy", "mesh_components", "cluster_simplify", "marching_cubes"}
    names |= {f"knn_k{k}{e}" for k in (8, 33) for e in ("", "_exclude_self")}
    assert names == set(W.TOOLS)
