"""Plane removal and Euclidean clustering on the device (csrc/segment.hip) against tests/segment_ref.py.

Plane scoring and the clusters are exact contracts: count / best / status and root are compared with `==`.  The refit is compared with
numpy's eigh to 1e-9 absolute per coefficient, a derived bound: a Jacobi f64 eigenvector is off by about eps / gap, the two fixed-order
sums differ by about n eps, so a few 1e-11 at n = 3000 and gap >= 0.9 (asserted), against the 6e-8 spacing of the f32 inputs.

The scene (segment_ref.scene): a jittered plane of 3000 points at y = -0.4, a sphere shell of 1000 points of radius 0.3, 100 uniform
outliers.  By the reference alone, seeds 0-2 at thr = 0.01, H = 256: best counts 3001-3002 with ties among hypotheses, one invalid draw
(seed 2), eigen-gaps 0.958-0.973, no point within 1e-9 of the threshold, no pair at the exact radius; after plane removal at radius
0.05 one cluster of 997-1000 points and ~97 of 1-7.  Outliers that happen to lie next to the sphere join its cluster; in seed 1 the one
that does is 0.0098 off the surface, so the wiring tests, which ask for every kept point within 0.02 of the sphere, use seed 1."""
import numpy as np
import pytest
import torch

import segment_ref as R
from shapeformer_amd import scan

pytestmark = pytest.mark.gpu

THR, HMAX = 0.01, 257


def _off(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(*ts):
    return [t.cpu().numpy() for t in ts]


@pytest.fixture(scope="module")
def scenes():
    """seeds 0-2: points, kinds, the 257 draws (a smaller H is their prefix) and the reference's count per draw, computed once"""
    out = []
    for seed in range(3):
        p, kind = R.scene(seed)
        tr = R.plane_hypotheses([len(p)], HMAX, seed)[0]
        count, _, status = R.plane_score_set(p, tr, THR)
        assert status == 0
        out.append(dict(p=p, kind=kind, tr=tr, count=count))
    return out


@pytest.fixture(scope="module")
def refits(scenes):
    """the reference's refit of each scene at H = 256, and the remainder after the plane is removed"""
    out = []
    for s in scenes:
        best = int(np.argmax(s["count"][:256]))
        plane, mask, n_in, dist, gap = R.plane_refit_set(s["p"], s["tr"][best], THR)
        out.append(dict(best=best, plane=plane, mask=mask, n_in=n_in, dist=dist, gap=gap, rest=s["p"][~mask]))
    return out


# ---- plane scoring: equal to the reference, no tolerance ---------------------------------------------------------------------------

@pytest.mark.parametrize("H", [1, 63, 64, 65, 257])
def test_score_scene(dev, scenes, H):
    p = np.concatenate([s["p"] for s in scenes])
    off = _off([len(s["p"]) for s in scenes])
    tr = np.stack([s["tr"][:H] for s in scenes])
    for seed, s in enumerate(scenes):                                         # the library's draws are the reference's
        assert np.array_equal(scan.plane_hypotheses([len(s["p"])], H, seed)[0], s["tr"][:H])
    runs = [_np(*scan.segment_plane_dev(_t(p, dev), off, THR, triples=tr)[3:]) for _ in range(2)]
    count, best, status = runs[0]
    for b, s in enumerate(scenes):
        ref = s["count"][:H]
        assert np.array_equal(count[b], ref)
        assert best[b] == (int(np.argmax(ref)) if (ref >= 0).any() else -1)
        assert status[b] == (0 if (ref >= 0).any() else 1)
    for a, b in zip(*runs):                                                   # two runs: the same bits
        assert np.array_equal(a, b)
    if H == 257:
        assert any((s["count"] == s["count"].max()).sum() > 1 for s in scenes)    # the tie rule is exercised
        assert sum(int((s["count"] < 0).sum()) for s in scenes) >= 1              # and an invalid draw


def test_score_ragged_batch_equals_per_set_calls(dev):
    """sets of 0 .. 4100 points: the kernel's chunk is 1024 points, so in the batch the 1000- and 4100-point sets are cut at other
    places than in their own calls"""
    rng = np.random.default_rng(5)
    sizes = [0, 1, 2, 3, 64, 65, 1000, 4100]
    off = _off(sizes)
    p = rng.uniform(-1, 1, (off[-1], 3))
    p[:, 2] = 0.3 * p[:, 0] + rng.normal(0, 0.004, len(p))
    p = p.astype(np.float32)
    H = 65
    tr = scan.plane_hypotheses(sizes, H, 3)
    plane, inl, n_in, count, best, status = _np(*scan.segment_plane_dev(_t(p, dev), off, THR, hypotheses=H, seed=3))
    rc, rb, rs = R.plane_score(p, off, tr, THR)
    assert np.array_equal(count, rc) and np.array_equal(best, rb) and np.array_equal(status, rs)
    assert rs.tolist() == [1, 1, 1, 0, 0, 0, 0, 0] and (rc[:3] == -1).all()
    for b, n in enumerate(sizes):
        one = _np(*scan.segment_plane_dev(_t(p[off[b]:off[b + 1]], dev), None, THR, hypotheses=H, seed=3))
        assert np.array_equal(one[3][0], count[b]) and one[4][0] == best[b] and one[5][0] == status[b]
        assert np.array_equal(one[0][0], plane[b], equal_nan=True) and one[2][0] == n_in[b]
        assert np.array_equal(one[1], inl[off[b]:off[b + 1]])
    assert np.isnan(plane[:3]).all() and (n_in[:3] == 0).all()                # no winner: NaN plane, empty mask


def test_score_all_points_on_the_plane(dev):
    g = np.stack(np.meshgrid(np.arange(40.), np.arange(33.), indexing="ij"), -1).reshape(-1, 2) / 64.0
    p = np.concatenate([g, np.full((len(g), 1), 0.25)], 1).astype(np.float32)  # dyadic: every product is exact
    _, inl, n_in, count, best, status = _np(*scan.segment_plane_dev(_t(p, dev), None, 0.0, hypotheses=64))
    rc, rb, rs = R.plane_score(p, [0, len(p)], scan.plane_hypotheses([len(p)], 64, 0), 0.0)
    assert np.array_equal(count, rc) and best[0] == rb[0] and status[0] == 0
    assert set(np.unique(count).tolist()) <= {-1, len(p)} and count[0, best[0]] == len(p)
    assert n_in[0] == len(p) and inl.all()


def test_score_hand_given_triples(dev, scenes):
    p = scenes[0]["p"].copy()
    n = len(p)
    p[10], p[11], p[12] = [0, 0, 0], [0.25, 0.5, -0.25], [0.5, 1.0, -0.5]      # three collinear points
    tr = np.array([[[5, 5, 9], [5, 9, n], [10, 11, 12], [-1, 5, 9], [5, 9, 5], [1, 2, 3], [2 ** 31 - 1, 2, 3], [4, 5, 6]]], np.int32)
    count, best, status = _np(*scan.segment_plane_dev(_t(p, dev), None, THR, triples=tr)[3:])
    rc, rb, rs = R.plane_score(p, [0, n], tr, THR)
    assert np.array_equal(count, rc) and np.array_equal(best, rb) and np.array_equal(status, rs)
    assert (count[0, [0, 1, 2, 3, 4, 6]] == -1).all() and (count[0, [5, 7]] >= 3).all()
    bad = _np(*scan.segment_plane_dev(_t(p, dev), None, THR, triples=_t(tr[:, :5], dev))[3:])      # device triples; none valid
    assert (bad[0] == -1).all() and bad[1][0] == -1 and bad[2][0] == 1


def test_score_non_finite_point(dev, scenes):
    a, b, c = scenes[0]["p"][:1500], scenes[1]["p"][:1300].copy(), scenes[2]["p"][:1100]
    b[1234, 1] = np.nan
    off = _off([len(a), len(b), len(c)])
    p = np.concatenate([a, b, c])
    tr = scan.plane_hypotheses(np.diff(off), 64, 0)
    plane, inl, n_in, count, best, status = _np(*scan.segment_plane_dev(_t(p, dev), off, THR, hypotheses=64))
    rc, rb, rs = R.plane_score(p, off, tr, THR)
    assert np.array_equal(count, rc) and np.array_equal(best, rb) and np.array_equal(status, rs)
    assert status.tolist() == [0, 2, 0] and (count[1] == -1).all() and best[1] == -1
    assert np.isnan(plane[1]).all() and n_in[1] == 0 and not inl[off[1]:off[2]].any()
    b[1234, 1] = np.inf
    count2, _, status2 = _np(*scan.segment_plane_dev(_t(np.concatenate([a, b, c]), dev), off, THR, hypotheses=64)[3:])
    assert np.array_equal(count2, count) and status2.tolist() == [0, 2, 0]


# ---- refit -------------------------------------------------------------------------------------------------------------------------

def test_refit_against_eigh(dev, scenes, refits):
    worst = 0.0
    for seed, (s, r) in enumerate(zip(scenes, refits)):
        assert r["gap"] >= 0.9 and r["n_in"] >= 3000                          # what the 1e-9 bound was derived for
        near = np.abs(np.abs(r["dist"]) - THR) <= 1e-9
        assert near.sum() == 0                                                # by the reference alone: the exclusion below excludes nothing
        runs = [_np(*scan.segment_plane_dev(_t(s["p"], dev), None, THR, triples=s["tr"][None, :256])) for _ in range(2)]
        plane, inl, n_in, _, best, _ = runs[0]
        assert best[0] == r["best"]
        err = np.abs(plane[0] - r["plane"]).max()
        worst = max(worst, err)
        print(f"refit seed {seed}: max |plane - eigh| = {err:.3e}, gap {r['gap']:.4f}, n_in {n_in[0]}")
        assert err <= 1e-9
        assert abs(np.linalg.norm(plane[0, :3]) - 1) < 1e-15
        differ = (inl != 0) != r["mask"]
        assert not (differ & ~near).any() and near.sum() <= 1e-3 * len(near)
        assert n_in[0] == inl.sum() == r["n_in"]
        for a, b in zip(*runs):
            assert np.array_equal(a, b, equal_nan=True)
    print(f"refit: measured maximum {worst:.3e} against the bound 1e-9")


def test_refit_up_flips_the_sign_only(dev, scenes):
    p = _t(scenes[0]["p"], dev)
    tr = scenes[0]["tr"][None, :256]
    base = _np(*scan.segment_plane_dev(p, None, THR, triples=tr))
    assert base[0][0, 1] > 0.99                                               # largest component positive: +y
    same = _np(*scan.segment_plane_dev(p, None, THR, triples=tr, up=(0, 1, 0)))
    flip = _np(*scan.segment_plane_dev(p, None, THR, triples=tr, up=np.array([[0.1, -1.0, 0]])))
    assert np.array_equal(same[0], base[0]) and np.array_equal(flip[0], -base[0])
    for k in range(1, 6):
        assert np.array_equal(same[k], base[k]) and np.array_equal(flip[k], base[k])


def test_refit_off_returns_the_winning_triple(dev, scenes, refits):
    s, r = scenes[2], refits[2]
    plane, inl, n_in, count, best, _ = _np(*scan.segment_plane_dev(_t(s["p"], dev), None, THR, triples=s["tr"][None, :256], refit=False))
    n, d, nn, ok = R.triple_plane(s["p"], s["tr"][best[0]])
    assert ok and np.array_equal(inl != 0, R.seed_inliers(s["p"], n, d, nn, THR)) and n_in[0] == inl.sum() == count[0, best[0]]
    ref = np.concatenate([n, [-d]]) / np.sqrt(nn)
    ref = -ref if ref[int(np.argmax(np.abs(ref[:3])))] < 0 else ref
    assert np.abs(plane[0] - ref).max() < 1e-14


def test_refit_from_a_seed_plane(dev, scenes):
    """any (n, dd) seeds the refit: a rough floor plane with a normal of length 2, a plane nowhere near the points, a zero normal and a
    NaN seed, in one ragged batch"""
    p = np.concatenate([scenes[0]["p"], scenes[1]["p"][:1000], scenes[2]["p"][:500], scenes[2]["p"][:300]])
    off = _off([len(scenes[0]["p"]), 1000, 500, 300])
    seed = np.array([[0.002, 2.0, -0.004, 0.8], [0, 1, 0, -5.0], [0, 0, 0, 0.4], [0, np.nan, 0, 0.4]])
    plane, inl, n_in = _np(*scan.refit_plane_dev(_t(p, dev), off, seed, THR))
    n = seed[0, :3]
    ref, mask, cnt, dist, gap = R.plane_refit_seed(scenes[0]["p"], n, -seed[0, 3], (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2], THR)
    assert gap >= 0.9 and cnt >= 3000 and not (np.abs(np.abs(dist) - THR) <= 1e-9).any()
    err = np.abs(plane[0] - ref).max()
    print(f"refit from a seed plane: max |plane - eigh| = {err:.3e}")
    assert err <= 1e-9 and np.array_equal(inl[:off[1]] != 0, mask) and n_in[0] == cnt
    assert np.isnan(plane[1:]).all() and not inl[off[1]:].any() and (n_in[1:] == 0).all()
    again = _np(*scan.refit_plane_dev(_t(scenes[0]["p"], dev), None, torch.from_numpy(plane[0]).to(dev), THR, up=(0, -1, 0)))
    assert np.abs(again[0][0] + plane[0]).max() <= 1e-9 and np.array_equal(again[1], inl[:off[1]])   # a fixed point, flipped by up


# ---- clusters: root equal to the reference -----------------------------------------------------------------------------------------

def _clusters(dev, p, off, radius, min_points=1):
    label, sizes, c_off, root = scan.euclidean_clusters_dev(_t(p, dev), off, radius, min_points, return_root=True)
    return label.cpu().numpy(), sizes.cpu().numpy(), c_off, root.cpu().numpy()


def _check_clusters(dev, p, radius, min_points=1):
    label, sizes, c_off, root = _clusters(dev, p, None, radius, min_points)
    ref = R.cluster_roots(p, radius)
    assert root.dtype == np.int32 and np.array_equal(root, ref)
    rl, rs = R.cluster_labels(ref, min_points)
    assert np.array_equal(label, rl) and np.array_equal(sizes, rs) and c_off.tolist() == [0, len(rs)]
    return label, sizes, root


@pytest.mark.parametrize("radius", [0.05, 0.08])
def test_clusters_scene_remainder(dev, refits, radius):
    for seed, r in enumerate(refits):
        rest = r["rest"]
        d2 = R.d2_matrix_rows(rest, 0, len(rest))
        assert not (d2 == np.float32(radius ** 2)).any()                      # no pair at the exact radius
        label, sizes, root = _check_clusters(dev, rest, radius)
        assert 990 <= sizes[0] <= 1010 and len(sizes) > 80 and sizes[1] < 10
        assert (np.diff(sizes) <= 0).all()                                    # size descending ...
        firsts = np.array([np.flatnonzero(label == k)[0] for k in range(len(sizes))])
        assert np.array_equal(root[firsts], firsts)                           # ... a cluster's root is its lowest index ...
        for k in range(len(sizes) - 1):
            assert sizes[k] > sizes[k + 1] or firsts[k] < firsts[k + 1]       # ... and root ascending among equal sizes
        label3, sizes3, _ = _check_clusters(dev, rest, radius, min_points=3)  # small clusters become -1; the ranks of the rest stay
        assert (sizes3 >= 3).all() and np.array_equal(sizes3, sizes[sizes >= 3])
        assert np.array_equal(label3, np.where(sizes[label] >= 3, label, -1))
        if seed == 0:
            again = _clusters(dev, rest, None, radius)
            assert np.array_equal(again[0], label) and np.array_equal(again[3], root)


def test_clusters_pair_at_the_exact_radius(dev):
    p = np.array([[0, 0, 0], [0.5, 0, 0]], np.float32)
    assert _check_clusters(dev, p, 0.5)[2].tolist() == [0, 0]                 # d2 == r2: joined
    p[1, 0] = np.nextafter(np.float32(0.5), np.float32(1))
    assert _check_clusters(dev, p, 0.5)[2].tolist() == [0, 1]                 # one ulp further: not joined
    p[1] = [np.nan, 0, 0]
    assert _check_clusters(dev, p, 0.5)[2].tolist() == [0, 1]


def test_clusters_shuffled_chain(dev):
    """4100 points in a row, 0.9 x radius apart, in shuffled index order: one cluster through every tile boundary and the deepest
    union-find trees; with one link of 1.1 x radius, two"""
    n, radius = 4100, 0.01
    rng = np.random.default_rng(11)
    perm = rng.permutation(n)
    x = np.arange(n) * (0.9 * radius)
    p = np.zeros((n, 3), np.float32)
    p[perm, 0] = x
    _, sizes, root = _check_clusters(dev, p, radius)
    assert sizes.tolist() == [n] and (root == 0).all()
    x[2500:] += 0.2 * radius
    p[perm, 0] = x
    label, sizes, root = _check_clusters(dev, p, radius)
    assert sorted(sizes.tolist()) == [1600, 2500] and sizes[0] == 2500
    assert np.array_equal(label == 0, np.argsort(perm) < 2500)                # perm[k] holds chain position k


def test_clusters_ragged_batch_equals_per_set_calls(dev, refits):
    rng = np.random.default_rng(2)
    sets = [np.zeros((0, 3), np.float32), rng.uniform(-1, 1, (1, 3)).astype(np.float32), refits[0]["rest"][:700],
            rng.uniform(-0.3, 0.3, (1100, 3)).astype(np.float32), np.zeros((0, 3), np.float32), refits[1]["rest"]]
    off = _off([len(s) for s in sets])
    label, sizes, c_off, root = _clusters(dev, np.concatenate(sets), off, 0.05, 2)
    assert c_off.shape == (7,) and c_off[0] == 0 and c_off[-1] == len(sizes)
    for b, s in enumerate(sets):
        ref = R.cluster_roots(s, 0.05)
        rl, rs = R.cluster_labels(ref, 2) if len(s) else (np.zeros(0, np.int32), np.zeros(0, np.int32))
        assert np.array_equal(root[off[b]:off[b + 1]], ref) and np.array_equal(label[off[b]:off[b + 1]], rl)
        assert np.array_equal(sizes[c_off[b]:c_off[b + 1]], rs)
        one = _clusters(dev, s, None, 0.05, 2)
        assert np.array_equal(one[0], rl) and np.array_equal(one[1], rs) and np.array_equal(one[3], ref)
    keep, count = scan.largest_cluster_mask_dev(_t(np.concatenate(sets), dev), off, 0.05, 2)
    assert np.array_equal(keep.cpu().numpy(), (label == 0).astype(np.uint8))
    assert count.cpu().numpy().tolist() == [int(sizes[c_off[b]]) if c_off[b + 1] > c_off[b] else 0 for b in range(6)]


# ---- wiring ------------------------------------------------------------------------------------------------------------------------

def _tilt():
    """a known rotation: 25 degrees about (1, 2, 3)"""
    a = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.radians(25.0)
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


def test_isolate_object_on_the_tilted_scene(dev, scenes):
    Q = _tilt()
    p = (scenes[1]["p"].astype(np.float64) @ Q.T).astype(np.float32)
    x = _t(p, dev)
    kept, k_off, mask, planes, rot = scan.isolate_object_dev(x, None, THR, 0.05, hypotheses=256, seed=1)
    kept, mask, planes, rot = _np(kept, mask, planes, rot)
    assert k_off.tolist() == [0, len(kept)] and 990 <= len(kept) <= 1010 and mask.sum() == len(kept)
    assert np.abs(np.linalg.norm(kept.astype(np.float64), axis=1) - 0.3).max() < 0.02          # the sphere is centred on the origin
    assert np.abs(np.linalg.norm(p[mask != 0].astype(np.float64), axis=1) - 0.3).max() < 0.02
    up = np.array([0.0, 1.0, 0.0])
    normal = Q @ up                                                           # the floor's true normal, on the object's side
    assert np.arccos(np.clip(planes[0, 0, :3] @ normal, -1, 1)) < 1e-3
    assert np.arccos(np.clip((rot[0] @ normal) @ up, -1, 1)) < 1e-3
    assert np.abs(rot[0] @ rot[0].T - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(rot[0]) - 1) < 1e-14
    assert np.array_equal(kept, (p[mask != 0].astype(np.float64) @ rot[0].T).astype(np.float32))
    assert kept[:, 1].min() > -0.32                                           # upright: the floor was below the sphere
    for mode, scale in (("mean_max", None), ("bbox", 0.9)):
        normed = scan.isolate_object_dev(x, None, THR, 0.05, hypotheses=256, seed=1, normalize=mode, scale=scale)[0]
        want = scan.normalize_scan(_t(kept, dev), mode, **({} if scale is None else {"scale": scale}))
        assert torch.equal(normed, want)
    keep2, planes2, taken2 = scan.remove_planes_dev(x, None, THR, max_planes=2, min_ratio=0.2, hypotheses=256, seed=1)
    assert taken2.cpu().numpy().tolist() == [1] and np.isnan(planes2[0, 1].cpu().numpy()).all()   # the sphere holds no second plane
    assert np.array_equal(keep2.cpu().numpy(), scan.remove_planes_dev(x, None, THR, hypotheses=256, seed=1)[0].cpu().numpy())


def test_clean_cloud_defaults_keep_their_bits(dev, scenes):
    x = _t(np.stack([scenes[0]["p"][:4096], scenes[1]["p"][:4096]]), dev)
    for voxel in (None, 0.02):
        a, ca = scan.clean_cloud_dev(x, k=8, std_ratio=1.5, out_N=1024, seed=3, voxel=voxel)
        b, cb = scan.clean_cloud_dev(x, k=8, std_ratio=1.5, out_N=1024, seed=3, voxel=voxel, remove_planes=None, keep_cluster=None)
        assert torch.equal(a, b) and torch.equal(ca, cb)


def test_clean_cloud_with_planes_and_cluster(dev, scenes):
    x = _t(np.stack([scenes[1]["p"][:4096], scenes[1]["p"][4:]]), dev)
    out, count = scan.clean_cloud_dev(x, k=8, std_ratio=3.0, out_N=2048, seed=1, remove_planes={"threshold": THR, "hypotheses": 256},
                                      keep_cluster={"radius": 0.05})
    assert out.shape == (2, 2048, 3) and out.dtype == torch.float32
    r = np.linalg.norm(out.cpu().numpy().astype(np.float64), axis=2)
    assert np.abs(r - 0.3).max() < 0.02                                       # every row is a point of the sphere
    assert ((count.cpu().numpy() >= 900) & (count.cpu().numpy() <= 1010)).all()
    out_v, count_v = scan.clean_cloud_dev(x, k=8, std_ratio=3.0, out_N=512, seed=1, voxel=0.01, resample="fps",
                                          remove_planes={"threshold": THR, "hypotheses": 256}, keep_cluster={"radius": 0.05})
    assert out_v.shape == (2, 512, 3) and np.abs(np.linalg.norm(out_v.cpu().numpy().astype(np.float64), axis=2) - 0.3).max() < 0.02


def test_callback_takes_the_new_arguments(dev):
    from shapeformer_amd import callbacks as CB
    ctx = {"voxel": 0.02, "remove_planes": {"threshold": THR}, "keep_cluster": {"radius": 0.05}}
    assert CB.VisShapeFormer(end_tokens=(4096, 4096), clean_context=ctx).clean_context == ctx
    with pytest.raises(ValueError, match="clean_context"):
        CB.VisShapeFormer(end_tokens=(4096, 4096), clean_context=dict(ctx, out_N=5))
