"""GPU tests of farthest point sampling, voxel-grid downsampling and their wiring into the cleaning front end (shapeformer_amd/scan.py,
csrc/downsample.hip) against tests/downsample_ref.py.  The shapes are the smallest that reach each path: the edges of
the three resident instances (1024, 4096, FPS_RESIDENT_MAX points), one set beyond them on the streaming form, sets smaller than n."""
import numpy as np
import pytest
import torch

import downsample_ref as R
import knn_ref as K
from shapeformer_amd import metrics as M
from shapeformer_amd import scan
from shapeformer_amd._lib import SfmiError

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 1000, 1024, 1025, 4096, 4097, scan.FPS_RESIDENT_MAX, scan.FPS_RESIDENT_MAX + 1]
SMALL = [s for s in SIZES if s <= 4097]                      # also sampled to their own size and five beyond
N_PICKS = 64


def _off(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(*ts):
    return [t.cpu().numpy() if isinstance(t, torch.Tensor) else t for t in ts]


def _sets(p, off):
    return [p[off[b]:off[b + 1]] for b in range(len(off) - 1)]


@pytest.fixture(scope="module")
def dyadic():
    """the ragged dyadic sets and, per set, the reference run at the largest n any test asks for (a smaller n is its prefix)"""
    rs = np.random.RandomState(0)
    off = _off(SIZES)
    p = R.dyadic(rs, off[-1])
    ref = [R.fps(x, max(N_PICKS, len(x) + 5) if len(x) <= 4097 else N_PICKS) for x in _sets(p, off)]
    return p, off, ref


@pytest.fixture(scope="module")
def floats():
    rs = np.random.RandomState(1)
    off = _off(SIZES)
    return (rs.rand(off[-1], 3) - 0.5).astype(np.float32), off


# ---- 1. FPS, bit for bit

def test_fps_bitwise_on_dyadic_sets(dev, dyadic):
    p, off, ref = dyadic
    idx, d2, count, status = _np(*scan.farthest_point_sample_dev(_t(p, dev), off, N_PICKS))
    assert idx.shape == (len(SIZES), N_PICKS) and idx.dtype == np.int32 and d2.dtype == np.float32 and count.dtype == np.int32
    assert np.array_equal(status, np.zeros(len(SIZES), np.int32))
    for b, size in enumerate(SIZES):
        assert count[b] == min(N_PICKS, size), size
        assert np.array_equal(idx[b], ref[b][0][:N_PICKS]), size
        assert np.array_equal(d2[b], ref[b][1][:N_PICKS]), size


@pytest.mark.parametrize("extra", [0, 5])
def test_fps_bitwise_full_order_and_tail(dev, dyadic, extra):
    p, off, ref = dyadic
    for b, size in enumerate(SIZES):
        if size > 4097:
            continue
        n = size + extra
        idx, d2, count, status = _np(*scan.farthest_point_sample_dev(_t(p[off[b]:off[b + 1]], dev), None, n))
        assert idx.shape == (1, n) and count[0] == size and status[0] == 0
        assert np.array_equal(idx[0], ref[b][0][:n]) and np.array_equal(d2[0], ref[b][1][:n]), size
        assert np.array_equal(np.sort(idx[0, :size]), np.arange(size))                       # a full ordering is a permutation
        assert np.all(idx[0, size:] == -1) and np.all(d2[0, size:] == 0)


def test_fps_copies_of_one_point(dev):
    p = np.repeat(np.float32([[0.25, -0.5, 0.125]]), 10, 0)
    idx, d2, count, status = _np(*scan.farthest_point_sample_dev(_t(p, dev), None, 12))
    assert count[0] == 10 and status[0] == 0 and np.array_equal(idx[0], np.r_[np.arange(10), -1, -1])
    assert np.isposinf(d2[0, 0]) and np.all(d2[0, 1:] == 0)


# ---- 2. FPS on random floats

def test_fps_greedy_on_floats(dev, floats):
    p, off = floats
    pt = _t(p, dev)
    idx, d2, count, status = _np(*scan.farthest_point_sample_dev(pt, off, N_PICKS))
    assert np.all(status == 0)
    for b, x in enumerate(_sets(p, off)):
        c = count[b]
        R.check_greedy(x, idx[b], d2[b], c)
        assert np.isposinf(d2[b, 0]) and np.all(np.diff(d2[b, 1:c]) <= 0) and len(set(idx[b, :c])) == c
    # two runs are identical; n = 16 is a prefix; a set alone gives its row of the batch
    again = _np(*scan.farthest_point_sample_dev(pt, off, N_PICKS))
    assert all(np.array_equal(a, b) for a, b in zip(again, (idx, d2, count, status)))
    i16, d16, c16, _ = _np(*scan.farthest_point_sample_dev(pt, off, 16))
    assert np.array_equal(i16, idx[:, :16]) and np.array_equal(d16, d2[:, :16]) and np.array_equal(c16, np.minimum(count, 16))
    for b in (0, 4, 7, 9, 10, 11):
        ia, da, ca, _ = _np(*scan.farthest_point_sample_dev(_t(p[off[b]:off[b + 1]], dev), None, N_PICKS))
        assert np.array_equal(ia[0], idx[b]) and np.array_equal(da[0], d2[b]) and ca[0] == count[b], SIZES[b]
    # the (B,M,3) batch form
    xb = p[:4 * 1000].reshape(4, 1000, 3)
    ib, db, cb, _ = _np(*scan.farthest_point_sample_dev(_t(xb, dev), None, 32))
    for b in range(4):
        i1, d1, _, _ = _np(*scan.farthest_point_sample_dev(_t(xb[b], dev), None, 32))
        assert np.array_equal(ib[b], i1[0]) and np.array_equal(db[b], d1[0]) and cb[b] == 32


def test_fps_d2_is_nn_dist_bit_for_bit(dev):
    """d2[t] is the distance from pick t to the nearest earlier pick in the arithmetic of the existing kernel: one ragged nn_dist call
    with n - 1 sets, set t - 1 = (pick t) against (picks 0 .. t - 1)"""
    rs = np.random.RandomState(2)
    p = (rs.rand(300, 3) - 0.5).astype(np.float32)
    idx, d2, _, _ = _np(*scan.farthest_point_sample_dev(_t(p, dev), None, N_PICKS))
    picks = p[idx[0]]
    q = np.concatenate([picks[:t] for t in range(1, N_PICKS)])
    got = M.nn_dist(_t(picks[1:], dev), _t(q, dev), np.arange(N_PICKS, dtype=np.int64), _off(range(1, N_PICKS))).cpu().numpy()
    assert np.array_equal(got, d2[0, 1:])


# ---- 3. arguments

def test_fps_start_per_set(dev, dyadic, floats):
    p, off, _ = dyadic
    start = np.array([0, 1, 62, 5, 64, 999, 1023, 1024, 4095, 17, scan.FPS_RESIDENT_MAX - 1, scan.FPS_RESIDENT_MAX])
    idx, d2, count, status = _np(*scan.farthest_point_sample_dev(_t(p, dev), off, 16, start=start))
    for b, x in enumerate(_sets(p, off)):
        want = R.fps(x, 16, start=start[b])
        assert np.array_equal(idx[b], want[0]) and np.array_equal(d2[b], want[1]) and count[b] == want[2] and status[b] == 0
    q, _ = floats
    idx, d2, count, _ = _np(*scan.farthest_point_sample_dev(_t(q, dev), off, 16, start=torch.from_numpy(start)))
    for b, x in enumerate(_sets(q, off)):
        R.check_greedy(x, idx[b], d2[b], count[b], start=start[b])
    one = _np(*scan.farthest_point_sample_dev(_t(q[off[5]:off[6]], dev), None, 16, start=999))       # a plain int for one set
    assert np.array_equal(one[0][0], idx[5]) and np.array_equal(one[1][0], d2[5])


def test_fps_valid_mask_is_the_compaction_route(dev, dyadic):
    p, off, _ = dyadic
    rs = np.random.RandomState(3)
    valid = (rs.rand(len(p)) < 0.5).astype(np.uint8)
    valid[off[5]:off[6]] = 0                                                                 # a set whose mask is all zero
    valid[off[4]] = 0                                                                        # the default start moves with the mask
    idx, d2, count, status = _np(*scan.farthest_point_sample_dev(_t(p, dev), off, N_PICKS, valid=_t(valid, dev)))
    sel = [np.flatnonzero(v) for v in _sets(valid, off)]
    coff = _off([len(s) for s in sel])
    packed = np.concatenate([x[s] for x, s in zip(_sets(p, off), sel)])
    jdx, e2, cnt, cst = _np(*scan.farthest_point_sample_dev(_t(packed, dev), coff, N_PICKS))
    assert np.array_equal(count, cnt) and np.array_equal(d2, e2) and np.array_equal(status, cst)
    for b in range(len(SIZES)):
        c = count[b]
        assert c == min(N_PICKS, len(sel[b])) and status[b] == (1 if len(sel[b]) == 0 else 0)
        assert np.array_equal(idx[b, :c], sel[b][jdx[b, :c]]) and np.all(idx[b, c:] == -1) and np.all(d2[b, c:] == 0)
        want = R.fps(p[off[b]:off[b + 1]], N_PICKS, valid=valid[off[b]:off[b + 1]])
        assert np.array_equal(idx[b], want[0]) and np.array_equal(d2[b], want[1]) and (c, status[b]) == want[2:]
    assert status[5] == 1 and count[5] == 0 and np.all(idx[5] == -1)


def test_fps_non_finite_point(dev, dyadic):
    p, off, ref = dyadic
    bad = p.copy()
    bad[off[6] + 700, 1] = np.nan                                                            # resident
    bad[off[11] + 16384, 2] = np.inf                                                         # streaming: the set's last point
    idx, d2, count, status = _np(*scan.farthest_point_sample_dev(_t(bad, dev), off, N_PICKS))
    for b in range(len(SIZES)):
        if b in (6, 11):
            assert status[b] == 2 and count[b] == 0 and np.all(idx[b] == -1) and np.all(d2[b] == 0)
        else:                                                                                # the other sets of the batch: untouched
            assert status[b] == 0 and np.array_equal(idx[b], ref[b][0][:N_PICKS]) and np.array_equal(d2[b], ref[b][1][:N_PICKS])
    valid = np.ones(len(p), np.uint8)
    valid[off[6] + 700] = valid[off[11] + 16384] = 0                                         # not candidates: not looked at
    idx, _, count, status = _np(*scan.farthest_point_sample_dev(_t(bad, dev), off, N_PICKS, valid=_t(valid, dev)))
    assert np.all(status == 0) and count[6] == N_PICKS and count[11] == N_PICKS
    assert 700 not in idx[6] and 16384 not in idx[11]
    assert scan.farthest_point_sample_dev(_t(p, dev), off, 0)[0].shape == (len(SIZES), 0)   # n = 0: nothing to write


# ---- 4. voxel grid

VOX_SIZES = [0, 1, 5, 1000, 40000]


@pytest.fixture(scope="module")
def clouds():
    rs = np.random.RandomState(4)
    off = _off(VOX_SIZES)
    return (rs.rand(off[-1], 3) - 0.5).astype(np.float32), off


def _check_voxels(dev, p, off, voxel):
    pt = _t(p, dev)
    out, out_off, first, count = _np(*scan.voxel_downsample_dev(pt, off, voxel))
    pf, pf_off, ffirst, fcount = _np(*scan.voxel_downsample_dev(pt, off, voxel, "first"))
    assert out_off.dtype == np.int64 and out.dtype == np.float32 and first.dtype == np.int32 and count.dtype == np.int32
    assert np.array_equal(out_off, pf_off) and np.array_equal(first, ffirst) and np.array_equal(count, fcount)
    assert out_off[0] == 0 and out_off[-1] == len(out) == len(first) == len(count)
    for b, x in enumerate(_sets(p, off)):
        want, wfirst, wcount = R.voxel_down(x, voxel)
        s = slice(out_off[b], out_off[b + 1])
        assert out_off[b + 1] - out_off[b] == len(want), (b, voxel)
        assert np.array_equal(first[s], wfirst) and np.array_equal(count[s], wcount)         # hence the voxel order
        assert count[s].sum() == len(x)
        assert np.array_equal(pf[s], x[wfirst])                                              # pick="first": bitwise
        assert R.ulps(out[s], want).max(initial=0) <= 1, (b, voxel)
    again = _np(*scan.voxel_downsample_dev(pt, off, voxel))
    assert all(np.array_equal(a, b) for a, b in zip(again, (out, out_off, first, count)))
    return out, out_off, first, count


@pytest.mark.parametrize("voxel", [0.5, 0.05, 0.013])
def test_voxel_against_reference(dev, clouds, voxel):
    p, off = clouds
    out, out_off, first, count = _check_voxels(dev, p, off, voxel)
    for b in (1, 3, 4):                                                                      # a set alone: the same bits as in the batch
        a = _np(*scan.voxel_downsample_dev(_t(p[off[b]:off[b + 1]], dev), None, voxel))
        s = slice(out_off[b], out_off[b + 1])
        assert np.array_equal(a[0], out[s]) and np.array_equal(a[2], first[s]) and np.array_equal(a[3], count[s])
        assert np.array_equal(a[1], [0, out_off[b + 1] - out_off[b]])


def test_voxel_larger_than_the_extent(dev, clouds):
    p, off = clouds
    out, out_off, first, count = _check_voxels(dev, p, off, 1.5)
    assert np.array_equal(out_off, [0, 0, 1, 2, 3, 4]) and np.array_equal(count, VOX_SIZES[1:]) and np.all(first == 0)
    xb = p[off[3]:off[4]].reshape(4, 250, 3)                                                 # the (B,M,3) form
    ob, ob_off, _, cb = _np(*scan.voxel_downsample_dev(_t(xb, dev), None, 1.5))
    assert np.array_equal(ob_off, np.arange(5)) and np.all(cb == 250)
    assert R.ulps(ob, xb.astype(np.float64).mean(1).astype(np.float32)).max() <= 1


def test_voxel_points_on_cell_faces_and_negative_coordinates(dev):
    g = np.arange(-4, 5) * 0.125
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    rs = np.random.RandomState(5)
    neg = (-rs.rand(3000, 3) * np.array([4.0, 0.25, 1.0]) - 1.0).astype(np.float32)          # every coordinate negative
    p, off = np.concatenate([lattice, lattice[::-1], neg]), _off([729, 729, 3000])
    out, out_off, first, count = _check_voxels(dev, p, off, 0.125)
    assert np.array_equal(out_off[:3], [0, 729, 1458]) and np.all(count[:1458] == 1)
    order = np.lexsort((lattice[:, 0], lattice[:, 1], lattice[:, 2]))                        # ascending in (cz, cy, cx)
    assert np.array_equal(first[:729], order) and np.array_equal(out[:729], lattice[order])
    assert np.array_equal(out[729:1458], lattice[order])                                     # the same voxels whatever the input order


def test_voxel_grid_too_fine_or_not_finite(dev, clouds):
    p, off = clouds
    x = np.float32([[0, 0, 0], [0.1, 0.2, 0.3], [1.0, 0.5, 0.25]])
    assert len(scan.voxel_downsample_dev(_t(x, dev), None, 1.0 / 65535)[0]) == 3             # 65 536 cells along x: the last grid that fits
    with pytest.raises(SfmiError, match="65536 cells or more"):
        scan.voxel_downsample_dev(_t(x, dev), None, 1.0 / 65537)
    with pytest.raises(SfmiError, match="65536 cells or more"):
        scan.voxel_downsample_dev(_t(p, dev), off, 1e-6)
    bad = p.copy()
    bad[off[4] + 7, 0] = np.nan
    with pytest.raises(SfmiError, match="not finite"):
        scan.voxel_downsample_dev(_t(bad, dev), off, 0.05)
    bad[off[4] + 7, 0] = -np.inf
    with pytest.raises(SfmiError, match="not finite"):
        scan.voxel_downsample_dev(_t(bad, dev), off, 0.05)


# ---- 5. the front end

@pytest.mark.parametrize("seed", [0, 1, 2])
def test_front_end_on_a_two_density_scan(dev, seed):
    p = R.two_density(seed)
    pt = _t(p, dev)
    vox, voff, _, _ = scan.voxel_downsample_dev(pt, None, 0.05)
    keep, kept, _ = scan.statistical_outlier_mask_dev(vox, voff, 16, 2.0)
    c, keep = vox.cpu().numpy().astype(np.float64), keep.cpu().numpy().astype(bool)
    far = np.linalg.norm(c, axis=1) > 0.7
    assert far.sum() >= 15 and not keep[far].any()                                           # every planted outlier's voxel is removed
    sparse = ~far & (c[:, 0] <= -0.02)
    assert sparse.sum() > 100 and keep[sparse].mean() >= 0.95, keep[sparse].mean()
    raw_keep = scan.statistical_outlier_mask_dev(pt, None, 16, 2.0)[0].cpu().numpy().astype(bool)
    assert raw_keep[12000:12600].mean() <= 0.5, raw_keep[12000:12600].mean()                 # the raw cloud loses its sparse half
    # resample="fps": distinct kept voxels in farthest-point order
    out, count = scan.clean_cloud_dev(pt[None], 16, 2.0, out_N=1024, voxel=0.05, resample="fps")
    assert out.shape == (1, 1024, 3) and int(count[0]) == int(kept[0]) == keep.sum() and keep.sum() >= 1024
    rows = out[0].cpu().numpy()
    kept_rows = {r.tobytes() for r in vox.cpu().numpy()[keep]}
    assert len({r.tobytes() for r in rows}) == 1024 and all(r.tobytes() in kept_rows for r in rows)
    r64 = rows.astype(np.float64)
    radius = np.array([((r64[t] - r64[:t]) ** 2).sum(-1).min() for t in range(1, 1024)])     # squared, to each row's predecessors
    assert np.all(np.diff(radius) <= 2 * K.RTOL * radius[:-1] + K.ATOL)
    # fewer kept points than out_N: the order repeats cyclically
    n = int(count[0])
    more, count2 = scan.clean_cloud_dev(pt[None], 16, 2.0, out_N=n + 300, voxel=0.05, resample="fps")
    more = more[0].cpu().numpy()
    assert int(count2[0]) == n and np.array_equal(more[:1024], rows) and np.array_equal(more[n:], more[:300])
    assert len({r.tobytes() for r in more[:n]}) == n
    # the random route on the voxels, and the defaults: two runs are equal
    rnd, count3 = scan.clean_cloud_dev(pt[None], 16, 2.0, out_N=512, voxel=0.05)
    assert int(count3[0]) == n and all(r.tobytes() in kept_rows for r in rnd[0].cpu().numpy())
    a, ca = scan.clean_cloud_dev(pt[None])
    b, cb = scan.clean_cloud_dev(pt[None])
    assert a.shape == (1, len(p), 3) and torch.equal(a, b) and torch.equal(ca, cb)


def test_front_end_fps_falls_back_to_all_points(dev):
    """two or fewer kept points: all the cloud's points, as the random route does"""
    x = np.float32([[[0, 0, 0], [0.5, 0, 0]], [[0.25, 0, 0], [0.25, 0, 0]]])                 # k + 1 > 2 points: SOR keeps all; count = 2
    out, count = scan.clean_cloud_dev(_t(x, dev), k=1, out_N=5, resample="fps")
    assert np.array_equal(count.cpu().numpy(), [2, 2])
    assert np.array_equal(out.cpu().numpy(), x[:, [0, 1, 0, 1, 0]])
