"""The three 3-D nearest-neighbour searches run one split search (csrc/sfmi_search.h): metrics.nn_dist, column 0 of
scan.knn_dev(k=1) and the correspondences of registration.evaluate_registration_dev at the identity pose give one set of bits, with
the target whole and with the target cut into chunks and merged.  Each search is held to its numpy / cKDTree statement in its own
file (test_metrics_gpu.py, test_scan_gpu.py, test_icp_gpu.py); here they are held to each other, `array_equal`, no tolerance.

Two ragged pairs.  Sources of 2049 and 1 points: two query blocks of 2048 (nn_dist, ICP; three of 1024 for knn's k <= 8 instance) and a
one-point set.  Targets of 257 and 700 points (one point past a 256-point tile; 2.7 tiles), where every plan reports one chunk, and of
1400 and 700 points, where every plan reports two (chunks of 700 and 350 points: the tile edge falls inside a chunk).  In each target
set one point is repeated in the set's last slot, which lies in the last chunk when the set is cut, and a source point sits exactly
on it: both copies are at d2 = 0 and the lower index has to win through the scan and through the merge."""
import numpy as np
import pytest
import torch

from shapeformer_amd import _lib, metrics, registration, scan

pytestmark = pytest.mark.gpu

SRC_SIZES = (2049, 1)


def _off(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


@pytest.mark.parametrize("tgt_sizes, split", [((257, 700), False), ((1400, 700), True)])
def test_one_set_of_bits_from_the_three_searches(dev, tgt_sizes, split):
    lib = _lib.lib()
    so, to = _off(SRC_SIZES), _off(tgt_sizes)
    N, M = int(so[-1]), int(to[-1])
    plain = 256                                                               # the block offsets alone: (B + 1) int64 on 256 bytes
    assert (lib.sfmi_icp_splits(2, N, M) > 1) == split
    assert (lib.sfmi_nn_dist_workspace_bytes(2, N, M) > plain) == split       # partial buffers only when the plan cuts the target
    assert (lib.sfmi_knn_workspace_bytes(2, N, M, 1) > plain) == split
    rs = np.random.RandomState(M)
    src = rs.uniform(-0.8, 0.8, (N, 3)).astype(np.float32)
    tgt = rs.uniform(-0.8, 0.8, (M, 3)).astype(np.float32)
    tie = ((5, 0), (3, N - 1))                                                # (target index in its set, source row sitting on it)
    for b, (j, i) in enumerate(tie):
        tgt[to[b + 1] - 1] = tgt[to[b] + j]
        src[i] = tgt[to[b] + j]
    s, t = torch.from_numpy(src).to(dev), torch.from_numpy(tgt).to(dev)
    d_nn, i_nn = metrics.nn_dist(s, t, so, to, return_index=True)
    d_knn, i_knn = scan.knn_dev(s, t, 1, so, to)
    _, _, i_icp, d_icp = registration.evaluate_registration_dev(s, t, so, to, 0.1)
    d_nn, i_nn, d_knn, i_knn, d_icp, i_icp = (x.cpu().numpy() for x in (d_nn, i_nn, d_knn, i_knn, d_icp, i_icp))
    assert d_nn.dtype == d_knn.dtype == d_icp.dtype == np.float32 and i_nn.dtype == i_knn.dtype == i_icp.dtype == np.int32
    assert np.array_equal(d_nn, d_knn[:, 0]) and np.array_equal(i_nn, i_knn[:, 0])
    assert np.array_equal(d_nn, d_icp) and np.array_equal(i_nn, i_icp)
    assert np.array_equal(d_nn, metrics.nn_dist(s, t, so, to).cpu().numpy())  # the merge without the index output
    for b, (j, i) in enumerate(tie):
        assert i_nn[i] == j and d_nn[i] == 0.0                                # not the copy in the last slot
    assert (i_nn[:2049] < tgt_sizes[0]).all() and (i_nn >= 0).all() and np.isfinite(d_nn).all()


PAIR_SIZES = (2049, 1024, 1, 0, 8)


def test_information_matrix_and_icp_step_give_one_set_of_bits(dev):
    """information_matrix_dev and icp_step_dev add their f64 sums with one piece of code (csrc/sfmi_ragged.h: sfmi_chunk_partial,
    sfmi_chunk_total): a lane's 4 points ascending, the wave butterfly, the 4 waves in order, the chunk partials in
    ascending order.  Five pairs: 3 chunks of 1024 source points, exactly one chunk, a single point, an empty pair (a chunk grid row
    with nothing to do) and a pair with a NaN.  Each target is a copy of its source and the poses are the identity, so the moved point
    is the f32 source exactly and every inlier has a = q: the point metric's J^T J of icp_step_dev (with a) and the information
    matrix (with q) are sums of the same terms, and the 21 upper entries must agree bit for bit.  Every fourth source point of the
    two large pairs is moved 10 units away and is no inlier, so lanes with nothing to add sit between lanes that add."""
    so = _off(PAIR_SIZES)
    N = int(so[-1])
    src = np.random.RandomState(28).uniform(-0.8, 0.8, (N, 3)).astype(np.float32)
    assert (src != 0).all()
    tgt = src.copy()
    for b in (0, 1):
        src[so[b]:so[b + 1]:4, 0] += 10.0
    tgt[so[4] + 3, 1] = np.nan
    s, t = torch.from_numpy(src).to(dev), torch.from_numpy(tgt).to(dev)
    _, _, sums, _, _, status = registration.icp_step_dev(s, t, so, so, 0.1)
    info, count, _, _, flag = registration.information_matrix_dev(s, t, so, so, 0.1, details=True)
    sums, status, info, count, flag = (x.cpu().numpy() for x in (sums, status, info, count, flag))
    assert sums.dtype == info.dtype == np.float64 and sums.shape == (5, 29) and info.shape == (5, 6, 6)
    iu = np.triu_indices(6)
    for b in range(4):
        assert np.array_equal(info[b][iu], sums[b, :21]), b
        assert count[b] == sums[b, 28], b
    assert count[:4].tolist() == [2049 - 513, 1024 - 256, 1, 0] and flag[:4].tolist() == [0, 0, 0, 0]
    assert status[4] == 4 and flag[4] == 1
    assert not info[4].any() and count[4] == 0
