"""CPU tests of the downsampling tools (shapeformer_amd/scan.py farthest_point_sample_dev / voxel_downsample_dev, csrc/downsample.hip;
DESIGN.md §5.15): the C-ABI surface, the two pure host entries through ctypes, every host-side refusal (raised before the library is
loaded), and the numpy references of tests/downsample_ref.py against brute-force definitions."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import downsample_ref as R
from shapeformer_amd import _lib as L
from shapeformer_amd import scan
from shapeformer_amd._lib import SfmiError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("sfmi_fps_resident_max", "sfmi_fps_workspace_bytes", "sfmi_fps_f32", "sfmi_voxel_keys_f32", "sfmi_voxel_reduce_f32")


@pytest.fixture()
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(L, "lib", refuse)


def test_symbols_are_exported_declared_and_bound():
    for name in ("farthest_point_sample_dev", "voxel_downsample_dev"):
        assert callable(getattr(scan, name))
    hdr = open(os.path.join(ROOT, "include", "sfmi.h")).read()
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in L.PROTOTYPES
    assert len(L.PROTOTYPES["sfmi_fps_f32"][1]) == 13 and len(L.PROTOTYPES["sfmi_voxel_reduce_f32"][1]) == 12
    par = inspect.signature(scan.clean_cloud_dev).parameters
    assert par["voxel"].default is None and par["resample"].default == "random"
    src = open(os.path.join(ROOT, "shapeformer_amd", "csrc", "downsample.hip")).read()
    assert '#include "sfmi_ragged.h"' in src
    for helper in ("sfmi_owner", "sfmi_shape_of", "wave_sum_f64", "cdiv", "align256", "blocks256"):       # used, not defined again
        assert not re.search(r"\b(int|double|size_t|unsigned|long long)\s+%s\s*\(" % helper, src), helper


def test_resident_max_and_workspace_bytes():
    from shapeformer_amd import build as B
    B.build(verbose=False)
    lib = ctypes.CDLL(L.LIB_PATH)
    rmax, ws = lib.sfmi_fps_resident_max, lib.sfmi_fps_workspace_bytes
    rmax.restype, rmax.argtypes = L.PROTOTYPES["sfmi_fps_resident_max"]
    ws.restype, ws.argtypes = L.PROTOTYPES["sfmi_fps_workspace_bytes"]
    assert rmax() >= 16384 and rmax() == scan.FPS_RESIDENT_MAX
    assert ws(0, 10, 4) == 0 and ws(-1, 10, 4) == 0 and ws(1, -1, 4) == 0 and ws(1, 10, -1) == 0
    assert 0 < ws(1, 0, 0) <= 4096 and 0 < ws(64, rmax(), 2048) <= 4096                  # nothing can stream: no distances in memory
    for B_, N in ((1, rmax() + 1), (3, 10 ** 5), (64, 10 ** 6)):
        assert (N + 4 * B_) * 4 <= ws(B_, N, 64) <= (N + 4 * B_) * 4 + 1024              # one f32 per point, each set's slice on 16 bytes
    assert ws(1, 10 ** 5, 1) == ws(1, 10 ** 5, 16384)


@pytest.mark.parametrize("n", [-1, 2.0, "8", None, True, 2 ** 31])
def test_fps_n_refused(no_library, n):
    with pytest.raises(SfmiError, match="n must be an integer"):
        scan.farthest_point_sample_dev(torch.zeros(10, 3), None, n)


def test_fps_refusals(no_library):
    p = torch.zeros(10, 3)
    for start in (10, -1, [0, 6], np.array([4, 0])):
        with pytest.raises(SfmiError, match="start out of range"):
            scan.farthest_point_sample_dev(p, [0, 4, 10], 4, start=start)
    with pytest.raises(SfmiError, match="start out of range"):                               # an empty set offers no start
        scan.farthest_point_sample_dev(p, [0, 0, 10], 4, start=0)
    for start in (1.0, [0.0, 1.0], True, [0, 1, 2], np.zeros((2, 1), np.int64)):
        with pytest.raises(SfmiError, match="start must be an integer"):
            scan.farthest_point_sample_dev(p, [0, 4, 10], 4, start=start)
    with pytest.raises(SfmiError, match="start together with valid"):
        scan.farthest_point_sample_dev(p, None, 4, start=0, valid=torch.ones(10, dtype=torch.uint8))
    for valid in (torch.ones(9, dtype=torch.uint8), torch.ones(10, 1, dtype=torch.uint8), torch.ones(1, 10, dtype=torch.uint8)):
        with pytest.raises(SfmiError, match="one entry per point"):
            scan.farthest_point_sample_dev(p, None, 4, valid=valid)
    with pytest.raises(SfmiError, match="one entry per point"):
        scan.farthest_point_sample_dev(torch.zeros(2, 5, 3), None, 4, valid=torch.ones(10, dtype=torch.uint8))
    for valid in (torch.ones(10, dtype=torch.bool), torch.ones(10), torch.ones(10, dtype=torch.int32), np.ones(10, np.uint8)):
        with pytest.raises(SfmiError, match="valid must be a uint8 torch tensor"):
            scan.farthest_point_sample_dev(p, None, 4, valid=valid)
    with pytest.raises(SfmiError, match="offsets go with"):
        scan.farthest_point_sample_dev(p[None], [0, 10], 4)
    with pytest.raises(SfmiError, match="end at 10"):
        scan.farthest_point_sample_dev(p, [0, 4, 9], 4)
    with pytest.raises(SfmiError, match=r"\(N,3\)"):
        scan.farthest_point_sample_dev(torch.zeros(10, 2), None, 4)
    # where the tensors live is reported last: valid arguments on the CPU
    for call in (lambda: scan.farthest_point_sample_dev(p, None, 4), lambda: scan.farthest_point_sample_dev(p, [0, 4, 10], 0, start=[3, 5]),
                 lambda: scan.farthest_point_sample_dev(p[None], None, 4, valid=torch.ones(1, 10, dtype=torch.uint8)),
                 lambda: scan.voxel_downsample_dev(p, None, 0.1), lambda: scan.voxel_downsample_dev(p[None], None, 1, "first"),
                 lambda: scan.clean_cloud_dev(p[None], voxel=0.05, resample="fps")):
        with pytest.raises(SfmiError, match="HIP device.*no CPU fallback"):
            call()


@pytest.mark.parametrize("voxel", [0, 0.0, -0.1, float("nan"), float("inf"), None, "0.1", True])
def test_voxel_refused(no_library, voxel):
    p = torch.zeros(10, 3)
    with pytest.raises(SfmiError, match="voxel must be a finite number > 0"):
        scan.voxel_downsample_dev(p, None, voxel)
    if voxel is not None:                                                                    # None is clean_cloud_dev's "no voxel pass"
        with pytest.raises(SfmiError, match="voxel must be a finite number > 0"):
            scan.clean_cloud_dev(p[None], voxel=voxel)


def test_voxel_and_front_end_refusals(no_library):
    p = torch.zeros(10, 3)
    for pick in ("mean", "", None, 0):
        with pytest.raises(SfmiError, match="pick must be one of"):
            scan.voxel_downsample_dev(p, None, 0.1, pick)
    with pytest.raises(SfmiError, match="fewer than 32768 sets"):
        scan.voxel_downsample_dev(torch.zeros(32768, 1, 3), None, 0.1)
    with pytest.raises(SfmiError, match="integer"):
        scan.voxel_downsample_dev(p, [0.0, 10.0], 0.1)
    for resample in ("FPS", "uniform", None, 1):
        with pytest.raises(SfmiError, match="resample must be one of"):
            scan.clean_cloud_dev(p[None], resample=resample)
        with pytest.raises(SfmiError, match="resample must be one of"):
            scan.clean_cloud_dev(p[None], voxel=0.1, resample=resample)
    with pytest.raises(SfmiError, match="k must be"):
        scan.clean_cloud_dev(p[None], k=0, voxel=0.1)
    from shapeformer_amd import callbacks as CB
    with pytest.raises(ValueError, match="clean_context"):
        CB.VisShapeFormer(end_tokens=(4096, 4096), clean_context={"voxel": 0.02, "resample": "fps", "out_N": 5})
    cb = CB.VisShapeFormer(end_tokens=(4096, 4096), clean_context={"voxel": 0.02, "resample": "fps"})
    assert cb.clean_context == {"voxel": 0.02, "resample": "fps"}
    with pytest.raises(SfmiError, match="HIP device.*no CPU fallback"):                      # the dict reaches clean_cloud_dev as it is
        scan.clean_cloud_dev(p[None], **cb.clean_context)


# ---- the references against brute-force definitions

@pytest.mark.parametrize("seed,m,n", [(0, 1, 4), (1, 2, 2), (2, 40, 40), (3, 200, 64), (4, 200, 205)])
def test_fps_reference_is_the_definition(seed, m, n):
    rs = np.random.RandomState(seed)
    p = R.dyadic(rs, m)
    idx, d2, count, status = R.fps(p, n)
    want = R.fps_brute(p, n)
    assert status == 0 and count == min(n, m) and np.array_equal(idx[:count], want) and np.all(idx[count:] == -1) and np.all(d2[count:] == 0)
    assert np.isposinf(d2[0]) and np.all(np.diff(d2[1:count]) <= 0) and len(set(idx[:count])) == count
    p64 = p.astype(np.float64)
    for t in range(1, count):                                             # d2[t]: the squared covering radius of the first t picks
        d = ((p64[:, None] - p64[idx[:t]][None]) ** 2).sum(-1).min(1)
        assert d2[t] == d.max() == d[idx[t]]
    R.check_greedy(p, idx, d2, count)
    q = (rs.rand(m, 3) - 0.5).astype(np.float32)                          # arbitrary floats: the f32 loop passes the f64 check
    R.check_greedy(q, *R.fps(q, n)[:3])
    assert np.array_equal(R.fps(p, min(n, 8))[0], idx[:min(n, 8)])        # a smaller n is a prefix


def test_fps_reference_arguments():
    rs = np.random.RandomState(7)
    p = R.dyadic(rs, 60)
    idx, d2, count, _ = R.fps(p, 10, start=17)
    assert idx[0] == 17 and np.isposinf(d2[0])
    R.check_greedy(p, idx, d2, count, start=17)
    valid = (rs.rand(60) < 0.5).astype(np.uint8)
    sel = np.flatnonzero(valid)
    idx, d2, count, status = R.fps(p, 100, valid=valid)
    jdx, e2, cnt, _ = R.fps(p[sel], 100)                                  # the compaction route
    assert status == 0 and count == cnt == len(sel) and np.array_equal(idx[:count], sel[jdx[:cnt]]) and np.array_equal(d2, e2)
    R.check_greedy(p, idx, d2, count, valid=valid)
    assert R.fps(p, 5, valid=np.zeros(60, np.uint8))[2:] == (0, 1)
    bad = p.copy()
    bad[3, 1] = np.nan
    idx, d2, count, status = R.fps(bad, 5)
    assert (count, status) == (0, 2) and np.all(idx == -1) and np.all(d2 == 0)
    assert R.fps(bad, 5, valid=(np.arange(60) != 3).astype(np.uint8))[3] == 0           # not among the candidates: not looked at
    idx, d2, count, _ = R.fps(np.repeat(p[:1], 10, 0), 12)                # ten copies of one point
    assert count == 10 and np.array_equal(idx[:10], np.arange(10)) and np.isposinf(d2[0]) and np.all(d2[1:] == 0)
    with pytest.raises(AssertionError):                                   # the check refuses a pick that is not an arg max
        wrong = R.fps(p, 10)
        wrong[0][5] = wrong[0][9]
        R.check_greedy(p, wrong[0], wrong[1], wrong[2])


@pytest.mark.parametrize("seed,m,voxel", [(0, 1, 0.1), (1, 300, 0.5), (2, 300, 0.05), (3, 500, 0.013), (4, 50, 7.0)])
def test_voxel_reference_is_the_definition(seed, m, voxel):
    rs = np.random.RandomState(seed)
    p = (rs.rand(m, 3) - 0.5).astype(np.float32)
    out, first, count = R.voxel_down(p, voxel)
    groups = R.voxel_brute(p, voxel)
    assert len(out) == len(groups) and count.sum() == m and out.dtype == np.float32
    assert [g[0] for g in groups] == first.tolist() and [len(g) for g in groups] == count.tolist()
    mean = np.array([p[g].astype(np.float64).mean(0) for g in groups])
    assert np.allclose(out, mean, rtol=1e-6, atol=1e-9)
    assert np.array_equal(R.voxel_down(p, voxel, "first")[0], p[first])
    if voxel > 2:
        assert len(out) == 1 and first[0] == 0


def test_voxel_reference_faces_and_empty():
    g = np.arange(-4, 5) * 0.125                                           # lattice points ON the cell faces: each goes to the upper cell
    p = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    out, first, count = R.voxel_down(p, 0.125)
    assert len(out) == 729 and np.all(count == 1) and np.array_equal(np.sort(first), np.arange(729))
    c = R.cells(p, 0.125)
    assert np.array_equal(c, np.round((p + 0.5) * 8).astype(np.int64))
    order = np.lexsort((c[:, 0], c[:, 1], c[:, 2]))                        # ascending in (cz, cy, cx)
    assert np.array_equal(first, order) and np.array_equal(out, p[order])
    out, first, count = R.voxel_down(np.zeros((0, 3), np.float32), 0.1)
    assert out.shape == (0, 3) and len(first) == 0 and len(count) == 0
    assert R.ulps(np.float32([1.0, -1.0, 0.0]), np.float32([np.nextafter(np.float32(1), np.float32(2)), -1.0, -0.0])).tolist() == [1, 0, 0]
