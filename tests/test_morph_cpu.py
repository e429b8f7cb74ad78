"""CPU tests of the watertight-voxelization contract: properties of the scipy restatement in tests/morph_ref.py, the
host-side argument checks of shapeformer_amd/morph.py (they raise before the library is loaded), the exported symbols, and
make_dataset's new flags (the winding route's stores do not change)."""
import os

import numpy as np
import pytest
import torch

import morph_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(24, 3), (33, 6), (20, 1), (16, 2)]


# ---- the restatement ---------------------------------------------------------------------------------------------------------

def test_ball_is_the_integer_ball():
    assert R.ball(0).shape == (1, 1, 1) and R.ball(0).all()
    assert R.ball(1).sum() == 7 and R.ball(2).sum() == 33 and R.ball(6).sum() == 925
    b = R.ball(3)
    assert b[3, 3, 0] and b[1, 1, 2] and not b[1, 1, 1] and not b[0, 3, 2]          # 9 + 0 + 0, 4 + 4 + 1 <= 9 < 4 + 4 + 4, 9 + 0 + 1


@pytest.mark.parametrize("G,r", CASES)
def test_closing_fills_a_shell_with_a_hole_narrower_than_2r(G, r):
    vox, inside = R.shell_grid(G, r)
    out, st = R.watertight_fill(vox, r)
    assert st == 0
    # the dilation closes the hole (2(r-1) cells) in the plane of its face, x = hi, so the flood does not get in; the erosion then
    # takes back what lies within r of the outside: over the hole the dilated cover is thinner than r, so the voxels less than r
    # behind the hole may go, and every voxel at least r behind that face stays, the far side of the interior wall included
    hi = (3 * G) // 4
    deep = inside.copy()
    deep[hi - r + 1:] = False
    assert deep.sum() > 0 and out[deep].all()
    away = inside.copy()                                        # beside the hole the cover is r thick: filled up to the face
    c = (G // 4 + hi) // 2
    away[:, c - 2 * r:c + 2 * r + 1, c - 2 * r:c + 2 * r + 1] = False
    assert out[away].all()
    assert out[0, 0, 0] == 0 and out[G - 1, 0, G - 1] == 0


@pytest.mark.parametrize("G,r", [(24, 3), (33, 6), (16, 2)])
def test_selem_zero_leaks_through_the_same_hole(G, r):
    vox, inside = R.shell_grid(G, r)
    out, st = R.watertight_fill(vox, 0)
    assert st == 0
    assert np.array_equal(out[inside], vox[inside])             # the flood reached every empty voxel inside: only the set ones stay
    assert np.array_equal(out, vox)                             # nothing is enclosed at all
    closed, _ = R.watertight_fill(R.closed_shell(G), 0)
    assert closed[G // 2, G // 2, G // 2] == 1                  # without the hole the inside is not reached


def test_pipeline_is_idempotent_on_a_solid_box():
    G, r = 24, 3
    box = np.zeros((G, G, G), np.uint8)
    box[6:18, 5:19, 7:16] = 1
    once, st = R.watertight_fill(box, r)
    twice, _ = R.watertight_fill(once, r)
    assert st == 0 and np.array_equal(once, twice) and once[box == 1].all()


def test_flood_is_26_connected_and_reports_a_set_seed():
    v = R.diagonal_chambers()
    region, st = R.flood(v)
    assert st == 0 and region[5, 5, 5] == 1 and region.sum() == 128
    six = R.flood(v, structure=np.abs(np.indices((3, 3, 3)) - 1).sum(0) <= 1)[0]
    assert six[5, 5, 5] == 0 and six.sum() == 64
    full = np.ones((5, 5, 5), np.uint8)
    region, st = R.flood(full)
    assert st == 3 and region.all()


def test_serpentine_is_one_long_corridor():
    v, corridor = R.serpentine(32)
    region, st = R.flood(v)
    assert st == 0 and np.array_equal(region.astype(bool), corridor) and corridor.sum() > 32 ** 3 // 4


def test_point2voxel_half_cell_boundaries_round_to_even():
    G = 32
    x = torch.tensor([-1 + 2 * m / G for m in range(1, G)], dtype=torch.float32)            # between cells m-1 and m: m - 0.5 exactly
    idx = R.point2index(torch.stack([x, x, x], 1), G)[:, 0]
    assert idx.tolist() == [m if m % 2 == 0 else m - 1 for m in range(1, G)]                # half to even
    c = torch.tensor([-1 + 2 * (m + 0.5) / G for m in range(G)], dtype=torch.float32)       # the cell centres: m exactly
    assert R.point2index(torch.stack([c, c, c], 1), G)[:, 2].tolist() == list(range(G))
    assert np.array_equal(R.index2point(G)[:: G * G + G + 1, 0], c.numpy())
    assert R.point2voxel(np.array([[np.nan, 0, 0], [0, 0, 0], [5, -5, 0.999]], np.float32), G).sum() == 2


def test_where_a_fused_multiply_subtract_would_differ():
    assert all(len(R.fma_sensitive(G)) == 0 for G in (32, 33, 40))
    x = R.fma_sensitive(97)
    assert len(x) == 1 and R.point2index(np.stack([x, x, x], 1), 97)[0].tolist() == [0, 0, 0] and R.fused_index(x, 97).tolist() == [1]


def test_soup_cube_is_a_soup():
    v, f = R.soup_cube()
    assert len(v) == 3 * len(f) and len(f) == 2 * (7 * 64 - 1)
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    top = np.isclose(v[f].reshape(-1, 3, 3)[:, :, 2], 0.5).all(1)                           # the +z side: normals up and down
    assert (n[top, 2] > 0).any() and (n[top, 2] < 0).any() and np.abs(v).max() == 0.5


# ---- the host argument checks: every one raises SfmiError before the library is loaded

@pytest.fixture()
def no_library(monkeypatch):
    from shapeformer_amd import _lib
    def refuse():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", refuse)


def test_point_argument_checks(no_library):
    from shapeformer_amd import morph as M
    from shapeformer_amd._lib import SfmiError
    p = torch.zeros(10, 3)
    for off, word in (([0, 5, 9], "end at 10"), ([1, 10], "start at 0"), ([0, 7, 5, 10], "nondecreasing"), ([0.0, 10.0], "integer")):
        with pytest.raises(SfmiError, match=word):
            M.point2voxel_dev(p, off)
    with pytest.raises(SfmiError, match=r"\(N,3\)"):
        M.point2voxel_dev(torch.zeros(10, 2))
    with pytest.raises(SfmiError, match="offsets go with"):
        M.point2voxel_dev(torch.zeros(2, 5, 3), [0, 5, 10])
    for g in (0, -1, 2.5, True):
        with pytest.raises(SfmiError, match="grid_dim"):
            M.point2voxel_dev(p, grid_dim=g)
    with pytest.raises(SfmiError, match="2\\^31"):
        M.point2voxel_dev(p, grid_dim=1291)                     # 1291^3 > 2^31
    with pytest.raises(SfmiError, match="2\\^31"):
        M.point2voxel_dev(torch.zeros(64, 5, 3), grid_dim=323)  # 64 * 323^3 >= 2^31 > 63 * 323^3
    with pytest.raises(SfmiError, match="HIP device"):          # all host checks pass: the device check is the last one
        M.point2voxel_dev(p, [0, 4, 10])


@pytest.mark.parametrize("name", ["ball_dilate_dev", "ball_erode_dev"])
def test_radius_argument_checks(no_library, name):
    from shapeformer_amd import morph as M
    from shapeformer_amd._lib import SfmiError
    fn = getattr(M, name)
    vox = torch.zeros(2, 8, 8, 8, dtype=torch.uint8)
    for r in (17, -1, 1.5, True, None):
        with pytest.raises(SfmiError, match="r = "):
            fn(vox, r)
    with pytest.raises(SfmiError, match=r"\(B,G,G,G\)"):
        fn(torch.zeros(2, 8, 8, 7), 1)
    with pytest.raises(SfmiError, match=r"\(B,G,G,G\)"):
        fn(torch.zeros(8, 8), 1)
    with pytest.raises(SfmiError, match="HIP device"):
        fn(vox, 16)
    with pytest.raises(SfmiError, match="HIP device"):
        fn(vox[0], 0)


def test_grid_argument_checks(no_library):
    from shapeformer_amd import morph as M
    from shapeformer_amd._lib import SfmiError
    vox = torch.zeros(8, 8, 8, dtype=torch.uint8)
    big = torch.zeros(1, dtype=torch.uint8).expand(64, 323, 323, 323)          # a view: B * G^3 >= 2^31 without the memory
    for fn in (M.flood_dev, M.watertight_fill_dev, lambda v: M.ball_dilate_dev(v, 1)):
        with pytest.raises(SfmiError, match="2\\^31"):
            fn(big)
        with pytest.raises(SfmiError, match="HIP device"):
            fn(vox)
        with pytest.raises(SfmiError, match="torch tensor"):
            fn(np.zeros((8, 8, 8), np.uint8))
    for s in (17, -1, 2.0):
        with pytest.raises(SfmiError, match="selem_size"):
            M.watertight_fill_dev(vox, s)
    with pytest.raises(SfmiError, match="point sets"):
        M.voxel_lookup_dev(vox, torch.zeros(2, 5, 3))


def test_mesh_argument_checks(no_library):
    from shapeformer_amd import morph as M
    from shapeformer_amd._lib import SfmiError
    v, f = torch.zeros(8, 3), torch.zeros(4, 3, dtype=torch.int32)
    with pytest.raises(SfmiError, match="integer"):
        M.morph_voxelization_dev(v, f.float())
    with pytest.raises(SfmiError, match="end at 8"):
        M.morph_voxelization_dev(v, f, [0, 4, 7], [0, 2, 4])
    with pytest.raises(SfmiError, match="different batch sizes"):
        M.morph_voxelization_dev(v, f, [0, 4, 8], [0, 4])
    with pytest.raises(SfmiError, match="no faces"):
        M.morph_voxelization_dev(v, f, [0, 4, 8], [0, 0, 4])
    with pytest.raises(SfmiError, match="selem_size"):
        M.morph_voxelization_dev(v, f, selem_size=17)
    with pytest.raises(SfmiError, match="grid_dim"):
        M.morph_voxelization_dev(v, f, grid_dim=0)
    with pytest.raises(SfmiError, match="sampleN"):
        M.morph_voxelization_dev(v, f, sampleN=0)
    with pytest.raises(SfmiError, match="2\\^31"):
        M.morph_voxelization_dev(v, f, grid_dim=1291)
    with pytest.raises(SfmiError, match="HIP device"):
        M.morph_voxelization_dev(v, f, [0, 4, 8], [0, 2, 4], sampleN=100, grid_dim=16, selem_size=1)


# ---- the library

def test_library_exports_the_morph_symbols():
    import ctypes
    from shapeformer_amd import _lib as L
    from shapeformer_amd import build as B
    B.build(verbose=False)
    lib = ctypes.CDLL(L.LIB_PATH)
    names = ["sfmi_morph_max_radius", "sfmi_morph_words", "sfmi_morph_workspace_bytes", "sfmi_voxelize_points_f32", "sfmi_voxelize_lookup_f32",
             "sfmi_morph_dilate_u32", "sfmi_morph_flood_u32", "sfmi_morph_pack_u8", "sfmi_morph_unpack_u8"]
    assert not [n for n in names if not hasattr(lib, n)]
    assert set(names) <= set(L.PROTOTYPES)
    hdr = open(os.path.join(ROOT, "include", "sfmi.h")).read()
    assert all(n + "(" in hdr for n in names)


def test_host_entries_refuse_bad_sizes_without_a_device():
    """the size functions are pure host code; every launcher returns SFMI_EINVAL before it touches the device"""
    from shapeformer_amd import _lib as L
    from shapeformer_amd import morph as M
    lib = L.lib()
    assert lib.sfmi_morph_max_radius() == M.MAX_RADIUS == 16
    assert lib.sfmi_morph_words(2, 33) == 2 * 33 * 33 * 2 and lib.sfmi_morph_words(1, 32) == 32 * 32
    assert lib.sfmi_morph_words(1, 1291) == 0 and lib.sfmi_morph_words(0, 8) == 0
    # 256^3 at r = 6: 7 planes of 2 MiB against 64 MiB of parents; 32^3 at r = 16: 17 planes of 4 KiB against 128 KiB
    assert lib.sfmi_morph_workspace_bytes(1, 256, 6) == 4 * 256 ** 3
    assert lib.sfmi_morph_workspace_bytes(1, 33, 16) == max(17 * 33 * 33 * 2 * 4, 4 * 33 ** 3)
    assert lib.sfmi_morph_workspace_bytes(1, 8, 17) == 0 and lib.sfmi_morph_workspace_bytes(1, 8, -1) == 0
    assert lib.sfmi_morph_workspace_bytes(64, 323, 0) == 0
    buf = np.zeros(64, np.uint32)
    p = buf.ctypes.data
    assert lib.sfmi_morph_dilate_u32(p, 1, 4, 17, 0, 0, p, p, None) == L.SFMI_EINVAL
    assert lib.sfmi_morph_dilate_u32(p, 1, 4, -1, 0, 0, p, p, None) == L.SFMI_EINVAL
    assert lib.sfmi_morph_dilate_u32(None, 1, 4, 1, 0, 0, p, p, None) == L.SFMI_EINVAL
    assert lib.sfmi_morph_dilate_u32(p, 64, 323, 1, 0, 0, p, p, None) == L.SFMI_EINVAL
    assert lib.sfmi_morph_flood_u32(p, 1, 4, p, p, p, None) == L.SFMI_EINVAL          # region must not be in
    assert lib.sfmi_morph_flood_u32(p, 0, 4, None, p, p, None) == L.SFMI_EINVAL
    assert lib.sfmi_voxelize_points_f32(p, None, 1, 4, 4, p, None) == L.SFMI_EINVAL
    assert lib.sfmi_voxelize_points_f32(p, p, 1, -1, 4, p, None) == L.SFMI_EINVAL
    assert lib.sfmi_voxelize_lookup_f32(p, p, 1, 4, 0, p, p, None) == L.SFMI_EINVAL
    assert lib.sfmi_morph_pack_u8(None, 1, 4, p, None) == L.SFMI_EINVAL
    assert lib.sfmi_morph_unpack_u8(p, 1, 4, None, None) == L.SFMI_EINVAL


# ---- make_dataset

def test_make_dataset_flags():
    from shapeformer_amd import make_dataset as MD
    base = ["a.obj", "--out", "o", "--dataset", "d"]
    a = MD.parse_args(base)
    assert (a.occupancy, a.morph_grid, a.selem, a.morph_samples, a.scale) == ("winding", 128, 6, 1_000_000, 1.0)
    a = MD.parse_args(base + ["--occupancy", "morph", "--morph-grid", "64", "--selem", "3", "--morph-samples", "5000", "--scale", "0.9"])
    assert (a.occupancy, a.morph_grid, a.selem, a.morph_samples, a.scale) == ("morph", 64, 3, 5000, 0.9)
    for bad in (["--occupancy", "sdf"], ["--selem", "17"], ["--selem", "-1"], ["--morph-grid", "0"], ["--morph-samples", "0"],
                ["--scale", "0"], ["--scale", "nan"]):
        with pytest.raises(SystemExit):
            MD.parse_args(base + bad)
    with pytest.raises(ValueError, match="occupancy"):
        MD.make_dataset([], "o", "d", occupancy="sdf")
    with pytest.raises(ValueError, match="scale"):
        MD.make_dataset([], "o", "d", scale=-1.0)


def _fake_device_route(monkeypatch, seen):
    """stand-ins for the two device calls of the winding route: deterministic functions of the vertices they are handed"""
    from shapeformer_amd import meshsdf, metrics

    def occupancy(v, f, voff, toff, grid_dim=64, return_status=False):
        seen.append(v.clone())
        B = len(voff) - 1
        o = torch.stack([((torch.arange(grid_dim ** 3) * 7 + int(v[voff[b]:voff[b + 1]].abs().sum() * 1000)) % 5 == 0)
                         .to(torch.uint8).reshape(grid_dim, grid_dim, grid_dim) for b in range(B)])
        return o, torch.zeros(B, dtype=torch.int32)

    def sample(v, f, voff, toff, n, seed=0):
        B = len(voff) - 1
        x = torch.stack([v[voff[b]:voff[b + 1]][torch.arange(n) % (voff[b + 1] - voff[b])] + seed for b in range(B)])
        return x.reshape(B * n, 3), torch.zeros(B, dtype=torch.int32)

    monkeypatch.setattr(meshsdf, "mesh_occupancy_dev", occupancy)
    monkeypatch.setattr(metrics, "sample_mesh_dev", sample)


def test_winding_store_is_unchanged_by_the_new_flags(monkeypatch, tmp_path):
    """--occupancy winding with the new flags at their defaults writes the bytes that no flags write, hands the device the normalised
    vertices themselves, and never touches the morph module; --scale reaches both device calls"""
    import sys
    from shapeformer_amd import make_dataset as MD, meshio, meshsdf
    v, f = R.soup_cube(2)
    paths = []
    for i, s in enumerate((1.0, 3.0, 0.25)):
        paths.append(str(tmp_path / f"m{i}.ply"))
        meshio.write_ply(paths[-1], v * s + i, f)
    seen = []
    _fake_device_route(monkeypatch, seen)
    monkeypatch.setitem(sys.modules, "shapeformer_amd.morph", None)           # importing it would raise
    kw = dict(split="train", grid=8, boundary_n=16, cates={"odd": "*m1*"}, seed=3, batch=2, device="cpu")
    d0 = MD.make_dataset(paths, str(tmp_path / "a"), "d", **kw)
    d1 = MD.make_dataset(paths, str(tmp_path / "b"), "d", occupancy="winding", morph_grid=128, selem=6, morph_samples=1_000_000, scale=1.0, **kw)
    files = sorted(os.listdir(d0))
    assert files == sorted(os.listdir(d1)) == ["Xbd.npy", "Ytg.npy", "cate_odd.npy"]
    for n in files:
        assert open(os.path.join(d0, n), "rb").read() == open(os.path.join(d1, n), "rb").read(), n
    want = torch.from_numpy(np.concatenate([meshsdf.normalize_point_set(meshio.read_mesh(p)[0]) for p in paths[:2]]).astype(np.float32))
    assert torch.equal(seen[0], want) and torch.equal(seen[2], want)
    seen.clear()
    MD.make_dataset(paths[:2], str(tmp_path / "c"), "d", scale=0.5, **kw)
    assert torch.equal(seen[0], torch.from_numpy((np.concatenate([meshsdf.normalize_point_set(meshio.read_mesh(p)[0]) for p in paths[:2]])
                                                  * 0.5).astype(np.float32)))
    x = np.load(os.path.join(str(tmp_path / "c"), "d", "train", "Xbd.npy"))
    assert np.abs(x - 3).max() <= 0.5                            # the samples are the scaled vertices (+ seed 3)
