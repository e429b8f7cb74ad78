"""GPU tests of the watertight voxelization (csrc/morph.hip, shapeformer_amd/morph.py) against the scipy / torch-CPU
restatement of tests/morph_ref.py.  Every step is an integer problem: all comparisons are exact."""
import functools

import numpy as np
import pytest
import torch

import morph_ref as R

pytestmark = pytest.mark.gpu


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _eq(t, a):
    return np.array_equal(t.cpu().numpy(), np.asarray(a))


# ---- voxelize ----------------------------------------------------------------------------------------------------------------

def _boundary_points(G, seed):
    """4096 random points; every coordinate value the rounding can turn on (the issue's x = -1 + 2 (m + 0.5) / G, the cell boundaries
    x = -1 + 2 m / G, each with its f32 neighbours above and below) on each axis in turn and on all three at once; points beyond +-1.  These check
    the rounding mode, the ties and the clamp; a grid on which a fused multiply-subtract lands elsewhere has a test of its own"""
    rs = np.random.RandomState(seed)
    m = np.arange(G + 1, dtype=np.float64)
    x = np.concatenate([-1 + 2 * (m[:-1] + 0.5) / G, -1 + 2 * m / G]).astype(np.float32)
    x = np.concatenate([x, np.nextafter(x, np.float32(np.inf)), np.nextafter(x, np.float32(-np.inf))])
    other = rs.uniform(-1, 1, (len(x), 3)).astype(np.float32)
    sets = [rs.uniform(-1, 1, (4096, 3)).astype(np.float32), np.stack([x, x, x], 1)]
    for ax in range(3):
        p = other.copy()
        p[:, ax] = x
        sets.append(p)
    far = np.array([[1.5, -1.5, 0.3], [-7, 9, 1.0000001], [3e38, -3e38, 0], [1, 1, 1], [-1, -1, -1]], np.float32)
    return np.concatenate(sets + [far])


@pytest.mark.parametrize("G", [32, 33])
def test_voxelize_matches_the_torch_statement(dev, G):
    from shapeformer_amd import morph as M
    a = _boundary_points(G, G)
    nan = np.array([[np.nan, 0, 0], [0.1, np.inf, 0], [0, 0, -np.inf]], np.float32)
    b = np.concatenate([a[::7], nan, a[3::11]])
    sets = [a, np.zeros((0, 3), np.float32), b, nan[:1]]
    off = np.concatenate([[0], np.cumsum([len(s) for s in sets])])
    vox = M.point2voxel_dev(_dev(np.concatenate(sets), dev), off, grid_dim=G)
    assert vox.shape == (4, G, G, G) and vox.dtype == torch.uint8
    for i, s in enumerate(sets):
        assert _eq(vox[i], R.point2voxel(s, G)), i
    assert int(vox[1].sum()) == 0 and int(vox[3].sum()) == 0
    assert vox[0, 0, 0, 0] == 1 and vox[0, G - 1, G - 1, G - 1] == 1
    # (B,N,3) input, and a batch equals the single calls
    pair = np.stack([a[:4000], a[-4000:]])
    v2 = M.point2voxel_dev(_dev(pair, dev), grid_dim=G)
    for i in range(2):
        assert _eq(v2[i], R.point2voxel(pair[i], G))
        assert torch.equal(v2[i], M.point2voxel_dev(_dev(pair[i], dev), grid_dim=G)[0])
    # the gather with the same index
    got = M.voxel_lookup_dev(v2, _dev(pair[::-1].copy(), dev))
    idx = R.point2index(pair[::-1].copy(), G)
    want = np.stack([v2[i].cpu().numpy()[idx[i, :, 0], idx[i, :, 1], idx[i, :, 2]] for i in range(2)])
    assert got.shape == (2, 4000) and _eq(got, want)


def test_voxelize_where_a_fused_multiply_subtract_rounds_differently(dev):
    """At G = 32 and 33 no f32 coordinate tells the reference's two roundings from a fused `p01 * G - 0.5` (morph_ref.fma_sensitive);
    G = 97 is the smallest grid that has one: -0.97938144, exactly between cells 0 and 1 unfused (a tie, half to even: 0), above it
    fused (1).  The kernel must land where the reference does."""
    from shapeformer_amd import morph as M
    G = 97
    x = R.fma_sensitive(G)
    assert len(x) >= 1 and (R.fused_index(x, G) != R.point2index(np.stack([x, x, x], 1), G).numpy()[:, 0]).all()
    rs = np.random.RandomState(97)
    sets = [np.stack([x, x, x], 1)]
    for ax in range(3):
        p = rs.uniform(-1, 1, (len(x), 3)).astype(np.float32)
        p[:, ax] = x
        sets.append(p)
    pts = np.concatenate(sets + [_boundary_points(G, 97)])
    assert _eq(M.point2voxel_dev(_dev(pts, dev), grid_dim=G)[0], R.point2voxel(pts, G))
    only = M.point2voxel_dev(_dev(sets[0], dev), grid_dim=G)[0]
    assert int(only.sum()) == len(np.unique(x)) and int(only[0, 0, 0]) == 1 and int(only[1, 1, 1]) == 0


# ---- dilate / erode ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("G,r", [(24, 3), (33, 6), (40, 1), (16, 2), (20, 16)])
def test_dilate_and_erode_match_scipy(dev, G, r):
    from shapeformer_amd import _lib as L, morph as M
    a, b = R.sparse_grid(G, seed=G), 1 - R.sparse_grid(G, seed=G + 1, p=0.03)
    batch = _dev(np.stack([a, b]), dev)
    d, e = M.ball_dilate_dev(batch, r), M.ball_erode_dev(batch, r)
    for i, v in enumerate((a, b)):
        assert _eq(d[i], R.dilate(v, r)), ("dilate", i)
        assert _eq(e[i], R.erode(v, r)), ("erode", i)
    assert torch.equal(M.ball_dilate_dev(batch[1], r), d[1]) and torch.equal(M.ball_erode_dev(batch[0], r), e[0])
    assert torch.equal(M.ball_dilate_dev(batch, 0), batch) and torch.equal(M.ball_erode_dev(batch, 0), batch)
    full = torch.ones(1, G, G, G, dtype=torch.uint8, device=dev)
    assert torch.equal(M.ball_erode_dev(full, r), full)          # the border counts as set
    assert int(M.ball_dilate_dev(torch.zeros_like(full), r).sum()) == 0
    # the words themselves: pad bits are 0 whatever the flags are, and set pad bits of the input are not lattice points
    Wz = (G + 31) // 32
    bits = M._pack(batch, 2, G)
    ws = M._workspace(2, G, r, dev)
    n_pad = 32 * Wz - G
    pad = (1 << 32) - (1 << (32 - n_pad))                       # the bits k >= G of a row's last word
    assert n_pad > 0
    dirty = bits.clone()
    dirty[..., Wz - 1] |= pad - (1 << 32)                       # the same bits as an int32
    for inv_in in (False, True):
        for inv_out in (False, True):
            w = M._dilate(bits, 2, G, r, inv_in, inv_out, ws)
            assert int((w[..., Wz - 1].contiguous().cpu().numpy().view(np.uint32) & np.uint32(pad)).max()) == 0
            assert torch.equal(M._dilate(dirty, 2, G, r, inv_in, inv_out, ws), w)
    assert torch.equal(M._unpack(M._dilate(bits, 2, G, r, True, True, ws), 2, G), e)
    assert L.lib().sfmi_morph_words(2, G) == bits.numel()


# ---- flood ---------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _flood_cases():
    serp, _ = R.serpentine(32)
    seed_set = R.closed_shell(16)
    seed_set[0:5, 0, 0] = 1                                      # a bar from the seed voxel to the shell: the set component
    seed_set[4, 0:5, 0] = 1
    seed_set[4, 4, 0:5] = 1
    seed_set[12, 14, 14] = 1                                     # and a set voxel that is not joined to it
    rs = np.random.RandomState(5)
    return {
        "empty": np.zeros((16, 16, 16), np.uint8),
        "full": np.ones((16, 16, 16), np.uint8),
        "closed_shell": R.closed_shell(16),
        "diagonal_chambers": R.diagonal_chambers(12),
        "serpentine": serp,
        "serpentine_mirrored": np.ascontiguousarray(serp[:, :, ::-1]),
        "seed_set": seed_set,
        "G33_noise": (rs.rand(33, 33, 33) < 0.25).astype(np.uint8) * (np.indices((33, 33, 33)).sum(0) > 0),
        "G33_shell": R.closed_shell(33),
        "G40_caves": (ndimage_smooth(rs.rand(40, 40, 40)) > 0.5).astype(np.uint8) * (np.indices((40, 40, 40)).sum(0) > 2),
    }


def ndimage_smooth(a):
    from scipy import ndimage
    return ndimage.uniform_filter(a, 5)


@pytest.mark.parametrize("name", ["empty", "full", "closed_shell", "diagonal_chambers", "serpentine", "serpentine_mirrored", "seed_set",
                                  "G33_noise", "G33_shell", "G40_caves"])
def test_flood_matches_the_statement(dev, name):
    from shapeformer_amd import morph as M
    v = _flood_cases()[name]
    want, st = R.flood(v)
    region, status = M.flood_dev(_dev(v, dev))
    assert region.shape == v.shape and status.tolist() == [st]
    assert _eq(region, want)
    if name == "empty":
        assert int(region.sum()) == v.size
    if name == "full":
        assert st == 3 and int(region.sum()) == v.size
    if name == "closed_shell":
        assert region[8, 8, 8] == 0 and region[15, 15, 15] == 1
    if name == "diagonal_chambers":
        assert region[5, 5, 5] == 1                              # 6-connectivity would stop at the vertex
    if name == "serpentine":
        assert _eq(region, R.serpentine(32)[1])
    if name == "seed_set":
        assert st == 3 and region[8, 4, 8] == 1 and region[12, 14, 14] == 0 and region[8, 8, 8] == 0


def test_flood_batch_equals_single_calls(dev):
    from shapeformer_amd import morph as M
    cases = _flood_cases()
    vs = [cases["closed_shell"], cases["seed_set"], cases["empty"], cases["full"]]
    region, status = M.flood_dev(_dev(np.stack(vs), dev))
    assert status.tolist() == [0, 3, 0, 3]
    for i, v in enumerate(vs):
        r1, s1 = M.flood_dev(_dev(v, dev))
        assert torch.equal(region[i], r1) and _eq(r1, R.flood(v)[0])


# ---- the fill ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("G,r", [(24, 3), (33, 6), (20, 1), (16, 2)])
def test_watertight_fill_matches_the_statement(dev, G, r):
    from shapeformer_amd import morph as M
    a, _ = R.shell_grid(G, r, seed=1)
    b, _ = R.shell_grid(G, r, seed=2, noise=0.01)
    b[G // 4 + 2:G // 2, G // 2, G // 2] = 1
    batch = _dev(np.stack([a, b]), dev)
    for sel in (r, 0):
        out, status = M.watertight_fill_dev(batch, sel, return_status=True)
        for i, v in enumerate((a, b)):
            want, st = R.watertight_fill(v, sel)
            assert _eq(out[i], want), (sel, i)
            assert int(status[i]) == st
            one = M.watertight_fill_dev(batch[i], sel)
            assert one.shape == (G, G, G) and torch.equal(one, out[i])          # a batch equals the single calls


# ---- end to end ----------------------------------------------------------------------------------------------------------------

def test_soup_cube_end_to_end(dev):
    """A cube [-0.5, 0.5]^3 as a soup: half its faces flipped, a square hole in one side, an interior partition.  What the
    winding-number route gives for it is recorded here, not asserted (measured on an MI355X, profiles/r17_kbench_morph.txt):
    mesh_occupancy_dev on the 32^3 lattice marks 0 of the 4096 lattice points inside the cube and 0 of those outside: with half the
    faces flipped the winding number cancels, |W| stays below 0.5 everywhere, and status is 0.  The watertight voxels of this test
    mark all 2744 cells whose centre is more than one cell inside the cube and none whose centre is more than one cell outside."""
    from shapeformer_amd import morph as M
    G, r, n = 32, 2, 20000
    v, f = R.soup_cube()
    vd, fd = _dev(v, dev), _dev(f, dev)
    vox, coords, status, samples = M.morph_voxelization_dev(vd, fd, sampleN=n, grid_dim=G, selem_size=r, seed=0, return_status=True,
                                                            return_coords=True, return_samples=True)
    assert vox.shape == (1, G, G, G) and samples.shape == (1, n, 3) and status.tolist() == [0]
    want, st = R.morph_from_samples(samples[0].cpu().numpy(), G, r)
    assert st == 0 and _eq(vox[0], want)
    assert _eq(coords, R.index2point(G))
    c = np.abs(R.index2point(G)).max(1).reshape(G, G, G)
    cell = 2.0 / G
    got = vox[0].cpu().numpy()
    assert got[c <= 0.5 - 2 * cell].all() and (c <= 0.5 - 2 * cell).sum() == 12 ** 3
    assert not got[c >= 0.5 + 2 * cell].any()
    # two runs give identical bits; a batch of two (the soup and a scaled copy) equals the single calls
    again = M.morph_voxelization_dev(vd, fd, sampleN=n, grid_dim=G, selem_size=r, seed=0)
    assert torch.equal(again, vox)
    both = M.morph_voxelization_dev(torch.cat([vd, vd * 1.5]), torch.cat([fd, fd]), [0, len(v), 2 * len(v)], [0, len(f), 2 * len(f)],
                                    sampleN=n, grid_dim=G, selem_size=r, seed=0)
    assert torch.equal(both[0], vox[0])
    assert torch.equal(both[1], M.morph_voxelization_dev(vd * 1.5, fd, sampleN=n, grid_dim=G, selem_size=r, seed=0)[0])
    big = np.abs(R.index2point(G)).max(1).reshape(G, G, G) <= 0.75 - 2 * cell
    assert both[1].cpu().numpy()[big].all()


def test_determinism(dev):
    from shapeformer_amd import morph as M
    G, r = 33, 6
    a, _ = R.shell_grid(G, r, seed=3, noise=0.02)
    serp, _ = R.serpentine(32)
    x, s = _dev(a, dev), _dev(serp, dev)
    pts = _dev(_boundary_points(G, 9), dev)
    first = (M.watertight_fill_dev(x, r), M.flood_dev(s)[0], M.point2voxel_dev(pts, grid_dim=G), M.ball_dilate_dev(x, r))
    for _ in range(3):
        again = (M.watertight_fill_dev(x, r), M.flood_dev(s)[0], M.point2voxel_dev(pts, grid_dim=G), M.ball_dilate_dev(x, r))
        assert all(torch.equal(p, q) for p, q in zip(first, again))


# ---- make_dataset --------------------------------------------------------------------------------------------------------------

def test_make_dataset_morph_route(dev, tmp_path):
    from shapeformer_amd import data as D, make_dataset as MD, meshio, meshsdf, morph as M
    from shapeformer_amd.metrics import sample_mesh_dev
    v, f = R.soup_cube()
    p = str(tmp_path / "soup.ply")
    meshio.write_ply(p, v, f)
    args = [p, "--out", str(tmp_path), "--dataset", "d", "--grid", "16", "--boundary-n", "64", "--occupancy", "morph", "--morph-grid", "32",
            "--selem", "2", "--morph-samples", "20000"]
    with pytest.raises(ValueError, match=r"soup\.ply.*--scale 0\.9"):       # normalised, the cube fills the box: the corner voxel is set
        MD.main(args)
    MD.main(args + ["--scale", "0.5"])
    Ytg = np.unpackbits(np.load(tmp_path / "d" / "train" / "Ytg.npy"), axis=-1).reshape(16, 16, 16)
    vn = (meshsdf.normalize_point_set(v) * 0.5).astype(np.float32)
    vd, fd = _dev(vn, dev), _dev(f, dev)
    samples = sample_mesh_dev(vd, fd, None, None, 20000, seed=0)[0]
    vox, st = R.morph_from_samples(samples.cpu().numpy(), 32, 2)
    lattice = D.make_grid([-1, -1, -1.], [1., 1, 1], [16] * 3).astype(np.float32)
    idx = R.point2index(lattice, 32).numpy()
    assert st == 0 and np.array_equal(Ytg.reshape(-1), vox[idx[:, 0], idx[:, 1], idx[:, 2]])
    inside = np.abs(lattice).max(1) <= 0.5 - 2 * 2.0 / 32
    assert Ytg.reshape(-1)[inside].all() and inside.sum() > 0
    Xbd = np.load(tmp_path / "d" / "train" / "Xbd.npy")
    assert Xbd.shape == (1, 64, 3) and np.abs(Xbd).max() <= 0.5 + 1e-6
