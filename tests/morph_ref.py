"""numpy / scipy / torch-CPU statement of the watertight-voxelization contract (include/sfmi.h): what
xgutils/geoutil.py:383-401 morph_voxelization computes after its surface samples, and the grids the tests run it on.

skimage is not installed where these tests run (the oracle stubs it), so morph_voxelization itself cannot be recorded as a golden
fixture.  This restatement is pinned to what skimage's functions call instead:
  morphology.ball(r)                   x^2 + y^2 + z^2 <= r^2 on the (2r+1)^3 stencil                                  -> ball
  morphology.binary_dilation(a, s)     scipy.ndimage.binary_dilation(a, structure=s)                                   -> dilate
  morphology.binary_erosion(a, s)      scipy.ndimage.binary_erosion(a, structure=s, border_value=True)                 -> erode
  morphology.flood(a, (0,0,0))         the voxels equal to a[0,0,0] and connected to it with connectivity=None, i.e. the full
                                       3^3 neighbourhood: ndimage.label(a == a[0,0,0], structure=ones((3,3,3)))          -> flood
  ptutil.point2voxel / point2index     f32 torch, exactly as the reference writes it                                   -> point2voxel
The flood's default connectivity (None = ndim = 26 neighbours) and the erosion's border_value=True are taken from skimage's documented
behaviour; they were not run here.
"""
import numpy as np
import torch
from scipy import ndimage


def ball(r):
    a = np.arange(-r, r + 1)
    X, Y, Z = np.meshgrid(a, a, a, indexing="ij")
    return (X * X + Y * Y + Z * Z) <= r * r


def dilate(vox, r):
    return ndimage.binary_dilation(np.asarray(vox) != 0, structure=ball(r)).astype(np.uint8)


def erode(vox, r):
    return ndimage.binary_erosion(np.asarray(vox) != 0, structure=ball(r), border_value=1).astype(np.uint8)


def flood(vox, structure=None):
    """-> region uint8, status (3: the seed voxel was set, the flood ran over the set voxels)"""
    a = np.asarray(vox) != 0
    lab, _ = ndimage.label(a == a[0, 0, 0], structure=np.ones((3, 3, 3)) if structure is None else structure)
    return (lab == lab[0, 0, 0]).astype(np.uint8), (3 if a[0, 0, 0] else 0)


def watertight_fill(vox, selem_size):
    """geoutil.py:393-400 -> voxels uint8, status"""
    vox = (np.asarray(vox) != 0).astype(np.uint8)
    if selem_size == 0:
        region, st = flood(vox)
        return (1 - region).astype(np.uint8), st
    region, st = flood(dilate(vox, selem_size))
    return erode(1 - region, selem_size), st


def point2index(points, grid_dim):
    """ptutil.point2index:446-450 (torch f32)"""
    points = torch.as_tensor(points, dtype=torch.float32)
    points01 = (points + 1) / 2
    shift_points = points01 * grid_dim - 0.5
    return torch.clamp(torch.round(shift_points), min=0.0, max=grid_dim - 1).long()


def point2voxel(points, grid_dim):
    """ptutil.point2voxel:533-543 for one set of points (n,3) -> (G,G,G) uint8; rows with a non-finite coordinate are skipped (the
    reference's behaviour there is undefined; the contract's is not)"""
    points = torch.as_tensor(points, dtype=torch.float32).reshape(-1, 3)
    points = points[torch.isfinite(points).all(1)]
    voxel = torch.zeros(grid_dim, grid_dim, grid_dim, dtype=torch.uint8)
    inds = point2index(points, grid_dim)
    voxel[inds[:, 0], inds[:, 1], inds[:, 2]] = 1
    return voxel.numpy()


def fused_index(x, grid_dim):
    """the index of coordinates x (f32) if `points01 * grid_dim - 0.5` were ONE rounding (a fused multiply-subtract, what a compiler
    that contracts makes of it): the product of a 24-bit and a small integer is exact in f64"""
    x = np.asarray(x, np.float32)
    p01 = ((x + np.float32(1)) / np.float32(2)).astype(np.float32)
    s = (p01.astype(np.float64) * grid_dim - 0.5).astype(np.float32)
    return np.clip(np.rint(s), 0, grid_dim - 1).astype(np.int64)


def fma_sensitive(grid_dim, span=8):
    """the f32 coordinates within `span` ulps of a cell boundary x = -1 + 2 m / G whose index differs between the reference's two
    roundings and a fused multiply-subtract.  The two can only part where the unfused sum is an exact tie (m - 0.5) and the fused one
    is not, which takes a coincidence of G and the f32 grid: there is none at G = 32, 33 or 40, and one at G = 97, 194 and 257 each."""
    m = np.arange(1, grid_dim)
    x0 = (-1 + 2 * m / grid_dim).astype(np.float32)
    x = (x0[:, None] + np.arange(-span, span + 1, dtype=np.float32)[None, :] * np.spacing(x0)[:, None]).astype(np.float32).reshape(-1)
    two = point2index(np.stack([x, x, x], 1), grid_dim).numpy()[:, 0]
    return x[fused_index(x, grid_dim) != two]


def index2point(grid_dim):
    """ptutil.index2point of every cell -> (G^3, 3) f32, first axis slowest"""
    c = (torch.arange(grid_dim, dtype=torch.float32) + 0.5) / grid_dim * 2 - 1
    return torch.stack(torch.meshgrid(c, c, c, indexing="ij"), -1).reshape(-1, 3).numpy()


def morph_from_samples(samples, grid_dim, selem_size):
    return watertight_fill(point2voxel(samples, grid_dim), selem_size)


# ---- grids ---------------------------------------------------------------------------------------------------------------------

def shell_grid(G, r, seed=0, noise=0.002):
    """A box shell on [G/4, 3G/4], a square hole of side 2(r-1) cells in its +x face, an interior wall, two isolated voxels near the
    border and `noise` random voxels.  Noise within r cells of the corner (0,0,0) on every axis is dropped, so that the dilated
    grid's seed voxel stays empty.  -> vox uint8, interior mask (strictly inside the shell, the wall included)"""
    lo, hi = G // 4, (3 * G) // 4
    v = np.zeros((G, G, G), np.uint8)
    v[lo:hi + 1, lo:hi + 1, lo:hi + 1] = 1
    v[lo + 1:hi, lo + 1:hi, lo + 1:hi] = 0
    side, c = 2 * (r - 1), (lo + hi) // 2
    if side > 0:
        v[hi, c - side // 2:c - side // 2 + side, c - side // 2:c - side // 2 + side] = 0
    v[lo + 1:hi, c + 1, lo + 1:hi - 1] = 1                       # the wall leaves a gap of one voxel at the top
    v[1, G // 2, G // 2] = 1
    v[G - 2, G // 2, 2] = 1
    rs = np.random.RandomState(seed)
    n = rs.rand(G, G, G) < noise
    n[:r + 1, :r + 1, :r + 1] = False
    v[n] = 1
    inside = np.zeros((G, G, G), bool)
    inside[lo + 1:hi, lo + 1:hi, lo + 1:hi] = True
    return v, inside


def sparse_grid(G, seed=0, p=0.01):
    """random sparse voxels plus set voxels in the corners and on the faces (padding and clipping)"""
    rs = np.random.RandomState(seed)
    v = (rs.rand(G, G, G) < p).astype(np.uint8)
    for c in np.ndindex(2, 2, 2):
        v[tuple((G - 1) * np.array(c))] = 1
    m = G // 2
    for ax in range(3):
        for end in (0, G - 1):
            idx = [m, m - 1, m + 1]
            idx[ax] = end
            v[tuple(idx)] = 1
    return v


def closed_shell(G):
    v = np.zeros((G, G, G), np.uint8)
    lo, hi = G // 4, (3 * G) // 4
    v[lo:hi + 1, lo:hi + 1, lo:hi + 1] = 1
    v[lo + 1:hi, lo + 1:hi, lo + 1:hi] = 0
    return v


def diagonal_chambers(G=12):
    """a full grid with two empty chambers, [0,4)^3 and [4,8)^3: voxels (3,3,3) and (4,4,4) touch across a vertex only"""
    v = np.ones((G, G, G), np.uint8)
    v[0:4, 0:4, 0:4] = 0
    v[4:8, 4:8, 4:8] = 0
    return v


def serpentine(G=32):
    """a full grid with an empty corridor one voxel wide from (0,0,0) through every even plane, every even row of it, end to end: one
    chain of ~G^3 / 4 voxels.  -> vox, corridor mask"""
    v = np.ones((G, G, G), np.uint8)
    side = 0                                                    # the k at which the current row is entered
    for n, i in enumerate(range(0, G, 2)):
        rows = list(range(0, G, 2))
        if n % 2:
            rows.reverse()                                      # the next plane is entered in the row the last one ended in
        for m, j in enumerate(rows):
            v[i, j, :] = 0
            side = G - 1 - side                                 # the row is left at its other end
            if m + 1 < len(rows):
                v[i, (j + rows[m + 1]) // 2, side] = 0          # to the next row of the plane
        if i + 2 < G:
            v[i + 1, rows[-1], side] = 0                        # to the next plane
    return v, v == 0


# ---- the soup of the end-to-end test ---------------------------------------------------------------------------------------

def soup_cube(n=8):
    """A cube [-0.5, 0.5]^3 as a triangle soup (every triangle has its own three vertices): each side n x n quads, one quad of the +x
    side cut out (a square hole of side 1/n), an interior partition at x = 0, every second triangle flipped.
    -> verts (V,3) f32, faces (T,3) int32"""
    t = np.linspace(-0.5, 0.5, n + 1)
    tris = []

    def quad(p00, p10, p11, p01):
        tris.append([p00, p10, p11])
        tris.append([p00, p11, p01])

    def side(axis, x, skip=None):
        u, w = [a for a in range(3) if a != axis]
        for a in range(n):
            for b in range(n):
                if skip == (a, b):
                    continue
                def p(ua, wb):
                    q = [0.0, 0.0, 0.0]
                    q[axis], q[u], q[w] = x, ua, wb
                    return q
                quad(p(t[a], t[b]), p(t[a + 1], t[b]), p(t[a + 1], t[b + 1]), p(t[a], t[b + 1]))

    for axis in range(3):
        side(axis, -0.5)
        side(axis, 0.5, skip=(n // 2, n // 2) if axis == 0 else None)
    side(0, 0.0)                                                 # the partition
    tri = np.asarray(tris, np.float32)
    tri[1::2] = tri[1::2, ::-1]                                  # half the faces flipped
    verts = tri.reshape(-1, 3)
    faces = np.arange(len(verts), dtype=np.int32).reshape(-1, 3)
    return verts, faces
