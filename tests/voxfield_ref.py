"""The numpy / scipy statement of the voxel-field contract (include/sfmi.h, "Smooth fields from binary voxel grids"):
what csrc/edt.hip must compute, written so that it can be read in a page.  Integer or fixed-order f64 arithmetic throughout, so the
device's results are compared with these bit for bit (the Gaussian: within a derived bound).  Grids are (G,G,G) bool arrays."""
from __future__ import annotations

import numpy as np
from scipy import ndimage


# ---- distance transform ----------------------------------------------------------------------------------------------------

def edt_sq_brute(grid, invert=False):
    """d2[v] = min |u - v|^2 over the voxels u that are set (invert: clear), by the double loop; 3 G^2 for an empty set.  Tiny grids."""
    g = np.asarray(grid, bool) ^ bool(invert)
    G = g.shape[0]
    pts = np.argwhere(g).astype(np.int64)
    if len(pts) == 0:
        return np.full(g.shape, 3 * G * G, np.int32)
    v = np.stack(np.meshgrid(*[np.arange(G)] * 3, indexing="ij"), -1).reshape(-1, 1, 3).astype(np.int64)
    return ((v - pts[None]) ** 2).sum(-1).min(1).reshape(g.shape).astype(np.int32)


def edt_sq(grid, invert=False):
    """the same through scipy (exact: test_voxfield_cpu.py checks it against the double loop), for grids of any size"""
    g = np.asarray(grid, bool) ^ bool(invert)
    G = g.shape[0]
    if not g.any():
        return np.full(g.shape, 3 * G * G, np.int32)
    return np.rint(ndimage.distance_transform_edt(~g) ** 2).astype(np.int32)


def edt_status(grid, invert=False):
    return int(not (np.asarray(grid, bool) ^ bool(invert)).any())


def signed_distance(grid, d2_to_clear=None, d2_to_set=None):
    """positive inside: sqrt(d2 to the nearest clear voxel) - 0.5 on a set voxel, -sqrt(d2 to the nearest set voxel) + 0.5 on a clear one"""
    g = np.asarray(grid, bool)
    a = edt_sq(g, True) if d2_to_clear is None else d2_to_clear
    b = edt_sq(g, False) if d2_to_set is None else d2_to_set
    return np.where(g, np.sqrt(a.astype(np.float64)) - 0.5, -np.sqrt(b.astype(np.float64)) + 0.5)


def signed_status(grid):
    g = np.asarray(grid, bool)
    return int(g.all() or not g.any())


# ---- Gaussian --------------------------------------------------------------------------------------------------------------

def gaussian(grid, sigma):
    return ndimage.gaussian_filter(np.asarray(grid, bool).astype(np.float64) - 0.5, sigma, mode="reflect")


# ---- constrained smoothing -------------------------------------------------------------------------------------------------

def laplace(u):
    """the Neumann Laplacian: indices clamped to the lattice, the sum in the contract's order, every operation rounded on its own"""
    p = np.pad(u, 1, mode="edge")
    c = slice(1, -1)
    s = p[2:, c, c] + p[:-2, c, c]
    s = s + p[c, 2:, c]
    s = s + p[c, :-2, c]
    s = s + p[c, c, 2:]
    s = s + p[c, c, :-2]
    return s - 6.0 * u


def energy(u):
    return 0.5 * float((laplace(u) ** 2).sum())


def band_of(d, band_radius=4.0):
    return np.abs(d) <= band_radius


def support_of(band):
    """the band and the voxels one clamped step from it: where L u is needed"""
    p = np.pad(band, 1, mode="edge")
    c = slice(1, -1)
    return band | p[2:, c, c] | p[:-2, c, c] | p[c, 2:, c] | p[c, :-2, c] | p[c, c, 2:] | p[c, c, :-2]


def constrained_step(u, d, grid, band):
    g = laplace(laplace(u))
    x = u - g / 84.0
    lo = np.where(grid, 0.0, -np.inf)
    hi = np.where(grid, np.inf, 0.0)
    x = np.where(x > hi, hi, x)                 # max(lo, min(hi, x)), a -0.0 left as it is
    x = np.where(x < lo, lo, x)
    return np.where(band, x, d)


def constrained(grid, d=None, band_radius=4.0, iters=200, trace=None):
    """u_0 = d; iters Jacobi steps.  trace: a list that receives E(u) before the first step and after every step"""
    g = np.asarray(grid, bool)
    d = signed_distance(g) if d is None else np.asarray(d, np.float64)
    band = band_of(d, band_radius)
    u = d.copy()
    if trace is not None:
        trace.append(energy(u))
    for _ in range(iters):
        u = constrained_step(u, d, g, band)
        if trace is not None:
            trace.append(energy(u))
    return u


# ---- the grids the tests share ---------------------------------------------------------------------------------------------

def sphere(G, r, centre=None):
    c = [(G - 1) / 2.0] * 3 if centre is None else centre
    i, j, k = np.meshgrid(*[np.arange(G, dtype=np.float64)] * 3, indexing="ij")
    return (i - c[0]) ** 2 + (j - c[1]) ** 2 + (k - c[2]) ** 2 <= r * r


def solve_grids():
    """name -> grid: an off-centre sphere at 17^3 and 33^3, thresholded smoothed noise at 17^3 and a slab on the lattice face at 17^3.
    The band touches the lattice face in all but the 33^3 sphere."""
    rng = np.random.default_rng(5)
    noise = ndimage.gaussian_filter(rng.standard_normal((17, 17, 17)), 1.5) > 0.0
    slab = np.zeros((17, 17, 17), bool)
    slab[:5] = True
    return {"sphere17": sphere(17, 5.3, (6.2, 8.9, 9.4)), "sphere33": sphere(33, 10.3, (16.4, 16.9, 15.8)), "noise17": noise, "slab17": slab}


def radius_std(field, centre, axis_lines=True):
    """std of the radius of the zero crossings of `field` along the lattice lines (linear interpolation between neighbouring voxels)"""
    G = field.shape[0]
    idx = np.stack(np.meshgrid(*[np.arange(G, dtype=np.float64)] * 3, indexing="ij"), -1)
    radii = []
    for ax in range(3):
        a = np.moveaxis(field, ax, 0)
        p = np.moveaxis(idx, ax, 0)
        f0, f1 = a[:-1], a[1:]
        cross = (f0 > 0) != (f1 > 0)
        t = f0[cross] / (f0[cross] - f1[cross])
        pos = p[:-1][cross] + t[:, None] * (p[1:][cross] - p[:-1][cross])
        radii.append(np.sqrt(((pos - np.asarray(centre)) ** 2).sum(-1)))
    return float(np.concatenate(radii).std())
