"""f64 restatement of hidden-point removal for the hpr tests: a point is visible iff it is a vertex of the convex hull of the
spherically flipped cloud plus the viewpoint, i.e. iff a plane through its flipped image f_i leaves every other point strictly on
the side of the viewpoint.  With w = u + a e1 + b e2 (u = f_i / |f_i|) that is the feasibility of a 2-D linear program in (a, b),
solved here by Seidel's incremental algorithm with the constraints in index order.  The device kernel (csrc/hpr.hip) is judged
against scipy's qhull; this file lets the CPU suite pin the mathematics without a device."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from shapeformer_amd import data as D  # noqa: E402

EPS, BOX = 1e-9, 1e3


def visible_mask(X, cam):
    X = X.astype(np.float64); f = D.spherical_flip(X, np.asarray(cam, float)[None], np.pi)
    P = np.concatenate([np.zeros((1, 3)), f]); out = np.zeros(len(X), bool)
    for i in range(len(X)):
        u = f[i] / np.linalg.norm(f[i]); e = np.zeros(3); e[np.argmin(np.abs(u))] = 1
        e1 = np.cross(u, e); e1 /= np.linalg.norm(e1); e2 = np.cross(u, e1)
        g = P - f[i]; nn = np.linalg.norm(g, axis=1)
        if (nn[1:i + 1] == 0).any(): continue                    # an earlier duplicate represents it
        g = g[nn > 0] / nn[nn > 0, None]
        al, be, ga = g @ u + EPS, g @ e1, g @ e2                  # al + be a + ga b <= 0
        a = b = -BOX; j = 0; ok = True                            # objective: min a, then b
        while ok:
            v = np.nonzero(al[j:] + be[j:] * a + ga[j:] * b > 0)[0]
            if not len(v): break
            j += v[0]; nb = np.array([be[j], ga[j]]); p0 = -al[j] * nb / (nb @ nb); d = np.array([-ga[j], be[j]])
            A = np.concatenate([be[:j] * d[0] + ga[:j] * d[1], [d[0], -d[0], d[1], -d[1]]])
            C = np.concatenate([al[:j] + be[:j] * p0[0] + ga[:j] * p0[1], [p0[0] - BOX, -p0[0] - BOX, p0[1] - BOX, -p0[1] - BOX]])
            if (C[A == 0] > 1e-12).any(): ok = False; break       # parallel: tolerance, never `> 0`
            hi = (-C[A > 0] / A[A > 0]).min(); lo = (-C[A < 0] / A[A < 0]).max()
            if lo > hi: ok = False; break
            a, b = p0 + (lo if d[0] > 0 else hi if d[0] < 0 else lo if d[1] > 0 else hi) * d; j += 1
        out[i] = ok
    return out


def row_set(rows):
    """coordinate rows as a set of byte strings (rows compared as sets, duplicates collapsed)"""
    rows = np.ascontiguousarray(rows)
    return {r.tobytes() for r in rows}


def rows_differing(a, b):
    return len(row_set(a) ^ row_set(b))
