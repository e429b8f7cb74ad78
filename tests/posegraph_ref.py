"""Multiway registration, the numpy statement of the contract of include/sfmi.h (csrc/posegraph.hip): the information
matrix of a registered pair, the pose-graph residual and its Jacobians, the Levenberg-Marquardt loop with a line process over the
uncertain edges, Open3D's two passes, and the whole pipeline on top of tests/icp_ref.py.  One graph at a time, f64.  Also here: the
scenes of the tests (synthetic graphs; the armchair fixture cut into a ring and a chain of overlapping scans).

Poses are 12 doubles, row-major [R | t], as in icp_ref.  A node pose X takes the scan's frame to the frame of node 0; an edge
(src, tgt, T) states p_tgt = T p_src, so its residual is D = T^-1 X_tgt^-1 X_src, the identity when the graph is consistent."""
import numpy as np

import icp_ref as R

MAX_NODES, MAX_EDGES = 32, 496
THETA_MAX = 3.1
# The ring scene's star (every scan onto scan 0) against its pose graph, in Chamfer distance to the fixture: the star loses the scans
# that share nothing with scan 0, a sixth of the object; a slab of width w left uncovered costs about (1/6) (w/4)^2 ~ 1e-4 for w ~ 0.1,
# where poses good to ~1e-4 cost ~1e-8.  Two orders of magnitude are asserted (tests/test_posegraph_cpu.py finds five).
STAR_FACTOR = 100.0
LAMBDA_MIN, LAMBDA_MAX = 1e-12, 1e12


# ---- SE(3) on 12 doubles -------------------------------------------------------------------------------------------------------------

def inv12(p):
    T = np.asarray(p, np.float64).reshape(3, 4)
    return R.pose12(T[:, :3].T, -(T[:, :3].T @ T[:, 3]))


def mul12(a, b):
    A, B = np.asarray(a, np.float64).reshape(3, 4), np.asarray(b, np.float64).reshape(3, 4)
    return R.pose12(A[:, :3] @ B[:, :3], A[:, :3] @ B[:, 3] + A[:, 3])


def skew(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], np.float64)


def rotvec(Rm):
    """-> (w, theta): w = theta / (2 sin theta) vee(R - R^T), theta = atan2(|vee| / 2, (tr - 1) / 2); the series below 1e-4"""
    Rm = np.asarray(Rm, np.float64)
    v = np.array([Rm[2, 1] - Rm[1, 2], Rm[0, 2] - Rm[2, 0], Rm[1, 0] - Rm[0, 1]])
    s = 0.5 * np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    c = 0.5 * (((Rm[0, 0] + Rm[1, 1]) + Rm[2, 2]) - 1.0)
    th = np.arctan2(s, c)
    t2 = th * th
    f = 0.5 * (1.0 + t2 / 6.0 + 7.0 * t2 * t2 / 360.0) if th < 1e-4 else th / (2.0 * np.sin(th))
    return f * v, th


def jl_inv(w, th):
    """Jl^-1(w) = I - [w]x / 2 + (1 / th^2 - (1 + cos th) / (2 th sin th)) [w]x^2; the series 1/12 + th^2/720 below 1e-4"""
    K = skew(w)
    t2 = th * th
    k = 1.0 / 12.0 + t2 / 720.0 if th < 1e-4 else 1.0 / t2 - (1.0 + np.cos(th)) / (2.0 * th * np.sin(th))
    return np.eye(3) - 0.5 * K + k * (K @ K)


def residual(xs, xt, T):
    """-> r (6,) = (w, v) of D = T^-1 X_tgt^-1 X_src, theta, A = T^-1 X_tgt^-1"""
    A = mul12(inv12(T), inv12(xt))
    D = mul12(A, xs).reshape(3, 4)
    w, th = rotvec(D[:, :3])
    return np.concatenate([w, D[:, 3]]), th, A


def jacobian(xs, xt, T):
    """J_src (6,6) = d r / d (dw, dv) of the source node under R <- dR R, t <- dR t + dv; J_tgt = -J_src"""
    r, th, A = residual(xs, xt, T)
    RA = A.reshape(3, 4)[:, :3]
    ts = np.asarray(xs, np.float64).reshape(3, 4)[:, 3]
    J = np.zeros((6, 6))
    J[:3, :3] = jl_inv(r[:3], th) @ RA
    J[3:, :3] = -RA @ skew(ts)
    J[3:, 3:] = RA
    return J


# ---- the optimiser -------------------------------------------------------------------------------------------------------------------

def evaluate(X, src, tgt, T, Lam, unc, alive, mu):
    """-> F, q (E,), l (E,), the largest theta over the alive edges.  l = 1 for certain edges and when the line process is off"""
    E = len(src)
    q, l, thmax, F = np.zeros(E), np.zeros(E), 0.0, 0.0
    for e in range(E):
        if not alive[e]:
            continue
        r, th, _ = residual(X[src[e]], X[tgt[e]], T[e])
        thmax = max(thmax, th)
        q[e] = r @ Lam[e] @ r
        if unc[e] and mu > 0:
            s = mu / (mu + q[e])
            l[e] = s * s
            F += l[e] * q[e] + mu * (s - 1.0) ** 2
        else:
            l[e] = 1.0
            F += q[e]
    return F, q, l, thmax


def normal_equations(X, src, tgt, T, Lam, alive, l):
    """H (n,n), g (n,) over the 6 (S - 1) free variables, and the sums of |term| that scale a bound on another summation order:
    Ha = sum l |J|^T |Lam| |J|, Ga = sum l |J|^T |Lam| |r|, and Gr = sum l |J|^T |Lam| 1 r_error, what the absolute error of the residuals
    themselves can move g by"""
    S, E = len(X), len(src)
    n = 6 * (S - 1)
    H, g, Ha, Ga, Gr = np.zeros((n + 6, n + 6)), np.zeros(n + 6), np.zeros((n + 6, n + 6)), np.zeros(n + 6), np.zeros(n + 6)
    for e in range(E):
        if not alive[e]:
            continue
        r, _, _ = residual(X[src[e]], X[tgt[e]], T[e])
        J = jacobian(X[src[e]], X[tgt[e]], T[e])
        M, b = l[e] * (J.T @ Lam[e] @ J), l[e] * (J.T @ Lam[e] @ r)
        Ma = l[e] * (np.abs(J).T @ np.abs(Lam[e]) @ np.abs(J))
        ba = l[e] * (np.abs(J).T @ np.abs(Lam[e]) @ np.abs(r))
        br = l[e] * (np.abs(J).T @ np.abs(Lam[e]) @ np.full(6, r_error(X[src[e]], X[tgt[e]], T[e])))
        s, t = 6 * src[e], 6 * tgt[e]
        for (i, j, sg) in ((s, s, 1), (t, t, 1), (s, t, -1), (t, s, -1)):
            H[i:i + 6, j:j + 6] += sg * M
            Ha[i:i + 6, j:j + 6] += Ma
        g[s:s + 6] -= b
        g[t:t + 6] += b
        Ga[s:s + 6] += ba
        Ga[t:t + 6] += ba
        Gr[s:s + 6] += br
        Gr[t:t + 6] += br
    return H[6:, 6:], g[6:], Ha[6:, 6:], Ga[6:], Gr[6:]


def r_error(xs, xt, T):
    """the absolute error of a residual computed in f64 by any order of the three products: 32 eps (1 + the largest translation)"""
    big = max(np.abs(np.asarray(p, np.float64).reshape(3, 4)[:, 3]).max() for p in (xs, xt, T))
    return 32 * np.finfo(np.float64).eps * (1.0 + big)


def cost_slack(X, src, tgt, T, Lam, alive):
    """what the absolute error of the residuals (r_error) can move F = sum r^T Lam r by: sum_e 2 r_error sum_ij |Lam_ij| |r_j|"""
    out = 0.0
    for e in range(len(src)):
        if alive[e]:
            r, _, _ = residual(X[src[e]], X[tgt[e]], T[e])
            out += 2.0 * r_error(X[src[e]], X[tgt[e]], T[e]) * (np.abs(Lam[e]) @ np.abs(r)).sum()
    return out


def cholesky_solve(A, g):
    """-> x or None: a pivot that is not positive and finite"""
    A = A.copy()
    n = len(A)
    for j in range(n):
        d = A[j, j] - (A[j, :j] ** 2).sum()
        if not d > 0 or not np.isfinite(d):
            return None
        A[j, j] = np.sqrt(d)
        A[j + 1:, j] = (A[j + 1:, j] - A[j + 1:, :j] @ A[j, :j]) / A[j, j]
    Lo = np.tril(A)
    return np.linalg.solve(Lo.T, np.linalg.solve(Lo, g))


def connected(S, src, tgt, alive):
    """(S,) bool: a chain of alive edges joins the node to node 0"""
    lab = np.arange(S)
    for _ in range(S):
        for e in range(len(src)):
            if alive[e]:
                lab[src[e]] = lab[tgt[e]] = min(lab[src[e]], lab[tgt[e]])
    return lab == 0


def optimize(X, src, tgt, T, Lam, unc, alive=None, mu=0.0, max_iter=100, tol=1e-10):
    """One graph.  -> dict(X (S,12), l (E,), cost, iterations, status, and of the last iteration H, g, delta, lam)"""
    X = np.array(X, np.float64).reshape(-1, 12)
    src, tgt = np.asarray(src, np.int64).reshape(-1), np.asarray(tgt, np.int64).reshape(-1)
    S, E = len(X), len(src)
    T, Lam = np.asarray(T, np.float64).reshape(E, 12), np.asarray(Lam, np.float64).reshape(E, 6, 6)
    unc = np.asarray(unc).reshape(E) != 0
    alive = np.ones(E, bool) if alive is None else np.asarray(alive).reshape(E) != 0
    out = dict(X=X, l=np.zeros(E), cost=0.0, iterations=0, status=4, H=None, g=None, delta=None, lam=0.0)
    if not (np.isfinite(X).all() and np.isfinite(T).all() and np.isfinite(Lam).all()):
        return out
    if E and (src.min() < 0 or tgt.min() < 0 or src.max() >= S or tgt.max() >= S or (src == tgt).any()):
        return out
    F, _, l, th = evaluate(X, src, tgt, T, Lam, unc, alive, mu)
    out.update(l=l, cost=F)
    if not connected(S, src, tgt, alive).all():
        return dict(out, status=2)
    if th > THETA_MAX:
        return dict(out, status=3)
    if S == 1:
        return dict(out, status=0)
    lam, status, it, small = 0.0, 1, 0, False
    for it in range(1, max_iter + 1):
        H, g, _, _, _ = normal_equations(X, src, tgt, T, Lam, alive, l)
        if it == 1:
            lam = 1e-5 * H.diagonal().max()
        while True:
            delta = cholesky_solve(H + lam * np.eye(len(H)), g)
            out.update(H=H, g=g, delta=delta, lam=lam)
            if delta is None:
                return dict(out, X=X, l=l, cost=F, iterations=it, status=3)
            Xn = X.copy()
            for k in range(1, S):
                Xn[k] = R.apply_step(X[k], delta[6 * (k - 1):6 * k])
            Fn, _, ln, th = evaluate(Xn, src, tgt, T, Lam, unc, alive, mu)
            if th > THETA_MAX:
                return dict(out, X=X, l=l, cost=F, iterations=it, status=3)
            small = np.abs(delta).max() < tol
            if Fn < F:
                X, F, l, lam = Xn, Fn, ln, max(lam / 3.0, LAMBDA_MIN)
                break
            if small:                                          # a fixed point: F cannot fall any more in f64
                break
            lam = 2.0 * lam
            if lam > LAMBDA_MAX:
                return dict(out, X=X, l=l, cost=F, iterations=it, status=3)
        if small:
            status = 0
            break
    return dict(out, X=X, l=l, cost=F, iterations=it, status=status)


def mu_of(Lam, alive, preference, max_dist):
    """Open3D's line-process weight: preference x the mean inlier count of the alive edges x max_dist^2"""
    Lam, alive = np.asarray(Lam, np.float64).reshape(-1, 6, 6), np.asarray(alive).reshape(-1) != 0
    return preference * Lam[alive, 5, 5].mean() * max_dist ** 2 if alive.any() else 0.0


def global_optimization(X, src, tgt, T, Lam, unc, alive=None, preference=2.0, max_dist=0.01, prune=0.25, **kw):
    """Open3D's two passes -> dict(X, kept (E,), l (E,) of pass one, status1, status2, first, second)"""
    E = len(src)
    alive = np.ones(E, bool) if alive is None else np.asarray(alive).reshape(E) != 0
    unc = np.asarray(unc).reshape(E) != 0
    a = optimize(X, src, tgt, T, Lam, unc, alive, mu_of(Lam, alive, preference, max_dist), **kw)
    kept = alive & ~(unc & (a["l"] < prune))
    b = optimize(a["X"], src, tgt, T, Lam, unc, kept, 0.0, **kw)
    return dict(X=b["X"], kept=kept, l=a["l"], status1=a["status"], status2=b["status"], first=a, second=b)


# ---- the information matrix of a registered pair -----------------------------------------------------------------------------------

def information_terms(tgt, idx, d2, max_dist):
    """(inliers, 6, 6): every inlier's G^T G, G = [-[q]x | I], q its target point.  Inlier iff d2 <= f32(max_dist^2) and 0 <= idx < m"""
    tgt = np.asarray(tgt, np.float32).reshape(-1, 3)
    inl = (idx >= 0) & (idx < len(tgt)) & (d2 <= R.maxd2_of(max_dist))
    q = tgt[idx[inl]].astype(np.float64)
    out = np.zeros((len(q), 6, 6))
    for k, p in enumerate(q):
        K = skew(p)
        out[k, :3, :3] = (p @ p) * np.eye(3) - np.outer(p, p)
        out[k, :3, 3:] = K
        out[k, 3:, :3] = K.T
        out[k, 3:, 3:] = np.eye(3)
    return out


def information(src, tgt, pose, max_dist):
    """-> Lambda (6,6), sum |term| (6,6), count, fitness, rmse under `pose`"""
    e = R.evaluate(src, tgt, None, pose, max_dist)
    t = information_terms(tgt, e["idx"], e["d2"], max_dist)
    return t.sum(0), np.abs(t).sum(0), len(t), e["fitness"], e["rmse"]


# ---- the whole pipeline --------------------------------------------------------------------------------------------------------------

def all_pairs(S):
    return [(i, j) for i in range(S) for j in range(i + 1, S)]


def chain_poses(S, edges, T):
    """initial node poses by walking the edges breadth-first from node 0 -> X (S,12), reached (S,) bool.  Edge k = (i, j): target i,
    source j, T[k] takes j's frame to i's"""
    X, seen, queue = np.tile(R.IDENTITY, (S, 1)), np.zeros(S, bool), [0]
    seen[0] = True
    while queue:
        a = queue.pop(0)
        for k, (i, j) in enumerate(edges):
            if i == a and not seen[j]:
                X[j], seen[j] = mul12(X[i], T[k]), True
                queue.append(j)
            elif j == a and not seen[i]:
                X[i], seen[i] = mul12(X[j], inv12(T[k])), True
                queue.append(i)
    return X, seen


def multiway(clouds, pairs=None, max_dists=(0.05, 0.01), min_fitness=0.1, preference=2.0, prune=0.25, **icp):
    """-> dict(poses (S,12), status (S,), chain (S,12) the breadth-first start, edges, T, fitness, info, l, kept, icp_status): every pair
    (i, j), i < j, is registered source j onto target i by consecutive point-metric stages; an edge is dropped for status >= 2 or a
    fitness below min_fitness; edges j = i + 1 are certain"""
    S = len(clouds)
    pairs = all_pairs(S) if pairs is None else [tuple(p) for p in pairs]
    edges, T, fit, info, stats = [], [], [], [], []
    for (i, j) in pairs:
        pose, st = R.IDENTITY.copy(), 1
        for md in max_dists:
            pose, f, _, _, st = R.icp(clouds[j], clouds[i], md, "point", init=pose, **icp)
            if st >= 2:
                break
        stats.append((i, j, st, f))
        if st >= 2 or f < min_fitness:
            continue
        lam, _, _, f, _ = information(clouds[j], clouds[i], pose, max_dists[-1])
        edges.append((i, j)), T.append(pose), fit.append(f), info.append(lam)
    X, seen = chain_poses(S, edges, T)
    node = np.cumsum(seen) - 1                                  # the reached scans, renumbered
    keep = [k for k, (i, j) in enumerate(edges) if seen[i] and seen[j]]
    status = np.where(seen, 0, 2).astype(np.int32)
    poses = X.copy()
    out = dict(chain=X, edges=edges, T=np.array(T).reshape(-1, 12), fitness=np.array(fit), info=np.array(info).reshape(-1, 6, 6),
               icp_status=stats, l=np.zeros(len(edges)), kept=np.zeros(len(edges), bool))
    if keep:
        src, tgt = [node[edges[k][1]] for k in keep], [node[edges[k][0]] for k in keep]
        unc = [edges[k][1] != edges[k][0] + 1 for k in keep]
        g = global_optimization(X[seen], src, tgt, out["T"][keep], out["info"][keep], unc, None, preference, max_dists[-1], prune)
        poses[seen] = g["X"]
        out["l"][keep], out["kept"][keep] = g["l"], g["kept"]
        status[seen] = g["status2"] if g["status2"] >= 2 else 0
        out.update(status1=g["status1"], status2=g["status2"])
    return dict(out, poses=poses, status=status)


# ---- scenes -------------------------------------------------------------------------------------------------------------------------

def random_pose(rs, deg, trans):
    ax = rs.randn(3)
    ax /= np.linalg.norm(ax)
    return R.pose12(R.rodrigues(ax * np.deg2rad(deg) * rs.uniform(0.3, 1.0)), rs.randn(3) * trans)


def random_spd(rs, scale=1.0):
    A = rs.randn(6, 6)
    return scale * (A @ A.T + 6 * np.eye(6))


def synthetic(S, seed=0, edges=None, noise=0.0, outliers=0, start=0.05):
    """A graph with known node poses: X_true (node 0 the identity), edges (all pairs i < j, or `edges` as (src, tgt)) whose transforms
    are the exact relative poses (times a small random motion of `noise` radians / units), a random SPD information matrix each, and a
    start perturbed by `start`.  `outliers`: that many further uncertain edges between non-neighbours, off by 20 degrees.  Edges of
    neighbours (|src - tgt| = 1) are certain.  -> dict(X_true, X0, src, tgt, T, Lam, unc)"""
    rs = np.random.RandomState(100 + seed)
    Xt = np.stack([R.IDENTITY] + [random_pose(rs, 60, 0.5) for _ in range(S - 1)])
    if edges is None:
        edges = [(j, i) for i in range(S) for j in range(i + 1, S)]
    src, tgt = [e[0] for e in edges], [e[1] for e in edges]
    T = []
    for s, t in zip(src, tgt):
        rel = mul12(inv12(Xt[t]), Xt[s])
        if noise:
            rel = mul12(rel, R.pose12(R.rodrigues(rs.randn(3) * noise), rs.randn(3) * noise))
        T.append(rel)
    unc = [abs(s - t) != 1 for s, t in zip(src, tgt)]
    for _ in range(outliers):
        while True:
            s, t = rs.randint(0, S, 2)
            if abs(s - t) > 1:
                break
        ax = rs.randn(3)
        ax /= np.linalg.norm(ax)
        wrong = R.pose12(R.rodrigues(ax * np.deg2rad(20)), rs.randn(3) * 0.1)
        src.append(int(s)), tgt.append(int(t)), T.append(mul12(mul12(inv12(Xt[t]), Xt[s]), wrong)), unc.append(True)
    Lam = np.array([random_spd(rs, 50.0) for _ in src]).reshape(-1, 6, 6)
    X0 = Xt.copy()
    for k in range(1, S):
        X0[k] = R.apply_step(Xt[k], rs.randn(6) * start)
    return dict(X_true=Xt, X0=X0, src=np.array(src, np.int32), tgt=np.array(tgt, np.int32), T=np.array(T).reshape(-1, 12), Lam=Lam,
                unc=np.array(unc, np.int32))


def graph_error(X, Xt):
    """(max || R - Rt ||_F, max |t - tt|) over the nodes"""
    e = [R.pose_error(x, np.asarray(t).reshape(3, 4)[:, :3], np.asarray(t).reshape(3, 4)[:, 3]) for x, t in zip(X, Xt)]
    return max(v[0] for v in e), max(v[1] for v in e)


def _slabs(K):
    X = R.fixture()
    e = np.quantile(X[:, 1], np.linspace(0, 1, K + 1))
    return X, e


def _move(parts, seed0):
    """scans 1.. in their own frames -> clouds, X_true (S,12): the motion that brings scan i back"""
    clouds, Xt = [np.ascontiguousarray(parts[0])], [R.IDENTITY.copy()]
    for i in range(1, len(parts)):
        Rm, t = R.motion(seed0 + i, 4)
        clouds.append(R.moved(parts[i], Rm, t))
        Xt.append(R.pose12(Rm, t))
    return clouds, np.stack(Xt)


def ring_scene():
    """the fixture cut into six slabs along y; scan i holds slabs i and (i + 1) % 6, so only neighbours (and 0 - 5) overlap"""
    X, e = _slabs(6)
    sx = np.clip(np.searchsorted(e, X[:, 1], "right") - 1, 0, 5)
    parts = [X[(sx == i) | (sx == (i + 1) % 6)] for i in range(6)]
    clouds, Xt = _move(parts, 40)
    return dict(clouds=clouds, X_true=Xt, fixture=X)


def chain_scene(K=5):
    """scan i of K holds e[i] <= y <= e[i + 2], e the K + 2 quantile edges of y: a chain whose ends share nothing"""
    X, e = _slabs(K + 1)
    parts = [X[(X[:, 1] >= e[i]) & (X[:, 1] <= e[i + 2])] for i in range(K)]
    clouds, Xt = _move(parts, 40)
    return dict(clouds=clouds, X_true=Xt, fixture=X)
