"""CPU: tests/train_vqdif_ref.py and the case tables of tests/test_train_vqdif_kernels_gpu.py.  Four things are proved here, without a GPU:
the tables reach every launch form (from the mirrors of the launch rules); every bound has teeth (a reference perturbed by a plausible
kernel error - a dropped term, a neighbour's weight, a flipped tap, a wrong coefficient index - exceeds its bound by a wide factor, while
an f32 restatement of the kernel's arithmetic stays inside it); the float64 references agree with torch autograd in float64 at tiny sizes
(so they are not checked against themselves); and the tie defect of the local max-pool backward: on a cloud with exact copies the rule
the kernel used to apply (every point that attains the maximum takes the whole gradient) breaks conservation and gives a wrong parameter
gradient, the contract (one winner, the lowest index) gives torch autograd's."""
import itertools
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import train_vqdif_ref as R             # noqa: E402
import test_train_vqdif_kernels_gpu as T   # noqa: E402  (plain data: the case tables)

F32, U, f64 = np.float32, R.U, R.f64
TEETH = 20.0        # a perturbed reference must miss its bound by at least this factor


def _rs(seed):
    return np.random.RandomState(seed)


def _t(a):
    return torch.from_numpy(np.asarray(a, np.float64))


# ---------------------------------------------------------------------------------------------------- the tables reach every form
def test_elementwise_tables_cover_one_block_its_edges_and_many_blocks():
    assert all(n % 4 == 0 for n in T.RELU_N) and {n // 4 for n in T.RELU_N} >= {1, 255, 256, 257} and max(T.RELU_N) // 4 > 65536
    assert {1, 255, 256, 257} <= set(T.LINCOMB_N) and max(T.LINCOMB_N) > 16 * 256
    assert T.lincomb_ab("sub", 7) == (1.0, -1.0) and T.lincomb_ab("commit", 8) == (1.0, 2 * T.QUANT_BETA / 8) and "no_y" in T.LINCOMB_AB
    assert T.AFFINE_CASES == [(1, 1, 4), (2, 5, 12), (3, 33, 64), (2, 64, 768)]


def test_chan_dot_stats_table_reaches_every_rpp_class_and_empty_slices():
    assert [R.chan_rpp(C)[1:] for C in T.CDS_C] == [(256, 0), (85, 1), (21, 4), (16, 0), (1, 64), (1, 0)]      # (rpp, idle threads)
    for C in T.CDS_C:
        rpp = R.chan_rpp(C)[1]
        mine = [c for c in T.CDS_CASES if c[2] == C]
        Vs = {c[1] for c in mine}
        assert {1, 3, rpp, rpp + 1, 4097} <= Vs and (rpp == 1 or rpp - 1 in Vs)
        assert {c[3] for c in mine} >= {1, 4, 16} and {c[0] for c in mine} >= {1, 3}
        empties = [(c, s) for c in mine for s in range(c[3]) if R.stats_slice(c[1], s, c[3])[0] == R.stats_slice(c[1], s, c[3])[1]]
        assert empties and any(c[3] > c[1] for c in mine)
        assert any(R.gn_splits(c[1]) == c[3] == 16 for c in mine)                                               # the trainer's own S at V = 4097
        for B, V, _, S in mine:                                                                                # slices tile [0, V) without gaps
            assert [R.stats_slice(V, s, S)[0] for s in range(S)] + [V] == [0] + [R.stats_slice(V, s, S)[1] for s in range(S)]
    assert [R.gn_splits(V) for V in T.GN_SPLIT_V] == [1, 1, 4, 4, 16, 16, 16, 64, 64]


def test_pool_tables_hold_every_tie_pattern():
    names, pat = R.pool_patterns()
    assert len(set(names)) == len(names) == 8 + 28 + 3 + 2 + 3
    for n, w in zip(names, pat):
        assert np.all(w * 8 == np.round(w * 8))                                      # the 2^-3 grid: window sums are exact
        top = np.flatnonzero(w == w.max())
        if n.startswith("unique"):
            assert list(top) == [int(n[6])]
        elif n.startswith("pair"):
            assert list(top) == [int(n[4]), int(n[5])]
        elif n.startswith("equal") or n == "neg_equal":
            assert len(top) == 8
        elif n.startswith("zeros"):
            assert len(top) == 2 and sorted(np.signbit(w[top])) == [False, True] and (np.delete(w, top) < 0).all()
            assert np.signbit(w[top[0]]) == (n == "zeros-+")
        if n.startswith("neg"):
            assert (w < 0).all()
    seen = set()
    for B, ext, C in T.POOL_CASES:
        x, idx = R.pool_input(B, *ext, C, T.pool_shift(B, ext, C))
        assert x.shape == (B, 2 * ext[0], 2 * ext[1], 2 * ext[2], C) and C % 4 == 0
        assert np.array_equal(R._windows(x).reshape(-1, 8), pat[idx])
        seen |= set(idx.tolist())
        y = R.maxpool2_ref(x)
        dx = R.maxpool2_bwd_ref(x, y, np.ones_like(y))
        assert (R._windows(dx).sum(-1) == 1).all()                                    # exactly one child per window
        first = np.argmax(R._windows(x) == y[..., None], -1)
        assert np.array_equal(np.argmax(R._windows(dx), -1), first)                   # and it is the first maximum in z-major order
    assert seen == set(range(len(pat)))
    assert {e for _, e, _ in T.POOL_CASES} == {(1, 2, 3), (3, 1, 2), (4, 4, 4)} and {c for _, _, c in T.POOL_CASES} == {4, 12, 64}
    assert max(B * np.prod(e) * 8 * C for B, e, C in T.POOL_CASES) > 256                # more than one block


def test_cell_coordinates_turn_every_boundary():
    for G in T.CELLS_G:
        v = np.sort(R.cell_boundary_coords(G))
        cloud = np.stack([v, np.zeros_like(v), np.zeros_like(v)], -1)
        cx = R.cells_ref(cloud, G)[0] % G
        assert set(cx.tolist()) == set(range(G))
        d = np.flatnonzero(np.diff(cx) > 0)
        assert len(d) == G - 1                                                        # every boundary is crossed ...
        assert all(np.nextafter(v[i], F32(np.inf)) == v[i + 1] for i in d)            # ... between two ADJACENT floats
        u = R.normalize_f32(v * F32(0.5))
        assert (u == 0).sum() > 2 and (u == R.NORM_HI).sum() > 2                      # both clamps of sfmi_normalize
        assert {1.0, -1.0, 0.0} <= set(v.tolist()) and v.min() < -1.101 and v.max() > 1.101


def _tie_census(cs):
    net, cell, ncell = cs["net"], cs["cell"], cs["ncell"]
    keys, _ = R.cell_max_ref(net, cell, ncell)
    k = R.f2key(net)
    census = dict(copies=0, distinct=0, three=0, three_distinct=0, empty=0, single=0, negative=0, signed_zero=0, late_winner=0)
    for b in range(net.shape[0]):
        n = np.bincount(cell[b], minlength=ncell)
        census["empty"] += int((n == 0).sum())
        census["single"] += int((n == 1).sum())
        for c_ in range(ncell):
            pts = np.flatnonzero(cell[b] == c_)
            if len(pts) and (net[b, pts] < 0).all():
                census["negative"] += 1
            for ch in range(net.shape[2]):
                att = pts[k[b, pts, ch] == keys[b, c_, ch]]
                if len(att) < 2:
                    if len(pts) and np.any(net[b, pts, ch] == 0) and len({bool(s) for s in np.signbit(net[b, pts, ch][net[b, pts, ch] == 0])}) == 2:
                        census["signed_zero"] += 1
                    continue
                rows = {net[b, p].tobytes() for p in att}
                census["copies"] += len(rows) < len(att)
                census["distinct"] += len(rows) > 1
                census["three"] += len(att) >= 3
                census["three_distinct"] += len(rows) >= 3
                census["late_winner"] += int(att.min() > pts.min())
    return census


def test_cell_pool_cases_hold_every_tie_pattern():
    for C in T.CELL_POOL_C:
        for seed in T.CELL_POOL_SEEDS:
            cs = R.cell_pool_case(C, seed)
            n = _tie_census(cs)
            assert all(v > 0 for v in n.values()), n
            assert n["empty"] == 2 and n["single"] == 2
            assert cs["cell"].min() >= 0 and cs["cell"].max() < cs["ncell"] == T.NCELL
    assert T.SCATTER_FORMS == [("one_cell", 300), ("one_each", 8)] and T.SCATTER_SCALES == (1.0, 1e-4, 1e-8)


def test_trilinear_table_holds_node_border_outside_and_face_points():
    assert {g for g, _, _ in T.TRI_CASES} == {2, 3, 64} and {c for _, c, _ in T.TRI_CASES} == {4, 32} and {n for _, _, n in T.TRI_CASES} == {1, 255, 257}
    for G, C, N in T.TRI_CASES:
        xyz = R.tri_points(G, N, G + C + N)
        assert xyz.shape == (2, N, 3)
        if N == 1:
            continue
        x = xyz.reshape(-1)
        i0, i1, w0, w1, ix = R.tri_axis(x, G)
        assert (np.abs(x) == 1).any() and (np.abs(x) > F32(1.101)).any()                                   # borders, outside (clamped)
        assert (w1 == 0).any() and (G == 2 or ((w1 == 0) & (np.abs(x) < 1.1)).any())                       # on a lattice node (G = 2: only node 0 is reachable)
        assert ((w1 > 0) & (w1 < 1e-4)).any() and ((w0 > 0) & (w0 < 1e-4)).any()                           # one ulp inside a cell face, both sides
        assert i0.min() == 0 and i1.max() == G - 1 and ((i0 == i1) & (ix == G - 1)).any() == (ix == G - 1).any()
        assert ((w0 + w1).astype(np.float64) <= 1 + 2 * U).all() and i1.max() < G
        assert N * C > 256 or N == 255 and C == 4                                                         # more than one block (but for one case)


def test_quantizer_and_loss_tables():
    assert {0.0, 1e-8, 1.0, 20.0, 88.0, 89.0, 104.0, 1e4} == {abs(x) for x in T.BCE_LOGITS} and all(-x in T.BCE_LOGITS for x in T.BCE_LOGITS)
    assert T.BCE_LABELS == (0.0, 1.0, 0.25) and T.BCE_N == (1, 255, 256, 257)
    for n in T.BCE_N[1:]:
        seen = set()
        for off in (0, 17):
            x, y = T.bce_inputs(n, off)
            seen |= set(zip(x.tolist(), y.tolist()))
        assert len(seen) == len(T.BCE_LOGITS) * len(T.BCE_LABELS)
    assert len({T.bce_inputs(1, o)[0][0].item() + 1j * T.bce_inputs(1, o)[1][0].item() for o in range(45)}) == 45
    assert set(T.VQ_STATS_CASES) == set(itertools.product((1, 300), (4, 256), (1, 5, 4096)))
    assert set(T.VQ_EMA_CASES) == set(itertools.product((1, 1000, 1024, 1025, 4096), (4, 256)))
    assert {-(-K // 1024) for K, _ in T.VQ_EMA_CASES} == {1, 2, 4}                                           # terms per thread of the n tree


def test_wgrad_table_reaches_every_tile_tap_and_slice_form():
    rows_mod, geoms = set(), set()
    for case in T.WG_CASES:
        name, B, Di, Hi, Wi, Cin, Cout, KS, st, pad, ldy, ldx, form = case
        rows = R.wgrad_rows(B, Di, Hi, Wi, KS, st, pad)
        ns = T.wg_nsplits(case)
        assert ns[:2] == [1, 3] and R.wgrad_empty_slices(rows, ns[2]) > 0 and R.wgrad_empty_slices(rows, 1) == 0
        assert all(R.rows_per_split(rows, n) % 16 == 0 and R.rows_per_split(rows, n) * n >= rows for n in ns)
        assert ldy >= Cout and ldx >= Cin
        rows_mod.add(rows % 16)
        geoms.add((KS, st, pad))
    assert geoms == {(1, 1, 0), (3, 1, 1), (2, 2, 0), (3, 1, 0)}
    assert len(rows_mod) > 3 and 0 in rows_mod                                                              # rows not a multiple of the 16-row stage
    lin = [c for c in T.WG_CASES if c[0].startswith("lin")]
    assert {c[4] for c in lin} == {1, 15, 16, 17, 700}
    assert any(c[5:7] == (3, 64) and c[11] == 16 for c in lin)                                              # fc_pos / fc_p: ldx 16 over 3 real columns
    assert any(c[12] == "fc_out" for c in lin) and any(c[6] == 1 and c[10] > 1 for c in lin)                 # ldy > Cout
    chans = {(c[5], c[6]) for c in T.WG_CASES}
    assert any(ci % 64 and ci < 64 for ci, _ in chans) and any(co % 64 and co > 64 for _, co in chans)      # partial ci / co tiles
    assert any(ci > 64 and ci % 64 for ci, _ in chans) and any(ci >= 128 for ci, _ in chans) and (768, 256) in chans   # several tiles
    assert {(32, 64), (64, 32), (128, 128)} <= chans
    for g in geoms:                                                                                         # every geometry on both extents
        assert {tuple(c[2:5]) for c in T.WG_CASES if c[7:10] == g and not c[0].startswith("lin")} == {(3, 4, 5), (4, 4, 4)}, g
    assert any(c[7:10] == (2, 2, 0) and (c[2] % 2 or c[4] % 2) for c in T.WG_CASES)                          # k2 s2 with an unread last plane / column
    # the slice counts VQDIFTrainer._wgrad_into picks for UNet3D's real layers appear in the table
    from shapeformer_amd import weights as W
    real = set()
    for res in (16, 32):
        for k, shp in W.vqdif_spec(res).items():
            if k.startswith("decoder.unet3d.") and k.endswith("conv.weight"):
                lvl = int(k.split(".")[3]) if ".encoders." in k else (1 - int(k.split(".")[3]) if ".decoders." in k else 0)
                D = res >> lvl
                real.add(R.wgrad_nsplit(D ** 3, shp[1], shp[0], shp[2]))
    assert real == set(T.WG_UNET_NSPLITS), sorted(real)
    k3 = [c for c in T.WG_CASES if c[7:10] == (3, 1, 1) and c[5] * c[6] <= 64 * 32]
    assert k3 and all(set(T.WG_UNET_NSPLITS) <= set(T.wg_nsplits(c)) for c in k3)


def test_redrawn_cloud_has_copies_and_no_tie_between_distinct_points():
    """the step test's cloud: about a third of the rows are copies, and in no pooled channel of any stage do two DISTINCT points tie - so
    the oracle's even split and the single arg-max give the same parameter gradients"""
    from oracle import vqdif_oracle as VO
    from shapeformer_amd import weights as W
    G = np.load(os.path.join(HERE, "golden", "vqdif_train.npz"))
    X = T.redrawn_cloud(G["Xbd"])
    Tn = X.shape[1]
    _, inv = np.unique(X[0], axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    assert 0.3 < 1 - (inv.max() + 1) / Tn < 0.42
    with torch.no_grad():
        _, cell, _, stages = VO.encoder_points(VO.to_torch_sd(W.make_state_dict(W.vqdif_spec(16))), torch.from_numpy(X) / 2, return_stages=True)
    cell = cell.numpy().astype(np.int32)
    cells, cinv = np.unique(cell[0], return_inverse=True)
    tied_copies = 0
    for s in stages[:4]:                                       # the four pooled stages
        net = s.numpy().astype(F32)[:, :, :]
        keys, _ = R.cell_max_ref(net, cinv[None].astype(np.int32), len(cells))
        att = R.f2key(net)[0] == keys[0][cinv]
        lo, hi = np.full(keys.shape[1:], Tn), np.full(keys.shape[1:], -1)
        for ch in range(net.shape[2]):
            a = att[:, ch]
            np.minimum.at(lo[:, ch], cinv[a], inv[a])
            np.maximum.at(hi[:, ch], cinv[a], inv[a])
        assert (lo == hi).all(), "two distinct points tie for a cell's maximum"
        n_att = np.zeros(keys.shape[1:], np.int64)
        for ch in range(net.shape[2]):
            np.add.at(n_att[:, ch], cinv[att[:, ch]], 1)
        tied_copies += int((n_att > 1).sum())
    assert tied_copies > 1000                                   # and copies DO tie, in every channel they win


def test_mirrors_at_known_values():
    assert R.rows_per_split(700, 3) == 240 and R.stats_slice(4097, 15, 16) == (3840, 4097) and R.wgrad_nsplit(4096, 128, 128, 3) == 10
    assert R.wgrad_rows(2, 3, 4, 5, 2, 2, 0) == 2 * 1 * 2 * 2 and R.chan_rpp(12) == (3, 85, 1)


# ---------------------------------------------------------------------------------------------------- the bounds have teeth
def _ratio(got, ref, bnd):
    return R.ratio(got, ref, bnd)


def test_elementwise_and_statistics_bounds_have_teeth():
    rs = _rs(1)
    x, y = rs.randn(500).astype(F32), rs.randn(500).astype(F32)
    for a, b in ((1.0, -1.0), (0.37, -1.9), (1.0, 2e-3 / 500)):
        ref, bnd = R.lincomb_ref(a, x, b, y)
        sep = (F32(a) * x).astype(F32) + (F32(b) * y).astype(F32)                                  # the separate form; fused: f64 then one rounding
        assert _ratio(sep, ref, bnd) <= 1 and _ratio(ref.astype(F32), ref, bnd) <= 1
        if abs(b) > 1e-3:       # the commit form's b y is ~1e-6 of a x: a wrong y there is within a few roundings of x and cannot be told apart
            assert _ratio(R.lincomb_ref(a, x, b, np.roll(y, 1))[0], ref, bnd) > TEETH              # a neighbour's y
            assert _ratio(R.lincomb_ref(a, x, 0.0, y)[0], ref, bnd) > TEETH                         # the dropped term
    u, v = rs.randn(2, 5, 12).astype(F32), rs.randn(2, 5, 12).astype(F32)
    A, Bc, Cc = (rs.randn(2, 12).astype(F32) for _ in range(3))
    ref, bnd = R.affine2_ref(u, v, A, Bc, Cc)
    sep = ((A[:, None] * u).astype(F32) + (Bc[:, None] * v).astype(F32)).astype(F32) + Cc[:, None]
    assert _ratio(sep, ref, bnd) <= 1
    assert _ratio(R.affine2_ref(u, v, A[::-1], Bc, Cc)[0], ref, bnd) > TEETH                        # the other sample's coefficient
    assert _ratio(R.affine2_ref(u, v, A, np.roll(Bc, 1, 1), Cc)[0], ref, bnd) > TEETH               # the neighbouring channel's
    ref, bnd = R.affine_ref(u, A, Cc)
    assert _ratio((A[:, None] * u).astype(F32) + Cc[:, None], ref, bnd) <= 1 and _ratio(R.affine_ref(u, A[::-1], Cc)[0], ref, bnd) > TEETH
    dy, xx = rs.randn(2, 300, 12).astype(F32), rs.randn(2, 300, 12).astype(F32)
    ref, bnd = R.chan_dot_stats_ref(dy, xx, 4)
    plain = np.stack([np.stack([np.stack([dy[:, a:b].astype(np.float64).sum(1), (dy[:, a:b].astype(np.float64) * xx[:, a:b]).sum(1)], -1)
                                for a, b in (R.stats_slice(300, s, 4) for s in range(4))], 1)])[0]
    assert (np.abs(plain - ref.astype(np.float64)) <= bnd).all()
    d2 = dy.copy(); d2[0, 7, 3] = 0                                                                 # one dropped voxel
    assert (np.abs(R.chan_dot_stats_ref(d2, xx, 4)[0] - ref).astype(np.float64) / np.maximum(bnd, 1e-300)).max() > 1e6
    assert not ref[:, :, :, :].astype(np.float64)[np.broadcast_to(bnd == 0, ref.shape)].any()


def test_fixed_point_and_pooling_bounds_have_teeth():
    rs = _rs(2)
    for scale in T.SCATTER_SCALES:
        src = (rs.randn(2, 300, 4) * scale).astype(F32)
        cell = np.full((2, 300), 5, np.int32)
        acc, cnt, s, sa = R.cell_scatter_ref(src, cell, 8)
        bnd = R.fix_bound(cnt[..., None], s)
        assert _ratio(R.fix_to_float(acc), s, bnd) <= 1
        assert (bnd[:, 5] < 4e-8 + 2 * U * np.abs(s[:, 5])).all()
        acc2 = R.cell_scatter_ref(src[:, 1:], cell[:, 1:], 8)[0]                                    # one dropped point
        if scale >= 1e-4:
            assert _ratio(R.fix_to_float(acc2), s, bnd) > TEETH
        m, bm = R.cell_mean_ref(s, cnt)
        got = (acc.astype(np.float64) / R.FIX / np.maximum(cnt, 1)[..., None]).astype(F32)
        assert _ratio(got, m, bm) <= 1
        if scale >= 1e-4:
            assert _ratio((acc.astype(np.float64) / R.FIX / (np.maximum(cnt, 1)[..., None] + 1)).astype(F32), m, bm) > TEETH
        dg = (rs.randn(2, 8, 4) * scale).astype(F32)
        ref, bb = R.cell_mean_bwd_ref(dg, cnt, cell)
        assert _ratio((dg[:, 5][:, None] / cnt[:, 5].astype(F32)[:, None, None]).astype(F32), ref, bb) <= 1
        assert _ratio(ref * (1 + 4 * U), ref, bb) > 2


def _tri_f32(xyz, grid, G):
    """the forward kernel's arithmetic restated: f32 weights as tri_axis forms them, eight fused multiply-adds"""
    B, N, _ = xyz.shape
    ax = [R.tri_axis(xyz[..., a], G) for a in range(3)]
    s = np.zeros((B, N, grid.shape[-1]), F32)
    for corner in range(8):
        sel = (corner & 1, (corner >> 1) & 1, corner >> 2)
        i = [ax[a][1] if sel[a] else ax[a][0] for a in range(3)]
        w = [ax[a][3] if sel[a] else ax[a][2] for a in range(3)]
        wt = ((w[0] * w[1]).astype(F32) * w[2]).astype(F32)
        idx = (i[2] * G + i[1]) * G + i[0]
        g = np.stack([grid[b][idx[b]] for b in range(B)])
        s = (g.astype(np.float64) * wt[..., None].astype(np.float64) + s.astype(np.float64)).astype(F32)
    return s


def test_trilinear_bounds_have_teeth():
    for G in (2, 3, 64):
        rs = _rs(G)
        xyz = R.tri_points(G, 257, G)
        grid = rs.randn(2, G ** 3, 4).astype(F32)
        ref, bnd = R.trilinear_ref(xyz, grid, G)
        assert _ratio(_tri_f32(xyz, grid, G), ref, bnd) <= 1
        flip = xyz.copy(); flip[..., 0] = -flip[..., 0]                                             # the neighbour's weight: w0 <-> w1 on x
        assert _ratio(_tri_f32(flip, grid, G), ref, bnd) > TEETH
        assert _ratio(_tri_f32(xyz[..., [1, 0, 2]], grid, G), ref, bnd) > TEETH                     # x and y swapped
        dout = rs.randn(2, 257, 4).astype(F32)
        s, b_acc, b_f = R.trilinear_bwd_ref(xyz, dout, G)
        idx, w = R.tri_corners(xyz, G)
        acc = np.zeros(s.shape, np.int64)
        ax = [R.tri_axis(xyz[..., a], G) for a in range(3)]
        for corner in range(8):
            sel = (corner & 1, (corner >> 1) & 1, corner >> 2)
            wq = [ax[a][3] if sel[a] else ax[a][2] for a in range(3)]
            wt = ((wq[0] * wq[1]).astype(F32) * wq[2]).astype(F32)
            for b in range(2):
                np.add.at(acc[b], idx[b, :, corner], R.to_fix((wt[b][:, None] * dout[b]).astype(F32)))
        assert _ratio(acc.astype(np.float64) / R.FIX, s, b_acc) <= 1 and _ratio(R.fix_to_float(acc), s, b_f) <= 1
        assert _ratio(R.trilinear_bwd_ref(xyz, np.roll(dout, 1, 1), G)[0], s, b_acc) > TEETH        # a neighbour's gradient
        assert _ratio(R.trilinear_bwd_ref(xyz[:, 1:], dout[:, 1:], G)[0], s, b_acc) > TEETH         # a dropped point
        assert np.abs(s.sum(1) - dout.astype(np.float64).sum(1)).max() < 1e-12                      # the weights of a point sum to one


def test_loss_and_quantizer_bounds_have_teeth():
    x, y = T.bce_inputs(45, 0)
    loss, bl, d, bd = R.bce_ref(x, y, 1 / 45)
    assert np.isfinite(loss).all() and np.isfinite(d).all()
    with np.errstate(over="ignore"):
        f_loss = (np.maximum(x, 0) - (x * y).astype(F32)).astype(F32) + np.log1p(np.exp(-np.abs(x)).astype(F32)).astype(F32)
        f_d = ((F32(1) / (F32(1) + np.exp(-x).astype(F32))).astype(F32) - y).astype(F32) * F32(1 / 45)
    assert _ratio(f_loss, loss, bl) <= 1 and _ratio(f_d, d, bd) <= 1
    assert _ratio(np.maximum(x, 0) - x * y, loss, bl) > TEETH                                       # log1p term dropped
    assert _ratio(loss * (1 + 40 * U), loss, bl) > 2 and _ratio(d + 40 * U / 45, d, bd) > 2
    assert _ratio(R.bce_ref(x, 1 - y, 1 / 45)[2], d, bd) > TEETH
    for K, D in ((5, 4), (1025, 4)):
        rs = _rs(K)
        N, z = (rs.rand(K) * 5 + 0.01).astype(F32), rs.randn(K, D).astype(F32)
        c = rs.randint(0, 6, size=K).astype(F32)
        s = (rs.randn(K, D) * c[:, None]).astype(F32)
        ref = R.vq_ema_ref(N, z, c, s, T.VQ_GAMMA, T.VQ_EPS)
        g, og, eps = F32(T.VQ_GAMMA), F32(1) - F32(T.VQ_GAMMA), F32(T.VQ_EPS)
        N1 = ((N * g).astype(F32) + (og * c).astype(F32)).astype(F32)
        z1 = ((z * g).astype(F32) + (og * s).astype(F32)).astype(F32)
        n = F32(0)
        for v in N1:
            n = F32(n + v)                                                                         # a serial f32 sum: deeper than the kernel's tree
        wgt = (((N1 + eps).astype(F32) / F32(n + F32(F32(K) * eps))).astype(F32) * n).astype(F32)
        emb = (z1 / wgt[:, None]).astype(F32)
        if K <= 1024:
            assert _ratio(N1, *ref["N"]) <= 1 and _ratio(z1, *ref["z"]) <= 1 and _ratio(emb, *ref["emb"]) <= 1
        bad = R.vq_ema_ref(N, z, np.roll(c, 1), s, T.VQ_GAMMA, T.VQ_EPS)
        assert _ratio(bad["N"][0], *ref["N"]) > TEETH and _ratio(bad["emb"][0], *ref["emb"]) > TEETH
        assert _ratio(ref["z"][0] / (f64(N)[:, None] + 1e-7), *ref["emb"]) > TEETH                 # the weight from N before its update


def test_wgrad_bound_has_teeth():
    rs = _rs(3)
    B, ext, Cin, Cout = 2, (3, 4, 5), 8, 12
    for KS, st, pad in ((3, 1, 1), (2, 2, 0), (1, 1, 0), (3, 1, 0)):
        e = ext
        rows = R.wgrad_rows(B, *e, KS, st, pad)
        dy, x = rs.randn(rows, Cout).astype(F32), rs.randn(B * int(np.prod(e)), Cin).astype(F32)
        dW, sa = R.wgrad_ref(dy, x, B, *e, Cin, Cout, KS, st, pad)
        for ns in (1, 3):
            bnd = R.wgrad_bound(sa, rows, ns)
            assert _ratio(dW.astype(F32), dW, bnd) <= 1
            if KS > 1:
                assert _ratio(dW[::-1], dW, bnd) > TEETH                                             # flipped taps
            d2 = dy.copy(); d2[rows // 2] = 0                                                        # a dropped row
            assert _ratio(R.wgrad_ref(d2, x, B, *e, Cin, Cout, KS, st, pad)[0], dW, bnd) > TEETH
            assert _ratio(dW * (1 + 1e-3), dW, bnd) > TEETH


# ---------------------------------------------------------------------------------------------------- references against torch autograd
def test_pool_and_resampling_references_match_torch():
    rs = _rs(4)
    for B, ext, C in ((1, (1, 2, 3), 4), (2, (2, 2, 2), 8)):
        x, _ = R.pool_input(B, *ext, C, 5)
        xt = _t(x).permute(0, 4, 1, 2, 3).requires_grad_(True)
        yt = F.max_pool3d(xt, 2)
        dy = rs.randn(*yt.shape).astype(F32)
        yt.backward(_t(dy))
        y = R.maxpool2_ref(x)
        assert np.array_equal(y, yt.detach().permute(0, 2, 3, 4, 1).numpy())
        ours = R.maxpool2_bwd_ref(x, y, dy.transpose(0, 2, 3, 4, 1))
        assert np.array_equal(ours.astype(np.float64), xt.grad.permute(0, 2, 3, 4, 1).numpy())        # ATen: the first maximum of a window
        low, skip = rs.randn(B, *ext, C), rs.randn(B, *(2 * e for e in ext), 4)
        lt, st_ = _t(low).permute(0, 4, 1, 2, 3).requires_grad_(True), _t(skip).permute(0, 4, 1, 2, 3).requires_grad_(True)
        ut = torch.cat([st_, F.interpolate(lt, scale_factor=2, mode="nearest")], 1)
        assert np.array_equal(R.upcat_ref(skip, low), ut.detach().permute(0, 2, 3, 4, 1).numpy())
        assert np.array_equal(R.upsample2_ref(low), ut.detach().permute(0, 2, 3, 4, 1).numpy()[..., 4:])
        d = rs.randn(*ut.shape)
        ut.backward(_t(d))
        assert np.abs(R.sumpool2_ref(d.transpose(0, 2, 3, 4, 1), 4, C) - lt.grad.permute(0, 2, 3, 4, 1).numpy()).max() < 1e-12


def test_cell_references_match_torch_scatter():
    from oracle import vqdif_oracle as VO
    rs = _rs(5)
    cloud = (rs.rand(2, 400, 3) * 2.3 - 1.15).astype(F32)
    cell, half = R.cells_ref(cloud, 64)
    ct = torch.from_numpy(cloud)
    assert np.array_equal(cell, VO.cell_index(VO.normalize_3d(ct / 2), 64).numpy()) and np.array_equal(half, (ct / 2).numpy())
    cell8 = R.cells_ref(cloud, 2)[0]
    net = rs.randn(2, 400, 4).astype(F32)
    keys, pooled = R.cell_max_ref(net, cell8, 8)
    nt = _t(net).requires_grad_(True)
    pt = VO.local_max_pool(nt, torch.from_numpy(cell8.astype(np.int64)), 8)
    assert np.array_equal(pooled.astype(np.float64), pt.detach().numpy())
    dp = rs.randn(2, 400, 4).astype(F32)
    pt.backward(_t(dp))
    acc, cnt, s, sa = R.cell_scatter_ref(dp, cell8, 8)
    dn = R.cell_max_bwd_ref(net, keys, acc, cell8)                                                  # no ties here: one arg-max per cell
    assert np.abs(dn - nt.grad.numpy()).max() <= (R.fix_bound(cnt[..., None], s)).max()
    c = rs.randn(2, 400, 4).astype(F32)
    ctt = _t(c).requires_grad_(True)
    idx = torch.from_numpy(cell8.astype(np.int64))[:, :, None].expand(2, 400, 4)
    sm = torch.zeros(2, 8, 4, dtype=torch.float64).scatter_add(1, idx, ctt)
    nn_ = torch.zeros(2, 8, 4, dtype=torch.float64).scatter_add(1, idx, torch.ones_like(ctt))
    mt = sm / nn_.clamp(min=1)
    _, cnt, s, _ = R.cell_scatter_ref(c, cell8, 8)
    m, _ = R.cell_mean_ref(s, cnt)
    assert np.abs(m - mt.detach().numpy()).max() < 1e-12
    dg = rs.randn(2, 8, 4).astype(F32)
    mt.backward(_t(dg))
    assert np.abs(R.cell_mean_bwd_ref(dg, cnt, cell8)[0] - ctt.grad.numpy()).max() < 1e-12


def test_trilinear_reference_matches_grid_sample():
    for G in (2, 3, 5):
        rs = _rs(G)
        xyz = R.tri_points(G, 64, G)
        grid = rs.randn(2, G ** 3, 4).astype(F32)
        ix = np.stack([R.tri_axis(xyz[..., a], G)[4] for a in range(3)], -1).astype(np.float64)       # the f32 lattice coordinate, (x, y, z)
        gt = _t(grid).view(2, G, G, G, 4).permute(0, 4, 1, 2, 3).requires_grad_(True)
        out = F.grid_sample(gt, _t(2 * ix / (G - 1) - 1).view(2, 64, 1, 1, 3), mode="bilinear", padding_mode="border", align_corners=True)
        out = out[:, :, :, 0, 0].permute(0, 2, 1)
        ref, _ = R.trilinear_ref(xyz, grid, G)
        assert np.abs(ref - out.detach().numpy()).max() < 1e-12
        d = rs.randn(2, 64, 4).astype(F32)
        out.backward(_t(d))
        s, _, _ = R.trilinear_bwd_ref(xyz, d, G)
        assert np.abs(s - gt.grad.permute(0, 2, 3, 4, 1).reshape(2, G ** 3, 4).numpy()).max() < 1e-12


def test_loss_quantizer_and_wgrad_references_match_torch():
    from oracle import vqdif_train_oracle as TO
    x, y = T.bce_inputs(45, 0)
    xt = _t(x).requires_grad_(True)
    lt = F.binary_cross_entropy_with_logits(xt, _t(y), reduction="none")
    lt.sum().backward()
    loss, _, d, _ = R.bce_ref(x, y, 1.0)
    assert np.abs(loss - lt.detach().numpy()).max() <= 1e-12 * np.abs(loss).max() and np.abs(d - xt.grad.numpy()).max() < 1e-15
    rs = _rs(6)
    K, D = 7, 4
    N, z = (rs.rand(K) + 0.1).astype(F32), rs.randn(K, D).astype(F32)
    xr, idx = rs.randn(20, D).astype(F32), rs.randint(0, K - 1, size=20)
    sums, cnt = R.vq_stats_ref(xr, idx.astype(np.int32), K)
    oh = F.one_hot(torch.from_numpy(idx), K).double()
    assert np.array_equal(cnt, oh.sum(0).numpy().astype(np.int32)) and cnt[K - 1] == 0 and not sums[K - 1].any()
    assert np.abs(sums / R.FIX - (oh.t() @ _t(xr)).numpy()).max() <= 20 * 2.0 ** -33
    sf = R.fix_to_float(sums)
    g32, e32 = float(F32(T.VQ_GAMMA)), float(F32(T.VQ_EPS))
    sd = {"quantizer.embedding.weight": torch.zeros(K, D, dtype=torch.float64), "quantizer.N": _t(N), "quantizer.z_avg": _t(z)}
    onehot_x = _t(sf)     # ema_update forms x^T onehot itself: feed rows that reproduce the converted sums (one row per code)
    Nn, zn, en = TO.ema_update(sd, onehot_x, torch.arange(K), gamma=g32, eps=e32)
    ref = R.vq_ema_ref(N, z, np.ones(K, F32), sf, T.VQ_GAMMA, T.VQ_EPS)
    for a, b in ((ref["N"][0], Nn), (ref["z"][0], zn), (ref["emb"][0], en)):
        assert np.abs(a - b.numpy()).max() <= 1e-13 * max(1.0, np.abs(a).max())
    for KS, st, pad, ext in ((3, 1, 1, (3, 4, 5)), (2, 2, 0, (2, 4, 6)), (2, 2, 0, (3, 4, 5)), (1, 1, 0, (3, 4, 5)), (3, 1, 0, (3, 4, 5))):
        B, Cin, Cout = 2, 3, 5
        rows = R.wgrad_rows(B, *ext, KS, st, pad)
        xx, dy = rs.randn(B * int(np.prod(ext)), Cin + 2).astype(F32), rs.randn(rows, Cout + 1).astype(F32)
        xt = _t(xx[:, :Cin]).view(B, *ext, Cin).permute(0, 4, 1, 2, 3)
        w = torch.zeros(Cout, Cin, KS, KS, KS, dtype=torch.float64, requires_grad=True)
        yt = F.conv3d(xt, w, None, stride=st, padding=pad)
        yt.backward(_t(dy[:, :Cout]).view(*yt.permute(0, 2, 3, 4, 1).shape).permute(0, 4, 1, 2, 3))
        dW, sa = R.wgrad_ref(dy, xx, B, *ext, Cin, Cout, KS, st, pad)
        assert np.abs(dW - w.grad.reshape(Cout, Cin, KS ** 3).permute(2, 0, 1).numpy()).max() < 1e-12 and (sa >= np.abs(dW) - 1e-12).all()
    dyv, xv = rs.randn(2, 50, 8).astype(F32), rs.randn(2, 50, 8).astype(F32)
    ref, _ = R.chan_dot_stats_ref(dyv, xv, 1)
    assert np.abs(ref[:, 0, :, 0].astype(np.float64) - _t(dyv).sum(1).numpy()).max() < 1e-12
    assert np.abs(ref[:, 0, :, 1].astype(np.float64) - (_t(dyv) * _t(xv)).sum(1).numpy()).max() < 1e-12


# ---------------------------------------------------------------------------------------------------- the tie defect, on the CPU
def test_old_tie_rule_breaks_conservation_and_the_contract_gives_autograds_parameter_gradient():
    """A one-layer point encoder net = p W^T with a local max pool, on a cloud in which a third of the rows are exact copies (the data
    loader's np.random.choice(..., replace=True)).  Copies have identical features, so torch's amax backward (an even split among the tied
    points), scatter_max's single arg-max and the contract (the lowest-indexed attaining point) all give the same dL/dW.  The rule the
    kernel applied before - every attaining point takes the whole gradient - multiplies a cell's gradient by its number of tied points."""
    rs = _rs(7)
    Tn, C, ncell = 600, 8, 8
    base = (rs.rand(1, Tn, 3) * 2 - 1).astype(F32)
    p = base[:, rs.choice(Tn, Tn, replace=True)]
    assert len(np.unique(p[0], axis=0)) < 0.7 * Tn
    W = rs.randn(C, 3).astype(F32)
    net = (p.astype(np.float64) @ W.astype(np.float64).T).astype(F32)           # copies of a point give bit-identical rows
    cell = R.cells_ref(p, 2)[0]
    keys, pooled = R.cell_max_ref(net, cell, ncell)
    r = rs.randn(1, Tn, C).astype(F32)                                          # upstream gradient of the pooled, gathered features
    acc, cnt, s, _ = R.cell_scatter_ref(r, cell, ncell)
    nt = _t(net).requires_grad_(True)
    idx = torch.from_numpy(cell.astype(np.int64))[:, :, None].expand(1, Tn, C)
    pt = torch.full((1, ncell, C), -np.inf, dtype=torch.float64).scatter_reduce(1, idx, nt, reduce="amax", include_self=True).gather(1, idx)
    pt.backward(_t(r))
    dW_torch = nt.grad[0].numpy().T @ p[0].astype(np.float64)
    new, old = R.cell_max_bwd_ref(net, keys, acc, cell), R.cell_max_bwd_old_rule(net, keys, acc, cell)
    g = R.fix_to_float(acc).astype(np.float64)
    tot_new, tot_old = np.zeros((ncell, C)), np.zeros((ncell, C))
    np.add.at(tot_new, cell[0], new[0].astype(np.float64))
    np.add.at(tot_old, cell[0], old[0].astype(np.float64))
    assert np.array_equal(tot_new, g[0])                                        # conservation, exactly
    n_tied = np.zeros((ncell, C))
    np.add.at(n_tied, cell[0], (R.f2key(net)[0] == keys[0][cell[0]]).astype(np.float64))
    assert n_tied.max() >= 2 and np.allclose(tot_old, g[0] * n_tied, rtol=1e-6)  # the old rule: n tied points -> n times the gradient
    scale = np.abs(dW_torch).max()
    dW_new, dW_old = new[0].astype(np.float64).T @ p[0], old[0].astype(np.float64).T @ p[0]
    assert np.abs(dW_new - dW_torch).max() < 1e-6 * scale
    assert np.abs(dW_old - dW_torch).max() > 0.1 * scale
    # the per-point statement the GPU test asserts fails under the old rule and holds under the contract
    assert not np.array_equal(old, new) and (np.count_nonzero(new, 1) <= ncell).all()
