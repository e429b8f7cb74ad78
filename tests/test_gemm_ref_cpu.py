"""CPU side of the GEMM harness (tests/gemm_ref.py): the Python mirrors against the library's host functions, the case tables of
tests/test_gemm_kernels_gpu.py against the mirrors of the device-side work split (every form reached, no row that adds nothing), the
soundness of the stream-K partition (every unit owned once, writer slot == reader slot), the bound against correct f32 products in
several summation orders and against the mutants (dropped k, skipped / doubled slice, swapped interleaved rows / columns, wrong
stride for resid / aux / C2, dropout indexed with ldc, bias after the activation), and the accept / refuse mirror against the
refusals of both entries.  No GPU: only host functions and refused calls are made.

What the shapes of the old tests (test_sgemm_gpu.py, test_sgemm_sk_gpu.py) did not reach, from the same mirrors
(test_what_the_old_tables_missed): a workgroup with a partial, whole tiles and a second partial in the 64 x 64 form; any workgroup that
mixes whole and cut tiles in the 128 x 128 form; three chunks per workgroup, K % 4 != 0 and a short panel after a full one in
csrc/sgemm.hip.  (S = 8 and its uneven cut WERE reached, by 256 x 256 x 4096 and 1024 x 256 x 3992.)  What their parametrisation
did not reach whatever the shape: the four <.., 1, 1> stream-K instances, the halving of S by a small scratch, any ld* other than the
row length, a slab or counter array of the exact size, sk_stagger, the device-memory seed, dropout against train_ref.dropout_mul.

How much room the bound leaves (printed with pytest -s): a correct f32 product reaches 0.59 of the bound (K = 4: the bound is five
roundings) and stays within it in every order at every case; each product mutant exceeds it by a factor of 10 to 10^9 wherever it
applies; the correct f32 epilogue reaches 0.39 of its bound."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import gemm_ref as R                                   # noqa: E402
import test_gemm_kernels_gpu as G                      # noqa: E402

SK_ALL = G.SK_CASES + [G.SK_ODD_K]
SG_ALL = G.SG_CASES + [G.SG_ODD_K]


def _lib():
    from shapeformer_amd import _lib as L
    return L.lib()


def _sg_S(M, N, K):
    """the slice counts the sgemm.hip product test launches a case with"""
    return sorted({R.mfma_launch_splits(M, N, K, None if w is None else w * M * N) for w in G.SG_WS})


# ---------------------------------------------------------------------------------------------------- mirrors == host functions
def test_mirrors_equal_the_host_functions():
    lib = _lib()
    dims = (1, 4, 63, 64, 65, 127, 128, 129, 132, 500, 1028, 2564, 4096, 16384)
    ks = (1, 4, 31, 32, 33, 255, 256, 511, 512, 513, 1023, 1024, 2051, 2052, 4096, 16384)
    for M in dims:
        for N in dims:
            assert lib.sfmi_sgemm_sk_cnt_ints(M, N) == R.sk_cnt_ints(M, N)
            for K in ks:
                assert lib.sfmi_sgemm_mfma_splits(M, N, K) == R.mfma_splits(M, N, K), (M, N, K)
                assert lib.sfmi_sgemm_sk_tile(M, N, K) == R.sk_tile(M, N, K), (M, N, K)
    assert lib.sfmi_sgemm_sk_slab_floats() == R.sk_slab_floats()
    assert {R.mfma_splits(M, N, K) for M in dims for N in dims for K in ks} == {1, 2, 4, 8}
    assert {R.sk_tile(M, N, K) for M in dims for N in dims for K in ks} == {1, 2}
    try:                                                   # the knob overrides the rule
        for knob in (1, 2):
            assert lib.sfmi_tune_set(b"sk_tile", knob) == 0
            assert lib.sfmi_sgemm_sk_tile(4096, 4096, 4096) == knob == R.sk_tile(4096, 4096, 4096, knob)
    finally:
        assert lib.sfmi_tune_set(b"sk_tile", 0) == 0
    # the scratch-driven halving: a slab for S - 1 slices launches S / 2
    M, N, K = 132, 132, 2052
    assert [R.mfma_launch_splits(M, N, K, w) for w in (None, 0, M * N, 2 * M * N - 1, 2 * M * N, 4 * M * N, 8 * M * N - 1, 8 * M * N)] == [1, 1, 1, 1, 2, 4, 4, 8]
    # sfmi_sgemm_sk_slab_floats() covers every geometry
    for M, N, K, tile, grid in SK_ALL:
        assert R.sk_geometry(M, N, K, tile, grid).slab <= R.sk_slab_floats() and 4 * R.sk_geometry(M, N, K, tile, grid).tiles <= R.sk_cnt_ints(M, N)


def test_block_orders_are_bijective():
    for nb in list(range(1, 70)) + [175, 256, 630, 1024]:
        assert sorted(R.xcd_remap(b, nb) for b in range(nb)) == list(range(nb))
    for nbm in range(1, 20):
        for nbn in (1, 2, 3, 9):
            tiles = [R.panel_tile(t, nbm, nbn) for t in range(nbm * nbn)]
            assert sorted(tiles) == [(m, n) for m in range(nbm) for n in range(nbn)]
    for M, N, K in SG_ALL:
        nbm, nbn = R.cdiv(M, 128), R.cdiv(N, 128)
        assert sorted(R.sg_blocks(M, N)) == [(m, n) for m in range(nbm) for n in range(nbn)]
        for S in _sg_S(M, N, K):
            cuts = R.sg_cuts(K, S)
            assert cuts[0][0] == 0 and cuts[-1][1] == R.cdiv(K, 32) and all(a[1] == b[0] for a, b in zip(cuts, cuts[1:]))
            assert all(hi > lo for lo, hi in cuts), "an empty slice would publish an all-zero partial: legal, but the tables avoid it"


# ---------------------------------------------------------------------------------------------------- partition soundness
@pytest.mark.parametrize("case", SK_ALL, ids=str)
def test_stream_k_partition_is_sound(case):
    M, N, K, tile, grid = case
    p = R.sk_plan(M, N, K, tile, grid)
    C, U_, G_ = p.C, p.units, p.G
    owned = np.zeros(U_, np.int64)
    writers = {}
    for v, segs in enumerate(p.wgs):
        assert segs, "a workgroup without work"
        assert R.sk_owner(R.sk_first_unit(v, U_, G_), U_, G_) == v
        for s in segs:
            owned[s.tile * C + s.c_lo:s.tile * C + s.c_hi] += 1
            for u in range(s.tile * C + s.c_lo, s.tile * C + s.c_hi):
                assert R.sk_owner(u, U_, G_) == v
            if not s.whole:
                writers.setdefault(s.tile, []).append((v, s.slot))
        assert sum(not s.whole for s in segs) <= 2 and all(s.whole for s in segs[1:-1])
        assert len({s.slot for s in segs if not s.whole}) == sum(not s.whole for s in segs), "two partial segments in one slot"
    assert bool((owned == 1).all())
    for t in range(p.tiles):
        w = writers.get(t, [])
        v_first, v_last = R.sk_owner(t * C, U_, G_), R.sk_owner(t * C + C - 1, U_, G_)
        if p.contributors[t] == 1:
            assert not w
            continue
        # the last arriver reads workgroups v_first .. v_last, each at the slot the READER computes
        assert [v for v, _ in w] == list(range(v_first, v_last + 1)) and len(w) == p.contributors[t]
        for v, slot in w:
            assert slot == (0 if R.sk_first_unit(v, U_, G_) // C == t else 1), (t, v)
    assert p.slab == G_ * 2 * p.BM * p.BM and (tile == 1 or p.BM == 128)


# ---------------------------------------------------------------------------------------------------- coverage from the mirrors
def _coverage(sk_cases, sg_cases):
    sk, sg, inst, sgforms = {}, {}, set(), set()
    for c in sk_cases:
        M, N, K, tile, grid = c
        sk[c] = R.sk_reaches(M, N, K, tile, grid)
        for f in G.forms_of(M, K):
            inst |= {(f, tile, loop) for loop in ((0, 1) if tile == 1 else (0,))}
    for c in sg_cases:
        M, N, K = c
        sg[c] = set().union(*(R.sg_reaches(M, N, K, S) for S in _sg_S(M, N, K)))
        sgforms |= set(G.forms_of(M, K))
    return sk, sg, inst, sgforms


def test_case_tables_reach_every_form_and_no_row_is_redundant():
    sk, sg, inst, sgforms = _coverage(SK_ALL, SG_ALL)
    missing = [f for f in R.SK_FORMS if f not in set().union(*sk.values())] + [f for f in R.SG_FORMS if f not in set().union(*sg.values())]
    missing += [f"stream-K instance {x}" for x in sorted({(f, t, l) for f in R.FORMS for t, l in G.SK_INSTANCES} - inst)]
    missing += [f"sgemm form {f}" for f in R.FORMS if f not in sgforms]
    assert not missing, f"the case tables no longer reach: {missing}"
    for table in (sk, sg):
        seen = set()
        for c, r in table.items():
            assert r - seen, f"case {c} reaches nothing the rows before it do not: remove it"
            seen |= r
    # the rows the issue names do what it says
    assert max(R.sk_plan(64, 64, 288, 1, 512).contributors) == 9
    assert set(R.sk_plan(640, 576, 224, 1, 256).contributors) == {3, 4} and set(R.sk_plan(640, 576, 224, 1, 512).contributors) == {5, 6}
    assert set(R.sk_plan(260, 132, 1060, 1, 256).contributors) == {17, 18}
    assert {"t1:wg:pw", "t1:wg:wp", "t1:wg:pwp"} <= sk[(1284, 1156, 68, 1, 256)] and R.cdiv(1284, 64) % 8 == 5
    assert _sg_S(132, 132, 2052) == [1, 2, 4, 8] and R.sg_cuts(2052, 8)[0] == (0, 8) and R.sg_cuts(2052, 8)[-1] == (56, 65)
    assert R.cdiv(1028, 128) == 9 and (9 * 2) % 8
    # the epilogue cases: every tile cut / every tile direct, S = 2 through the reduce kernel / S = 1
    for t in (1, 2):
        assert min(R.sk_plan(*G.SK_EPI_CASES["cut"], t, 512).contributors) > 1 and max(R.sk_plan(*G.SK_EPI_CASES["direct"], t, 512).contributors) == 1
    assert R.mfma_splits(*G.SG_EPI_CASES["reduce"]) == 2 and R.mfma_splits(*G.SG_EPI_CASES["direct"]) == 1
    assert len({hi - lo for lo, hi in R.sg_cuts(G.SG_EPI_CASES["reduce"][2], 2)}) == 2


def test_what_the_old_tables_missed():
    """the shapes of test_sgemm_gpu.py / test_sgemm_sk_gpu.py through the same mirrors (recorded in the module docstring)"""
    old_sk = [(M, N, K, t, 512) for t in (1, 2) for (M, N, K) in [(4, 4, 4), (256, 256, 64), (300, 132, 100), (500, 1024, 1024), (1024, 260, 499), (128, 4128, 1024),
                                                                 (1000, 384, 520)]]
    old_sk += [(M, N, K, R.sk_tile(M, N, K), g) for g in R.SK_GRIDS for (M, N, K) in [(499, 1024, 4096), (499, 1024, 3072), (3072, 1024, 499), (499, 4096, 1024),
                                                                                    (3992, 1024, 1024), (4096, 1024, 499)]]
    old_sg = [(256, 256, 64), (300, 132, 100), (128, 4128, 1024), (1000, 384, 520), (4, 4, 4), (515, 1024, 256), (515, 256, 1024), (1024, 256, 3992), (256, 256, 4096),
              (3992, 1024, 512)]
    got_sk = set().union(*(R.sk_reaches(*c) for c in old_sk))
    got_sg = set().union(*(R.sg_reaches(M, N, K, S) for (M, N, K) in old_sg for S in {1, R.mfma_splits(M, N, K)}))
    miss = [f for f in R.SK_FORMS if f not in got_sk] + [f for f in R.SG_FORMS if f not in got_sg]
    print("work-split forms the old shape tables do not reach:", miss)
    assert {"t1:wg:pwp", "t2:wg:pw", "t2:wg:wp", "t2:wg:pwp", "chunks:3", "K%4", "short-last-panel"} == set(miss)


# ---------------------------------------------------------------------------------------------------- reference, bound, mutants
_SHAPES = {}


def _shape(M, N, K):
    """operands, float64 product and |A| |B| of one shape: computed once, shared, never modified"""
    if (M, N, K) not in _SHAPES:
        op = R.operands(M, N, K, seed=M + N + K, epilogue=False)
        _SHAPES[(M, N, K)] = (op["A"], op["B"], R.f64(op["A"]) @ R.f64(op["B"]), R.abs_product(op["A"], op["B"]))
    return _SHAPES[(M, N, K)]


def _c_of(case):
    return max(R.sk_plan(*case).contributors) if len(case) == 5 else max(_sg_S(*case))


def test_correct_f32_products_stay_within_the_bound_in_every_order():
    worst = 0.0
    for case in SK_ALL + SG_ALL:
        M, N, K = case[:3]
        A, B, P, AB = _shape(M, N, K)
        bound = R.gamma(K + _c_of(case)) * AB
        cuts = [R.sg_cuts(K, S) for S in _sg_S(M, N, K)] if len(case) == 3 else [R.sg_cuts(K, min(_c_of(case), R.cdiv(K, 32)))]
        for order, ct in [("blas", None), ("chunks", None), ("reverse", None)] + [("slices", c) for c in cuts]:
            r = R.ratio(R.product_f32(A, B, order, ct), P, bound)
            worst = max(worst, r)
            assert r <= 1.0, (case, order, r)
    print(f"[ratio] correct f32 products, every order: largest error / bound {worst:.3f}")
    assert worst > 0.01, "a bound a correct product never comes near has no teeth"


def _cut_tile(case):
    """(M-tile, N-tile, BM, c_lo, c_hi) of one partial segment of a stream-K case, or the second slice of a sgemm.hip case"""
    if len(case) == 3:
        M, N, K = case
        S = max(_sg_S(M, N, K))
        if S == 1:
            return None
        return (R.cdiv(M, 128) - 1, R.cdiv(N, 128) - 1, 128) + R.sg_cuts(K, S)[1]
    p = R.sk_plan(*case)
    for segs in reversed(p.wgs):
        for s in segs:
            if not s.whole:
                return R.panel_tile(s.tile, p.nbm, p.nbn, R.SK_GM) + (p.BM, s.c_lo, s.c_hi)
    return None


def test_every_product_mutant_exceeds_the_bound():
    caught = {k: [] for k in ("drop_k", "skip_slice", "double_slice", "swap_rows", "swap_cols")}
    for case in SK_ALL + SG_ALL:
        M, N, K = case[:3]
        if M * N > 800 * 800 and case[:3] != (1284, 1156, 68):      # one large shape is enough here; the GPU test runs them all
            continue
        A, B, P, AB = _shape(M, N, K)
        bound = R.gamma(K + _c_of(case)) * AB
        P32 = R.product_f32(A, B, "chunks")
        BM = 64 * case[3] if len(case) == 5 else 128
        muts = {}
        if K % 32:                                                    # the last k of the K tail, in the last tile
            muts["drop_k"] = R.mut_drop_k(P32, A, B, R.cdiv(M, BM) - 1, R.cdiv(N, BM) - 1, BM, K - 1)
        ct = _cut_tile(case)
        if ct is not None:
            muts["skip_slice"] = R.mut_slice(P32, A, B, *ct, 0)
            muts["double_slice"] = R.mut_slice(P32, A, B, *ct, 2)
        if M >= 64 and N >= 64:
            band = (M // 64 - 1, N // 64 - 1)
            muts["swap_rows"] = R.mut_swap(P32, band[0], 13, 0)
            muts["swap_cols"] = R.mut_swap(P32, band[1], 13, 1)
        for k, X in muts.items():
            r = R.ratio(X, P, bound)
            assert r > 1.0, (case, k, r)                              # wherever a mutant applies it is caught, not only "on at least one case"
            caught[k].append(r)
    for k, v in caught.items():
        assert v, f"mutant {k} applied to no case"
        print(f"[teeth] {k}: caught at {len(v)} cases, error / bound {min(v):.3g} .. {max(v):.3g}")


def _epi_config(mutant):
    """the epilogue combination in which a mutant shows"""
    return dict(resid_ld=dict(resid=True), aux_ld=dict(act=3), c2_ld=dict(act=2), drop_ld=dict(p=0.1), bias_after=dict(act=2, bias=True))[mutant]


@pytest.mark.parametrize("shape", [G.SK_EPI_CASES["cut"], G.SG_EPI_CASES["reduce"]], ids=str)
def test_epilogue_reference_and_every_epilogue_mutant(shape):
    M, N, K = shape
    op = R.operands(M, N, K, seed=K)
    P, bP = R.product_ref(op["A"], op["B"], R.cdiv(K, 32))
    P32 = R.product_f32(op["A"], op["B"], "chunks")

    def run(ldc, mutant=None, acc=False, bias=False, act=0, resid=False, p=0.0, seed=9):
        kw = dict(C0=op["C0"] if acc else None, bias=op["bias"] if bias else None, act=act, aux=op["aux"], resid=op["resid"] if resid else None, p=p, seed=seed)
        want = R.epilogue_ref(P, bP, **kw)
        C, C2 = R.epilogue_f32(P32, ldc, mutant=mutant, **kw)
        r = R.ratio(C[:, :N], want["y"], want["b"])
        if act == 2:
            r = max(r, R.ratio(C2[:, :N], want["pre"], want["b_pre"]))
        return r

    worst = 0.0
    for act in (0, 1, 2, 3):                                          # the correct emulation stays within the bound in every combination
        for acc in (False, True):
            for bias in (False, True):
                for resid in (False, True):
                    for p in G.EPI_P:
                        r = run(N + 4, None, acc, bias, act, resid, p)
                        worst = max(worst, r)
                        assert r <= 1.0, (act, acc, bias, resid, p, r)
    print(f"[ratio] correct f32 epilogue {shape}: largest error / bound {worst:.3f}")
    for mutant in R.EPILOGUE_MUTANTS:
        cfg = _epi_config(mutant)
        for ldc in (N + 4, N + 36):                                   # caught at ldc > N
            assert run(ldc, mutant, **cfg) > 1.0, (mutant, ldc)
        if mutant != "bias_after":                                    # and invisible while ldc == N: gap 4 of the old tests
            assert run(N, mutant, **cfg) <= 1.0, mutant


# ---------------------------------------------------------------------------------------------------- accept / refuse
def test_accept_refuse_mirror_against_the_library():
    """every row the mirror refuses is refused by the library (SFMI_EINVAL before anything could launch); the rows it accepts are run on
    the device by test_gemm_kernels_gpu.py::test_argument_checks_by_return_value"""
    lib = _lib()
    dummy = np.zeros(64, np.float32)
    ptrs = {k: dummy.ctypes.data for k in ("A", "B", "C", "aux", "ws", "slab", "cnt")}
    refused = {"sg": 0, "sk": 0}
    names = [n for n, _ in G.ARG_TABLE]
    assert len(set(names)) == len(names)
    for name, over in G.ARG_TABLE:
        a, x = G.arg_case(over)
        for entry, ok in zip(("sg", "sk"), G.arg_expect(name, a, x)):
            if ok is None or ok:
                continue
            assert G.arg_call(lib, entry, a, x, ptrs, None) == G.EINVAL, (name, entry)
            refused[entry] += 1
    exp = {n: G.arg_expect(n, *G.arg_case(o)) for n, o in G.ARG_TABLE}
    assert exp["base"] == (True, True) and exp["padded"] == (True, True) and exp["K odd form 10"] == (True, True)
    assert exp["act 3"] == (False, False) and exp["act 3 aux"] == (False, True) and exp["act 4"] == (False, False)
    for n in ("lda<K", "lda<M transA", "ldb<K", "ldb<N", "ldc<N"):
        assert exp[n] == (False, False), n
    for n in ("lda=M transA", "ldb=N", "p=.9"):
        assert exp[n] == (True, True), n
    assert exp["sg ws_floats<0"] == (False, None) and exp["sg ws small"] == (True, None)
    assert exp["sk slab short"] == (None, False) and exp["sk cnt short"] == (None, False)
    assert refused["sg"] >= 20 and refused["sk"] >= 24
    # the in-tree callers pass natural strides
    for tA, tB in R.FORMS:
        M, N, K = 500, 1024, 4096
        assert R.mfma_accepts(tA, tB, M, N, K, M if tA else K, K if tB else N, N) and R.sk_accepts(tA, tB, M, N, K, M if tA else K, K if tB else N, N)
