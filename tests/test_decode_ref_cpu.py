"""CPU side of the decode-kernel harness (tests/decode_ref.py): the fragment-packed layout against the library's packers, the float64
references against the model's definition, the error bounds against deliberate mistakes (a bound that a dropped k16-step, a
swapped row, a missing split-K slice or a dropped key does not exceed would let those bugs pass), dgemm_form against the launcher's
padded-row contract, and the decode GEMM's argument checks.  No GPU."""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import decode_ref as R   # noqa: E402


def _lib():
    from shapeformer_amd import _lib as L
    return L.lib()


@pytest.mark.parametrize("N,K", [(64, 32), (50, 48), (4097, 16), (3, 96)])
def test_pack_matches_host_packer_and_pack_skinny16(N, K):
    from shapeformer_amd.gpt import pack_skinny16
    lib = _lib()
    w = torch.randn(N, K, generator=torch.Generator().manual_seed(N * K))
    want = np.empty(lib.sfmi_skinny16_pack_floats(N, K), np.float32)
    assert lib.sfmi_skinny16_pack_weight(w.numpy().ctypes.data, N, K, want.ctypes.data) == 0
    got = R.pack(w)
    assert np.array_equal(got.numpy(), want)
    assert torch.equal(got, pack_skinny16(w))
    assert torch.equal(R.unpack_weight(torch.from_numpy(want), N, K), w)


@pytest.mark.parametrize("M,N,rows", [(1, 16, None), (17, 48, None), (80, 32, 96), (192, 4096, None)])
def test_unpack_inverts_pack_and_pk_off_is_the_layout(M, N, rows):
    a = torch.randn(M, N, generator=torch.Generator().manual_seed(M + N))
    p = R.pack(a, rows)
    assert p.numel() == (rows or (M + 15) // 16 * 16) * N
    assert torch.equal(R.unpack(p, M, N), a)
    m, n = np.meshgrid(np.arange(M), np.arange(N), indexing="ij")
    assert np.array_equal(p.numpy()[R.pk_off(m, n, N)], a.numpy())


def test_references_restate_the_model():
    """ln_linear_ref is nn.LayerNorm -> nn.Linear -> exact GELU -> + resid (mingpt.py:103-111); decode_attn_ref is causal softmax
    attention of the last query over the cache with the step's own key / value at t; causal_attn_ref is masked softmax attention."""
    g = torch.Generator().manual_seed(1)
    x, W, b = torch.randn(5, 48, generator=g), torch.randn(20, 48, generator=g), torch.randn(20, generator=g)
    gam, bet, res = torch.randn(48, generator=g), torch.randn(48, generator=g), torch.randn(5, 20, generator=g)
    ln = torch.nn.functional.layer_norm(x.double(), (48,), gam.double(), bet.double(), 1e-5)
    want = torch.nn.functional.gelu(ln @ W.double().T + b.double()) + res.double()
    assert torch.allclose(R.ln_linear_ref(x, W, gam, bet, b, 1, res), want, rtol=1e-12, atol=1e-12)
    B, H, HD, L = 3, 2, 16, 40
    q, kn, vn = (torch.randn(B, H, HD, generator=g) for _ in range(3))
    Kc, Vc = torch.randn(B, H, L, HD, generator=g), torch.randn(B, H, L, HD, generator=g)
    lens = [1, 17, 40]
    y, bound = R.decode_attn_ref(q, kn, vn, Kc, Vc, lens)
    for b_ in range(B):
        t = lens[b_] - 1
        k = torch.cat([Kc[b_, :, :t], kn[b_, :, None]], 1).double()
        v = torch.cat([Vc[b_, :, :t], vn[b_, :, None]], 1).double()
        p = torch.softmax(torch.einsum("hd,htd->ht", q[b_].double(), k) / math.sqrt(HD), -1)
        assert torch.allclose(y[b_], torch.einsum("ht,htd->hd", p, v), rtol=1e-12, atol=1e-12)
    assert bool((bound > 0).all()) and float(bound.max()) < 1e-4
    # shared prefix: positions < shared_len come from row 0's cache
    ys, _ = R.decode_attn_ref(q, kn, vn, Kc, Vc, lens, shared_len=10)
    Ke, Ve = Kc.clone(), Vc.clone()
    Ke[:, :, :10], Ve[:, :, :10] = Kc[0, :, :10], Vc[0, :, :10]
    ye, _ = R.decode_attn_ref(q, kn, vn, Ke, Ve, lens)
    assert torch.equal(ys, ye)
    qq, kk, vv = (torch.randn(B, H, L, HD, generator=g) for _ in range(3))
    yc, _ = R.causal_attn_ref(qq, kk, vv, [40, 7, 1])
    mask = torch.ones(L, L, dtype=torch.bool).tril()
    s = (qq.double() @ kk.double().transpose(-1, -2) / math.sqrt(HD)).masked_fill(~mask, -math.inf)
    assert torch.allclose(yc[0], torch.softmax(s, -1)[0] @ vv[0].double(), rtol=1e-12, atol=1e-12)
    assert torch.allclose(yc[1, :, :7], torch.softmax(s[1, :, :7, :7], -1) @ vv[1, :, :7].double(), rtol=1e-12, atol=1e-12)


# ---------------------------------------------------------------------------------------------------- the bounds have teeth
def _ratio_rows(perturbed, ref, bound, rows):
    """per affected row: the largest |perturbed - ref| / bound over its outputs (> 1: the GPU assertion would fail on that row)"""
    return ((perturbed - ref).abs() / bound)[rows].amax(1)


@pytest.mark.parametrize("K,S,NW", [(1024, 1, 8), (4096, 1, 16), (4096, 4, 8), (1280, 5, 8), (576, 3, 4), (96, 1, 1)])
def test_gemm_bound_has_teeth(K, S, NW):
    """A dropped k16-step, two swapped rows and a missing split-K slice each exceed the [GEMM] bound on every row they touch (random
    N(0,1) activations, weights of the decode GEMMs' scale, bias and residual)."""
    g = torch.Generator().manual_seed(K + S)
    M, N = 8, 64
    x, W = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * 0.05
    c2, res = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    for act in (0, 1):
        bound = R.dgemm_plain_bound(x, W, c2, act, res, R.dgemm_depth(K, S, NW))
        ref = R.ln_linear_ref(x, W, bias=c2, act=act, resid=res)
        xd = x.clone()
        xd[:, K // 2:K // 2 + 16] = 0                                     # one k16-step missing from every row
        assert float(_ratio_rows(R.ln_linear_ref(xd, W, bias=c2, act=act, resid=res), ref, bound, slice(None)).min()) > 1
        xs = x.clone()
        xs[[2, 5]] = x[[5, 2]]                                            # rows 2 and 5 swapped
        assert float(_ratio_rows(R.ln_linear_ref(xs, W, bias=c2, act=act, resid=res), ref, bound, [2, 5]).min()) > 1
        if S > 1:
            xo = x.clone()
            xo[:, (S - 1) * (K // S):] = 0                                # the last slice of the split never added
            assert float(_ratio_rows(R.ln_linear_ref(xo, W, bias=c2, act=act, resid=res), ref, bound, slice(None)).min()) > 1


@pytest.mark.parametrize("mean_over_std", [0.0, 3.0, 30.0])
def test_layernorm_bound_has_teeth(mean_over_std):
    """The LayerNorm-fold bound at K = 4096 (its loosest point in the GPU grid: the one-pass variance and the centring A - c1 mean
    lose digits with (1 + mean^2 / var)) still sees one k16-step of (x - mean) dropped from a row: by about 7x at |mean|/std = 30
    (measured), so a bound ten times wider would let that row pass - this test fails then.  Swapped rows exceed it as well."""
    g = torch.Generator().manual_seed(int(mean_over_std) + 7)
    M, N, K = 8, 64, 4096
    x = torch.randn(M, K, generator=g) + mean_over_std
    W = torch.randn(N, K, generator=g) * 0.05
    gam, bet, bias = 1 + 0.1 * torch.randn(K, generator=g), 0.1 * torch.randn(K, generator=g), torch.randn(N, generator=g)
    c1 = (W * gam).double().sum(1).float()                                # what sfmi_ln_fold_pack_f32 stores
    bound = R.dgemm_ln_bound(x, W, gam, bet, bias, c1, 0, None, R.dgemm_depth(K, 1, 16), R.dgemm_stats_depth(K, 1, 16))
    ref = R.ln_linear_ref(x, W, gam, bet, bias)
    xd = x.clone()
    xd[:, 2048:2064] = x.double().mean(1, keepdim=True).float()           # (x - mean) of one k16-step dropped
    assert float(_ratio_rows(R.ln_linear_ref(xd, W, gam, bet, bias), ref, bound, slice(None)).min()) > 1
    xs = x.clone()
    xs[[1, 6]] = x[[6, 1]]
    assert float(_ratio_rows(R.ln_linear_ref(xs, W, gam, bet, bias), ref, bound, [1, 6]).min()) > 1


@pytest.mark.parametrize("HD,t", [(64, 1023), (16, 1023), (64, 256), (32, 63), (4, 1)])
def test_attention_bound_has_teeth(HD, t):
    """Dropping one key (the middle one of t + 1) exceeds the [ATTN] bound for every (row, head)."""
    g = torch.Generator().manual_seed(HD * 1000 + t)
    B, H = 3, 4
    q, kn, vn = (torch.randn(B, H, HD, generator=g) for _ in range(3))
    Kc, Vc = torch.randn(B, H, t + 1, HD, generator=g), torch.randn(B, H, t + 1, HD, generator=g)
    lens = [t + 1] * B
    y, bound = R.decode_attn_ref(q, kn, vn, Kc, Vc, lens)
    keep = torch.ones(t + 1, dtype=torch.bool)
    keep[t // 2] = False
    Kf, Vf = Kc.double().clone(), Vc.double().clone()
    Kf[:, :, t], Vf[:, :, t] = kn.double(), vn.double()
    p = torch.softmax(torch.einsum("bhd,bhtd->bht", q.double(), Kf)[..., keep] / math.sqrt(HD), -1)
    yd = torch.einsum("bht,bhtd->bhd", p, Vf[:, :, keep])
    assert float(((yd - y).abs() / bound).amax(-1).min()) > 1


def test_prefill_bound_has_teeth():
    g = torch.Generator().manual_seed(5)
    B, H, P, HD = 2, 2, 130, 32
    q, k, v = (torch.randn(B, H, P, HD, generator=g) for _ in range(3))
    y, bound = R.causal_attn_ref(q, k, v, [P, P])
    kd = k.clone()
    kd[:, :, 60] = -1e4 * q[:, :, 129]                                    # key 60 all but removed for the last query
    yd, _ = R.causal_attn_ref(q, kd, v, [P, P])
    assert float(((yd - y).abs() / bound)[:, :, 129].amax(-1).min()) > 1


# ---------------------------------------------------------------------------------------------------- launcher rules
def test_dgemm_form_stays_within_padded_rows():
    """Every form the launcher picks for M in 1..192 (and the test grid's K, S and knob values) addresses groups * MT * 16 rows of the
    fragment-packed operands: never more than sfmi_decode_gemm_padded_rows(M), the size every caller allocates."""
    lib = _lib()
    knobs = [{}, {"dgemm_nt2": 0}, {"dgemm_nt2": 2}, {"dgemm_nw": 4}, {"dgemm_nw": 16}, {"dgemm_un": 1}, {"dgemm_un": 3}]
    seen = set()
    for M in range(1, 193):
        padded = int(lib.sfmi_decode_gemm_padded_rows(M))
        assert padded % 16 == 0 and padded >= M
        for K, S in [(1024, 1), (1024, 4), (4096, 1), (4096, 2), (192, 1), (192, 3), (576, 1), (48, 1), (96, 1), (96, 3), (1280, 5), (384, 1)]:
            for kn in knobs:
                NT, MT, NW, UN, groups = R.dgemm_form(M, K, S, kn)
                assert groups * MT * 16 <= padded, (M, K, S, kn)
                assert groups * MT * 16 >= M and MT >= 1
                assert (NT, MT, NW, UN) in R.DGEMM_INSTANCES, (M, K, S, kn)
                steps = K // S // NW // 16
                assert steps % UN == 0 and (NT == 1 or steps % 2 == 0), "UN must divide the k16-steps of a wave"
                seen.add((NT, MT, NW, UN))
    with pytest.raises(ValueError):
        R.dgemm_form(16, 1024, 3)          # K % S
    with pytest.raises(ValueError):
        R.dgemm_form(16, 40, 1)            # K-slice not a multiple of 16


def test_decode_gemm_argument_checks():
    """sfmi_decode_gemm_f32 refuses, before any launch, a row-major output whose row stride is shorter than N or not a multiple of
    4 (rows are written as float4s up to round_up(N, 4)) and the other malformed shapes.  Runs only where no HIP device is
    visible: a check that went missing must never launch with these pointers."""
    if torch.cuda.is_available():
        pytest.skip("a HIP device is visible: the malformed launches are only attempted without one")
    lib = _lib()
    buf = np.zeros(1 << 16, np.float32)
    cnt = np.zeros(64, np.int32)
    p = buf.ctypes.data

    def call(M=16, N=50, K=64, ldo=52, packed=0, S=1, ln=0):
        return lib.sfmi_decode_gemm_f32(p, p, p if ln else None, None, None, p, M, N, K, ldo, ln, 0, packed, S,
                                        p if S > 1 else None, cnt.ctypes.data if S > 1 else None, None)
    assert call(ldo=48) == -1            # ldo < N
    assert call(ldo=50) == -1            # ldo >= N but not a multiple of 4
    assert call(ldo=54) == -1
    assert call(N=50, packed=1, ldo=0) == -1
    assert call(K=64, S=3) == -1
    assert call(K=40) == -1
    assert call(M=193, ldo=52) == -1
    assert call(M=0) == -1


def test_condtuplegpt_rejects_unsupported_head_dims():
    """Like the VQDIF modules (tests/test_plugin_gpu.py), a hyper-parameter the kernels are not built for names the limit at
    construction (before any device work), not as an SfmiError from inside the first decode step."""
    from shapeformer_amd.gpt import CondTupleGPT
    with pytest.raises(ValueError, match="n_embd=100 must be a multiple of n_head=3"):
        CondTupleGPT(n_embd=100, n_head=3, device="cuda:0")
    with pytest.raises(ValueError, match="head dim n_embd/n_head=48"):
        CondTupleGPT(n_embd=192, n_head=4, device="cuda:0")
    with pytest.raises(ValueError, match="head dim n_embd/n_head=128"):
        CondTupleGPT(n_embd=256, n_head=2, device="cuda:0")
