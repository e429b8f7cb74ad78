"""CPU tests of shapeformer_amd/_ragged.py: the host-side argument handling and tensor idioms the mesh tools share.
Every refusal is an SfmiError raised before the library is loaded; the prefix-sum and run helpers are checked against numpy on CPU
tensors (they are plain torch and run wherever their input lives)."""
import numpy as np
import pytest
import torch

from shapeformer_amd import _ragged as R
from shapeformer_amd._lib import SfmiError


@pytest.fixture()
def no_library(monkeypatch):
    from shapeformer_amd import _lib
    def refuse():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", refuse)


# ---- host_offsets

def test_host_offsets_accepts(no_library):
    o = R.host_offsets(None, 7, "x")
    assert o.dtype == np.int64 and o.tolist() == [0, 7]
    assert R.host_offsets(None, 0, "x").tolist() == [0, 0]
    for off in ([0, 3, 3, 7], np.array([0, 3, 3, 7], np.int32), torch.tensor([0, 3, 3, 7]), (0, 3, 3, 7)):
        o = R.host_offsets(off, 7, "x")
        assert o.dtype == np.int64 and o.tolist() == [0, 3, 3, 7]
    assert R.host_offsets([0], 0, "x", empty_ok=True).tolist() == [0]
    assert R.host_offsets([0, 5], 5, "x", empty_ok=True).tolist() == [0, 5]
    assert R.host_offsets(np.array([[0, 2, 5]]), 5, "x", flatten=True).tolist() == [0, 2, 5]


@pytest.mark.parametrize("off,n,kw,word", [
    ([0], 0, {}, "length B\\+1"),                          # B = 0 only with empty_ok
    ([], 0, dict(empty_ok=True), "length B\\+1"),
    ([0.0, 5.0], 5, {}, "integer"),
    (np.array([0, 5], np.float32), 5, dict(flatten=True), "integer"),
    ([False, True], 1, {}, "integer"),
    ([[0, 5]], 5, {}, "1-D"),
    (5, 5, {}, "1-D"),
    ([0, 4, 2, 5], 5, {}, "nondecreasing"),
    ([0, 3, 4], 5, {}, "end at 5"),
    ([0, 3, 6], 5, {}, "end at 5"),
    ([1, 5], 5, {}, "start at 0"),
    ([1], 1, dict(empty_ok=True), "start at 0"),
    ([0], 1, dict(empty_ok=True), "end at 1"),
])
def test_host_offsets_refuses(no_library, off, n, kw, word):
    with pytest.raises(SfmiError, match=word) as e:
        R.host_offsets(off, n, "the_name", **kw)
    assert "the_name" in str(e.value) and "offsets" in str(e.value)


# ---- mesh_args

def _mesh():
    return dict(verts=torch.zeros(8, 3), faces=torch.zeros(4, 3, dtype=torch.int32), voff=[0, 4, 8], toff=[0, 2, 4])


@pytest.mark.parametrize("index32", [False, True])
@pytest.mark.parametrize("change,words", [
    (dict(verts=np.zeros((8, 3), np.float32)), ["torch tensor", "verts", "HIP device", "no CPU fallback"]),
    (dict(faces=[[0, 1, 2]] * 4), ["torch tensor", "faces"]),
    (dict(verts=torch.zeros(8, 2)), [r"verts \(V,3\)", r"\(8, 2\)"]),
    (dict(verts=torch.zeros(24)), [r"verts \(V,3\)"]),
    (dict(faces=torch.zeros(4, 4, dtype=torch.int32)), [r"faces \(T,3\)", r"\(4, 4\)"]),
    (dict(faces=torch.zeros(4, 3)), ["faces", "integer"]),
    (dict(faces=torch.zeros(4, 3, dtype=torch.float64)), ["faces", "integer"]),
    (dict(faces=torch.zeros(4, 3, dtype=torch.bool)), ["faces", "integer"]),
    (dict(voff=[0, 4, 7]), ["voff", "end at 8"]),
    (dict(voff=[1, 4, 8]), ["voff", "start at 0"]),
    (dict(voff=[0, 9, 8]), ["voff", "nondecreasing"]),
    (dict(voff=[0.0, 4.0, 8.0]), ["voff", "integer"]),
    (dict(toff=[0, 2, 5]), ["toff", "end at 4"]),
    (dict(toff=[0, 3, 2, 4]), ["toff", "nondecreasing"]),
    (dict(toff=torch.tensor([0.0, 2.0, 4.0])), ["toff", "integer"]),
    (dict(voff=[0], toff=[0]), ["voff", "offsets"]),                      # B = 0 only with empty_ok
    (dict(toff=[0, 4]), ["different batch sizes", "shapes", "2 and 1"]),
    (dict(voff=None), ["different batch sizes", "1 and 2"]),
])
def test_mesh_args_refuses(no_library, index32, change, words):
    a = _mesh()
    a.update(change)
    with pytest.raises(SfmiError) as e:
        R.mesh_args(a["verts"], a["faces"], a["voff"], a["toff"], "some_call", index32=index32)
    import re
    assert str(e.value).startswith("some_call")
    for w in words:
        assert re.search(w, str(e.value)), (w, str(e.value))


def test_mesh_args_size_bounds(no_library):
    # views: the sizes without the memory.  Both bounds are refused before anything is copied
    v, row = torch.zeros(1, 3), torch.zeros(1, 3, dtype=torch.int32)
    with pytest.raises(SfmiError, match="32-bit"):                                    # 3 T >= 2^31
        R.mesh_args(v, row.expand(2 ** 31 // 3 + 1, 3), None, None, "f", index32=True)
    with pytest.raises(SfmiError, match="32-bit"):                                    # V + T + B + 1 >= 2^31
        R.mesh_args(v.expand(2 ** 31 - 6, 3), row.expand(4, 3), None, None, "f", index32=True)
    with pytest.raises(SfmiError, match="2\\^31 faces"):                              # without index32: per shape
        R.mesh_args(v, row.expand(2 ** 31, 3), None, None, "f")


def test_mesh_args_accepts(no_library):
    a = _mesh()
    v, f, vo, to = R.mesh_args(a["verts"], a["faces"], a["voff"], a["toff"], "f")
    assert v is a["verts"] and f is a["faces"]                                        # already f32 / int32 contiguous: not copied
    assert vo.dtype == to.dtype == np.int64 and vo.tolist() == [0, 4, 8] and to.tolist() == [0, 2, 4]
    v, f, vo, to = R.mesh_args(a["verts"].double(), a["faces"].long(), None, None, "f", index32=True)
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and vo.tolist() == [0, 8] and to.tolist() == [0, 4]
    v, f, vo, to = R.mesh_args(a["verts"].t().contiguous().t(), a["faces"], np.array([0, 8]), torch.tensor([0, 4]), "f")
    assert v.is_contiguous() and torch.equal(v, a["verts"])
    # B = 0, and offsets of any array shape: what components / simplify pass
    v, f, vo, to = R.mesh_args(torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32), [0], [0], "f", index32=True, empty_ok=True)
    assert vo.tolist() == [0] and to.tolist() == [0]
    v, f, vo, to = R.mesh_args(a["verts"], a["faces"], np.array([[0, 4, 8]]), np.array([[0], [2], [4]]), "f", flatten_offsets=True)
    assert vo.tolist() == [0, 4, 8] and to.tolist() == [0, 2, 4]
    with pytest.raises(SfmiError, match="1-D"):
        R.mesh_args(a["verts"], a["faces"], np.array([[0, 4, 8]]), a["toff"], "f")
    # the device is not mesh_args' business: the caller's on_device comes last
    with pytest.raises(SfmiError, match="HIP device.*no CPU fallback"):
        R.on_device("f", v, f)


# ---- points

def test_point_sets(no_library):
    g = torch.Generator().manual_seed(0)
    p = torch.randn(3, 5, 3, generator=g)
    flat, o, shape = R.point_sets(p, None, "f")
    flat2, o2, shape2 = R.point_sets(p.reshape(15, 3), [0, 5, 10, 15], "f")
    assert shape == (3, 5) and shape2 is None
    assert torch.equal(flat, flat2) and flat.shape == (15, 3)
    assert o.dtype == o2.dtype == np.int64 and o.tolist() == o2.tolist() == [0, 5, 10, 15]
    flat, o, shape = R.point_sets(p[0], None, "f")                                    # no offsets: one set
    assert torch.equal(flat, p[0]) and o.tolist() == [0, 5] and shape is None
    flat, o, shape = R.point_sets(p[:, :0], None, "f")                                # empty sets
    assert flat.shape == (0, 3) and o.tolist() == [0, 0, 0, 0] and shape == (3, 0)
    assert R.point_sets(p.reshape(15, 3), [0, 0, 15, 15], "f")[1].tolist() == [0, 0, 15, 15]
    for bad, word in ((np.zeros((5, 3)), "torch tensor"), (torch.zeros(5, 2), r"\(N,3\)"), (torch.zeros(3), r"\(N,3\)"),
                      (torch.zeros(()), r"\(N,3\)"), (torch.zeros(2, 2, 5, 3), r"\(B,N,3\)")):
        with pytest.raises(SfmiError, match=word):
            R.point_sets(bad, None, "f")
        with pytest.raises(SfmiError, match=word):
            R.points_arg(bad, "f")
    with pytest.raises(SfmiError, match="offsets go with"):
        R.point_sets(p, [0, 5, 10, 15], "f")
    with pytest.raises(SfmiError, match="end at 15"):
        R.point_sets(p.reshape(15, 3), [0, 5, 10], "f")


# ---- pairs of clouds

def test_pair_sets_accepts(no_library):
    g = torch.Generator().manual_seed(1)
    a, b = torch.randn(7, 3, generator=g), torch.randn(9, 3, generator=g)
    fa, fb, ao, bo, shape = R.pair_sets(a, b, [0, 3, 3, 7], torch.tensor([0, 4, 9, 9]), "f")          # flat clouds with offsets
    assert fa.data_ptr() == a.data_ptr() and torch.equal(fa, a) and torch.equal(fb, b) and shape is None    # views, not copies
    assert ao.dtype == bo.dtype == np.int64 and ao.tolist() == [0, 3, 3, 7] and bo.tolist() == [0, 4, 9, 9]
    fa, fb, ao, bo, shape = R.pair_sets(a, b, None, None, "f")                                        # no offsets: one pair
    assert ao.tolist() == [0, 7] and bo.tolist() == [0, 9] and shape is None
    pa, pb = torch.randn(2, 5, 3, generator=g), torch.randn(2, 4, 3, generator=g)                     # two batches of equal B
    fa, fb, ao, bo, shape = R.pair_sets(pa, pb, None, None, "f")
    assert shape == (2, 5) and torch.equal(fa, pa.reshape(10, 3)) and torch.equal(fb, pb.reshape(8, 3))
    assert ao.dtype == bo.dtype == np.int64 and ao.tolist() == [0, 5, 10] and bo.tolist() == [0, 4, 8]
    fa, fb, ao, bo, shape = R.pair_sets(pa[:, :0], pb, None, None, "f")                               # empty sets
    assert fa.shape == (0, 3) and ao.tolist() == [0, 0, 0] and shape == (2, 0)
    ao, bo = R.pair_offsets([0, 2, 7], 7, np.array([0, 9, 9]), 9, "f", ("p", "q"))
    assert ao.dtype == bo.dtype == np.int64 and ao.tolist() == [0, 2, 7] and bo.tolist() == [0, 9, 9]
    assert [o.tolist() for o in R.pair_offsets(None, 7, None, 9, "f")] == [[0, 7], [0, 9]]


def test_pair_sets_refuses(no_library):
    a, b = torch.zeros(7, 3), torch.zeros(9, 3)
    pa, pb = torch.zeros(2, 5, 3), torch.zeros(2, 4, 3)
    for x, y, xo, yo in ((pa, b, None, None), (a, pb, None, None), (a, pb, None, [0, 4, 8]),      # mixed dimensions
                         (pa, torch.zeros(3, 4, 3), None, None),                                  # unequal B
                         (pa, pb, [0, 5, 10], None), (pa, pb, None, [0, 4, 8])):                  # offsets with batches
        with pytest.raises(SfmiError, match=r"same B and no offsets.*\(N,3\) left needs an \(M,3\) right"):
            R.pair_sets(x, y, xo, yo, "f", ("left", "right"))
    with pytest.raises(SfmiError, match="^the_call: left has 2 sets, right has 1$"):                  # the caller's names
        R.pair_sets(a, b, [0, 3, 7], None, "the_call", ("left", "right"))
    with pytest.raises(SfmiError, match="source has 1 sets, target has 3"):
        R.pair_sets(a, b, None, [0, 4, 4, 9], "f")
    with pytest.raises(SfmiError, match="p has 1 sets, q has 2"):
        R.pair_offsets(None, 7, [0, 4, 9], 9, "f", ("p", "q"))
    with pytest.raises(SfmiError, match="f l_off.*end at 7"):                                         # the offsets are named by initials
        R.pair_sets(a, b, [0, 3, 6], [0, 4, 9], "f", ("left", "right"))
    with pytest.raises(SfmiError, match="f r_off.*integer"):
        R.pair_sets(a, b, [0, 3, 7], [0.0, 4.0, 9.0], "f", ("left", "right"))
    for bad, word in ((np.zeros((5, 3)), "torch tensor"), (torch.zeros(5, 2), r"\(N,3\)")):
        with pytest.raises(SfmiError, match="f left.*" + word):
            R.pair_sets(bad, b, None, None, "f", ("left", "right"))
        with pytest.raises(SfmiError, match="f right.*" + word):
            R.pair_sets(a, bad, None, None, "f", ("left", "right"))


def test_pair_sets_bounds(no_library):
    a, b = torch.zeros(4, 3), torch.zeros(4, 3)
    assert R.pair_sets(a, b, [0, 1, 2, 4], [0, 2, 3, 4], "f", max_sets=3)[2].tolist() == [0, 1, 2, 4]
    with pytest.raises(SfmiError, match="at most 2 pairs"):
        R.pair_sets(a, b, [0, 1, 2, 4], [0, 2, 3, 4], "f", max_sets=2)
    with pytest.raises(SfmiError, match="at most 2 pairs"):
        R.pair_sets(torch.zeros(3, 2, 3), torch.zeros(3, 1, 3), None, None, "f", max_sets=2)
    many = np.arange(65537 + 1)
    row = torch.zeros(1, 3)
    with pytest.raises(SfmiError, match="at most 65535 pairs"):                                       # the default: a grid's y limit
        R.pair_sets(row.expand(65537, 3), row.expand(65537, 3), many, many, "f")
    assert len(R.pair_sets(row.expand(65535, 3), row.expand(65535, 3), many[:65536], many[:65536], "f")[2]) == 65536
    assert len(R.pair_sets(row.expand(65537, 3), row.expand(65537, 3), many, many, "f", max_sets=None)[2]) == 65538
    # views: the sizes without the memory
    with pytest.raises(SfmiError, match=r"below 2\^31 points"):
        R.pair_sets(row.expand(2 ** 31, 3), row, None, None, "f")
    with pytest.raises(SfmiError, match=r"below 2\^31 points"):
        R.pair_sets(row, row.expand(2 ** 31 + 1, 3), [0, 0, 1], [0, 2 ** 31, 2 ** 31 + 1], "f")
    assert R.pair_sets(row.expand(2 ** 31, 3), row, None, None, "f", max_sets=None)[2].tolist() == [0, 2 ** 31]


# ---- numbers

def test_check_number(no_library):
    inf = float("inf")
    assert R.check_number(2, "f", "x", 0, 5) == 2.0 and isinstance(R.check_number(2, "f", "x", 0, 5), float)
    assert R.check_number(np.float32(0.5), "f", "x", 0, 1) == 0.5 and R.check_number(np.int64(1), "f", "x", 0, 1) == 1.0
    for v in (True, False, "1", None, [1.0], np.array([1.0]), torch.tensor(1.0), 1j, float("nan"), np.float64("nan")):
        with pytest.raises(SfmiError, match=r"^the_call: the_x must be a number in \[0, 5\], got "):
            R.check_number(v, "the_call", "the_x", 0, 5)
    for v in (-1e-300, -1, 5.000001, 6, inf, -inf):                                                   # both bounds
        with pytest.raises(SfmiError, match="x must be"):
            R.check_number(v, "f", "x", 0, 5)
    # closed ends take the bound itself, open ends do not; the text says which
    assert R.check_number(0, "f", "x", 0, 5) == 0.0 and R.check_number(5.0, "f", "x", 0, 5) == 5.0
    with pytest.raises(SfmiError, match=r"in \(0, 5\]"):
        R.check_number(0, "f", "x", 0, 5, lo_open=True)
    with pytest.raises(SfmiError, match=r"in \[0, 5\)"):
        R.check_number(5, "f", "x", 0, 5, hi_open=True)
    assert R.check_number(5, "f", "x", 0, 5, lo_open=True) == 5.0 and R.check_number(0, "f", "x", 0, 5, hi_open=True) == 0.0
    assert R.check_number(1e-300, "f", "x", 0, 5, lo_open=True, hi_open=True) == 1e-300
    # no upper bound: +inf only with allow_inf, NaN never
    assert R.check_number(1e308, "f", "x", 0, inf) == 1e308
    with pytest.raises(SfmiError, match="x must be a finite number >= 0, got inf"):
        R.check_number(inf, "f", "x", 0, inf)
    with pytest.raises(SfmiError, match="x must be a finite number > 0, got 0"):
        R.check_number(0, "f", "x", 0, inf, lo_open=True)
    assert R.check_number(inf, "f", "x", 0, inf, allow_inf=True) == inf
    for v in (float("nan"), -1, -inf, True):
        with pytest.raises(SfmiError, match="x must be a number >= 0, got"):
            R.check_number(v, "f", "x", 0, inf, allow_inf=True)
    with pytest.raises(SfmiError, match="got inf"):                                                   # a finite hi keeps +inf out either way
        R.check_number(inf, "f", "x", 0, 5, allow_inf=True)
    assert R.check_nonneg(0, "f", "x") == 0.0
    for v in (inf, -1e-9, True, float("nan")):
        with pytest.raises(SfmiError, match="x must be a finite number >= 0"):
            R.check_nonneg(v, "f", "x")


# ---- which sets hold a row that is not finite

def test_nonfinite_sets():
    x = torch.zeros(7, 3)
    od = R.offsets_dev(np.array([0, 3, 3, 7]), "cpu")                                                 # three sets, the middle one empty
    assert od.dtype == torch.int64 and od.tolist() == [0, 3, 3, 7]
    out = R.nonfinite_sets(x, od)
    assert out.dtype == torch.int32 and out.tolist() == [0, 0, 0]
    x[1, 2] = float("nan")
    assert R.nonfinite_sets(x, od).tolist() == [1, 0, 0]
    x[6, 0] = float("-inf")
    assert R.nonfinite_sets(x, od).tolist() == [1, 0, 1]
    x[1, 2] = 0.0
    assert R.nonfinite_sets(x, od).tolist() == [0, 0, 1]
    assert R.nonfinite_sets(x[:, :1], od).tolist() == [0, 0, 1]                                       # rows of any width
    assert R.nonfinite_sets(x, R.offsets_dev([0, 7], "cpu")).tolist() == [1]
    assert R.nonfinite_sets(x[:0], R.offsets_dev([0, 0], "cpu")).tolist() == [0]


# ---- prefix sums and runs, against numpy

@pytest.mark.parametrize("counts", [[], [0], [3], [0, 0, 0], [2, 0, 5, 1, 0, 0, 7], list(range(40))])
def test_excl_and_excl_at(counts):
    x = torch.tensor(counts, dtype=torch.uint8)
    want = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    got = R.excl(x)
    assert got.dtype == torch.int32 and got.tolist() == want.tolist()
    assert R.excl(x.to(torch.int32)).tolist() == want.tolist()
    incl = torch.cumsum(x, 0, dtype=torch.int32)
    n = len(counts)
    for off in ([0, n], [0, 0, n], [0, n // 2, n // 2, n], list(range(n + 1))):
        got = R.excl_at(incl, torch.tensor(off, dtype=torch.int32))
        assert got.dtype == torch.int32 and got.tolist() == want[off].tolist()


@pytest.mark.parametrize("keys,n", [
    ([], 0), ([], 3), ([0], 1), ([2, 2, 2], 4), ([3, 0, 3, 1, 0, 3], 4), ([5, 1, 5, 1], 6),
    ([1, 0x7fffffff, 0, 0x7fffffff, 1], 2),                                           # keys >= n sort behind every run
])
def test_runs(keys, n):
    k = torch.tensor(keys, dtype=torch.int32)
    order, seg = R.runs(k, n)
    assert order.dtype == seg.dtype == torch.int32 and seg.shape == (n + 1,)
    a = np.asarray(keys, np.int64)
    want_order = np.argsort(a, kind="stable")
    assert order.tolist() == want_order.tolist()
    assert seg.tolist() == np.searchsorted(a[want_order], np.arange(n + 1)).tolist()
    for c in range(n):                                                                # run c = the records of key c, in input order
        assert order[seg[c]:seg[c + 1]].tolist() == np.nonzero(a == c)[0].tolist()


def test_host_to_device_helpers():
    # i32_dev / f32_dev / batch_meshes with "cpu" as the device: dtype, layout, offsets
    a = R.i32_dev(np.arange(6, dtype=np.int64)[::2], "cpu")
    assert a.dtype == torch.int32 and a.tolist() == [0, 2, 4] and a.is_contiguous()
    t = torch.zeros(2, 3, dtype=torch.float64)
    assert R.f32_dev(t, "cpu") is t                                                   # a tensor stays as it is
    f = R.f32_dev(np.arange(6.0).reshape(2, 3).T, "cpu")
    assert f.dtype == torch.float32 and f.is_contiguous() and f.tolist() == [[0, 3], [1, 4], [2, 5]]
    m = [(np.zeros((4, 3)), np.array([[0, 1, 2]])), (np.ones((3, 3)), np.array([[0, 1, 2], [2, 1, 0]], np.int64))]
    v, fc, vo, to = R.batch_meshes(m, "cpu")
    assert v.dtype == torch.float32 and v.shape == (7, 3) and fc.dtype == torch.int32 and fc.shape == (3, 3)
    assert vo.dtype == to.dtype == np.int64 and vo.tolist() == [0, 4, 7] and to.tolist() == [0, 1, 3]
    assert R.mesh_args(v, fc, vo, to, "f")[2].tolist() == [0, 4, 7]
