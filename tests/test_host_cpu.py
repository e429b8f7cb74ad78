"""CPU tests of the host logic: C-ABI surface, plugin boundary (YAML loader / dotted-class resolution),
multi-process sharding (gloo, world_size 2).  No GPU, no compute calls into the HIP library."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    hdr = open(os.path.join(ROOT, "include", "sfmi.h")).read()
    return sorted(set(re.findall(r"\b(sfmi_\w+)\s*\(", hdr)))


def test_library_exports_every_declared_symbol():
    import ctypes
    from shapeformer_amd import _lib as L
    from shapeformer_amd import build as B
    B.build(verbose=False)  # hipcc cross-compiles gfx950 without a GPU
    lib = ctypes.CDLL(L.LIB_PATH)
    names = _declared()
    assert len(names) >= 35
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    assert set(L.PROTOTYPES) == set(names), set(L.PROTOTYPES) ^ set(names)  # python binding == header
    assert lib.sfmi_version() >= 100
    lib.sfmi_sdf_pack_floats.restype = ctypes.c_size_t
    assert lib.sfmi_sdf_pack_floats() == 15876


_SYNTHETIC_HEADER = """
/* a block comment that quotes a call: sfmi_fake(int) must yield nothing;
 * nor may its second line: int sfmi_fake2(void); */
#ifndef X_H
#define X_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif
#define SFMI_OK 0
#define SFMI_EINVAL (-1)   /* bad arguments */
#define SFMI_ELAUNCH (-2)  // sfmi_fake(
// sfmi_fake(int x);
int sfmi_version(void);
size_t sfmi_bytes(int B, long long n);   /* trailing comment; with a semicolon */
long long sfmi_words(const unsigned* m,
                     unsigned seed,
                     unsigned long long seed64);
int sfmi_mixed(float* const* p, void** out, const char* name, const char* const* names, const float* x, unsigned char* mask,
               float eps,
               double tol, const int n, void* stream);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_header_parser_on_synthetic_text():
    """Declarations over several lines, every pointer and scalar spelling the header uses, (void), size_t / long long returns; comments
    and preprocessor lines yield no declaration, and #define SFMI_* integers come back as the return codes."""
    import ctypes as C
    from shapeformer_amd import _lib as L
    protos, codes = L.parse_header(_SYNTHETIC_HEADER)
    assert list(protos) == ["sfmi_version", "sfmi_bytes", "sfmi_words", "sfmi_mixed"]
    want = {
        "sfmi_version": (C.c_int, []),
        "sfmi_bytes": (C.c_size_t, [C.c_int, C.c_longlong]),
        "sfmi_words": (C.c_longlong, [C.c_void_p, C.c_uint, C.c_ulonglong]),
        "sfmi_mixed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_double, C.c_int,
                                 C.c_void_p]),
    }
    for name, (res, args) in want.items():
        assert protos[name][0] is res, name
        assert len(protos[name][1]) == len(args) and all(a is b for a, b in zip(protos[name][1], args)), (name, protos[name][1])
    assert codes == {"SFMI_OK": 0, "SFMI_EINVAL": -1, "SFMI_ELAUNCH": -2}
    # the module's own table is this parser over include/sfmi.h, and the codes it exports are the header's
    with open(L.HEADER) as f:
        real, rc = L.parse_header(f.read())
    assert real == L.PROTOTYPES and sorted(real) == _declared()
    assert (L.SFMI_OK, L.SFMI_EINVAL) == (rc["SFMI_OK"], rc["SFMI_EINVAL"]) == (0, -1)
    assert rc == {"SFMI_OK": 0, "SFMI_EINVAL": -1, "SFMI_ELAUNCH": -2, "SFMI_ENOBLAS": -3, "SFMI_ELDS": -4}


@pytest.mark.parametrize("decl, names", [
    ("int sfmi_bad_param(int n, short x, void* stream);", ["sfmi_bad_param", "short x"]),
    ("short sfmi_bad_return(int n);", ["sfmi_bad_return", "short"]),
    ("int sfmi_unnamed(int);", ["sfmi_unnamed", "int"]),
    ("int sfmi_uint(unsigned int n);", ["sfmi_uint", "unsigned int n"]),
    ("int sfmi_noargs();", ["sfmi_noargs"]),
    ("typedef int sfmi_t;", ["sfmi_t"]),
])
def test_header_parser_refuses_what_it_cannot_map(decl, names):
    """An unknown parameter type, an unknown return type and anything that is not `ret name(type name, ...)` raise SfmiError naming the
    function (and the parameter text): the parser never guesses."""
    from shapeformer_amd import _lib as L
    with pytest.raises(L.SfmiError) as e:
        L.parse_header("int sfmi_fine(int a);\n" + decl)
    for n in names:
        assert n in str(e.value), (n, str(e.value))


def test_missing_header_fails_loudly(monkeypatch, tmp_path):
    from shapeformer_amd import _lib as L
    monkeypatch.setattr(L, "HEADER", str(tmp_path / "nope.h"))
    with pytest.raises(L.SfmiError, match="REQUIRED"):
        L.load_header()


def _hipcc_sibling(tool):
    """`tool`, or its LLVM twin from the toolchain that built the library."""
    import shutil
    from shapeformer_amd import build as B
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(B._hipcc())))
    for c in (shutil.which(tool), os.path.join(rocm, "llvm", "bin", "llvm-" + tool), os.path.join(rocm, "lib", "llvm", "bin", "llvm-" + tool)):
        if c and os.path.exists(c):
            return c
    raise AssertionError(f"no {tool} / llvm-{tool} on this machine")


def test_exports_and_declarations_agree_both_ways():
    """The dynamic symbol table of the built library against the header: an `extern "C"` definition that the header does not declare
    still compiles, so `every export is declared` needs its own check beside `every declaration is exported`."""
    from shapeformer_amd import _lib as L
    from shapeformer_amd import build as B
    B.build(verbose=False)
    out = subprocess.run([_hipcc_sibling("nm"), "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {w[-1].split("@")[0] for w in (ln.split() for ln in out.splitlines()) if w and w[-1].startswith("sfmi_")}
    declared = set(L.PROTOTYPES)
    assert len(exported) >= 243
    assert exported - declared == set(), f"exported but not declared in include/sfmi.h: {sorted(exported - declared)}"
    assert declared - exported == set(), f"declared but not exported: {sorted(declared - exported)}"


def test_compiler_refuses_a_definition_that_differs_from_the_header(tmp_path):
    """The mechanism itself: a source that includes sfmi.h cannot define an entry point with other parameter types."""
    from shapeformer_amd import build as B
    src = tmp_path / "drift.hip"
    src.write_text('#include "sfmi.h"\nextern "C" int sfmi_version(int) { return 0; }\n')
    r = subprocess.run([B._hipcc()] + B.FLAGS + ["--offload-host-only", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                        "-o", str(tmp_path / "drift.o")], capture_output=True, text=True)
    assert r.returncode != 0 and "conflicting types" in r.stderr, r.stderr
    src.write_text('#include "sfmi.h"\nextern "C" int sfmi_version(void) { return 0; }\n')       # the control: the true signature compiles
    r = subprocess.run([B._hipcc()] + B.FLAGS + ["--offload-host-only", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                        "-o", str(tmp_path / "drift.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _hipcc_host(tmp_path, name, text, *more):
    """Compile `text` as the library's sources are compiled (build.FLAGS, the same include paths), host side only."""
    from shapeformer_amd import build as B
    src = tmp_path / (name + ".hip")
    src.write_text(text)
    return subprocess.run([B._hipcc()] + B.FLAGS + ["--offload-host-only", "-I", os.path.join(ROOT, "include"), "-I", B.CSRC, str(src)]
                          + list(more), capture_output=True, text=True)


def test_sfmi_try_returns_elaunch_for_a_refused_call(tmp_path):
    """SFMI_TRY in a stand-alone host program (no runtime call is made): hipSuccess passes through to the statements after it, any other
    hipError_t leaves the enclosing function with SFMI_ELAUNCH."""
    exe = tmp_path / "try"
    r = _hipcc_host(tmp_path, "try", '#include "sfmi_common.h"\n'
                    "static int f(hipError_t e) { SFMI_TRY(e); return SFMI_OK; }\n"
                    "int main() { return (f(hipSuccess) == SFMI_OK ? 0 : 1) + (f(hipErrorInvalidValue) == SFMI_ELAUNCH ? 0 : 2); }\n",
                    "-o", str(exe))
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(exe)], timeout=60).returncode == 0


def test_compiler_refuses_an_unchecked_runtime_call(tmp_path):
    """The mechanism that keeps the rule: under build.FLAGS a runtime call whose hipError_t is dropped does not compile, the SFMI_TRY
    form does, and no flag switches a warning category off."""
    from shapeformer_amd import build as B
    body = '#include "sfmi_common.h"\nextern "C" int sfmi_version(void) { %s; return SFMI_OK; }\n'
    r = _hipcc_host(tmp_path, "bare", body % "hipMemsetAsync(nullptr, 0, 4, nullptr)", "-c", "-o", str(tmp_path / "bare.o"))
    assert r.returncode != 0 and "nodiscard" in r.stderr, r.stderr
    r = _hipcc_host(tmp_path, "tried", body % "SFMI_TRY(hipMemsetAsync(nullptr, 0, 4, nullptr))", "-c", "-o", str(tmp_path / "tried.o"))
    assert r.returncode == 0, r.stderr
    assert [f for f in B.FLAGS if f.startswith("-Wno-")] == []


def test_runtime_calls_have_one_spelling():
    """No source silences a runtime call's result with a cast, and the dynamic-LDS limit is raised in one place (sfmi_lds_raise)."""
    import glob
    csrc = os.path.join(ROOT, "shapeformer_amd", "csrc")
    paths = sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h")))
    assert len(paths) >= 33
    texts = {os.path.basename(p): open(p).read() for p in paths}
    assert [n for n, t in texts.items() if "(void)hip" in t] == []
    assert [n for n, t in texts.items() if "hipFuncSetAttribute" in t] == ["sfmi_common.h"]


def test_check_names_the_code():
    from shapeformer_amd import _lib as L
    assert L.CODES == {"SFMI_OK": 0, "SFMI_EINVAL": -1, "SFMI_ELAUNCH": -2, "SFMI_ENOBLAS": -3, "SFMI_ELDS": -4}
    assert L.check(0, "x") is None
    with pytest.raises(L.SfmiError, match=r"x failed with code -2 \(SFMI_ELAUNCH\)"):
        L.check(-2, "x")
    with pytest.raises(L.SfmiError, match=r"x failed with code -4 \(SFMI_ELDS\)"):
        L.check(-4, "x")
    with pytest.raises(L.SfmiError, match=r"x failed with code 98 \(hipError_t\)"):
        L.check(98, "x")


_REFUSED = r"""
import ctypes, sys, numpy as np
sys.path.insert(0, %r)
from shapeformer_amd import _lib as L
lib = ctypes.CDLL(L.LIB_PATH)
def fn(name):
    f = getattr(lib, name)
    f.restype, f.argtypes = L.PROTOTYPES[name]
    return f
p = lambda a: a.ctypes.data
B, G = 1, 4
off, bits = np.zeros(B + 1, np.int32), np.zeros(B * G * G * 1, np.uint32)                   # G = 4: one word per z column
rc = [fn("sfmi_voxelize_points_f32")(None, p(off), B, 0, G, p(bits), None)]
Q0, Lv, Q = 2, 1, 3                                                                         # 27 lattice points: one word per bit set
pbits, cbits = np.zeros(1, np.uint32), np.zeros(1, np.uint32)
rc.append(fn("sfmi_iso_seed_i32")(1, Q0, Lv, Q, p(pbits), p(cbits), None))
idx, hist, mode = np.zeros(8, np.int32), np.zeros(2 * 5, np.int32), np.zeros(2, np.int32)   # n = 8, K = 5, rows = 2
rc.append(fn("sfmi_mode_i32")(p(idx), 8, 5, 2, p(hist), p(mode), None))
x, y = np.zeros(8, np.float32), np.zeros(8, np.float32)
rc.append(fn("sfmi_sigmoid_f32")(p(x), p(y), 8, None))
print("RC", *rc, flush=True)
"""


@pytest.mark.skipif(torch.cuda.is_available(), reason="with a device present the runtime accepts these calls: host buffers would be wrong arguments")
def test_refused_memset_is_reported():
    """Without a device every runtime call is refused (hipErrorNoDevice), cleanly.  An entry point whose first runtime call is a memset
    returns SFMI_ELAUNCH for it instead of launching on and returning the launch's error; one that only launches keeps the positive
    hipError_t.  Host buffers of the stated sizes, a fresh process."""
    from shapeformer_amd import _lib as L
    from shapeformer_amd import build as B
    B.build(verbose=False)
    out = subprocess.run([sys.executable, "-c", _REFUSED % ROOT], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    rc = [int(v) for v in re.search(r"^RC (.*)$", out.stdout, re.M).group(1).split()]
    assert rc[:3] == [L.CODES["SFMI_ELAUNCH"]] * 3, rc
    assert rc[3] > 0, rc


def test_every_source_reaches_the_header():
    """Follow the #include "..." lines from each csrc/*.hip through csrc/*.h: every one arrives at sfmi.h, so every definition meets its
    declaration.  And no source restates what the header states: no SFMI_* code, no declaration of an entry point without its body."""
    import glob
    csrc = os.path.join(ROOT, "shapeformer_amd", "csrc")

    def reaches(path, seen):
        for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(path).read(), re.M):
            if inc == "sfmi.h":
                return True
            nxt = os.path.join(csrc, inc)
            if nxt not in seen and os.path.exists(nxt) and reaches(nxt, seen | {nxt}):
                return True
        return False

    srcs = sorted(glob.glob(os.path.join(csrc, "*.hip")))
    assert len(srcs) >= 31
    assert [os.path.basename(s) for s in srcs if not reaches(s, {s})] == []
    for path in srcs + sorted(glob.glob(os.path.join(csrc, "*.h"))):
        text = open(path).read()
        assert not re.search(r"#\s*define\s+SFMI_(OK|E[A-Z]+)\b", text), path
        assert re.findall(r"\b(?:int|size_t|long long)\s+(sfmi_\w+)\s*\([^;{}]*\)\s*;", text) == [], path


def test_host_packers_match_torch_layouts():
    """[host] packers are pure C (no GPU): fragment orders must equal the documented index formulas."""
    import ctypes
    from shapeformer_amd import _lib as L
    from shapeformer_amd.gpt import pack_skinny16
    lib = L.lib()
    w = torch.randn(70, 32)
    out = np.empty(lib.sfmi_skinny16_pack_floats(70, 32), np.float32)
    assert lib.sfmi_skinny16_pack_weight(w.numpy().ctypes.data, 70, 32, out.ctypes.data) == 0
    assert np.array_equal(pack_skinny16(w).numpy(), out)
    cw = torch.randn(6, 4, 3, 3, 3)
    co = np.empty(cw.numel(), np.float32)
    assert lib.sfmi_conv_pack_weight(cw.numpy().ctypes.data, 6, 4, 3, co.ctypes.data) == 0
    assert np.array_equal(co.reshape(27, 6, 4), cw.reshape(6, 4, 27).permute(2, 0, 1).numpy())
    assert lib.sfmi_conv_pack_weight(None, 6, 4, 3, co.ctypes.data) == -1  # error convention: negative code, no throw


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from shapeformer_amd import _lib as L
    monkeypatch.setattr(L, "_lib", None)
    monkeypatch.setattr(L, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(L.SfmiError, match="REQUIRED"):
        L.lib()


def test_product_path_refuses_cpu_devices():
    from shapeformer_amd import _lib as L
    from shapeformer_amd.gpt import CondTupleGPT
    from shapeformer_amd.vqdif import VQDIF
    with pytest.raises(L.SfmiError):
        VQDIF(res=16, device="cpu")
    with pytest.raises(L.SfmiError):
        CondTupleGPT(device="cpu")


def test_yaml_loader_and_plugin_resolution(tmp_path):
    from shapeformer_amd import plugin as P
    base = tmp_path / "vq" / "base.yaml"
    base.parent.mkdir()
    base.write_text("expr_name: a/b\npl_model_opt:\n  class: shapeformer.models.vqdif.vqdif.VQDIF\n  kwargs:\n    vq_beta: .001\n"
                    "    encoder_opt: {class: x, kwargs: {hidden_dim: 32}}\ncallbacks:\n  vis: {class: c, kwargs: {n: [1, 2]}}\n")
    child = tmp_path / "demo" / "child.yaml"
    child.parent.mkdir()
    child.write_text("inherit_from: ../vq/base.yaml\npl_model_opt:\n  kwargs:\n    vq_beta: 1.0\ncallbacks:\n  vis:\n    kwargs: {n: all}\n")
    opt = P.get_opt(str(child))
    assert opt["pl_model_opt"]["class"].endswith("VQDIF") and opt["pl_model_opt"]["kwargs"]["vq_beta"] == 1.0
    assert opt["pl_model_opt"]["kwargs"]["encoder_opt"]["kwargs"]["hidden_dim"] == 32      # recursive merge
    assert opt["callbacks"]["vis"]["kwargs"]["n"] == "all"                                  # type mismatch -> replaced
    assert opt["meta_info"]["checkpoints_dir"].endswith("experiments/a/b/checkpoints")
    assert P.instantiate_from_opt({"class": None}) is None and P.instantiate_from_opt({}) is None
    assert P.load_object("shapeformer.models.vqdif.vqdif.VQDIF") is P.VQDIFModel
    assert P.load_object("shapeformer.models.shapeformer.representers.AR_N") is P.ARNRepresenter
    from shapeformer_amd import vqdif as V
    for path, cls in (("enc.LocalPoolPointnet", V.LocalPoolPointnet), ("quantizer.Quantizer", V.Quantizer), ("dec.LocalDecoder", V.LocalDecoder)):
        assert P.load_object("shapeformer.models.vqdif." + path) is cls          # B1: the three VQDIF sub-modules (vqdif.py:28-32)
    with pytest.raises(ValueError, match="c_dim=128"):                           # unsupported hyper-parameters name the limit
        V.LocalPoolPointnet()                                                    # (the reference's own ctor defaults: c_dim 128)
    with pytest.raises(ValueError, match="vocab_size=1000"):
        V.Quantizer(1000, 128)
    with pytest.raises(NotImplementedError):
        P.load_object("shapeformer.trainer.Trainer")
    from shapeformer_amd import data as D
    assert P.load_object("shapeformer.datamodule.DataModule") is D.DataModule
    assert P.load_object("shapeformer.data.partial.VirtualScanSelector") is D.VirtualScanSelector
    with pytest.raises(NotImplementedError):
        P.load_object("shapeformer.data.ar_datasets.imnet_datasets.Imnet2LowResDataset_AR")
    # the shipped YAMLs resolve unchanged: their merged model options as committed fixtures (oracle/make_golden_configs.py,
    # oracle/make_golden_demo.py)
    gold = os.path.join(ROOT, "tests", "golden")
    o = P.get_opt(os.path.join(gold, "shapenet_scale_opt.yaml"))
    kw = o["pl_model_opt"]["kwargs"]
    assert P.load_object(o["pl_model_opt"]["class"]) is P.ShapeFormerModel
    assert kw["transformer_opt"]["kwargs"]["n_layers"] == [20, 4] and kw["block_size"] == 812
    d = P.get_opt(os.path.join(gold, "demo_ds", "demo_vqdif.yaml"))
    assert d["pl_model_opt"]["kwargs"] == P.default_vqdif_kwargs(16) | {"optim_opt": d["pl_model_opt"]["kwargs"]["optim_opt"]}


def test_rank_striding_matches_reference_rule():
    from shapeformer_amd import dist as D
    for n in range(0, 20):
        for world in (1, 2, 5, 8):
            parts = [D.effective_indices(np.arange(n) * 2, r, world) for r in range(world)]
            assert sorted(np.concatenate(parts).tolist()) == (np.arange(n) * 2).tolist()
            assert D.unshard([p.tolist() for p in parts], n) == (np.arange(n) * 2).tolist()
    assert D.effective_indices(np.arange(8), 1, 5).tolist() == [1, 6]  # plutil.py:123-139 docstring example


_WORKER = r"""
import os, sys, numpy as np, torch
sys.path.insert(0, %r)
from shapeformer_amd import dist as D
rank, world, dist = D.init_from_env("gloo")
items = np.arange(7)
mine = D.effective_indices(items, rank, world)
tok = torch.full((4, 6, 2), -1, dtype=torch.int32); ln = torch.zeros(4, dtype=torch.int32)
for j, it in enumerate(mine):
    tok[j, : it + 1] = int(it); ln[j] = int(it) + 1
tl, ll = D.gather_ragged_tokens(tok, ln, dist, world)
flat = D.unshard([[ (t[j], l[j]) for j in range(4)] for t, l in zip(tl, ll)], len(items))
ok = all(int(l) == i + 1 and bool((t[: i + 1] == i).all()) for i, (t, l) in enumerate(flat))
t = torch.tensor([float(rank + 1)]); dist.all_reduce(t, op=dist.ReduceOp.MAX)
g = torch.arange(6, dtype=torch.float32) * (rank + 1)          # flat "gradient" buffer of the trainer
D.allreduce_mean_(g, dist)
ok = ok and torch.allclose(g, torch.arange(6, dtype=torch.float32) * (1 + world) / 2)
# bucketed, overlapped gradient all-reduce of the trainer (dist.GradBuckets): buckets become ready in backward order
flat = torch.arange(40, dtype=torch.float32) * (rank + 1)
bk = D.GradBuckets(flat, {"L0": (0, 12), "L1": (12, 24), "heads": (24, 30), "emb": (30, 40)}, dist)
for name in ("heads", "L1", "L0"):
    bk.ready(name)
order = bk.finish()                                              # "emb" was never marked: finish() launches it
ok = ok and order == ["heads", "L1", "L0", "emb"] and torch.allclose(flat, torch.arange(40, dtype=torch.float32) * (1 + world) / 2)
flat.mul_(rank + 1); bk.ready("L0"); bk.finish()                 # reusable for the next step
ok = ok and torch.allclose(flat, torch.arange(40, dtype=torch.float32) * (1 + world) / 2 * (1 + world) / 2)
# north_star's path (mode "rs_ag"): in-place reduce-scatter per bucket, "optimizer" on the rank's slice only, in-place all-gather of
# the updated values; a bucket the world size does not divide ("odd", 7 elements) falls back to the ring all-reduce
base = torch.arange(47, dtype=torch.float32)
flat = base * (rank + 1)
rs = D.GradBuckets(flat, {"L0": (0, 12), "L1": (12, 24), "heads": (24, 30), "emb": (30, 40), "odd": (40, 47)}, dist, mode="rs_ag")
ok = ok and [rs.sharded(n) for n in rs.ranges] == [True, True, True, True, False] and rs.shard("L1") == (12 + 6 * rank, 18 + 6 * rank)
for name in ("heads", "L1", "L0"):
    rs.ready(name)
ok = ok and rs.finish() == ["heads", "L1", "L0", "emb", "odd"]
mean = base * (1 + world) / 2
mine = torch.zeros(47, dtype=torch.bool)
for lo, hi in rs.shard_ranges():
    mine[lo:hi] = True
ok = ok and torch.allclose(flat[mine], mean[mine]) and int(mine.sum()) == 6 + 6 + 3 + 5 + 7    # own halves + the whole odd bucket
flat[~mine] = -1.0                       # whatever the other rank's slices hold is never read ...
flat[mine] = 10.0 - 0.5 * flat[mine]     # ... the "update" touches the own slices only
rs.all_gather_params()
ok = ok and torch.allclose(flat, 10.0 - 0.5 * mean)
# the overlapped form of the same parameter gather: one collective per bucket launched in the NEXT forward's read order, each waited
# for right before its first use (GPTTrainer._param_ready); the ring bucket ("odd") has nothing to gather
flat[~mine] = -7.0
flat[mine] = 3.0 + mean[mine]
launched = rs.launch_param_gathers(["emb", "L0", "L1", "heads", "odd"])
ok = ok and launched == ["emb", "L0", "L1", "heads"] and rs.params_in_flight() == launched
ok = ok and rs.wait_params("emb") and not rs.wait_params("emb") and not rs.wait_params("odd")
ok = ok and torch.allclose(flat[30:40], 3.0 + mean[30:40]) and rs.params_in_flight() == ["L0", "L1", "heads"]
for name in rs.params_in_flight():
    ok = ok and rs.wait_params(name)
ok = ok and torch.allclose(flat, 3.0 + mean) and rs.params_in_flight() == []
# SURVEY 8(e) single-shape option (dist.sample_n_sharded): row split, collective early stop, gather in global row order - with a
# stand-in sampler (the real one needs the GPU: tests/test_ddp_gpu.py).  Row g "ends" after g + 2 checks; the loop may stop only
# when EVERY row of EVERY rank has ended: 7 rows -> after check 8, on both ranks.
class FakeGPT:
    MAX_CHAIN_ROWS, dev = 192, "cpu"
    def sample(self, rows, lens, row_offset=0, rows_total=None, ended_reduce=None, to_host=True, max_steps=64, check_every=4, stop_early=True, **kw):
        n, checks, done = rows.shape[0], 0, 0
        assert rows_total == 7 and kw.get("shared_prefix") == "auto" and bool((rows == rows[:1]).all())
        while done < max_steps:
            done += check_every; checks += 1
            mine = all(checks >= row_offset + j + 2 for j in range(n))
            if stop_early and ended_reduce(mine):
                break
        g = torch.arange(row_offset, row_offset + n)
        return dict(samples=(g[:, None, None] * 100 + torch.arange(done)[None, :, None] + torch.zeros(1, 1, 2, dtype=torch.long)),
                    log_prob=g[:, None, None].float() * torch.ones(1, done, 2), steps=done, state="not gathered")
c1 = torch.full((1, 5, 2), 3, dtype=torch.int32)
r = D.sample_n_sharded(FakeGPT(), c1, torch.tensor([5], dtype=torch.int32), 7, dist, max_steps=64, check_every=4)
ok = ok and r["steps"] == 32 and r["samples"].shape == (7, 32, 2) and r["samples"][:, 0, 0].tolist() == [0, 100, 200, 300, 400, 500, 600]
ok = ok and r["log_prob"][:, 0, 0].tolist() == [0., 1., 2., 3., 4., 5., 6.] and "state" not in r
r = D.sample_n_sharded(FakeGPT(), c1, torch.tensor([5], dtype=torch.int32), 7, dist, max_steps=12, check_every=4, stop_early=False)
ok = ok and r["steps"] == 12 and r["samples"].shape == (7, 12, 2)
try:
    D.sample_n_sharded(FakeGPT(), c1, torch.tensor([5], dtype=torch.int32), 1, dist)       # fewer sequences than ranks, early stop on:
    ok = False                                                                              # refused on EVERY rank (nobody waits in a collective)
except ValueError:
    pass
# SURVEY 8(e), the other single-shape option (dist.sdf_query_sharded): lattice planes split over the ranks (uneven: 5 planes on 2 ranks), slabs
# padded to the largest, all-gathered and cut - with a stand-in decoder whose "logit" of lattice point p is p itself
class FakeVQ:
    def decode_index(self, code_ind, grid_Q=None, sigmoid=False, x_range=None):
        x0, x1 = x_range if x_range is not None else (0, grid_Q)
        pts = torch.arange(x0 * grid_Q * grid_Q, x1 * grid_Q * grid_Q, dtype=torch.float32)
        return dict(logits=(pts + (1000.0 if sigmoid else 0.0))[None, :, None].repeat(code_ind.shape[0], 1, 1))
for sg in (False, True):
    lg = D.sdf_query_sharded(FakeVQ(), torch.zeros(3, 2, 2, 2), 5, dist, sigmoid=sg)["logits"]
    ok = ok and lg.shape == (3, 125, 1) and torch.equal(lg[1, :, 0], torch.arange(125, dtype=torch.float32) + (1000.0 if sg else 0.0))
try:
    D.sdf_query_sharded(FakeVQ(), torch.zeros(1, 2, 2, 2), 1, dist)      # fewer planes than ranks
    ok = False
except ValueError:
    pass
try:      # 2 x 768 + 1 rows: only rank 1's shard (769) is over the limit, but the test is on ceil(S / world): BOTH ranks refuse
    D.sample_n_sharded(FakeGPT(), c1, torch.tensor([5], dtype=torch.int32), 2 * 4 * 192 + 1, dist, stop_early=False)
    ok = False
except ValueError as e:
    ok = ok and "769 rows" in str(e)
try:      # the ranks hold DIFFERENT conditions (the reference's item split): refused on every rank before anyone samples
    D.sample_n_sharded(FakeGPT(), c1 + rank, torch.tensor([5], dtype=torch.int32), 7, dist, max_steps=8, check_every=4)
    ok = False
except ValueError as e:
    ok = ok and "different conditions" in str(e)
print("OK" if ok and t.item() == world else "FAIL", flush=True)
dist.barrier(); dist.destroy_process_group()
"""


def test_two_process_gloo_sharding(tmp_path):
    script = tmp_path / "w.py"
    script.write_text(_WORKER % ROOT)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29731", WORLD_SIZE="2")
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = [p.communicate(timeout=180)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    assert all("OK" in o for o in outs), outs


def test_reference_dotted_paths_become_importable():
    """B1: `importlib.import_module("shapeformer....")` - what the reference's own sysutil.load_object does - resolves to the
    native classes once plugin.install_aliases() ran (synthetic modules; the reference tree is not on sys.path here)."""
    import importlib
    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "from shapeformer_amd import plugin as P, data as D\n"
        "assert P.install_aliases()\n"
        "import importlib\n"
        "m = importlib.import_module('shapeformer.models.vqdif.vqdif')\n"
        "assert m.VQDIF is P.VQDIFModel and callable(m.VisSparseRecon3D)\n"
        "from shapeformer_amd import vqdif as V\n"
        "assert importlib.import_module('shapeformer.models.vqdif.enc').LocalPoolPointnet is V.LocalPoolPointnet\n"
        "assert importlib.import_module('shapeformer.models.vqdif.quantizer').Quantizer is V.Quantizer\n"
        "assert importlib.import_module('shapeformer.models.vqdif.dec').LocalDecoder is V.LocalDecoder\n"
        "assert importlib.import_module('shapeformer.models.shapeformer.transformer.mingpt').CondTupleGPT is P.CondTupleGPTModel\n"
        "assert importlib.import_module('shapeformer.data.partial').VirtualScanSelector is D.VirtualScanSelector\n"
        "from shapeformer.models.shapeformer.representers import AR_N\n"
        "assert AR_N is P.ARNRepresenter\n"
        "import shapeformer.datamodule as dm; assert dm.DataModule is D.DataModule\n"
        "print('OK')\n") % ROOT
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "OK" in out.stdout, out.stderr


def test_default_chain_count_rule():
    """pipeline.default_chains: <= 64 rows per chain below 192 rows, four chains (one per hardware queue) from 192 rows on."""
    from shapeformer_amd.pipeline import default_chains
    assert [default_chains(b) for b in (1, 16, 31, 32, 64, 65, 128, 191)] == [1, 1, 1, 2, 2, 2, 2, 3]
    assert [default_chains(b) for b in (192, 256, 320, 384, 1024)] == [4, 4, 4, 4, 4]
    assert default_chains(1025) == 4      # never more chains than hardware queues: a chain holds <= 192 rows, batches beyond 768 rows
                                          # run as successive rounds of 4 chains (gpt.sample_microbatched; GPU: test_pipeline_gpu)


def test_bench_refuses_inconsistent_rank_environment(monkeypatch):
    """bench.launch_ranks: a WORLD_SIZE that disagrees with --gpus is an error, never a silent 1-rank run (no GPU needed)."""
    import argparse
    import bench
    monkeypatch.setenv("WORLD_SIZE", "4")
    with pytest.raises(SystemExit) as e:
        bench.launch_ranks(argparse.Namespace(gpus=2, share_device=False))
    assert "WORLD_SIZE=4" in str(e.value)
    bench.launch_ranks(argparse.Namespace(gpus=4, share_device=False))   # consistent: returns (we are a torchrun rank)
    monkeypatch.delenv("WORLD_SIZE")
    bench.launch_ranks(argparse.Namespace(gpus=1, share_device=False))   # one rank: nothing to launch
    import torch
    if torch.cuda.device_count() < 2:                                    # more ranks than visible GPUs (0 here, 1 on the test box)
        with pytest.raises(SystemExit) as e:
            bench.launch_ranks(argparse.Namespace(gpus=2, share_device=False))
        assert f"only {torch.cuda.device_count()} GPU" in str(e.value)


def test_bench_plain_run_options_and_output_dump(monkeypatch, tmp_path):
    """bench.py: a plain run turns every extra measurement off, --full turns them back on (each --no-* option still applies);
    --dump-outputs writes float32 / float64 arrays within the budget - whole lattices of seeded rows, or seeded points of one
    lattice when a lattice alone is over it (fake outputs, budget shrunk, no GPU needed)."""
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "3"])
    a = bench.parse()
    assert a.steps == 3 and not a.full and a.no_roofline and a.no_kernels and a.no_subrecords and a.no_cpu_baseline
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--no-kernels"])
    a = bench.parse()
    assert a.full and not (a.no_roofline or a.no_subrecords or a.no_cpu_baseline) and a.no_kernels
    monkeypatch.setattr(bench, "DUMP_BYTES", 400_000)
    g = torch.Generator().manual_seed(0)
    for B, P, n_rows, sampled in ((6, 20_000, 3, False), (2, 200_000, 1, True)):
        ri = lambda hi, *shape: torch.randint(0, hi, shape, generator=g, dtype=torch.int32)
        r = dict(c_ind=ri(4097, B, 40, 2), Lc=ri(40, B), empty_index=ri(4096, B), dense=ri(4097, B, 16, 16, 16).long(),
                 log_prob=torch.randn(B, 32, 2, generator=g), occupancy=torch.randn(B, P, generator=g),
                 state=dict(seq=ri(4097, B, 50, 2), len=ri(50, B)))
        d = tmp_path / f"B{B}_P{P}"
        bench.dump_outputs(str(d), r)
        out = {f.stem: np.load(f) for f in d.iterdir()}
        assert all(v.dtype in (np.float32, np.float64) for v in out.values())
        assert sum(v.nbytes for v in out.values()) <= bench.DUMP_BYTES
        assert np.array_equal(out["tokens"], r["state"]["seq"].numpy()) and np.array_equal(out["dense"], r["dense"].numpy())
        assert np.allclose(out["occupancy_mean"], r["occupancy"].double().mean(1).numpy(), rtol=0, atol=1e-12)
        rows = out["occupancy_rows"].astype(np.int64)
        ref = r["occupancy"].numpy()[rows]
        assert rows.size == n_rows and ("occupancy_points" in out) == sampled
        if sampled:
            ref = ref[:, out["occupancy_points"].astype(np.int64)]
        assert np.array_equal(out["occupancy"], ref)


def test_oracle_frozen_branch_hooks_reproduce_the_natural_forward():
    """oracle.vqdif_oracle.RELU_MASKS / POOL_INDEX (the frozen-branch gradient comparison of tests/test_train_vqdif_gpu.py): with
    the masks / selections of the oracle's OWN forward installed, the UNet gives the same output and input gradient."""
    import torch
    import torch.nn.functional as F
    from oracle import vqdif_oracle as VO
    from shapeformer_amd import weights as W
    sd = VO.to_torch_sd(W.make_state_dict(W.vqdif_spec(16)))
    x = torch.randn(1, 128, 8, 8, 8)
    rec_m, rec_p = [], []
    relu0, pool0 = VO._relu, VO._max_pool2

    def relu_tap(t):
        y = F.relu(t)
        rec_m.append((y > 0).permute(0, 2, 3, 4, 1).contiguous() if t.dim() == 5 else (y > 0))
        return y

    def pool_tap(t):
        y, ind = F.max_pool3d(t, 2, return_indices=True)
        D = t.shape[-1]
        k = ((ind // (D * D)) % 2) * 4 + (((ind // D) % D) % 2) * 2 + (ind % D) % 2
        rec_p.append(k.permute(0, 2, 3, 4, 1).contiguous())
        return y
    VO._relu, VO._max_pool2 = relu_tap, pool_tap
    try:
        xa = x.clone().requires_grad_(True)
        ya = VO.unet3d(sd, xa)
        ga, = torch.autograd.grad(ya.square().sum(), xa)
    finally:
        VO._relu, VO._max_pool2 = relu0, pool0
    assert len(rec_m) == 10 and len(rec_p) == 2
    VO.RELU_MASKS, VO.POOL_INDEX = list(rec_m), list(rec_p)
    try:
        xb = x.clone().requires_grad_(True)
        yb = VO.unet3d(sd, xb)
        gb, = torch.autograd.grad(yb.square().sum(), xb)
        assert not VO.RELU_MASKS and not VO.POOL_INDEX
    finally:
        VO.RELU_MASKS = VO.POOL_INDEX = None
    assert torch.equal(ya, yb) and torch.allclose(ga, gb, rtol=0, atol=1e-6 * float(ga.abs().max()))
