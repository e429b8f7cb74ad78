"""CPU test of the workspace layouts (csrc/sfmi_ragged.h's SfmiCarver): every ported sfmi_*_workspace_bytes returns, byte
for byte, what it returned when its launcher still re-derived the offsets by hand.  Pure host arithmetic of the built library."""
import ctypes

import pytest

from shapeformer_amd import _lib as L

# Recorded from the build of commit 2872531 (the last one whose size functions added up align256 terms next to a hand-written carve).
# Each table holds the refused arguments (0), N = 0 / T = 0 / B = 1, a shape with S == 1 and one with S > 1 where a split search
# decides the layout (nn_dist, mesh_sdf, knn), k in each knn instance (8, 16, 32, 64), tangent batches whose centroid reuse
# (24 B bytes) exceeds the forest, and odd P and N for emd.
SIZES = {
    "nn_dist": [
        ((0, 10, 10), 0),
        ((1, -1, 10), 0),
        ((1, 10, -1), 0),
        ((1, 0, 0), 256),
        ((3, 0, 5), 256),
        ((1, 100, 100), 256),
        ((1, 100, 40000), 51456),
        ((2, 1000, 100000), 512256),
        ((1, 100000, 100000), 32800512),
        ((90, 9000000, 9000000), 768),
        ((7, 333, 77777), 56576),
    ],
    "mesh_sdf": [
        ((0, 10, 10), 0),
        ((1, -1, 10), 0),
        ((1, 10, -1), 0),
        ((1, 0, 0), 512),
        ((1, 0, 12), 1280),
        ((1, 200, 0), 4352),
        ((2, 200, 12), 5120),
        ((1, 777, 100001), 8796160),
        ((3, 5000, 300000), 29120256),
        ((1, 2000000, 50000), 68000256),
        ((2, 1024, 12), 17664),
        ((1, 512, 4096), 852224),
    ],
    "hpr": [
        ((0, 10), 0),
        ((1, -1), 0),
        ((1, 0), 1280),
        ((5, 0), 1280),
        ((1, 1), 1280),
        ((2, 300), 9216),
        ((3, 1001), 28928),
        ((64, 1000000), 28000512),
    ],
    "knn": [
        ((0, 1, 1, 8), 0),
        ((1, -1, 1, 8), 0),
        ((1, 1, -1, 8), 0),
        ((1, 100, 100, 0), 0),
        ((1, 100, 100, 65), 0),
        ((1, 0, 0, 8), 256),
        ((3, 0, 100, 64), 256),
        ((1, 100, 100, 8), 256),
        ((1, 100, 40000, 8), 409856),
        ((1, 100, 40000, 9), 819456),
        ((1, 100, 40000, 16), 819456),
        ((1, 100, 40000, 32), 1638656),
        ((1, 100, 40000, 33), 3277056),
        ((1, 100, 40000, 64), 3277056),
        ((1, 40000, 40000, 8), 81920256),
        ((2, 777, 99999, 5), 3182848),
        ((64, 1048576, 1048576, 16), 768),
        ((1, 1001, 1001, 64), 256),
    ],
    "tangent": [
        ((0, 10), 0),
        ((1, -1), 0),
        ((1, 2147483648), 0),
        ((1, 0), 256),
        ((1, 1), 2816),
        ((2, 300), 12544),
        ((3, 1001), 37120),
        ((1, 100000), 3601152),
        ((1000, 10), 24064),
        ((65535, 0), 1572864),
        ((4096, 4096), 147712),
    ],
    "emd": [
        ((0, 10), 0),
        ((1, -1), 0),
        ((1, 1099511627776), 0),
        ((3, 0), 512),
        ((1, 1), 2048),
        ((1, 255), 7680),
        ((2, 1001), 29184),
        ((4, 8192), 229888),
        ((3, 6151), 174080),
        ((261, 4097), 129024),
    ],
    "mc": [
        ((1, 2), 1024),
        ((1, 8), 8704),
        ((2, 8), 16896),
        ((1, 17), 79360),
        ((3, 33), 1726720),
        ((1, 128), 33579520),
        ((2, 65), 8795136),
    ],
    "poisson_cg": [
        ((0, 17), 0),
        ((1, 0), 0),
        ((1, 17), 60928),
        ((2, 17), 120064),
        ((1, 33), 433408),
        ((3, 65), 9892608),
        ((1, 129), 25770496),
        ((2, 257), 407432192),
    ],
}


@pytest.fixture(scope="module")
def lib():
    from shapeformer_amd import build as B
    B.build(verbose=False)
    return ctypes.CDLL(L.LIB_PATH)


@pytest.mark.parametrize("tool", sorted(SIZES))
def test_workspace_bytes_are_unchanged(lib, tool):
    f = getattr(lib, "sfmi_%s_workspace_bytes" % tool)
    f.restype, f.argtypes = L.PROTOTYPES["sfmi_%s_workspace_bytes" % tool]
    for args, want in SIZES[tool]:
        assert f(*args) == want, (tool, args)


def test_tables_cover_what_they_claim(lib):
    """the shapes named in the comment above are in the tables: a refusal, a split and an unsplit shape, every knn instance"""
    plain = 256                                              # one set's block offsets alone
    for tool in ("nn_dist", "knn"):
        sizes = [w for _, w in SIZES[tool]]
        assert 0 in sizes and plain in sizes and max(sizes) > 4096
    assert len({w for a, w in SIZES["knn"] if a[:3] == (1, 100, 40000)}) == 4
    assert any(w == 0 for _, w in SIZES["mesh_sdf"]) and any(w == 0 for _, w in SIZES["emd"])
    assert dict(SIZES["tangent"])[(1000, 10)] == (24 * 1000 + 255) // 256 * 256             # the centroids win over a 10-point forest
