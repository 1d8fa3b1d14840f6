"""pw_rows.hip without a GPU: the header / Makefile / binding, the query's answers on the model's expand convolutions and on the shapes
it must refuse, the column groups it chooses, and the entry point's argument checks (they come before any launch)."""
import os

import pytest

from cfpnet_amd import hip, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the expand convolutions of the inverted-residual blocks at batch 8, 480 x 640: (layers, M, K, N, launches per forward, column groups)
MODEL_SHAPES = [
    ("conv3.0.0", 38400, 56, 224, 1, 2),
    ("conv3.0.1 - conv3.0.4", 9600, 112, 448, 4, 7),
    ("conv3.1.0", 9600, 112, 672, 1, 7),
    ("conv3.1.1 - conv3.1.6", 9600, 136, 816, 6, 7),
    ("conv4.0", 9600, 136, 816, 1, 7),
    ("conv4.1 - conv4.11", 2400, 232, 1392, 11, 11),
]


def test_symbols_header_makefile_and_binding():
    lib = hip.load()
    for name in ("cfp_pw_rows", "cfp_pw_rows_fits", "cfp_pw_rows_groups"):
        assert hasattr(lib, name)
    text = open(os.path.join(ROOT, "include", "cfpnet_hip.h")).read()
    assert "int cfp_pw_rows_fits(long long M, int K, int N, int in_ld, int out_ld, int dtype);" in text
    assert "int cfp_pw_rows(const void* in, int in_ld, const void* w, const float* scale, const float* shift, int act, void* out, int out_ld," in text
    mk = open(os.path.join(ROOT, "cfpnet_amd", "csrc", "Makefile")).read()
    assert "pw_rows.hip" in mk and "pw_rows.o" in mk


@pytest.mark.parametrize("name,M,K,N,count,groups", MODEL_SHAPES)
def test_the_models_expand_convolutions_are_taken(name, M, K, N, count, groups):
    for dt in (hip.BF16, hip.F16):
        assert ops.pw_rows_fits(M, K, N, K, N, dt), name
        assert ops.pw_rows_fits(M, K, N, K + 256, N + 8, dt), name      # a slice of a concatenation buffer
    assert not ops.pw_rows_fits(M, K, N, K, N, hip.F32), name
    auto, most = ops.pw_rows_groups(M, K, N)
    assert (auto, most) == (groups, (N + 31) // 32), name
    rows = 128 if M >= 8192 else 64                                     # rows of a workgroup: 32 per wave from 8 192 rows up
    assert -(-M // rows) * auto >= 400, name                            # about two workgroups per CU


def test_the_launch_count_of_the_table():
    assert sum(c for *_, c, _ in MODEL_SHAPES) == 24


@pytest.mark.parametrize("bad", [
    (100, 264, 64, 264, 64),      # K above the register cap
    (100, 60, 64, 64, 64),        # K % 8
    (100, 64, 60, 64, 64),        # N % 8
    (100, 64, 64, 68, 64),        # input pitch not a 16-byte multiple
    (100, 64, 64, 64, 68),        # output pitch
    (100, 64, 64, 56, 64),        # pitches that do not cover the channels
    (100, 64, 64, 64, 56),
    (0, 64, 64, 64, 64),
    (1 << 31, 64, 64, 64, 64),
    (100, 0, 64, 64, 64),
])
def test_the_query_says_no(bad):
    assert not ops.pw_rows_fits(*bad, hip.BF16)
    assert ops.pw_rows_fits(100, 64, 64, 64, 64, hip.BF16) and ops.pw_rows_fits(100, 256, 8, 256, 8, hip.F16)


def test_groups_are_clamped_and_never_empty():
    for M, N in ((16, 16), (69, 816), (2400, 1392), (38400, 224), (200, 24), (64, 4096)):
        auto, most = ops.pw_rows_groups(M, 64, N)
        chunks = (N + 31) // 32
        assert most == chunks and 1 <= auto <= chunks
        cpg = -(-chunks // auto)
        assert (auto - 1) * cpg < chunks <= auto * cpg and cpg <= 64      # scale / shift of a group fit behind the weight stages


def test_error_codes():
    lib = hip.load()
    p = 4096      # never dereferenced: every check below fails before a launch
    ok = dict(inp=p, in_ld=64, w=p, scale=0, shift=0, act=hip.ACT_SILU, out=p, out_ld=64, M=100, K=64, N=64, groups=0, dt=hip.BF16)

    def rc(**kw):
        a = dict(ok, **kw)
        return lib.cfp_pw_rows(a["inp"], a["in_ld"], a["w"], a["scale"], a["shift"], a["act"], a["out"], a["out_ld"], a["M"], a["K"], a["N"],
                               a["groups"], a["dt"], 0)

    for null in ("inp", "w", "out"):
        assert rc(**{null: 0}) == -1 and b"null pointer" in lib.cfp_last_error()
    for act in (hip.ACT_RELU, hip.ACT_LRELU, hip.ACT_GELU, hip.ACT_SIGMOID, 17, -1):
        assert rc(act=act) == -1 and b"activation" in lib.cfp_last_error()
    for dt in (hip.F32, 3, 9):
        assert rc(dt=dt) == -1 and b"storage" in lib.cfp_last_error()
    assert rc(groups=-1) == -1
    assert rc(K=264, in_ld=264) == -2 and rc(K=60) == -2 and rc(N=60) == -2 and rc(in_ld=68) == -2 and rc(M=0) == -2
    assert rc(inp=p + 8) == -1 and rc(out=p + 2) == -1 and rc(scale=p + 4) == -1 and b"aligned" in lib.cfp_last_error()
