"""The `_stats` twins of the three head entry points (per-pixel uncertainty planes) reject what their twins reject, with the same negative
code and a message, `stats` given -- no kernel is launched, this runs without a GPU; and the model refuses the map in training mode."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from cfpnet_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return hip.load()


def test_plane_constants_match_the_header():
    from cfpnet_amd import hip
    text = open(os.path.join(ROOT, "include", "cfpnet_hip.h")).read()
    assert "enum { CFP_UNC_STD = 0, CFP_UNC_ENTROPY = 1, CFP_UNC_PMAX = 2 };" in text
    assert (hip.UNC_STD, hip.UNC_ENTROPY, hip.UNC_PMAX) == (0, 1, 2)


def test_stats_entry_points_validate_like_their_twins(lib):
    """Each pair is called with the same invalid arguments (16 = a non-null, 16-byte aligned dummy pointer; nothing is dereferenced):
    same code, and a message naming the problem."""
    from cfpnet_amd import hip
    P = 16

    def pair(name, args, stats_at, code, word):
        rc0 = getattr(lib, name)(*args)
        msg0 = hip.last_error()
        rc1 = getattr(lib, name + "_stats")(*(args[:stats_at] + (P,) + args[stats_at:]))
        msg1 = hip.last_error()
        assert rc0 == rc1 == code, (name, rc0, rc1)
        assert word in msg0 and msg1 == msg0, (name, msg0, msg1)

    # cfp_bin_softmax(logits, ld, centers, prob, pred, B, HW, nbins, dtype, stream)
    pair("cfp_bin_softmax", (P, 256, P, 0, 0, 1, 64, 256, hip.F32, 0), 5, -1, "null")               # null pred
    pair("cfp_bin_softmax", (P, 256, P, 0, P, 1, 64, 256, 7, 0), 5, -1, "dtype")                    # bad dtype
    pair("cfp_bin_softmax", (P, 256, P, 0, P, 1, 64, 100, hip.F32, 0), 5, -2, "64, 128 or 256")     # nbins = 100
    # cfp_bin_head_fused(x, x_ld, w, bias, centers, prob, pred, B, HW, Cin, dtype, stream)
    pair("cfp_bin_head_fused", (P, 128, P, P, P, 0, 0, 1, 64, 128, hip.BF16, 0), 7, -1, "null")
    pair("cfp_bin_head_fused", (P, 128, P, P, P, 0, 0, 1, 64, 128, hip.F32X3, 0), 7, -1, "null")
    pair("cfp_bin_head_fused", (P, 128, P, P, P, 0, P, 1, 64, 128, hip.F32, 0), 7, -1, "bf16/f16 or CFP_F32X3")
    pair("cfp_bin_head_fused", (P, 128, P, P, P, 0, P, 1, 60, 128, hip.F16, 0), 7, -2, "multiples of 8")     # HW % 8
    pair("cfp_bin_head_fused", (P, 128, P, P, P, 0, P, 1, 62, 128, hip.F32X3, 0), 7, -2, "multiples of 4")   # HW % 4
    # cfp_depth_head_fused(x, x_ld, w3, scale3, shift3, wout_perm, bias_out, centers, prob, pred, ram_out, B, H, W, flags, dtype, stream)
    pair("cfp_depth_head_fused", (P, 128, P, 0, 0, P, P, P, 0, 0, 0, 1, 16, 16, 0, hip.F16, 0), 10, -1, "null")
    pair("cfp_depth_head_fused", (P, 128, P, 0, 0, P, P, P, 0, P, 0, 1, 16, 16, 0, hip.F32, 0), 10, -1, "bf16/f16 only")
    pair("cfp_depth_head_fused", (P, 128, P, 0, 0, P, P, P, 0, P, 0, 1, 12, 14, 0, hip.BF16, 0), 10, -2, "multiple of 16")   # H*W % 16
    with pytest.raises(RuntimeError, match="cfp_bin_softmax_stats failed"):
        hip.call("cfp_bin_softmax_stats", P, 256, P, 0, P, P, 1, 64, 100, hip.F32, 0)


def test_uncertainty_needs_eval_mode():
    """The training head is another kernel: asking a model in .train() for the map is a host-side ValueError before anything runs."""
    from cfpnet_amd import config
    from cfpnet_amd.deltar import make_model
    args = config.parse_args(["@" + os.path.join(ROOT, "configs", "cfpnet_combine1.txt")])
    m = make_model(args).train()
    with pytest.raises(ValueError, match="return_uncertainty"):
        m({"rgb": None}, return_uncertainty=True)
    m.eval()
