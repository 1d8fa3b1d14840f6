"""The f16x3 training numerics without a GPU: the cross-compiled library exports their entry points (bound by cfpnet_amd.hip), the
header documents them, and the training CLI / Trainer / module accept the "f32x3" switch."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

X3_TRAIN_SYMBOLS = ["cfp_grad_absmax", "cfp_grad_scale", "cfp_conv2d_wgrad_x3", "cfp_conv2d_dgrad_x3_ws_bytes", "cfp_conv2d_dgrad_x3",
                    "cfp_pack_w_x3_blocks", "cfp_pack_w_x3_batch"]


def test_x3_training_symbols_are_exported_declared_and_bound():
    from cfpnet_amd import hip
    lib = hip.load()
    header = open(os.path.join(ROOT, "include", "cfpnet_hip.h")).read()
    for name in X3_TRAIN_SYMBOLS:
        assert name in hip.SIGNATURES and name + "(" in header
        assert getattr(lib, name) is not None
    # host-side helpers answer without a device
    assert lib.cfp_pack_w_x3_blocks(64, 72) == (64 * 3 * 32 + 2047) // 2048
    assert lib.cfp_conv2d_dgrad_x3_ws_bytes(2, 5, 7, 16, 24, 2) == (64 + 2 * 9 * 13 * 16) * 4
    assert lib.cfp_conv2d_dgrad_x3_ws_bytes(0, 5, 7, 16, 24, 2) == 0


def test_x3_training_entry_points_validate_their_arguments():
    from cfpnet_amd import hip
    lib = hip.load()
    assert lib.cfp_pack_w_x3_batch(None, None, None, 1, 1, None) != 0
    assert lib.cfp_grad_absmax(None, 4, 10, 4, None, None) != 0
    assert lib.cfp_grad_scale(None, 4, 1, 2, 2, 4, 1, None, None, None, 0, None) != 0
    assert "cfp_grad_scale" in hip.last_error()


def test_train_cli_accepts_dtype_f32x3():
    import train as train_cli
    assert train_cli.TRAIN_DTYPES["f32x3"] == "f32x3"
    argv = ["--dtype", "f32x3", "--bs", "2"]
    assert train_cli.TRAIN_DTYPES[train_cli._pop(argv, "--dtype", "bf16")] == "f32x3" and argv == ["--bs", "2"]


def test_tape_and_module_take_the_f32x3_switch():
    import torch
    from cfpnet_amd.autograd_hip import Tape
    from cfpnet_amd.deltar import Deltar
    assert Tape("cpu", torch.float32, x3=True).x3 and not Tape("cpu", torch.float32).x3
    with pytest.raises(AssertionError):
        Tape("cpu", torch.bfloat16, x3=True)
    with pytest.raises(ValueError):
        Deltar(n_bins=16, train_dtype="f16x2")
