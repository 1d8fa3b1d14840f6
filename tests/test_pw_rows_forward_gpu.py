"""The whole forward with the expand convolutions of the inverted-residual blocks through cfp_pw_rows (CFP_PW_ROWS=1, the default)
against the implicit GEMM (CFP_PW_ROWS=0): bit-identical in both 16-bit modes."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from cfpnet_amd import hip, spec, synthetic, weights  # noqa: E402
from cfpnet_amd.engine import Engine  # noqa: E402

DEV = "cuda:0"


@pytest.fixture(scope="module")
def state_dict():
    return weights.make_torch_state_dict(spec.model_manifest(spec.COMBINE1_LAYERS))


# 192 x 256 with 8 x 8 zones of 20 px at batch 2: the smallest input the fusion geometry of tests/test_x2i_inplace_gpu.py accepts
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_forward_is_bit_identical_with_the_switch_off_and_on(dtype, state_dict, monkeypatch):
    inp = synthetic.make_inputs(2, 192, 256, 8, 20, seed=31, drop_hist=0.25)
    dinp = synthetic.to_device(inp, DEV)
    blocks = sum(1 for b in spec.ENC_BLOCKS if b.kind == "ir")
    res, launches = [], []
    real = hip.call
    for on in ("0", "1"):
        monkeypatch.setenv("CFP_PW_ROWS", on)
        eng = Engine(state_dict, layer_names=spec.COMBINE1_LAYERS, dtype=dtype)
        assert eng.pw_rows == (on == "1")
        names = []

        def rec(name, *a):
            names.append(name)
            real(name, *a)

        monkeypatch.setattr(hip, "call", rec)
        res.append([t.clone() for t in eng.forward(dinp)])
        torch.cuda.synchronize()
        monkeypatch.setattr(hip, "call", real)
        launches.append(names)
        del eng
    assert launches[0].count("cfp_pw_rows") == 0 and launches[1].count("cfp_pw_rows") == blocks == 24
    assert len(launches[0]) == len(launches[1])
    for name, a, b in zip(("bin_edges", "pred", "prob"), res[0], res[1]):
        assert bool(torch.isfinite(a.float()).all()), name
        assert torch.equal(a, b), (name, dtype)
