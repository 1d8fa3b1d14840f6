"""Argument validation of the two fused-tail entry points, cfp_loftr_tail and cfp_lkpm_tail, for the three storage modes they take:
every rejection comes back as the documented code with its message before anything is launched (no GPU needed: the pointers are
fake, 16-byte-aligned integers)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EINVAL, ESHAPE = -1, -2
P = 0x10000          # a non-null, 16-byte-aligned "pointer"
DTYPES = ("BF16", "F16", "F32X3")


@pytest.fixture(scope="module")
def lib():
    from cfpnet_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return hip.load()


def loftr_args(dtype, **kw):
    a = dict(q=P, q_ld=64, kv=P, ksum=P, x=P, x_ld=64, out=P, out_ld=64, w_q=P, w_merge=P, w_mlp0=P, w_mlp2=P, ln1_g=P, ln1_b=P, ln2_g=P,
             ln2_b=P, ln_eps=1e-5, NB=2, Hq=5, Wq=7, qth=3, qtw=3, v_length=9.0, eps=1e-6, heads=8, D=64, dtype=dtype, stream=0)
    assert set(kw) <= set(a)
    a.update(kw)
    return list(a.values())


def lkpm_args(dtype, **kw):
    a = dict(t=P, t_ld=64, xin=P, x_ld=64, out=P, out_ld=64, w1=P, b1=P, w2=P, b2=P, ln_g=P, ln_b=P, ln_eps=1e-6, rows=70, D=64, dtype=dtype,
             stream=0)
    assert set(kw) <= set(a)
    a.update(kw)
    return list(a.values())


def pitch_phrase(name):
    return "pitches must be >= D and multiples of " + ("4" if name == "F32X3" else "8")


def loftr_cases(name):
    pitch = pitch_phrase(name)
    yield "null tensor", dict(x=0), EINVAL, "null pointer"
    yield "null weights", dict(w_mlp0=0), EINVAL, "null pointer"
    yield "q and w_q both null", dict(q=0, w_q=0), EINVAL, "null pointer"
    yield "bad grid", dict(qth=0), ESHAPE, "bad grid"
    yield "D = 48", dict(D=48), ESHAPE, "D must be 32/64/128"
    yield "heads = 3", dict(heads=3), ESHAPE, "D must be 32/64/128"
    yield "pitch below D", dict(x_ld=56), ESHAPE, pitch
    yield "q pitch below D", dict(w_q=0, q_ld=56), ESHAPE, pitch
    yield "pitch no multiple of 4 or 8", dict(out_ld=66), ESHAPE, pitch
    # a multiple of 4 but not of 8: a float32 pitch of whole 16-byte vectors, not a 16-bit one.  The float32 call is then stopped by
    # the NEXT check (a misaligned pointer), which shows that it passed this one
    if name == "F32X3":
        yield "pitch 68", dict(x_ld=68, out_ld=68, x=P + 4), EINVAL, "16-byte aligned"
    else:
        yield "pitch 68", dict(x_ld=68, out_ld=68, x=P + 4), ESHAPE, pitch
    yield "misaligned tensor", dict(out=P + 8), EINVAL, "16-byte aligned"
    yield "misaligned weights", dict(w_merge=P + 2), EINVAL, "16-byte aligned"
    yield "2^31 rows", dict(NB=2, Hq=32768, Wq=32768), ESHAPE, ("bad grid", "too many rows")
    # the q pitch is not looked at when the kernel projects q itself: the call gets as far as the alignment check
    yield "q pitch unused with w_q", dict(q_ld=3, kv=P + 4), EINVAL, "16-byte aligned"


def lkpm_cases(name):
    pitch = pitch_phrase(name)
    yield "null tensor", dict(xin=0), EINVAL, "null pointer"
    yield "null bias", dict(b2=0), EINVAL, "null pointer"
    yield "D = 48", dict(D=48), ESHAPE, "D must be 32/64/128"
    yield "no rows", dict(rows=0), ESHAPE, "D must be 32/64/128"
    yield "pitch below D", dict(t_ld=56), ESHAPE, pitch
    yield "pitch no multiple of 4 or 8", dict(out_ld=66), ESHAPE, pitch
    if name == "F32X3":
        yield "pitch 68", dict(t_ld=68, x_ld=68, out_ld=68, w1=P + 4), EINVAL, "16-byte aligned"
    else:
        yield "pitch 68", dict(t_ld=68, x_ld=68, out_ld=68, w1=P + 4), ESHAPE, pitch
    yield "misaligned tensor", dict(t=P + 8), EINVAL, "16-byte aligned"
    yield "misaligned weights", dict(w2=P + 2), EINVAL, "16-byte aligned"


@pytest.mark.parametrize("name", DTYPES)
@pytest.mark.parametrize("fn, make_args, cases", [("cfp_loftr_tail", loftr_args, loftr_cases), ("cfp_lkpm_tail", lkpm_args, lkpm_cases)],
                         ids=["loftr", "lkpm"])
def test_tail_entry_points_reject_bad_arguments_before_any_launch(lib, fn, make_args, cases, name):
    from cfpnet_amd import hip
    dtype = getattr(hip, name)
    for what, change, code, phrase in cases(name):
        rc = getattr(lib, fn)(*make_args(dtype, **change))
        msg = hip.last_error()
        print(f"{fn} {name} {what}: rc = {rc}, {msg!r}")
        assert rc == code, (what, rc, msg)
        assert msg.startswith(fn + ":"), (what, msg)
        assert any(p in msg for p in ([phrase] if isinstance(phrase, str) else phrase)), (what, msg)


@pytest.mark.parametrize("fn, make_args", [("cfp_loftr_tail", loftr_args), ("cfp_lkpm_tail", lkpm_args)], ids=["loftr", "lkpm"])
def test_tail_entry_points_refuse_plain_float32(lib, fn, make_args):
    from cfpnet_amd import hip
    # the plain float32 parity mode runs the unfused kernels; it is refused first, whatever else is wrong with the call
    for change in (dict(), dict(out=0), dict(D=48)):
        rc = getattr(lib, fn)(*make_args(hip.F32, **change))
        msg = hip.last_error()
        assert rc == EINVAL and msg.startswith(fn + ":") and "bf16 / f16 or CFP_F32X3" in msg, (change, rc, msg)
        rc = getattr(lib, fn)(*make_args(7, **change))
        assert rc == EINVAL and "bf16 / f16 or CFP_F32X3" in hip.last_error(), (change, rc)
