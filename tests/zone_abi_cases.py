"""The refusals `cfp_tof_zone_consistency` and `cfp_tof_zone_loss` share (`zone_args`, csrc/zone_core.h), as one table for the abi tests of
both: every message carries the entry's own name, and the first refusal reported follows the same order of kinds."""
EINVAL, ESHAPE = -1, -2

NAN = float("nan")
TABLE = (   # (return code, message after "<entry>: ", the argument sets that earn it)
    (ESHAPE, "non-positive dimension", (dict(b=0), dict(h=0), dict(w=-1), dict(hp=0), dict(wp=-3), dict(z=0), dict(z=-2))),
    (ESHAPE, "image too large", (dict(h=70000, w=70000, interp=1), dict(hp=70000, wp=70000, interp=1))),
    (ESHAPE, "sizes differ and interpolate is off", (dict(hp=4, wp=4), dict(hp=8, wp=4), dict(h=16, w=16))),
    (EINVAL, "empty depth range", (dict(lo=2.0, hi=1.0), dict(lo=1.0, hi=1.0), dict(lo=NAN, hi=1.0), dict(lo=0.0, hi=NAN),
                                   dict(lo=10.0, hi=10.0), dict(lo=5.0, hi=1.0), dict(lo=NAN))),
    (ESHAPE, "bins must be in 1..1024", (dict(bins=0), dict(bins=-1), dict(bins=1025))),
    (EINVAL, "bad histogram parameters", (dict(md=0.0), dict(md=-1.0), dict(md=NAN), dict(bw=0.0), dict(bw=NAN), dict(floor=-1))),
    (ESHAPE, "too many zones", (dict(b=1 << 16, z=1 << 15),)),
)


def check_shared_refusals(entry, call):
    """`call(**kw)` -> (return code, last error): `entry` called with valid arguments on dummy non-null pointers, except for `kw` (pred, hp,
    wp, h, w, b, interp, lo, hi, rect, mask, raw, z, md, bins, bw, floor): every case fails a check before anything is dereferenced."""
    for code, text, cases in TABLE:
        for kw in cases:
            rc, msg = call(**kw)
            assert rc == code and f"{entry}: {text}" in msg, (entry, kw, rc, msg)
    # the order of the kinds: a null pointer before a dimension before the sizes before the range before the histogram before B * Z
    assert f"{entry}: null pointer" in call(pred=0, b=0)[1] and "non-positive" in call(b=0, hp=4)[1]
    assert "sizes differ" in call(hp=4, lo=2.0, hi=1.0)[1] and "empty depth range" in call(lo=2.0, hi=1.0, bins=0)[1]
    assert "bins must be" in call(bins=0, md=0.0)[1] and "bad histogram" in call(md=0.0, b=1 << 16, z=1 << 15)[1]
