"""The conv epilogue in the scaled domain stores the same bits as the unscaled sequence (CPU, numpy).

The f16x3 kernels leave their K loops with accumulators acc1 + acc2 * 2^-11 = o * 2^-8.  The unscaled epilogue multiplies by 2^8,
adds the bias, decodes an H16 residual to x, applies the activation and multiplies by 2^-8 again to encode an H16 output.  The
scaled epilogue (csrc/conv_common.h, conv_epilogue_scaled) drops every one of those multiplications: bias * 2^-8, residual decoded
without the unscale, LeakyReLU as max(o, 0.1 o), h16_encode4_scaled, and one * 2^8 in front of an fp32 store.  Both sequences are
replayed here operation by operation in float32 / float16 with the rounding of the device (round to nearest even, fp16
conversions that saturate at +-65504 like MODE.FP16_OVFL, subnormals kept), and their (hi, lo) halves or float32 results are
compared bit for bit, NaN, -0 and inf included.

A multiplication by a power of two is exact unless its result is an fp32 subnormal.  So the only inputs left out are those where a
value of the scaled sequence - x * 2^-8 for a bias, an fp32 residual, a sum or 0.1 times a sum x - is a nonzero fp32 subnormal
(|x| < 2^-118 = 3e-36); `_scaled_subnormal` marks them, the random and edge sets below contain none, and a last test shows that
the exclusion is needed (such an input does differ) so the mask is not vacuous.  NaNs compare as NaNs: which payload an operation
hands on is the host library's business here, the device quiets it either way."""
import itertools

import numpy as np
import pytest

F32, F16 = np.float32, np.float16
A, INV_A, INV_LO, LO = F32(1 / 256), F32(256), F32(1 / 2048), F32(2048)
TENTH = F32(0.1)
ACTS = ("linear", "leaky", "relu")
RES_NONE, RES_AFTER, RES_BEFORE = 0, 1, 2
TINY = np.finfo(F32).tiny                     # 2^-126


def _f16_sat(v):
    """float32 -> float16, round to nearest even; a finite value beyond the range saturates at +-65504, inf and NaN pass"""
    with np.errstate(over="ignore", invalid="ignore"):
        h = v.astype(F16)
    over = np.isfinite(v) & np.isinf(h)
    return np.where(over, np.copysign(F16(65504), v.astype(F16)), h)


def _encode(xs):
    """(hi, lo) of a value that is already x * 2^-8"""
    with np.errstate(invalid="ignore", over="ignore"):
        hi = _f16_sat(xs)
        lo = _f16_sat((xs - hi.astype(F32)) * LO)
    return hi, lo


def _act_unscaled(name, o):
    with np.errstate(invalid="ignore"):
        if name == "leaky":
            return np.where(o > 0, o, o * TENTH)
        if name == "relu":
            return np.where(o > 0, o, F32(0))
    return o


def _act_scaled(name, o):
    with np.errstate(invalid="ignore"):
        if name == "leaky":
            return np.fmax(o, o * TENTH)      # v_max_f32: a NaN only where both operands are NaN, -0 where both are -0
        if name == "relu":
            return np.where(o > 0, o, F32(0))
    return o


def _unscaled(acc1, acc2, bias, res, res_h16, act, res_mode, y_h16):
    """today's sequence; res: (hi, lo) float16 arrays where res_h16, else a float32 array"""
    with np.errstate(invalid="ignore", over="ignore"):
        o = (acc1 + acc2 * INV_LO) * INV_A                         # 1. recombine
        o = o + bias                                               # 2. bias
        rs = None
        if res_mode:                                               # 3. residual decode
            rs = (res[0].astype(F32) + res[1].astype(F32) * INV_LO) * INV_A if res_h16 else res
        if res_mode == RES_BEFORE:                                 # 4. residual add before ...
            o = o + rs
        o = _act_unscaled(act, o)                                  # 5. activation
        if res_mode == RES_AFTER:                                  # 4. ... or after it
            o = o + rs
        return _encode(o * A) if y_h16 else o                      # 6. H16 encode or fp32 store


def _scaled(acc1, acc2, bias, res, res_h16, act, res_mode, y_h16, stages=None):
    with np.errstate(invalid="ignore", over="ignore"):
        o = acc1 + acc2 * INV_LO
        bs = bias * A
        o = o + bs
        seen = [bs, o]
        rs = None
        if res_mode:
            rs = res[0].astype(F32) + res[1].astype(F32) * INV_LO if res_h16 else res * A
            seen.append(rs)
        if res_mode == RES_BEFORE:
            o = o + rs
            seen.append(o)
        if act == "leaky":
            seen.append(o * TENTH)
        o = _act_scaled(act, o)
        if res_mode == RES_AFTER:
            o = o + rs
            seen.append(o)
        if stages is not None:
            stages.extend(seen)
        return _encode(o) if y_h16 else o * INV_A


def _scaled_subnormal(*args):
    """inputs for which some value of the scaled sequence is a nonzero fp32 subnormal: the one class the equality leaves out"""
    stages = []
    _scaled(*args, stages=stages)
    bad = np.zeros(stages[0].shape, bool)
    for s in stages:
        bad |= (s != 0) & (np.abs(s) < TINY)
    return bad


def _bits(v):
    """bit pattern with every NaN mapped to one pattern"""
    u = v.view(np.uint16 if v.dtype == F16 else np.uint32).copy()
    u[np.isnan(v)] = 0x7FFF if v.dtype == F16 else 0x7FFFFFFF
    return u


def _same(a, b):
    if isinstance(a, tuple):
        return np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1]))
    return np.array_equal(_bits(a), _bits(b))


def _signed_log_uniform(rng, n, lo, hi):
    return (np.exp(rng.uniform(np.log(lo), np.log(hi), n)) * rng.choice([-1.0, 1.0], n)).astype(F32)


def _accumulators(rng, x):
    """(acc1, acc2) of a K loop whose recombined value is about x * 2^-8: the cross-term sum carries 2^11 times its weight"""
    acc2 = (x * A * rng.uniform(-1, 1, x.shape) * 8).astype(F32)
    acc1 = (x * A - acc2 * INV_LO).astype(F32)
    return acc1, acc2


def _value_sets():
    """name -> (output pre-images x, bias, residual values): float32 arrays of one length per set"""
    rng = np.random.RandomState(5)
    n = 20000
    sets = {}
    sets["random 1e-4..1e4"] = (_signed_log_uniform(rng, n, 1e-4, 1e4), _signed_log_uniform(rng, n, 1e-4, 1e1), _signed_log_uniform(rng, n, 1e-4, 1e4))
    # |x| < 0.016: x * 2^-8 < 6.1e-5, the hi half is an fp16 subnormal or the lo half is
    sets["subnormal lo half"] = (_signed_log_uniform(rng, n, 1e-4, 0.016), _signed_log_uniform(rng, n, 1e-5, 1e-3), _signed_log_uniform(rng, n, 1e-4, 0.016))
    # the saturation guard: 65504 * 256 = 1.677e7, values on both sides of it
    top = 65504.0 * 256
    sets["saturation guard"] = ((rng.uniform(0.97, 1.03, n) * top * rng.choice([-1.0, 1.0], n)).astype(F32), _signed_log_uniform(rng, n, 1e-2, 1e3),
                                (rng.uniform(-1.0, 1.0, n) * 0.05 * top).astype(F32))
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 10.0, -10.0, 65504.0 * 256, -65504.0 * 256], F32)
    sx, sb, sr = (np.array(v, F32) for v in zip(*itertools.product(special, [F32(0), F32(-0.0), F32(0.5)], special)))
    sets["+-0, +-inf, NaN"] = (sx, sb, sr)
    return sets


def _operands(name, x, bias, r):
    rng = np.random.RandomState(len(name))
    if name == "+-0, +-inf, NaN":
        acc1, acc2 = (x * A).astype(F32), np.zeros_like(x)       # the special value itself leaves the K loop
    else:
        acc1, acc2 = _accumulators(rng, x)
    with np.errstate(invalid="ignore", over="ignore"):
        r_h16 = _encode(r * A)                                     # an H16 residual is what an earlier layer encoded
    return acc1, acc2, r_h16


@pytest.mark.parametrize("y_h16", [True, False], ids=["H16 out", "F32 out"])
@pytest.mark.parametrize("res_h16", [True, False], ids=["H16 res", "F32 res"])
@pytest.mark.parametrize("act", ACTS)
def test_scaled_epilogue_stores_the_same_bits(act, res_h16, y_h16):
    for name, (x, bias, r) in _value_sets().items():
        acc1, acc2, r_h16 = _operands(name, x, bias, r)
        res = r_h16 if res_h16 else r
        for res_mode in (RES_NONE, RES_AFTER, RES_BEFORE):
            if res_mode == RES_NONE and not res_h16:
                continue                                           # no residual: one of the two formats is enough
            args = (acc1, acc2, bias, res, res_h16, act, res_mode, y_h16)
            assert not _scaled_subnormal(*args).any(), (name, "the input sets hold no value the equality leaves out")
            assert _same(_unscaled(*args), _scaled(*args)), (name, act, res_mode)


def test_special_values_keep_their_kind():
    """-0 stays -0 through linear and LeakyReLU, ReLU maps it (and a NaN) to +0, infinities keep their sign, a NaN stays one"""
    x = np.array([-0.0, 0.0, np.inf, -np.inf, np.nan], F32)
    z = np.full_like(x, -0.0)                                      # (a +0 cross-term sum or bias would turn the -0 into +0 in both sequences)
    for act, want in (("linear", [-0.0, 0.0, np.inf, -np.inf, np.nan]), ("leaky", [-0.0, 0.0, np.inf, -np.inf, np.nan]),
                      ("relu", [0.0, 0.0, np.inf, 0.0, 0.0])):
        for seq in (_unscaled, _scaled):
            got = seq(x * A, z, np.full_like(x, -0.0), None, False, act, RES_NONE, False)
            assert np.array_equal(_bits(got), _bits(np.array(want, F32))), (act, seq.__name__, got)


def test_the_exclusion_is_needed_and_narrow():
    """a bias whose 2^-8 multiple is an fp32 subnormal loses bits in the scaled sequence: that input is marked, and does differ;
    one binade up nothing is marked and nothing differs"""
    z = np.zeros(1, F32)
    tiny_bias = np.nextafter(np.array([TINY * 96], F32), F32(1))   # odd last mantissa bit, 2^-8 of it is below 2^-126: the shift rounds
    args = (z, z, tiny_bias, None, False, "linear", RES_NONE, False)
    assert _scaled_subnormal(*args).all()
    assert not _same(_unscaled(*args), _scaled(*args))
    ok_bias = np.nextafter(np.array([TINY * 256], F32), F32(1))
    args = (z, z, ok_bias, None, False, "linear", RES_NONE, False)
    assert not _scaled_subnormal(*args).any()
    assert _same(_unscaled(*args), _scaled(*args))
