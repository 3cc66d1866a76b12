"""The f64 <-> torus conversions of the f64-FFT path on exact rationals, host models of the device copies, and the
corner corpus every conversion test feeds (host only).

Reference paths are relative to tfhe/src/core_crypto.

* ``ref_from_torus`` (commons/math/torus/mod.rs:72-78) and ``ref_s64_to_f64`` (the `into_signed().cast_into()` of
  fft_impl/fft64/math/fft/mod.rs:227-269): on ``fractions.Fraction`` and Python integers, no float arithmetic, written
  from the reference's text and independent of oracle/.
* ``model_s64_to_f64`` / ``model_torus_words`` / ``model_add_torus``: RESTATEMENTS in Python of the device functions of
  csrc/fft64_device.hpp (``s64_to_f64``, ``torus_words`` / ``from_torus_scaled``, ``add_torus``), line by line from
  the header with ``math.floor`` and float operations (a Python float is the device's f64; every product here is by a
  power of two and every FMA of the header has an exact result, so plain float operations give the same bits).
  ``hw_fract`` restates the hardware fraction instruction: t - floor(t) rounded to nearest, clamped below 1.
* ``expected_backward`` / ``add_torus_class`` / ``expected_add_torus``: the contract of the header in numbers, on
  rationals.  The tests assert the device against these, and the models against these on the CPU.
* ``MUTANTS``: one-off wrong versions of the models; tests/test_torus_corners.py asserts the corpus tells each
  from the true function.
* ``forward_words`` / ``backward_values`` / ``add_torus_values``: the corpora.

Which device copy is reached by which test (tests/test_torus_corners_gpu.py, every one at N = 2048, 32, 64, 128, 32768):

* ``test_forward_conversion_exact``: ``s64_to_f64`` x 2^-64 in ``fwd_torus_kernel`` (fft64_pbs.hip, N = 2048) and
  ``TorusSrc`` (fft64_generic.hip).
* ``test_backward_conversion_exact``: ``from_torus_scaled`` in ``bwd_torus_kernel`` (N = 2048) and ``TorusSink``
  (generic), stored and added.
* ``test_add_torus_contract``: ``add_torus`` in the one-wave external product's sink (``ext_product_add``,
  fft64_pbs.hip) and ``AccSink`` (generic); its digit-1 input also passes ``s64_to_f64`` of ``GlweDigitSrc``.

fft64_multi_bit.hip has its own call site of ``add_torus`` (the multi-bit blind rotation's accumulation), but the
function is the shared one of fft64_device.hpp that the external product pins here; no entry point reaches that call
site with a chosen double.

How one coefficient sees an exactly known double: a polynomial that is x at coefficient 0 (N/2) and zero elsewhere
transforms to the constant f64(i64(x)) 2^-64 in the real (imaginary) part of every frequency, and a constant spectrum
(t_re, t_im) inverts to t_re at coefficient 0, t_im at coefficient N/2 and zero elsewhere; sums of equal doubles over
a power-of-two count, differences of equal doubles and products with the twiddle 1 are exact, so the transform adds
no rounding (the tests assert the zero words, which proves it on each engine).
"""
import math
import struct
from fractions import Fraction

import numpy as np

M64 = 1 << 64
HALF = Fraction(1, 2)


# ---- rounding on rationals -----------------------------------------------------------------------------------------
def round_half_away(q) -> int:
    """f64::round: nearest integer, ties away from zero."""
    q = Fraction(q)
    f = math.floor(q)
    d = q - f
    if d > HALF or (d == HALF and q > 0):
        return f + 1
    return f


def round_half_even(q) -> int:
    """rint under the default rounding mode: nearest integer, ties to even."""
    q = Fraction(q)
    f = math.floor(q)
    d = q - f
    if d > HALF or (d == HALF and f % 2 == 1):
        return f + 1
    return f


# ---- the reference on exact numbers --------------------------------------------------------------------------------
def ref_from_torus(t: float) -> int:
    """Scalar::from_torus for u64 / f64: fract = t - round(t) (exact in f64 for every finite t), round(fract 2^64)
    (exact), `as i64` (saturating), `as u64`."""
    x = Fraction(t)
    fract = x - round_half_away(x)
    v = round_half_away(fract * M64)
    v = max(-(1 << 63), min((1 << 63) - 1, v))
    return v % M64


def ref_s64_to_f64(x: int) -> float:
    """`x as i64 as f64`: Python's int -> float conversion is correctly rounded (nearest, ties to even)."""
    x %= M64
    return float(x - M64 if x >> 63 else x)


def scaled(t: float) -> Fraction:
    """t 2^64, exact."""
    return Fraction(t) * M64


def is_half(t: float) -> bool:
    """t 2^64 is an exact half-integer (the two roundings differ there)."""
    return scaled(t).denominator == 2


def fract_is_plus_half(t: float) -> bool:
    """The reference's fract = t - round(t) is +1/2 (t = -(n + 1/2), n >= 0): it saturates to i64::MAX."""
    x = Fraction(t)
    return x - round_half_away(x) == HALF


def expected_backward(t: float) -> int:
    """from_torus_scaled(t 2^64): round-half-even of t 2^64, wrapped mod 2^64.  Equal to ``ref_from_torus`` except
    on exact half-integers of t 2^64 (the nearest even word) and on fract = +1/2 (2^63, not i64::MAX)."""
    return round_half_even(scaled(t)) % M64


# ---- the contract of add_torus in numbers --------------------------------------------------------------------------
TINY = 2.0 ** -12   # below it a non-negative t has bits under 2^-64


def add_torus_class(t: float) -> str:
    """The class of t under add_torus (fft64_device.hpp):

    * ``exact``      t >= 2^-12, or t >= 0 with t 2^64 an integer, or t <= -1/2 with fract != 1/2, or -1/2 < t < 0
                     with t a multiple of 2^-53 (1 + t is a double): the reference's word.
    * ``plus_half``  t = -(n + 1/2): 2^63 where the reference saturates to 2^63 - 1.
    * ``round``      0 < t < 2^-12 with t 2^64 no integer: round-half-even of t 2^64 (the reference rounds half away:
                     one unit apart on exact halves, equal elsewhere) ...
    * ``carry``      ... except where t 2^64 mod 2^32 >= 2^32 - 1/2: the low word rounds up to 2^32, reads as 0 and the
                     carry into the high word is dropped: exactly 2^32 below the reference.
    * ``neg_small``  -1/2 < t < 0 otherwise: fract(t) = 1 + t is rounded to a double of [1/2, 1] (a multiple of 2^-53),
                     so the word is off by at most 2^10, and by at most 2^11 where 1 + t rounds to 1 and is clamped to
                     1 - 2^-53 (-2^-54 <= t < 0: the word 2^64 - 2^11).
    """
    x = Fraction(t)
    if x >= 0:
        y = x * M64
        if t >= TINY or y.denominator == 1:
            return "exact"
        return "carry" if y % (1 << 32) >= (1 << 32) - HALF else "round"
    if x <= -HALF:
        return "plus_half" if fract_is_plus_half(t) else "exact"
    return "exact" if (x * (1 << 53)).denominator == 1 else "neg_small"


def expected_add_torus(t: float):
    """(word, slack): the device's from_torus(t) inside add_torus is within `slack` of `word`; slack 0 is bit-exact."""
    cls = add_torus_class(t)
    ref = ref_from_torus(t)
    if cls == "exact":
        return ref, 0
    if cls == "plus_half":
        return 1 << 63, 0
    if cls == "round":
        return round_half_even(scaled(t)) % M64, 0
    if cls == "carry":
        return (ref - (1 << 32)) % M64, 0
    return ref, (1 << 11) if Fraction(t) >= -Fraction(1, 1 << 54) else (1 << 10)


def word_distance(a: int, b: int) -> int:
    d = (a - b) % M64
    return min(d, M64 - d)


# ---- host models of the device functions (restatements of csrc/fft64_device.hpp) -----------------------------------
def _bits(d: float) -> int:
    return struct.unpack("<q", struct.pack("<d", d))[0]


def _rint(y: float) -> float:
    return y if abs(y) >= 2.0 ** 52 else math.copysign(float(round(y)), y)   # round(): ties to even


def model_s64_to_f64(x: int) -> float:
    """(double)(int64_t)x"""
    x %= M64
    return float(x - M64 if x >> 63 else x)


def model_torus_words(y: float) -> int:
    """torus_words / from_torus_scaled of y = t 2^64."""
    r = _rint(y)
    z = r - _rint(r * 2.0 ** -64) * 2.0 ** 64
    hi = float(math.floor(z * 2.0 ** -32))
    lo = z - hi * 2.0 ** 32
    h = _bits(hi + 1.5 * 2.0 ** 52) & 0xFFFFFFFF
    l = _bits(lo + 2.0 ** 52) & 0xFFFFFFFF
    return (h << 32) | l


def hw_fract(t: float) -> float:
    """The hardware fraction: t - floor(t) rounded to nearest, clamped to the largest double below 1."""
    f = t - float(math.floor(t))
    return min(f, 1.0 - 2.0 ** -53)


def model_add_torus(acc: int, t: float) -> int:
    """add_torus(acc, t)."""
    f = hw_fract(t)
    s = f * 2.0 ** 32
    h = int(s) & 0xFFFFFFFF
    l = _bits(hw_fract(s) * 2.0 ** 32 + 2.0 ** 52) & 0xFFFFFFFF
    alo, ahi = acc & 0xFFFFFFFF, acc >> 32
    nlo = (alo + l) & 0xFFFFFFFF
    nhi = (ahi + h + (1 if nlo < alo else 0)) & 0xFFFFFFFF
    return (nhi << 32) | nlo


# ---- one-off mutants -----------------------------------------------------------------------------------------------
def _mut_words(y, rnd=_rint, saturate=False):
    r = rnd(y)
    z = int(r - _rint(r * 2.0 ** -64) * 2.0 ** 64)
    if saturate:
        z = min(z, (1 << 63) - 1)
    return z % M64


def _trunc(y):
    return float(math.trunc(y))


def _half_away(y):
    return y if abs(y) >= 2.0 ** 52 else float(round_half_away(Fraction(y)))


def _mut_add(acc, t, *, trunc_low=False, carry_word_up=False, keep_round_carry=False):
    f = hw_fract(t)
    s = f * 2.0 ** 32
    h = int(s) & 0xFFFFFFFF
    low = hw_fract(s) * 2.0 ** 32
    lw = int(low) if trunc_low else _bits(low + 2.0 ** 52) & 0x1FFFFFFFF
    if keep_round_carry:
        h = (h + (lw >> 32)) & 0xFFFFFFFF
    l = lw & 0xFFFFFFFF
    alo, ahi = acc & 0xFFFFFFFF, acc >> 32
    nlo = (alo + l) & 0xFFFFFFFF
    carry = 0 if carry_word_up else (1 if nlo < alo else 0)
    return (((ahi + h + carry) & 0xFFFFFFFF) << 32) | nlo


# name -> (kind, function); kind names the model it replaces
MUTANTS = {
    "words_truncate": ("words", lambda y: _mut_words(y, rnd=_trunc)),
    "words_half_away": ("words", lambda y: _mut_words(y, rnd=_half_away)),
    "words_saturate": ("words", lambda y: _mut_words(y, saturate=True)),
    "add_truncate_low_word": ("add", lambda acc, t: _mut_add(acc, t, trunc_low=True)),
    "add_carry_dropped_one_word_higher": ("add", lambda acc, t: _mut_add(acc, t, carry_word_up=True)),
    "add_rounding_carry_kept": ("add", lambda acc, t: _mut_add(acc, t, keep_round_carry=True)),
    "forward_unsigned_cast": ("forward", lambda x: float(x % M64)),   # (double)(uint64_t)x
}


# ---- corpora -------------------------------------------------------------------------------------------------------
ACCUMULATORS = (0, M64 - 1, 1 << 63)


def forward_words(n_random=300, seed=0x746F72) -> list:
    """u64 words for s64_to_f64: the exact range, ties to even above 2^53, both signs' ends, random words."""
    fixed = [0, 1, 1 << 53, (1 << 53) + 1, (1 << 53) + 3, (1 << 54) + 2, (1 << 54) + 6, (1 << 63) - 1, 1 << 63,
             (1 << 63) + 1, M64 - 1, M64 - (1 << 53) - 1,
             # the same ties on the negative side, and words whose top set bit walks down
             M64 - (1 << 53) - 3, M64 - (1 << 54) - 2, M64 - (1 << 54) - 6, (1 << 63) - (1 << 9) - 1, (1 << 62) + 255]
    g = np.random.default_rng(seed)
    rnd = [int(v) for v in g.integers(0, M64, size=n_random, dtype=np.uint64)]
    # random words of every bit length: a uniform word almost never has fewer than 53 significant bits
    short = [int(v) >> int(s) for v, s in zip(g.integers(0, M64, size=64, dtype=np.uint64), range(64))]
    return fixed + rnd + short


def _pm(vals):
    out = []
    for v in vals:
        out += [v, -v]
    return out


def backward_values(n_random=200, seed=0x746F73) -> list:
    """Torus values t (doubles) for from_torus: zero, the first words, exact halves of t 2^64 (odd and even floor),
    fract = +-1/2, integers, large magnitudes with a fraction, bits below 2^-64, halves near 2^52 where a double's
    spacing is 2^-64 / 2 ... and random values with exponents -70 .. 40."""
    u = 2.0 ** -64
    vals = [0.0] + _pm([u, 2.0 ** -65, 1.5 * u, 2.5 * u, 0.5, 1.0])
    vals += [0.5 - 2.0 ** -54, -(0.5 - 2.0 ** -54), 0.25, 3.25, -7.75, 2.0 ** 20 + 0.375, -(2.0 ** 30) + 2.0 ** -20,
             1.0 - 2.0 ** -53, -(2.0 ** -70), -(2.0 ** -60), 1.5, -1.5, 2.5, -2.5, 0.75, -0.75, 2.0 ** 40 + 0.5,
             -(2.0 ** 40) - 0.5, 0.5 + 2.0 ** -53, -0.5 - 2.0 ** -53, 0.5 - u, -0.5 + u]
    for k in ((1 << 52) - 2, (1 << 52) - 1, (1 << 51) + 1, (1 << 51) + 2, 3, 4):
        vals += _pm([(k + 0.5) * u])
    g = np.random.default_rng(seed)
    exps = g.integers(-70, 41, size=n_random)
    mant = 1.0 + g.random(n_random)
    sign = np.where(g.random(n_random) < 0.5, -1.0, 1.0)
    vals += [float(s * m * 2.0 ** int(e)) for s, m, e in zip(sign, mant, exps)]
    return vals


def add_torus_values(n_random=60, seed=0x746F74) -> list:
    """The backward corpus plus the corners of add_torus's own classes, and values just outside each."""
    u = 2.0 ** -64
    up = lambda v: math.nextafter(v, math.inf)
    dn = lambda v: math.nextafter(v, -math.inf)
    vals = backward_values(n_random, seed)
    # -0.3 and neighbours whose last mantissa bit is set (1 + t needs one bit more than a double of [1/2, 1) has)
    vals += [-0.3, up(-0.3), dn(-0.3), up(up(-0.3)), -0.1, -0.2, dn(-0.2), -0.4999, -(2.0 ** -30), up(-(2.0 ** -30))]
    # exact members of (-1/2, 0): multiples of 2^-53
    vals += [-0.25, -0.375, -(2.0 ** -53), -3 * 2.0 ** -53, -0.5 + 2.0 ** -53, -(2.0 ** -20)]
    # the edge of the class at -1/2 and the clamp at -2^-54
    vals += [-0.5, dn(-0.5), up(-0.5), -0.5 + 2.0 ** -54, -(2.0 ** -54), up(-(2.0 ** -54)), dn(-(2.0 ** -54)),
             -(2.0 ** -55), -3 * 2.0 ** -55, -(2.0 ** -100)]
    # the dropped carry: t 2^64 mod 2^32 in [2^32 - 1/2, 2^32), and just outside (exactly 2^32 - 3/4, integers)
    vals += [2.0 ** -32 - 2.0 ** -66, 2.0 ** -32 - 2.0 ** -65, 2.0 ** -32 - 3 * 2.0 ** -66, 2.0 ** -32 - u, 2.0 ** -32,
             5 * 2.0 ** -32 - 2.0 ** -66, 2.0 ** -13 - 2.0 ** -66, 2.0 ** -13 - 2.0 ** -65, 2.0 ** -12 - 2.0 ** -65]
    # the edge of the rounding class at 2^-12: the last value with a half, the first values without
    vals += [TINY, up(TINY), dn(TINY), dn(dn(TINY)), 2.0 ** -11 - u, 2.0 ** -12 + 2.0 ** -32 - u]
    # a carry out of the low word of the accumulator's add at every accumulator: low words 1 and 2^32 - 1
    vals += [u, (2.0 ** 32 - 1) * u, 2.0 ** -32 + u, 1.0 - u * 2048, 0.5 + u * 2048]
    return vals
