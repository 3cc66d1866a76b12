"""Accuracy of the f64-FFT path measured against a high-precision reference (host only; the tests are
tests/test_fft_accuracy.py and tests/test_fft_accuracy_gpu.py).

* ``forward_as_torus_ld`` / ``forward_as_integer_ld``: the transforms of oracle/fft_oracle.py in ``np.longdouble``
  (x87 extended, a 64-bit mantissa: 2^11 finer than f64).  Twisting factors and twiddles come from cosl / sinl of exactly
  reduced indices (``cis_ld``: the index is taken mod the period in integers and folded into (-pi, pi]); the transform
  is an iterative radix-2 with one table per stage, so N = 2^18 takes seconds.  ``dft_direct_ld`` is the O(m^2)
  definition for validating it.
* ``error_stats`` / ``within_margin``: the criterion.  No absolute tolerance: for identical inputs the error of the
  numpy restatement and the error of the result under test are both taken against the high-precision (or exact integer)
  answer, as rms and max normalised by the rms of the true result, and the result under test may be at most ``MARGIN``
  times worse in either.  Why 4: another radix split and twiddles derived by a few products change the error constant by
  a small factor, not the order; it is the margin the PBS noise tests use.
* ``forward_as_torus_f64``: an f64 radix-2 restatement with injectable twisting factors and stage tables, for the
  mutants that show the criterion's power.
* ``exact_products`` / ``exact_ext_product``: the exact external product in Z_2^64[X]/(X^N + 1).
"""
import numpy as np

import fft_oracle as F

LD = np.longdouble
CLD = np.clongdouble
MARGIN = 4.0
P = 0xFFFFFFFF00000001

assert np.finfo(LD).nmant >= 63, "np.longdouble has no 64-bit mantissa on this platform"

# pi to 64 bits: the double nearest pi plus the double nearest the remainder (1.2246e-16), summed in long double
PI_LD = LD(3.141592653589793) + LD(1.2246467991473532e-16)


def cis_ld(num, den: int, sign: int = 1) -> np.ndarray:
    """exp(sign 2 pi i num / den) in long double; num an integer array of any size (reduced mod den exactly)."""
    k = np.asarray(num, dtype=np.int64) % den
    k = np.where(2 * k > den, k - den, k)
    ang = (2 * PI_LD) * k.astype(LD) / LD(den)
    out = np.empty(k.shape, CLD)
    out.real = np.cos(ang)
    out.imag = sign * np.sin(ang)
    return out


def _bitrev(m: int) -> np.ndarray:
    bits = m.bit_length() - 1
    r = np.arange(m)
    out = np.zeros(m, np.int64)
    for b in range(bits):
        out |= ((r >> b) & 1) << (bits - 1 - b)
    return out


def stage_tables_ld(m: int, sign: int = -1) -> list:
    """One table per radix-2 stage: stage L = 2, 4, .., m holds exp(sign 2 pi i k / L), k < L / 2."""
    out, L = [], 2
    while L <= m:
        out.append(cis_ld(np.arange(L // 2), L, sign))
        L *= 2
    return out


def _radix2(z, tables, dif=False):
    """Radix-2 over the last axis, in the precision of z and the tables: decimation in time (bit-reversed input,
    stages L = 2 .. m), or with ``dif`` decimation in frequency (stages L = m .. 2 on (a - b) w, bit-reversed output),
    where each entry of the first stage's table meets exactly one butterfly."""
    m = z.shape[-1]
    a = z if dif else z[..., _bitrev(m)]
    lead = a.shape[:-1]
    for tw in (tables[::-1] if dif else tables):
        half = tw.shape[0]
        a = a.reshape(lead + (m // (2 * half), 2 * half))
        if dif:
            u, v = a[..., :half], a[..., half:]
            a = np.concatenate([u + v, (u - v) * tw], axis=-1)
        else:
            u, v = a[..., :half], a[..., half:] * tw
            a = np.concatenate([u + v, u - v], axis=-1)
    a = a.reshape(lead + (m,))
    return a[..., _bitrev(m)] if dif else a


def fft_ld(z, inverse: bool = False) -> np.ndarray:
    z = np.asarray(z, dtype=CLD)
    m = z.shape[-1]
    out = _radix2(z, stage_tables_ld(m, 1 if inverse else -1))
    return out / LD(m) if inverse else out


def dft_direct_ld(z) -> np.ndarray:
    """The definition, sum_j z_j exp(-2 pi i j k / m), every factor from cosl / sinl of (j k) mod m."""
    z = np.asarray(z, dtype=CLD)
    m = z.shape[-1]
    j = np.arange(m, dtype=np.int64)
    w = cis_ld(np.outer(j, j), m, -1)
    return z @ w


def twisties_ld(m: int) -> np.ndarray:
    """exp(i pi j / (2 m)) = exp(2 pi i j / (4 m)), j < m."""
    return cis_ld(np.arange(m), 4 * m, 1)


def _signed_ld(x) -> np.ndarray:
    return np.asarray(x, dtype=np.uint64).view(np.int64).astype(LD)   # exact: 64-bit mantissa


def _fold_ld(x, scale) -> np.ndarray:
    m = x.shape[-1] // 2
    z = np.empty(x.shape[:-1] + (m,), CLD)
    z.real = _signed_ld(x[..., :m]) * scale
    z.imag = _signed_ld(x[..., m:]) * scale
    return z * twisties_ld(m)


def forward_as_torus_ld(std) -> np.ndarray:
    return fft_ld(_fold_ld(np.asarray(std, dtype=np.uint64), LD(2.0) ** -64))


def forward_as_integer_ld(x) -> np.ndarray:
    return fft_ld(_fold_ld(np.asarray(x, dtype=np.uint64), LD(1.0)))


# ---- the criterion -------------------------------------------------------------------------------------------------
def error_stats(got, true) -> tuple:
    """(rms, max) of |got - true| over every element, normalised by the rms of |true|; in long double."""
    got = np.asarray(got)
    cplx = np.iscomplexobj(got) or np.iscomplexobj(true)
    d = np.abs(got.astype(CLD if cplx else LD) - np.asarray(true).astype(CLD if cplx else LD))
    scale = np.sqrt(np.mean(np.abs(np.asarray(true).astype(CLD if cplx else LD)) ** 2))
    return float(np.sqrt(np.mean(d ** 2)) / scale), float(d.max() / scale)


def word_error_stats(got, true) -> tuple:
    """The same for torus words: the signed 64-bit distance, normalised by the rms of the true signed words."""
    d = F.signed_diff(got, true).astype(LD)
    scale = np.sqrt(np.mean(_signed_ld(true) ** 2))
    return float(np.sqrt(np.mean(d ** 2)) / scale), float(d.max() / scale)


def word_error_bits(got, true) -> tuple:
    """(log2 rms, log2 max) of the signed distance in units of 2^-64."""
    d = F.signed_diff(got, true)
    return float(np.log2(max(np.sqrt(np.mean(d ** 2)), 1.0))), float(np.log2(max(d.max(), 1.0)))


def ratios(test, ref) -> tuple:
    return test[0] / ref[0], test[1] / ref[1]


def within_margin(test, ref, margin: float = MARGIN) -> bool:
    """test = (rms, max) of the result under test, ref = (rms, max) of the numpy restatement."""
    return test[0] <= margin * ref[0] and test[1] <= margin * ref[1]


def old_criterion(got, want) -> bool:
    """The bar of tests/test_fft_gpu.py and tests/test_fft_generic_gpu.py: within 1e-13 max|want| of np.fft."""
    return bool(np.abs(got - want).max() / np.abs(want).max() < 1e-13)


# ---- an f64 restatement with injectable tables (the mutants) -------------------------------------------------------
def twisties_f64(m: int) -> np.ndarray:
    return twisties_ld(m).astype(np.complex128)


def stage_tables_f64(m: int) -> list:
    return [t.astype(np.complex128) for t in stage_tables_ld(m, -1)]


def forward_as_torus_f64(std, twist=None, tables=None, dif=False) -> np.ndarray:
    """forward_as_torus in f64 through the radix-2 above; correctly rounded twisting factors and tables by default."""
    std = np.asarray(std, dtype=np.uint64)
    m = std.shape[-1] // 2
    twist = twisties_f64(m) if twist is None else twist
    tables = stage_tables_f64(m) if tables is None else tables
    s = lambda a: a.view(np.int64).astype(np.float64)
    z = (s(std[..., :m]) + 1j * s(std[..., m:])) * 2.0 ** -64
    return _radix2(z * twist, tables, dif)


# ---- the exact external product ------------------------------------------------------------------------------------
def _signed_mod_p(u):
    """two's complement u64 (small signed values) -> residues mod p"""
    s = u.view(np.int64)
    return np.where(s < 0, (np.uint64(P) - (np.uint64(0) - u)), u).astype(np.uint64)


def exact_products(oracle, a, d, base_log):
    """a (..., N) u64 times d (..., N) small signed digits (two's complement), negacyclic mod 2^64, exact.  Through
    the oracle's Solinas transform with 32-bit limbs of a when N 2^32 2^(B-1) < p / 2, by rotation sums otherwise."""
    n = a.shape[-1]
    if n.bit_length() - 1 + base_log < 31:
        plan = oracle.Plan.try_new(n, P)
        flat_a = np.ascontiguousarray(a.reshape(-1, n))
        d_hat = plan.fwd(np.ascontiguousarray(_signed_mod_p(d.reshape(-1, n))), threads=16)
        out = np.zeros_like(flat_a)
        with np.errstate(over="ignore"):
            for t in range(2):
                limb = (flat_a >> np.uint64(32 * t)) & np.uint64(0xFFFFFFFF)
                v = plan.inv(plan.mul_assign_normalize(plan.fwd(limb, threads=16), d_hat), threads=16)
                v = np.where(v > np.uint64(P // 2), v - np.uint64(P), v)
                out += v << np.uint64(32 * t)
        return out.reshape(a.shape)
    out = np.zeros(a.reshape(-1, n).shape, np.uint64)
    fa, fd = a.reshape(-1, n), d.reshape(-1, n)
    with np.errstate(over="ignore"):
        for i in range(fa.shape[0]):
            for j in range(n):
                if fd[i, j]:
                    out[i] += fd[i, j] * np.concatenate([np.uint64(0) - fa[i, n - j:], fa[i, : n - j]])
    return out.reshape(a.shape)


def exact_ext_product(oracle, glwe, ggsw, base_log, level):
    """sum over levels li and rows r of digit_li(glwe[r]) x ggsw[li][r][c], exact in Z_2^64[X]/(X^N + 1)"""
    kp1, n = glwe.shape
    terms = F.decompose(glwe, base_log, level)  # least significant level first
    a = np.stack([np.broadcast_to(ggsw[li, r], (kp1, n)) for li in range(level) for r in range(kp1)])
    d = np.stack([np.broadcast_to(terms[li][r], (kp1, n)) for li in range(level) for r in range(kp1)])
    prods = exact_products(oracle, np.ascontiguousarray(a), np.ascontiguousarray(d), base_log)
    with np.errstate(over="ignore"):
        return prods.sum(axis=0, dtype=np.uint64)
