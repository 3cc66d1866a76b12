"""The high-precision reference of tests/fft_accuracy.py validated, and the power of its criterion shown, on the host.

* The long-double radix-2 against the long-double direct DFT for m <= 1024, and against mpmath at 50 digits for m = 16
  (only where mpmath is installed).
* The numpy restatement's own error against it: the scale every GPU measurement is compared with.
* The criterion: the restatement passes against itself with ratio 1, the clean f64 radix-2 restatement passes, and
  mutants the old bar (1e-13 max|want| of np.fft) cannot see are rejected.
"""
import numpy as np
import pytest

import fft_accuracy as A
import fft_oracle as F
import tfhe_helpers as H

EPS_LD = 2.0 ** -64   # half an ulp of the 64-bit mantissa


def _poly(seed, batch, n):
    return H.uniform_u64(H.rng(seed), (batch, n))


@pytest.mark.parametrize("m", [2, 16, 64, 256, 1024])
def test_radix2_matches_direct_dft(m):
    """Both are long-double sums of the same products; each rounds about log2(m) (radix-2) or up to m (direct) times.
    Bound: 16 log2(2m) half-ulps of the rms for the max error -- three roundings per stage (twiddle, product, sum) with
    headroom for a peak above the rms; 2^6 or more below the f64 restatement's error, which is what matters here."""
    g = H.rng(40 + m)
    z = (g.standard_normal((2, m)) + 1j * g.standard_normal((2, m))).astype(A.CLD)
    rms, mx = A.error_stats(A.fft_ld(z), A.dft_direct_ld(z))
    bound = 16 * np.log2(2 * m) * EPS_LD
    print(f"radix-2 vs direct long-double DFT m={m}: rms {rms:.2e} max {mx:.2e} (bound {bound:.2e})")
    assert mx <= bound
    back = A.fft_ld(A.fft_ld(z), inverse=True)
    assert A.error_stats(back, z)[1] <= 2 * bound


def test_reference_matches_mpmath_at_m16():
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    x = _poly(7, 1, 32)[0]
    m = 16
    s = [int(v) - (1 << 64) if int(v) >> 63 else int(v) for v in x]
    want = []
    for k in range(m):
        acc = mp.mpc(0)
        for j in range(m):
            zj = mp.mpc(s[j], s[j + m]) / mp.mpf(2) ** 64
            acc += zj * mp.expjpi(mp.mpf(j) / (2 * m)) * mp.expjpi(mp.mpf(-2 * j * k) / m)
        want.append(acc)
    got = A.forward_as_torus_ld(x)
    scale = float(mp.sqrt(sum(abs(w) ** 2 for w in want) / m))
    err = max(float(abs(mp.mpc(mp.mpf(float(g.real)) + mp.mpf(float(g.real - A.LD(float(g.real)))),
                               mp.mpf(float(g.imag)) + mp.mpf(float(g.imag - A.LD(float(g.imag))))) - w))
              for g, w in zip(got, want))
    print(f"long-double forward_as_torus vs mpmath (50 digits), m=16: max error {err / scale:.2e} of the rms")
    assert err / scale <= 16 * np.log2(2 * m) * EPS_LD


@pytest.mark.parametrize("n", [32, 256, 2048])
def test_numpy_restatement_error_scale(n):
    """The restatement's own error against the long-double spectrum: a few f64 half-ulps (1.1e-16) of the rms."""
    x = _poly(100 + n, 4, n)
    ref = A.error_stats(F.forward_as_torus(x), A.forward_as_torus_ld(x))
    print(f"numpy forward_as_torus N={n}: rms {ref[0]:.2e} max {ref[1]:.2e}")
    assert 2.0 ** -56 < ref[0] < 16 * 2.0 ** -53 and ref[1] < 64 * 2.0 ** -53
    # backward from the long-double spectrum rounded to f64, against the integers it came from
    spec = A.forward_as_torus_ld(x).astype(np.complex128)
    bits = A.word_error_bits(F.backward_as_torus(spec), x)
    print(f"numpy backward_as_torus N={n}: error 2^{bits[0]:.1f} rms 2^{bits[1]:.1f} max (units of 2^-64)")
    assert bits[1] < 16   # 53-bit values of 64-bit words


def _mutants(m, g):
    """name -> (twist, tables) of forward_as_torus_f64 run as a decimation in frequency, where a table entry of the first
    stage is read by one butterfly (a stage table of the decimation in time is shared by every block of its stage)."""
    twist, tables = A.twisties_f64(m), A.stage_tables_f64(m)
    out = {}
    out["twisties with 3e-14 of phase noise"] = (twist * np.exp(1j * 3e-14 * g.standard_normal(m)), tables)
    t = [a.copy() for a in tables]
    t[-1][5] += 1e-12   # the first stage of the decimation in frequency: one butterfly of input-sized values
    out["one twiddle entry off by 1e-12"] = (twist, t)
    t = [a.copy() for a in tables]
    t[-1][5] = np.complex128(np.complex64(t[-1][5]))
    out["one twiddle rounded through float32"] = (twist, t)
    return out


def test_criterion_passes_the_restatements():
    n = 2048
    x = _poly(11, 4, n)
    true = A.forward_as_torus_ld(x)
    ref = A.error_stats(F.forward_as_torus(x), true)
    assert A.ratios(ref, ref) == (1.0, 1.0) and A.within_margin(ref, ref)
    clean = A.error_stats(A.forward_as_torus_f64(x), true)
    print(f"clean f64 radix-2 vs numpy, N={n}: ratios rms {clean[0] / ref[0]:.2f} max {clean[1] / ref[1]:.2f}")
    assert A.within_margin(clean, ref)
    assert A.old_criterion(A.forward_as_torus_f64(x), F.forward_as_torus(x))
    dif = A.error_stats(A.forward_as_torus_f64(x, dif=True), true)
    print(f"clean f64 radix-2 (decimation in frequency) vs numpy: ratios rms {dif[0] / ref[0]:.2f} max {dif[1] / ref[1]:.2f}")
    assert A.within_margin(dif, ref)


@pytest.mark.parametrize("name", ["twisties with 3e-14 of phase noise", "one twiddle entry off by 1e-12",
                                  "one twiddle rounded through float32"])
def test_criterion_rejects_mutant(name):
    """Each mutant fails the 4x criterion.  The first two pass the old bar, 1e-13 max|want|, so the old tests could not
    see them; a float32 twiddle (6e-8 relative) is within reach of the old bar wherever it is placed, so for it only the
    rejection is asserted."""
    n = 2048
    x = _poly(11, 4, n)
    true = A.forward_as_torus_ld(x)
    want = F.forward_as_torus(x)
    ref = A.error_stats(want, true)
    twist, tables = _mutants(n // 2, H.rng(12))[name]
    got = A.forward_as_torus_f64(x, twist, tables, dif=True)
    st = A.error_stats(got, true)
    r = A.ratios(st, ref)
    old = float(np.abs(got - want).max() / np.abs(want).max())
    print(f"{name}: rms {st[0]:.2e} ({r[0]:.0f}x numpy) max {st[1]:.2e} ({r[1]:.0f}x); old bar {old:.2e} of 1e-13")
    assert not A.within_margin(st, ref)
    assert max(r) > 2 * A.MARGIN   # rejected with room, not at the edge
    if "float32" not in name:
        assert A.old_criterion(got, want)


def test_exact_products_agree_between_their_two_paths(oracle):
    """exact_products takes the Solinas transform when N 2^32 2^(B-1) < p / 2 and rotation sums otherwise."""
    g = H.rng(13)
    n = 32
    a = H.uniform_u64(g, (3, n))
    d = g.integers(-(1 << 9), 1 << 9, size=(3, n), dtype=np.int64).astype(np.uint64)
    assert np.array_equal(A.exact_products(oracle, a, d, 10), A.exact_products(oracle, a, d, 40))
