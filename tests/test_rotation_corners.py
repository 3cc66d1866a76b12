"""The modulus switch, the centered body correction and the monomial rotation, pinned on the host: every restatement in
the tree against the big-integer transcription of tests/rotation_corners.py, on that module's corner corpus; the corpus
itself (it reaches its corners, and it tells every one-off mistake from the true function); and the oracle's whole PBS on
a noiseless gadget key, whose result is the LUT times a known monomial.  tests/test_rotation_corners_gpu.py feeds the same
corpus to every device copy."""
import numpy as np
import pytest

import fft_oracle as F
import multi_bit_helpers as MB
import pbs128_helpers as P128
import rotation_corners as R

M64 = R.M64
P = R.P
SIZES = [32, 512, 2048, 8192]
LENGTHS = [1, 7, 40, 131]


def _native_corpus(n):
    words = [w for w, _, _ in R.native_words(n)]
    return words + [0, 1, M64 - 1, 1 << 63, (1 << 63) - 1]


def _corner4(n):
    return R.corner4(n)


def _centered_masks(n):
    for kind in R.KINDS:
        for length in LENGTHS:
            yield kind, length, R.centered_mask(n, length, kind, 0, _corner4(n))


# ---- 1. agreement of every restatement -----------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_modulus_switch_restatements(oracle, n):
    words = _native_corpus(n)
    for log in sorted({n.bit_length(), 12}):
        want = [R.py_modulus_switch(w, log) for w in words]
        assert all(0 <= v < (1 << log) for v in want)
        assert [oracle.modulus_switch(w, log) for w in words] == want
        assert F.modulus_switch(np.array(words, np.uint64), log).tolist() == want
        assert [P128.modulus_switch(w, log) for w in words] == want
    assert [R.py_modulus_switch(w, n.bit_length()) for w, _, _ in R.native_words(n)] == [d for _, d, _ in R.native_words(n)]
    assert R.py_modulus_switch(0xDEADBEEF, 64) == oracle.modulus_switch(0xDEADBEEF, 64) == 0xDEADBEEF


@pytest.mark.parametrize("n", SIZES)
def test_non_native_switch_restatements(oracle, n):
    for x, val, kind in R.nonnative_words(n, P):
        assert R.py_ms_non_native(x, n, P) == val == oracle.pbs_modulus_switch_non_native(x, n, P), (x, kind)
    for d in R.degrees(n) + [2 * n]:                                    # the ranges are tight
        lo, hi = R.nonnative_range(d, n, P)
        if lo > 0:
            assert R.py_ms_non_native(lo - 1, n, P) == d - 1 == oracle.pbs_modulus_switch_non_native(lo - 1, n, P)
        if hi < P - 1:
            assert R.py_ms_non_native(hi + 1, n, P) == d + 1 == oracle.pbs_modulus_switch_non_native(hi + 1, n, P)


@pytest.mark.parametrize("n", SIZES)
def test_centered_correction_restatements(oracle, n):
    log = n.bit_length()
    for kind, length, mask in _centered_masks(n):
        corr = R.py_centered_correction(mask, log)
        assert oracle.centered_ms_body_correction(np.array(mask, np.uint64), log) == corr, (kind, length)
        assert P128.centered_body_correction(mask, log) == corr, (kind, length)
        for body, d in R.centered_bodies(n, corr):
            lwe = mask + [body]
            want = R.py_switch_lwe(lwe, log, True)
            assert want[-1] == d
            assert P128.switch_lwe(lwe, log, True) == want
            assert oracle.lwe_ms64(np.array([lwe], np.uint64), log, True)[0].tolist() == want


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("centered", [False, True])
def test_lwe_ms64_and_ms32_restatements(oracle, n, centered):
    """The stand-alone switches on whole ciphertexts, at log2(2N) and at 12; the u32 form on the corpus built at 32 bits."""
    for log in sorted({n.bit_length(), 12}):
        lwe = R.roll_batch(_native_corpus(n), _native_corpus(n))
        want = [R.py_switch_lwe([int(x) for x in row], log, centered) for row in lwe]
        assert oracle.lwe_ms64(lwe, log, centered).tolist() == want
        assert [P128.switch_lwe([int(x) for x in row], log, centered) for row in lwe] == want
    log = n.bit_length()
    words32 = [w for w, _, _ in R.native_words(n, 32)] + [0, 1, (1 << 32) - 1, 1 << 31]
    lwe32 = R.roll_batch(words32, words32).astype(np.uint32)
    want = [R.py_switch_lwe([int(x) for x in row], log, centered, 32) for row in lwe32]
    assert oracle.lwe_ms32(lwe32, log, centered).tolist() == want
    for kind in R.KINDS:                                                # the centered kinds at 32 bits
        mask = R.centered_mask(n, 40, kind, 1, bits=32)
        corr = R.py_centered_correction(mask, log, 32)
        rows = [mask + [b] for b, _ in R.centered_bodies(n, corr, 32)]
        want = [R.py_switch_lwe(r, log, True, 32) for r in rows]
        assert [w[-1] for w in want] == [d for _, d in R.centered_bodies(n, corr, 32)]
        assert oracle.lwe_ms32(np.array(rows, np.uint32), log, True).tolist() == want


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("q", [0, P])
def test_monomial_restatements(oracle, n, q):
    g = np.random.default_rng(n + (q != 0))
    poly = g.integers(0, q or M64, size=n, dtype=np.uint64)
    poly[:3] = [0, 1, (q or M64) - 1]
    ints = [int(x) for x in poly]
    glwe = g.integers(0, q or M64, size=(3, n), dtype=np.uint64)
    assert oracle.sample_extract(glwe.reshape(-1), n, 2, q).tolist() == R.py_sample_extract(R.rows(glwe), q)
    for d in R.degrees(n) + [2 * n]:
        mul, div = R.py_monomial_mul(ints, d, q), R.py_monomial_div(ints, d, q)
        assert oracle.poly_monomial_mul(poly, d, q).tolist() == mul, d
        assert oracle.poly_monomial_div(poly, d, q).tolist() == div, d
        assert R.py_monomial_div(mul, d, q) == ints and R.py_monomial_mul(ints, (2 * n - d) % (2 * n), q) == div
        if q == 0 and d < 2 * n:
            assert MB.monomial_mul(poly, d).tolist() == mul
            assert F._monomial_mul(poly[None, None, :], np.array([d]))[0, 0].tolist() == mul
            assert [v % M64 for v in P128.monomial_mul(ints, d)] == mul
            assert [v % M64 for v in P128.monomial_div(ints, d)] == div


@pytest.mark.parametrize("q", [0, P])
def test_blind_rotate_is_the_stepwise_rotation(q):
    """py_blind_rotate's single multiplication equals the division by X^body and one multiplication per set bit, with the
    non-native 2N among the switched values."""
    n = 32
    g = np.random.default_rng(5 + (q != 0))
    acc = R.rows(g.integers(0, q or M64, size=(2, n), dtype=np.uint64))
    values = R.degrees(n) + [2 * n]
    for b, body in enumerate(values):
        switched = values[b:] + values[:b] + [body]
        bits = R.secret_bits(len(values), b)
        assert R.py_blind_rotate(acc, switched, bits, q) == R.py_blind_rotate_stepwise(acc, switched, bits, q)


def test_reference_kat_halving_correction(oracle):
    """modulus_switch.rs test_ms_halving_correction: mask (1, 1), body 0, log 12: correction -1 - half_case, body 4095."""
    half_case = 1 << 51
    want = (-1 - half_case) % M64
    assert R.py_centered_correction([1, 1], 12) == want
    assert oracle.centered_ms_body_correction(np.array([1, 1], np.uint64), 12) == want
    assert P128.centered_body_correction([1, 1], 12) == want
    assert R.py_switch_lwe([1, 1, 0], 12, True) == [0, 0, 4095]
    assert P128.switch_lwe([1, 1, 0], 12, True) == [0, 0, 4095]
    assert oracle.lwe_ms64(np.array([[1, 1, 0]], np.uint64), 12, True).tolist() == [[0, 0, 4095]]
    # Scalar = u32: the same words, half_case 2^19
    assert R.py_centered_correction([1, 1], 12, 32) == (-1 - (1 << 19)) % (1 << 32)
    assert oracle.lwe_ms32(np.array([[1, 1, 0]], np.uint32), 12, True).tolist() == [[0, 0, 4095]]


# ---- 2. the corpus hits its corners --------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_corpus_reaches_its_corners(n):
    ds = R.degrees(n)
    assert ds[:6] == [0, 1, n - 1, n, n + 1, 2 * n - 1] and 1 < ds[6] < n - 1 and n + 1 < ds[7] < 2 * n - 1
    u, log = R.unit(n), n.bit_length()
    native = R.native_words(n)
    for d in ds:                                                         # every degree with both edges, and they are edges
        kinds = {k: w for w, dd, k in native if dd == d}
        assert set(kinds) == {"grid", "low", "high"}
        assert R.py_modulus_switch((kinds["low"] - 1) % M64, log) == (d - 1) % (2 * n)
        assert R.py_modulus_switch((kinds["high"] + 1) % M64, log) == (d + 1) % (2 * n)
    assert (M64 - u // 2, 0, "low") in native                            # the tie past the top wraps to 0
    nonnative = R.nonnative_words(n, P)
    for d in ds + [2 * n]:
        assert {k for _, dd, k in nonnative if dd == d} >= {"low", "high"}
    assert (P - 1, 2 * n, "high") in nonnative                           # 2N occurs unfolded
    assert (0, 0, "zero") in nonnative and (1, 0, "one") in nonnative
    # the sign boundary e < rem / m >= N - rem: both sides are reached by rem in {0, 1, N - 1} and full in {0, 1}
    assert {(d // n, d % n) for d in ds} >= {(0, 0), (0, 1), (0, n - 1), (1, 0), (1, 1), (1, n - 1)}
    for kind, length, mask in _centered_masks(n):
        sum_half, hed = R.centered_sums(mask, log)
        small = [a for a in mask if a not in _corner4(n)]
        assert all(R.py_modulus_switch(a, log) == 0 for a in small)
        if kind == "hed_zero":
            assert hed == 0 and sum_half < (1 << 63)
        elif kind == "sum_half_wraps":
            assert hed == 0 and sum_half >= (1 << 63)                    # a negative total: the u64 sum wrapped
        elif kind == "hed_odd_positive":
            assert hed > 0 and hed % 2 == 1
        else:
            assert hed < 0 and hed % 2 == 1 and R.trunc_div2(hed) != hed // 2
        corr = R.py_centered_correction(mask, log)
        got = [R.py_modulus_switch((b + corr) % M64, log) for b, _ in R.centered_bodies(n, corr)]
        assert got == [d for _, d in R.centered_bodies(n, corr)]
        assert set(got) >= set(ds) | {(d - 1) % (2 * n) for d in ds}     # both sides of every edge, 2^64's included
    # some mask has an odd negative rounding error (a positive odd word): err / 2 truncates
    assert any(0 < a < u // 2 and a % 2 for _, _, m in _centered_masks(n) for a in m)


# ---- 3. the corpus discriminates -----------------------------------------------------------------------------------
def _mut_ms_tie_down(x, log):
    return ((x + (1 << (63 - log)) - 1) % M64) >> (64 - log)


def _mut_mul(poly, d, q, mode):
    n = len(poly)
    full, rem = (d // n) % 2, d % n
    if mode == "unfolded":
        full = d // n                                                   # 2N / N = 2 read as "negate"
    if mode == "full_ignored" and rem == 0:
        return list(poly)
    edge = (lambda e: e <= rem) if mode == "boundary" else (lambda e: e < rem)
    return [R._neg(poly[(e - rem) % n], q) if bool(full) ^ edge(e) else poly[(e - rem) % n] for e in range(n)]


def _mut_div(poly, d, q, mode):
    n = len(poly)
    full, rem = (d // n) % 2, d % n
    if mode == "unfolded":
        full = d // n
    if mode == "full_ignored" and rem == 0:
        return list(poly)
    edge = (lambda m: m > n - rem) if mode == "boundary" else (lambda m: m >= n - rem)
    return [R._neg(poly[(m + rem) % n], q) if bool(full) ^ edge(m) else poly[(m + rem) % n] for m in range(n)]


def _mut_correction(mask, log, floor_err, floor_total):
    sum_half, hed = 0, 0
    for a in mask:
        err = R._signed(((R.py_modulus_switch(a, log) << (64 - log)) - a) % M64)
        half = err // 2 if floor_err else R.trunc_div2(err)
        hed += 2 * half - err
        sum_half += half
    return (sum_half - (hed // 2 if floor_total else R.trunc_div2(hed)) - (1 << (63 - log))) % M64


@pytest.mark.parametrize("n", SIZES)
def test_corpus_discriminates(n):
    log = n.bit_length()
    native = [w for w, _, _ in R.native_words(n)]
    assert any(_mut_ms_tie_down(w, log) != R.py_modulus_switch(w, log) for w in native)         # the tie rounds down
    poly = list(range(1, n + 1))                                        # no coefficient equals its own negation
    for q in (0, P):
        sw = R.degrees(n) + [v for _, v, _ in R.nonnative_words(n, P)]
        for mode in ("unfolded", "boundary", "full_ignored"):
            assert any(_mut_mul(poly, d, q, mode) != R.py_monomial_mul(poly, d, q) for d in sw), mode
            assert any(_mut_div(poly, d, q, mode) != R.py_monomial_div(poly, d, q) for d in sw), mode
    masks = [m for _, _, m in _centered_masks(n)]
    assert any(_mut_correction(m, log, True, False) != R.py_centered_correction(m, log) for m in masks)
    assert any(_mut_correction(m, log, False, True) != R.py_centered_correction(m, log) for m in masks)
    # ... and the difference reaches the switched body through a body on the cell edge
    for floor_err, floor_total in ((True, False), (False, True)):
        hit = False
        for m in masks:
            corr = R.py_centered_correction(m, log)
            bad = _mut_correction(m, log, floor_err, floor_total)
            hit |= any(R.py_modulus_switch((b + bad) % M64, log) != d for b, d in R.centered_bodies(n, corr))
        assert hit
    words = [x for x, _, _ in R.nonnative_words(n, P)]                  # x = 1 skipped like x = 0
    assert [(i, d) for i, d in R.py_steps_non_native(words, n, P) if words[i] > 1] != R.py_steps_non_native(words, n, P)
    assert (words.index(1), 0) in R.py_steps_non_native(words, n, P)
    assert all(d != 0 for _, d in R.py_steps_native(native, log)) and len(R.py_steps_native(native, log)) < len(native)


# ---- 4. the oracle's PBS on a noiseless gadget key -------------------------------------------------------------------
def _trivial_case(oracle, n, base_log, level, bnf, mode):
    """(ctx, lwe batch, secret bits, LUT, NTT-domain key, switched values per item)."""
    q, k = (0 if bnf else P), 1
    log = n.bit_length()
    if mode == 2:
        lwe = R.pre_switched_batch(n)
        switched = lwe.tolist()
    elif mode == 1:
        lwe = R.centered_batch(n, R.KINDS[2])
        switched = [R.py_switch_lwe([int(x) for x in row], log, True) for row in lwe]
    elif bnf:
        lwe = R.standard_batch(n)
        switched = [R.py_switch_lwe([int(x) for x in row], log) for row in lwe]
    else:
        lwe = R.standard_batch(n, P)
        switched = [[R.py_ms_non_native(int(x), n, P) for x in row] for row in lwe]
    bits = R.secret_bits(lwe.shape[1] - 1, n)
    lut = R.gadget_lut(k, n, base_log, level, 7, q)
    std = R.gadget_key(bits, k, n, base_log, level)
    ctx = oracle.NttContext(n)
    key = ctx.bsk_to_ntt(std.reshape(-1), 64 if bnf else 0, normalize=not bnf)
    return ctx, lwe, bits, lut, key, switched


@pytest.mark.parametrize("n,base_log,level", [(256, 23, 1), (256, 12, 2), (2048, 23, 1), (2048, 12, 2)])
@pytest.mark.parametrize("bnf,mode", [(True, 0), (True, 1), (True, 2), (False, 0), (False, 2)])
def test_oracle_pbs_on_trivial_key(oracle, n, base_log, level, bnf, mode):
    """Every CMUX of a noiseless gadget key selects exactly (the LUT's coefficients are multiples of 2^(64 - B l) of
    magnitude < 2^62, so each difference X^a acc - acc decomposes exactly), so the oracle's blind rotation must return
    LUT * X^(sum s_i a_i - body) and its PBS the extracted sample of that, bit for bit."""
    q, k = (0 if bnf else P), 1
    ctx, lwe, bits, lut, key, switched = _trivial_case(oracle, n, base_log, level, bnf, mode)
    batch = lwe.shape[0]
    want = [R.expected_rotation(lut, switched[b], bits, q) for b in range(batch)]
    accs = np.broadcast_to(lut, (batch, k + 1, n)).copy()
    got = ctx.blind_rotate_batch(accs, lwe, key, k, base_log, level, bnf=bnf, ms_mode=mode)
    assert np.array_equal(got, np.stack([w[0] for w in want]))
    assert len({R.py_rotation_degree(s, bits, n) for s in switched}) > batch // 3   # the items rotate differently
    if mode == 2:
        return                                                          # .pbs takes raw ciphertexts
    for b in range(batch):
        out = ctx.pbs(lwe[b], lut.reshape(-1), key, k, base_log, level, bnf=bnf, centered=mode == 1)
        assert np.array_equal(out, want[b][1]), b


@pytest.mark.parametrize("base_log,level", [(23, 1), (12, 2)])
def test_fft_oracle_pbs_on_trivial_key(base_log, level):
    """The f64 restatement on the same key at N = 2048, under the project's f64 bound (test_fft_gpu
    test_external_product_vs_exact)."""
    n, k = 2048, 1
    lwe = R.standard_batch(n)
    bits = R.secret_bits(lwe.shape[1] - 1, n)
    lut = R.gadget_lut(k, n, base_log, level, 7)
    fbsk = F.forward_as_torus(R.gadget_key(bits, k, n, base_log, level))
    got = F.pbs(lwe, lut, fbsk, base_log, level)
    want = np.stack([R.expected_rotation(lut, R.py_switch_lwe([int(x) for x in row], 12), bits)[1] for row in lwe])
    err = F.signed_diff(got, want).max()
    print(f"f64 oracle PBS on the gadget key ({base_log},{level}): log2 err = {np.log2(max(err, 1)):.1f}")
    assert err < 2.0 ** max(48, base_log + 24), np.log2(err)
