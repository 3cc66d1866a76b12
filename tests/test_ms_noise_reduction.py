"""The drift-technique modulus switch noise reduction without a device: the CPU restatements the GPU tests compare
against (tests/ms_noise_helpers.py) are checked against each other, against the reference's own statistical tests,
and against one-off mutants; and the C ABI's argument checks, which run before any device call."""
import ctypes
import math

import numpy as np
import pytest

import ms_noise_helpers as MS


def _scalar_all(c, **mutant):
    got = [MS.choose_scalar(x, c.zeros, c.p, **mutant) for x in c.lwe]
    return np.array([g[0] for g in got], np.int64), np.array([g[1] for g in got], np.int32)


def test_restatements_agree_on_the_corpora():
    for c in MS.small_corpora():
        cand, sat, _, _ = c.expected
        scand, ssat = _scalar_all(c)
        assert np.array_equal(cand, scand) and np.array_equal(sat, ssat), c.name
        table = MS.all_measures_np(c.lwe, c.zeros, c.p)
        for b in (0, len(c.lwe) - 1):
            x = [int(v) for v in c.lwe[b]]
            assert table[b, 0] == MS.measure_scalar(x[:-1], x[-1], c.p)
            for ci in (0, 63, 64, 129):
                z = [int(v) for v in c.zeros[ci]]
                w = [(a + b_) % 2**64 for a, b_ in zip(x, z)]
                assert table[b, 1 + ci] == MS.measure_scalar(w[:-1], w[-1], c.p), (c.name, b, ci)
        # the kernel's tile walk is the same function
        tiles = MS.prepared_tiles(c.zeros)
        walk = [MS.choose_tiled(x, tiles, len(c.zeros), c.p) for x in c.lwe]
        assert [w[0] for w in walk] == cand.tolist() and [w[1] for w in walk] == sat.tolist(), c.name


def test_restatements_agree_on_the_sweeps():
    """Every log modulus and zeros count at lwe_dim 1 and 33 (918 is beyond a pure-Python loop; the numpy form covers
    it in the GPU tests).  Below log modulus 10 the i64 -> f64 conversion rounds."""
    rounds = False
    for lwe, zeros, p in MS.sweep_cases(lwe_dims=(1, 33), items=2):
        cand, sat = MS.choose_np(lwe, zeros, p)
        for b in range(len(lwe)):
            assert MS.choose_scalar(lwe[b], zeros, p) == (cand[b], sat[b]), (lwe.shape, len(zeros), p.log_modulus)
        e = MS.round_error(lwe, p.log_modulus)
        rounds |= bool((e.astype(np.float64).astype(np.int64) != e).any())
    assert rounds


def test_corpora_cover_what_they_were_built_for():
    """Asserted so that a reseed cannot hollow the corpora out."""
    planted = [c for c in MS.planted_corpora() if c.name.startswith("planted-") and c.name != "planted-pairs"]
    hit = set()
    for c in planted:
        cand, sat, _, _ = c.expected
        assert sat.all()
        hit |= {t for t, got in zip(MS.PLANT_TARGETS, cand) if got == t}
        # a planted candidate measures the least a measure can be
        table = MS.all_measures_np(c.lwe, c.zeros, c.p)
        for i, t in enumerate(MS.PLANT_TARGETS):
            assert table[i, 1 + t] == math.sqrt(c.p.modular_variance) * c.p.r_sigma
        assert (table[:, 0] > c.p.bound).all()
    assert hit == set(MS.PLANT_TARGETS)
    by_name = {c.name: c for c in MS.small_corpora()}
    pairs = by_name["planted-pairs"]
    cand, sat, _, _ = pairs.expected
    assert cand.tolist() == [first for first, _ in MS.PLANT_PAIRS] and sat.all()
    table = MS.all_measures_np(pairs.lwe, pairs.zeros, pairs.p)
    for i, (first, second) in enumerate(MS.PLANT_PAIRS):
        assert table[i, 1 + second] < table[i, 1 + first] <= pairs.p.bound  # the later one is the better one
    cand, sat, improved, _ = by_name["base-satisfied"].expected
    assert (cand == -1).all() and sat.all() and np.array_equal(improved, by_name["base-satisfied"].lwe)
    never = by_name["never-satisfied"]
    cand, sat, _, _ = never.expected
    table = MS.all_measures_np(never.lwe, never.zeros, never.p)
    assert cand[0] == 5 and table[0, 1 + 5] == table[0, 1 + 70] == table[0, 1 + 129] == table[0].min()
    assert cand[1] == -1 and table[1, 0] == table[1, 1 + 3] == table[1].min()
    assert cand[2] >= 0 and not sat.any()
    every = by_name["everything-passes"]
    cand, sat, improved, _ = every.expected
    assert (cand == -1).all() and sat.all() and np.array_equal(improved, every.lwe)
    # all three outcomes occur: satisfied at base, satisfied by a candidate, not satisfied
    outcomes = set()
    for c in MS.small_corpora():
        cand, sat, _, _ = c.expected
        outcomes |= {(bool(s), bool(k >= 0)) for k, s in zip(cand, sat)}
    assert {(True, False), (True, True), (False, True), (False, False)} <= outcomes


def _outcomes(fn):
    return [[fn(x, c) for x in c.lwe] for c in MS.small_corpora()]


def test_corpora_tell_the_mutants_from_the_true_function():
    truth = _outcomes(lambda x, c: MS.choose_scalar(x, c.zeros, c.p))
    # `<=` in the best update: the later duplicate and the all-zero row win
    assert _outcomes(lambda x, c: MS.choose_scalar(x, c.zeros, c.p, le_update=True)) != truth
    # the kernel-walk mutants
    walk = lambda **m: _outcomes(lambda x, c: MS.choose_tiled(x, MS.prepared_tiles(c.zeros), len(c.zeros), c.p, **m))
    assert walk() == truth
    assert walk(best_of_walk=True) != truth
    # padded lanes voting: harmless over the library's zero fill (such a lane measures what the input does), so the
    # mask is what protects a key whose padding is not zero: pad with a row that beats every candidate of item 2
    c = MS.never_satisfied_corpus()
    with np.errstate(over="ignore"):
        best_row = (MS.switch_np(c.lwe[2], c.p.log_modulus) << np.uint64(64 - c.p.log_modulus)) - c.lwe[2]
    tiles = MS.prepared_tiles(c.zeros, padding=np.repeat(best_row[None], 64, axis=0))
    padded = lambda mask: [MS.choose_tiled(x, tiles, len(c.zeros), c.p, mask_padding=mask) for x in c.lwe]
    want = [MS.choose_scalar(x, c.zeros, c.p) for x in c.lwe]
    assert padded(True) == want
    assert padded(False) != want and padded(False)[2] == (len(c.zeros), 0)
    # the two summation mutants change measures of the corpus (and are the true function when switched off)
    c = MS.planted_corpora()[0]
    fused = pairwise = 0
    for x in c.lwe:
        for z in c.zeros[::8]:
            w = [(int(a) + int(b)) % 2**64 for a, b in zip(x, z)]
            m = MS.measure_scalar(w[:-1], w[-1], c.p)
            fused += MS.measure_scalar(w[:-1], w[-1], c.p, fused=True) != m
            pairwise += MS.measure_scalar(w[:-1], w[-1], c.p, pairwise=True) != m
    assert fused > 0 and pairwise > 0, (fused, pairwise)


def test_reference_statistics_at_test_param():
    """The reference's three tests (algorithms/test/modulus_switch_noise_reduction.rs) under the numpy restatement, at
    its TEST_PARAM with a fixed seed and 4096 ciphertexts; the bands are the reference's own."""
    sk, zeros, lwe = MS.reference_shape_data()
    cand, sat, improved = MS.reference_shape_expected()
    # improve_modulus_switch_noise_test_individual_check_p_success, on the first 64 inputs' 92 736 checks
    table = MS.all_measures_np(lwe[:64], zeros, MS.TEST_PARAM)
    p_success = float((table[:, 1:] <= MS.TEST_PARAM.bound).mean())
    # improve_modulus_switch_noise_test_average_number_checks
    assert sat.all(), "No candidate was good enough"
    average_number_checks = float((1 + (cand + 1)).mean())
    # check_noise_improve_modulus_switch_noise
    base_variance = MS.sample_variance(MS.ms_noise(sk, lwe, lwe, MS.TEST_PARAM.log_modulus))
    variance_improved = MS.sample_variance(MS.ms_noise(sk, lwe, improved, MS.TEST_PARAM.log_modulus))
    print(f"p_success {p_success} / {MS.TEST_P_SUCCESS}; checks {average_number_checks} / {1 / MS.TEST_P_SUCCESS}; "
          f"base {base_variance / MS.expected_base_variance(MS.TEST_LWE_DIM, 12)}; "
          f"improved {variance_improved / MS.expected_improved_variance()}; max index {cand.max()}")
    assert MS.both_ratio_under(p_success, MS.TEST_P_SUCCESS, 1.1)
    assert MS.both_ratio_under(average_number_checks, 1 / MS.TEST_P_SUCCESS, 1.1)
    assert MS.both_ratio_under(base_variance, MS.expected_base_variance(MS.TEST_LWE_DIM, 12), 1.03)
    assert MS.both_ratio_under(variance_improved, MS.expected_improved_variance(), 1.03)


# ---- the C ABI's checks that need no device --------------------------------------------------------------------

_NAN_MSG = "ms_bound, ms_r_sigma_factor and ms_input_variance must not be NaN"
_NEG_MSG = "ms_r_sigma_factor and ms_input_variance must not be negative"


def _create(L, zeros, lwe_dim, count, bound, r_sigma, variance, out=True):
    h = ctypes.c_void_p()
    st = L.mi_ms_noise_key_create(zeros, lwe_dim, count, bound, r_sigma, variance, 0, None,
                                  ctypes.byref(h) if out else None)
    assert not h.value
    return st, L.mi_last_error_message().decode()


def test_ms_noise_key_create_rejections(engine):
    from tfhe_ntt_amd import _lib

    L = _lib.lib()
    INVALID = _lib.MI_ERR_INVALID_ARG
    words = (ctypes.c_uint64 * 4)()  # never dereferenced
    z = ctypes.addressof(words)
    nan, inf = math.nan, math.inf
    assert _create(L, None, 8, 4, 1.0, 1.0, 1.0) == (INVALID, "zeros is NULL")
    assert _create(L, z, 8, 4, 1.0, 1.0, 1.0, out=False) == (INVALID, "out_key is NULL")
    for dim in (0, 1 << 24):
        assert _create(L, z, dim, 4, 1.0, 1.0, 1.0) == (INVALID, "lwe dimension out of range")
    assert _create(L, z, 8, 0, 1.0, 1.0, 1.0) == (INVALID, "expected at least one encryption of zero")
    assert _create(L, z, 8, 1 << 32, 1.0, 1.0, 1.0) == (INVALID, "zeros_count out of range")
    for triple in ((nan, 1.0, 1.0), (1.0, nan, 1.0), (1.0, 1.0, nan)):
        assert _create(L, z, 8, 4, *triple) == (INVALID, _NAN_MSG)
    for triple in ((1.0, -1.0, 1.0), (1.0, 1.0, -1e-300), (inf, 1.0, -inf)):
        assert _create(L, z, 8, 4, *triple) == (INVALID, _NEG_MSG)
    # the first failing rule answers
    assert _create(L, None, 0, 0, nan, -1.0, -1.0, out=False) == (INVALID, "zeros is NULL")
    assert _create(L, z, 0, 0, nan, -1.0, -1.0) == (INVALID, "lwe dimension out of range")
    assert _create(L, z, 8, 0, nan, -1.0, -1.0) == (INVALID, "expected at least one encryption of zero")
    assert _create(L, z, 8, 4, nan, -1.0, -1.0) == (INVALID, _NAN_MSG)


def test_ms_noise_null_handles(engine):
    from tfhe_ntt_amd import _lib

    L = _lib.lib()
    INVALID = _lib.MI_ERR_INVALID_ARG

    def other_error():  # so that the message read next is the following call's own
        assert L.mi_lwe_ksk_create(None, 8, 10, 4, 4, 0, None, None) == INVALID
        assert L.mi_last_error_message() == b"out_key is NULL"

    assert L.mi_ms_noise_key_destroy(None) == _lib.MI_OK
    for call in (lambda: L.mi_ms_noise_key_info(None, None, None, None, None, None),
                 lambda: L.mi_lwe_ms_noise_measure_batch(None, None, None, 1, 12, 0, None),
                 lambda: L.mi_lwe_ms_noise_choose_batch(None, None, None, None, 1, 12, None),
                 lambda: L.mi_lwe_ms_noise_improve_batch(None, None, None, 1, 12, None, None, None),
                 lambda: L.mi_lwe_ms_noise_improve_and_switch_batch(None, None, None, 1, 12, None),
                 lambda: L.mi_lwe_ms_noise_improve_and_switch_batch(None, None, None, 0, 12, None)):
        other_error()
        assert call() == INVALID
        assert L.mi_last_error_message() == b"key is NULL"


def test_python_mirror_is_exported(engine):
    M = engine.modulus_switch_noise_reduction
    for name in ("ModulusSwitchNoiseReductionKey", "measure_modulus_switch_noise_estimation_for_binary_key",
                 "choose_candidate_to_improve_modulus_switch_noise_for_binary_key",
                 "improve_lwe_ciphertext_modulus_switch_noise_for_binary_key"):
        assert hasattr(M, name)
    assert hasattr(M.ModulusSwitchNoiseReductionKey, "improve_modulus_switch_noise")
    assert hasattr(M.ModulusSwitchNoiseReductionKey, "improve_noise_and_modulus_switch")
