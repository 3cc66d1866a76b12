"""The drift-technique modulus switch noise reduction on the GPU (`-m gpu`) against the CPU restatement of
tests/ms_noise_helpers.py.

Bar: bit for bit.  The measures are compared as u64 views of the f64 values, which pins the FMA contraction, the
summation order, the i64 -> f64 conversion and the square root all at once; candidates, outputs and switched words are
integers.  The reference's own statistical tests are repeated on the device's results with the reference's bands.
"""
import numpy as np
import pytest

import ms_noise_helpers as MS
import tfhe_helpers as H

pytestmark = pytest.mark.gpu


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.uint64).view(np.int64)).cuda()  # a copy: the shared data is read-only


def host(t):
    return t.cpu().numpy().view(np.uint64)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def M(engine):
    return engine.modulus_switch_noise_reduction


def make_key(M, zeros, p):
    return M.ModulusSwitchNoiseReductionKey(dev(zeros), p.bound, p.r_sigma, p.input_variance)


@pytest.fixture(scope="module")
def reference_key(M):
    _, zeros, _ = MS.reference_shape_data()
    return make_key(M, zeros, MS.TEST_PARAM)


def check_all_entries(M, key, lwe, p, want):
    """choose / improve (out of place with the choice, in place without) / improve_and_switch against
    (candidate, satisfied, improved, switched)."""
    import torch
    cand, sat, improved, switched = want
    x = dev(lwe)
    got_cand, got_sat = M.choose_candidate_to_improve_modulus_switch_noise_for_binary_key(key, x, p.log_modulus)
    assert np.array_equal(got_cand.cpu().numpy(), cand)
    assert np.array_equal(got_sat.cpu().numpy(), sat)
    out = torch.zeros_like(x)
    got_cand, got_sat = M.improve_lwe_ciphertext_modulus_switch_noise_for_binary_key(key, x, p.log_modulus, output=out,
                                                                                     return_candidates=True)
    assert np.array_equal(host(out), improved) and np.array_equal(host(x), lwe)
    assert np.array_equal(got_cand.cpu().numpy(), cand) and np.array_equal(got_sat.cpu().numpy(), sat)
    sw = torch.zeros_like(x)
    key.improve_noise_and_modulus_switch(x, sw, p.log_modulus)
    assert np.array_equal(host(sw), switched)
    key.improve_modulus_switch_noise(x, p.log_modulus)  # in place, candidate / satisfied NULL
    assert np.array_equal(host(x), improved)


def test_measures_reference_shape(M, reference_key):
    """64 LWEs x (1 + 1449) measures at the reference's TEST_PARAM, bit for bit; and the reference's
    improve_modulus_switch_noise_test_individual_check_p_success on that table."""
    _, zeros, lwe = MS.reference_shape_data()
    want = MS.all_measures_np(lwe[:64], zeros, MS.TEST_PARAM)
    x = dev(lwe[:64])
    got = M.measure_modulus_switch_noise_estimation_for_binary_key(reference_key, x, 12, all_candidates=True)
    got = got.cpu().numpy()
    assert got.shape == (64, 1 + MS.TEST_ZEROS)
    differ = np.flatnonzero(bits(got) != bits(want))
    assert differ.size == 0, (differ.size, differ[:8], got.reshape(-1)[differ[:8]], want.reshape(-1)[differ[:8]])
    base = M.measure_modulus_switch_noise_estimation_for_binary_key(reference_key, x, 12).cpu().numpy()
    assert np.array_equal(bits(base), bits(want[:, 0]))
    p_success = float((got[:, 1:] <= MS.TEST_PARAM.bound).mean())
    print(f"p_success {p_success} / {MS.TEST_P_SUCCESS}")
    assert MS.both_ratio_under(p_success, MS.TEST_P_SUCCESS, 1.1)


@pytest.mark.parametrize("lwe_dim", MS.LWE_DIMS)
def test_sweeps(M, lwe_dim):
    """Every log modulus (below 10 the conversion to f64 rounds; at 64 every error is 0) and every zeros count around
    the tile size, at three dimensions: the whole measure table and every entry's result."""
    for lwe, zeros, p in MS.sweep_cases(lwe_dims=(lwe_dim,)):
        key = make_key(M, zeros, p)
        got = M.measure_modulus_switch_noise_estimation_for_binary_key(key, dev(lwe), p.log_modulus, all_candidates=True)
        assert np.array_equal(bits(got.cpu().numpy()), bits(MS.all_measures_np(lwe, zeros, p))), \
            (lwe_dim, len(zeros), p.log_modulus)
        cand, sat = MS.choose_np(lwe, zeros, p)
        improved = MS.improve_np(lwe, zeros, cand)
        check_all_entries(M, key, lwe, p, (cand, sat, improved, MS.switch_np(improved, p.log_modulus)))


def test_corpora(M):
    """The planted targets around the tile borders, the earlier-but-worse satisfying candidate, the ties of the
    first-minimum path, bound 0 and bound +inf."""
    for c in MS.small_corpora():
        check_all_entries(M, make_key(M, c.zeros, c.p), c.lwe, c.p, c.expected)


def test_reference_shape_4096(M, reference_key):
    """4096 encryptions at TEST_PARAM: every entry equals the restatement, and the reference's
    improve_modulus_switch_noise_test_average_number_checks and check_noise_improve_modulus_switch_noise hold on the
    device's own outputs (same seed as the CPU test)."""
    sk, zeros, lwe = MS.reference_shape_data()
    cand, sat, improved = MS.reference_shape_expected()
    p = MS.TEST_PARAM
    check_all_entries(M, reference_key, lwe, p, (cand, sat, improved, MS.switch_np(improved, p.log_modulus)))
    x = dev(lwe)
    got_cand, got_sat = M.improve_lwe_ciphertext_modulus_switch_noise_for_binary_key(reference_key, x, p.log_modulus,
                                                                                     return_candidates=True)
    got_cand, got_sat = got_cand.cpu().numpy(), got_sat.cpu().numpy()
    assert got_sat.all(), "No candidate was good enough"
    average_number_checks = float((1 + (got_cand + 1)).mean())
    variance_improved = MS.sample_variance(MS.ms_noise(sk, lwe, host(x), p.log_modulus))
    print(f"checks {average_number_checks} / {1 / MS.TEST_P_SUCCESS}; "
          f"improved {variance_improved / MS.expected_improved_variance()}")
    assert MS.both_ratio_under(average_number_checks, 1 / MS.TEST_P_SUCCESS, 1.1)
    assert MS.both_ratio_under(variance_improved, MS.expected_improved_variance(), 1.03)


def test_through_a_bootstrap(engine, M):
    """Real keys at the smallest shape of the NTT PBS tests (n = 64, N = 2048, BNF).  improve_and_switch -> PBS at
    MS_PRE_SWITCHED equals the restatement's improved LWEs -> the same PBS at MS_STANDARD bit for bit, and decrypts to
    the LUT's values; some inputs take an encryption of zero and some do not."""
    P = 0xFFFFFFFF00000001
    N, K, n_lwe, base_log, level, msg_mod = 2048, 1, 64, 23, 1, 4
    delta = (1 << 63) // msg_mod
    g = H.rng(1718)
    lwe_sk = H.binary_key(g, n_lwe)
    glwe_sk = H.binary_key(g, (K, N))
    bsk = H.bsk_gen(g, lwe_sk, glwe_sk, base_log, level, 17, 0)
    f = lambda v: (3 * v + 1) % msg_mod
    lut = H.pbs_lut(N, K, msg_mod, delta, f, 0)
    msgs = np.array(list(range(msg_mod)) * 3)
    lwe = H.lwe_encrypt_batch(g, (msgs * delta).astype(np.uint64), lwe_sk, 30)
    zeros = H.lwe_encrypt_batch(g, np.zeros(70, np.uint64), lwe_sk, 30)
    p = MS.Params(0.0, MS.TEST_PARAM.r_sigma, 2.0**60 / 3 / 2.0**128, 12)
    p.bound = float(np.median(MS.measures_np(lwe, np.zeros((1, n_lwe + 1), np.uint64), p)))
    cand, sat = MS.choose_np(lwe, zeros, p)
    assert (cand >= 0).any() and (cand == -1).any()
    improved = MS.improve_np(lwe, zeros, cand)

    Pbs = engine.ntt64_pbs
    plan = engine.Plan.try_new(N, P)
    gkey = dev(np.zeros_like(bsk))
    Pbs.convert_standard_lwe_bootstrap_key_to_ntt64(plan, dev(bsk), gkey, normalize=False, input_modulus_width=64)
    key = Pbs.NttBootstrapKey(plan, gkey, base_log, level, Pbs.BNF)
    ms_key = make_key(M, zeros, p)
    switched = dev(np.zeros_like(lwe))
    ms_key.improve_noise_and_modulus_switch(dev(lwe), switched, p.log_modulus)
    out_a = dev(np.zeros((len(msgs), K * N + 1), np.uint64))
    out_b = dev(np.zeros((len(msgs), K * N + 1), np.uint64))
    Pbs.programmable_bootstrap_ntt64_bnf_lwe_ciphertext_mem_optimized(switched, out_a, dev(lut), key,
                                                                      Pbs.MS_PRE_SWITCHED)
    Pbs.programmable_bootstrap_ntt64_bnf_lwe_ciphertext_mem_optimized(dev(improved), out_b, dev(lut), key,
                                                                      Pbs.MS_STANDARD)
    assert np.array_equal(host(out_a), host(out_b))
    out_sk = H.glwe_sk_as_lwe_sk(glwe_sk)
    for i, m in enumerate(msgs):
        assert H.decode(H.lwe_decrypt(host(out_a)[i], out_sk, 0), delta, msg_mod, 0) == f(int(m))


def test_python_layer_errors(engine, M):
    import torch
    c = MS.everything_passes_corpus()
    with pytest.raises(ValueError, match="Expected at least one encryption of zero"):
        M.ModulusSwitchNoiseReductionKey(dev(c.zeros[:0]), 1.0, 1.0, 1.0)
    with pytest.raises(ValueError):
        M.ModulusSwitchNoiseReductionKey(dev(c.zeros.reshape(-1)), 1.0, 1.0, 1.0)
    key = make_key(M, c.zeros, c.p)
    x = dev(c.lwe)
    size = c.lwe.shape[1]
    with pytest.raises(ValueError, match=rf"input lwe size \(=LweSize\({size - 1}\)\) != encryptions of zero lwe size \(=LweSize\({size}\)\)"):
        M.choose_candidate_to_improve_modulus_switch_noise_for_binary_key(key, x[:, :-1], 12)
    with pytest.raises(ValueError, match="input lwe size"):
        key.improve_modulus_switch_noise(x[:, 1:].contiguous(), 12)
    with pytest.raises(ValueError):
        key.improve_noise_and_modulus_switch(x, torch.zeros_like(x)[:2], 12)
    for log_modulus in (0, 65):
        with pytest.raises(engine.MiError) as e:
            key.improve_modulus_switch_noise(x, log_modulus)
        assert e.value.status == 1
    # every batch entry: the log modulus is checked before the buffers, and an empty batch is fine
    import ctypes
    L = engine._lib.lib()
    dim, count = ctypes.c_size_t(), ctypes.c_size_t()
    doubles = [ctypes.c_double() for _ in range(3)]
    assert L.mi_ms_noise_key_info(key._h, ctypes.byref(dim), ctypes.byref(count), *map(ctypes.byref, doubles)) == 0
    assert (dim.value, count.value) == (size - 1, len(c.zeros))
    assert [d.value for d in doubles] == [c.p.bound, c.p.r_sigma, c.p.input_variance]
    entries = (lambda b, lm: L.mi_lwe_ms_noise_measure_batch(key._h, None, None, b, lm, 1, None),
               lambda b, lm: L.mi_lwe_ms_noise_choose_batch(key._h, None, None, None, b, lm, None),
               lambda b, lm: L.mi_lwe_ms_noise_improve_batch(key._h, None, None, b, lm, None, None, None),
               lambda b, lm: L.mi_lwe_ms_noise_improve_and_switch_batch(key._h, None, None, b, lm, None))
    for entry in entries:
        for log_modulus in (0, 65):
            assert entry(1, log_modulus) == 1 and L.mi_last_error_message() == b"log_modulus must be in [1, 64]"
        assert entry(1, 64) == 1 and L.mi_last_error_message() == b"buffer is NULL"
        assert entry(0, 12) == 0
    key.improve_modulus_switch_noise(x[:0], 12)
    assert np.array_equal(host(x), c.lwe)
