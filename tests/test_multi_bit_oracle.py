"""The numpy restatement of the multi-bit PBS (tests/multi_bit_helpers.py) against fft_oracle, on the host.

What the GPU tests lean on is pinned here first: the closed-form monomial transform, the selection / combination of
key bits, the degree rule at its corners, and that the restated bootstrap decrypts f(m).
"""
import numpy as np
import pytest

import fft_oracle as F
import multi_bit_helpers as MB
import tfhe_helpers as H

N = 2048
DEGREES = [0, 1, 5, 1023, 1024, 1025, 2047, 2048, 2049, 3071, 3072, 4095]


def _monomial(d):
    """X^d mod (X^N + 1) as a coefficient vector, d in [0, 2N)."""
    x = np.zeros(N, np.uint64)
    x[d % N] = np.uint64(1) if d < N else np.uint64(2**64 - 1)
    return x


@pytest.mark.parametrize("d", DEGREES)
def test_closed_form_monomial_matches_the_transform(d):
    want = F.forward_as_integer(_monomial(d))
    got = MB.monomial_fourier(d, N)
    err = np.abs(got - want).max()
    print(f"d = {d}: max |closed form - forward_as_integer| = {err:.3e}")
    assert err < 1e-13  # the project's transform tolerance (unit-modulus values)


def test_selection_bits():
    assert MB.selection_bits(3, 3) == [0, 1, 1]
    assert MB.selection_bits(0, 4) == [0, 0, 0, 0]
    assert MB.selection_bits(8, 4) == [1, 0, 0, 0]
    assert MB.selection_bits(1, 2) == [0, 1]


@pytest.mark.parametrize("g", [2, 3, 4])
def test_combined_key_bits(g):
    rng = H.rng(40 + g)
    sk = H.binary_key(rng, 6 * g)
    sk[:g] = 0        # group 0: all key bits 0 -> only idx 0 is 1
    sk[g:2 * g] = 1   # group 1: all key bits 1 -> only idx 2^g - 1 is 1
    bits = MB.combined_key_bits(sk, g)
    assert bits.shape == (6, 1 << g)
    assert np.array_equal(bits.sum(axis=1), np.ones(6, np.uint64))  # exactly one GGSW of a group encrypts 1
    groups = sk.reshape(6, g).astype(np.int64)
    assert np.array_equal(bits[:, 0], np.prod(1 - groups, axis=1).astype(np.uint64))  # idx 0: prod (1 - s)
    assert bits[0, 0] == 1 and bits[1, (1 << g) - 1] == 1
    for i in range(6):  # the GGSW that encrypts 1 selects exactly the key bits that are set
        idx = int(np.argmax(bits[i]))
        assert MB.selection_bits(idx, g) == groups[i].tolist()


def test_degree_rule_corners():
    two = lambda a, b: MB.group_degrees(np.array([a, b], np.uint64), 2)
    # idx 3 selects both elements, idx 2 the first (m = 0), idx 1 the second
    assert two(2**63, 2**63).tolist() == [0, 2048, 2048, 0]       # the sum wraps 2^64
    assert two(2**50, 2**50).tolist() == [0, 0, 0, 1]             # 2^51 is the tie: the sum switches to 1 ...
    assert int(F.modulus_switch(np.uint64(2**50), 12)) == 0       # ... where per-element switching gives 0 + 0
    assert two(2**51, 0).tolist() == [0, 0, 1, 1]                 # a sum of exactly 2^51
    assert two(2**51 - 1, 0).tolist() == [0, 0, 0, 0]
    assert two(2**64 - 2**51, 0).tolist() == [0, 0, 0, 0]         # rounds up to 2N = 0
    assert two(2**64 - 2**51 - 1, 0).tolist() == [0, 0, 4095, 4095]
    d = MB.group_degrees(np.array([1 << 52, 2 << 52, 4 << 52], np.uint64), 3).tolist()
    assert d == [0, 4, 2, 6, 1, 5, 3, 7]                          # bit_m(idx) = (idx >> (g - 1 - m)) & 1


def test_integer_bundle_is_a_signed_rotation():
    rng = H.rng(7)
    grp = H.uniform_u64(rng, (4, 1, 2, 2, N))
    deg = np.array([0, 5, 2048 + 7, 4095])
    got = MB.integer_bundle(grp, deg)
    with np.errstate(over="ignore"):
        want = grp[0] + np.roll(grp[1], 5, axis=-1) * np.where(np.arange(N) < 5, np.uint64(2**64 - 1), np.uint64(1))
        r2 = np.roll(grp[2], 7, axis=-1) * np.where(np.arange(N) < 7, np.uint64(2**64 - 1), np.uint64(1))
        want = want - r2
        r3 = np.roll(grp[3], -1, axis=-1) * np.where(np.arange(N) < N - 1, np.uint64(1), np.uint64(2**64 - 1))
        want = want + r3  # X^4095 = X^-1: p[j + 1] at j, -p[0] at N - 1
    assert np.array_equal(got, want)


@pytest.mark.parametrize("g", [2, 3, 4])
def test_restatement_decrypts(g):
    """N = 2048, k = 1, B = 2^22, l = 1, n = 24: every output of the numpy multi-bit PBS decodes to f(m)."""
    n_lwe, base_log, level, msg_mod = 24, 22, 1, 4
    delta = (1 << 63) // msg_mod
    rng = H.rng(2400 + g)
    lwe_sk = H.binary_key(rng, n_lwe)
    glwe_sk = H.binary_key(rng, (1, N))
    bsk = MB.multi_bit_bsk_gen(rng, None, lwe_sk, glwe_sk, base_log, level, 17, g)
    f = lambda x: (3 * x + 1) % msg_mod
    lut = H.pbs_lut(N, 1, msg_mod, delta, f)
    msgs = np.arange(6) % msg_mod
    lwe = H.lwe_encrypt_batch(rng, msgs.astype(np.uint64) * np.uint64(delta), lwe_sk, 45)
    out = MB.multi_bit_pbs(lwe, lut, F.forward_as_torus(bsk), base_log, level, g)
    pts = H.lwe_decrypt_batch(out, H.glwe_sk_as_lwe_sk(glwe_sk))
    with np.errstate(over="ignore"):
        dec = ((pts + np.uint64(delta // 2)) // np.uint64(delta)) % np.uint64(2 * msg_mod)
    assert list(dec) == [f(int(m)) for m in msgs]
