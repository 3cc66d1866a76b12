"""The packing keyswitch / compression references of packing_helpers.py, checked on the host (no GPU).

* the composed reference (oracle LWE keyswitch over the pre-rounded mask + monomial multiplications) equals the
  line-by-line transcription of lwe_packing_keyswitch.rs:102-187, 296-379 on tiny shapes;
* it differs from the composition without the pre-rounding on the mask word 2^63 - 1: the balanced-rounding tie of
  decompose(closest_representable(a)) is not decompose(a)'s;
* the big-integer pack equals the reference's loop (packed_integers.rs:89-121) and unpack inverts it;
* real keys: 256 messages packed, compressed at 12 bits, extracted, sample-extracted and decrypted.
"""
import numpy as np
import pytest

import packing_helpers as P
import tfhe_helpers as H


@pytest.mark.parametrize("in_dim,k,n,base_log,level,count", [
    (5, 1, 8, 4, 3, 8),     # full-degree rotation
    (3, 2, 4, 7, 2, 3),     # k = 2, fewer ciphertexts than N
    (6, 1, 8, 2, 5, 1),     # a single ciphertext: keyswitch_lwe_ciphertext_into_glwe_ciphertext
    (4, 1, 16, 10, 2, 11),
    (2, 3, 4, 21, 3, 4),    # rep = 63
])
def test_composed_reference_matches_transcription(oracle, in_dim, k, n, base_log, level, count):
    g = H.rng(in_dim * 131 + n + base_log)
    pksk = H.uniform_u64(g, (in_dim, level, (k + 1) * n))
    lwe = H.uniform_u64(g, (count, in_dim + 1))
    flat = lwe[:, :in_dim].reshape(-1)
    ties = P.tie_words(base_log, level)[:flat.size]
    flat[:len(ties)] = ties
    lwe[:, :in_dim] = flat.reshape(count, in_dim)
    want = P.packing_keyswitch_transcription(oracle, pksk, lwe, k, n, base_log, level)
    got = P.packing_keyswitch_ref(oracle, pksk, lwe, k, n, base_log, level, count)
    assert got.shape == (1, k + 1, n)
    assert np.array_equal(got.reshape(-1), want)


def test_pre_rounding_changes_the_tie(oracle):
    """a = 2^63 - 1 at rep = 12: decompose(a) balances the state 2^11 (rounding bit 1), decompose(closest_
    representable(a)) does not (rounding bit 0), so the digit chains and the outputs differ."""
    in_dim, k, n, base_log, level = 1, 1, 4, 4, 3
    g = H.rng(0x7e1)
    pksk = H.uniform_u64(g, (in_dim, level, (k + 1) * n))
    lwe = np.array([[(1 << 63) - 1, 12345]], dtype=np.uint64)
    want = P.packing_keyswitch_transcription(oracle, pksk, lwe, k, n, base_log, level)
    rounded = P.packing_keyswitch_ref(oracle, pksk, lwe, k, n, base_log, level, 1).reshape(-1)
    plain = P.packing_keyswitch_ref(oracle, pksk, lwe, k, n, base_log, level, 1, rounded=False).reshape(-1)
    assert np.array_equal(rounded, want)
    assert not np.array_equal(plain, want)
    # away from the tie the two compositions agree
    lwe[0, 0] = (1 << 63) - (1 << 51) - 1
    assert np.array_equal(P.packing_keyswitch_ref(oracle, pksk, lwe, k, n, base_log, level, 1),
                          P.packing_keyswitch_ref(oracle, pksk, lwe, k, n, base_log, level, 1, rounded=False))


@pytest.mark.parametrize("log_modulus", [1, 5, 12, 13, 31, 63, 64])
def test_pack_restatement_matches_the_reference_loop(oracle, log_modulus):
    g = H.rng(log_modulus)
    for count in (1, 7, 64, 129):
        vals = [oracle.modulus_switch(int(v), log_modulus) for v in H.uniform_u64(g, count)]
        packed = P.pack_ref(vals, log_modulus)
        assert np.array_equal(packed, P.pack_loop(vals, log_modulus))
        assert P.unpack_ref(packed, count, log_modulus) == vals


def test_real_keys_pack_compress_extract_decrypt(oracle):
    """256 LWE encryptions -> one GLWE by the packing keyswitch -> compressed at 12 bits -> extracted -> sample
    extraction of coefficient d -> decrypts to message d."""
    in_dim, k, n, base_log, level, log_modulus = 48, 1, 256, 8, 3, 12
    msg_mod, delta = 8, 1 << 60
    g = H.rng(0x9ac)
    in_sk = H.binary_key(g, in_dim)
    glwe_sk = H.binary_key(g, (k, n))
    pksk = P.pksk_gen(g, in_sk, glwe_sk, base_log, level, noise_log2=10)
    msgs = g.integers(0, msg_mod, size=n, dtype=np.uint64)
    lwe = H.lwe_encrypt_batch(g, msgs * np.uint64(delta), in_sk, noise_log2=10)
    packed_glwe = P.packing_keyswitch_ref(oracle, pksk, lwe, k, n, base_log, level, n)[0]
    words = P.compress_ref(oracle, packed_glwe, k, n, n, log_modulus)
    assert words.size == ((k + 1) * n * log_modulus + 63) // 64
    glwe = P.extract_ref(words, k, n, n, log_modulus)
    big_sk = H.glwe_sk_as_lwe_sk(glwe_sk)
    got = [H.decode(H.lwe_decrypt(oracle.sample_extract_nth(glwe, n, k, d), big_sk), delta, msg_mod)
           for d in range(n)]
    assert got == [int(m) for m in msgs]
