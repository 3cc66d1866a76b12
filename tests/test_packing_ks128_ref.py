"""Host checks of the references of the 128-bit packing keyswitch and compression (tests/packing128_helpers.py): the
vectorised reference against the statement-by-statement transcription, the transcription against the u64 one, the
mutant without pre-rounding, and the big-integer restatement of PackedIntegers<u128> against the Rust's own loop and
against the u64 packer.  No GPU."""
import numpy as np
import pytest

import packing128_helpers as Q
import packing_helpers as P
import pbs128_helpers as R
import tfhe_helpers as H

SHAPES = [(61, 1), (24, 3), (4, 3), (7, 2), (8, 1), (63, 2)]  # (base_log, level)


def _inputs(seed, in_dim, k, n, level, n_lwe, base_log):
    g = R.rng(seed)
    size = (k + 1) * n
    pksk = [[R.uniform_u128(g, size) for _ in range(level)] for _ in range(in_dim)]
    lwe = [R.uniform_u128(g, in_dim + 1) for _ in range(n_lwe)]
    ties = Q.tie_words128(base_log, level)
    for j, w in enumerate(ties):  # the corners spread over the ciphertexts' masks
        lwe[j % n_lwe][(j // n_lwe) % in_dim] = w
    return pksk, lwe


@pytest.mark.parametrize("base_log,level", SHAPES)
def test_vectorised_reference_equals_transcription(base_log, level):
    in_dim, k, n, per, n_lwe = 5, 2, 8, 3, 7
    pksk, lwe = _inputs(base_log * 10 + level, in_dim, k, n, level, n_lwe, base_log)
    key_words = R.to_words(pksk).reshape(in_dim, level, k + 1, n, 2)
    got = Q.packing_keyswitch128_ref(key_words, R.to_words(lwe), k, n, base_log, level, per)
    assert got.shape == (3, k + 1, n, 2)
    for gi in range(3):
        want = Q.packing_keyswitch128_transcription(pksk, lwe[gi * per:(gi + 1) * per], k, n, base_log, level)
        assert R.from_words(got[gi].reshape(-1, 2)) == want


@pytest.mark.parametrize("base_log,level", [(4, 3), (7, 2), (8, 1), (24, 2), (61, 1)])
def test_transcription_agrees_with_the_u64_one_on_top_words(oracle, base_log, level):
    """A u64 word placed in the top half of a u128 decomposes to the same digits, so with key and ciphertexts shifted
    up by 64 bits the 128-bit transcription's top words are the u64 transcription's result."""
    in_dim, k, n, count = 4, 1, 8, 5
    g = H.rng(0x128 + base_log)
    pksk = H.uniform_u64(g, (in_dim, level, (k + 1) * n))
    lwe = H.uniform_u64(g, (count, in_dim + 1))
    lwe[0, :in_dim] = P.tie_words(base_log, level)[2:2 + in_dim]
    want = P.packing_keyswitch_transcription(oracle, pksk, lwe, k, n, base_log, level)
    up = lambda a: [[int(v) << 64 for v in row] for row in a]
    got = Q.packing_keyswitch128_transcription([up(block) for block in pksk], up(lwe), k, n, base_log, level)
    assert all(v & R.MASK64 == 0 for v in got)
    assert [v >> 64 for v in got] == [int(v) for v in want]


@pytest.mark.parametrize("base_log,level", SHAPES)
def test_mutant_without_pre_rounding_differs_on_the_ties(base_log, level):
    ties = Q.tie_words128(base_log, level)
    differs = [w for w in ties if Q.digits128(w, base_log, level) != Q.digits128(w, base_log, level, rounded=False)]
    # decompose(a) balances the tie state 2^(rep-1) when a's rounding bit is set, the pre-rounded word never has one:
    # the two differ exactly on [2^127 - step, 2^127 - 1], whose ends are in the corpus; 2^127 - step - 1 lies just
    # outside and pins the interval's edge
    step = 1 << (127 - base_log * level)
    assert differs == [(1 << 127) - 1, (1 << 127) - step]
    # and through the keyswitch: one ciphertext whose mask is the tie words
    in_dim, k, n = len(ties), 1, 4
    g = R.rng(base_log + 100 * level)
    pksk = [[R.uniform_u128(g, (k + 1) * n) for _ in range(level)] for _ in range(in_dim)]
    lwe = [ties + [12345]]
    good = Q.packing_keyswitch128_transcription(pksk, lwe, k, n, base_log, level)
    bad = Q.packing_keyswitch128_transcription(pksk, lwe, k, n, base_log, level, rounded=False)
    assert good != bad
    key_words = R.to_words(pksk).reshape(in_dim, level, k + 1, n, 2)
    mutant = Q.packing_keyswitch128_ref(key_words, R.to_words(lwe), k, n, base_log, level, 1, rounded=False)
    assert R.from_words(mutant[0].reshape(-1, 2)) == bad


@pytest.mark.parametrize("log_modulus", [1, 5, 12, 63, 64, 65, 100, 127, 128])
def test_pack128_ref_equals_the_rust_loop(log_modulus):
    g = R.rng(log_modulus)
    for count in (1, 2, 37, 128, 131):
        values = [v & ((1 << log_modulus) - 1) for v in R.uniform_u128(g, count)]
        values[0] = (1 << log_modulus) - 1
        packed = Q.pack128_ref(values, log_modulus)
        assert packed == Q.pack128_loop(values, log_modulus)
        assert Q.unpack128_ref(packed, count, log_modulus) == values


@pytest.mark.parametrize("log_modulus", [1, 12, 31, 63, 64])
def test_packed_words_are_the_u64_packer_s_padded_to_an_even_count(log_modulus):
    g = R.rng(0x40 + log_modulus)
    for count in (1, 3, 64, 77):
        values = [v & ((1 << log_modulus) - 1) for v in R.uniform_u128(g, count)]
        want = [int(w) for w in P.pack_ref(values, log_modulus)]
        want += [0] * (len(want) % 2)
        got = R.to_words(Q.pack128_ref(values, log_modulus)).reshape(-1)
        assert [int(w) for w in got] == want


def test_compress_extract_restatement_round_trip():
    k, n = 2, 8
    g = R.rng(9)
    glwe = R.uniform_u128(g, (k + 1) * n)
    for bodies in (0, 1, n):
        packed = Q.compress128_ref(glwe, k, n, bodies, 128)
        assert packed == glwe[:k * n + bodies]  # the production log_modulus: a copy of the kept words
        assert Q.extract128_ref(packed, k, n, bodies, 128) == glwe[:k * n + bodies] + [0] * (n - bodies)
        for log_modulus in (12, 65):
            back = Q.extract128_ref(Q.compress128_ref(glwe, k, n, bodies, log_modulus), k, n, bodies, log_modulus)
            want = [(Q.modulus_switch128(v, log_modulus) << (128 - log_modulus)) & R.MASK128
                    for v in glwe[:k * n + bodies]]
            assert back == want + [0] * (n - bodies)


def test_signed_byte_recoding_inverts():
    g = R.rng(3)
    for x in R.uniform_u128(g, 50) + [0, R.MASK128, 1 << 127, (1 << 127) - 1, 0x80 * ((1 << 128) // 255)]:
        b = Q.signed_bytes(x, 16)
        assert all(-128 <= s <= 127 for s in b) and Q.from_signed_bytes(b) == x
    for fill in (-128, 127):
        assert Q.signed_bytes(Q.from_signed_bytes([fill] * 16), 16) == [fill] * 16
