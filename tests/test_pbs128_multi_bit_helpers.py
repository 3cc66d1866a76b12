"""tests/pbs128_multi_bit_helpers.py against itself, and the limb rule of ``mi_pbs128_multi_bit_limb_plan`` (no device).

* the word form of the bundle equals the Python-integer form;
* one step on a noise-free gadget key of known key bits is the accumulator rotated by the degree of the set-bit subset,
  for every key-bit pattern of every grouping factor;
* the mutant that switches each mask element before summing is told apart on the degree corpus: where every element
  lies just under half a switching unit its degrees and its step result differ from the true ones;
* the limb rule in big integers against the ABI's, and the production figures."""
import ctypes
import itertools

import numpy as np
import pytest

import pbs128_helpers as R
import pbs128_multi_bit_helpers as H

PRODUCTION = (2048, 2, 23, 3, 4)  # N, k, base_log, level, grouping factor


@pytest.mark.parametrize("g", [2, 3, 4])
def test_bundle_words_equal_the_integer_bundle(g):
    n, k, level = 16, 1, 2
    rng = R.rng(40 + g)
    words = H.uniform_key_words(rng, 1, g, k, n, level)[0]
    degrees = [0] + [int(v) for v in rng.integers(0, 2 * n, size=(1 << g) - 1)]
    degrees[1:4] = [0, n, 2 * n - 1][:min(3, (1 << g) - 1)]
    assert R.from_words(H.bundle_words(words, degrees)) == H.bundle(R.from_words(words), degrees)


@pytest.mark.parametrize("g", [2, 3, 4])
def test_gadget_step_rotates_by_the_set_bit_subset(g):
    n, k, base_log, level = 64, 1, 23, 2
    rng = R.rng(50 + g)
    log_mod = n.bit_length()
    acc = R.uniform_glwe(rng, k, n)
    rounded = [[R.closest_representable(x, base_log, level) for x in p] for p in acc]
    for bits in itertools.product((0, 1), repeat=g):
        mask = [int(v) for v in rng.integers(0, R.M64, size=g, dtype=np.uint64)]
        words = H.key_words(H.gadget_key(list(bits), k, n, base_log, level, g))[0]
        sel = H.selected_index(bits)
        assert [int(any(x for x in R.from_words(words[idx])[0][0][0])) for idx in range(1 << g)] == \
            [int(idx == sel) for idx in range(1 << g)]
        degree = R.modulus_switch(sum(a for a, b in zip(mask, bits) if b) & R.MASK64, log_mod) % (2 * n)
        assert H.subset_degrees(mask, g, log_mod)[sel] == degree
        assert H.step(acc, mask, words, base_log, level, g) == [R.monomial_mul(p, degree) for p in rounded]


@pytest.mark.parametrize("g", [2, 3, 4])
def test_per_element_mutant_is_told_apart(g):
    n, k, base_log, level = 64, 1, 23, 1
    rng = R.rng(60 + g)
    log_mod = n.bit_length()
    groups, first_half = H.corner_mask_groups(g, n, rng)
    seen = set()
    for mask in groups:
        seen |= set(H.subset_degrees(mask, g, log_mod))
    assert {0, 1, n - 1, n, n + 1, 2 * n - 1} <= seen
    words = H.uniform_key_words(rng, 1, g, k, n, level)[0]
    acc = R.uniform_glwe(rng, k, n)
    for mask in groups[first_half:]:
        true, mutant = H.subset_degrees(mask, g, log_mod), H.per_element_degrees(mask, g, log_mod)
        assert all(v == 0 for v in mutant), "every element alone switches to 0"
        assert all(true[idx] != 0 for idx in range(1, 1 << g) if bin(idx).count("1") >= 2)
        assert H.step(acc, mask, words, base_log, level, g) != \
            H.step(acc, mask, words, base_log, level, g, degrees=H.per_element_degrees)


def test_limb_rule(engine):
    from tfhe_ntt_amd import _lib

    n, k, base_log, level, _ = PRODUCTION
    assert H.limb_rule(n, k, base_log, level, 4) == (22, 6)
    assert 144 * (1 << 33) * ((1 << 22) - 1) <= (R.P - 1) // 2 < 144 * (1 << 33) * ((1 << 23) - 1)
    for g in (2, 3, 4):
        assert engine.pbs128.multi_bit_limb_plan(n, k, base_log, level, g) == H.limb_rule(n, k, base_log, level, g)
    for shape in [(256, 1, 23, 1), (512, 3, 16, 4), (2048, 1, 42, 3), (1024, 2, 10, 5), (4096, 1, 30, 2)]:
        for g in (2, 3, 4):
            want = H.limb_rule(*shape, g)
            w, nl = ctypes.c_int(-1), ctypes.c_int(-1)
            st = _lib.lib().mi_pbs128_multi_bit_limb_plan(*shape, g, ctypes.byref(w), ctypes.byref(nl))
            assert (w.value, nl.value) == want, (shape, g)
            assert st == (_lib.MI_OK if 0 < want[1] <= 32 else _lib.MI_ERR_UNSUPPORTED), (shape, g)
    # the classic rule is the multi-bit one at 2^0 GGSWs per column, and is left as it was
    assert engine.pbs128.limb_plan(n, k, 24, 3) == R.limb_rule(n, k, 24, 3) == (25, 6)
    L = _lib.lib()
    for g in (0, 1, 5, -1):
        assert L.mi_pbs128_multi_bit_limb_plan(n, k, base_log, level, g, None, None) == _lib.MI_ERR_INVALID_ARG
        assert L.mi_last_error_message() == b"grouping factor must be 2, 3 or 4"
    assert L.mi_pbs128_multi_bit_limb_plan(n + 1, k, base_log, level, 4, None, None) == _lib.MI_ERR_INVALID_ARG
    assert L.mi_pbs128_multi_bit_limb_plan(n, k, 43, 3, 4, None, None) == _lib.MI_ERR_INVALID_ARG
    # a column of 2^g GGSWs leaves up to 4 bits less per limb, so the multi-bit plan stops at 32 limbs where the classic
    # one stops at 16: a shape the classic plan takes at its 16 limbs is taken here too
    assert engine.pbs128.limb_plan(2048, 1, 42, 3) == (8, 16)
    assert engine.pbs128.multi_bit_limb_plan(2048, 1, 42, 3, 2) == (6, 22)
    assert engine.pbs128.multi_bit_limb_plan(2048, 1, 42, 3, 4) == (4, 32)
    w, nl = ctypes.c_int(-1), ctypes.c_int(-1)  # more limbs than that: the outputs are still written
    assert L.mi_pbs128_multi_bit_limb_plan(n, k, 45, 2, 4, ctypes.byref(w), ctypes.byref(nl)) == _lib.MI_ERR_UNSUPPORTED
    assert L.mi_last_error_message() == b"the multi-bit limb plan needs more than 32 limbs"
    assert (w.value, nl.value) == H.limb_rule(n, k, 45, 2, 4) and nl.value > 32
