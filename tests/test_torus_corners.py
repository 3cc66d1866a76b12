"""The conversion corner corpus on the host (tests/torus_corners.py): the Fraction model against the numpy restatement's
from_torus, the host models of the device functions against the contract in numbers, and the corpus's power: every
one-off mutant of a conversion differs from the true function somewhere on it.  The device side is
tests/test_torus_corners_gpu.py."""
import math

import numpy as np
import pytest

import fft_oracle as F
import torus_corners as C


def test_fraction_model_matches_oracle_from_torus():
    vals = C.add_torus_values()
    got = F.from_torus(np.array(vals, np.float64))
    for t, g in zip(vals, got):
        assert int(g) == C.ref_from_torus(t), t
    # the two classes the reference itself singles out: ties away from zero, and +1/2 saturating to i64::MAX
    assert C.ref_from_torus(0.5) == 1 << 63 and C.ref_from_torus(-0.5) == (1 << 63) - 1
    assert C.ref_from_torus(1.5 * 2.0 ** -64) == 2 and C.ref_from_torus(2.5 * 2.0 ** -64) == 3
    assert C.ref_from_torus(-2.5 * 2.0 ** -64) == C.M64 - 3 and C.ref_from_torus(2.0 ** -65) == 1


def test_forward_model_is_the_correctly_rounded_signed_cast():
    words = C.forward_words()
    for x in words:
        assert C.model_s64_to_f64(x) == C.ref_s64_to_f64(x)
    # numpy's own cast agrees (the restatement's _signed)
    a = np.array(words, np.uint64).view(np.int64).astype(np.float64)
    assert a.tolist() == [C.ref_s64_to_f64(x) for x in words]
    # ties to even: 2^53 + 1 -> 2^53, 2^53 + 3 -> 2^53 + 4, 2^54 + 2 -> 2^54, 2^54 + 6 -> 2^54 + 8
    assert [C.ref_s64_to_f64(x) for x in ((1 << 53) + 1, (1 << 53) + 3, (1 << 54) + 2, (1 << 54) + 6)] == [
        2.0 ** 53, 2.0 ** 53 + 4, 2.0 ** 54, 2.0 ** 54 + 8]
    assert C.ref_s64_to_f64((1 << 63) - 1) == 2.0 ** 63 and C.ref_s64_to_f64(1 << 63) == -(2.0 ** 63)
    assert C.ref_s64_to_f64(C.M64 - 1) == -1.0


def test_torus_words_model_meets_its_contract():
    """from_torus_scaled = round-half-even of t 2^64 mod 2^64: the reference's word outside the two documented
    classes, the nearest even word on exact halves, 2^63 on fract = +1/2."""
    n_half = n_plus = 0
    for t in C.add_torus_values():
        got = C.model_torus_words(t * 2.0 ** 64)
        assert got == C.expected_backward(t), t
        ref = C.ref_from_torus(t)
        if C.fract_is_plus_half(t):
            assert got == 1 << 63 and ref == (1 << 63) - 1
            n_plus += 1
        elif C.is_half(t):
            assert got % 2 == 0 and C.word_distance(got, ref) <= 1, t
            n_half += 1
        else:
            assert got == ref, t
    assert n_half >= 12 and n_plus >= 3


def test_add_torus_model_meets_its_contract():
    """add_torus: exact equality where fft64_device.hpp says exact, within 2^11 of the reference elsewhere, exactly 2^32
    below it on the dropped carry; every class of the contract occurs in the corpus."""
    seen = {}
    for t in C.add_torus_values():
        cls = C.add_torus_class(t)
        seen[cls] = seen.get(cls, 0) + 1
        word, slack = C.expected_add_torus(t)
        ref = C.ref_from_torus(t)
        for acc in C.ACCUMULATORS + (0x00000000FFFFFFFF, 0x123456789ABCDEF0):
            got = (C.model_add_torus(acc, t) - acc) % C.M64
            assert C.word_distance(got, word) <= slack, (t, acc, cls)
            if cls == "carry":
                assert (ref - got) % C.M64 == 1 << 32, t
            else:
                assert C.word_distance(got, ref) <= 1 << 11, (t, cls)
            if cls == "exact":
                assert got == ref
    assert all(seen.get(c, 0) >= 3 for c in ("exact", "plus_half", "round", "carry", "neg_small")), seen


def test_add_torus_classes_are_as_narrow_as_stated():
    """Values just outside each class are exact, and inside each class the deviation is real (the class is not
    wider than it has to be, nor the contract looser than the function)."""
    up, dn = (lambda v: math.nextafter(v, math.inf)), (lambda v: math.nextafter(v, -math.inf))
    d = lambda t: C.word_distance(C.model_add_torus(0, t), C.ref_from_torus(t))
    # the fraction of a negative t in (-1/2, 0): -0.3 = -(0x1.3333333333333p-2) has its last bit set
    assert C.add_torus_class(-0.3) == "neg_small" and 0 < d(-0.3) <= 1 << 10
    assert C.add_torus_class(-0.25) == "exact" and d(-0.25) == 0
    assert C.add_torus_class(-0.5 - 2.0 ** -53) == "exact" and d(dn(-0.5)) == 0
    assert C.add_torus_class(up(-0.5)) == "neg_small" and d(up(-0.5)) == 1 << 10   # a tie of 1 + t, to even
    assert d(-(2.0 ** -100)) == 1 << 11 and d(-(2.0 ** -54)) == 1 << 10 and d(-(2.0 ** -53)) == 0
    assert C.model_add_torus(0, -(2.0 ** -100)) == C.M64 - (1 << 11)
    # the carry: [2^32 - 1/2, 2^32) of the low word
    assert C.add_torus_class(2.0 ** -32 - 2.0 ** -66) == "carry" and C.model_add_torus(0, 2.0 ** -32 - 2.0 ** -66) == 0
    assert C.add_torus_class(2.0 ** -32 - 2.0 ** -65) == "carry"
    assert C.add_torus_class(2.0 ** -32 - 3 * 2.0 ** -66) == "round" and d(2.0 ** -32 - 3 * 2.0 ** -66) == 0
    assert C.add_torus_class(2.0 ** -32 - 2.0 ** -64) == "exact"
    # rounding below 2^-12: halves with an even floor differ by one; the last double below 2^-12 is a half whose low
    # word is 2^32 - 1/2 (the carry); 2^-12 and above are integers
    assert C.add_torus_class(C.TINY - 3 * 2.0 ** -65) == "round" and d(C.TINY - 3 * 2.0 ** -65) == 1
    assert C.add_torus_class(dn(C.TINY)) == "carry" and C.add_torus_class(dn(dn(C.TINY))) == "exact"
    assert C.add_torus_class(C.TINY) == "exact" and C.add_torus_class(up(C.TINY)) == "exact"
    # fract = +1/2
    assert C.add_torus_class(-0.5) == "plus_half" and C.model_add_torus(0, -0.5) == 1 << 63
    assert C.add_torus_class(0.5) == "exact" and C.model_add_torus(0, 0.5) == 1 << 63 == C.ref_from_torus(0.5)


@pytest.mark.parametrize("name", list(C.MUTANTS))
def test_corpus_separates_mutant(name):
    kind, fn = C.MUTANTS[name]
    if kind == "forward":
        hits = [x for x in C.forward_words() if fn(x) != C.model_s64_to_f64(x)]
    elif kind == "words":
        hits = [t for t in C.backward_values() if fn(t * 2.0 ** 64) != C.model_torus_words(t * 2.0 ** 64)]
    else:
        hits = [(t, a) for t in C.add_torus_values() for a in C.ACCUMULATORS
                if fn(a, t) != C.model_add_torus(a, t)]
    assert hits, name
    # the fixed part of each corpus alone separates it (not only a lucky random draw)
    if kind == "forward":
        assert any(fn(x) != C.model_s64_to_f64(x) for x in C.forward_words(n_random=0)[:17])
    elif kind == "words":
        assert any(fn(t * 2.0 ** 64) != C.model_torus_words(t * 2.0 ** 64) for t in C.backward_values(n_random=0))
    else:
        assert any(fn(a, t) != C.model_add_torus(a, t) for t in C.add_torus_values(n_random=0) for a in C.ACCUMULATORS)


def test_mutants_are_one_off():
    """Each mutant agrees with the true function on most of the corpus: it is the corners that tell them apart."""
    for name, (kind, fn) in C.MUTANTS.items():
        if kind == "words":
            vals = [t for t in C.backward_values() if abs(t) < 0.4 and not C.is_half(t) and abs(t) >= 2.0 ** -11]
            assert vals and all(fn(t * 2.0 ** 64) == C.model_torus_words(t * 2.0 ** 64) for t in vals), name
