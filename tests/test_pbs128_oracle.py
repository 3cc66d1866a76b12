"""The host side of the 128-bit bootstrap: the Python-integer restatement (tests/pbs128_helpers.py) against an
independent schoolbook and against itself, the limb rule of ``mi_pbs128_limb_plan``, and the entry points' argument
validation.  No GPU: the limb plan and every rejection answer before any device call."""
import ctypes

import pytest

import native_oracle
import pbs128_helpers as H

SHAPES = [(23, 1), (24, 3), (16, 4), (8, 15), (1, 1), (42, 3), (64, 1), (63, 2), (127, 1), (9, 7)]  # (base_log, level)


def _saturating_pairs(n, base_log, level):
    """(digit polynomial, key polynomial) pairs of the saturating input: every reachable digit extreme against a key of
    2^128 - 1 and against a key with one limb of 2^25 - 1."""
    pairs = []
    for kind in ("plus", "minus", "index0"):
        poly = H.saturating_poly(base_log, level, n, kind)
        for li in range(level):
            digits = [H.py_decompose(x, base_log, level)[li] & H.MASK128 for x in poly]
            pairs += [(digits, [H.MASK128] * n), (digits, [((1 << 25) - 1) << 50] * n)]
    return pairs


@pytest.mark.parametrize("n", [16, 32])
def test_product_equals_schoolbook(n):
    g = H.rng(100 + n)
    pairs = [(H.uniform_u128(g, n), H.uniform_u128(g, n)) for _ in range(4)] + _saturating_pairs(n, 24, 3)
    for a, b in pairs:
        assert H.negacyclic_mul(a, b) == [int(v) for v in native_oracle.schoolbook(a, b, 128)]


@pytest.mark.parametrize("n,k,base_log,level", [(16, 1, 23, 1), (32, 2, 24, 3), (16, 1, 42, 3)])
def test_external_product_equals_schoolbook(n, k, base_log, level):
    """Both forms of the column sums (packed big integers; the compiled loops) against sums of schoolbook products, on
    random inputs and on the saturating ones."""
    g = H.rng(7 * n + base_log)
    ggsws = [H.uniform_ggsw(g, k, n, level), [[[[H.MASK128] * n] * (k + 1)] * (k + 1)] * level]
    glwes = [H.uniform_glwe(g, k, n)] + [[H.saturating_poly(base_log, level, n, kind)] * (k + 1)
                                         for kind in ("plus", "minus", "index0")]
    for ggsw in ggsws:
        packed = H.PackedGgsw(ggsw, base_log)
        for glwe in glwes:
            digits = H.decompose_glwe(glwe, base_log, level)
            want = []
            for c in range(k + 1):
                acc = [0] * n
                for li in range(level):
                    for r in range(k + 1):
                        prod = native_oracle.schoolbook([d & H.MASK128 for d in digits[li][r]], ggsw[li][r][c], 128)
                        acc = [(x + int(y)) & H.MASK128 for x, y in zip(acc, prod)]
                want.append(acc)
            assert packed.column_sums(digits) == want
            assert H.accelerator() is not None, "the suite runs where build() ran: a C compiler is there"
            assert H.fast_external_sums(packed, glwe, level) == want


@pytest.mark.parametrize("base_log,level", SHAPES)
def test_decomposer_forms_agree_and_recompose(base_log, level):
    g = H.rng(base_log * 131 + level)
    words = H.corner_words(base_log, level) + H.uniform_u128(g, 300)
    bound = 1 << (base_log - 1)
    for x in words:
        terms = H.py_decompose(x, base_log, level)
        assert terms == H.py_decompose_split(x, base_log, level), hex(x)
        assert H.recompose(terms, base_log, level) == H.closest_representable(x, base_log, level), hex(x)
        assert all(-bound <= t <= bound for t in terms), hex(x)


@pytest.mark.parametrize("base_log,level", [s for s in SHAPES if s[0] <= 63])
def test_compiled_decomposition_equals_python(base_log, level):
    import numpy as np

    lib = H.accelerator()
    assert lib is not None, "the suite runs where build() ran: a C compiler is there"
    g = H.rng(base_log * 17 + level)
    words = H.corner_words(base_log, level) + H.uniform_u128(g, 300)
    w = np.ascontiguousarray(H.to_words(words))
    digits = np.empty((level, len(words)), np.int64)
    lib.pbs128_decompose(digits.ctypes.data, w.ctypes.data, len(words), base_log, level, 2)
    assert digits.T.tolist() == [H.py_decompose(x, base_log, level) for x in words]


def test_corpus_holds_its_corners():
    """The corpus really contains what its name promises, for base_log * level below and above 64."""
    for base_log, level in [(23, 1), (16, 3), (24, 3), (42, 3)]:
        words = H.corner_words(base_log, level)
        rep, top = base_log * level, 1 << (base_log - 1)
        half = 1 << (128 - rep - 1)
        assert {0, 1 << 127, H.MASK128, half, half - 1} <= set(words)
        digit_sets = [set() for _ in range(level)]
        for x in words:
            for li, t in enumerate(H.py_decompose(x, base_log, level)):
                digit_sets[li].add(t)
        assert all({top, -top} <= s for s in digit_sets), (base_log, level)
        # a rounding carry that crosses bit 64: the low word all ones above the tie, the high word changes
        if half < H.M64:
            assert any((x & H.MASK64) >= H.M64 - half and
                       (H.closest_representable(x, base_log, level) >> 64) != (x >> 64) for x in words)
        # a digit field that straddles the word boundary exists exactly when a field boundary is not at bit 64
        if any(128 - rep + j * base_log < 64 < 128 - rep + (j + 1) * base_log for j in range(level)):
            j = next(j for j in range(level) if 128 - rep + j * base_log < 64 < 128 - rep + (j + 1) * base_log)
            lo_bit = 128 - rep + j * base_log
            assert (((1 << base_log) - 1) << lo_bit) in words
    for base_log, level in [(23, 1), (24, 3), (42, 3)]:
        for negative in (False, True):
            x = H.saturating_word(base_log, level, negative)
            assert H.py_decompose(x, base_log, level) == H.saturating_digits(base_log, level, negative)


def test_monomials_and_extraction():
    g = H.rng(5)
    n = 16
    p = H.uniform_u128(g, n)
    x = [0, 1] + [0] * (n - 2)
    for d in (0, 1, n - 1, n, 2 * n - 1, 7):
        mono = [0] * n
        mono[d % n] = 1 if d < n else H.MASK128
        assert H.monomial_mul(p, d) == H.negacyclic_mul(p, mono)
        assert H.monomial_mul(H.monomial_div(p, d), d) == p
    assert H.monomial_mul(p, 1) == H.negacyclic_mul(p, x)


def _limb_plan(engine, n, k, base_log, level):
    from tfhe_ntt_amd import _lib

    w, nl = ctypes.c_int(-1), ctypes.c_int(-1)
    st = _lib.lib().mi_pbs128_limb_plan(n, k, base_log, level, ctypes.byref(w), ctypes.byref(nl))
    return st, w.value, nl.value


def test_limb_plan_rule(engine):
    from tfhe_ntt_amd import _lib

    half = (H.P - 1) // 2
    seen = {}
    for n in (256, 512, 1024, 2048, 4096):
        for k in (1, 2, 3):
            for base_log, level in [(23, 1), (24, 3), (16, 4), (8, 15), (1, 1), (42, 3)]:
                st, w, nl = _limb_plan(engine, n, k, base_log, level)
                d = (k + 1) * level * n * (1 << (base_log - 1))
                # the rule, both sides in Python integers: w fits, w + 1 does not
                assert w == 0 or d * ((1 << w) - 1) <= half, (n, k, base_log, level)
                assert d * ((1 << (w + 1)) - 1) > half, (n, k, base_log, level)
                assert (w, nl) == H.limb_rule(n, k, base_log, level)
                assert nl == (-(-128 // w) if w else 0)
                assert st == (_lib.MI_OK if 1 <= nl <= 16 else _lib.MI_ERR_UNSUPPORTED), (n, k, base_log, level)
                if st != _lib.MI_OK:
                    assert _lib.lib().mi_last_error_message() == b"the limb plan needs more than 16 limbs"
                seen[(n, k, base_log, level)] = (w, nl)
    assert seen[(2048, 2, 24, 3)] == (25, 6)
    assert seen[(2048, 1, 23, 1)] == (29, 5)
    assert engine.pbs128.limb_plan(2048, 2, 24, 3) == (25, 6)
    assert _lib.lib().mi_pbs128_limb_plan(2048, 2, 24, 3, None, None) == _lib.MI_OK


_POW2 = "polynomial size must be a power of two"
_GLWE = "glwe dimension must be >= 1"
_DECOMP = "decomposition base_log * level must be in [1, 127]"


@pytest.mark.parametrize("args,message", [
    ((0, 1, 23, 1), _POW2), ((48, 1, 23, 1), _POW2), ((2049, 1, 23, 1), _POW2),
    ((1 << 32, 1, 23, 1), "polynomial size must be at most 2^31"),
    ((2048, 0, 23, 1), _GLWE), ((2048, -1, 23, 1), _GLWE),
    ((2048, 65536, 23, 1), "glwe dimension must be at most 65535"),
    ((2048, 1, 0, 1), _DECOMP), ((2048, 1, 23, 0), _DECOMP), ((2048, 1, 64, 2), _DECOMP), ((2048, 1, 43, 3), _DECOMP),
    ((2048, 1, 128, 1), _DECOMP),
    ((48, 0, 0, 0), _POW2), ((2048, 0, 0, 0), _GLWE),  # the first failing rule answers
])
def test_limb_plan_invalid_arguments(engine, args, message):
    from tfhe_ntt_amd import _lib

    st, w, nl = _limb_plan(engine, *args)
    assert (st, _lib.lib().mi_last_error_message().decode()) == (_lib.MI_ERR_INVALID_ARG, message)
    assert (w, nl) == (-1, -1)  # nothing written


def test_limb_plan_unsupported(engine):
    from tfhe_ntt_amd import _lib

    for args in [(4096, 3, 42, 3), (2048, 1, 60, 2), (1 << 20, 1, 50, 1)]:
        st, w, nl = _limb_plan(engine, *args)
        assert (st, _lib.lib().mi_last_error_message()) == (_lib.MI_ERR_UNSUPPORTED,
                                                            b"the limb plan needs more than 16 limbs")
        assert (w, nl) == H.limb_rule(*args)


def test_key_create_rejections_before_any_device_call(engine):
    """The create's rules that need no plan: the handle stays NULL and each returns its message."""
    from tfhe_ntt_amd import _lib

    L = _lib.lib()
    INVALID = _lib.MI_ERR_INVALID_ARG
    words = (ctypes.c_uint64 * 4)()  # never dereferenced
    bsk = ctypes.addressof(words)
    plan = ctypes.addressof(words)  # stands for a non-NULL plan in the rules that come before it is read
    h = ctypes.c_void_p()
    assert L.mi_pbs128_key_create(plan, bsk, 8, 2, 2048, 24, 3, None, None) == INVALID
    assert L.mi_last_error_message() == b"out_key is NULL"
    for args, message in [((None, bsk, 8, 2, 2048, 24, 3), "plan is NULL"),
                          ((plan, None, 8, 2, 2048, 24, 3), "bsk_std is NULL"),
                          ((plan, bsk, 0, 2, 2048, 24, 3), "lwe dimension out of range"),
                          ((plan, bsk, 1 << 24, 2, 2048, 24, 3), "lwe dimension out of range"),
                          ((plan, bsk, 8, 2, 2000, 24, 3), _POW2),
                          ((plan, bsk, 8, 0, 2048, 24, 3), _GLWE),
                          ((plan, bsk, 8, 2, 2048, 64, 2), _DECOMP)]:
        st = L.mi_pbs128_key_create(*args, None, ctypes.byref(h))
        assert (st, L.mi_last_error_message().decode()) == (INVALID, message), args
        assert not h.value


def test_pbs128_null_handles(engine):
    from tfhe_ntt_amd import _lib

    L = _lib.lib()

    def other_error():  # so that the message read next is the following call's own
        assert L.mi_pbs128_key_create(None, None, 8, 2, 2048, 24, 3, None, None) == _lib.MI_ERR_INVALID_ARG
        assert L.mi_last_error_message() == b"out_key is NULL"

    assert L.mi_pbs128_key_destroy(None) == _lib.MI_OK
    for call in (lambda: L.mi_pbs128_key_info(None, *[None] * 7),
                 lambda: L.mi_ext_product128_batch(None, 0, None, None, 1, None),
                 lambda: L.mi_cmux128_batch(None, 0, None, None, 1, None),
                 lambda: L.mi_blind_rotate128_batch(None, None, None, 1, 0, None),
                 lambda: L.mi_pbs128_batch(None, None, None, None, 1, 0, None)):
        other_error()
        assert call() == _lib.MI_ERR_INVALID_ARG
        assert L.mi_last_error_message() == b"key is NULL"
