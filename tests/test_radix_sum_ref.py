"""The radix sum of ciphertexts and the radix multiplication on the host: the Python model (tests/radix_sum_ref.py)
against the integers, its mutants, the library's schedule (mi_radix_sum_schedule) against the model, the ABI of the new
calls, and the noise condition of the decrypting GPU tests.  No GPU."""
import ctypes
import itertools

import numpy as np
import pytest

import radix_sum_ref as S
import shortint_ref as R

INVALID, UNSUPPORTED = 1, 6
MODULI = [(4, 4), (8, 8), (8, 4)]


def L():
    from tfhe_ntt_amd import _lib
    return _lib.lib()


def rng(seed):
    return np.random.default_rng(seed)


def mul_inputs(m, blocks, g):
    top = m**blocks
    pairs = [(top - 1, top - 1), (0, top - 1), (1, top - 1), (top - 1, 1)]
    pairs += [tuple(int(v) for v in g.integers(0, top, 2)) for _ in range(6)]
    return pairs


def sum_inputs(m, blocks, g):
    """(terms, first_block): all-(m - 1) dense terms at several counts, ragged ones, random ones."""
    s_max = 2 * m + 3
    cases = []
    for n_terms in (1, 2, 3, s_max, 13, 3 * s_max + 1):
        cases.append(([[m - 1] * blocks for _ in range(n_terms)], [0] * n_terms))
        cases.append(([[int(v) for v in g.integers(0, m, blocks)] for _ in range(n_terms)], [0] * n_terms))
    first = [int(v) for v in g.integers(0, blocks + 1, 11)]
    cases.append(([[0] * f + [m - 1] * (blocks - f) for f in first], first))
    return cases


# ---- values ----

def test_exhaustive_at_2_2():
    """Every pair of B <= 3 block integers at (2, 2), and every triple of terms at B <= 2: the integers, with no block
    of any round passing m c - 1 (a lookup would refuse it)."""
    m = c = 2
    for blocks in (1, 2, 3):
        top = m**blocks
        for a, b in itertools.product(range(top), repeat=2):
            got = S.mul(R.digits(a, m, blocks), R.digits(b, m, blocks), m, c)
            assert R.value(got, m) == (a * b) % top and max(got) < m, (blocks, a, b, got)
    for blocks in (1, 2):
        top = m**blocks
        for n_terms in (3, 4, 5):
            for vals in itertools.product(range(top), repeat=n_terms):
                got = S.sum_terms([R.digits(v, m, blocks) for v in vals], None, blocks, m, c)
                assert R.value(got, m) == sum(vals) % top, (blocks, vals, got)


@pytest.mark.parametrize("m,c", MODULI)
def test_sum_and_mul_are_the_integers(m, c):
    g = rng(0x5a00 + m * c)
    for blocks in range(1, 9):
        top = m**blocks
        for terms, first in sum_inputs(m, blocks, g):
            got = S.sum_terms(terms, first, blocks, m, c)
            assert R.value(got, m) == sum(R.value(t, m) for t in terms) % top and max(got) < m, (blocks, first)
        for a, b in mul_inputs(m, blocks, g):
            got = S.mul(R.digits(a, m, blocks), R.digits(b, m, blocks), m, c)
            assert R.value(got, m) == (a * b) % top and max(got) < m, (blocks, a, b)


MUTANTS = {"chunk of s + 1": S.Rule(chunk_extra=1), "carry out of the last column": S.Rule(last_column_carry=True),
           "rest from the front": S.Rule(rest_from_front=True), "exactly s left alone": S.Rule(skip_exact=True)}


def outcome(f):
    try:
        return f()
    except OverflowError:
        return "overflow"


@pytest.mark.parametrize("name", list(MUTANTS))
def test_mutants_are_told_apart(name):
    """Each mutant differs from the true rule on at least one of the inputs above: in the integer, in a block passing
    m c - 1, or (the value being order-independent) in the rounds' column lengths and chunk counts, or in the rows a
    chunk holds, which is what decides the bits of the ciphertexts."""
    rule = MUTANTS[name]
    told = False
    for m, c in MODULI:
        g = rng(0x5a00 + m * c)
        for blocks in range(1, 9):
            for terms, first in sum_inputs(m, blocks, g):
                labels = [[(t, b) for b in range(blocks)] for t in range(len(terms))]
                want = (outcome(lambda: S.partial_sum(terms, first, blocks, m, c)),
                        S.run_rounds(S.initial_columns(labels, first, blocks), m, c, lambda r, b, w, k: (("m", tuple(r)), ("c", tuple(r)) if w else None)))
                got = (outcome(lambda: S.partial_sum(terms, first, blocks, m, c, rule)),
                       outcome(lambda: S.run_rounds(S.initial_columns(labels, first, blocks), m, c,
                                                    lambda r, b, w, k: (("m", tuple(r)), ("c", tuple(r)) if w else None), rule)))
                told = told or got != want
    assert told, name


def test_a_chunk_of_s_plus_one_overflows():
    """The chunk size is tight: s + 1 rows of m - 1 pass m c - 1 and a lookup refuses them."""
    for m, c in MODULI:
        ones = [[m - 1] * 3 for _ in range(3 * m + 4)]
        assert outcome(lambda: S.partial_sum(ones, None, 3, m, c, MUTANTS["chunk of s + 1"])) == "overflow"
        assert outcome(lambda: S.partial_sum(ones, None, 3, m, c)) != "overflow"


# ---- the library's schedule ----

def lib_schedule(n_blocks, first_block, m, c, n_terms=None):
    n_terms = len(first_block) if n_terms is None else n_terms
    fb = (ctypes.c_uint32 * max(len(first_block), 1))(*first_block)
    rounds = ctypes.c_size_t()
    st = L().mi_radix_sum_schedule(n_blocks, n_terms, fb if first_block else None, m, c, ctypes.byref(rounds), None, None, 0)
    if st != 0:
        return st, L().mi_last_error_message().decode()
    r = rounds.value
    lens = (ctypes.c_uint32 * ((r + 1) * n_blocks))()
    chunks = (ctypes.c_uint32 * max(r * n_blocks, 1))()
    assert L().mi_radix_sum_schedule(n_blocks, n_terms, fb if first_block else None, m, c, ctypes.byref(rounds), lens,
                                     chunks, r) == 0
    assert rounds.value == r
    return ([list(lens[i * n_blocks:(i + 1) * n_blocks]) for i in range(r + 1)],
            [list(chunks[i * n_blocks:(i + 1) * n_blocks]) for i in range(r)])


def schedule_grid():
    grid = []
    for m, c in [(4, 4), (2, 2), (8, 8), (8, 4), (4, 2)]:
        for blocks in list(range(1, 9)) + [32]:
            grid.append((blocks, S.mul_first_block(blocks, m), m, c))
        grid.append((3, [0] * 13, m, c))
        grid.append((3, [0] * 5, m, c))
        grid.append((3, [0, 0, 1, 2, 2, 0, 1], m, c))
        grid.append((4, [4, 4, 0], m, c))
        grid.append((2, [], m, c))
        grid.append((5, [0] * 300 + [3] * 40, m, c))
    return grid


def test_schedule_equals_the_model(engine):
    seen_rounds = set()
    for blocks, first, m, c in schedule_grid():
        want = S.schedule(blocks, first, m, c)
        got = lib_schedule(blocks, first, m, c)
        assert got == (want["lens"], want["chunks"]), (blocks, first, m, c)
        seen_rounds.add((blocks, len(first), m, len(want["chunks"])))
    # 13 dense terms of 3 blocks at (4, 4) take two rounds, 5 take none; the mul pattern at B = 4 one, with columns 1 3 5 7
    assert (3, 13, 4, 2) in seen_rounds and (3, 5, 4, 0) in seen_rounds and (4, 7, 4, 1) in seen_rounds
    assert S.schedule(4, S.mul_first_block(4, 4), 4, 4)["lens"][0] == [1, 3, 5, 7]
    assert S.schedule(4, S.mul_first_block(4, 4), 4, 4)["rounds"][0][-1][2] is False  # the last column: no carry
    assert len(S.schedule(5, S.mul_first_block(5, 4), 4, 4)["chunks"]) == 2
    # NULL first_block is all zeros
    fb = None
    rounds = ctypes.c_size_t()
    assert L().mi_radix_sum_schedule(3, 13, fb, 4, 4, ctypes.byref(rounds), None, None, 0) == 0 and rounds.value == 2


def test_schedule_rejections(engine):
    for m, c in [(4, 8), (2, 4), (1, 1), (4, 1), (4, 0)]:
        st, msg = lib_schedule(3, [0, 0, 0], m, c)
        assert st == UNSUPPORTED and "carry_modulus" in msg, (m, c, st, msg)
    st, msg = lib_schedule(0, [0], 4, 4)
    assert st == INVALID and "n_blocks is 0" in msg
    st, msg = lib_schedule(3, [0, 4], 4, 4)
    assert st == INVALID and "first_block is past the end" in msg
    assert lib_schedule(3, [0, 3], 4, 4)[0] == [[1, 1, 1]]  # first_block = n_blocks: a term that is zero everywhere
    st, msg = lib_schedule(1 << 12, [], 4, 4, n_terms=1 << 12)
    assert st == INVALID and "batch too large" in msg
    rounds = ctypes.c_size_t()
    lens = (ctypes.c_uint32 * 16)()
    assert L().mi_radix_sum_schedule(3, 13, None, 4, 4, ctypes.byref(rounds), lens, None, 1) == INVALID
    assert b"rounds_capacity" in L().mi_last_error_message()


# ---- ABI ----

NEW = ["mi_radix_sum_schedule", "mi_radix_sum_batch", "mi_radix_sum_pass_integers", "mi_radix_mul_batch",
       "mi_radix_mul_pass_integers"]


def test_header_declares_and_library_exports(engine):
    from tfhe_ntt_amd import _lib
    syms = set(_lib.declared_symbols())
    assert set(NEW) <= syms and all(s in _lib._SIGS for s in NEW)
    for s in NEW:
        assert getattr(L(), s) is not None


def test_null_key_is_answered_before_anything_else(engine):
    words = (ctypes.c_uint64 * 8)()
    p = ctypes.addressof(words)
    n = ctypes.c_size_t()
    for call in (lambda: L().mi_radix_sum_batch(None, p, p, 3, None, 2, 1, None),
                 lambda: L().mi_radix_mul_batch(None, p, p, p, 2, 1, None),
                 lambda: L().mi_radix_sum_pass_integers(None, 3, None, 2, 1, ctypes.byref(n)),
                 lambda: L().mi_radix_mul_pass_integers(None, 2, 1, ctypes.byref(n))):
        assert L().mi_lwe_ksk_create(None, 8, 10, 4, 4, 0, None, None) == INVALID  # another message in between
        assert call() == INVALID and L().mi_last_error_message() == b"key is NULL"


# ---- the noise condition of the decrypting GPU tests (tests/test_radix_mul_gpu.py) ----

@pytest.mark.parametrize("name,m,c,multi_bit", [("real", 4, 4, False), ("real", 4, 4, True), ("real", 2, 2, False),
                                                ("real4096", 8, 8, False)],
                         ids=["real-4-4", "real-4-4-multi-bit", "real-2-2", "real4096-8-8"])
def test_linear_steps_stay_inside_the_box(engine, oracle, name, m, c, multi_bit):
    """The linear steps this feature puts in front of a bootstrap are the sum of s = (m c - 1) / (m - 1) bootstrap
    outputs (chunk sums and block sums) and the pack m x + y of two operand blocks, which are fresh encryptions (noise
    2^10, far below a bootstrap's output) or bootstrap outputs.  With e_out the worst absolute output error of a
    bootstrap and e_in the worst absolute error the keyswitch and the modulus switch add in front of the next one,
    both measured on the host under the very key set the GPU test decrypts with (shortint_gpu_helpers.measure_noise,
    as test_shortint_ref.py::test_real_key_sets_keep_two_bits_of_margin measures them), the phase error in front of a
    bootstrap is at most e_in + f e_out in absolute value, f = max(s, m + 1) (absolute errors add with the absolute
    coefficients: s ones, or m and 1; in variance the factors are s and m^2 + 1).  That has to stay below the decoding
    half box 2^63 / (m c) / 2; the test asks for one more bit."""
    import shortint_gpu_helpers as G

    ks = G.key_set(engine, oracle, name, device=False)
    e_in, e_out = G.measure_noise(oracle, ks, m, c, 0x5f00 + m * c, multi_bit)
    f = max(S.max_sum_size(m, c), m + 1)
    half_box = (1 << 63) // (m * c) // 2
    worst = e_in + f * e_out
    print(f"noise {name} ({m}, {c}){' multi-bit' if multi_bit else ''}: input 2^{np.log2(e_in):.2f}, output "
          f"2^{np.log2(e_out):.2f}, f = {f}, worst 2^{np.log2(worst):.2f}, half box 2^{np.log2(half_box):.2f}")
    assert 2 * worst <= half_box, (e_in, e_out, f, half_box)
