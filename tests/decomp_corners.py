"""The signed decomposition on big integers, and the corner corpus every decomposer test feeds (host only).

Reference paths are relative to tfhe/src/core_crypto/commons/math/decomposition.

* ``py_decompose`` / ``py_decompose_nonnative``: SignedDecomposer (decomposer.rs:156-185, iter.rs:103-151) and
  SignedDecomposerNonNative (decomposer.rs:521-548, iter.rs:623-745) statement by statement on Python integers,
  written from the reference's text and independent of the C oracle.
* ``corner_words`` / ``corner_words_nonnative``: the words at which a decomposer can go wrong and a uniform random word
  almost never lands: the rounding tie, a digit of exactly +-2^(B-1) at every level, the carry that runs through every
  level, the unbalanced top tie.
* ``corner_poly`` / ``corner_batch``: polynomials (rows of a batch) that put the corpus in front of every coefficient
  slot of a kernel.
"""
import json
import os

import numpy as np

import packing_helpers

M64 = 1 << 64
KAT_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decomposition_kat.json")


def kat():
    with open(KAT_PATH) as f:
        return json.load(f)


def closest_representable(x, base_log, level):
    """native_closest_representable (decomposer.rs:25-49) of a u64."""
    shift = 64 - base_log * level - 1
    return ((((x >> shift) + 1) & (M64 - 2)) << shift) % M64


def _signed(v):
    return v - M64 if v >> 63 else v


def _one_level(base_log, state):
    """decompose_one_level (iter.rs:131-151) on a u64 state: (signed term, next state)."""
    r = state & ((1 << base_log) - 1)
    state = (_signed(state) >> base_log) % M64                      # arithmetic shift of the signed state
    carry = ((((r - 1) % M64) | state) & r) >> (base_log - 1)
    state = (state + carry) % M64
    return r - (carry << base_log), state


def py_decompose(x, base_log, level):
    """SignedDecomposer::decompose of a u64: signed terms, least significant level first (the iterator's order)."""
    rep = base_log * level
    res = x >> (64 - rep - 1)                                       # init_decomposer_state, decomposer.rs:156-185
    rbit = res & 1
    res = ((res + 1) >> 1) & ((1 << rep) - 1)
    need = ((((res - 1) % M64) | (rbit << (rep - 1))) & res) >> (rep - 1)
    state = (res - (need << rep)) % M64
    terms = []
    for _ in range(level):
        t, state = _one_level(base_log, state)
        terms.append(t)
    return terms


def py_decompose_pre_rounded(x, base_log, level):
    """The packing keyswitch's digits: decompose(closest_representable(x)) (lwe_packing_keyswitch.rs:173-174)."""
    return py_decompose(closest_representable(x, base_log, level), base_log, level)


def py_decompose_nonnative(x, base_log, level, p):
    """SignedDecomposerNonNative::decompose of x < p: signed terms (add p to a negative one for the value mod p),
    least significant level first."""
    bits = (p - 1).bit_length()                                     # ceil_ilog2 of a modulus that is no power of two
    if x < (p + 1) // 2:                                            # div_ceil(2): the sign changes at p/2 + 1 (p odd)
        mag, negative = x, False
    else:
        mag, negative = p - x, True
    to_native = 64 - bits
    closest = closest_representable(mag << to_native, base_log, level) >> to_native
    state = closest >> (bits - base_log * level)                    # iter.rs:648-667
    terms = []
    for _ in range(level):
        t, state = _one_level(base_log, state)
        terms.append(-t if negative else t)
    return terms


def recompose(terms, base_log, level):
    """sum_j term_j 2^(64 - B (L - j)) mod 2^64 (least significant first)."""
    return sum(t << (64 - base_log * (level - j)) for j, t in enumerate(terms)) % M64


def _dedup(words):
    seen, out = set(), []
    for w in words:
        w %= M64
        if w not in seen:
            seen.add(w)
            out.append(w)
    return out


def corner_words(base_log, level):
    """The deterministic corner corpus of SignedDecomposer(base_log, level): a list of distinct u64 words."""
    rep = base_log * level
    step = 1 << (64 - rep)           # distance between representable values
    half = step >> 1                 # the rounding tie
    pos = [64 - rep + j * base_log for j in range(level)]           # bit position of field j (0 = least significant)
    top = 1 << (base_log - 1)        # the field value that ties between +2^(B-1) and -2^(B-1)
    words = [0, M64 - 1, 1 << 63, (1 << 63) - 1]
    for c in (0, 1 << 63):           # both ends of the rounding interval, and one below each
        words += [c + half, c + half - 1, c - half, c - half - 1, c + 1, c + half + 1, c - half + 1, c + step, c - step,
                  c + step + half, c + step + half - 1, c - step - half, c - step - half - 1]
    words += [1 << 62, (1 << 62) - 1, 3 << 62, (3 << 62) - 1]
    lows = [0, half, half - 1, -1, -half, -half - 1, step, -step]
    for j in range(level):
        w = top << pos[j]
        # the next field's top bit decides whether an inner +2^(B-1) is balanced to -2^(B-1)
        nexts = [0, top << pos[j + 1]] if j + 1 < level else [0]
        words += [w + nb + low for nb in nexts for low in lows]
    chain = sum(top << q for q in pos)                              # every field 2^(B-1): the carry runs through all levels
    words += [chain, chain + 1, chain - 1, chain + half, chain + half - 1, chain - half, chain - half - 1,
              -chain, -chain + 1, -chain - 1, -chain - half, -chain + half - 1]
    words += packing_helpers.tie_words(base_log, level)
    if (base_log, level) == (17, 3):
        words.append(int(kat()["sign_handling"]["word"], 16))
    return _dedup(words)


def corner_words_nonnative(base_log, level, p):
    """The corpus of SignedDecomposerNonNative(base_log, level, p): words < p around the sign threshold p/2 + 1, 0 and
    p - 1, and every native corner magnitude m <= p/2 on both sides (m and p - m)."""
    bits = (p - 1).bit_length()
    half_p = p // 2 + 1
    q = 1 << (bits - 1 - base_log * level)                          # the rounding tie of the magnitude
    base = [half_p, half_p - 1, half_p + 1, p // 2, 0, 1, 2, p - 1, p - 2, q, q - 1, q // 2, q // 2 + 1, 3 * q // 2,
            1 << (bits - 2), (1 << (bits - 1)) - 1 - p // 2]
    words = []
    for c in base:
        for d in (-1, 0, 1):
            words += [(c + d) % p, (p - c - d) % p]
    for w in corner_words(base_log, level):
        m = w >> (64 - bits)
        if m <= p // 2:
            words += [m, (p - m) % p]
    seen, out = set(), []
    for w in words:
        if w not in seen:
            seen.add(w)
            out.append(w)
    return out


def corner_poly(words, n, rng, roll=0, q=0):
    """n coefficients: coefficient j is words[(j + roll) % len(words)] on even repetitions of the corpus and a seeded
    random word (below q, or any u64 at q = 0) on odd ones, so that every word is present and the slots between
    repetitions differ."""
    m = len(words)
    assert n >= m, "the polynomial must hold the whole corpus"
    rnd = rng.integers(0, q, size=n, dtype=np.uint64) if q else rng.integers(0, M64, size=n, dtype=np.uint64)
    j = np.arange(n)
    corpus = np.array([words[(i + roll) % m] for i in range(n)], dtype=np.uint64)
    return np.where((j // m) % 2 == 0, corpus, rnd)


def corner_batch(words, shape, rng, q=0):
    """An array of shape (..., n) whose rows are corner_poly with the corpus rolled by the row index."""
    n = shape[-1]
    rows = int(np.prod(shape[:-1], dtype=np.int64))
    return np.stack([corner_poly(words, n, rng, roll=r, q=q) for r in range(rows)]).reshape(shape)


# ---- the (base_log, level) shapes of the GPU corner tests (tests/test_decomposition_corners_gpu.py); the CPU pins
# (tests/test_decomposition_kat.py) run every restatement on the same shapes ----
KS_SHAPES = [(5, 1), (6, 2), (4, 4), (3, 8),                       # ks_digits_l_kernel<1|2|4|8>, one byte per digit
             (7, 3), (12, 1), (17, 3),                             # ks_digits_kernel
             (7, 2), (8, 2), (15, 4), (16, 2), (23, 2), (24, 2), (31, 2),  # the steps of the bytes-per-digit count
             (32, 1), (33, 1), (40, 1), (63, 1)]                   # digits wider than 32 bits
KS32_SHAPES = [(2, 8), (16, 2), (32, 1)]
NTT_SHAPES = [(23, 1), (31, 1), (12, 2), (17, 3), (4, 4), (1, 9), (32, 1), (40, 1), (7, 3)]
FFT_SHAPES = [(23, 1), (31, 1), (12, 2), (8, 3), (10, 2)]
ALL_SHAPES = sorted(set(KS_SHAPES + KS32_SHAPES + NTT_SHAPES + FFT_SHAPES))


def probe_ggsw(level, k, n, li, row, const):
    """An NTT-domain GGSW (level, k + 1, k + 1, N) whose only non-zero row (level li, input component `row`) is the
    transform of the constant polynomial `const` (the same value at every point) in every output column: the
    external product then returns the digit polynomial li of component `row`, scaled by const, in every column."""
    g = np.zeros((level, k + 1, k + 1, n), np.uint64)
    g[li, row] = np.uint64(const)
    return g


def bnf_switch(v, p):
    """The p -> 2^64 switch of the BNF external product (ntt64.rs:184-197, the OR with p >> 1) of v < p."""
    return (((v << 64) | (p >> 1)) // p) % M64
