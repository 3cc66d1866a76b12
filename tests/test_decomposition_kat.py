"""CPU pins of every restatement of the signed decomposition the tests rely on — no GPU.

The restatements: ``decomp_corners.py_decompose`` (big integers), the C oracle's ``decomp_init_native`` +
``decompose_one_level`` (pbs_oracle.c), ``fft_oracle.decompose`` (numpy), and the packing keyswitch's
``packing_helpers._closest_representable`` + the oracle's state machine.  Pinned here:

* the reference's two known-answer tests (tests/golden/decomposition_kat.json: commons/math/decomposition/
  tests.rs:204-226 and :228-247), on each restatement;
* on the corner corpus (decomp_corners.corner_words) plus 2,000 seeded random words, for every (base_log, level) the
  GPU corner tests use: all restatements agree, the terms recompose to closest_representable, |term| <= 2^(B-1);
* the corpus itself: every level position sees both +2^(B-1) and -2^(B-1), and the packing keyswitch's pre-rounded
  digits differ from the plain ones on at least one word;
* the non-native transcription against the oracle's Solinas external product through a one-row probe, and the BNF
  probe the GPU tests use;
* the kernels' own digit functions (csrc/core_scalar.hpp: decomp_init / decomp_next, NttDigits; csrc/ks_decomp.hpp:
  signed_byte), compiled for the host: the keyswitches' on the corpus and on every base_log 1..63
  (tests/cpp/ks_decomp_check.cpp), the NTT paths' digit stream on the corpus of the probes above
  (tests/cpp/ntt_digits_check.cpp).
"""
import os
import subprocess

import numpy as np
import pytest

import decomp_corners as D
import packing_helpers
import tfhe_helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
M64 = 1 << 64
P = 0xFFFFFFFF00000001


def _signed(v):
    v = int(v)
    return v - M64 if v >> 63 else v


def _oracle_terms(oracle, x, base_log, level):
    state = oracle.decomp_init_native(x, base_log, level)
    terms = []
    for _ in range(level):
        t, state = oracle.decompose_one_level(base_log, state)
        terms.append(_signed(t))
    return terms


def _fft_terms(x, base_log, level):
    import fft_oracle as F
    return [_signed(t[0]) for t in F.decompose(np.array([x], np.uint64), base_log, level)]


def _packing_terms(oracle, x, base_log, level):
    """The digits packing_keyswitch_transcription computes (lwe_packing_keyswitch.rs:173-179)."""
    return _oracle_terms(oracle, packing_helpers._closest_representable(x, base_log, level), base_log, level)


def _restatements(oracle):
    return {
        "py_decompose": D.py_decompose,
        "oracle": lambda x, b, l: _oracle_terms(oracle, x, b, l),
        "fft_oracle": _fft_terms,
        "packing": lambda x, b, l: _packing_terms(oracle, x, b, l),
    }


NAMES = ["py_decompose", "oracle", "fft_oracle", "packing"]


@pytest.mark.parametrize("name", NAMES)
def test_sign_handling_vector(oracle, name):
    """tests.rs:228-247: the terms of the word whose state starts negative, in the iterator's order, and their
    recomposition.  (The word is no rounding tie, so the packing keyswitch's pre-rounded digits are the same.)"""
    v = D.kat()["sign_handling"]
    word, b, l = int(v["word"], 16), v["base_log"], v["level"]
    terms = _restatements(oracle)[name](word, b, l)
    assert terms == v["terms"]
    assert D.recompose(terms, b, l) == D.closest_representable(word, b, l)


@pytest.mark.parametrize("name", NAMES)
def test_single_level_balanced_vector(oracle, name):
    """tests.rs:204-226: over all 2^13 patterns of the top B + 1 bits the level-1 terms sum to 0.  The packing
    keyswitch's digits are those of the pre-rounded word: the one pattern 0111..1 rounds to 2^63, whose rounding bit
    is then 0, so its digit is +2^(B-1) where the plain one is -2^(B-1), and the sum is 2^B."""
    v = D.kat()["single_level_balanced"]
    b, l, bits = v["base_log"], v["level"], v["pattern_bits"]
    assert l == 1 and bits == b + 1
    if name == "fft_oracle":
        import fft_oracle as F
        words = np.arange(1 << bits, dtype=np.uint64) << np.uint64(64 - bits)
        total = sum(int(t) for t in F.decompose(words, b, l)[0].view(np.int64))
    else:
        fn = _restatements(oracle)[name]
        total = sum(fn(val << (64 - bits), b, l)[0] for val in range(1 << bits))
    assert total == (v["expected_sum"] + (1 << b) if name == "packing" else v["expected_sum"])


def _words(base_log, level):
    g = H.rng(base_log * 64 + level)
    return D.corner_words(base_log, level) + [int(w) for w in H.uniform_u64(g, 2000)]


@pytest.mark.parametrize("base_log,level", D.ALL_SHAPES)
def test_restatements_agree_on_corners(oracle, base_log, level):
    import fft_oracle as F
    words = _words(base_log, level)
    arr = np.array(words, dtype=np.uint64)
    fft = [t.view(np.int64) for t in F.decompose(arr, base_log, level)]
    fft_pre = [t.view(np.int64) for t in F.decompose(packing_helpers.pre_round(arr, base_log, level), base_log, level)]
    bound = 1 << (base_log - 1)
    for i, x in enumerate(words):
        terms = D.py_decompose(x, base_log, level)
        assert _oracle_terms(oracle, x, base_log, level) == terms, hex(x)
        assert [int(t[i]) for t in fft] == terms, hex(x)
        assert D.recompose(terms, base_log, level) == D.closest_representable(x, base_log, level), hex(x)
        assert all(abs(t) <= bound for t in terms), hex(x)
        pre = D.py_decompose_pre_rounded(x, base_log, level)
        assert _packing_terms(oracle, x, base_log, level) == pre, hex(x)
        assert [int(t[i]) for t in fft_pre] == pre, hex(x)
        assert D.recompose(pre, base_log, level) == D.closest_representable(x, base_log, level), hex(x)
        assert all(abs(t) <= bound for t in pre), hex(x)


@pytest.mark.parametrize("base_log,level", D.ALL_SHAPES)
def test_corpus_reaches_every_extreme_digit(base_log, level):
    """A condition on the inputs: the corpus puts +2^(B-1) and -2^(B-1) in front of every level position, and holds
    a word on which the packing keyswitch's pre-rounded digits differ from the plain ones."""
    words = D.corner_words(base_log, level)
    assert 20 <= len(words) <= 200
    assert len(set(words)) == len(words) and all(0 <= w < M64 for w in words)
    for w in [0, M64 - 1, 1 << 63, (1 << 63) - 1] + packing_helpers.tie_words(base_log, level):
        assert w in words
    top = 1 << (base_log - 1)
    digits = [D.py_decompose(w, base_log, level) for w in words]
    for j in range(level):
        seen = {d[j] for d in digits}
        assert top in seen, f"level position {j} never sees +2^(B-1)"
        assert -top in seen, f"level position {j} never sees -2^(B-1)"
    assert any(D.py_decompose_pre_rounded(w, base_log, level) != d for w, d in zip(words, digits))


def test_corner_poly_holds_the_whole_corpus():
    words = D.corner_words(7, 3)
    g = H.rng(5)
    for roll in (0, 1, len(words) - 1):
        poly = D.corner_poly(words, 512, g, roll=roll)
        assert poly.dtype == np.uint64 and poly.shape == (512,)
        assert set(words) <= {int(v) for v in poly}
        assert int(poly[0]) == words[roll]
    batch = D.corner_batch(words, (3, 2, 512), H.rng(5))
    assert int(batch[2, 1, 0]) == words[5]
    sol = D.corner_poly(D.corner_words_nonnative(7, 3, P), 1024, g, q=P)
    assert int(sol.max()) < P


# ---- the non-native transcription and the probes of the GPU tests, against the oracle's external products ----
PROBE_N = 1024


@pytest.mark.parametrize("base_log,level", D.NTT_SHAPES)
def test_nonnative_transcription_matches_oracle_probe(oracle, base_log, level):
    """One-row probe: the only non-zero GGSW row (level li, input component r) is the transform of the constant 1 / N
    (the oracle's inverse transform is not normalised), so ora_ext_product_solinas returns digit polynomial li of
    component r mod p in every output column.  It equals the big-integer SignedDecomposerNonNative transcription."""
    words = D.corner_words_nonnative(base_log, level, P)
    ctx = oracle.NttContext(PROBE_N)
    glwe = D.corner_batch(words, (2, PROBE_N), H.rng(base_log + level), q=P)
    want = [[D.py_decompose_nonnative(int(x), base_log, level, P) for x in comp] for comp in glwe]
    bound = 1 << (base_log - 1)
    assert all(abs(t) <= bound for comp in want for terms in comp for t in terms)
    for li in range(level):
        for r in range(2):
            ggsw = D.probe_ggsw(level, 1, PROBE_N, li, r, ctx.plan.n_inv)
            got = ctx.ext_product(np.zeros(2 * PROBE_N, np.uint64), ggsw.reshape(-1), glwe.reshape(-1), 1, base_log,
                                  level, bnf=False).reshape(2, PROBE_N)
            digits = np.array([terms[li] % P for terms in want[r]], dtype=np.uint64)
            assert np.array_equal(got[0], digits) and np.array_equal(got[1], digits)


@pytest.mark.parametrize("base_log,level", D.NTT_SHAPES)
def test_bnf_probe_returns_the_digits(oracle, base_log, level):
    """The BNF probe (constant 1: this path normalises): ora_ext_product_bnf returns the p -> 2^64 switch of digit
    polynomial li mod p, which is the digit itself mod 2^64 while |digit| < 2^31."""
    words = D.corner_words(base_log, level)
    ctx = oracle.NttContext(PROBE_N)
    glwe = D.corner_batch(words, (2, PROBE_N), H.rng(base_log + level))
    want = [[D.py_decompose(int(x), base_log, level) for x in comp] for comp in glwe]
    for li in range(level):
        for r in range(2):
            ggsw = D.probe_ggsw(level, 1, PROBE_N, li, r, 1)
            got = ctx.ext_product(np.zeros(2 * PROBE_N, np.uint64), ggsw.reshape(-1), glwe.reshape(-1), 1, base_log,
                                  level, bnf=True).reshape(2, PROBE_N)
            switched = np.array([D.bnf_switch(terms[li] % P, P) for terms in want[r]], dtype=np.uint64)
            assert np.array_equal(got[0], switched) and np.array_equal(got[1], switched)
            if base_log <= 31:
                assert np.array_equal(switched, np.array([terms[li] % M64 for terms in want[r]], dtype=np.uint64))


# ---- the kernels' own digit functions, compiled for the host ----
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_keyswitch_digit_functions_on_host(tmp_path):
    """csrc/core_scalar.hpp's decomp_init / decomp_next and csrc/ks_decomp.hpp's signed_byte against
    tests/cpp/ks_decomp_check.cpp's restatement and against py_decompose's digits, plain
    and pre-rounded, on the corpus of every keyswitch shape (digits wider than 32 bits included); the check itself
    adds every base_log 1..63 at one level.  Each digit must also recompose from the signed bytes the GEMM gets."""
    exe = str(tmp_path / "ks_decomp_check")
    subprocess.run([HIPCC, "-O2", "-x", "hip", os.path.join(ROOT, "tests", "cpp", "ks_decomp_check.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=300)
    lines = []
    for base_log, level in sorted(set(D.KS_SHAPES + D.KS32_SHAPES)):
        for w in D.corner_words(base_log, level):
            for pre, fn in ((0, D.py_decompose), (1, D.py_decompose_pre_rounded)):
                lines.append(" ".join([str(base_log), str(level), str(pre), f"{w:x}"] + [str(t) for t in fn(w, base_log, level)]))
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout
    assert f"{len(lines)} listed cases" in out.stdout and " 0 mismatches" in out.stdout


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_ntt_digit_streams_on_host(oracle, tmp_path):
    """csrc/core_scalar.hpp's NttDigits<true> / NttDigits<false> (the digit stream of pbs_kernels.hip and pbs_large.hip)
    on the corpus of the two probe tests above at D.NTT_SHAPES.  Required: the digits the oracle's one-row probe
    returns for component 0 (Solinas: the digit polynomial itself mod p; BNF: its p -> 2^64 switch, an injective map of
    [0, p), so the digit mod p whose switch the probe returned)."""
    exe = str(tmp_path / "ntt_digits_check")
    subprocess.run([HIPCC, "-O2", "-x", "hip", os.path.join(ROOT, "tests", "cpp", "ntt_digits_check.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=300)
    ctx = oracle.NttContext(PROBE_N)
    lines = []
    for base_log, level in D.NTT_SHAPES:
        for bnf in (1, 0):
            words = D.corner_words(base_log, level) if bnf else D.corner_words_nonnative(base_log, level, P)
            glwe = D.corner_batch(words, (2, PROBE_N), H.rng(base_log + level), q=0 if bnf else P)
            digits = []
            for li in range(level):
                ggsw = D.probe_ggsw(level, 1, PROBE_N, li, 0, 1 if bnf else ctx.plan.n_inv)
                got = ctx.ext_product(np.zeros(2 * PROBE_N, np.uint64), ggsw.reshape(-1), glwe.reshape(-1), 1, base_log,
                                      level, bnf=bool(bnf)).reshape(2, PROBE_N)[0]
                if bnf:  # undo the switch: the candidates are the digits mod p of the big-integer decomposition
                    cand = [D.py_decompose(int(x), base_log, level)[li] % P for x in glwe[0]]
                    assert [D.bnf_switch(c, P) for c in cand] == [int(v) for v in got]
                    got = cand
                digits.append([int(v) for v in got])
            for j in range(len(words)):  # coefficient j of component 0 is words[j] (corner_poly, roll 0)
                assert int(glwe[0, j]) == words[j]
                lines.append(" ".join([str(bnf), str(base_log), str(level), f"{words[j]:x}"] +
                                      [str(digits[li][j]) for li in range(level)]))
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout
    assert f"{len(lines)} listed cases" in out.stdout and " 0 mismatches" in out.stdout
