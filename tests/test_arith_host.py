"""Host check of csrc/mi_arith.hpp (Goldilocks, Montgomery, Shoup32) against unsigned __int128
(tests/cpp/arith_check.cpp): the 73 x 73 limb-corner grid of tests/arith_corners.py, mul_pow2 at all 192 exponents, the
lazy forms on non-canonical words, the generic and the 32-bit test primes, random operands, and every branch arm of
every primitive taken at least once (or listed in the program with its unreachability argument).  No GPU: hipcc builds
the header's host side."""
import os
import re
import subprocess

import pytest

import arith_corners as AC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_primitives_match_int128_and_take_every_arm(tmp_path, oracle):
    exe = str(tmp_path / "arith_check")
    subprocess.run([HIPCC, "-O2", "-x", "hip", os.path.join(ROOT, "tests", "cpp", "arith_check.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=300)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-4000:]
    assert " 0 mismatches, 0 arms untaken" in out.stdout
    # the program's primes are the GPU tests' (tests/test_ntt_gpu.py _primes, tests/test_native_gpu.py _primes32)
    f = oracle.largest_prime_in_arithmetic_progression64
    want64 = {"p64": f(1 << 16, 1, 1 << 63, 2**64 - 1), "p63": f(1 << 16, 1, 1 << 62, 1 << 63),
              "p62": f(1 << 16, 1, 1 << 61, 1 << 62), "p50": f(1 << 16, 1, 1 << 49, 1 << 50), "p30": 1062862849}
    got64 = {m.group(1): int(m.group(2)) for m in re.finditer(r"^montgomery (\w+) (\d+)$", out.stdout, re.M)}
    assert got64 == want64
    want32 = {1062862849, 1073479681, f(1 << 16, 1, 1 << 30, 1 << 31), f(1 << 16, 1, 1 << 31, 1 << 32)}
    assert {int(v) for v in re.findall(r"^shoup32 (\d+)$", out.stdout, re.M)} == want32


def test_corpus_reaches_the_rare_goldilocks_arms():
    """values(p) on Python integers: 73 residues for the Solinas prime, and its operand grid takes the reduction's
    borrow fix and both "no carry but >= p" arms (the counts the corpus was designed to)."""
    p, eps, m64 = AC.SOLINAS_P, 0xFFFFFFFF, (1 << 64) - 1
    v = AC.values(p)
    assert len(v) == 73 and len(set(v)) == 73 and all(0 <= x < p for x in v)
    borrow = ge_red = ge_add = 0
    for a in v:
        for b in v:
            ge_add += p <= a + b <= m64
            t = a * b
            lo, hi = t & m64, t >> 64
            hh, hl = hi >> 32, hi & eps
            t0 = (lo - hh) & m64
            if lo < hh:
                borrow += 1
                t0 = (t0 - eps) & m64
            r = t0 + ((hl << 32) - hl)
            ge_red += p <= r <= m64
    assert (borrow, ge_red, ge_add) == (107, 283, 492)


def test_montgomery_wrap_pairs_reach_the_arm(oracle):
    """montgomery_wrap_pairs: a b + m p = 2^128 exactly, so REDC's thi + mhi is 2^64 - 1 with a carry in."""
    p = oracle.largest_prime_in_arithmetic_progression64(1 << 16, 1, 1 << 63, 2**64 - 1)
    pairs = AC.montgomery_wrap_pairs(p)
    assert len(pairs) == 8
    pinv = (-pow(p, -1, 1 << 64)) % (1 << 64)
    for a, b in pairs:
        assert 0 < a < p and 0 < b < p
        t = a * b
        m = (t * pinv) % (1 << 64)
        assert (t >> 64) + ((m * p) >> 64) == (1 << 64) - 1 and t % (1 << 64) != 0
    assert AC.montgomery_wrap_pairs((1 << 62) - 57) == []   # below 2^63 the sum cannot reach 2^64
