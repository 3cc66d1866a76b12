"""Host check of the 128-bit packing keyswitch's digit functions (the pre-rounded SignedDecomposer<u128> of
csrc/core_scalar.hpp and the signed-byte recodings of csrc/ks128_decomp.hpp): tests/cpp/ks128_decomp_check.cpp compares
them with a restatement in unsigned __int128 (and the plain decomposition of the 128-bit bootstraps with it too) and
with the digits pbs128_helpers.py_decompose gives for closest_representable(word), on corner_words, tie_words128 and
random words at the six (base_log, level) pairs of the packing keyswitch tests; every digit recomposes from its nd
signed bytes and every word from its 16.  No GPU: hipcc builds the headers' host side."""
import os
import subprocess

import pytest

import packing128_helpers as Q
import pbs128_helpers as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
SHAPES = [(61, 1), (24, 3), (4, 3), (7, 2), (8, 1), (63, 2)]

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ks128_decomp") / "ks128_decomp_check")
    subprocess.run([HIPCC, "-O2", "-x", "hip", os.path.join(ROOT, "tests", "cpp", "ks128_decomp_check.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=300)
    return exe


def _cases():
    g = R.rng(0x128d)
    lines, count = [], 0
    for base_log, level in SHAPES:
        words = R.corner_words(base_log, level) + Q.tie_words128(base_log, level) + R.uniform_u128(g, 200)
        for w in words:
            terms = Q.digits128(w, base_log, level)
            lines.append(f"{base_log} {level} {w >> 64:x} {w & R.MASK64:x} " + " ".join(map(str, terms)))
        count += len(words)
    return "\n".join(lines) + "\n", count


def test_host_decomposition_and_recodings(checker):
    text, count = _cases()
    r = subprocess.run([checker], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith(f"{count} listed cases, ") and last.endswith(" 0 mismatches"), last


def test_checker_catches_a_decomposer_without_pre_rounding(checker):
    """The digits of decompose(word) listed in place of decompose(closest_representable(word)) on the tie interval's
    ends: the checker must report them."""
    lines = []
    for base_log, level in SHAPES:
        step = 1 << (127 - base_log * level)
        for w in ((1 << 127) - step, (1 << 127) - 1):
            terms = Q.digits128(w, base_log, level, rounded=False)
            lines.append(f"{base_log} {level} {w >> 64:x} {w & R.MASK64:x} " + " ".join(map(str, terms)))
    r = subprocess.run([checker], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 1
    assert int(r.stdout.strip().splitlines()[-1].split()[-2]) >= len(lines)  # at least one digit of every case
