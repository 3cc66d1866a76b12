"""Host check of csrc/ntt64_plan_tables.hpp, the tables and constants plan_create uploads: tests/cpp/plan_tables_check.cpp
dumps them for one (N, p), and every word is compared here against restatements that do not read the C++ (the oracle's
plan, Python integers, the twist table of tests/tw_tables_ref.py).  No GPU: hipcc builds the header's host side."""
import glob
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN
from tw_tables_ref import P, tables as twist_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
R = 1 << 64

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")


def _golden_primes_n16():
    ps = []
    for f in sorted(glob.glob(os.path.join(GOLDEN, "prime64_*_n16.npz"))):
        with np.load(f, allow_pickle=False) as z:
            ps.append(int(z["p"][0]))
    return ps


PRIMES16 = _golden_primes_n16()
P_SMALL = next(p for p in PRIMES16 if p < 1 << 32)
P_BIG = max(p for p in PRIMES16 if p != P)


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """dump(n, p) -> {section name: list of Python ints}; the program is built once and each (n, p) runs once."""
    d = tmp_path_factory.mktemp("plan_tables")
    exe = str(d / "plan_tables_check")
    subprocess.run([HIPCC, "-O2", "-x", "hip", os.path.join(ROOT, "tests", "cpp", "plan_tables_check.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=300)
    cache = {}

    def run(n, p):
        if (n, p) not in cache:
            path = str(d / f"{n}_{p}.bin")
            subprocess.run([exe, str(n), str(p), path], check=True, timeout=60)
            raw, pos, out = open(path, "rb").read(), 0, {}
            while pos < len(raw):
                name = raw[pos:pos + 8].rstrip(b"\0").decode()
                (count,) = struct.unpack_from("<Q", raw, pos + 8)
                out[name] = list(struct.unpack_from(f"<{count}Q", raw, pos + 16))
                pos += 16 + 8 * count
            cache[(n, p)] = out
        return cache[(n, p)]

    return run


def test_golden_primes_cover_the_cases():
    assert P in PRIMES16 and len(PRIMES16) >= 8 and P_SMALL < 1 << 32 < P_BIG


@pytest.mark.parametrize("n,p", [(16, p) for p in PRIMES16] + [(2048, P)])
def test_base_tables_equal_the_oracle_plan(dump, oracle, n, p):
    t, plan = dump(n, p), oracle.Plan.try_new(n, p)
    assert t["twid"] == [int(v) for v in plan.twid]
    assert t["inv_twid"] == [int(v) for v in plan.inv_twid]
    assert t["n_inv"] == [int(plan.n_inv)]
    assert ("shoup32" in t) == (p < 1 << 32)
    assert ("twist" in t) == (n == 2048) and "blk" not in t


def test_shoup32_words(dump):
    p, t = P_SMALL, dump(16, P_SMALL)
    assert t["shoup32"] == [w | ((w << 32) // p) << 32 for w in t["twid"] + t["inv_twid"]]


def test_device_form_of_a_generic_prime(dump):
    p, t = P_BIG, dump(16, P_BIG)
    mp, pinv, r1, r2 = t["mont"]
    assert mp == p and pinv * p % R == R - 1 and r1 == R % p and r2 == (1 << 128) % p
    assert t["dev_tw"] == [w * R % p for w in t["twid"]]
    assert t["dev_itw"] == [w * R % p for w in t["inv_twid"]]
    assert t["montform"] == t["dev_tw"]
    n_inv = t["n_inv"][0]
    assert n_inv * 16 % p == 1
    # normalize multiplies by N^-1 R (one REDC leaves x N^-1); mul_assign_normalize by N^-1 R^2 (two REDCs);
    # mul_accumulate enters Montgomery form with R^2
    assert t["consts"] == [n_inv * R % p, n_inv * R * R % p, r2]


def test_device_form_of_the_solinas_prime(dump):
    t = dump(16, P)
    assert t["dev_tw"] == t["twid"] and t["dev_itw"] == t["inv_twid"] and t["mont"] == [0, 0, 0, 0]
    assert t["consts"] == [t["n_inv"][0], t["n_inv"][0], 0]


def test_twist_table_regions(dump, oracle):
    n, t = 2048, dump(2048, P)
    _, f, i = twist_ref(oracle)
    tab, n_inv, reg = t["twist"], t["n_inv"][0], n + 32
    assert t["tower_ok"] == [1]
    assert len(tab) == 4 * reg + 32 and len(f) == len(i) == reg
    r1, r2, r3 = tab[:reg], tab[reg:2 * reg], tab[2 * reg:3 * reg]
    r4, r5 = tab[3 * reg:3 * reg + 32], tab[3 * reg + 32:]
    assert r1 == f
    assert r2 == i
    assert r3 == [v * n_inv % P for v in r2[:n]] + r2[n:]
    omega_inv = pow(8, P - 2, P)  # omega = psi^64 = 8
    assert r4 == [pow(omega_inv, 2 * (e % 16) + e // 16, P) for e in range(32)]
    assert r5 == [v * n_inv % P for v in r1[:n]] + r1[n:]


def test_split_block_table(dump, oracle):
    n, t = 4096, dump(4096, P)
    psi = int(oracle.Plan.try_new(n, P).twid[int(format(1, "012b")[::-1], 2)])
    assert t["twid"][1 << 11] == psi
    blk = t["blk"]
    assert len(blk) == 2 * n
    for b in range(2):
        alpha = pow(psi, (2 * b + 1 - 2) % (2 * n), P)  # bitrev_1(b) = b
        ainv = pow(alpha, P - 2, P)
        assert blk[b * 2048:(b + 1) * 2048] == [pow(alpha, j, P) for j in range(2048)]
        assert blk[n + b * 2048:n + (b + 1) * 2048] == [pow(ainv, j, P) for j in range(2048)]
    assert t["pow2_ok"] == [1] and t["root_ok"] == [1]
    assert t["pow2_bad"] == [0]  # entry 1 of twid perturbed
