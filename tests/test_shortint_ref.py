"""The host restatement of the shortint lookup tables and the radix carry propagation (tests/shortint_ref.py) against
first principles, and the library's host functions against it (no GPU): the LUT fill, the propagation on cleartext
blocks (exhaustive where it is small), the three one-off mutants, and the argument rules of mi_shortint_key_create
(mi_shortint_key_check states them on plain numbers)."""
import itertools

import numpy as np
import pytest

import shortint_ref as R
import tfhe_helpers as H

M = C = 4


@pytest.mark.parametrize("n,k,m,c", [(2048, 1, 4, 4), (1024, 1, 4, 4), (1024, 2, 2, 2), (512, 1, 8, 8), (64, 1, 4, 8)])
def test_lut_fill_is_the_pbs_lut_and_the_library(engine, n, k, m, c):
    f = lambda x: (5 * x * x + 3) % (m * c)
    table = [f(x) for x in range(m * c)]
    ref = R.lut_fill(n, k, m, c, table)
    assert np.array_equal(ref, H.pbs_lut(n, k, m * c, (1 << 63) // (m * c), f))
    got = engine.shortint.lut_fill(n, k, m, c, table)
    assert got.tobytes() == ref.tobytes()
    # values above m c wrap as the reference's wrapping_mul does
    wide = [(1 << 64) - 1 - x for x in range(m * c)]
    assert engine.shortint.lut_fill(n, k, m, c, wide).tobytes() == R.lut_fill(n, k, m, c, wide).tobytes()


def test_lut_fill_at_one_coefficient_per_box(engine):
    """m c = N / 2 is the largest table: boxes of two coefficients, a half box of one."""
    n, m, c = 64, 4, 8
    table = list(range(m * c))
    got = engine.shortint.lut_fill(n, 1, m, c, table)
    assert got.tobytes() == R.lut_fill(n, 1, m, c, table).tobytes()
    assert int(got[1, n - 1]) == 0 and int(got[1, 0]) == 0 and int(got[1, 1]) == (1 << 63) // (m * c)


def test_lut_fill_rejections(engine):
    from tfhe_ntt_amd import MiError

    for args in [(2048, 1, 3, 4, [0] * 12), (2048, 1, 4, 4, [0] * 15), (2048, 1, 64, 32, [0] * 2048), (100, 1, 4, 4, [0] * 16),
                 (2048, 0, 4, 4, [0] * 16)]:
        with pytest.raises(MiError) as e:
            engine.shortint.lut_fill(*args)
        assert e.value.status == 1


def test_bivariate_table_indexing():
    t = R.bivariate_table(M, C, lambda a, b: 10 * a + b)
    assert [t[M * a + b] for a in range(M) for b in range(M)] == [10 * a + b for a in range(M) for b in range(M)]


def check_propagation(blocks, m=M, c=C):
    out, carry, rounds = R.propagate_single_carry(blocks, m, c)
    total = R.value(blocks, m)
    b = len(blocks)
    assert all(0 <= x < m for x in out), (blocks, out)
    assert R.value(out, m) == total % m**b and carry == total // m**b, (blocks, out, carry)
    assert rounds == (1 if b == 1 else 2 + (b - 1).bit_length())


@pytest.mark.parametrize("n_blocks", [1, 2, 3])
def test_propagation_exhaustive(n_blocks):
    for blocks in itertools.product(range(2 * (M - 1) + 1), repeat=n_blocks):
        check_propagation(list(blocks))


@pytest.mark.parametrize("n_blocks", [4, 5, 8, 9])
def test_propagation_random(n_blocks):
    g = H.rng(0x5a00 + n_blocks)
    cases = [[M - 1] * n_blocks, [2 * (M - 1)] * n_blocks, [0] * n_blocks, [M] + [M - 1] * (n_blocks - 1),
             [2 * (M - 1)] + [M - 1] * (n_blocks - 1)]
    cases += [list(map(int, g.integers(0, 2 * (M - 1) + 1, n_blocks))) for _ in range(400)]
    # long PROPAGATED runs behind a GENERATED block are what the scan is for
    cases += [list(map(int, np.where(g.integers(0, 4, n_blocks) == 0, g.integers(0, 7, n_blocks), M - 1)))
              for _ in range(400)]
    for blocks in cases:
        check_propagation(blocks)


def test_scan_round_count():
    assert [R.scan_rounds(b) for b in (1, 2, 3, 4, 5, 8, 9, 32)] == [0, 1, 2, 2, 3, 3, 4, 5]


@pytest.mark.parametrize("m,c", [(4, 4), (2, 2), (2, 4), (8, 2), (8, 8)])
@pytest.mark.parametrize("n_blocks", [1, 2, 3, 5, 8])
def test_full_propagation_from_full_blocks(m, c, n_blocks):
    """Every block at m c - 1, and random blocks: the integer is the sum of the block values mod m^B."""
    g = H.rng(0x5b00 + 16 * m + c)
    for blocks in [[m * c - 1] * n_blocks] + [list(map(int, g.integers(0, m * c, n_blocks))) for _ in range(50)]:
        out = R.full_propagate(blocks, m, c)
        assert all(0 <= x < m for x in out)
        assert R.value(out, m) == R.value(blocks, m) % m**n_blocks


def test_add_is_the_integer_sum():
    g = H.rng(0x5c00)
    for n_blocks in (1, 2, 3, 5, 8):
        top = M**n_blocks
        pairs = [(top - 1, 1), (top - 1, top - 1), (0, 0)] + [tuple(map(int, g.integers(0, top, 2))) for _ in range(100)]
        for a, b in pairs:
            out, carry, _ = R.add(R.digits(a, M, n_blocks), R.digits(b, M, n_blocks), M, C)
            assert (R.value(out, M), carry) == ((a + b) % top, (a + b) // top)


def _wrong_somewhere(rule, shapes):
    for n_blocks, blocks in shapes:
        try:
            out, carry, _ = R.propagate_single_carry(blocks, M, C, rule)
        except OverflowError:
            return True
        total = R.value(blocks, M)
        if R.value(out, M) != total % M**n_blocks or carry != total // M**n_blocks:
            return True
    return False


@pytest.mark.parametrize("rule", [R.Rule(scan_offset=1), R.Rule(block0_propagated=True),
                                  R.Rule(drop_last_scan_round=True)],
                         ids=["scan-offset", "block0-propagated", "dropped-round"])
def test_the_model_tells_the_mutants(rule):
    """Each one-off mutant gives a wrong integer or carry on some input of the sets the true rule passes on."""
    shapes = [(b, list(blocks)) for b in (2, 3) for blocks in itertools.product(range(2 * (M - 1) + 1), repeat=b)]
    shapes += [(5, [M] + [M - 1] * 4), (5, [M - 1] * 5), (9, [M] + [M - 1] * 8)]
    assert not _wrong_somewhere(R.Rule(), shapes)
    assert _wrong_somewhere(rule, shapes)


# ---- the argument rules of mi_shortint_key_create ----
NTT, FFT, MULTI = 0, 1, 2
BNF, SOLINAS = 1, 0
GOOD = dict(ksk_in=2048, ksk_out=918, n_lwe=918, k=1, n=2048, pbs=NTT, variant=BNF, has_ms=0, ms_dim=0, ms_mode=0,
            m=4, c=4)


def key_check(engine, **change):
    from tfhe_ntt_amd import _lib

    a = dict(GOOD, **change)
    st = _lib.lib().mi_shortint_key_check(a["ksk_in"], a["ksk_out"], a["n_lwe"], a["k"], a["n"], a["pbs"], a["variant"],
                                          a["has_ms"], a["ms_dim"], a["ms_mode"], a["m"], a["c"])
    return st, _lib.lib().mi_last_error_message().decode() if st else ""


def test_key_check_accepts(engine):
    for change in [{}, dict(pbs=FFT), dict(pbs=MULTI), dict(ms_mode=1), dict(has_ms=1, ms_dim=918),
                   dict(pbs=FFT, has_ms=1, ms_dim=918), dict(m=32, c=32), dict(k=2, ksk_in=4096), dict(m=2, c=1)]:
        assert key_check(engine, **change) == (0, ""), change


@pytest.mark.parametrize("change,status,text", [
    (dict(pbs=3), 1, "unknown pbs engine"),
    (dict(variant=SOLINAS), 6, "Solinas-variant"),
    (dict(ksk_out=917), 1, "output dimension"),
    (dict(ksk_in=2047), 1, "input dimension"),
    (dict(k=2), 1, "input dimension"),
    (dict(m=3), 1, "powers of two"),
    (dict(c=0), 1, "powers of two"),
    (dict(m=64, c=32), 1, "at most N / 2"),
    (dict(m=1 << 40, c=1 << 40), 1, "at most N / 2"),
    (dict(ms_mode=2), 1, "ms_mode"),
    (dict(pbs=MULTI, has_ms=1, ms_dim=918), 1, "multi-bit"),
    (dict(pbs=MULTI, ms_mode=1), 1, "multi-bit"),
    (dict(has_ms=1, ms_dim=918, ms_mode=1), 1, "drift"),
    (dict(has_ms=1, ms_dim=900), 1, "ms-noise key's dimension"),
])
def test_key_check_rejects(engine, change, status, text):
    st, msg = key_check(engine, **change)
    assert st == status and text in msg, (change, st, msg)


# ---- the noise condition of the decrypting tests at other moduli (tests/test_shortint_corners_gpu.py, part D) ----
@pytest.mark.parametrize("name,m,c,multi_bit", [("real", 8, 4, False), ("real4096", 8, 8, False),
                                                ("real2048n16", 8, 8, False), ("real2048n16", 8, 8, True)],
                         ids=["real-8-4", "real4096-8-8", "real2048n16-8-8", "real2048n16-8-8-multi-bit"])
def test_real_key_sets_keep_two_bits_of_margin(engine, oracle, name, m, c, multi_bit):
    """Every value 0 .. m c - 1 through keyswitch, modulus switch and the identity bootstrap of the reference
    restatements under the real key set that the GPU tests decrypt with at (m, c), at the tightest (m, c) of each
    set: the worst absolute phase error of the switched input and of the output stays at or below a quarter of the
    decoding half box 2^63 / (m c) / 2, because the radix drivers add up to m + 1 outputs before the next bootstrap.

    Measured, as log2 (input, output | bound): real (N = 2048, n = 64, keyswitch 2^4 x 4) at (8, 4) 54.00, 47.68 | 55;
    real4096 (N = 4096, n = 64, 2^4 x 6) at (8, 8) 52.58, 48.93 | 54; real2048n16 (N = 2048, n = 16, 2^4 x 6) at
    (8, 8) 53.00, 47.17 | 54, and 53.00 through the multi-bit switch.  The present set "real" does not meet the
    condition at (8, 8): over three seeds its worst input error is 2^54.00, 2^54.32 and 2^54.00 against 2^54, and
    six keyswitch levels leave that as it is (2^54.32, 2^53.58, 2^54.00), because the modulus switch to 2 N = 4096
    over n = 64 key bits is what dominates (a standard deviation near 2^52.7); hence N = 4096 for (8, 8), and n = 16
    for the multi-bit engine, which has N = 2048 only."""
    import shortint_gpu_helpers as G

    ks = G.key_set(engine, oracle, name, device=False)
    e_in, e_out = G.measure_noise(oracle, ks, m, c, 0x5e00 + m * c, multi_bit)
    bound = (1 << 63) // (m * c) // 2 // 4
    print(f"noise margin {name} ({m}, {c}){' multi-bit' if multi_bit else ''}: input 2^{np.log2(e_in):.2f}, "
          f"output 2^{np.log2(e_out):.2f}, bound 2^{np.log2(bound):.2f}")
    assert e_in <= bound and e_out <= bound, (e_in, e_out, bound)
