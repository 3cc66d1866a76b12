"""Radix integers under real keys (`-m gpu`): every result is decrypted.  The key set has PARAM_MESSAGE_2_CARRY_2's
shape (N = 2048, k = 1, m = c = 4, keyswitch base 2^4 with 4 levels, bootstrap base 2^23 with 1 level) over a small
LWE dimension of 64, as test_keyswitch_decrypts_and_feeds_pbs builds it, and serves the NTT engine, the f64 engine and the
multi-bit engine at grouping factor 2 (tests/shortint_gpu_helpers.py, made once per process)."""
import numpy as np
import pytest

import shortint_gpu_helpers as G
import tfhe_helpers as H

pytestmark = pytest.mark.gpu

M = G.MSG
SERVERS = [("ntt", False), ("ntt", True), ("fft", False), ("fft", True), ("multi-bit", False)]
IDS = ["ntt", "ntt-drift", "fft", "fft-drift", "multi-bit"]


@pytest.fixture(scope="module")
def keys(engine, oracle):
    return G.key_set(engine, oracle, "real")


def radix(engine, ks, g, values, blocks, degree=M - 1):
    return engine.integer.RadixCiphertext(G.dev(G.encrypt_blocks(ks, g, G.radix_digits(values, blocks))), [degree] * blocks)


def decrypted(ks, ct):
    return G.decrypt_blocks(ks, G.host(ct.blocks if hasattr(ct, "blocks") else ct))


@pytest.mark.parametrize("which,drift", SERVERS, ids=IDS)
@pytest.mark.parametrize("blocks", [1, 2, 3, 5, 8])
def test_add(engine, keys, which, drift, blocks):
    """The all-ones integer plus 1 (the ripple through every block), max + max, 0 + 0 and random pairs: every output
    block decrypts below m, the integer is (a + b) mod m^B and the carry block the true carry."""
    I = engine.integer.ServerKey(keys.server(which, drift))
    g = H.rng(0x1a00 + 16 * blocks + IDS.index(which + ("-drift" if drift else "")))
    top = M**blocks
    pairs = [(top - 1, 1), (top - 1, top - 1), (0, 0), (1, top - 1)]
    pairs += [tuple(int(v) for v in g.integers(0, top, 2)) for _ in range(3)]
    a = radix(engine, keys, g, [p[0] for p in pairs], blocks)
    b = radix(engine, keys, g, [p[1] for p in pairs], blocks)
    out, carry = I.unsigned_overflowing_add_parallelized(a, b)
    digits = decrypted(keys, out)
    assert (digits < M).all(), digits
    assert G.radix_values(digits) == [(x + y) % top for x, y in pairs]
    assert decrypted(keys, carry).tolist() == [(x + y) // top for x, y in pairs]
    assert out.degrees == [M - 1] * blocks
    assert G.radix_values(decrypted(keys, I.add_parallelized(a, b))) == [(x + y) % top for x, y in pairs]


@pytest.mark.parametrize("which,drift", SERVERS, ids=IDS)
def test_full_propagate_from_full_blocks(engine, keys, which, drift):
    I = engine.integer.ServerKey(keys.server(which, drift))
    g = H.rng(0x1b00)
    blocks = 5
    values = np.array([[15] * blocks, [15, 0, 15, 3, 12], list(g.integers(0, 16, blocks))], dtype=np.uint64)
    ct = engine.integer.RadixCiphertext(G.dev(G.encrypt_blocks(keys, g, values)), [15] * blocks)
    I.full_propagate_parallelized(ct)
    digits = decrypted(keys, ct)
    assert (digits < M).all(), digits
    assert G.radix_values(digits) == [v % M**blocks for v in G.radix_values(values)]
    assert ct.degrees == [M - 1] * blocks


@pytest.mark.parametrize("which,drift", [("ntt", False), ("fft", True), ("multi-bit", False)],
                         ids=["ntt", "fft-drift", "multi-bit"])
def test_scalar_add_bitwise_and_unchecked(engine, keys, which, drift):
    sk = keys.server(which, drift)
    I = engine.integer.ServerKey(sk)
    g = H.rng(0x1c00)
    blocks, top = 3, M**3
    xs, ys = [63, 0, 27, 41], [63, 5, 38, 22]
    a, b = radix(engine, keys, g, xs, blocks), radix(engine, keys, g, ys, blocks)
    for scalar in (1, 37, top - 1, top + 2):
        assert G.radix_values(decrypted(keys, I.scalar_add_parallelized(a, scalar))) == [(x + scalar) % top for x in xs]
    for op, f in (("and", lambda x, y: x & y), ("or", lambda x, y: x | y), ("xor", lambda x, y: x ^ y)):
        out = getattr(I, f"bit{op}_parallelized")(a, b)
        assert G.radix_values(decrypted(keys, out)) == [f(x, y) for x, y in zip(xs, ys)], op
    # the unchecked sum keeps the carries in the blocks; full propagation then gives the integer
    s = I.unchecked_add(a, b)
    assert s.degrees == [2 * (M - 1)] * blocks
    assert (decrypted(keys, s) == G.radix_digits(xs, blocks) + G.radix_digits(ys, blocks)).all()
    I.full_propagate_parallelized(s)
    assert G.radix_values(decrypted(keys, s)) == [(x + y) % top for x, y in zip(xs, ys)]
    # shortint: a lookup table per item, the bivariate form, the extracts, the scalar operations
    blocks4 = G.dev(G.encrypt_blocks(keys, g, np.array([0, 5, 10, 15], dtype=np.uint64)))
    luts = G.dev(np.stack([G.host(sk.generate_lookup_table(lambda x: (x + 1) % 16)),
                           G.host(sk.generate_lookup_table(lambda x: (3 * x) % 16))]))
    got = G.decrypt_blocks(keys, G.host(sk.apply_lookup_table(blocks4, luts, G.i32([0, 1, 1, 0]))))
    assert got.tolist() == [1, 15, 14, 0]
    assert G.decrypt_blocks(keys, G.host(sk.message_extract(blocks4))).tolist() == [0, 1, 2, 3]
    assert G.decrypt_blocks(keys, G.host(sk.carry_extract(blocks4))).tolist() == [0, 1, 2, 3]
    lhs = G.dev(G.encrypt_blocks(keys, g, np.array([0, 1, 2, 3], dtype=np.uint64)))
    rhs = G.dev(G.encrypt_blocks(keys, g, np.array([3, 3, 1, 2], dtype=np.uint64)))
    mul = sk.generate_lookup_table_bivariate(lambda x, y: (x * y) % M)
    assert G.decrypt_blocks(keys, G.host(sk.unchecked_apply_lookup_table_bivariate(lhs, rhs, mul))).tolist() == [0, 3, 2, 2]
    assert G.decrypt_blocks(keys, G.host(sk.unchecked_scalar_add(lhs, 5))).tolist() == [5, 6, 7, 8]
    assert G.decrypt_blocks(keys, G.host(sk.unchecked_scalar_mul(lhs, 3))).tolist() == [0, 3, 6, 9]


def test_degree_guard(engine, keys):
    I = engine.integer.ServerKey(keys.server("ntt"))
    g = H.rng(0x1d00)
    a = radix(engine, keys, g, [5], 2)
    s = a
    for _ in range(4):  # degrees 6, 9, 12, 15
        s = I.unchecked_add(s, a)
    assert s.degrees == [15, 15]
    with pytest.raises(ValueError, match="degree 18"):
        I.unchecked_add(s, a)
    with pytest.raises(ValueError, match="clean"):
        I.add_parallelized(s, a)
    with pytest.raises(ValueError):
        engine.integer.RadixCiphertext(a.blocks, [3])
