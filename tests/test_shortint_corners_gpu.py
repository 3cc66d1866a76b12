"""The shortint atomic pattern and the radix drivers at their shape and alias corners (`-m gpu`).  tests/test_shortint_gpu.py
and tests/test_integer_gpu.py stay in one region: k = 1, the fused engines, at most 112 items, m = c = 4 decrypted,
no aliasing.  This file leaves it, one part per gap:

A  the index kernels of csrc/lwe_linear_algebra.hip (index_rule, lut_rule, index_pairs, mask_lut_index) on two and three
   workgroups: I = 29 integers of B = 9 blocks (T = 261, 2 T = 522, 29 packed rows in the scan round s = 8), and one
   apply of 600 items over 7 inputs, against the sequences of tests/shortint_gpu_helpers.py, whose index arrays are
   written in numpy.
B  k = 2 (N = 1024 on the NTT and f64 engines, N = 2048 on the multi-bit engine): the composites against their
   sequences, and the apply against the oracle's keyswitch and bootstrap, the one check of the key-LUT and LUT-list
   stride (k + 1) N that is not the library against itself.
C  the multi-pass, multi-lane bootstraps under the composite's scratch: N = 8192 at m = c = 8 (PARAM_MESSAGE_3_CARRY_3's
   shape), I = 8, B = 5: round 1 is 80 items on several lanes, the scan rounds 40 items with kept blocks on one.
D  decryption at (m, c) = (8, 8), (8, 4) (the single-carry form) and (2, 2), (4, 8) (the B-round fallback of
   mi_radix_full_propagate_batch, against shortint_ref.full_propagate, the model of the reference's sequential loop).
E  aliasing: radix_out == lhs, == rhs, == both; apply in place with in_index and n_items != n_in.  (The rejection of
   an overlapping carry_out is in tests/test_abi_shortint.py.)
F  the empty ends of the atomic pattern, and B = 1 at more than 64 items.

The noise margin of part D is a condition, measured on the host by tests/test_shortint_ref.py
test_real_key_sets_keep_two_bits_of_margin: the worst absolute phase error of the switched input and of the output of
one keyswitch + bootstrap stays at or below a quarter of the decoding half box 2^63 / (m c) / 2.  As log2 (input,
output | bound): "real" (N = 2048, n = 64, keyswitch 2^4 x 4) at (8, 4) and (4, 8) 54.00, 47.68 | 55, at (2, 2) under
2^54 | 58; "real4096" (N = 4096, n = 64, 2^4 x 6) at (8, 8) 52.58, 48.93 | 54; "real2048n16" (N = 2048, n = 16,
2^4 x 6; the multi-bit engine has N = 2048 only) at (8, 8) 53.00, 47.17 | 54.  "real" misses the condition at (8, 8)
(2^54.32 on one seed of three, with four or six keyswitch levels: the modulus switch dominates), so (8, 8) does not
run on it.  On the GPU the worst phase error of a decrypted output block of part D is printed by each test
(GPU_WORST_LOG2 below records the run this file was written with).

Left unpinned: the grid-stride loop of the four index kernels takes a second trip only above 4096 workgroups, 2^20
items (the drivers accept up to 2^22 - 1); that many bootstraps is out of reach of a test of seconds."""
import ctypes

import numpy as np
import pytest

import shortint_gpu_helpers as G
import shortint_ref as R
import tfhe_helpers as H

pytestmark = pytest.mark.gpu

SENTINEL = G.SENTINEL
# the worst |phase error| of a decrypted output block over part D on an MI355X, as log2, per key set
GPU_WORST_LOG2 = {"real": 48.59, "real4096": 49.29, "real2048n16": 49.01}
_worst = {}


def sentinel(shape):
    import torch
    return torch.full(shape, int(SENTINEL), dtype=torch.int64, device="cuda")


def c_stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return None if t is None else t.data_ptr()


def c_add(engine, sk, out, lhs, rhs, carry, blocks, n_int):
    return engine._lib.lib().mi_radix_add_batch(sk._h, ptr(out), ptr(lhs), ptr(rhs), ptr(carry), blocks, n_int, c_stream())


def c_apply(engine, sk, out, inp, n_in, in_index, luts, lut_index, n_items):
    return engine._lib.lib().mi_shortint_apply_lut_batch(sk._h, ptr(out), ptr(inp), n_in, ptr(in_index), ptr(luts),
                                                         ptr(lut_index), int(luts.shape[0]), n_items, c_stream())


def check_composite(engine, ks, sk, what, n_int, blocks, g):
    """One driver against the same LC / APPLY calls issued from Python, bit for bit, on uniform words."""
    import torch
    I = engine.integer.ServerKey(sk)
    m, top = sk.message_modulus, sk.max_degree
    words = H.uniform_u64(g, (2, n_int, blocks, ks.size))
    tag = (what, n_int, blocks)
    if what in ("propagate-carry", "propagate"):
        with_carry = what == "propagate-carry"
        got, want = G.dev(words[0]), G.dev(words[0])
        c_got, c_want = sentinel((n_int, ks.size)), sentinel((n_int, ks.size))
        I._propagate_single_carry(got, c_got if with_carry else None)
        G.seq_propagate(engine, sk, want, c_want if with_carry else None)
        assert torch.equal(got, want) and torch.equal(c_got, c_want), tag
        assert with_carry == bool((G.host(c_got) != SENTINEL).any()), tag
        assert not torch.equal(got, G.dev(words[0])), tag
    elif what == "full":
        ct = engine.integer.RadixCiphertext(G.dev(words[0]), [top] * blocks)
        want = G.dev(words[0])
        I.full_propagate_parallelized(ct)
        G.seq_full_propagate(engine, sk, want)
        assert torch.equal(ct.blocks, want) and not torch.equal(want, G.dev(words[0])), tag
    else:
        a = engine.integer.RadixCiphertext(G.dev(words[0]), [m - 1] * blocks)
        b = engine.integer.RadixCiphertext(G.dev(words[1]), [m - 1] * blocks)
        got, carry = I.unsigned_overflowing_add_parallelized(a, b)
        want, c_want = sentinel((n_int, blocks, ks.size)), sentinel((n_int, ks.size))
        G.seq_add(engine, sk, want, a.blocks, b.blocks, c_want)
        assert torch.equal(got.blocks, want) and torch.equal(carry, c_want), tag
        assert not (G.host(want) == SENTINEL).all(axis=-1).any() and not (G.host(c_want) == SENTINEL).all(axis=-1).any()


COMPOSITES = ["propagate-carry", "propagate", "full", "add"]


# ---- A: the index kernels across workgroups ----
@pytest.mark.parametrize("what", COMPOSITES)
def test_index_kernels_across_workgroups(engine, oracle, what):
    ks = G.key_set(engine, oracle, "u1024")
    check_composite(engine, ks, ks.server("ntt"), what, 29, 9, H.rng(0xc0a0 + COMPOSITES.index(what)))


def test_apply_600_items_over_7_inputs(engine, oracle):
    """mask_lut_index_kernel and the gather on three workgroups: in_index cycles through 0 .. 8 (7 and 8 out of range),
    lut_index through 0 .. 3 over 3 tables; kept rows keep the sentinel, past item 512 too."""
    import torch
    ks = G.key_set(engine, oracle, "u1024")
    sk = ks.server("ntt")
    g = H.rng(0xc0a8)
    n_items, n_in, n_lut = 600, 7, 3
    lwe, luts = G.dev(H.uniform_u64(g, (n_in, ks.size))), G.dev(H.uniform_u64(g, (n_lut, 2, ks.n)))
    j = np.arange(n_items)
    ii, li = G.i32(j % 9), G.i32(j % 4)
    got, want = sentinel((n_items, ks.size)), sentinel((n_items, ks.size))
    sk.apply_lookup_table_batch(got, lwe, luts, li, ii)
    G.seq_apply(engine, sk, want, lwe, luts, li, ii)
    assert torch.equal(got, want)
    kept = (G.host(got) == SENTINEL).all(axis=1)
    assert kept.tolist() == ((j % 9 >= n_in) | (j % 4 >= n_lut)).tolist()
    assert kept[512:].any() and not kept[512:].all()
    assert not (G.host(got)[~kept] == SENTINEL).any()


# ---- B: k = 2 ----
K2 = {"ntt-k2": ("u1024k2", "ntt", False), "fft-k2-drift": ("u1024k2", "fft", True),
      "multi-bit-k2": ("u2048k2", "multi-bit", False)}


def k2_server(engine, oracle, name):
    which, eng, drift = K2[name]
    ks = G.key_set(engine, oracle, which)
    assert ks.k == 2 and ks.size == 2 * ks.n + 1
    return ks, ks.server(eng, drift=drift)


@pytest.mark.parametrize("name", list(K2))
def test_apply_lut_equals_its_stages_k2(engine, oracle, name):
    import torch
    ks, sk = k2_server(engine, oracle, name)
    g = H.rng(0xc0b0 + list(K2).index(name))
    lwe, luts = G.dev(H.uniform_u64(g, (4, ks.size))), G.dev(H.uniform_u64(g, (3, 3, ks.n)))
    for in_index, lut_index in [([1, 1, 3, G.NONE, 0, 4, 2], [0, 1, 2, 0, 3, 1, 2]), (None, [2, 2, 0, 1]),
                                ([0, 1, 2], None)]:
        items = len(in_index or lut_index)
        got, want = sentinel((items, ks.size)), sentinel((items, ks.size))
        ii = None if in_index is None else G.i32(in_index)
        li = None if lut_index is None else G.i32(lut_index)
        sk.apply_lookup_table_batch(got, lwe, luts, li, ii)
        G.seq_apply(engine, sk, want, lwe, luts, li, ii)
        assert torch.equal(got, want), (name, in_index, lut_index)
        assert not (G.host(got) == SENTINEL).all(), name


@pytest.mark.parametrize("what", COMPOSITES)
@pytest.mark.parametrize("name", list(K2))
def test_radix_composites_equal_their_sequences_k2(engine, oracle, name, what):
    ks, sk = k2_server(engine, oracle, name)
    g = H.rng(0xc0b8 + 4 * list(K2).index(name) + COMPOSITES.index(what))
    for n_int, blocks in [(2, 1), (2, 3)]:
        check_composite(engine, ks, sk, what, n_int, blocks, g)


@pytest.mark.parametrize("mode", ["standard", "centered"])
def test_apply_lut_matches_oracle_k2(engine, oracle, mode):
    """The index pattern of test_shortint_gpu.py test_apply_lut_matches_oracle at k = 2, and the key's own tables
    (MSG and CARRY through message_extract / carry_extract's kind of call) against the oracle with tables filled by
    shortint_ref.lut_fill: the key-LUT stride and the body offset k N."""
    import torch
    ks = G.key_set(engine, oracle, "u1024k2")
    ms_mode = int(mode == "centered")
    sk = ks.server("ntt", False, ms_mode)
    g = H.rng(0xc0c0 + ms_mode)
    n_in, n_lut = 5, 3
    lwe = H.uniform_u64(g, (n_in, ks.size))
    luts = H.uniform_u64(g, (n_lut, 3, ks.n))
    in_index = [0, 0, 3, 1, G.NONE, 4, n_in, 2, 2]
    lut_index = [0, 2, 1, n_lut, 0, 2, 1, G.NONE, 1]
    out = sentinel((len(in_index), ks.size))
    sk.apply_lookup_table_batch(out, G.dev(lwe), G.dev(luts), G.i32(lut_index), G.i32(in_index))
    want, live = G.oracle_apply(oracle, ks, lwe, luts, lut_index, in_index, ms_mode, False, k=2)
    assert live.tolist() == [True, True, True, False, False, True, False, False, True]
    assert np.array_equal(G.host(out), want)
    # the key's own MSG and CARRY tables (tables 0 and 1 of its list): at m = c = 2 full propagation of one integer of
    # two blocks is two rounds of msg_0 | msg_1 + carry_0, here with tables filled by shortint_ref.lut_fill
    sk22 = ks.server("ntt", False, ms_mode, m=2, c=2)
    tables = np.stack([R.lut_fill(ks.n, 2, 2, 2, [0, 1, 0, 1]), R.lut_fill(ks.n, 2, 2, 2, [0, 0, 1, 1])])
    ct = engine.integer.RadixCiphertext(G.dev(lwe[:2].reshape(1, 2, ks.size)), [3] * 2)
    cur = lwe[:2]
    for _ in range(2):
        work, _ = G.oracle_apply(oracle, ks, cur, tables, [0, 0, 1, 1], [0, 1, 0, 1], ms_mode, False, k=2)
        with np.errstate(over="ignore"):
            cur = np.stack([work[0], work[1] + work[2]])
    engine.integer.ServerKey(sk22).full_propagate_parallelized(ct)
    assert np.array_equal(G.host(ct.blocks)[0], cur)


# ---- C: the multi-pass, multi-lane engines ----
@pytest.mark.parametrize("what", ["propagate-carry", "full", "add"])
@pytest.mark.parametrize("which", ["ntt", "fft"])
def test_composites_on_the_lane_engines(engine, oracle, which, what):
    ks = G.key_set(engine, oracle, "u8192")
    sk = ks.server(which, m=8, c=8)
    check_composite(engine, ks, sk, what, 8, 5, H.rng(0xc0d0 + 4 * (which == "fft") + COMPOSITES.index(what)))


def test_apply_lut_matches_oracle_at_8192(engine, oracle):
    ks = G.key_set(engine, oracle, "u8192")
    sk = ks.server("ntt", m=8, c=8)
    g = H.rng(0xc0d8)
    lwe, luts = H.uniform_u64(g, (2, ks.size)), H.uniform_u64(g, (2, 2, ks.n))
    in_index, lut_index = [1, 2, 0], [0, 1, 1]
    out = sentinel((3, ks.size))
    sk.apply_lookup_table_batch(out, G.dev(lwe), G.dev(luts), G.i32(lut_index), G.i32(in_index))
    want, live = G.oracle_apply(oracle, ks, lwe, luts, lut_index, in_index, 0, False)
    assert live.tolist() == [True, False, True]
    assert np.array_equal(G.host(out), want)


# ---- D: decryption at other moduli ----
def real_keys(engine, oracle, m, c, which):
    name = G.REAL_MULTI_BIT_8_8 if (which, m, c) == ("multi-bit", 8, 8) else G.REAL_FOR[(m, c)]
    ks = G.key_set(engine, oracle, name)
    return name, ks, ks.server(which, m=m, c=c)


def decrypted(name, ks, cts, m, c, expect=None):
    """Block values mod 2 m c; with the expected values, the worst phase error joins the record of the key set."""
    cts = G.host(cts)
    digits = G.decrypt_blocks(ks, cts, m, c)
    if expect is not None and np.array_equal(digits, np.asarray(expect)):
        worst = int(np.abs(G.phase_errors(cts, ks.big_sk, expect, m, c)).max())
        _worst[name] = max(_worst.get(name, 0), worst)
        print(f"worst output phase error so far under {name}: 2^{np.log2(max(_worst[name], 1)):.2f}")
    return digits


SINGLE = [(8, 8, "ntt"), (8, 8, "fft"), (8, 8, "multi-bit"), (8, 4, "ntt"), (8, 4, "fft")]
FALLBACK = [(2, 2, "ntt"), (2, 2, "fft"), (4, 8, "ntt"), (4, 8, "fft")]


@pytest.mark.parametrize("blocks", [1, 2, 3, 5])
@pytest.mark.parametrize("m,c,which", SINGLE, ids=[f"{m}-{c}-{w}" for m, c, w in SINGLE])
def test_add_decrypts(engine, oracle, m, c, which, blocks):
    """As test_integer_gpu.py test_add, at m = 8: STATE's x == m - 1 and SCAN's (x / m) % m at a modulus other than 4."""
    name, ks, sk = real_keys(engine, oracle, m, c, which)
    I = engine.integer.ServerKey(sk)
    g = H.rng(0xc1a0 + 64 * SINGLE.index((m, c, which)) + blocks)
    top = m**blocks
    pairs = [(top - 1, 1), (top - 1, top - 1), (0, 0), (1, top - 1)]
    pairs += [tuple(int(v) for v in g.integers(0, top, 2)) for _ in range(3)]
    a, b = (engine.integer.RadixCiphertext(
        G.dev(G.encrypt_blocks(ks, g, G.radix_digits([p[i] for p in pairs], blocks, m), m, c)), [m - 1] * blocks)
        for i in (0, 1))
    out, carry = I.unsigned_overflowing_add_parallelized(a, b)
    sums = [x + y for x, y in pairs]
    digits = decrypted(name, ks, out.blocks, m, c, G.radix_digits([s % top for s in sums], blocks, m))
    assert (digits < m).all(), digits
    assert G.radix_values(digits, m) == [s % top for s in sums]
    assert decrypted(name, ks, carry, m, c, [s // top for s in sums]).tolist() == [s // top for s in sums]
    assert G.radix_values(decrypted(name, ks, I.add_parallelized(a, b).blocks, m, c), m) == [s % top for s in sums]


def full_rows(g, m, c, blocks):
    """All blocks at m c - 1, a mixed row, a seeded row, and the ripple: a carry out of block 0 that every other block
    (at m - 1) passes on, the one row that needs all B rounds of the fallback (the others settle in two)."""
    mixed = [m * c - 1, 0, m * c - 1, m - 1, m * c - m]
    ripple = [m * c - 1] + [m - 1] * (blocks - 1)
    return np.array([[m * c - 1] * blocks, mixed[:blocks], list(g.integers(0, m * c, blocks)), ripple], dtype=np.uint64)


def check_full_propagate(engine, oracle, m, c, which, blocks, seed):
    name, ks, sk = real_keys(engine, oracle, m, c, which)
    I = engine.integer.ServerKey(sk)
    g = H.rng(seed)
    values = full_rows(g, m, c, blocks)
    ct = engine.integer.RadixCiphertext(G.dev(G.encrypt_blocks(ks, g, values, m, c)), [m * c - 1] * blocks)
    I.full_propagate_parallelized(ct)
    model = np.array([R.full_propagate([int(x) for x in row], m, c) for row in values])
    digits = decrypted(name, ks, ct.blocks, m, c, model)
    assert np.array_equal(digits, model), (digits, model)
    assert (digits < m).all() and G.radix_values(digits, m) == [v % m**blocks for v in G.radix_values(values, m)]
    assert ct.degrees == [m - 1] * blocks
    return I, ks, g


@pytest.mark.parametrize("m,c,which", SINGLE, ids=[f"{m}-{c}-{w}" for m, c, w in SINGLE])
def test_full_propagate_decrypts(engine, oracle, m, c, which):
    check_full_propagate(engine, oracle, m, c, which, 5, 0xc1b0 + SINGLE.index((m, c, which)))


@pytest.mark.parametrize("blocks", [1, 3, 5])
@pytest.mark.parametrize("m,c,which", FALLBACK, ids=[f"{m}-{c}-{w}" for m, c, w in FALLBACK])
def test_full_propagate_fallback_decrypts(engine, oracle, m, c, which, blocks):
    """(2, 2) and (4, 8) have no single-carry form: B extract-and-add rounds leave the blocks of the reference's
    sequential loop (shortint_ref.full_propagate), and the single-carry addition answers MI_ERR_UNSUPPORTED."""
    assert not R.single_carry_supported(m, c)
    I, ks, g = check_full_propagate(engine, oracle, m, c, which, blocks, 0xc1c0 + 8 * FALLBACK.index((m, c, which)) + blocks)
    if blocks > 1:
        clean = engine.integer.RadixCiphertext(G.dev(G.encrypt_blocks(ks, g, np.zeros((1, blocks), np.uint64), m, c)),
                                               [m - 1] * blocks)
        with pytest.raises(engine.MiError) as e:
            I.add_parallelized(clean, clean)
        assert e.value.status == 6


# ---- E: aliasing ----
@pytest.mark.parametrize("form", ["out-is-lhs", "out-is-rhs", "all-one"])
def test_add_in_place_equals_out_of_place(engine, oracle, form):
    import torch
    ks = G.key_set(engine, oracle, "u2048")
    sk = ks.server("ntt")
    n_int, blocks = 3, 5
    words = H.uniform_u64(H.rng(0xc0e0), (2, n_int, blocks, ks.size))
    lhs, rhs = G.dev(words[0]), G.dev(words[0 if form == "all-one" else 1])
    want, c_want = sentinel(lhs.shape), sentinel((n_int, ks.size))
    assert c_add(engine, sk, want, lhs, rhs, c_want, blocks, n_int) == 0
    assert torch.equal(lhs, G.dev(words[0])) and not (G.host(want) == SENTINEL).all(axis=-1).any()
    carry = sentinel((n_int, ks.size))
    if form == "out-is-lhs":
        assert c_add(engine, sk, lhs, lhs, rhs, carry, blocks, n_int) == 0
        assert torch.equal(lhs, want) and torch.equal(rhs, G.dev(words[1]))
    elif form == "out-is-rhs":
        assert c_add(engine, sk, rhs, lhs, rhs, carry, blocks, n_int) == 0
        assert torch.equal(rhs, want) and torch.equal(lhs, G.dev(words[0]))
    else:
        assert c_add(engine, sk, lhs, lhs, lhs, carry, blocks, n_int) == 0
        assert torch.equal(lhs, want)
    assert torch.equal(carry, c_want)


def test_add_to_itself_in_place_decrypts(engine, oracle):
    ks = G.key_set(engine, oracle, "real")
    sk = ks.server("ntt")
    g = H.rng(0xc0e8)
    m, blocks = G.MSG, 3
    top = m**blocks
    values = [top - 1, int(g.integers(0, top))]
    a = G.dev(G.encrypt_blocks(ks, g, G.radix_digits(values, blocks)))
    carry = sentinel((len(values), ks.size))
    assert c_add(engine, sk, a, a, a, carry, blocks, len(values)) == 0
    digits = G.decrypt_blocks(ks, G.host(a))
    assert (digits < m).all() and G.radix_values(digits) == [2 * v % top for v in values]
    assert G.decrypt_blocks(ks, G.host(carry)).tolist() == [2 * v // top for v in values]


@pytest.mark.parametrize("which", G.ENGINES)
def test_apply_in_place_with_in_index(engine, oracle, which):
    """lwe_out == lwe_in with n_in = 3 inputs in a buffer of n_items = 5 rows: every input is keyswitched before a row
    is written, the item whose in_index is out of range keeps what the buffer held."""
    import torch
    ks = G.key_set(engine, oracle, "u2048")
    sk = ks.server(which)
    g = H.rng(0xc0f0)
    words = H.uniform_u64(g, (5, ks.size))
    luts = G.dev(H.uniform_u64(g, (2, 2, ks.n)))
    ii, li = G.i32([2, 0, 7, 1, 0]), G.i32([0, 1, 1, 1, 0])
    want = G.dev(words)
    assert c_apply(engine, sk, want, G.dev(words[:3]), 3, ii, luts, li, 5) == 0
    buf = G.dev(words)
    assert c_apply(engine, sk, buf, buf, 3, ii, luts, li, 5) == 0
    assert torch.equal(buf, want)
    changed = (G.host(buf) != words).any(axis=1)
    assert changed.tolist() == [True, True, False, True, True]


# ---- F: the empty ends ----
@pytest.mark.parametrize("which", G.ENGINES)
def test_apply_with_nothing_to_do(engine, oracle, which):
    import torch
    ks = G.key_set(engine, oracle, "u2048")
    sk = ks.server(which)
    g = H.rng(0xc0f8)
    words = H.uniform_u64(g, (2, ks.size))
    lwe, luts = G.dev(words), G.dev(H.uniform_u64(g, (4, 2, ks.n)))
    li = G.i32([0, 1, 3, 0])
    out = sentinel((4, ks.size))
    # n_in = 0: no input at all (a NULL input is accepted), so every in_index is out of range
    assert c_apply(engine, sk, out, None, 0, G.i32([0, 1, G.NONE, 3]), luts, li, 4) == 0
    assert c_apply(engine, sk, out, lwe, 0, G.i32([0, 1, G.NONE, 3]), luts, None, 4) == 0
    # n_in = 2, every in_index out of range: the bootstrap gets a batch that is all 0xFFFFFFFF
    assert c_apply(engine, sk, out, lwe, 2, G.i32([2, 3, G.NONE, 1 << 31]), luts, li, 4) == 0
    assert c_apply(engine, sk, out, lwe, 2, G.i32([2, 3, G.NONE, 1 << 31]), luts, None, 4) == 0
    # n_items = 0, with and without buffers
    assert c_apply(engine, sk, out, lwe, 2, li, luts, None, 0) == 0
    assert c_apply(engine, sk, None, None, 0, None, luts, None, 0) == 0
    torch.cuda.synchronize()
    assert (G.host(out) == SENTINEL).all() and np.array_equal(G.host(lwe), words)


@pytest.mark.parametrize("what", ["propagate-carry", "propagate"])
@pytest.mark.parametrize("which", G.ENGINES)
def test_one_block_integers_past_64_items(engine, oracle, which, what):
    ks = G.key_set(engine, oracle, "u2048")
    check_composite(engine, ks, ks.server(which), what, 70, 1, H.rng(0xc100 + COMPOSITES.index(what)))
