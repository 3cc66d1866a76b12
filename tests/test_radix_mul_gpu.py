"""The radix sum of ciphertexts and the radix multiplication on the GPU (`-m gpu`).

A  bit for bit against the written sequences of tests/radix_mul_gpu_helpers.py (public calls driven by the Python
   model's schedule) on the five server configurations of tests/test_integer_gpu.py at (4, 4), uniform key words.
B  decryption under real keys; the noise condition is measured on the host by tests/test_radix_sum_ref.py
   test_linear_steps_stay_inside_the_box under the same key sets.
C  aliasing, untouched rows below first_block, the pass boundary of the scratch cap, the argument rules that need a
   key."""
import ctypes

import numpy as np
import pytest

import radix_mul_gpu_helpers as RM
import radix_sum_ref as S
import shortint_gpu_helpers as G
import shortint_ref as R
import tfhe_helpers as H

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 6
SERVERS = [("ntt", False), ("ntt", True), ("fft", False), ("fft", True), ("multi-bit", False)]
IDS = ["ntt", "ntt-drift", "fft", "fft-drift", "multi-bit"]
RAGGED = [0, 0, 1, 2, 2, 0, 1]


def sentinel(shape):
    import torch
    return torch.full(shape, int(G.SENTINEL), dtype=torch.int64, device="cuda")


def no_sentinel_row(t):
    return not (G.host(t) == G.SENTINEL).all(axis=-1).any()


# ---- A: the written sequences ----

@pytest.mark.parametrize("which,drift", SERVERS, ids=IDS)
def test_mul_equals_its_sequence(engine, oracle, which, drift):
    """B = 1 (one lsb table), 2, 4 (the smallest with a round: columns 1, 3, 5, 7, no carry out of the last) and 5 (a
    carry moved into a column that then needs a second round), three integers."""
    import torch
    ks = G.key_set(engine, oracle, "u2048")
    sk = ks.server(which, drift)
    for blocks in (1, 2, 4, 5):
        g = H.rng(0x6a00 + 8 * IDS.index(IDS[SERVERS.index((which, drift))]) + blocks)
        lhs, rhs = (G.dev(H.uniform_u64(g, (3, blocks, ks.size))) for _ in range(2))
        got, want = sentinel(lhs.shape), sentinel(lhs.shape)
        assert RM.c_mul(engine, sk, got, lhs, rhs, blocks, 3) == 0
        RM.seq_mul(engine, sk, want, lhs, rhs)
        assert torch.equal(got, want) and no_sentinel_row(got), blocks


@pytest.mark.parametrize("which,drift", SERVERS, ids=IDS)
def test_sum_equals_its_sequence(engine, oracle, which, drift):
    """13 dense terms of 3 blocks (two rounds), 2 terms, 1 term, no term, and a ragged first_block, two integers."""
    import torch
    ks = G.key_set(engine, oracle, "u2048")
    sk = ks.server(which, drift)
    blocks, n_int = 3, 2
    for n_terms, first in [(13, None), (2, None), (1, None), (0, None), (len(RAGGED), RAGGED)]:
        g = H.rng(0x6b00 + 16 * SERVERS.index((which, drift)) + n_terms)
        terms = G.dev(H.uniform_u64(g, (n_terms, n_int, blocks, ks.size))) if n_terms else None
        got, want = sentinel((n_int, blocks, ks.size)), sentinel((n_int, blocks, ks.size))
        assert RM.c_sum(engine, sk, got, terms, n_terms, first, blocks, n_int) == 0
        RM.seq_sum(engine, sk, want, terms, first)
        assert torch.equal(got, want) and no_sentinel_row(got), (n_terms, first)
        if n_terms == 0:
            assert not G.host(got).any()


# ---- B: decryption under real keys ----

def radix(engine, ks, g, values, blocks, m, c):
    digits = G.radix_digits(values, blocks, m, c)
    return engine.integer.RadixCiphertext(G.dev(G.encrypt_blocks(ks, g, digits, m, c)), [m - 1] * blocks)


def check_mul(engine, ks, sk, pairs, blocks, m, c, seed):
    I = engine.integer.ServerKey(sk)
    g = H.rng(seed)
    a = radix(engine, ks, g, [p[0] for p in pairs], blocks, m, c)
    b = radix(engine, ks, g, [p[1] for p in pairs], blocks, m, c)
    out = I.mul_parallelized(a, b)
    digits = G.decrypt_blocks(ks, G.host(out.blocks), m, c)
    top = m**blocks
    assert (digits < m).all(), digits
    assert G.radix_values(digits, m, c) == [(x * y) % top for x, y in pairs]
    assert out.degrees == [m - 1] * blocks
    for x, y in pairs:  # the model agrees (and no block of it passes m c - 1)
        assert R.value(S.mul(R.digits(x, m, blocks), R.digits(y, m, blocks), m, c), m) == (x * y) % top


@pytest.mark.parametrize("which", G.ENGINES)
def test_mul_decrypts_at_4_4(engine, oracle, which):
    """B = 5: 0, 1, the all-ones integer squared (every column full, every carry), pairs whose product ripples."""
    ks = G.key_set(engine, oracle, "real")
    blocks, top = 5, 4**5
    g = H.rng(0x6c00 + G.ENGINES.index(which))
    pairs = [(0, top - 1), (1, top - 1), (top - 1, top - 1), (top - 1, 1), (0x3FF, 0x3FF), (341, 3), (683, 682)]
    pairs += [tuple(int(v) for v in g.integers(0, top, 2)) for _ in range(3)]
    check_mul(engine, ks, ks.server(which), pairs, blocks, 4, 4, 0x6c10 + G.ENGINES.index(which))


def test_mul_decrypts_at_2_2(engine, oracle):
    """m = 2: no msb terms, s = 3, and the B-round fallback of the full propagation."""
    ks = G.key_set(engine, oracle, "real")
    pairs = [(15, 15), (0, 15), (1, 15), (7, 9), (13, 11), (5, 3), (10, 10)]
    check_mul(engine, ks, ks.server("ntt", m=2, c=2), pairs, 4, 2, 2, 0x6c20)


def test_mul_decrypts_at_8_8(engine, oracle):
    ks = G.key_set(engine, oracle, "real4096")
    top = 8**3
    pairs = [(top - 1, top - 1), (0, top - 1), (1, top - 1), (73, 7), (455, 333), (64, 8)]
    check_mul(engine, ks, ks.server("ntt", m=8, c=8), pairs, 3, 8, 8, 0x6c30)


def test_sum_of_13_terms_decrypts(engine, oracle):
    ks = G.key_set(engine, oracle, "real")
    I = engine.integer.ServerKey(ks.server("ntt"))
    blocks, top, n_terms = 3, 4**3, 13
    g = H.rng(0x6c40)
    values = [[top - 1] * n_terms, [0] * n_terms, [int(v) for v in g.integers(0, top, n_terms)],
              [int(v) for v in g.integers(0, top, n_terms)]]
    cts = [radix(engine, ks, g, [v[t] for v in values], blocks, 4, 4) for t in range(n_terms)]
    out = I.sum_ciphertexts_parallelized(cts)
    digits = G.decrypt_blocks(ks, G.host(out.blocks))
    assert (digits < 4).all(), digits
    assert G.radix_values(digits) == [sum(v) % top for v in values]
    assert I.unchecked_sum_ciphertexts_vec_parallelized([]) is None
    dirty = engine.integer.RadixCiphertext(cts[0].blocks, [6] * blocks)
    with pytest.raises(ValueError, match="clean"):
        I.sum_ciphertexts_parallelized([cts[1], dirty])
    with pytest.raises(ValueError, match="clean"):
        I.mul_parallelized(dirty, cts[1])


# ---- C: aliasing, untouched rows, the pass boundary, the argument rules ----

def test_aliasing(engine, oracle):
    """radix_out == lhs, radix_out == rhs and lhs == rhs equal the out-of-place call bit for bit."""
    import torch
    ks = G.key_set(engine, oracle, "u1024")
    sk = ks.server("ntt", True)
    blocks, n_int = 4, 3
    g = H.rng(0x6d00)
    a, b = H.uniform_u64(g, (n_int, blocks, ks.size)), H.uniform_u64(g, (n_int, blocks, ks.size))
    want = sentinel((n_int, blocks, ks.size))
    assert RM.c_mul(engine, sk, want, G.dev(a), G.dev(b), blocks, n_int) == 0
    lhs, rhs = G.dev(a), G.dev(b)
    assert RM.c_mul(engine, sk, lhs, lhs, rhs, blocks, n_int) == 0
    assert torch.equal(lhs, want) and torch.equal(rhs, G.dev(b))
    lhs, rhs = G.dev(a), G.dev(b)
    assert RM.c_mul(engine, sk, rhs, lhs, rhs, blocks, n_int) == 0
    assert torch.equal(rhs, want) and torch.equal(lhs, G.dev(a))
    square = sentinel((n_int, blocks, ks.size))
    assert RM.c_mul(engine, sk, square, G.dev(a), G.dev(a), blocks, n_int) == 0
    lhs, out = G.dev(a), sentinel((n_int, blocks, ks.size))
    assert RM.c_mul(engine, sk, out, lhs, lhs, blocks, n_int) == 0
    assert torch.equal(out, square) and not torch.equal(square, want)
    assert RM.c_mul(engine, sk, lhs, lhs, lhs, blocks, n_int) == 0  # all three the same buffer
    assert torch.equal(lhs, square)


def test_rows_below_first_block_are_untouched(engine, oracle):
    """Rows below first_block hold a sentinel, then other words: the result is the same, and the terms keep their
    words."""
    import torch
    ks = G.key_set(engine, oracle, "u1024")
    sk = ks.server("fft")
    blocks, n_int = 3, 2
    g = H.rng(0x6d10)
    live = H.uniform_u64(g, (len(RAGGED), n_int, blocks, ks.size))
    results = []
    for fill in (np.uint64(G.SENTINEL), np.uint64(0xFFFFFFFFFFFFFFFF)):
        words = live.copy()
        for t, f in enumerate(RAGGED):
            words[t, :, :f] = fill
        terms = G.dev(words)
        out = sentinel((n_int, blocks, ks.size))
        assert RM.c_sum(engine, sk, out, terms, len(RAGGED), RAGGED, blocks, n_int) == 0
        assert torch.equal(terms, G.dev(words))
        results.append(out)
    assert torch.equal(results[0], results[1]) and no_sentinel_row(results[0])
    # reading them would change the result: with first_block all 0 the same buffers give something else
    other = sentinel((n_int, blocks, ks.size))
    assert RM.c_sum(engine, sk, other, terms, len(RAGGED), None, blocks, n_int) == 0
    assert not torch.equal(other, results[1])


def test_pass_boundary(engine, oracle):
    """The real scratch cap at N = 1024: a batch two integers longer than a pass equals the two per-pass calls bit for
    bit, and the pool then holds no more than the per-pass calls leave (no block for the whole batch); a repeated
    call leaves it as it is."""
    import torch
    M = engine.ntt64_pbs
    ks = G.key_set(engine, oracle, "u1024")
    sk = ks.server("ntt")
    blocks = 2
    n = ctypes.c_size_t()
    lib = engine._lib.lib()
    assert lib.mi_radix_mul_pass_integers(sk._h, blocks, 1 << 20, ctypes.byref(n)) == 0
    per_pass = n.value
    n_int = per_pass + 2
    print(f"pass boundary: {per_pass} integers of {blocks} blocks per pass")
    assert lib.mi_radix_mul_pass_integers(sk._h, blocks, 5, ctypes.byref(n)) == 0 and n.value == 5
    g = H.rng(0x6d20)
    a = G.dev(H.uniform_u64(g, (n_int, blocks, ks.size)))
    b = G.dev(H.uniform_u64(g, (n_int, blocks, ks.size)))
    parts = sentinel(a.shape)
    torch.cuda.synchronize()
    M.scratch_trim(0)
    assert RM.c_mul(engine, sk, parts[:per_pass], a[:per_pass], b[:per_pass], blocks, per_pass) == 0
    assert RM.c_mul(engine, sk, parts[per_pass:], a[per_pass:], b[per_pass:], blocks, 2) == 0
    torch.cuda.synchronize()
    one_pass = M.scratch_bytes(0)  # what the two per-pass calls leave
    whole = sentinel(a.shape)
    M.scratch_trim(0)
    assert RM.c_mul(engine, sk, whole, a, b, blocks, n_int) == 0
    torch.cuda.synchronize()
    assert torch.equal(whole, parts) and no_sentinel_row(whole)
    after = M.scratch_bytes(0)
    assert 0 < after <= one_pass, (after, one_pass)
    assert RM.c_mul(engine, sk, whole, a, b, blocks, n_int) == 0  # repeated: the pool does not grow
    torch.cuda.synchronize()
    assert M.scratch_bytes(0) == after and torch.equal(whole, parts)


def test_argument_rules_with_a_key(engine, oracle):
    """Answered before any device call: the buffers keep their words."""
    import torch
    ks = G.key_set(engine, oracle, "u1024")
    sk = ks.server("ntt")
    lib = engine._lib.lib()
    size, row = ks.size, 8 * ks.size
    buf = sentinel((16, size))
    p = buf.data_ptr()

    def answered(st, status, text):
        msg = lib.mi_last_error_message().decode()
        assert st == status and text in msg, (st, msg)

    mul, add = lib.mi_radix_mul_batch, lib.mi_radix_sum_batch
    answered(mul(sk._h, p, p + 4 * row, p + 8 * row, 0, 1, None), INVALID, "n_blocks is 0")
    answered(add(sk._h, p, p + 4 * row, 2, None, 0, 1, None), INVALID, "n_blocks is 0")
    answered(mul(sk._h, p, p + row, p + 8 * row, 2, 2, None), INVALID, "partially overlaps")
    answered(mul(sk._h, p + row, p + 8 * row, p, 2, 2, None), INVALID, "partially overlaps")
    answered(add(sk._h, p + 2 * row, p, 2, None, 2, 1, None), INVALID, "radix_out overlaps terms")
    answered(add(sk._h, p, p, 1, None, 2, 1, None), INVALID, "radix_out overlaps terms")
    answered(mul(sk._h, p, p, p, 1 << 21, 2, None), INVALID, "batch too large")
    answered(add(sk._h, p, p + 8 * row, 1 << 12, None, 1 << 12, 1, None), INVALID, "batch too large")
    answered(mul(sk._h, None, p, p, 2, 1, None), INVALID, "buffer is NULL")
    answered(add(sk._h, p, None, 2, None, 2, 1, None), INVALID, "buffer is NULL")
    fb = (ctypes.c_uint32 * 2)(0, 3)
    answered(add(sk._h, p, p + 4 * row, 2, fb, 2, 1, None), INVALID, "first_block is past the end")
    answered(mul(sk._h, p, p, p, 129, 1, None), UNSUPPORTED, "at most 128 blocks")
    answered(add(sk._h, p, p + 4 * row, 1, None, 129, 0, None), UNSUPPORTED, "at most 128 blocks")
    assert mul(sk._h, None, None, None, 3, 0, None) == 0 and add(sk._h, None, None, 3, None, 3, 0, None) == 0
    four_eight = ks.server("ntt", m=4, c=8)
    answered(four_eight_call(lib, four_eight, p, row), UNSUPPORTED, "carry_modulus")
    eight_four = ks.server("ntt", m=8, c=4)
    answered(mul(eight_four._h, p, p, p, 2, 1, None), UNSUPPORTED, "carry_modulus must equal message_modulus")
    torch.cuda.synchronize()
    assert (G.host(buf) == G.SENTINEL).all()


def four_eight_call(lib, key, p, row):
    return lib.mi_radix_sum_batch(key._h, p, p + 4 * row, 2, None, 2, 1, None)


# ---- D: the index kernels ----

@pytest.mark.parametrize("m,c", [(4, 4), (2, 2)], ids=["4-4", "2-2"])
def test_index_arrays_equal_the_model(engine, m, c):
    """B = 32 x 5 integers: every index array the driver writes on the device (the triangular pair rule and every
    round of the schedule kernel, 5120 product rows at (4, 4): twenty workgroups), copied back and compared with the
    arrays made from the model's schedule."""
    import torch
    blocks, n_int = 32, 5
    lib = engine._lib.lib()
    want = RM.model_index_arrays(blocks, n_int, m, c)
    cap = max(len(a) for step in want for a in step.values() if a is not None)
    assert cap > 4 * 256
    for step, arrays in enumerate(want):
        index, in_index, lut_index = (torch.full((cap + 8,), -2, dtype=torch.int32, device="cuda") for _ in range(3))
        coeff = torch.full((cap + 8,), -2, dtype=torch.int64, device="cuda")
        n_index, n_items = ctypes.c_size_t(), ctypes.c_size_t()
        st = lib.mi_radix_mul_index_arrays(m, c, blocks, n_int, step, index.data_ptr(), coeff.data_ptr(),
                                           in_index.data_ptr(), lut_index.data_ptr(), cap, ctypes.byref(n_index),
                                           ctypes.byref(n_items), 0, RM.c_stream())
        assert st == 0, lib.mi_last_error_message()
        torch.cuda.synchronize()
        assert n_index.value == len(arrays["index"]), step
        assert n_items.value == (0 if arrays["in_index"] is None else len(arrays["in_index"])), step
        got = {"index": index, "coeff": coeff, "in_index": in_index, "lut_index": lut_index}
        for name, a in arrays.items():
            if a is None or name == "coeff" and step > 0:
                continue
            h = got[name].cpu().numpy()
            h = h.view(np.uint32) if name != "coeff" else h
            assert np.array_equal(h[:len(a)].astype(np.int64), np.asarray(a, dtype=np.int64)), (step, name)
            if step == 0:  # a later step leaves the earlier steps' entries behind: only here nothing follows the arrays
                assert (got[name].cpu().numpy()[len(a):] == -2).all(), (step, name)
    st = lib.mi_radix_mul_index_arrays(m, c, blocks, n_int, len(want), index.data_ptr(), coeff.data_ptr(),
                                       in_index.data_ptr(), lut_index.data_ptr(), cap, None, None, 0, None)
    assert st == INVALID and b"step is past" in lib.mi_last_error_message()
    st = lib.mi_radix_mul_index_arrays(m, c, blocks, n_int, 1, index.data_ptr(), coeff.data_ptr(),
                                       in_index.data_ptr(), lut_index.data_ptr(), 16, None, None, 0, None)
    assert st == INVALID and b"capacity" in lib.mi_last_error_message()
