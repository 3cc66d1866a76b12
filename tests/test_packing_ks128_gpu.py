"""GPU parity of the 128-bit LWE packing keyswitch and GLWE compression against packing128_helpers.py (`-m gpu`).

Bar: bit-exact vs the vectorised reference (pinned to the transcription of lwe_packing_keyswitch.rs:102-187, 296-379
by tests/test_packing_ks128_ref.py) and vs plain big-integer sums: the tile edges of the GEMM mod 2^128 on the int8
matrix cores, the decomposer's corner words, the int32 accumulators at the depth rule's edge, the production shape,
the chunked and piecewise scratch plans, compress / extract against the big-integer restatement of packed_integers.rs,
a functional round trip with real keys, and the argument checks.  A u128 tensor is (..., 2) words (lo, hi).
"""
import ctypes

import numpy as np
import pytest

import packing128_helpers as Q
import pbs128_helpers as R

pytestmark = pytest.mark.gpu

SHAPES = [(61, 1), (24, 3), (4, 3), (7, 2), (8, 1), (63, 2)]  # (base_log, level)


def dev(words):
    import torch
    return torch.from_numpy(np.ascontiguousarray(words, dtype=np.uint64).view(np.int64)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


def filled(shape):
    """-1 everywhere: every word must be written."""
    import torch
    return torch.full(shape, -1, dtype=torch.int64, device="cuda")


def zeros(shape):
    import torch
    return torch.zeros(shape, dtype=torch.int64, device="cuda")


def uniform_words(g, shape):
    return g.integers(0, 1 << 64, size=tuple(shape) + (2,), dtype=np.uint64)


def run_pack(engine, key, lwe, k, n, lwe_per_glwe):
    K = engine.noise_squashing_compression
    n_glwe = (lwe.shape[0] + lwe_per_glwe - 1) // lwe_per_glwe
    out = filled((n_glwe, k + 1, n, 2))
    K.keyswitch_lwe_ciphertext_list_and_pack_in_glwe_ciphertext(key, dev(lwe), out, lwe_per_glwe)
    return host(out)


@pytest.mark.parametrize("in_dim", [5, 37])
@pytest.mark.parametrize("base_log,level", SHAPES)
def test_tile_edges(engine, base_log, level, in_dim):
    """k = 2, N = 8: 24 columns (not a multiple of 16); depths in_dim level and digit bytes that are multiples of
    neither 64 nor 16; row counts around the 16-row tile; GLWEs of 1, 3 and 8 ciphertexts, ragged last ones."""
    K = engine.noise_squashing_compression
    k, n = 2, 8
    g = R.rng(1000 * base_log + 10 * level + in_dim)
    pksk = uniform_words(g, (in_dim, level, k + 1, n))
    lwe = uniform_words(g, (37, in_dim + 1))
    ties = Q.tie_words128(base_log, level)
    lwe[0, :min(in_dim, len(ties))] = R.to_words(ties[:in_dim])
    key = K.LwePackingKeyswitchKey128(dev(pksk), base_log, level)
    rows = Q.single_keyswitch_rows128(pksk, lwe, k, n, base_log, level)
    for n_lwe in (1, 15, 16, 17, 37):
        for per in (1, 3, 8):
            got = run_pack(engine, key, lwe[:n_lwe], k, n, per)
            assert np.array_equal(got, Q.pack_rows128(rows[:n_lwe], k, n, per)), (n_lwe, per)
    single = filled((37, k + 1, n, 2))
    K.keyswitch_lwe_ciphertext_into_glwe_ciphertext(key, dev(lwe), single)
    assert np.array_equal(host(single).reshape(37, -1, 2), rows)


@pytest.mark.parametrize("base_log,level", SHAPES)
def test_corner_words(engine, base_log, level):
    """Every mask word from corner_words and tie_words128; the bodies 0, 2^127 and 2^128 - 1."""
    K = engine.noise_squashing_compression
    in_dim, k, n, per = 37, 2, 8, 3
    corpus = R.corner_words(base_log, level) + Q.tie_words128(base_log, level)
    n_lwe = max(3, -(-len(corpus) // in_dim))
    g = R.rng(77 + base_log)
    pksk = uniform_words(g, (in_dim, level, k + 1, n))
    masks = [corpus[i % len(corpus)] for i in range(n_lwe * in_dim)]
    bodies = [[0, 1 << 127, R.MASK128][i % 3] for i in range(n_lwe)]
    lwe = R.to_words([masks[i * in_dim:(i + 1) * in_dim] + [bodies[i]] for i in range(n_lwe)])
    key = K.LwePackingKeyswitchKey128(dev(pksk), base_log, level)
    got = run_pack(engine, key, lwe, k, n, per)
    assert np.array_equal(got, Q.packing_keyswitch128_ref(pksk, lwe, k, n, base_log, level, per))
    # the reference itself against the transcription on the first GLWE
    want = Q.packing_keyswitch128_transcription(R.from_words(pksk.reshape(in_dim, level, -1, 2)),
                                                R.from_words(lwe[:per]), k, n, base_log, level)
    assert R.from_words(got[0].reshape(-1, 2)) == want


def test_accumulator_range(engine):
    """Base 2^7, one level, in_dim 131071 (the largest depth the rule in_dim level nd < 2^17 admits), one ciphertext
    whose every mask word 2^127 decomposes to +2^6 (at one level the pre-rounded decomposer cannot give -2^6: the
    state 2^6 is never balanced), against the two key words whose 16 signed bytes are all -128 and all +127: every
    int32 accumulator ends at 131071 * 64 * -128 = -(2^30 - 2^13) or 131071 * 64 * 127.  Reference: big integers."""
    K = engine.noise_squashing_compression
    in_dim, k, n, base_log, level = 131071, 1, 8, 7, 1
    assert Q.digits128(1 << 127, base_log, level) == [64]
    words = [Q.from_signed_bytes([-128] * 16), Q.from_signed_bytes([127] * 16)]
    assert [Q.signed_bytes(w, 16) for w in words] == [[-128] * 16, [127] * 16]
    cols = [words[c % 2] for c in range((k + 1) * n)]
    pksk = np.broadcast_to(R.to_words(cols), (in_dim, level, (k + 1) * n, 2)).reshape(in_dim, level, k + 1, n, 2)
    body = 0x0123456789abcdef0fedcba987654321
    lwe = R.to_words([[1 << 127] * in_dim + [body]])
    key = K.LwePackingKeyswitchKey128(dev(pksk), base_log, level)
    got = run_pack(engine, key, lwe, k, n, 1)
    want = [((body if c == k * n else 0) - in_dim * 64 * cols[c]) & R.MASK128 for c in range((k + 1) * n)]
    assert R.from_words(got[0].reshape(-1, 2)) == want
    with pytest.raises(engine.MiError):  # one more coefficient breaks the depth rule
        K.LwePackingKeyswitchKey128(zeros((131072, 1, 2, 8, 2)), 7, 1)


def test_production_depth_and_width(engine):
    """V1_4_NOISE_SQUASHING_COMP_PARAM_MESSAGE_2_CARRY_2: in_dim 4096, k = 6, N = 1024, base 2^61, one level; three
    ciphertexts into one GLWE of 128 slots.  64 sampled columns per polynomial (the wrapping ones among them) against
    big-integer sums over the source columns j - d, the whole GLWE against the vectorised reference."""
    K = engine.noise_squashing_compression
    in_dim, k, n, base_log, level, n_lwe, per = 4096, 6, 1024, 61, 1, 3, 128
    g = R.rng(0x4096)
    pksk = uniform_words(g, (in_dim, level, k + 1, n))
    lwe = uniform_words(g, (n_lwe, in_dim + 1))
    lwe[0, :6] = R.to_words(Q.tie_words128(base_log, level))
    key = K.LwePackingKeyswitchKey128(dev(pksk), base_log, level)
    got = run_pack(engine, key, lwe, k, n, per)
    assert got.shape == (1, k + 1, n, 2)
    cts = R.from_words(lwe)
    digits = [np.array([Q.digits128(a, base_log, level)[0] for a in ct[:-1]], dtype=object) for ct in cts]
    flat = pksk.reshape(in_dim, (k + 1) * n, 2)

    def t_word(d, c):  # word c of ciphertext d's keyswitched row
        col = flat[:, c, 0].astype(object) | (flat[:, c, 1].astype(object) << 64)
        return ((cts[d][-1] if c == k * n else 0) - int(np.dot(digits[d], col))) & R.MASK128

    sample = [0, 1, 2, 3, n - 1, n - 2] + [int(j) for j in g.integers(4, n - 2, size=58)]
    out = R.from_words(got[0])
    for p in range(k + 1):
        for j in sample:
            want = sum((-1 if j < d else 1) * t_word(d, p * n + (j - d) % n) for d in range(n_lwe)) & R.MASK128
            assert out[p][j] == want, (p, j)
    assert np.array_equal(got, Q.packing_keyswitch128_ref(pksk, lwe, k, n, base_log, level, per))


@pytest.mark.parametrize("per,n_lwe,piecewise", [
    (512, 2 * 512 + 512 + 37, False),  # a GLWE's rows are 32 MiB: two GLWEs per 64 MiB chunk, the second chunk ragged
    (2048, 2048 + 37, True),           # a GLWE's rows are 128 MiB: two pieces summed into the output, then a ragged GLWE
])
def test_chunked_and_piecewise_scratch(engine, per, n_lwe, piecewise):
    """N = 2048, k = 1: one keyswitched row is 64 KiB, so the 64 MiB cap on the rows of one GEMM launch cuts these
    calls (pks_plan_rows at 16-byte words); the sign wrap at every degree below 2048."""
    K = engine.noise_squashing_compression
    in_dim, k, n, base_log, level = 3, 1, 2048, 7, 2
    row_bytes = (k + 1) * n * 16
    assert (per * row_bytes > 64 << 20) == piecewise and n_lwe * row_bytes > 64 << 20
    g = R.rng(per)
    pksk = uniform_words(g, (in_dim, level, k + 1, n))
    lwe = uniform_words(g, (n_lwe, in_dim + 1))
    key = K.LwePackingKeyswitchKey128(dev(pksk), base_log, level)
    got = run_pack(engine, key, lwe, k, n, per)
    assert np.array_equal(got, Q.packing_keyswitch128_ref(pksk, lwe, k, n, base_log, level, per))


@pytest.mark.parametrize("log_modulus", [1, 12, 63, 64, 65, 127, 128])
def test_compress_extract_match_restatement(engine, log_modulus):
    C = engine.noise_squashing_compression.CompressedModulusSwitchedGlweCiphertext128
    k, n, batch = 2, 32, 3
    g = R.rng(0xc0 + log_modulus)
    glwe = uniform_words(g, (batch, k + 1, n))
    glwe[0, 0, :6] = R.to_words([0, R.MASK128, 1 << 127, (1 << 127) - 1, 1 << (127 - min(log_modulus, 127)),
                                 R.MASK128 - 1])
    ints = [R.from_words(glwe[b].reshape(-1, 2)) for b in range(batch)]
    for bodies in (0, 1, n):
        ct = C.compress(dev(glwe), log_modulus, bodies)
        want = [Q.compress128_ref(ints[b], k, n, bodies, log_modulus) for b in range(batch)]
        packed = host(ct.packed_integers)
        assert packed.shape == (batch, C.packed_words(k, n, bodies, log_modulus), 2) == (batch, len(want[0]), 2)
        assert np.array_equal(packed, R.to_words(want))
        out = filled((batch, k + 1, n, 2))  # the tail of the body polynomial must be zeroed
        ct.extract(out)
        want_glwe = [Q.extract128_ref(want[b], k, n, bodies, log_modulus) for b in range(batch)]
        assert np.array_equal(host(out).reshape(batch, -1, 2), R.to_words(want_glwe))
        assert not host(out)[:, k, bodies:].any()
        if log_modulus == 128:  # the production value: the identity on the kept words
            assert np.array_equal(packed, glwe.reshape(batch, -1, 2)[:, :k * n + bodies])
            assert np.array_equal(host(out).reshape(batch, -1, 2)[:, :k * n + bodies],
                                  glwe.reshape(batch, -1, 2)[:, :k * n + bodies])


def test_functional_round_trip(engine):
    """128 messages encrypted as u128 LWEs under a binary key, packed with a pksk128_gen key (TUniform 2^3 noise,
    the production base 2^61 and one level, N reduced to 128), compressed at log_modulus 128, extracted, and the GLWE
    decrypted on the host: coefficient d decodes to message d.  The allowed error is computed from the shape: the
    rounding of the mask, in_dim 2^(127 - base_log level), plus the key noise under the digits,
    in_dim level 2^(base_log - 1) 2^3."""
    K = engine.noise_squashing_compression
    in_dim, k, n, base_log, level, per = 64, 1, 128, 61, 1, 128
    msg_mod, delta = 16, 1 << 123
    bound = in_dim * (1 << (127 - base_log * level)) + in_dim * level * (1 << (base_log - 1)) * (1 << 3)
    assert 2 * bound < delta
    g = R.rng(0x5a5a)
    in_sk = R.binary_key(g, in_dim)
    glwe_sk = [R.binary_key(g, n) for _ in range(k)]
    pksk = R.to_words(Q.pksk128_gen(g, in_sk, glwe_sk, base_log, level, noise_log2=3))
    msgs = [int(m) for m in g.integers(0, msg_mod, size=per)]
    lwe = R.to_words([Q.lwe_encrypt_u128(g, m * delta, in_sk) for m in msgs])
    key = K.LwePackingKeyswitchKey128(dev(pksk), base_log, level)
    lists = K.compress_noise_squashed_ciphertexts_into_list(key, dev(lwe), per)
    assert len(lists) == 1 and lists[0].bodies_count == per and lists[0].log_modulus == 128
    glwe = host(lists[0].extract())
    assert glwe.shape == (1, k + 1, n, 2)
    assert np.array_equal(glwe, Q.packing_keyswitch128_ref(pksk, lwe, k, n, base_log, level, per))
    dec = R.glwe_decrypt(R.from_words(glwe[0]), glwe_sk)
    errors = []
    for d, m in enumerate(msgs):
        e = (dec[d] - m * delta) & R.MASK128
        errors.append(min(e, (1 << 128) - e))
    print("largest error 2^%.2f, bound 2^%.2f" % (np.log2(float(max(errors)) + 1), np.log2(float(bound))))
    assert max(errors) <= bound
    assert [R.decode(v, delta, msg_mod) % msg_mod for v in dec[:per]] == msgs


def test_list_with_a_remainder_chunk(engine):
    """compress_noise_squashed_ciphertexts_into_list: 11 ciphertexts, 4 per GLWE: two full GLWEs of 4 bodies and one
    of 3, each compressed with its own body count."""
    K = engine.noise_squashing_compression
    in_dim, k, n, base_log, level, per, n_lwe = 9, 1, 8, 24, 3, 4, 11
    g = R.rng(11)
    pksk = uniform_words(g, (in_dim, level, k + 1, n))
    lwe = uniform_words(g, (n_lwe, in_dim + 1))
    key = K.LwePackingKeyswitchKey128(dev(pksk), base_log, level)
    full, rest = K.compress_noise_squashed_ciphertexts_into_list(key, dev(lwe), per)
    want = Q.packing_keyswitch128_ref(pksk, lwe, k, n, base_log, level, per)
    assert (full.bodies_count, rest.bodies_count) == (4, 3)
    assert np.array_equal(host(full.packed_integers), want[:2].reshape(2, -1, 2)[:, :k * n + 4])
    assert np.array_equal(host(rest.packed_integers), want[2:].reshape(1, -1, 2)[:, :k * n + 3])
    assert K.compress_noise_squashed_ciphertexts_into_list(key, zeros((0, in_dim + 1, 2)), per) == []


def test_argument_checks(engine):
    import torch
    K = engine.noise_squashing_compression
    L = engine._lib.lib()
    bad, unsupported, ok = engine._lib.MI_ERR_INVALID_ARG, engine._lib.MI_ERR_UNSUPPORTED, engine._lib.MI_OK
    key = K.LwePackingKeyswitchKey128(zeros((8, 3, 2, 16, 2)), 4, 3)
    pack = K.keyswitch_lwe_ciphertext_list_and_pack_in_glwe_ciphertext
    with pytest.raises(ValueError):  # lwe_per_glwe > N
        pack(key, zeros((40, 9, 2)), zeros((2, 2, 16, 2)), 20)
    with pytest.raises(ValueError):  # a whole list longer than N into one GLWE
        pack(key, zeros((17, 9, 2)), zeros((2, 16, 2)))
    with pytest.raises(ValueError):  # input LweDimension
        pack(key, zeros((4, 8, 2)), zeros((1, 2, 16, 2)), 4)
    with pytest.raises(ValueError):  # output PolynomialSize
        pack(key, zeros((4, 9, 2)), zeros((1, 2, 8, 2)), 4)
    with pytest.raises(ValueError):  # output GlweDimension
        pack(key, zeros((4, 9, 2)), zeros((1, 3, 16, 2)), 4)
    with pytest.raises(ValueError):  # GLWE count
        pack(key, zeros((9, 9, 2)), zeros((2, 2, 16, 2)), 4)
    with pytest.raises(ValueError):  # u64 words, not (lo, hi) pairs
        pack(key, zeros((4, 9)), zeros((1, 2, 16, 2)), 4)
    with pytest.raises(ValueError):
        K.keyswitch_lwe_ciphertext_into_glwe_ciphertext(key, zeros((3, 9, 2)), zeros((2, 2, 16, 2)))
    with pytest.raises(ValueError):
        K.LwePackingKeyswitchKey128(zeros((8, 2, 2, 16, 2)), 4, 3)
    # the empty batch is a no-op; an empty list zeroes its GLWE, as the reference does
    pack(key, zeros((0, 9, 2)), zeros((0, 2, 16, 2)), 4)
    one = filled((2, 16, 2))
    pack(key, zeros((0, 9, 2)), one)
    assert not host(one).any()
    # the C ABI itself: codes, never aborts, nothing written
    lwe, out = zeros((4, 9, 2)), filled((1, 2, 16, 2))
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    pk = L.mi_lwe_packing_keyswitch128_batch
    assert pk(None, p(out), p(lwe), 4, 4, None) == bad
    assert pk(key._h, None, p(lwe), 4, 4, None) == bad
    assert pk(key._h, p(out), None, 4, 4, None) == bad
    assert pk(key._h, p(out), p(lwe), 4, 17, None) == bad
    assert pk(key._h, p(out), p(lwe), 4, 0, None) == bad
    assert pk(key._h, None, None, 0, 4, None) == ok
    torch.cuda.synchronize()
    assert (host(out) == np.uint64(R.MASK64)).all()
    words = zeros((8, 2))
    create = lambda *a: L.mi_lwe_pksk128_create(*a)
    message = lambda: L.mi_last_error_message().decode()
    # (in_dim, glwe_dim, N, base_log, level) -> status, message
    for args, status, text in [((0, 1, 16, 4, 3), bad, "lwe dimension out of range"),
                               ((8, 1, 12, 4, 3), bad, "polynomial size must be a power of two"),
                               ((8, 1, 0, 4, 3), bad, "polynomial size must be a power of two"),
                               ((8, 0, 16, 4, 3), bad, "glwe size out of range"),
                               ((8, 1, 16, 16, 8), bad, "decomposition base_log * level must be in [1, 127]"),
                               ((8, 1, 16, 0, 3), bad, "decomposition base_log * level must be in [1, 127]"),
                               ((8, 1, 16, 4, 0), bad, "decomposition base_log * level must be in [1, 127]"),
                               ((8, 1, 16, 64, 1), unsupported,
                                "base_log above 63 is not supported (a digit must fit 64 bits)"),
                               ((131072, 1, 2, 7, 1), unsupported,
                                "in_dim * level * ceil((base_log + 1) / 8) must stay below 2^17"),
                               ((16384, 1, 2, 61, 1), unsupported,
                                "in_dim * level * ceil((base_log + 1) / 8) must stay below 2^17")]:
        h = ctypes.c_void_p()
        assert (create(p(words), *args, 0, None, ctypes.byref(h)), message()) == (status, text), args
        assert not h.value
    h = ctypes.c_void_p()
    assert create(None, 8, 1, 16, 4, 3, 0, None, ctypes.byref(h)) == bad and not h.value and message() == "pksk is NULL"
    assert create(p(words), 8, 1, 16, 4, 3, 0, None, None) == bad and message() == "out_key is NULL"
    assert L.mi_lwe_pksk128_info(None, None, None, None, None, None) == bad and message() == "key is NULL"
    assert L.mi_lwe_pksk128_destroy(None) == ok
    dims = (ctypes.c_size_t(), ctypes.c_int(), ctypes.c_size_t(), ctypes.c_int(), ctypes.c_int())
    assert L.mi_lwe_pksk128_info(key._h, *[ctypes.byref(d) for d in dims]) == ok
    assert [d.value for d in dims] == [8, 1, 16, 4, 3]
    # base_log * level = 126 <= 127 is accepted at u128 (it is not at u64)
    K.LwePackingKeyswitchKey128(zeros((2, 2, 2, 16, 2)), 63, 2)
    # compression
    C = K.CompressedModulusSwitchedGlweCiphertext128
    glwe = filled((2, 2, 16, 2))
    for log_modulus, bodies in ((0, 4), (129, 4), (12, 17)):
        with pytest.raises(ValueError):
            C.compress(glwe, log_modulus, bodies)
        w = ctypes.c_size_t(123)
        assert L.mi_glwe_compressed_words128(16, 1, bodies, log_modulus, ctypes.byref(w)) == bad and w.value == 123
        assert L.mi_glwe_compress128_batch(p(glwe), p(glwe), 16, 1, bodies, log_modulus, 2, 0, None) == bad
        assert L.mi_glwe_extract128_batch(p(glwe), p(glwe), 16, 1, bodies, log_modulus, 2, 0, None) == bad
    assert L.mi_glwe_compressed_words128(16, 1, 4, 12, None) == bad
    assert L.mi_glwe_compress128_batch(None, p(glwe), 16, 1, 4, 12, 2, 0, None) == bad
    assert L.mi_glwe_extract128_batch(p(glwe), None, 16, 1, 4, 12, 2, 0, None) == bad
    assert L.mi_glwe_compress128_batch(None, None, 16, 1, 4, 12, 0, 0, None) == ok
    torch.cuda.synchronize()
    assert (host(glwe) == np.uint64(R.MASK64)).all()
    with pytest.raises(ValueError):  # packed length
        C(zeros((2, 3, 2)), 1, 16, 4, 12).extract()
    assert C.compress(zeros((0, 2, 16, 2)), 12, 4).extract().shape == (0, 2, 16, 2)
