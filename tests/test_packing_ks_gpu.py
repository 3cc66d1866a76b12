"""GPU parity of the LWE packing keyswitch and the GLWE compression against packing_helpers.py (`-m gpu`).

Bar: bit-exact vs the composed reference (restating lwe_packing_keyswitch.rs:102-187, 296-379) on seeded random keys
and ciphertexts whose first mask words sit on the rounding corners of the pre-rounded decomposition — the
COMP_PARAM_MESSAGE_2_CARRY_2 shape, every digit kernel, every padding path of the GEMM, ragged and partial GLWEs,
the sign wrap at N = 2048 and the chunked scratch; compress / extract against the big-integer restatement of
packed_integers.rs; the round trip with real keys; the argument checks.
"""
import ctypes

import numpy as np
import pytest

import packing_helpers as P
import tfhe_helpers as H

pytestmark = pytest.mark.gpu


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


def zeros(shape):
    import torch
    return torch.zeros(shape, dtype=torch.int64, device="cuda")


def inputs(in_dim, k, n, base_log, level, n_lwe):
    g = H.rng(in_dim * 7 + n * 3 + base_log + n_lwe)
    pksk = H.uniform_u64(g, (in_dim, level, k + 1, n))
    lwe = H.uniform_u64(g, (n_lwe, in_dim + 1))
    ties = P.tie_words(base_log, level)[:in_dim]
    lwe[0, :len(ties)] = ties
    return pksk, lwe


def run_pack(engine, pksk, lwe, base_log, level, lwe_per_glwe):
    K = engine.lwe_packing_keyswitch
    key = K.LwePackingKeyswitchKey(dev(pksk), base_log, level)
    n_glwe = (lwe.shape[0] + lwe_per_glwe - 1) // lwe_per_glwe
    out = zeros((n_glwe,) + pksk.shape[2:])
    out.fill_(-1)  # every word must be written
    K.keyswitch_lwe_ciphertext_list_and_pack_in_glwe_ciphertext(key, dev(lwe), out, lwe_per_glwe)
    return host(out)


@pytest.mark.parametrize("in_dim,k,n,base_log,level,lwe_per_glwe,n_lwe", [
    (2048, 4, 256, 4, 3, 256, 293),    # COMP_PARAM_MESSAGE_2_CARRY_2, ragged last GLWE, generic digit kernel
    (13, 1, 16, 7, 3, 16, 16),         # K < 64, one column group, full-degree rotation
    (20, 2, 8, 4, 3, 5, 13),           # 24 columns padded to 32, lwe_per_glwe < N, three GLWEs
    (33, 1, 32, 10, 2, 32, 40),        # two bytes per digit
    (6, 1, 32, 21, 3, 32, 32),         # three bytes per digit
    (10, 1, 16, 40, 1, 16, 20),        # a digit wider than 32 bits (six bytes)
    (50, 1, 64, 6, 2, 64, 320),        # level-2 digit kernel; GLWE boundaries inside 256-row groups
    (70, 1, 16, 5, 1, 16, 300),        # level 1
    (24, 3, 16, 3, 8, 16, 9),          # level 8; one partial GLWE
    (64, 1, 2048, 4, 2, 2048, 2148),   # sign wrap at N = 2048; two scratch chunks, the second ragged
])
def test_packing_keyswitch_matches_reference(engine, oracle, in_dim, k, n, base_log, level, lwe_per_glwe, n_lwe):
    pksk, lwe = inputs(in_dim, k, n, base_log, level, n_lwe)
    got = run_pack(engine, pksk, lwe, base_log, level, lwe_per_glwe)
    want = P.packing_keyswitch_ref(oracle, pksk, lwe, k, n, base_log, level, lwe_per_glwe)
    assert np.array_equal(got, want)


def test_packing_keyswitch_one_glwe_larger_than_the_scratch_cap(engine, oracle):
    """N = 4096, k = 1: 4096 keyswitched rows are 256 MiB, four times the 64 MiB scratch cap, so one GLWE is summed
    from four pieces of rows (the degree offset of a piece, accumulation into the output); a ragged second GLWE."""
    in_dim, k, n, base_log, level, n_lwe = 8, 1, 4096, 6, 1, 4096 + 37
    pksk, lwe = inputs(in_dim, k, n, base_log, level, n_lwe)
    got = run_pack(engine, pksk, lwe, base_log, level, n)
    assert np.array_equal(got, P.packing_keyswitch_ref(oracle, pksk, lwe, k, n, base_log, level, n))


def test_single_keyswitch_into_glwe(engine, oracle):
    """keyswitch_lwe_ciphertext_into_glwe_ciphertext over a batch: one GLWE per ciphertext, no rotation; and the
    reference's one-list-one-GLWE form of the list function."""
    in_dim, k, n, base_log, level, batch = 21, 2, 16, 5, 4, 7
    K = engine.lwe_packing_keyswitch
    pksk, lwe = inputs(in_dim, k, n, base_log, level, batch)
    key = K.LwePackingKeyswitchKey(dev(pksk), base_log, level)
    out = zeros((batch, k + 1, n))
    K.keyswitch_lwe_ciphertext_into_glwe_ciphertext(key, dev(lwe), out)
    want = P.single_keyswitch_rows(oracle, pksk, lwe, k, n, base_log, level)
    assert np.array_equal(host(out).reshape(batch, -1), want)
    one = zeros((k + 1, n))
    K.keyswitch_lwe_ciphertext_list_and_pack_in_glwe_ciphertext(key, dev(lwe), one)
    assert np.array_equal(host(one), P.packing_keyswitch_ref(oracle, pksk, lwe, k, n, base_log, level, batch)[0])


@pytest.mark.parametrize("log_modulus", [1, 5, 12, 13, 31, 63, 64])
def test_compress_extract_match_restatement(engine, oracle, log_modulus):
    C = engine.lwe_packing_keyswitch.CompressedModulusSwitchedGlweCiphertext
    k, n, batch = 2, 32, 3
    g = H.rng(0xc0 + log_modulus)
    glwe = H.uniform_u64(g, (batch, k + 1, n))
    glwe[0, 0, :6] = [0, P.M64, 1 << 63, (1 << 63) - 1, (1 << (63 - min(log_modulus, 63))), P.M64 - 1]
    for bodies in (1, n - 1, n):
        ct = C.compress(dev(glwe), log_modulus, bodies)
        packed = host(ct.packed_integers)
        want = np.stack([P.compress_ref(oracle, glwe[b], k, n, bodies, log_modulus) for b in range(batch)])
        assert packed.shape == want.shape == (batch, C.packed_words(k, n, bodies, log_modulus))
        assert np.array_equal(packed, want)
        out = zeros((batch, k + 1, n))
        out.fill_(-1)  # the tail of the body polynomial must be zeroed
        ct.extract(out)
        want_glwe = np.stack([P.extract_ref(want[b], k, n, bodies, log_modulus) for b in range(batch)])
        assert np.array_equal(host(out), want_glwe)
        assert not host(out)[:, k, bodies:].any()


def test_real_keys_round_trip(engine, oracle):
    """256 LWE encryptions -> packed, compressed at 12 bits, extracted and sample-extracted on the GPU -> decrypted
    on the host: the messages come back."""
    K, M = engine.lwe_packing_keyswitch, engine.ntt64_pbs
    in_dim, k, n, base_log, level, log_modulus = 48, 1, 256, 8, 3, 12
    msg_mod, delta = 8, 1 << 60
    g = H.rng(0x9ac)
    in_sk = H.binary_key(g, in_dim)
    glwe_sk = H.binary_key(g, (k, n))
    pksk = P.pksk_gen(g, in_sk, glwe_sk, base_log, level, noise_log2=10)
    msgs = g.integers(0, msg_mod, size=n, dtype=np.uint64)
    lwe = H.lwe_encrypt_batch(g, msgs * np.uint64(delta), in_sk, noise_log2=10)
    key = K.LwePackingKeyswitchKey(dev(pksk), base_log, level)
    glwe = zeros((1, k + 1, n))
    K.keyswitch_lwe_ciphertext_list_and_pack_in_glwe_ciphertext(key, dev(lwe), glwe, n)
    assert np.array_equal(host(glwe), P.packing_keyswitch_ref(oracle, pksk, lwe, k, n, base_log, level, n))
    ct = K.CompressedModulusSwitchedGlweCiphertext.compress(glwe, log_modulus, n)
    back = ct.extract()
    out = zeros((1, n, k * n + 1))
    M.extract_lwe_sample_from_glwe_ciphertext(back, out, nth=0, nth_stride=1, nth_count=n)
    dec = H.lwe_decrypt_batch(host(out)[0], H.glwe_sk_as_lwe_sk(glwe_sk))
    assert [H.decode(int(d), delta, msg_mod) for d in dec] == [int(m) for m in msgs]


def test_argument_checks(engine):
    import torch
    K = engine.lwe_packing_keyswitch
    L = engine._lib.lib()
    bad = engine._lib.MI_ERR_INVALID_ARG
    key = K.LwePackingKeyswitchKey(zeros((8, 3, 2, 16)), 4, 3)
    pack = K.keyswitch_lwe_ciphertext_list_and_pack_in_glwe_ciphertext
    with pytest.raises(ValueError):  # lwe_per_glwe > N
        pack(key, zeros((40, 9)), zeros((2, 2, 16)), 20)
    with pytest.raises(ValueError):  # a whole list longer than N into one GLWE
        pack(key, zeros((17, 9)), zeros((2, 16)))
    with pytest.raises(ValueError):  # input LweDimension
        pack(key, zeros((4, 8)), zeros((1, 2, 16)), 4)
    with pytest.raises(ValueError):  # output PolynomialSize
        pack(key, zeros((4, 9)), zeros((1, 2, 8)), 4)
    with pytest.raises(ValueError):  # output GlweDimension
        pack(key, zeros((4, 9)), zeros((1, 3, 16)), 4)
    with pytest.raises(ValueError):  # GLWE count
        pack(key, zeros((9, 9)), zeros((2, 2, 16)), 4)
    with pytest.raises(ValueError):
        K.keyswitch_lwe_ciphertext_into_glwe_ciphertext(key, zeros((3, 9)), zeros((2, 2, 16)))
    with pytest.raises(ValueError):
        K.LwePackingKeyswitchKey(zeros((8, 2, 2, 16)), 4, 3)
    with pytest.raises(engine.MiError):  # base_log * level >= 64 (SignedDecomposer::new asserts)
        K.LwePackingKeyswitchKey(zeros((8, 8, 2, 16)), 8, 8)
    with pytest.raises(engine.MiError):  # N not a power of two
        K.LwePackingKeyswitchKey(zeros((8, 3, 2, 12)), 4, 3)
    with pytest.raises(engine.MiError):  # GEMM depth 66000 * 2 >= 2^17
        K.LwePackingKeyswitchKey(zeros((66000, 2, 2, 2)), 4, 2)
    # the empty batch is a no-op; an empty list zeroes its GLWE, as the reference does
    pack(key, zeros((0, 9)), zeros((0, 2, 16)), 4)
    one = zeros((2, 16))
    one.fill_(-1)
    pack(key, zeros((0, 9)), one)
    assert not host(one).any()
    # the C ABI itself: codes, never aborts
    lwe, out = zeros((4, 9)), zeros((1, 2, 16))
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert L.mi_lwe_packing_keyswitch_batch(None, p(out), p(lwe), 4, 4, None) == bad
    assert L.mi_lwe_packing_keyswitch_batch(key._h, None, p(lwe), 4, 4, None) == bad
    assert L.mi_lwe_packing_keyswitch_batch(key._h, p(out), None, 4, 4, None) == bad
    assert L.mi_lwe_packing_keyswitch_batch(key._h, p(out), p(lwe), 4, 17, None) == bad
    assert L.mi_lwe_packing_keyswitch_batch(key._h, p(out), p(lwe), 4, 0, None) == bad
    assert L.mi_lwe_packing_keyswitch_batch(key._h, None, None, 0, 4, None) == engine._lib.MI_OK
    h = ctypes.c_void_p()
    assert L.mi_lwe_pksk_create(None, 8, 1, 16, 4, 3, 0, None, ctypes.byref(h)) == bad and not h.value
    assert L.mi_lwe_pksk_create(p(lwe), 8, 1, 16, 4, 3, 0, None, None) == bad
    assert L.mi_lwe_pksk_info(None, None, None, None, None, None) == bad
    assert L.mi_lwe_pksk_destroy(None) == engine._lib.MI_OK
    dims = (ctypes.c_size_t(), ctypes.c_int(), ctypes.c_size_t(), ctypes.c_int(), ctypes.c_int())
    assert L.mi_lwe_pksk_info(key._h, *[ctypes.byref(d) for d in dims]) == engine._lib.MI_OK
    assert [d.value for d in dims] == [8, 1, 16, 4, 3]
    torch.cuda.synchronize()
    # compression
    C = K.CompressedModulusSwitchedGlweCiphertext
    glwe = zeros((2, 2, 16))
    for log_modulus, bodies in ((0, 4), (65, 4), (12, 17)):
        with pytest.raises(ValueError):
            C.compress(glwe, log_modulus, bodies)
        w = ctypes.c_size_t()
        assert L.mi_glwe_compressed_words(16, 1, bodies, log_modulus, ctypes.byref(w)) == bad
        assert L.mi_glwe_compress_batch(p(glwe), p(glwe), 16, 1, bodies, log_modulus, 2, 0, None) == bad
        assert L.mi_glwe_extract_batch(p(glwe), p(glwe), 16, 1, bodies, log_modulus, 2, 0, None) == bad
    assert L.mi_glwe_compressed_words(16, 1, 4, 12, None) == bad
    assert L.mi_glwe_compress_batch(None, p(glwe), 16, 1, 4, 12, 2, 0, None) == bad
    assert L.mi_glwe_extract_batch(p(glwe), None, 16, 1, 4, 12, 2, 0, None) == bad
    assert L.mi_glwe_compress_batch(None, None, 16, 1, 4, 12, 0, 0, None) == engine._lib.MI_OK
    with pytest.raises(ValueError):  # packed length
        C(zeros((2, 3)), 1, 16, 4, 12).extract()
    assert C.compress(zeros((0, 2, 16)), 12, 4).extract().shape == (0, 2, 16)
