"""The WoP-PBS references on the CPU (no GPU): the private functional packing keyswitch restatement and its key list
decrypt as the reference's do, the whole f64 restatement decodes test_wop_add_one, and mi_lwe_pfpksk_list_create rejects
what the reference asserts on.  tests/test_wopbs_gpu.py holds the GPU to these."""
import ctypes

import numpy as np

import tfhe_helpers as H
import wopbs_helpers as W


def test_pfpks_restatement_decrypts_to_minus_m_times_key_polynomial(oracle):
    """in_dim 64, k = 1, N = 64, (base_log, level) = (15, 2): Enc(m) under key j decrypts to -m S_j (to m for the last
    key), within the rounding of the decomposition; and the oracle-composed form is the same bits."""
    in_dim, k, n, base_log, level, noise = 64, 1, 64, 15, 2, 4
    g = H.rng(0xF1)
    in_sk, glwe_sk = H.binary_key(g, in_dim), H.binary_key(g, (k, n))
    key = W.pfpksk_gen(g, in_sk, glwe_sk, base_log, level, noise)
    msgs = [1 << 60, 5 << 58, (1 << 64) - (3 << 59), 0]
    lwe = H.lwe_encrypt_batch(g, msgs, in_sk, noise)
    out = W.pfpks_ref(key, lwe, base_log, level)
    assert out.shape == (len(msgs), k + 1, k + 1, n)
    assert np.array_equal(out, W.pfpks_ref_oracle(oracle, key, lwe, base_log, level))
    # every one of the in_dim + 1 decomposed words is rounded to base_log * level bits: at most 2^(63 - 30) each, times
    # the key polynomial's bits, plus the key noise times the digits (< 2^(noise + base_log) each)
    bound = (in_dim + 1) * (1 << (63 - base_log * level)) + (in_dim + 1) * level * (1 << (noise + base_log)) * 2
    for b, m in enumerate(msgs):
        for j in range(k + 1):
            pt = H.glwe_decrypt(out[b, j], glwe_sk)
            want = np.zeros(n, np.uint64)
            if j < k:
                want[:] = [(-m * int(s)) % 2**64 for s in glwe_sk[j]]
            else:
                want[0] = m % 2**64
            with np.errstate(over="ignore"):
                err = np.abs((pt - want).view(np.int64))
            assert int(err.max()) <= bound, (b, j, int(err.max()), bound)


def test_pfpks_restatement_decomposes_the_body_and_adds_nothing():
    """The body word goes through the decomposer like a mask word (a key whose only non-zero block is the body's)
    and a zero key gives a zero output (nothing is added)."""
    in_dim, base_log, level, n = 3, 4, 3, 4
    key = np.zeros((1, in_dim + 1, level, 2, n), np.uint64)
    lwe = H.uniform_u64(H.rng(3), (2, in_dim + 1))
    assert not W.pfpks_ref(key, lwe, base_log, level).any()
    key[0, in_dim, :, 1, 0] = [1 << (64 - base_log * (level - li)) for li in range(level)]   # recomposes the body
    out = W.pfpks_ref(key, lwe, base_log, level)
    import decomp_corners as D
    for b in range(2):
        want = (-D.closest_representable(int(lwe[b, in_dim]), base_log, level)) % 2**64
        assert int(out[b, 0, 1, 0]) == want and not out[b, 0, 0].any()


def test_wop_restatement_decodes_add_one():
    """Shape A: n = 8, k = 1, N = 256, PBS (9, 4), KS (4, 7), pfks (15, 2), cbs (6, 4), 10 input bits; the LUT
    i -> (i + 1) mod 2^10 of the reference's test_wop_add_one.  All 8 seeded messages decode."""
    shape = W.SHAPE_A
    msgs = W.messages(8)
    lwe = W.encrypt_messages(shape, msgs)
    out, bits = W.wop_ref(shape, lwe, [W.add_one_lut(shape.N)])
    ks = W.keys(shape)
    got_bits = (H.lwe_decrypt_batch(bits, ks["small_sk"]) + np.uint64(1 << 62)) >> np.uint64(63)
    for b, m in enumerate(msgs):
        assert [int(v) for v in got_bits[b]] == [(m >> (9 - j)) & 1 for j in range(10)], (b, m)
    assert W.decode_output(out[:, 0], ks["big_sk"]) == [(m + 1) % 1024 for m in msgs]


def test_restatement_selects_every_leaf_by_encrypted_bits():
    """Shape A, r = 4: for every m < 16, m's bits encrypted at delta_log 63, circuit-bootstrapped, then the CMUX tree
    over W.leaf_lut; all N coefficients of item m decode to leaf m at 4 bits (margin 2^59).  At r >= 3 the bit-reversed
    and the natural leaf order differ in more than a swap.  Measured: worst absolute error 2^42.7 here, 2^43.1 at
    SHAPE_N512 with r = 3 (about 9 s on the host, so only tests/test_wopbs_corners_gpu.py runs that shape)."""
    import fft_oracle as F

    shape, r = W.SHAPE_A, 4
    ks = W.keys(shape)
    fbsk = F.forward_as_torus(ks["bsk"])
    ggsw = W.circuit_bootstrap_ref(W.leaf_selector_lwes(shape, r), fbsk, *shape.pbs, shape.k, shape.N, ks["pfpksk"],
                                   *shape.pfks, 63, *shape.cbs)
    fggsw = F.forward_as_torus(ggsw).reshape((1 << r, r) + ggsw.shape[1:-1] + (shape.N // 2,))
    lut = W.leaf_lut(r, shape.N)
    assert len({tuple(row >> np.uint64(60)) for row in lut}) == 1 << r  # the leaves are distinct
    got, err = W.decode_leaves(W.cmux_tree_ref(lut, fggsw, *shape.cbs, shape.k), ks["glwe_sk"])
    print(f"\nleaf selection {shape.name} r={r}: numpy worst error 2^{np.log2(max(err, 1)):.1f}", end="")
    assert np.array_equal(got, lut >> np.uint64(60))


_DIM = "lwe dimension out of range"
_POW2, _GLWE = "polynomial size must be a power of two", "glwe size out of range"
_KEYS = "n_keys * (glwe_dim + 1) * polynomial_size must be in [1, 2^24)"
_DEPTH = "(in_dim + 1) * level * ceil((base_log + 1) / 8) must stay below 2^17"
_DECOMP = "decomposition base_log * level must be in [1, 63]"


def test_lwe_pfpksk_list_create_rejections(engine):
    from tfhe_ntt_amd import _lib

    L = _lib.lib()
    INVALID, UNSUPPORTED = _lib.MI_ERR_INVALID_ARG, _lib.MI_ERR_UNSUPPORTED
    words = (ctypes.c_uint64 * 4)()  # never dereferenced

    def create(args, key=ctypes.addressof(words)):
        h = ctypes.c_void_p()
        st = L.mi_lwe_pfpksk_list_create(key, *args, 0, None, ctypes.byref(h))
        assert not h.value, args
        return st, L.mi_last_error_message().decode()

    # (n_keys, in_dim, glwe_dim, N, base_log, level)
    assert L.mi_lwe_pfpksk_list_create(ctypes.addressof(words), 2, 8, 1, 16, 4, 3, 0, None, None) == INVALID
    assert L.mi_last_error_message() == b"out_key is NULL"
    assert create((2, 8, 1, 16, 4, 3), key=None) == (INVALID, "pfpksk_list is NULL")
    for args, status, message in [((2, 0, 1, 16, 4, 3), INVALID, _DIM),
                                  ((2, 1 << 24, 1, 16, 4, 3), INVALID, _DIM),
                                  ((2, 8, 1, 12, 4, 3), INVALID, _POW2),
                                  ((2, 8, 1, 0, 4, 3), INVALID, _POW2),
                                  ((2, 8, 0, 16, 4, 3), INVALID, _GLWE),
                                  ((2, 8, 1, 1 << 24, 4, 3), INVALID, _GLWE),
                                  ((0, 8, 1, 16, 4, 3), INVALID, _KEYS),
                                  ((1 << 20, 8, 1, 16, 4, 3), INVALID, _KEYS),
                                  ((2, 8, 1, 16, 8, 8), INVALID, _DECOMP),
                                  ((2, 8, 1, 16, 0, 3), INVALID, _DECOMP),
                                  ((2, 8, 1, 16, 4, 0), INVALID, _DECOMP),
                                  ((2, 8, 1, 16, 64, 1), INVALID, _DECOMP),
                                  ((2, 65535, 1, 2, 4, 2), UNSUPPORTED, _DEPTH),    # (in_dim + 1) * 2 = 2^17
                                  ((2, 32767, 1, 2, 9, 2), UNSUPPORTED, _DEPTH)]:   # two bytes per digit
        assert create(args) == (status, message), args
    # the first failing rule answers: dimension, then the GLWE shape, then the decomposition
    assert create((2, 0, 1, 12, 8, 8)) == (INVALID, _DIM)
    assert create((2, 8, 1, 12, 8, 8)) == (INVALID, _POW2)


def test_lwe_pfpksk_list_null_handles(engine):
    from tfhe_ntt_amd import _lib

    L = _lib.lib()

    def other_error():  # so that the message read next is the following call's own
        assert L.mi_lwe_ksk_create(None, 8, 10, 4, 4, 0, None, None) == _lib.MI_ERR_INVALID_ARG
        assert L.mi_last_error_message() == b"out_key is NULL"

    other_error()
    assert L.mi_lwe_pfpksk_list_info(None, None, None, None, None, None, None) == _lib.MI_ERR_INVALID_ARG
    assert L.mi_last_error_message() == b"key is NULL"
    assert L.mi_lwe_pfpksk_list_destroy(None) == _lib.MI_OK
    other_error()
    assert L.mi_lwe_pfpks_batch(None, None, None, 1, None) == _lib.MI_ERR_INVALID_ARG
    assert L.mi_last_error_message() == b"key is NULL"
    # the stages reject NULL keys and plans the same way, before any device work
    for call in (lambda: L.mi_fft64_extract_bits_batch(None, None, None, None, 54, 10, 1, None),
                 lambda: L.mi_fft64_circuit_bootstrap_boolean_batch(None, None, None, None, None, None, 1, 63, 6, 4, None),
                 lambda: L.mi_fft64_circuit_bootstrap_boolean_vertical_packing_batch(None, None, None, None, None, 10,
                                                                                    None, 4, 1, 6, 4, 1, None)):
        other_error()
        assert call() == _lib.MI_ERR_INVALID_ARG
        assert L.mi_last_error_message() == b"key is NULL"
    for call in (lambda: L.mi_fft64_cmux_tree_batch(None, None, None, 4, 1, None, 2, 0, 2, 1, 6, 4, 1, None),
                 lambda: L.mi_fft64_wop_blind_rotate_batch(None, None, 1, None, 2, 0, 2, 1, 6, 4, 1, None),
                 lambda: L.mi_fft64_vertical_packing_batch(None, None, None, 4, 1, None, 10, 1, 6, 4, 1, None),
                 lambda: L.mi_fft64_cmux_batch_indexed(None, None, None, None, None, 1, 1, 6, 4, 1, None)):
        other_error()
        assert call() == _lib.MI_ERR_INVALID_ARG
        assert L.mi_last_error_message() == b"plan is NULL"
