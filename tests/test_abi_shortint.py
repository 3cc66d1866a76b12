"""The C ABI of the shortint / radix layer answers bad arguments with a status and a message, never a crash: NULL
handles and the checks that come before any device call (no GPU), and the rejection rules of mi_shortint_key_create read
off real handles (`-m gpu`)."""
import ctypes

import numpy as np
import pytest

import tfhe_helpers as H

INVALID, UNSUPPORTED = 1, 6


def L():
    from tfhe_ntt_amd import _lib
    return _lib.lib()


def answered(st, status, text):
    msg = L().mi_last_error_message().decode()
    assert st == status and text in msg, (st, msg)


def other_error():
    """So that the message read next is the following call's own."""
    assert L().mi_lwe_ksk_create(None, 8, 10, 4, 4, 0, None, None) == INVALID
    assert L().mi_last_error_message() == b"out_key is NULL"


def test_header_declares_the_layer(engine):
    from tfhe_ntt_amd import _lib
    syms = set(_lib.declared_symbols())
    want = {"mi_lwe_linear_combination_batch", "mi_shortint_key_check", "mi_shortint_key_create",
            "mi_shortint_key_destroy", "mi_shortint_key_info", "mi_shortint_lut_fill", "mi_shortint_apply_lut_batch",
            "mi_radix_propagate_single_carry_batch", "mi_radix_full_propagate_batch", "mi_radix_add_batch"}
    assert want <= syms and all(s in _lib._SIGS for s in want)


def test_null_handles(engine):
    words = (ctypes.c_uint64 * 8)()
    p = ctypes.addressof(words)
    h = ctypes.c_void_p()
    calls = [
        (lambda: L().mi_shortint_key_create(None, 0, p, None, 0, 4, 4, ctypes.byref(h)), "key is NULL"),
        (lambda: L().mi_shortint_key_create(p, 0, None, None, 0, 4, 4, ctypes.byref(h)), "key is NULL"),
        (lambda: L().mi_shortint_key_create(p, 0, p, None, 0, 4, 4, None), "out_key is NULL"),
        (lambda: L().mi_shortint_key_info(None, None, None, None, None, None, None, None), "key is NULL"),
        (lambda: L().mi_shortint_apply_lut_batch(None, p, p, 1, None, p, None, 1, 1, None), "key is NULL"),
        (lambda: L().mi_radix_propagate_single_carry_batch(None, p, None, 2, 1, None), "key is NULL"),
        (lambda: L().mi_radix_full_propagate_batch(None, p, 2, 1, None), "key is NULL"),
        (lambda: L().mi_radix_add_batch(None, p, p, p, None, 2, 1, None), "key is NULL"),
        (lambda: L().mi_shortint_lut_fill(None, 2048, 1, 4, 4, words, 16), "buffer is NULL"),
        (lambda: L().mi_shortint_lut_fill(words, 2048, 1, 4, 4, None, 16), "buffer is NULL"),
    ]
    for call, text in calls:
        other_error()
        answered(call(), INVALID, text)
        assert not h.value
    assert L().mi_shortint_key_destroy(None) == 0


def test_linear_combination_argument_rules(engine):
    words = (ctypes.c_uint64 * 64)()
    idx = (ctypes.c_uint32 * 8)()
    p, ip = ctypes.addressof(words), ctypes.addressof(idx)
    lc = L().mi_lwe_linear_combination_batch
    for dim in (0, 1 << 24):
        other_error()
        answered(lc(p, p + 256, dim, 1, 1, 1, ip, None, None, 0, None), INVALID, "lwe dimension out of range")
    other_error()
    answered(lc(p, p + 256, 3, 1 << 31, 1, 1, ip, None, None, 0, None), INVALID, "batch too large")
    other_error()
    answered(lc(p, p + 256, 3, 1, 1, 1 << 16, ip, None, None, 0, None), INVALID, "terms out of range")
    assert lc(None, None, 3, 0, 0, 2, None, None, None, 0, None) == 0  # an empty batch reads nothing
    other_error()
    answered(lc(None, p, 3, 1, 1, 1, ip, None, None, 0, None), INVALID, "buffer is NULL")
    other_error()
    answered(lc(p, None, 3, 1, 1, 1, ip, None, None, 0, None), INVALID, "buffer is NULL")
    other_error()
    answered(lc(p, p + 256, 3, 1, 1, 1, None, None, None, 0, None), INVALID, "index is NULL")
    # rows of 4 words: out = words [0, 8), in = words [4, 12) share a row; [8, 16) does not (checked before the launch)
    other_error()
    answered(lc(p, p + 32, 3, 2, 2, 1, ip, None, None, 0, None), INVALID, "lwe_out overlaps lwe_in")
    other_error()
    answered(lc(p, p, 3, 2, 2, 1, ip, None, None, 0, None), INVALID, "lwe_out overlaps lwe_in")


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()


@pytest.mark.gpu
def test_key_create_rejections_on_real_handles(engine):
    """Every rule of mi_shortint_key_create on handles of a small shape (N = 1024, k = 1, n = 8), then the rules of the
    calls that take the key."""
    import torch
    M, X, KS, N = engine.ntt64_pbs, engine.fft64, engine.lwe_keyswitch, engine.modulus_switch_noise_reduction
    S = engine.shortint
    n, k, small = 1024, 1, 8
    g = H.rng(0xab1)
    plan = engine.Plan.try_new(n, engine.SOLINAS_P)
    bsk = dev(H.uniform_u64(g, (small, 1, 2, 2, n)) % np.uint64(engine.SOLINAS_P))
    bnf, sol = M.NttBootstrapKey(plan, bsk, 23, 1, M.BNF), M.NttBootstrapKey(plan, bsk, 23, 1, M.SOLINAS)
    fbsk = torch.zeros((small, 1, 2, 2, n // 2, 2), dtype=torch.float64, device="cuda")
    fkey = X.FourierLweBootstrapKey(fbsk, 23, 1)
    mbsk = torch.zeros((small // 2, 4, 1, 2, 2, 2048 // 2, 2), dtype=torch.float64, device="cuda")
    mkey = X.FourierLweMultiBitBootstrapKey(mbsk, 23, 1, 2)
    ksk = KS.LweKeyswitchKey(dev(H.uniform_u64(g, (k * n, 3, small + 1))), 4, 3)
    ksk_out = KS.LweKeyswitchKey(dev(H.uniform_u64(g, (k * n, 3, small + 2))), 4, 3)
    ksk_in = KS.LweKeyswitchKey(dev(H.uniform_u64(g, (k * n - 1, 3, small + 1))), 4, 3)
    ksk_2048 = KS.LweKeyswitchKey(dev(H.uniform_u64(g, (2048, 3, small + 1))), 4, 3)
    msk = N.ModulusSwitchNoiseReductionKey(dev(H.uniform_u64(g, (4, small + 1))), 0.1, 1.0, 1e-30)
    msk_dim = N.ModulusSwitchNoiseReductionKey(dev(H.uniform_u64(g, (4, small + 2))), 0.1, 1.0, 1e-30)

    def rejected(status, text, *args, **kw):
        with pytest.raises(engine.MiError) as e:
            S.ShortintServerKey(*args, **kw)
        assert e.value.status == status and text in str(e.value), str(e.value)

    rejected(UNSUPPORTED, "Solinas-variant", ksk, sol, 4, 4)
    rejected(INVALID, "output dimension", ksk_out, bnf, 4, 4)
    rejected(INVALID, "input dimension", ksk_in, bnf, 4, 4)
    rejected(INVALID, "input dimension", ksk_2048, fkey, 4, 4)
    rejected(INVALID, "powers of two", ksk, bnf, 3, 4)
    rejected(INVALID, "powers of two", ksk, fkey, 4, 6)
    rejected(INVALID, "at most N / 2", ksk, bnf, 32, 32)
    rejected(INVALID, "ms_mode", ksk, bnf, 4, 4, ms_mode=2)
    rejected(INVALID, "multi-bit", ksk_2048, mkey, 4, 4, msk)
    rejected(INVALID, "multi-bit", ksk_2048, mkey, 4, 4, ms_mode=1)
    rejected(INVALID, "drift", ksk, bnf, 4, 4, msk, ms_mode=1)
    rejected(INVALID, "ms-noise key's dimension", ksk, bnf, 4, 4, msk_dim)
    with pytest.raises(TypeError):
        S.ShortintServerKey(ksk, object(), 4, 4)

    key = S.ShortintServerKey(ksk, bnf, 4, 4, msk)
    eng, mode, has, m, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_uint64(), ctypes.c_uint64()
    big, sm = ctypes.c_size_t(), ctypes.c_size_t()
    assert L().mi_shortint_key_info(key._h, *map(ctypes.byref, (eng, mode, has, m, c, big, sm))) == 0
    assert (eng.value, mode.value, has.value, m.value, c.value, big.value, sm.value) == (0, 0, 1, 4, 4, n, small)

    size = k * n + 1
    buf = torch.zeros((6, size), dtype=torch.int64, device="cuda")
    lut = torch.zeros((2, 2, n), dtype=torch.int64, device="cuda")
    p, lp = buf.data_ptr(), lut.data_ptr()
    ap = L().mi_shortint_apply_lut_batch
    answered(ap(key._h, p, p + 8 * size * 3, 2, None, lp, None, 2, 3, None), INVALID, "n_items must equal n_in")
    answered(ap(key._h, p, p + 8 * size * 3, 3, None, lp, None, 2, 3, None), INVALID, "n_lut must be at least n_items")
    answered(ap(key._h, p, p + 8 * size, 2, None, lp, None, 2, 2, None), INVALID, "partially overlaps")
    answered(ap(key._h, None, p, 2, None, lp, None, 2, 2, None), INVALID, "buffer is NULL")
    answered(ap(key._h, p, p + 8 * size * 3, 1 << 22, None, lp, None, 2, 1 << 22, None), INVALID, "batch too large")
    assert ap(key._h, None, None, 0, None, None, None, 0, 0, None) == 0
    answered(L().mi_radix_add_batch(key._h, p, p, p, None, 0, 1, None), INVALID, "n_blocks is 0")
    answered(L().mi_radix_add_batch(key._h, p, p + 8 * size, p, None, 2, 1, None), INVALID, "partially overlaps")
    answered(L().mi_radix_full_propagate_batch(key._h, None, 2, 1, None), INVALID, "buffer is NULL")
    answered(L().mi_radix_propagate_single_carry_batch(key._h, p, None, 1 << 21, 2, None), INVALID, "batch too large")
    assert L().mi_radix_add_batch(key._h, None, None, None, None, 3, 0, None) == 0
    small_mod = S.ShortintServerKey(ksk, bnf, 2, 2)
    answered(L().mi_radix_propagate_single_carry_batch(small_mod._h, p, None, 2, 1, None), UNSUPPORTED, "single carry")
    answered(L().mi_radix_add_batch(small_mod._h, p, p, p, None, 2, 1, None), UNSUPPORTED, "single carry")
    eight_two = S.ShortintServerKey(ksk, bnf, 8, 2)
    answered(L().mi_radix_propagate_single_carry_batch(eight_two._h, p, None, 2, 1, None), UNSUPPORTED, "single carry")
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_carry_out_overlap_is_rejected(engine):
    """carry_out is written after radix / radix_out: one that overlaps the radix, the output or an operand (its first
    row, its last row, the same address, one word) is MI_ERR_INVALID_ARG before any device call (the buffers keep their
    words); a disjoint carry_out in the same tensor, on either side, is accepted and gives what a separate tensor gives."""
    import torch
    M, KS, S = engine.ntt64_pbs, engine.lwe_keyswitch, engine.shortint
    n, small, n_int, blocks = 1024, 8, 2, 3
    total, size = n_int * blocks, n + 1
    g = H.rng(0xab2)
    plan = engine.Plan.try_new(n, engine.SOLINAS_P)
    bnf = M.NttBootstrapKey(plan, dev(H.uniform_u64(g, (small, 1, 2, 2, n)) % np.uint64(engine.SOLINAS_P)), 23, 1, M.BNF)
    ksk = KS.LweKeyswitchKey(dev(H.uniform_u64(g, (n, 3, small + 1))), 4, 3)
    key = S.ShortintServerKey(ksk, bnf, 4, 4)
    row = 8 * size
    words = H.uniform_u64(g, (3, total + 2 * n_int, size))  # rows [2, 8) are the radix, [0, 2) and [8, 10) beside it
    prop, add = L().mi_radix_propagate_single_carry_batch, L().mi_radix_add_batch
    first = n_int * row

    def fresh():
        return [dev(w) for w in words]

    # carry_out at these byte offsets from the radix's start overlaps it
    bad = [-row, (total - 1) * row, 0, 2 * row, -first + 8, total * row - 8]
    for off in bad:
        a, b, c = fresh()
        before = [t.clone() for t in (a, b, c)]
        pa, pb, pc = (t.data_ptr() + first for t in (a, b, c))
        other_error()
        answered(prop(key._h, pa, pa + off, blocks, n_int, None), INVALID, "carry_out overlaps")
        for out, lhs, rhs, carry in [(pa, pb, pc, pa + off), (pa, pb, pc, pb + off), (pa, pb, pc, pc + off),
                                     (pa, pa, pb, pa + off), (pa, pb, pa, pb + off)]:
            other_error()
            answered(add(key._h, out, lhs, rhs, carry, blocks, n_int, None), INVALID, "carry_out overlaps")
        torch.cuda.synchronize()
        assert all(torch.equal(t, u) for t, u in zip((a, b, c), before)), off
    # B = 1: the radix is n_integers rows
    a = fresh()[0]
    other_error()
    answered(prop(key._h, a.data_ptr(), a.data_ptr() + row, 1, 3, None), INVALID, "carry_out overlaps")
    # accepted: right before and right after the radix, in the same tensor
    want_r, want_c = dev(words[0][n_int:n_int + total]), torch.zeros((n_int, size), dtype=torch.int64, device="cuda")
    assert prop(key._h, want_r.data_ptr(), want_c.data_ptr(), blocks, n_int, None) == 0
    sum_r, sum_c = torch.zeros_like(want_r), torch.zeros_like(want_c)
    lhs, rhs = dev(words[1][n_int:n_int + total]), dev(words[2][n_int:n_int + total])
    assert add(key._h, sum_r.data_ptr(), lhs.data_ptr(), rhs.data_ptr(), sum_c.data_ptr(), blocks, n_int, None) == 0
    for off, rows in [(-first, slice(0, n_int)), (total * row, slice(n_int + total, None))]:
        a = fresh()[0]
        pa = a.data_ptr() + first
        assert prop(key._h, pa, pa + off, blocks, n_int, None) == 0
        assert torch.equal(a[n_int:n_int + total], want_r) and torch.equal(a[rows], want_c), off
        assert add(key._h, pa, lhs.data_ptr(), rhs.data_ptr(), pa + off, blocks, n_int, None) == 0
        assert torch.equal(a[n_int:n_int + total], sum_r) and torch.equal(a[rows], sum_c), off
    assert prop(key._h, a.data_ptr() + first, None, blocks, n_int, None) == 0  # no carry_out: nothing to overlap
    torch.cuda.synchronize()
