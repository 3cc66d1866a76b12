"""Every device copy of the signed decomposition on its rounding corners (`-m gpu`).

Uniform random inputs reach a rounding tie, a digit of exactly +-2^(B-1) or the carry through every level with
probability 2^-B or less per word; here the corpus of tests/decomp_corners.py (pinned by tests/test_decomposition_kat.py)
is placed in front of each decomposer, in every coefficient slot.  Integer paths are compared bit for bit with the
oracle and, where a probe isolates the digits, with the big-integer transcription; the f64 paths with the exact integer
product under the bound of test_fft_gpu.test_external_product_vs_exact.

Device decomposer                                                   reached by
  keyswitch.hip ks_digits_l_kernel<1|2|4|8> (core_scalar.hpp)        test_keyswitch_digit_probe (5,1) (6,2) (4,4) (3,8)
  keyswitch.hip ks_digits_kernel                                     test_keyswitch_digit_probe, every other shape
  ... pre_rounded (packing)                                          test_packing_keyswitch_digit_probe
  ... KS32                                                           test_ks32_digit_probe
  pbs_tw.hip generated bodies (gen_pbs_kernel.py decompose[_sol])    test_ntt_external_product_corners N = 2048 (23,1) (31,1),
                                                                     test_pbs_one_step_corners N = 2048 (23,1)
  core_scalar.hpp NttDigits                                          ... N = 2048 every other shape, N = 512 k = 4
    (pbs_kernels.hip, runtime level count)
  pbs_large.hip                                                      ... N = 8192
  fft64_decomp.hpp decompose_l1_hi (fft64_pbs.hip, level 1)          test_fft_external_product_corners N = 2048 (23,1) (31,1),
                                                                     test_fft_pbs_one_step_corners
  core_scalar.hpp (fft64_pbs.hip multi-level)                        test_fft_external_product_corners N = 2048 (12,2) (8,3)
  core_scalar.hpp (fft64_generic.hip)                                test_fft_external_product_corners N = 256
"""
import numpy as np
import pytest

import decomp_corners as D
import fft_oracle as F
import packing_helpers
import tfhe_helpers as H

pytestmark = pytest.mark.gpu

P = 0xFFFFFFFF00000001
M64 = 1 << 64
KS_ROWS = 17


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()


def dev32(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


def rand_q(g, shape, q):
    return g.integers(0, q, size=shape, dtype=np.uint64) if q else H.uniform_u64(g, shape)


# ---- keyswitch digit probes: KSK[i][l][c] = 1 iff c == i * level + l, so output column c is -digit(i, l) ----
def _probe_lwe(base_log, level):
    """KS_ROWS ciphertexts whose mask is the whole corpus, rolled by the row index; random bodies."""
    words = D.corner_words(base_log, level)
    m = len(words)
    lwe = np.array([[words[(i + r) % m] for i in range(m)] + [0] for r in range(KS_ROWS)], dtype=np.uint64)
    lwe[:, -1] = H.uniform_u64(H.rng(base_log * 100 + level), KS_ROWS)
    return lwe


def _probe_key(in_dim, level, out_size, dtype=np.uint64):
    ksk = np.zeros((in_dim, level, out_size), dtype)
    for i in range(in_dim):
        for l in range(level):
            ksk[i, l, i * level + l] = 1
    return ksk


def _minus_digits(lwe, base_log, level, decompose, mod):
    return np.array([[(-t) % mod for x in row[:-1] for t in decompose(int(x), base_log, level)] for row in lwe],
                    dtype=np.uint64)


@pytest.mark.parametrize("base_log,level", D.KS_SHAPES)
def test_keyswitch_digit_probe(engine, oracle, base_log, level):
    """(5,1) (6,2) (4,4) (3,8): ks_digits_l_kernel<1|2|4|8> (one byte per digit); every other shape: ks_digits_kernel,
    with 2 .. 8 bytes per digit; (32,1) .. (63,1): digits that do not fit 32 bits."""
    import torch
    K = engine.lwe_keyswitch
    lwe = _probe_lwe(base_log, level)
    in_dim = lwe.shape[1] - 1
    out_dim = in_dim * level
    ksk = _probe_key(in_dim, level, out_dim + 1)
    want = np.concatenate([_minus_digits(lwe, base_log, level, D.py_decompose, M64), lwe[:, -1:]], axis=1)
    assert np.array_equal(oracle.lwe_keyswitch(ksk, lwe, out_dim, base_log, level), want)
    out = torch.zeros((KS_ROWS, out_dim + 1), dtype=torch.int64, device="cuda")
    K.keyswitch_lwe_ciphertext(K.LweKeyswitchKey(dev(ksk), base_log, level), dev(lwe), out)
    assert np.array_equal(host(out), want)


@pytest.mark.parametrize("base_log,level", D.KS32_SHAPES)
def test_ks32_digit_probe(engine, oracle, base_log, level):
    """KS32 (u32 key, sums mod 2^32): (2,8) ks_digits_l_kernel<8>, (16,2) and (32,1) ks_digits_kernel."""
    K = engine.lwe_keyswitch
    lwe = _probe_lwe(base_log, level)
    in_dim = lwe.shape[1] - 1
    out_dim = in_dim * level
    ksk = _probe_key(in_dim, level, out_dim + 1, np.uint32)
    want = oracle.lwe_keyswitch32(ksk, lwe, out_dim, base_log, level, 32)
    digits = _minus_digits(lwe, base_log, level, D.py_decompose, 1 << 32).astype(np.uint32)
    assert np.array_equal(want[:, :-1], digits)
    out = dev32(np.zeros((KS_ROWS, out_dim + 1), np.uint32))
    K.keyswitch_lwe_ciphertext_with_scalar_change(K.LweKeyswitchKey32(dev32(ksk), base_log, level, 32), dev(lwe), out)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want)


@pytest.mark.parametrize("base_log,level", D.KS_SHAPES)
def test_packing_keyswitch_digit_probe(engine, oracle, base_log, level):
    """The pre_rounded digits (decompose(closest_representable(a_i))) of both digit kernels; the corpus holds
    packing_helpers.tie_words, on which they differ from the LWE keyswitch's."""
    import torch
    K = engine.lwe_packing_keyswitch
    lwe = _probe_lwe(base_log, level)
    in_dim = lwe.shape[1] - 1
    k, n = 1, 16
    while 2 * n < in_dim * level + 1:
        n *= 2
    pksk = _probe_key(in_dim, level, 2 * n).reshape(in_dim, level, k + 1, n)
    want = np.zeros((KS_ROWS, 2 * n), np.uint64)
    want[:, :in_dim * level] = _minus_digits(lwe, base_log, level, D.py_decompose_pre_rounded, M64)
    with np.errstate(over="ignore"):
        want[:, k * n] += lwe[:, -1]
    assert not np.array_equal(want[:, :in_dim * level], _minus_digits(lwe, base_log, level, D.py_decompose, M64))
    assert np.array_equal(packing_helpers.single_keyswitch_rows(oracle, pksk, lwe, k, n, base_log, level), want)
    out = torch.zeros((KS_ROWS, k + 1, n), dtype=torch.int64, device="cuda")
    K.keyswitch_lwe_ciphertext_into_glwe_ciphertext(K.LwePackingKeyswitchKey(dev(pksk), base_log, level), dev(lwe), out)
    assert np.array_equal(host(out).reshape(KS_ROWS, -1), want)


@pytest.mark.parametrize("key_word", [0x7F7F7F7F7F7F7F80, 0x7F7F7F7F7F7F7F7F])
def test_keyswitch_int32_accumulation_at_the_depth_cap(engine, oracle, key_word):
    """The exact-int32 claim of the int8 GEMM at its cap: depth K = 16383 * 8 = 131,064 < 2^17 (ks_digits_l_kernel<8>),
    every digit of a row of one sign and near-maximal (mask fields 1000000 decompose to -64, -63 x 7; the negated word
    to +64, +63 x 7) against key words whose eight signed bytes are all -128 / all +127.  The largest plane sum is
    16383 * (64 + 7 * 63) * 128 = 1,058,997,120 = 2^29.98 (2^29.97 with +127), against 2^22 or so on random data."""
    import torch
    in_dim, out_dim, base_log, level, batch = 16383, 15, 7, 8, 20
    g = H.rng(key_word & 0xFFFF)
    chain = sum(64 << (8 + 7 * j) for j in range(level))
    signs = np.where(np.arange(batch) % 2 == 0, np.uint64(chain), np.uint64(M64 - chain))
    with np.errstate(over="ignore"):
        lwe = signs[:, None] + g.integers(0, 128, size=(batch, in_dim + 1), dtype=np.uint64)  # below the rounding tie
    lwe[:, -1] = H.uniform_u64(g, batch)
    assert D.py_decompose(chain, base_log, level) == [-64] + [-63] * 7
    assert D.py_decompose(M64 - chain + 127, base_log, level) == [64] + [63] * 7
    key_bytes = [-128] * 8 if key_word & 0x80 else [127] * 8
    assert sum(b << (8 * t) for t, b in enumerate(key_bytes)) % M64 == key_word
    row_sum = sum(D.py_decompose(int(lwe[0, 0]), base_log, level)) * in_dim  # every word of a row has the same digits
    assert all(D.py_decompose(int(x), base_log, level) == D.py_decompose(int(lwe[0, 0]), base_log, level)
               for x in lwe[0, :64])
    assert 2 ** 29 < abs(row_sum * key_bytes[0]) < 2 ** 31
    ksk = np.full((in_dim, level, out_dim + 1), key_word, np.uint64)
    K = engine.lwe_keyswitch
    out = torch.zeros((batch, out_dim + 1), dtype=torch.int64, device="cuda")
    K.keyswitch_lwe_ciphertext(K.LweKeyswitchKey(dev(ksk), base_log, level), dev(lwe), out)
    assert np.array_equal(host(out), oracle.lwe_keyswitch(ksk, lwe, out_dim, base_log, level, threads=16))


# ---- NTT external product and CMUX ----
NTT_CASES = ([(2048, 1, b, l) for b, l in [(23, 1), (31, 1),                                # pbs_tw.hip generated bodies
                                           (12, 2), (17, 3), (4, 4), (1, 9), (32, 1), (40, 1)]]  # pbs_kernels.hip
             + [(512, 4, 23, 1), (512, 4, 7, 3)]                                             # pbs_kernels.hip, k = 4
             + [(8192, 1, 23, 1), (8192, 1, 12, 2)])                                         # pbs_large.hip


def _words(base_log, level, bnf):
    return D.corner_words(base_log, level) if bnf else D.corner_words_nonnative(base_log, level, P)


@pytest.mark.parametrize("bnf", [True, False])
@pytest.mark.parametrize("n,k,base_log,level", NTT_CASES)
def test_ntt_external_product_corners(engine, oracle, n, k, base_log, level, bnf):
    q = 0 if bnf else P
    M = engine.ntt64_pbs
    plan, ctx = engine.Plan.try_new(n, P), oracle.NttContext(n)
    g = H.rng(n + 31 * k + 7 * base_log + level + 1000 * bnf)
    batch = 2
    glwe = D.corner_batch(_words(base_log, level, bnf), (batch, k + 1, n), g, q=q)
    ggsw = rand_q(g, (level, k + 1, k + 1, n), P)
    out0 = rand_q(g, (batch, k + 1, n), q)
    want = np.stack([ctx.ext_product(out0[b].reshape(-1), ggsw.reshape(-1), glwe[b].reshape(-1), k, base_log, level,
                                     bnf=bnf).reshape(k + 1, n) for b in range(batch)])
    out = dev(out0)
    (M.add_external_product_ntt64_bnf_assign if bnf else M.add_external_product_ntt64_assign)(
        plan, out, dev(ggsw), dev(glwe), base_log, level)
    assert np.array_equal(host(out), want)
    # CMUX: ct1 - ct0 is the corner GLWE
    ct1 = H.add_q(out0, glwe, q)
    t0, t1 = dev(out0), dev(ct1)
    (M.cmux_ntt64_bnf_assign if bnf else M.cmux_ntt64_assign)(plan, t0, t1, dev(ggsw), base_log, level)
    assert np.array_equal(host(t1), glwe)
    want0 = np.stack([ctx.cmux(out0[b].reshape(-1), ct1[b].reshape(-1), ggsw.reshape(-1), k, base_log, level,
                               bnf=bnf).reshape(k + 1, n) for b in range(batch)])
    assert np.array_equal(want0, want)
    assert np.array_equal(host(t0), want0)


@pytest.mark.parametrize("bnf", [True, False])
@pytest.mark.parametrize("base_log,level", D.NTT_SHAPES)
def test_ntt_external_product_digit_probe(engine, oracle, base_log, level, bnf):
    """N = 2048, k = 1 ((23,1), (31,1): pbs_tw.hip, the others pbs_kernels.hip).  One GGSW row is the transform of a
    constant (1 for BNF, which normalises; 1 / N for the Solinas modulus), so the result is digit polynomial li of one
    component: compared with the big-integer transcriptions and with the oracle."""
    n, k = 2048, 1
    q = 0 if bnf else P
    M = engine.ntt64_pbs
    plan, ctx = engine.Plan.try_new(n, P), oracle.NttContext(n)
    glwe = D.corner_batch(_words(base_log, level, bnf), (k + 1, n), H.rng(base_log + 64 * level + bnf), q=q)
    if bnf:
        digits = [[D.py_decompose(int(x), base_log, level) for x in comp] for comp in glwe]
    else:
        digits = [[D.py_decompose_nonnative(int(x), base_log, level, P) for x in comp] for comp in glwe]
    for li in range(level):
        for r in range(k + 1):
            ggsw = D.probe_ggsw(level, k, n, li, r, 1 if bnf else ctx.plan.n_inv)
            if bnf:
                poly = np.array([D.bnf_switch(t[li] % P, P) for t in digits[r]], dtype=np.uint64)
                if base_log <= 31:
                    assert np.array_equal(poly, np.array([t[li] % M64 for t in digits[r]], dtype=np.uint64))
            else:
                poly = np.array([t[li] % P for t in digits[r]], dtype=np.uint64)
            want = ctx.ext_product(np.zeros(2 * n, np.uint64), ggsw.reshape(-1), glwe.reshape(-1), k, base_log, level,
                                   bnf=bnf).reshape(k + 1, n)
            assert np.array_equal(want, np.stack([poly, poly]))  # the digits reach the oracle's output unchanged
            out = dev(np.zeros((1, k + 1, n), np.uint64))
            (M.add_external_product_ntt64_bnf_assign if bnf else M.add_external_product_ntt64_assign)(
                plan, out, dev(ggsw), dev(glwe[None]), base_log, level)
            assert np.array_equal(host(out)[0], want), (li, r)


@pytest.mark.parametrize("n", [2048, 1024, 4096, 32768])
def test_forward_from_decomp_on_digit_polynomials(engine, oracle, n):
    """forward_from_decomp (ntt64.rs:221-240) on the digit polynomials themselves, as wrapping u64 with +-2^(B-1)
    present: the fused N = 2048 body, the window kernels (1024), the split transform (4096), the large-N passes."""
    view = engine.ntt64.Ntt64(P, n).as_view()
    ctx = oracle.NttContext(n)
    rows = []
    for base_log, level in [(23, 1), (7, 3), (31, 1), (40, 1)]:
        poly = D.corner_poly(D.corner_words(base_log, level), n, H.rng(n + base_log))
        terms = [D.py_decompose(int(x), base_log, level) for x in poly]
        for li in range(level):
            row = [t[li] % M64 for t in terms]
            assert (1 << (base_log - 1)) in row and M64 - (1 << (base_log - 1)) in row
            rows.append(row)
    d = np.array(rows, dtype=np.uint64)
    dst = dev(np.zeros_like(d))
    view.forward_from_decomp(dst, dev(d))
    assert np.array_equal(host(dst), ctx.forward_from_decomp(d))


# ---- one blind-rotation step: n_lwe = 1, the mask word switching to 1 and the body to 0, so the decomposed GLWE
# is X * LUT - LUT, which a LUT built by prefix sums makes the corpus ----
def _one_step_lut(words, k, n, g, q):
    """(LUT (k + 1, N), target (k + 1, N)): coefficient j >= 1 of X * LUT - LUT is target[., j]."""
    target = D.corner_batch(words, (k + 1, n), g, q=q)
    mod = q or M64
    lut = np.zeros((k + 1, n), np.uint64)
    for c in range(k + 1):
        acc, col = 0, [0]
        for j in range(1, n):       # (X L - L)[j] = L[j - 1] - L[j]
            acc = (acc - int(target[c, j])) % mod
            col.append(acc)
        lut[c] = col
    return lut, target


def _assert_corners_reach_the_decomposer(oracle, lut, target, q):
    for c in range(lut.shape[0]):
        rot = oracle.poly_monomial_mul(lut[c], 1, q)
        diff = H.sub_q(rot, lut[c], q)
        assert np.array_equal(diff[1:], target[c, 1:])


def _mask_switching_to_one(oracle, n, q):
    log2n = n.bit_length()  # log2(2N)
    if not q:
        a = 1 << (64 - log2n)
        assert oracle.modulus_switch(a, log2n) == 1 and oracle.modulus_switch(0, log2n) == 0
    else:
        a = (q + n) // (2 * n)
        assert oracle.pbs_modulus_switch_non_native(a, n, q) == 1 and oracle.pbs_modulus_switch_non_native(0, n, q) == 0
    return a


@pytest.mark.parametrize("bnf", [True, False])
@pytest.mark.parametrize("n,k,base_log,level", [
    (2048, 1, 23, 1),   # the fused pbs_tw.hip kernels
    (2048, 1, 12, 2),   # pbs_kernels.hip
    (512, 4, 23, 1),    # pbs_kernels.hip, k = 4
    (8192, 1, 12, 2),   # pbs_large.hip
])
def test_pbs_one_step_corners(engine, oracle, n, k, base_log, level, bnf):
    q = 0 if bnf else P
    M = engine.ntt64_pbs
    plan, ctx = engine.Plan.try_new(n, P), oracle.NttContext(n)
    g = H.rng(3 * n + k + base_log + bnf)
    lut, target = _one_step_lut(_words(base_log, level, bnf), k, n, g, q)
    _assert_corners_reach_the_decomposer(oracle, lut, target, q)
    a = _mask_switching_to_one(oracle, n, q)
    lwe = np.array([[a, 0], [a + 1, 0]], dtype=np.uint64)   # two ciphertexts, both one step of X^1
    bsk = rand_q(g, (1, level, k + 1, k + 1, n), P)
    want = np.stack([ctx.pbs(row, lut.reshape(-1), bsk.reshape(-1), k, base_log, level, bnf=bnf) for row in lwe])
    key = M.NttBootstrapKey(plan, dev(bsk), base_log, level, M.BNF if bnf else M.SOLINAS)
    out = dev(np.zeros((2, k * n + 1), np.uint64))
    (M.programmable_bootstrap_ntt64_bnf_lwe_ciphertext_mem_optimized if bnf else
     M.programmable_bootstrap_ntt64_lwe_ciphertext_mem_optimized)(dev(lwe), out, dev(lut), key)
    assert np.array_equal(host(out), want)


# ---- the f64 paths: against the exact integer product, under the bound of test_external_product_vs_exact ----
def _negacyclic(a, b):
    """a (signed digits as wrapping u64) x b in Z_2^64[X] / (X^N + 1)."""
    n = a.size
    out = np.zeros(n, np.uint64)
    with np.errstate(over="ignore"):
        for j in np.nonzero(a)[0]:
            j = int(j)
            out += a[j] * np.concatenate([np.uint64(0) - b[n - j:], b[:n - j]])
    return out


def _exact_ext_product(glwe, ggsw, base_log, level):
    """test_fft_gpu._exact_ext_product for any N: sum over levels and rows of digit polynomial x GGSW row."""
    kp1, n = glwe.shape
    out = np.zeros((kp1, n), np.uint64)
    with np.errstate(over="ignore"):
        for li, term in enumerate(F.decompose(glwe, base_log, level)):
            for r in range(kp1):
                for c in range(kp1):
                    out[c] += _negacyclic(term[r], ggsw[li, r, c])
    return out


@pytest.mark.parametrize("n,base_log,level", [
    (2048, 23, 1), (2048, 31, 1),   # fft64_pbs.hip, level 1: decompose_l1_hi
    (2048, 12, 2), (2048, 8, 3),    # fft64_pbs.hip, the multi-level path
    (256, 23, 1), (256, 10, 2),     # fft64_generic.hip
])
def test_fft_external_product_corners(engine, n, base_log, level):
    import torch
    k, batch = 1, 2
    fft = engine.fft64.Fft(n)
    g = H.rng(9000 + n + base_log + level)
    ggsw = H.uniform_u64(g, (level, k + 1, k + 1, n))
    fg = torch.zeros((level, k + 1, k + 1, n // 2, 2), dtype=torch.float64, device="cuda")
    fft.forward_as_torus(fg, dev(ggsw))
    glwe = D.corner_batch(D.corner_words(base_log, level), (batch, k + 1, n), g)
    out0 = H.uniform_u64(g, (batch, k + 1, n))
    out = dev(out0)
    engine.fft64.add_external_product_assign(out, fg, dev(glwe), base_log, level, fft)
    got = host(out)
    for b in range(batch):
        with np.errstate(over="ignore"):
            want = out0[b] + _exact_ext_product(glwe[b], ggsw, base_log, level)
        err = F.signed_diff(got[b], want).max()
        print(f"f64 ext N={n} ({base_log},{level}) row {b}: log2 err = {np.log2(max(err, 1)):.1f}")
        assert err < 2.0 ** max(48, base_log + 24), (b, np.log2(err))


def test_fft_pbs_one_step_corners(engine, oracle):
    """fft64_pbs.hip pbs_kernel_k1l1 at N = 2048 (23,1).  One step: acc = LUT + GGSW (.) (X LUT - LUT), and the
    extracted sample is a signed permutation of acc's coefficients, so the external product's bound carries over."""
    import torch
    n, k, base_log, level = 2048, 1, 23, 1
    fft = engine.fft64.Fft(n)
    g = H.rng(9100)
    lut, target = _one_step_lut(D.corner_words(base_log, level), k, n, g, 0)
    _assert_corners_reach_the_decomposer(oracle, lut, target, 0)
    a = _mask_switching_to_one(oracle, n, 0)
    assert int(F.modulus_switch(np.array([a], np.uint64), n.bit_length())[0]) == 1
    lwe = np.array([[a, 0], [a + 1, 0]], dtype=np.uint64)
    bsk = H.uniform_u64(g, (1, level, k + 1, k + 1, n))
    fbsk = torch.zeros((1, level, k + 1, k + 1, n // 2, 2), dtype=torch.float64, device="cuda")
    engine.fft64.convert_standard_lwe_bootstrap_key_to_fourier(dev(bsk), fbsk, fft)
    key = engine.fft64.FourierLweBootstrapKey(fbsk, base_log, level, fft)
    out = dev(np.zeros((2, k * n + 1), np.uint64))
    engine.fft64.programmable_bootstrap_lwe_ciphertext(dev(lwe), out, dev(lut), key)
    ct1 = np.stack([H.sub_q(oracle.poly_monomial_mul(lut[c], 1, 0), lut[c], 0) for c in range(k + 1)])
    with np.errstate(over="ignore"):
        acc = lut + _exact_ext_product(ct1, bsk[0], base_log, level)
    want = oracle.sample_extract(acc.reshape(-1), n, k, 0)
    err = F.signed_diff(host(out), np.stack([want, want])).max()
    print(f"f64 one-step PBS: log2 err = {np.log2(max(err, 1)):.1f}")
    assert err < 2.0 ** max(48, base_log + 24), np.log2(err)
