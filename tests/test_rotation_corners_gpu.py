"""Every device copy of the modulus switch, the centered body correction and the monomial rotation on their wrap corners
(`-m gpu`).

Uniform random ciphertexts reach a corner degree (0, 1, N - 1, N, N + 1, 2N - 1), a rounding edge of the switch or a body
on a cell edge with probability about 1 / 2N per word; here the corpus of tests/rotation_corners.py (pinned on the host by
tests/test_rotation_corners.py) is placed in front of each copy, in every key position.  Integer paths are compared bit
for bit with the oracle on a random NTT-domain key; the f64 paths run a noiseless gadget key, whose exact result is the
LUT times a known monomial, under the bound of test_fft_gpu.test_external_product_vs_exact (2^max(48, base_log + 24)),
after asserting on the host that a degree off by one, by N, or a sign boundary off by one moves a coefficient by >= 2^58.

MI_MS_PRE_SWITCHED: the header's contract is "values in [0, 2N)", so the corner degrees are sent and 2N itself is not
(the non-native switch's own 2N is reached through MI_MS_STANDARD on the top words of [0, p)).

Device copy                                                          reached by
  pbs_tw.hip pbs_tw_kernel (BNF: switch, per-step rotation of the      test_integer_paths[2048-1-23-1, BNF x 3 modes],
    generated MI_PBS_BODY_* bodies, final rotation + extraction)       test_lut_indexed[2048-1-23-1]
  pbs_tw.hip centered_body_correction (128 lanes)                      test_centered_lengths[2048-1-23-1], W = 128
  pbs_tw.hip pbs_tw_sol_kernel (LUT pre-rotation into LDS) and         test_integer_paths[2048-1-23-1, Solinas standard]: the
    ms_non_native_kernel (launch_ms_non_native; no entry point          non-native words (x = 1, the top of [0, p) -> 2N)
    exposes its output, so it is covered through this PBS)              go through the kernel; [Solinas pre-switched] skips it
  pbs_kernels.hip pbs_kernel<LOGN, K> (launch_pbs: block =             test_integer_paths[2048-1-12-2] T = 256,
    Shape<LOGN, K>::T = N / 8 for k <= 2, N / 4 for k >= 3),            [512-4-23-1] T = 128, [1024-2-15-2] T = 128,
    lift_switched_kernel for PRE_SWITCHED                               [4096-1-23-1] T = 512; test_lut_indexed[2048-1-12-2]
  core_device.hpp centered_body_correction<T> (pbs_kernels.hip)        test_centered_lengths, the same four shapes, W = T
  pbs_large.hip large_init_acc, large_extract (finishing pass)         every N >= 8192 case below
  pbs_large.hip large_rotdec_top<2, ., true> (split_first_pass:        test_integer_paths[8192-1-23-1], [8192-1-12-2] (MAC
    logn - 11 = 2 in one pass)                                          fused: inv_mac_supported l (k + 1) = 2, 4),
                                                                        [8192-1-4-5] (l (k + 1) = 10: the separate large_mac +
                                                                        accumulating inverse), test_large_two_lanes (batch 70)
  pbs_large.hip large_rotdec_top<3, ., true>                           test_large_other_tops[16384]
  pbs_large.hip large_rotdec_tile<4 | 5, ., true> (the third rotate     test_large_other_tops[32768], [65536] (rotdec_top_launch:
    site: K >= 4 and N >> K >= 64)                                       not selectable below N = 32768)
  pbs_large.hip large_rotdec_top<3, ., false>                          test_large_other_tops[131072] (two top passes)
  pbs_large.hip large_rotate_decompose                                 NOT REACHED: launch_pbs_large takes it only without
                                                                        split tables, and every Solinas plan with
                                                                        2^12 <= N <= 2^20 has them (split_of), while
                                                                        check_pbs_shape stops at N = 2^17
  pbs_large.hip large_rotdec_top<1 | 4 | 5, ., .>, <2, ., false>       NOT REACHED: split_first_pass gives K = 1 only at
                                                                        N = 4096 (pbs_kernels.hip's), K >= 4 goes to the tile
  pbs_passes.hip body correction (256 threads)                         test_centered_lengths[8192-1-23-1], W = 256;
                                                                        test_fft_centered_lengths[1024-1-23-1] (corr[] pass)
  fft64_pbs.hip pbs_kernel_k1l1                                        test_fft_paths[2048-1-23-1]
  fft64_pbs.hip pbs_kernel<K, L1> (multi-level, k = 2)                 test_fft_paths[2048-1-12-2], [2048-2-12-2], [2048-2-23-1]
  core_device.hpp centered_body_correction<TG>, TG = 64 (k + 1)        test_fft_centered_lengths[2048-1-23-1] W = 128,
                                                                        [2048-2-12-2] W = 192
  fft64_generic.hip rotate / decompose pass, LUT division, lanes       test_fft_paths[256-1-23-1], [1024-1-10-2],
                                                                        [8192-1-12-2] (batch 70: four lanes)
  keyswitch.hip launch_lwe_ms64 / launch_lwe_ms32                      test_standalone_switches
  pbs128.hip, fft64_multi_bit.hip                                      their own tests (test_pbs128_gpu, test_multi_bit_gpu)
"""
import numpy as np
import pytest

import fft_oracle as F
import rotation_corners as R
import tfhe_helpers as H

pytestmark = pytest.mark.gpu

P = R.P
M64 = R.M64
CTX = {}


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


def rand_q(g, shape, q):
    return g.integers(0, q, size=shape, dtype=np.uint64) if q else H.uniform_u64(g, shape)


def ctx_for(oracle, n):
    if n not in CTX:
        CTX[n] = oracle.NttContext(n)
    return CTX[n]


def _batch_for(n, bnf, mode, seed=0):
    if mode == 2:
        return R.pre_switched_batch(n)
    if mode == 1:
        return R.centered_batch(n, R.KINDS[2 + seed % 2], seed)
    return R.standard_batch(n, 0 if bnf else P)


def _ntt_key(engine, n, bsk, base_log, level, bnf):
    M = engine.ntt64_pbs
    return M.NttBootstrapKey(engine.Plan.try_new(n, P), dev(bsk), base_log, level, M.BNF if bnf else M.SOLINAS)


def _pbs_fn(M, bnf):
    return (M.programmable_bootstrap_ntt64_bnf_lwe_ciphertext_mem_optimized if bnf
            else M.programmable_bootstrap_ntt64_lwe_ciphertext_mem_optimized)


def _run_both(engine, oracle, n, k, base_log, level, bnf, mode, lwe, seed, rotate=True):
    """The LWE-output PBS (one shared LUT) and the GLWE-output blind rotation (one accumulator per item) of `lwe`, bit for
    bit against the oracle's blind rotation of the same items (its PBS is that rotation plus sample_extract)."""
    q = 0 if bnf else P
    g = H.rng(seed)
    batch, n_lwe = lwe.shape[0], lwe.shape[1] - 1
    bsk = rand_q(g, (n_lwe, level, k + 1, k + 1, n), P)
    lut = rand_q(g, (k + 1, n), q)
    accs = rand_q(g, (batch, k + 1, n), q) if rotate else np.zeros((0, k + 1, n), np.uint64)
    c = ctx_for(oracle, n)
    both = np.concatenate([np.broadcast_to(lut, (batch, k + 1, n)), accs])
    lwe2 = np.concatenate([lwe, lwe[:accs.shape[0]]])
    rot = c.blind_rotate_batch(both, lwe2, bsk.reshape(-1), k, base_log, level, bnf=bnf, ms_mode=mode, threads=16)
    want = np.stack([oracle.sample_extract(rot[b].reshape(-1), n, k, q) for b in range(batch)])
    M = engine.ntt64_pbs
    key = _ntt_key(engine, n, bsk, base_log, level, bnf)
    out = dev(np.zeros((batch, k * n + 1), np.uint64))
    _pbs_fn(M, bnf)(dev(lwe), out, dev(lut), key, mode)
    got = host(out)
    bad = [b for b in range(batch) if not np.array_equal(got[b], want[b])]
    assert not bad, ("pbs", bad, lwe[bad[0]].tolist())
    if rotate:
        t = dev(accs)
        (M.blind_rotate_ntt64_bnf_assign if bnf else M.blind_rotate_ntt64_assign)(dev(lwe), t, key, mode)
        got = host(t)
        bad = [b for b in range(batch) if not np.array_equal(got[b], rot[batch + b])]
        assert not bad, ("blind rotate", bad, lwe[bad[0]].tolist())


# ---- integer paths ---------------------------------------------------------------------------------------------------
INT_SHAPES = [
    (2048, 1, 23, 1),   # pbs_tw.hip, both kernels
    (2048, 1, 12, 2),   # pbs_kernels.hip, T = 256
    (512, 4, 23, 1),    # pbs_kernels.hip, k = 4, T = 128
    (1024, 2, 15, 2),   # pbs_kernels.hip, k = 2, T = 128
    (4096, 1, 23, 1),   # pbs_kernels.hip, T = 512
    (8192, 1, 23, 1),   # pbs_large.hip large_rotdec_top<2, ., true>, MAC fused (l (k + 1) = 2)
    (8192, 1, 12, 2),   # ... MAC fused (4)
]
MODES = [(True, 0), (True, 1), (True, 2), (False, 0), (False, 2)]
# ... and the separate MAC pass (l (k + 1) = 10) behind the same rotation kernel: the standard switch of both moduli
INT_CASES = [s + m for s in INT_SHAPES for m in MODES] + [(8192, 1, 4, 5, True, 0), (8192, 1, 4, 5, False, 0)]


@pytest.mark.parametrize("n,k,base_log,level,bnf,mode", INT_CASES)
def test_integer_paths(engine, oracle, n, k, base_log, level, bnf, mode):
    """BNF standard / centered / pre-switched and Solinas standard / pre-switched on the corpus batch: about 25 items,
    the mask the corpus rolled by the item index."""
    lwe = _batch_for(n, bnf, mode, seed=n + base_log)
    _run_both(engine, oracle, n, k, base_log, level, bnf, mode, lwe, 10 * n + 3 * mode + bnf + base_log)


@pytest.mark.parametrize("bnf", [True, False])
@pytest.mark.parametrize("n,k,base_log,level", [(2048, 1, 23, 1), (2048, 1, 12, 2), (8192, 1, 23, 1)])
def test_lut_indexed(engine, oracle, n, k, base_log, level, bnf):
    """One LUT-indexed run per kernel family (pbs_tw.hip, pbs_kernels.hip, pbs_large.hip): item b through LUT b % 3."""
    import torch
    q = 0 if bnf else P
    g = H.rng(5000 + n + base_log + bnf)
    lwe = R.standard_batch(n, q)
    batch, n_lwe = lwe.shape[0], lwe.shape[1] - 1
    bsk = rand_q(g, (n_lwe, level, k + 1, k + 1, n), P)
    luts = rand_q(g, (3, k + 1, n), q)
    idx = (np.arange(batch) % 3).astype(np.int32)
    rot = ctx_for(oracle, n).blind_rotate_batch(luts[idx], lwe, bsk.reshape(-1), k, base_log, level, bnf=bnf, ms_mode=0,
                                                threads=16)
    want = np.stack([oracle.sample_extract(rot[b].reshape(-1), n, k, q) for b in range(batch)])
    out = dev(np.zeros((batch, k * n + 1), np.uint64))
    _pbs_fn(engine.ntt64_pbs, bnf)(dev(lwe), out, dev(luts), _ntt_key(engine, n, bsk, base_log, level, bnf),
                                   lut_index=torch.from_numpy(idx).cuda())
    assert np.array_equal(host(out), want)


@pytest.mark.parametrize("bnf", [True, False])
def test_large_two_lanes(engine, oracle, bnf):
    """70 items = two lanes of 35 of the chunk-and-lane driver (pbs_passes.hpp lanes_wanted) at N = 8192: the mask is the
    eight ties (every degree's low edge), the bodies the corpus cycled, so both lanes rotate by every corner degree."""
    n, k, base_log, level = 8192, 1, 23, 1
    if bnf:
        ties = [w for w, _, kind in R.native_words(n) if kind == "low"]
        bodies = [w for w, _, _ in R.native_words(n)]
    else:
        ties = [w for w, _, kind in R.nonnative_words(n, P) if kind == "low"][:8]
        bodies = [w for w, _, _ in R.nonnative_words(n, P)]
    lwe = R.roll_batch(ties, [bodies[b % len(bodies)] for b in range(70)])
    _run_both(engine, oracle, n, k, base_log, level, bnf, 0, lwe, 8192070 + bnf)


@pytest.mark.parametrize("bnf", [True, False])
@pytest.mark.parametrize("n", [16384, 32768, 65536, 131072])
def test_large_other_tops(engine, oracle, n, bnf):
    """The rotate sites no shape selects at N = 8192 (rotdec_top / rotdec_top_launch with split_first_pass): 16384
    large_rotdec_top<3, ., true>, 32768 / 65536 large_rotdec_tile<4 | 5>, 131072 large_rotdec_top<3, ., false>.  Eight
    items, the mask the eight ties, the bodies the high edges: every corner degree in every position, at the oracle's
    cost of 64 CMUX steps."""
    if bnf:
        words = R.native_words(n)
    else:
        words = R.nonnative_words(n, P)[2:]
    ties = [w for w, _, kind in words if kind == "low"][:8]
    highs = [w for w, _, kind in words if kind == "high"][-8:]           # non-native: the top of [0, p) (-> 2N) included
    _run_both(engine, oracle, n, 1, 23, 1, bnf, 0, R.roll_batch(ties, highs), n + bnf, rotate=False)


# (N, k, base_log, level, W): W the reduction width of the copy of the correction the shape runs
CENTERED_SHAPES = [
    (2048, 1, 23, 1, 128),   # pbs_tw.hip centered_body_correction
    (2048, 1, 12, 2, 256),   # core_device.hpp centered_body_correction<T>, T = Shape<11, 1>::T
    (512, 4, 23, 1, 128),    # T = Shape<9, 4>::T
    (1024, 2, 15, 2, 128),   # T = Shape<10, 2>::T
    (4096, 1, 23, 1, 512),   # T = Shape<12, 1>::T
    (8192, 1, 23, 1, 256),   # pbs_passes.hip launch_body_correction
]


@pytest.mark.parametrize("which", range(5))
@pytest.mark.parametrize("n,k,base_log,level,width", CENTERED_SHAPES)
def test_centered_lengths(engine, oracle, n, k, base_log, level, width, which):
    """The strided reduction of the in-kernel correction at n_lwe in {1, W - 1, W, W + 1, 2W + 3}: sixteen items with
    cheap zero-switching masks (skipped steps) plus four corner words, every kind of parity and sign, the body on a cell
    edge after the correction; bit for bit against ctx.pbs(..., centered=True)."""
    n_lwe = R.length_cases(width)[which]
    lwe = R.centered_length_batch(n, n_lwe)
    g = H.rng(n + 7 * n_lwe + k)
    bsk = rand_q(g, (n_lwe, level, k + 1, k + 1, n), P)
    lut = H.uniform_u64(g, (k + 1, n))
    c = ctx_for(oracle, n)
    want = c.pbs_batch_bnf(lwe, lut.reshape(-1), bsk.reshape(-1), k, base_log, level, threads=16, centered=True)
    assert np.array_equal(want[0], c.pbs(lwe[0], lut.reshape(-1), bsk.reshape(-1), k, base_log, level, centered=True))
    M = engine.ntt64_pbs
    out = dev(np.zeros((lwe.shape[0], k * n + 1), np.uint64))
    _pbs_fn(M, True)(dev(lwe), out, dev(lut), _ntt_key(engine, n, bsk, base_log, level, True), M.MS_CENTERED)
    got = host(out)
    bad = [b for b in range(lwe.shape[0]) if not np.array_equal(got[b], want[b])]
    assert not bad, (n_lwe, bad)


# ---- the f64 paths: the noiseless gadget key ----------------------------------------------------------------------------
def _fourier_key(engine, n, bits, k, base_log, level):
    import torch
    fft = engine.fft64.Fft(n)
    std = R.gadget_key(bits, k, n, base_log, level)
    fbsk = torch.zeros((len(bits), level, k + 1, k + 1, n // 2, 2), dtype=torch.float64, device="cuda")
    engine.fft64.convert_standard_lwe_bootstrap_key_to_fourier(dev(std), fbsk, fft)
    return engine.fft64.FourierLweBootstrapKey(fbsk, base_log, level, fft)


def _mutant_gap(lut_rows, d):
    """The smallest, over the mutants, of the largest coefficient distance between LUT X^d and the mutant's result:
    degree - 1, degree + 1, degree + N, and the sign boundary moved by one (e <= rem for e < rem)."""
    n = len(lut_rows[0])
    poly = lut_rows[-1]
    true = R.py_monomial_mul(poly, d)
    rem, full = d % n, (d // n) % 2
    moved = [R._neg(poly[(e - rem) % n], 0) if full ^ (e <= rem) else poly[(e - rem) % n] for e in range(n)]
    mutants = [R.py_monomial_mul(poly, (d - 1) % (2 * n)), R.py_monomial_mul(poly, (d + 1) % (2 * n)),
               R.py_monomial_mul(poly, (d + n) % (2 * n)), moved]
    return min(max(abs(R._signed((a - b) % M64)) for a, b in zip(true, m)) for m in mutants)


def _run_fft(engine, n, k, base_log, level, mode, lwe, switched, tag):
    """PBS (shared LUT) and blind_rotate_assign (the LUT copied per item) on the gadget key against the exact rotation."""
    batch, n_lwe = lwe.shape[0], lwe.shape[1] - 1
    bits = R.secret_bits(n_lwe, n + base_log)
    lut = R.gadget_lut(k, n, base_log, level, 11)
    lut_rows = R.rows(lut)
    want_glwe, want_lwe, by_degree = [], [], {}
    for b in range(batch):
        d = R.py_rotation_degree(switched[b], bits, n)
        if d not in by_degree:
            assert _mutant_gap(lut_rows, d) >= 1 << 58, (b, d)            # the bound below cannot hide a mutant
            acc = [R.py_monomial_mul(p, d) for p in lut_rows]
            by_degree[d] = (acc, R.py_sample_extract(acc))
        want_glwe.append(by_degree[d][0])
        want_lwe.append(by_degree[d][1])
    want_glwe, want_lwe = np.array(want_glwe, dtype=np.uint64), np.array(want_lwe, dtype=np.uint64)
    key = _fourier_key(engine, n, bits, k, base_log, level)
    bound = 2.0 ** max(48, base_log + 24)
    out = dev(np.zeros((batch, k * n + 1), np.uint64))
    engine.fft64.programmable_bootstrap_lwe_ciphertext(dev(lwe), out, dev(lut), key, mode)
    err = F.signed_diff(host(out), want_lwe).max(axis=1)
    print(f"f64 {tag} N={n} k={k} ({base_log},{level}) mode {mode} pbs: log2 err = {np.log2(max(err.max(), 1)):.1f}")
    assert err.max() < bound, ("pbs", [int(b) for b in np.nonzero(err >= bound)[0]], np.log2(err.max()))
    acc = dev(np.broadcast_to(lut, (batch, k + 1, n)))
    engine.fft64.blind_rotate_assign(dev(lwe), acc, key, mode)
    err = F.signed_diff(host(acc), want_glwe).reshape(batch, -1).max(axis=1)
    print(f"f64 {tag} N={n} k={k} ({base_log},{level}) mode {mode} rotate: log2 err = {np.log2(max(err.max(), 1)):.1f}")
    assert err.max() < bound, ("blind rotate", [int(b) for b in np.nonzero(err >= bound)[0]], np.log2(err.max()))


FFT_SHAPES = [
    (2048, 1, 23, 1),   # fft64_pbs.hip pbs_kernel_k1l1
    (2048, 1, 12, 2),   # fft64_pbs.hip pbs_kernel<1, false>
    (2048, 2, 12, 2),   # fft64_pbs.hip pbs_kernel<2, false>
    (2048, 2, 23, 1),   # fft64_pbs.hip pbs_kernel<2, true>
    (256, 1, 23, 1),    # fft64_generic.hip
    (1024, 1, 10, 2),   # fft64_generic.hip
    (8192, 1, 12, 2),   # fft64_generic.hip, batch 70: lanes
]


@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("n,k,base_log,level", FFT_SHAPES)
def test_fft_paths(engine, n, k, base_log, level, mode):
    """Standard and pre-switched on the corpus batch (the centered mode: test_fft_centered_lengths)."""
    lwe = _batch_for(n, True, mode)
    if n == 8192:
        lwe = np.concatenate([lwe, lwe, lwe])[:70]
    if mode == 2:
        switched = lwe.tolist()
    else:
        switched = [R.py_switch_lwe([int(x) for x in row], n.bit_length()) for row in lwe]
    _run_fft(engine, n, k, base_log, level, mode, lwe, switched, "corpus")


# (N, k, base_log, level, W)
FFT_CENTERED = [
    (2048, 1, 23, 1, 128),   # core_device.hpp centered_body_correction<TG>, TG = 64 (k + 1) = 128 (pbs_kernel_k1l1)
    (2048, 2, 12, 2, 192),   # TG = 192 (pbs_kernel<2, false>): not a power of two
    (1024, 1, 23, 1, 256),   # fft64_generic.hip: pbs_passes.hip launch_body_correction into corr[]
]


@pytest.mark.parametrize("which", range(5))
@pytest.mark.parametrize("n,k,base_log,level,width", FFT_CENTERED)
def test_fft_centered_lengths(engine, n, k, base_log, level, width, which):
    """The centered switch on the f64 paths at the length cases of each copy's reduction: a correction off by one, or a
    lane's partial sum lost, moves the body across its cell edge and the rotation by a whole degree."""
    n_lwe = R.length_cases(width)[which]
    lwe = R.centered_length_batch(n, n_lwe)
    switched = [R.py_switch_lwe([int(x) for x in row], n.bit_length(), True) for row in lwe]
    _run_fft(engine, n, k, base_log, level, 1, lwe, switched, f"centered n_lwe={n_lwe}")


# ---- the stand-alone switches ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("centered", [False, True])
@pytest.mark.parametrize("n", [512, 8192])
def test_standalone_switches(engine, oracle, n, centered):
    """lwe_ciphertext_modulus_switch (u64) and ...32 on the corpus batch, the centered kinds at mask length 40 and the
    length cases of a 256-thread reduction, at log 12 and log2(2N), against the big-integer switch and the oracle."""
    K = engine.lwe_keyswitch
    for log in sorted({12, n.bit_length()}):
        for bits, mod_switch, ora in ((64, K.lwe_ciphertext_modulus_switch, oracle.lwe_ms64),
                                      (32, K.lwe_ciphertext_modulus_switch32, oracle.lwe_ms32)):
            words = [w for w, _, _ in R.native_words(n, bits)] + [0, 1, (1 << bits) - 1, 1 << (bits - 1)]
            batches = [R.roll_batch(words, words)]
            batches += [R.centered_length_batch(n, length, bits) for length in [40] + R.length_cases(256)]
            for lwe in batches:
                want = np.array([R.py_switch_lwe([int(x) for x in row], log, centered, bits) for row in lwe], np.uint64)
                typed = lwe if bits == 64 else lwe.astype(np.uint32)
                assert np.array_equal(ora(typed, log, centered), want)
                import torch
                src = dev(lwe) if bits == 64 else torch.from_numpy(typed.view(np.int32)).cuda()
                out = dev(np.zeros(lwe.shape, np.uint64))
                mod_switch(src, out, log, centered)
                assert np.array_equal(host(out), want), (log, bits, lwe.shape)
