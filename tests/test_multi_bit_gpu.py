"""GPU parity of the multi-bit PBS on the f64-FFT path (tfhe_ntt_amd.fft64, csrc/fft64_multi_bit.hip) (`-m gpu`).

The bar is the f64-FFT path's own (tests/test_fft_gpu.py): one blind-rotation step within the f64 bound of the EXACT
integer result, every subset's monomial degree pinned through a noiseless trivial key, outputs that decrypt to f(m)
under real keys with the phase noise of the numpy restatement (tests/multi_bit_helpers.py), and one fixed order.
"""
import ctypes

import numpy as np
import pytest

import fft_oracle as F
import multi_bit_helpers as MB
import tfhe_helpers as H

pytestmark = pytest.mark.gpu

N, M = 2048, 1024


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


@pytest.fixture(scope="module")
def fft(engine):
    return engine.fft64.Fft(N)


def fourier_key(engine, fft, bsk_std, base_log, level, g):
    """standard multi-bit key (groups, 2^g, level, k+1, k+1, N) u64 -> FourierLweMultiBitBootstrapKey"""
    import torch
    fbsk = torch.zeros(bsk_std.shape[:-1] + (M, 2), dtype=torch.float64, device="cuda")
    engine.fft64.convert_standard_lwe_multi_bit_bootstrap_key_to_fourier(dev(bsk_std), fbsk, fft)
    return engine.fft64.FourierLweMultiBitBootstrapKey(fbsk, base_log, level, g, fft)


def decode(pts, delta, msg_mod):
    with np.errstate(over="ignore"):
        return ((pts + np.uint64(delta // 2)) // np.uint64(delta)) % np.uint64(2 * msg_mod)


# ---- 1. one step against the exact integer result ----------------------------------------------------------------
@pytest.mark.parametrize("k,base_log,level,g", [(1, 22, 1, 4), (1, 23, 1, 2), (1, 10, 2, 3), (2, 15, 1, 2),
                                                (2, 8, 3, 4), (1, 31, 1, 3)])
def test_one_step_vs_exact(engine, fft, k, base_log, level, g):
    rng = H.rng(1000 * k + 10 * base_log + level + 100 * g)
    batch = 3
    grp = H.uniform_u64(rng, (1, 1 << g, level, k + 1, k + 1, N))
    key = fourier_key(engine, fft, grp, base_log, level, g)
    acc0 = H.uniform_u64(rng, (batch, k + 1, N))
    acc0[0, 0, :4] = np.array([0, 2**64 - 1, 2**63, 2**63 - 1], np.uint64)
    lwe = H.uniform_u64(rng, (batch, g + 1))
    acc = dev(acc0)
    engine.fft64.multi_bit_blind_rotate_assign(dev(lwe), acc, key)
    got = host(acc)
    for b in range(batch):
        want = MB.exact_single_step(acc0[b], lwe[b], grp[0], base_log, level, g)
        err = F.signed_diff(got[b], want).max()
        print(f"k={k} B={base_log} l={level} g={g} item {b}: log2 err = {np.log2(max(err, 1.0)):.2f}")
        # the f64 bound of an external product (test_fft_gpu.py test_external_product_vs_exact)
        assert err < 2.0 ** max(48, base_log + 24), (b, np.log2(err))


# ---- 2. every subset's degree, pinned ----------------------------------------------------------------------------
def _split(rng, total, parts):
    """`parts` u64 values whose wrapping sum is `total`."""
    v = H.uniform_u64(rng, parts)
    with np.errstate(over="ignore"):
        v[-1] = np.uint64(total % 2**64) - v[:-1].sum(dtype=np.uint64)
    return v


def _corner_masks(rng, idx, g):
    """(7, g) masks and the degree each must give for subset `idx` (popcount >= 1); unselected elements are random."""
    sel = [m for m, bit in enumerate(MB.selection_bits(idx, g)) if bit]
    s = len(sel)
    pair = lambda v: np.array([v, v] + [0] * (s - 2), np.uint64)
    rows = [
        (pair(2**63) if s >= 2 else _split(rng, 0, s), 0),                    # a sum that wraps 2^64
        (_split(rng, 2**51, s), 1),                                             # the tie
        (pair(2**50) if s >= 2 else _split(rng, 2**51, s), 1),                # element-wise switching gives 0
        (_split(rng, (1500 << 52) + 12345, s), 1500),                           # [N/2, N)
        (_split(rng, (3000 << 52) - 99, s), 3000),                              # [N, 2N)
        (_split(rng, 2**51 - 1, s), 0),                                         # degree 0
        (_split(rng, 2**64 - 2**51 - 1, s), 4095),                              # degree 2N - 1
    ]
    masks = H.uniform_u64(rng, (len(rows), g))
    for i, (vals, _) in enumerate(rows):
        masks[i, sel] = vals
    return masks, [d for _, d in rows]


@pytest.mark.parametrize("g", [2, 3, 4])
def test_every_subset_degree(engine, fft, g):
    """A noiseless trivial key: GGSW idx* is the gadget matrix, the others are zero, so the step's output is
    closest_representable(acc) X^(d_idx*).  acc[j] = j 2^52: a degree off by one moves every coefficient by 2^52."""
    k, base_log, level = 1, 16, 3
    rng = H.rng(500 + g)
    acc0 = np.broadcast_to((np.arange(N, dtype=np.uint64) << np.uint64(52)), (k + 1, N)).copy()
    gadget = np.zeros((level, k + 1, k + 1, N), np.uint64)
    for li in range(level):
        for r in range(k + 1):
            gadget[li, r, r, 0] = np.uint64(1 << (64 - base_log * (level - li)))
    for idx in range(1 << g):
        grp = np.zeros((1, 1 << g, level, k + 1, k + 1, N), np.uint64)
        grp[0, idx] = gadget
        key = fourier_key(engine, fft, grp, base_log, level, g)
        if idx == 0:
            masks, want_d = H.uniform_u64(rng, (7, g)), [0] * 7  # GGSW 0 is never rotated
        else:
            masks, want_d = _corner_masks(rng, idx, g)
            assert MB.group_degrees(masks, g)[:, idx].tolist() == want_d  # the masks hit their corners
        body = H.uniform_u64(rng, (masks.shape[0], 1))
        lwe = np.concatenate([masks, body], axis=1)
        acc = dev(np.broadcast_to(acc0, (lwe.shape[0], k + 1, N)))
        engine.fft64.multi_bit_blind_rotate_assign(dev(lwe), acc, key)
        got = host(acc)
        for b in range(lwe.shape[0]):
            body_d = int(F.modulus_switch(lwe[b, g], 12)) % (2 * N)
            want = MB.monomial_mul(acc0, (2 * N - body_d + want_d[b]) % (2 * N))
            err = F.signed_diff(got[b], want).max()
            assert err < 2.0 ** 48, (idx, b, want_d[b], np.log2(max(err, 1.0)))


# ---- real keys ---------------------------------------------------------------------------------------------------
_KEYS = {}


def real_key(engine, fft, oracle, k, level, base_log, g, n_lwe=48):
    """One seeded key set per shape, shared by the tests below (the standard key stays on the host for the restatement)."""
    at = (k, level, base_log, g, n_lwe)
    if at not in _KEYS:
        rng = H.rng(4800 + 1000 * k + 100 * level + 10 * g + base_log)
        lwe_sk = H.binary_key(rng, n_lwe)
        glwe_sk = H.binary_key(rng, (k, N))
        bsk = MB.multi_bit_bsk_gen(rng, oracle, lwe_sk, glwe_sk, base_log, level, 17, g)
        _KEYS[at] = (lwe_sk, glwe_sk, bsk, fourier_key(engine, fft, bsk, base_log, level, g))
    return _KEYS[at]


MSG_MOD = 4
DELTA = (1 << 63) // MSG_MOD


def _inputs(seed, lwe_sk, count):
    rng = H.rng(seed)
    msgs = np.arange(count) % MSG_MOD
    return msgs, H.lwe_encrypt_batch(rng, msgs.astype(np.uint64) * np.uint64(DELTA), lwe_sk, 30)


@pytest.mark.parametrize("g", [2, 3, 4])
@pytest.mark.parametrize("k,level,base_log", [(1, 1, 22), (1, 2, 12), (2, 1, 23), (2, 2, 12)])
def test_real_keys_decrypt(engine, fft, oracle, k, level, base_log, g):
    lwe_sk, glwe_sk, _, key = real_key(engine, fft, oracle, k, level, base_log, g)
    f = lambda x: (x + 3) % MSG_MOD
    lut = H.pbs_lut(N, k, MSG_MOD, DELTA, f)
    msgs, lwe = _inputs(31 + g, lwe_sk, 8)
    out = dev(np.zeros((len(msgs), k * N + 1), np.uint64))
    engine.fft64.multi_bit_programmable_bootstrap_lwe_ciphertext(dev(lwe), out, dev(lut), key)
    pts = H.lwe_decrypt_batch(host(out), H.glwe_sk_as_lwe_sk(glwe_sk))
    assert list(decode(pts, DELTA, MSG_MOD)) == [f(int(m)) for m in msgs]


def test_phase_noise_matches_the_restatement(engine, fft, oracle):
    """(k, l, B) = (1, 1, 22), g = 4, batch 256: the rms phase noise within a factor 4 either way of the numpy
    restatement's over 8 of the same inputs (the form of test_pbs_config4_full_batch_real_keys)."""
    base_log, level, g, batch = 22, 1, 4, 256
    lwe_sk, glwe_sk, bsk, key = real_key(engine, fft, oracle, 1, level, base_log, g)
    f = lambda x: (3 * x + 2) % MSG_MOD
    lut = H.pbs_lut(N, 1, MSG_MOD, DELTA, f)
    msgs, lwe = _inputs(256, lwe_sk, batch)
    out = dev(np.zeros((batch, N + 1), np.uint64))
    engine.fft64.multi_bit_programmable_bootstrap_lwe_ciphertext(dev(lwe), out, dev(lut), key)
    sk = H.glwe_sk_as_lwe_sk(glwe_sk)
    pts = H.lwe_decrypt_batch(host(out), sk)
    want_pt = np.array([f(int(m)) for m in msgs], np.uint64) * np.uint64(DELTA)
    assert np.array_equal(decode(pts, DELTA, MSG_MOD), want_pt // np.uint64(DELTA))
    noise = F.signed_diff(pts, want_pt)
    idx = np.array([0, 1, 2, 3, 100, 101, 254, 255])
    ref = MB.multi_bit_pbs(lwe[idx], lut, F.forward_as_torus(bsk), base_log, level, g)
    ref_noise = F.signed_diff(H.lwe_decrypt_batch(ref, sk), want_pt[idx])
    rms = lambda e: float(np.sqrt(np.mean(e ** 2)))
    print(f"log2 rms: gpu {np.log2(rms(noise)):.2f}, restatement {np.log2(rms(ref_noise)):.2f}")
    assert rms(ref_noise) / 4 < rms(noise) < 4 * rms(ref_noise), (np.log2(rms(noise)), np.log2(rms(ref_noise)))


# ---- 4. ragged batches on the 4-per-workgroup form ---------------------------------------------------------------
@pytest.mark.parametrize("g", [2, 4])
@pytest.mark.parametrize("batch", [1, 5, 7])
def test_ragged_batches(engine, fft, oracle, batch, g):
    lwe_sk, glwe_sk, _, key = real_key(engine, fft, oracle, 1, 1, 22, g)
    f = lambda x: (3 * x + 1) % MSG_MOD
    lut = H.pbs_lut(N, 1, MSG_MOD, DELTA, f)
    msgs, lwe = _inputs(900 + 10 * batch + g, lwe_sk, batch)
    sentinel = np.full((batch + 1, N + 1), 0x5A5A5A5A5A5A5A5A, np.uint64)
    out = dev(sentinel)
    engine.fft64.multi_bit_programmable_bootstrap_lwe_ciphertext(dev(lwe), out[:batch], dev(lut), key)
    got = host(out)
    assert np.array_equal(got[batch], sentinel[batch])  # nothing written past the batch
    pts = H.lwe_decrypt_batch(got[:batch], H.glwe_sk_as_lwe_sk(glwe_sk))
    assert list(decode(pts, DELTA, MSG_MOD)) == [f(int(m)) for m in msgs]


# ---- 5. one fixed order ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,level,base_log", [(1, 1, 22), (2, 2, 12)])
def test_one_fixed_order(engine, fft, oracle, k, level, base_log):
    """The same ciphertext at all 9 positions of a batch (every slot of a 4-per-workgroup group, a ragged last one):
    bit-identical outputs, and a second call repeats them."""
    lwe_sk, glwe_sk, _, key = real_key(engine, fft, oracle, k, level, base_log, 4)
    lut = dev(H.pbs_lut(N, k, MSG_MOD, DELTA, lambda x: (x + 1) % MSG_MOD))
    _, one = _inputs(77, lwe_sk, 1)
    lwe = dev(np.repeat(one, 9, axis=0))
    outs = []
    for _ in range(2):
        out = dev(np.zeros((9, k * N + 1), np.uint64))
        engine.fft64.multi_bit_programmable_bootstrap_lwe_ciphertext(lwe, out, lut, key)
        outs.append(host(out))
    assert all(np.array_equal(outs[0][0], outs[0][i]) for i in range(9))
    assert np.array_equal(outs[0], outs[1])
    pts = H.lwe_decrypt_batch(outs[0], H.glwe_sk_as_lwe_sk(glwe_sk))
    assert list(decode(pts, DELTA, MSG_MOD)) == [1] * 9


# ---- 6. LUT forms ------------------------------------------------------------------------------------------------
def test_lut_forms(engine, fft, oracle):
    import torch
    g = 2
    lwe_sk, glwe_sk, _, key = real_key(engine, fft, oracle, 1, 1, 22, g)
    sk = H.glwe_sk_as_lwe_sk(glwe_sk)
    batch = 6
    msgs, lwe = _inputs(66, lwe_sk, batch)
    fs = [lambda x, c=c: (x + c) % MSG_MOD for c in range(batch)]
    luts = np.stack([H.pbs_lut(N, 1, MSG_MOD, DELTA, f) for f in fs])
    # one accumulator per item (NULL index)
    out = dev(np.zeros((batch, N + 1), np.uint64))
    engine.fft64.batch_multi_bit_programmable_bootstrap_lwe_ciphertext(dev(lwe), out, dev(luts), key)
    dec = decode(H.lwe_decrypt_batch(host(out), sk), DELTA, MSG_MOD)
    assert list(dec) == [fs[b](int(msgs[b])) for b in range(batch)]
    # an index list with one out-of-range entry: that row keeps its sentinel
    index = np.array([2, 0, 3, 3, 1, 0], np.int32)
    index[3] = 3 + 100
    sentinel = np.full((batch, N + 1), 0x5A5A5A5A5A5A5A5A, np.uint64)
    out = dev(sentinel)
    engine.fft64.multi_bit_programmable_bootstrap_lwe_ciphertext(dev(lwe), out, dev(luts[:4]), key,
                                                                 lut_index=torch.from_numpy(index).cuda())
    got = host(out)
    assert np.array_equal(got[3], sentinel[3])
    keep = [b for b in range(batch) if b != 3]
    dec = decode(H.lwe_decrypt_batch(got[keep], sk), DELTA, MSG_MOD)
    assert list(dec) == [fs[int(index[b])](int(msgs[b])) for b in keep]
    # the rotated GLWE itself decrypts to the rotated LUT's sample 0
    acc = dev(luts)
    engine.fft64.multi_bit_blind_rotate_assign(dev(lwe), acc, key)
    dec = decode(H.lwe_decrypt_batch(MB.sample_extract0(host(acc)), sk), DELTA, MSG_MOD)
    assert list(dec) == [fs[b](int(msgs[b])) for b in range(batch)]


# ---- 7. errors ---------------------------------------------------------------------------------------------------
def test_errors(engine, fft):
    from tfhe_ntt_amd import _lib
    L = _lib.lib()
    INVALID, UNSUPPORTED = _lib.MI_ERR_INVALID_ARG, _lib.MI_ERR_UNSUPPORTED
    words = (ctypes.c_double * 4)()  # never dereferenced
    fbsk = ctypes.addressof(words)
    create = L.mi_fft64_multi_bit_pbs_key_create

    def rejected(args, status, message):
        h = ctypes.c_void_p(1)
        st = create(*args, ctypes.byref(h))
        assert (st, L.mi_last_error_message().decode()) == (status, message), args
        assert not h.value, args

    plan = fft.handle
    # (plan, fbsk, n_lwe, k, base_log, level, grouping_factor)
    assert create(plan, fbsk, 48, 1, 22, 1, 4, None) == INVALID
    assert L.mi_last_error_message() == b"out_key is NULL"
    rejected((None, fbsk, 48, 1, 22, 1, 4), INVALID, "plan is NULL")
    rejected((plan, None, 48, 1, 22, 1, 4), INVALID, "bsk is NULL")
    for g in (0, 1, 5, -2):
        rejected((plan, fbsk, 60, 1, 22, 1, g), INVALID, "grouping factor must be 2, 3 or 4")
    rejected((plan, fbsk, 0, 1, 22, 1, 4), INVALID, "n_lwe out of range")
    for n_lwe, g in ((49, 2), (50, 3), (50, 4)):
        rejected((plan, fbsk, n_lwe, 1, 22, 1, g), INVALID, "n_lwe must be a multiple of the grouping factor")
    for base_log, level in ((0, 1), (22, 0), (32, 2), (8, 8), (64, 1), (-3, -3)):
        rejected((plan, fbsk, 48, 1, base_log, level, 4), INVALID, "decomposition base_log * level must be in [1, 63]")
    for k in (0, 3):
        rejected((plan, fbsk, 48, k, 22, 1, 4), UNSUPPORTED, "the multi-bit PBS runs for k in {1, 2}")
    rejected((engine.fft64.Fft(1024).handle, fbsk, 48, 1, 22, 1, 4), UNSUPPORTED, "the multi-bit PBS runs at N = 2048")

    assert L.mi_fft64_multi_bit_pbs_key_destroy(None) == _lib.MI_OK
    for call in (lambda: L.mi_fft64_multi_bit_pbs_key_info(None, None, None, None, None, None),
                 lambda: L.mi_fft64_multi_bit_pbs_batch(None, None, None, None, 1, None),
                 lambda: L.mi_fft64_multi_bit_pbs_batch_lut_indexed(None, None, None, None, None, 1, 1, None),
                 lambda: L.mi_fft64_multi_bit_blind_rotate_batch(None, None, None, 1, None)):
        assert create(plan, fbsk, 48, 1, 22, 1, 4, None) == INVALID  # so that the message read next is the call's own
        assert call() == INVALID
        assert L.mi_last_error_message() == b"key is NULL"

    # a key that is created reports its shape, grouping factor included
    h = ctypes.c_void_p()
    assert create(plan, fbsk, 48, 2, 12, 2, 3, ctypes.byref(h)) == _lib.MI_OK and h.value
    n_lwe, k, bl, lv, g = ctypes.c_size_t(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert L.mi_fft64_multi_bit_pbs_key_info(h, *(ctypes.byref(v) for v in (n_lwe, k, bl, lv, g))) == _lib.MI_OK
    assert (n_lwe.value, k.value, bl.value, lv.value, g.value) == (48, 2, 12, 2, 3)
    assert L.mi_fft64_multi_bit_pbs_batch(h, None, None, None, 0, None) == _lib.MI_OK  # an empty batch is a no-op
    assert L.mi_fft64_multi_bit_pbs_batch(h, None, None, None, 1, None) == INVALID
    assert L.mi_last_error_message() == b"buffer is NULL"
    assert L.mi_fft64_multi_bit_pbs_key_destroy(h) == _lib.MI_OK
