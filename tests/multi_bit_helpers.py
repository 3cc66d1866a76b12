"""numpy restatement of the multi-bit programmable bootstrap of tfhe core_crypto (host only, test infrastructure).

Built on ``fft_oracle`` (the f64 transform, decomposition and modulus switch) and ``tfhe_helpers`` (seeded keys).
Reference paths relative to /root/reference/tfhe/src/core_crypto:

* ``selection_bits``          algorithms/lwe_multi_bit_programmable_bootstrapping.rs:55-65 (selection_bit)
* ``combined_key_bits``       algorithms/lwe_multi_bit_bootstrap_key_generation.rs:398-421 (combine_key_bits)
* ``group_degrees``           lwe_multi_bit_programmable_bootstrapping.rs:30-51 (modulus_switch_multi_bit: the switch
                              is applied to the wrapping sum of the selected mask elements)
* ``monomial_fourier``        fft_impl/fft64/math/fft/mod.rs:436-473 (incomplete_monomial_forward_as_integer), closed form
* ``multi_bit_blind_rotate``  lwe_multi_bit_programmable_bootstrapping.rs:115-154 (prepare_multi_bit_ggsw_mem_optimized),
                              644-869 (multi_bit_deterministic_blind_rotate_assign)
* ``multi_bit_pbs``           the same plus extract_lwe_sample_from_glwe_ciphertext at degree 0

Fourier arrays are in natural frequency order, as in ``fft_oracle``.  A multi-bit key is an array
(n / g, 2^g, level, k+1, k+1, N): group-major, GGSW ``idx`` of group i encrypting
prod_m (s[i g + m] XOR NOT bit_m(idx)).
"""
import numpy as np

import fft_oracle as F
import tfhe_helpers as H

U64 = np.uint64


def selection_bits(idx: int, g: int) -> list:
    """bit_m(idx) = (idx >> (g - 1 - m)) & 1 for m < g: which mask elements of a group GGSW ``idx`` selects."""
    return [(idx >> (g - 1 - m)) & 1 for m in range(g)]


def combined_key_bits(lwe_sk, g: int) -> np.ndarray:
    """(n / g, 2^g) messages of the key GGSWs: 1 iff every key bit of the group equals its selection bit."""
    sk = np.asarray(lwe_sk, dtype=np.int64).reshape(-1, g)
    out = np.zeros((sk.shape[0], 1 << g), U64)
    for idx in range(1 << g):
        sel = np.array(selection_bits(idx, g), np.int64)
        out[:, idx] = np.prod(np.where(sel[None, :] == 1, sk, 1 - sk), axis=1).astype(U64)
    return out


def multi_bit_bsk_gen(g_rng, oracle, lwe_sk, glwe_sk, base_log, level, noise_log2, g):
    """Standard-domain multi-bit bootstrap key (n / g, 2^g, level, k+1, k+1, N), highest level first."""
    bits = combined_key_bits(lwe_sk, g)
    k, n = glwe_sk.shape
    if k == 1 and level == 1:
        flat = H.bsk_gen_native_l1(g_rng, bits.reshape(-1), glwe_sk, base_log, noise_log2)
    else:
        flat = H.bsk_gen_fast(g_rng, oracle, bits.reshape(-1), glwe_sk, base_log, level, noise_log2)
    return flat.reshape(bits.shape[0], 1 << g, level, k + 1, k + 1, n)


def group_degrees(mask_group, g: int, log_mod: int = 12) -> np.ndarray:
    """mask_group (..., g) u64 -> (..., 2^g) monomial degrees in [0, 2^log_mod), log_mod = log2(2N): the switch of
    the wrapping sum of the elements GGSW ``idx`` selects; entry 0 is 0 (GGSW 0 is not rotated)."""
    a = np.asarray(mask_group, dtype=U64)
    out = np.zeros(a.shape[:-1] + (1 << g,), np.int64)
    for idx in range(1, 1 << g):
        s = np.zeros(a.shape[:-1], U64)
        with np.errstate(over="ignore"):
            for m, bit in enumerate(selection_bits(idx, g)):
                if bit:
                    s = s + a[..., m]
        out[..., idx] = F.modulus_switch(s, log_mod).astype(np.int64) % (1 << log_mod)
    return out


def monomial_fourier(d, n: int) -> np.ndarray:
    """forward_as_integer of X^d mod (X^n + 1), d in [0, 2n), in closed form: zeta^(d (1 - 4 f) mod 2n) at natural
    frequency f < n / 2, zeta = exp(i pi / n).  d (...,) -> (..., n / 2) complex."""
    d = np.asarray(d, dtype=np.int64)[..., None]
    f = np.arange(n // 2, dtype=np.int64)
    e = (d * (1 - 4 * f)) % (2 * n)
    a = np.pi * e.astype(np.float64) / n
    return np.cos(a) + 1j * np.sin(a)


def monomial_mul(p, d) -> np.ndarray:
    """X^d p mod (X^N + 1) exactly, for one degree d in [0, 2N); p (..., N) u64."""
    p = np.asarray(p, dtype=U64)
    n = p.shape[-1]
    src = (np.arange(n) - int(d)) % (2 * n)
    with np.errstate(over="ignore"):
        return np.where(src >= n, U64(0) - p[..., src % n], p[..., src % n])


def _ext_product_per_item(glwe, bundle, base_log, level):
    """bundle (B, level, k+1, k+1, M) complex per item (.) glwe (B, k+1, N) -> (B, k+1, N) u64."""
    acc = 0
    for li, term in enumerate(F.decompose(glwe, base_log, level)):
        acc = acc + np.einsum("brm,brcm->bcm", F.forward_as_integer(term), bundle[:, li])
    return F.backward_as_torus(acc)


def multi_bit_blind_rotate(acc, lwe_in, fbsk, base_log: int, level: int, g: int) -> np.ndarray:
    """acc (B, k+1, N) u64 rotated by lwe_in (B, n + 1); fbsk (n / g, 2^g, level, k+1, k+1, N/2) complex."""
    acc = np.array(acc, dtype=U64)
    lwe_in = np.atleast_2d(np.asarray(lwe_in, dtype=U64))
    n = acc.shape[-1]
    n_lwe = lwe_in.shape[1] - 1
    assert n_lwe % g == 0 and fbsk.shape[0] == n_lwe // g
    log_mod = int(np.log2(n)) + 1
    body = F.modulus_switch(lwe_in[:, n_lwe], log_mod).astype(np.int64) % (2 * n)
    acc = np.stack([monomial_mul(acc[b], (2 * n - int(body[b])) % (2 * n)) for b in range(acc.shape[0])])
    for i in range(n_lwe // g):
        deg = group_degrees(lwe_in[:, i * g:(i + 1) * g], g, log_mod)  # (B, 2^g)
        bundle = np.broadcast_to(fbsk[i, 0], (acc.shape[0],) + fbsk[i, 0].shape).copy()
        for idx in range(1, 1 << g):
            bundle += fbsk[i, idx][None] * monomial_fourier(deg[:, idx], n)[:, None, None, None, :]
        acc = _ext_product_per_item(acc, bundle, base_log, level)  # 0 + bundle (.) acc
    return acc


def multi_bit_pbs(lwe_in, lut, fbsk, base_log: int, level: int, g: int) -> np.ndarray:
    """lut (k+1, N) shared or (B, k+1, N) per item -> (B, k N + 1) u64 (sample 0 of the rotated accumulator)."""
    lwe_in = np.atleast_2d(np.asarray(lwe_in, dtype=U64))
    lut = np.asarray(lut, dtype=U64)
    if lut.ndim == 2:
        lut = np.broadcast_to(lut, (lwe_in.shape[0],) + lut.shape)
    acc = multi_bit_blind_rotate(lut, lwe_in, fbsk, base_log, level, g)
    return sample_extract0(acc)


def sample_extract0(acc) -> np.ndarray:
    bsz, kp1, n = acc.shape
    out = np.zeros((bsz, (kp1 - 1) * n + 1), U64)
    for c in range(kp1 - 1):
        out[:, c * n] = acc[:, c, 0]
        with np.errstate(over="ignore"):
            out[:, c * n + 1:(c + 1) * n] = U64(0) - acc[:, c, :0:-1]
    out[:, -1] = acc[:, kp1 - 1, 0]
    return out


def integer_bundle(group_std, degrees) -> np.ndarray:
    """G_0 + sum_idx X^(d_idx) G_idx exactly in Z_{2^64}[X]/(X^N + 1): group_std (2^g, level, k+1, k+1, N) u64,
    degrees (2^g,) (entry 0 unused)."""
    out = group_std[0].copy()
    with np.errstate(over="ignore"):
        for idx in range(1, group_std.shape[0]):
            out += monomial_mul(group_std[idx], int(degrees[idx]))
    return out


def exact_single_step(acc, lwe, group_std, base_log, level, g):
    """The exact integer result of a one-group blind rotation of one item: acc (k+1, N), lwe (g + 1,)."""
    from test_fft_gpu import _exact_ext_product

    n = acc.shape[-1]
    log_mod = int(np.log2(n)) + 1
    body = int(F.modulus_switch(lwe[g], log_mod)) % (2 * n)
    rotated = monomial_mul(acc, (2 * n - body) % (2 * n))
    deg = group_degrees(lwe[:g], g, log_mod)
    return _exact_ext_product(rotated, integer_bundle(group_std, deg), base_log, level)
