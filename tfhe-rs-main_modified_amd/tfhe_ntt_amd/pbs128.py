"""Host-side mirror of the core_crypto 128-bit programmable bootstrap over the C ABI (``mi_pbs128_*``).

Reference (paths relative to /root/reference/tfhe/src/core_crypto):

* ``programmable_bootstrap_f128_lwe_ciphertext``  algorithms/lwe_programmable_bootstrapping/fft128_pbs.rs:174
* ``blind_rotate_assign_split`` / ``blind_rotate_u128``  fft_impl/fft128_u128/crypto/bootstrap.rs:60-247
* ``add_external_product_assign_split`` / ``cmux_split``  fft_impl/fft128_u128/crypto/ggsw.rs:17, :621-675

* ``multi_bit_programmable_bootstrap_f128_lwe_ciphertext`` / ``multi_bit_f128_deterministic_blind_rotate_assign``
  algorithms/lwe_multi_bit_programmable_bootstrapping.rs:2257-2700 (``mi_pbs128_multi_bit_*``, csrc/pbs128_multi_bit.hip)

The reference multiplies with a double-double FFT; the engine runs exact limb products on the Goldilocks NTT
(csrc/pbs128.hip), so every result equals plain integer arithmetic mod 2^128 bit for bit.  A u128 tensor is int64 (or
uint64) storage with a trailing dimension of 2: the little-endian words (lo, hi).  The reference works on one
ciphertext per call; here a leading batch dimension is allowed.  Shape mismatches raise ``ValueError`` where the
reference panics on ``assert!``.
"""
from __future__ import annotations

import ctypes

from ._lib import check, lib, release
from .ntt64_pbs import _dev, _stream
from .prime64 import SOLINAS_P, Plan

MS_STANDARD, MS_CENTERED, MS_PRE_SWITCHED = 0, 1, 2


def limb_plan(polynomial_size: int, glwe_dimension: int, base_log: int, level: int) -> tuple[int, int]:
    """(limb_bits, n_limbs) of the exact limb split (``mi_pbs128_limb_plan``; needs no device): limb_bits is the
    largest w with (k + 1) level N 2^(base_log - 1) (2^w - 1) <= (p - 1) / 2, n_limbs = ceil(128 / w)."""
    w, nl = ctypes.c_int(), ctypes.c_int()
    check(lib().mi_pbs128_limb_plan(polynomial_size, glwe_dimension, base_log, level, ctypes.byref(w),
                                    ctypes.byref(nl)))
    return w.value, nl.value


def _u128(t, name, tail):
    """The device pointer of a u128 tensor whose trailing dimensions are (*tail, 2); returns (pointer, batch)."""
    want = (*tail, 2)
    if t.dim() < len(want) or tuple(t.shape[-len(want):]) != want:
        raise ValueError(f"assertion failed: {name} shape {tuple(t.shape)} != (..., {', '.join(map(str, want))})")
    count = 1
    for d in want:
        count *= d
    return _dev(t, name), t.numel() // count


class LweBootstrapKey128:
    """An ``LweBootstrapKey<u128>`` prepared for the 128-bit bootstrap (``mi_pbs128_key``).

    ``bsk``: device tensor (n_ggsw, level, k + 1, k + 1, N, 2) in the reference's standard-domain layout (level
    matrices in the order ``ggsw.into_levels()`` yields them).  A private prepared copy (transformed limb polynomials)
    is made; ``bsk`` may be released afterwards."""

    def __init__(self, bsk, base_log: int, level: int, plan: Plan | None = None):
        if bsk.dim() != 6 or bsk.shape[1] != level or bsk.shape[2] != bsk.shape[3] or bsk.shape[5] != 2:
            raise ValueError(f"assertion failed: bsk shape {tuple(bsk.shape)} != (n_ggsw, {level}, k + 1, k + 1, N, 2)")
        self.input_lwe_dimension = int(bsk.shape[0])
        self.glwe_dimension = int(bsk.shape[2]) - 1
        self.polynomial_size = int(bsk.shape[4])
        self.decomposition_base_log, self.decomposition_level_count = base_log, level
        self.device = bsk.device
        # kept alive with the key; by default the process-wide plan of Ntt64::new
        self.plan = plan if plan is not None else Plan.cached(self.polynomial_size, SOLINAS_P, bsk.device.index or 0)
        h = ctypes.c_void_p()
        check(lib().mi_pbs128_key_create(self.plan.handle, _dev(bsk, "bsk"), self.input_lwe_dimension,
                                         self.glwe_dimension, self.polynomial_size, base_log, level, _stream(bsk),
                                         ctypes.byref(h)))
        self._h = h
        w, nl = ctypes.c_int(), ctypes.c_int()
        check(lib().mi_pbs128_key_info(h, None, None, None, None, None, ctypes.byref(w), ctypes.byref(nl)))
        self.limb_bits, self.n_limbs = w.value, nl.value

    def __del__(self):
        release(self, "mi_pbs128_key_destroy")

    def _glwe(self):
        return (self.glwe_dimension + 1, self.polynomial_size)


def add_external_product_assign(out, key: LweBootstrapKey128, ggsw_index: int, glwe) -> None:
    """out += GGSW[ggsw_index] (.) glwe for every GLWE of the batch (add_external_product_assign_split)."""
    po, batch = _u128(out, "out", key._glwe())
    pg, b2 = _u128(glwe, "glwe", key._glwe())
    if b2 != batch:
        raise ValueError("assertion failed: out and glwe batch sizes differ")
    check(lib().mi_ext_product128_batch(key._h, ggsw_index, po, pg, batch, _stream(out)))


def cmux_assign(ct0, ct1, key: LweBootstrapKey128, ggsw_index: int) -> None:
    """ct1 -= ct0, then ct0 += GGSW[ggsw_index] (.) ct1 (cmux_split: ct1 is left holding the difference)."""
    p0, batch = _u128(ct0, "ct0", key._glwe())
    p1, b2 = _u128(ct1, "ct1", key._glwe())
    if b2 != batch:
        raise ValueError("assertion failed: ct0 and ct1 batch sizes differ")
    check(lib().mi_cmux128_batch(key._h, ggsw_index, p0, p1, batch, _stream(ct0)))


def _lwe_in(key, lwe_in, batch):
    size = key.input_lwe_dimension + 1
    if lwe_in.shape[-1] != size or lwe_in.numel() // size != batch:
        raise ValueError(f"assertion failed: lwe_in shape {tuple(lwe_in.shape)} != ({batch}, {size})")
    return _dev(lwe_in, "lwe_in")


def blind_rotate_assign(key: LweBootstrapKey128, acc, lwe_in, ms_mode: int = MS_STANDARD) -> None:
    """acc[b] /= X^ms(body), then the CMUX loop over lwe_in[b] (u64, native modulus), in place
    (blind_rotate_assign_split)."""
    pa, batch = _u128(acc, "acc", key._glwe())
    check(lib().mi_blind_rotate128_batch(key._h, pa, _lwe_in(key, lwe_in, batch), batch, ms_mode, _stream(acc)))


def programmable_bootstrap_f128_lwe_ciphertext(lwe_in, lwe_out, accumulator, key: LweBootstrapKey128,
                                               ms_mode: int = MS_STANDARD) -> None:
    """lwe_out[b] (k N + 1 u128) = PBS of lwe_in[b] (n_ggsw + 1 u64) through the one shared LUT GLWE
    ``accumulator`` ((k + 1, N, 2))."""
    po, batch = _u128(lwe_out, "lwe_out", (key.glwe_dimension * key.polynomial_size + 1,))
    pl, one = _u128(accumulator, "accumulator", key._glwe())
    if one != 1:
        raise ValueError("assertion failed: one accumulator is shared by the batch")
    check(lib().mi_pbs128_batch(key._h, po, _lwe_in(key, lwe_in, batch), pl, batch, ms_mode, _stream(lwe_out)))


def multi_bit_limb_plan(polynomial_size: int, glwe_dimension: int, base_log: int, level: int,
                        grouping_factor: int) -> tuple[int, int]:
    """(limb_bits, n_limbs) of the multi-bit limb split (``mi_pbs128_multi_bit_limb_plan``; needs no device): a column
    sums the 2^g GGSWs of a group, so limb_bits is the largest w with
    2^g (k + 1) level N 2^(base_log - 1) (2^w - 1) <= (p - 1) / 2, n_limbs = ceil(128 / w)."""
    w, nl = ctypes.c_int(), ctypes.c_int()
    check(lib().mi_pbs128_multi_bit_limb_plan(polynomial_size, glwe_dimension, base_log, level, grouping_factor,
                                              ctypes.byref(w), ctypes.byref(nl)))
    return w.value, nl.value


class LweMultiBitBootstrapKey128:
    """An ``LweMultiBitBootstrapKey<u128>`` prepared for the multi-bit 128-bit bootstrap (``mi_pbs128_multi_bit_key``).

    ``bsk``: device tensor (n_lwe / g, 2^g, level, k + 1, k + 1, N, 2) in the reference's standard-domain layout:
    group-major, GGSW ``idx`` of group i encrypting prod_m (s[i g + m] XOR NOT bit_m(idx)), each GGSW as
    ``LweBootstrapKey128`` takes it.  A private prepared copy is made; ``bsk`` may be released afterwards."""

    def __init__(self, bsk, base_log: int, level: int, grouping_factor: int, plan: Plan | None = None):
        if (bsk.dim() != 7 or bsk.shape[1] != 1 << grouping_factor or bsk.shape[2] != level
                or bsk.shape[3] != bsk.shape[4] or bsk.shape[6] != 2):
            raise ValueError(f"assertion failed: bsk shape {tuple(bsk.shape)} != "
                             f"(n_lwe / g, {1 << grouping_factor}, {level}, k + 1, k + 1, N, 2)")
        self.grouping_factor = grouping_factor
        self.input_lwe_dimension = int(bsk.shape[0]) * grouping_factor
        self.glwe_dimension = int(bsk.shape[3]) - 1
        self.polynomial_size = int(bsk.shape[5])
        self.decomposition_base_log, self.decomposition_level_count = base_log, level
        self.device = bsk.device
        # kept alive with the key; by default the process-wide plan of Ntt64::new
        self.plan = plan if plan is not None else Plan.cached(self.polynomial_size, SOLINAS_P, bsk.device.index or 0)
        h = ctypes.c_void_p()
        check(lib().mi_pbs128_multi_bit_key_create(self.plan.handle, _dev(bsk, "bsk"), self.input_lwe_dimension,
                                                   self.glwe_dimension, self.polynomial_size, base_log, level,
                                                   grouping_factor, _stream(bsk), ctypes.byref(h)))
        self._h = h
        w, nl = ctypes.c_int(), ctypes.c_int()
        check(lib().mi_pbs128_multi_bit_key_info(h, None, None, None, None, None, None, ctypes.byref(w),
                                                 ctypes.byref(nl)))
        self.limb_bits, self.n_limbs = w.value, nl.value

    def __del__(self):
        release(self, "mi_pbs128_multi_bit_key_destroy")

    def _glwe(self):
        return (self.glwe_dimension + 1, self.polynomial_size)


def multi_bit_blind_rotate_assign(key: LweMultiBitBootstrapKey128, acc, lwe_in) -> None:
    """acc[b] /= X^ms(body), then the n_lwe / g steps acc <- bundle (.) acc over lwe_in[b] (u64, native modulus), in
    place (multi_bit_f128_deterministic_blind_rotate_assign)."""
    pa, batch = _u128(acc, "acc", key._glwe())
    check(lib().mi_pbs128_multi_bit_blind_rotate_batch(key._h, pa, _lwe_in(key, lwe_in, batch), batch, _stream(acc)))


def multi_bit_programmable_bootstrap_f128_lwe_ciphertext(lwe_in, lwe_out, accumulator,
                                                         key: LweMultiBitBootstrapKey128) -> None:
    """lwe_out[b] (k N + 1 u128) = the multi-bit PBS of lwe_in[b] (n_lwe + 1 u64) through the one shared LUT GLWE
    ``accumulator`` ((k + 1, N, 2))."""
    po, batch = _u128(lwe_out, "lwe_out", (key.glwe_dimension * key.polynomial_size + 1,))
    pl, one = _u128(accumulator, "accumulator", key._glwe())
    if one != 1:
        raise ValueError("assertion failed: one accumulator is shared by the batch")
    check(lib().mi_pbs128_multi_bit_batch(key._h, po, _lwe_in(key, lwe_in, batch), pl, batch, _stream(lwe_out)))


__all__ = ["LweBootstrapKey128", "limb_plan", "add_external_product_assign", "cmux_assign", "blind_rotate_assign",
           "programmable_bootstrap_f128_lwe_ciphertext", "LweMultiBitBootstrapKey128", "multi_bit_limb_plan",
           "multi_bit_blind_rotate_assign", "multi_bit_programmable_bootstrap_f128_lwe_ciphertext",
           "MS_STANDARD", "MS_CENTERED", "MS_PRE_SWITCHED"]
