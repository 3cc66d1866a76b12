"""Host-side mirror of shortint's server key over the C ABI (``mi_shortint_*``): lookup tables and the KS -> MS -> PBS
atomic pattern, batched.

Reference (paths relative to tfhe/src/shortint):

* ``fill_accumulator_with_encoding``               engine/mod.rs:80-141
* ``generate_lookup_table``                         server_key/mod.rs:805 (:1649)
* ``generate_lookup_table_bivariate``               server_key/bivariate_pbs.rs:57-115
* ``apply_lookup_table[_assign]``                   server_key/mod.rs:935-960 (apply_programmable_bootstrap :1542)
* ``unchecked_apply_lookup_table_bivariate``        server_key/bivariate_pbs.rs:141-167
* ``message_extract`` / ``carry_extract``           server_key/mod.rs:1189 / :1111
* ``unchecked_add`` / ``unchecked_scalar_add`` / ``unchecked_scalar_mul``   server_key/add.rs, scalar_add.rs, scalar_mul.rs

A ciphertext batch is a device tensor (..., k N + 1) of u64 under the big key (the KS-PBS order); the reference's
degree and noise bookkeeping lives one layer up (``integer.RadixCiphertext``), every operation here is its unchecked
form.  A lookup table is a device tensor (k + 1, N), a list of them (n_lut, k + 1, N) with one int32 index per item.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import lwe_linear_algebra as LA
from ._lib import check, lib, release
from .fft64 import FourierLweBootstrapKey, FourierLweMultiBitBootstrapKey
from .ntt64_pbs import MS_CENTERED, MS_STANDARD, NttBootstrapKey, _dev, _index, _stream

PBS_NTT64, PBS_FFT64, PBS_FFT64_MULTI_BIT = 0, 1, 2


def lut_fill(polynomial_size: int, k: int, message_modulus: int, carry_modulus: int, table) -> np.ndarray:
    """``mi_shortint_lut_fill``: the accumulator (k + 1, N) of the table's m c values, as a host array."""
    table = np.ascontiguousarray(np.asarray(table, dtype=np.uint64))
    out = np.zeros((k + 1, polynomial_size), np.uint64)
    p64 = ctypes.POINTER(ctypes.c_uint64)
    check(lib().mi_shortint_lut_fill(out.ctypes.data_as(p64), polynomial_size, k, message_modulus, carry_modulus,
                                     table.ctypes.data_as(p64), table.size))
    return out


class ShortintServerKey:
    """``shortint::ServerKey`` in the KS-PBS order (``mi_shortint_key``): a keyswitch key k N -> n, a bootstrap key
    (``NttBootstrapKey`` of the BNF variant, ``FourierLweBootstrapKey`` or ``FourierLweMultiBitBootstrapKey``), an
    optional ``ModulusSwitchNoiseReductionKey`` (the drift technique) and the modulus switch of the bootstrap.  The
    handles are borrowed: this object keeps the Python keys alive."""

    def __init__(self, ksk, bootstrapping_key, message_modulus: int, carry_modulus: int,
                 modulus_switch_noise_reduction_key=None, ms_mode: int = MS_STANDARD):
        b = bootstrapping_key
        if isinstance(b, NttBootstrapKey):
            self.pbs_engine = PBS_NTT64
        elif isinstance(b, FourierLweBootstrapKey):
            self.pbs_engine = PBS_FFT64
        elif isinstance(b, FourierLweMultiBitBootstrapKey):
            self.pbs_engine = PBS_FFT64_MULTI_BIT
        else:
            raise TypeError("bootstrapping_key must be an NttBootstrapKey, a FourierLweBootstrapKey or a "
                            "FourierLweMultiBitBootstrapKey")
        self.key_switching_key, self.bootstrapping_key = ksk, b
        self.modulus_switch_noise_reduction_key = modulus_switch_noise_reduction_key
        self.message_modulus, self.carry_modulus, self.ms_mode = int(message_modulus), int(carry_modulus), ms_mode
        self.glwe_dimension, self.polynomial_size = b.glwe_dimension, b.polynomial_size
        self.lwe_size = b.glwe_dimension * b.polynomial_size + 1
        self.device = ksk.device
        msk = modulus_switch_noise_reduction_key
        h = ctypes.c_void_p()
        check(lib().mi_shortint_key_create(ksk._h, self.pbs_engine, b._h, msk._h if msk is not None else None, ms_mode,
                                           self.message_modulus, self.carry_modulus, ctypes.byref(h)))
        self._h = h
        self.max_degree = self.message_modulus * self.carry_modulus - 1
        self.delta = (1 << 63) // (self.message_modulus * self.carry_modulus)
        self._cache = {}

    def __del__(self):
        release(self, "mi_shortint_key_destroy")

    # ---- lookup tables ----
    def _table(self, table):
        import torch

        acc = lut_fill(self.polynomial_size, self.glwe_dimension, self.message_modulus, self.carry_modulus, table)
        return torch.from_numpy(acc.view(np.int64)).to(self.device)

    def generate_lookup_table(self, f):
        """The accumulator of ``f`` over [0, m c) (server_key/mod.rs:805)."""
        sup = self.message_modulus * self.carry_modulus
        return self._table([int(f(x)) % (1 << 64) for x in range(sup)])

    def generate_lookup_table_bivariate(self, f):
        """The accumulator of ``f(lhs, rhs)`` on the packed input ``m lhs + rhs`` (bivariate_pbs.rs:57-115)."""
        m = self.message_modulus
        return self.generate_lookup_table(lambda x: f((x // m) % m, (x % m) % m))

    def _cached_lut(self, name, f, bivariate=False):
        if name not in self._cache:
            self._cache[name] = (self.generate_lookup_table_bivariate if bivariate else self.generate_lookup_table)(f)
        return self._cache[name]

    # ---- the atomic pattern ----
    def apply_lookup_table_batch(self, output, input, lut_list, lut_index=None, in_index=None) -> None:
        """``mi_shortint_apply_lut_batch`` itself: input (n_in, k N + 1) -> output (n_items, k N + 1); ``lut_list``
        (n_lut, k + 1, N); ``lut_index`` / ``in_index`` int32 device tensors of n_items entries or None (item j: table
        j / input j).  An item whose input or table index is out of range keeps its output row."""
        size = self.lwe_size
        glwe = (self.glwe_dimension + 1, self.polynomial_size)
        if input.dim() != 2 or output.dim() != 2 or input.shape[1] != size or output.shape[1] != size:
            raise ValueError(f"assertion failed: ciphertext shapes {tuple(input.shape)} -> {tuple(output.shape)} != "
                             f"(batch, {size})")
        if lut_list.dim() != 3 or tuple(lut_list.shape[1:]) != glwe:
            raise ValueError(f"assertion failed: lookup table list shape {tuple(lut_list.shape)} != (n_lut, *{glwe})")
        n_in, n_items = int(input.shape[0]), int(output.shape[0])
        ii = None if in_index is None else _index(in_index, n_items, output.device, "in_index")
        li = None if lut_index is None else _index(lut_index, n_items, output.device, "lut_index")
        check(lib().mi_shortint_apply_lut_batch(self._h, _dev(output, "output"), _dev(input, "input"), n_in, ii,
                                                _dev(lut_list, "lut_list"), li, int(lut_list.shape[0]), n_items,
                                                _stream(output)))

    def _apply(self, output, ct, lut, lut_index):
        import torch

        flat_in, flat_out = ct.reshape(-1, self.lwe_size), output.reshape(-1, self.lwe_size)
        if lut.dim() == 2:
            if lut_index is not None:
                raise ValueError("assertion failed: lut_index needs a list of lookup tables")
            lut = lut.unsqueeze(0)
            lut_index = torch.zeros(flat_in.shape[0], dtype=torch.int32, device=ct.device)
        elif lut_index is None:
            raise ValueError("assertion failed: a list of lookup tables needs lut_index, one entry per ciphertext")
        self.apply_lookup_table_batch(flat_out, flat_in, lut, lut_index)

    def apply_lookup_table(self, ct, lut, lut_index=None):
        """A new batch: every ciphertext through ``lut``, or through ``lut[lut_index[b]]`` (a table per item)."""
        import torch

        if not ct.is_contiguous():
            raise ValueError("ct must be contiguous")
        out = torch.empty_like(ct)
        self._apply(out, ct, lut, lut_index)
        return out

    def apply_lookup_table_assign(self, ct, lut, lut_index=None) -> None:
        if not ct.is_contiguous():
            raise ValueError("ct must be contiguous")
        self._apply(ct, ct, lut, lut_index)

    def unchecked_apply_lookup_table_bivariate(self, ct_left, ct_right, lut):
        """``lut`` at ``m ct_left + ct_right`` (bivariate_pbs.rs:141-167): one packing call, one atomic pattern."""
        import torch

        packed = torch.empty_like(ct_left)
        LA._combine(packed, [ct_left, ct_right], [self.message_modulus, 1])
        self._apply(packed, packed, lut, None)
        return packed

    def message_extract(self, ct):
        m = self.message_modulus
        return self.apply_lookup_table(ct, self._cached_lut("message", lambda x: x % m))

    def carry_extract(self, ct):
        m = self.message_modulus
        return self.apply_lookup_table(ct, self._cached_lut("carry", lambda x: x // m))

    # ---- leveled operations ----
    def unchecked_add(self, ct_left, ct_right):
        import torch

        out = torch.empty_like(ct_left)
        LA.lwe_ciphertext_add(out, ct_left, ct_right)
        return out

    def unchecked_scalar_add(self, ct, scalar):
        """ct + scalar (an int, or one per ciphertext): the plaintext scalar * 2^63 / (m c) on the body."""
        import torch

        out = ct.clone()
        if isinstance(scalar, int):
            pt = (scalar * self.delta) % (1 << 64)
        else:
            pt = scalar.to(torch.int64) * self.delta
        LA.lwe_ciphertext_plaintext_add_assign(out, pt)
        return out

    def unchecked_scalar_mul(self, ct, scalar):
        import torch

        out = torch.empty_like(ct)
        LA.lwe_ciphertext_cleartext_mul(out, ct, scalar)
        return out


__all__ = ["PBS_NTT64", "PBS_FFT64", "PBS_FFT64_MULTI_BIT", "MS_STANDARD", "MS_CENTERED", "lut_fill",
           "ShortintServerKey"]
