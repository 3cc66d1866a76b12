"""Host-side mirror of the core_crypto LWE packing keyswitch and GLWE compression over the C ABI.

Reference (paths relative to tfhe/src/core_crypto):

* ``LwePackingKeyswitchKey``       entities/lwe_packing_keyswitch_key.rs (in_dim blocks x level GLWEs of (k + 1) N)
* ``keyswitch_lwe_ciphertext_into_glwe_ciphertext``               algorithms/lwe_packing_keyswitch.rs:102-187
* ``keyswitch_lwe_ciphertext_list_and_pack_in_glwe_ciphertext``   algorithms/lwe_packing_keyswitch.rs:296-379
* ``CompressedModulusSwitchedGlweCiphertext`` (``compress`` / ``extract``)
  entities/compressed_modulus_switched_glwe_ciphertext.rs:169-256 over entities/packed_integers.rs:39-222

The reference packs one list into one GLWE per call; here leading batch dimensions are allowed (one GEMM on the int8
matrix cores for every ciphertext of the call, csrc/keyswitch.hip, then the rotate-and-sum pass of
csrc/packing_keyswitch.hip).  Shape mismatches raise ``ValueError`` where the reference panics on ``assert!``.
"""
from __future__ import annotations

import ctypes

from ._lib import check, lib, release
from .ntt64_pbs import _dev, _stream


class LwePackingKeyswitchKey:
    """A device packing keyswitch key prepared for the two keyswitches below (``mi_lwe_pksk``).

    ``pksk``: device tensor (in_dim, level, k + 1, N) of u64 in the reference layout (levels as
    generate_lwe_packing_keyswitch_key stores them, lwe_packing_keyswitch_key_generation.rs:129-156).  A private
    matrix-core copy is made; ``pksk`` may be released afterwards."""

    def __init__(self, pksk, base_log: int, level: int):
        if pksk.dim() != 4 or pksk.shape[1] != level or pksk.shape[2] < 2:
            raise ValueError(f"assertion failed: pksk shape {tuple(pksk.shape)} != (in_dim, {level}, k + 1, N)")
        self.input_key_lwe_dimension = int(pksk.shape[0])
        self.output_key_glwe_dimension = int(pksk.shape[2]) - 1
        self.output_key_polynomial_size = int(pksk.shape[3])
        self.decomposition_base_log, self.decomposition_level_count = base_log, level
        self.device = pksk.device
        h = ctypes.c_void_p()
        check(lib().mi_lwe_pksk_create(_dev(pksk, "pksk"), self.input_key_lwe_dimension,
                                       self.output_key_glwe_dimension, self.output_key_polynomial_size, base_log,
                                       level, pksk.device.index or 0, _stream(pksk), ctypes.byref(h)))
        self._h = h

    def __del__(self):
        release(self, "mi_lwe_pksk_destroy")


def _check_glwe(k: LwePackingKeyswitchKey, glwe):
    kp1, n = k.output_key_glwe_dimension + 1, k.output_key_polynomial_size
    if glwe.dim() < 2 or glwe.shape[-2] != kp1:
        raise ValueError(f"assertion failed: Mismatched output GlweDimension {glwe.shape[-2] - 1 if glwe.dim() >= 2 else None}"
                         f" != {kp1 - 1}")
    if glwe.shape[-1] != n:
        raise ValueError(f"assertion failed: Mismatched output PolynomialSize {glwe.shape[-1]} != {n}")
    return glwe.numel() // (kp1 * n)


def _check_lwe(k: LwePackingKeyswitchKey, lwe):
    if lwe.dim() < 1 or lwe.shape[-1] != k.input_key_lwe_dimension + 1:
        raise ValueError(f"assertion failed: Mismatched input LweDimension {lwe.shape[-1] - 1 if lwe.dim() else None} "
                         f"!= {k.input_key_lwe_dimension}")


def keyswitch_lwe_ciphertext_into_glwe_ciphertext(lwe_pksk: LwePackingKeyswitchKey, input_lwe_ciphertext,
                                                  output_glwe_ciphertext) -> None:
    """output[b] = the GLWE whose body's constant coefficient encrypts input[b] (lwe_packing_keyswitch.rs:102-187):
    input (..., in_dim + 1) -> output (..., k + 1, N), one GLWE per ciphertext."""
    k = lwe_pksk
    _check_lwe(k, input_lwe_ciphertext)
    n_glwe = _check_glwe(k, output_glwe_ciphertext)
    batch = input_lwe_ciphertext.numel() // (k.input_key_lwe_dimension + 1)
    if n_glwe != batch:
        raise ValueError("assertion failed: input and output batch sizes differ")
    check(lib().mi_lwe_packing_keyswitch_batch(k._h, _dev(output_glwe_ciphertext, "output_glwe_ciphertext"),
                                               _dev(input_lwe_ciphertext, "input_lwe_ciphertext"), batch, 1,
                                               _stream(output_glwe_ciphertext)))


def keyswitch_lwe_ciphertext_list_and_pack_in_glwe_ciphertext(lwe_pksk: LwePackingKeyswitchKey,
                                                              input_lwe_ciphertext, output_glwe_ciphertext,
                                                              lwe_per_glwe: int | None = None) -> None:
    """Packs a list of LWE ciphertexts (n_lwe, in_dim + 1) into GLWEs (lwe_packing_keyswitch.rs:296-379): ciphertext
    d of a GLWE lands on coefficient d of its body polynomial.  Without ``lwe_per_glwe`` the whole list goes into the
    one GLWE ``output`` (k + 1, N), as in the reference; with it, ``output`` (ceil(n_lwe / lwe_per_glwe), k + 1, N)
    gets one GLWE per ``lwe_per_glwe`` ciphertexts, the last one holding the remainder (shortint's
    ``chunks(lwe_per_glwe)``)."""
    k = lwe_pksk
    _check_lwe(k, input_lwe_ciphertext)
    n_glwe = _check_glwe(k, output_glwe_ciphertext)
    n_lwe = input_lwe_ciphertext.numel() // (k.input_key_lwe_dimension + 1)
    per = n_lwe if lwe_per_glwe is None else int(lwe_per_glwe)
    if lwe_per_glwe is not None and per < 1:
        raise ValueError("assertion failed: lwe_per_glwe must be >= 1")
    if per > k.output_key_polynomial_size:
        raise ValueError(f"assertion failed: input lwe_ciphertext_count {per} > output polynomial_size "
                         f"{k.output_key_polynomial_size}")
    want = 1 if lwe_per_glwe is None else (n_lwe + per - 1) // per
    if n_glwe != want:
        raise ValueError(f"assertion failed: output holds {n_glwe} GLWE ciphertexts, the list packs into {want}")
    if n_lwe == 0:  # the reference zeroes the output of an empty list
        output_glwe_ciphertext.zero_()
        return
    check(lib().mi_lwe_packing_keyswitch_batch(k._h, _dev(output_glwe_ciphertext, "output_glwe_ciphertext"),
                                               _dev(input_lwe_ciphertext, "input_lwe_ciphertext"), n_lwe, per,
                                               _stream(output_glwe_ciphertext)))


class CompressedModulusSwitchedGlweCiphertext:
    """A batch of modulus-switched, bit-packed GLWE ciphertexts
    (compressed_modulus_switched_glwe_ciphertext.rs:100-257): ``packed_integers`` is a device tensor
    (..., words) of u64, ``words = ceil((k N + bodies_count) log_modulus / 64)`` per GLWE."""

    def __init__(self, packed_integers, glwe_dimension: int, polynomial_size: int, bodies_count: int,
                 log_modulus: int):
        self.packed_integers = packed_integers
        self.glwe_dimension, self.polynomial_size = glwe_dimension, polynomial_size
        self.bodies_count, self.log_modulus = bodies_count, log_modulus

    @staticmethod
    def packed_words(glwe_dimension: int, polynomial_size: int, bodies_count: int, log_modulus: int) -> int:
        _check_compress_params(polynomial_size, bodies_count, log_modulus)
        out = ctypes.c_size_t()
        check(lib().mi_glwe_compressed_words(polynomial_size, glwe_dimension, bodies_count, log_modulus,
                                             ctypes.byref(out)))
        return out.value

    @classmethod
    def compress(cls, ct, log_modulus: int, bodies_count: int):
        """``compress`` (:169-220) of every GLWE of ``ct`` (..., k + 1, N), native modulus."""
        import torch

        if ct.dim() < 2 or ct.shape[-2] < 2:
            raise ValueError(f"assertion failed: glwe shape {tuple(ct.shape)} != (..., k + 1, N)")
        kp1, n = int(ct.shape[-2]), int(ct.shape[-1])
        words = cls.packed_words(kp1 - 1, n, bodies_count, log_modulus)
        batch = ct.numel() // (kp1 * n)
        packed = torch.empty(tuple(ct.shape[:-2]) + (words,), dtype=ct.dtype, device=ct.device)
        check(lib().mi_glwe_compress_batch(_dev(packed, "packed"), _dev(ct, "ct"), n, kp1 - 1, bodies_count,
                                           log_modulus, batch, ct.device.index or 0, _stream(ct)))
        return cls(packed, kp1 - 1, n, bodies_count, log_modulus)

    def extract(self, out=None):
        """``extract`` (:226-256): the GLWEs (..., k + 1, N) at the native modulus, the body polynomial zero past
        ``bodies_count``."""
        import torch

        p = self.packed_integers
        k, n = self.glwe_dimension, self.polynomial_size
        words = self.packed_words(k, n, self.bodies_count, self.log_modulus)
        if p.dim() < 1 or p.shape[-1] != words:
            raise ValueError(f"assertion failed: Mismatch between actual(={p.shape[-1] if p.dim() else None}) and "
                             f"maximal(={words}) CompressedModulusSwitchedGlweCiphertext packed_coeffs size")
        shape = tuple(p.shape[:-1]) + (k + 1, n)
        if out is None:
            out = torch.empty(shape, dtype=p.dtype, device=p.device)
        elif tuple(out.shape) != shape:
            raise ValueError(f"assertion failed: out shape {tuple(out.shape)} != {shape}")
        batch = p.numel() // words
        check(lib().mi_glwe_extract_batch(_dev(out, "out"), _dev(p, "packed_integers"), n, k, self.bodies_count,
                                          self.log_modulus, batch, p.device.index or 0, _stream(p)))
        return out


def _check_compress_params(polynomial_size: int, bodies_count: int, log_modulus: int) -> None:
    if not 0 <= bodies_count <= polynomial_size:
        raise ValueError(f"assertion failed: Number of stored bodies (asked {bodies_count}) cannot be bigger than "
                         f"polynomial_size ={polynomial_size}")
    if not 1 <= log_modulus <= 64:
        raise ValueError(f"assertion failed: The log_modulus (={log_modulus}) for modulus switch compression must be "
                         "in [1, 64]")


__all__ = ["LwePackingKeyswitchKey", "keyswitch_lwe_ciphertext_into_glwe_ciphertext",
           "keyswitch_lwe_ciphertext_list_and_pack_in_glwe_ciphertext", "CompressedModulusSwitchedGlweCiphertext"]
