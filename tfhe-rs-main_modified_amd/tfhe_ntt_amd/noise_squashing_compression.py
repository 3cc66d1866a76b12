"""Host-side mirror of the compression of noise-squashed ciphertexts over the C ABI: the LWE packing keyswitch and the
GLWE modulus-switch compression at Scalar = u128 (the u128 twin of ``lwe_packing_keyswitch.py``).

Reference (paths relative to tfhe/src):

* ``LwePackingKeyswitchKey128``     core_crypto/entities/lwe_packing_keyswitch_key.rs at Scalar = u128
* ``keyswitch_lwe_ciphertext_list_and_pack_in_glwe_ciphertext``   core_crypto/algorithms/lwe_packing_keyswitch.rs:296-379
  (calling :102-187)
* ``CompressedModulusSwitchedGlweCiphertext128`` (``compress`` / ``extract``)
  core_crypto/entities/compressed_modulus_switched_glwe_ciphertext.rs:169-256 over entities/packed_integers.rs:39-222
* ``compress_noise_squashed_ciphertexts_into_list``   shortint/list_compression/noise_squashing_compression.rs:23-118

A u128 tensor is int64 (or uint64) storage with a trailing dimension of 2, the little-endian words (lo, hi), as in
``pbs128.py``.  The GEMM mod 2^128 runs on the int8 matrix cores (csrc/packing_keyswitch128.hip).  Shape mismatches
raise ``ValueError`` where the reference panics on ``assert!``.
"""
from __future__ import annotations

import ctypes

from ._lib import check, lib, release
from .ntt64_pbs import _dev, _stream


class LwePackingKeyswitchKey128:
    """A device ``LwePackingKeyswitchKey<u128>`` prepared for the packing keyswitch (``mi_lwe_pksk128``).

    ``pksk``: device tensor (in_dim, level, k + 1, N, 2) in the reference layout (levels as
    generate_lwe_packing_keyswitch_key stores them, lwe_packing_keyswitch_key_generation.rs:129-156).  A private
    matrix-core copy of the same size is made; ``pksk`` may be released afterwards."""

    def __init__(self, pksk, base_log: int, level: int):
        if pksk.dim() != 5 or pksk.shape[1] != level or pksk.shape[2] < 2 or pksk.shape[4] != 2:
            raise ValueError(f"assertion failed: pksk shape {tuple(pksk.shape)} != (in_dim, {level}, k + 1, N, 2)")
        self.input_key_lwe_dimension = int(pksk.shape[0])
        self.output_key_glwe_dimension = int(pksk.shape[2]) - 1
        self.output_key_polynomial_size = int(pksk.shape[3])
        self.decomposition_base_log, self.decomposition_level_count = base_log, level
        self.device = pksk.device
        h = ctypes.c_void_p()
        check(lib().mi_lwe_pksk128_create(_dev(pksk, "pksk"), self.input_key_lwe_dimension,
                                          self.output_key_glwe_dimension, self.output_key_polynomial_size, base_log,
                                          level, pksk.device.index or 0, _stream(pksk), ctypes.byref(h)))
        self._h = h

    def __del__(self):
        release(self, "mi_lwe_pksk128_destroy")


def _check_glwe(k: LwePackingKeyswitchKey128, glwe):
    kp1, n = k.output_key_glwe_dimension + 1, k.output_key_polynomial_size
    if glwe.dim() < 3 or glwe.shape[-1] != 2 or glwe.shape[-3] != kp1:
        raise ValueError(f"assertion failed: Mismatched output GlweDimension: shape {tuple(glwe.shape)} != "
                         f"(..., {kp1}, {n}, 2)")
    if glwe.shape[-2] != n:
        raise ValueError(f"assertion failed: Mismatched output PolynomialSize {glwe.shape[-2]} != {n}")
    return glwe.numel() // (kp1 * n * 2)


def _check_lwe(k: LwePackingKeyswitchKey128, lwe):
    size = k.input_key_lwe_dimension + 1
    if lwe.dim() < 2 or lwe.shape[-1] != 2 or lwe.shape[-2] != size:
        raise ValueError(f"assertion failed: Mismatched input LweDimension: shape {tuple(lwe.shape)} != "
                         f"(..., {size}, 2)")
    return lwe.numel() // (size * 2)


def keyswitch_lwe_ciphertext_into_glwe_ciphertext(lwe_pksk: LwePackingKeyswitchKey128, input_lwe_ciphertext,
                                                  output_glwe_ciphertext) -> None:
    """output[b] = the GLWE whose body's constant coefficient encrypts input[b] (lwe_packing_keyswitch.rs:102-187):
    input (..., in_dim + 1, 2) -> output (..., k + 1, N, 2), one GLWE per ciphertext."""
    k = lwe_pksk
    batch = _check_lwe(k, input_lwe_ciphertext)
    if _check_glwe(k, output_glwe_ciphertext) != batch:
        raise ValueError("assertion failed: input and output batch sizes differ")
    check(lib().mi_lwe_packing_keyswitch128_batch(k._h, _dev(output_glwe_ciphertext, "output_glwe_ciphertext"),
                                                  _dev(input_lwe_ciphertext, "input_lwe_ciphertext"), batch, 1,
                                                  _stream(output_glwe_ciphertext)))


def keyswitch_lwe_ciphertext_list_and_pack_in_glwe_ciphertext(lwe_pksk: LwePackingKeyswitchKey128,
                                                              input_lwe_ciphertext, output_glwe_ciphertext,
                                                              lwe_per_glwe: int | None = None) -> None:
    """Packs a list of u128 LWE ciphertexts (n_lwe, in_dim + 1, 2) into GLWEs (lwe_packing_keyswitch.rs:296-379):
    ciphertext d of a GLWE lands on coefficient d of its body polynomial.  Without ``lwe_per_glwe`` the whole list
    goes into the one GLWE ``output`` (k + 1, N, 2), as in the reference; with it, ``output``
    (ceil(n_lwe / lwe_per_glwe), k + 1, N, 2) gets one GLWE per ``lwe_per_glwe`` ciphertexts, the last one holding the
    remainder (shortint's ``par_chunks(lwe_per_glwe)``)."""
    k = lwe_pksk
    n_lwe = _check_lwe(k, input_lwe_ciphertext)
    n_glwe = _check_glwe(k, output_glwe_ciphertext)
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
    check(lib().mi_lwe_packing_keyswitch128_batch(k._h, _dev(output_glwe_ciphertext, "output_glwe_ciphertext"),
                                                  _dev(input_lwe_ciphertext, "input_lwe_ciphertext"), n_lwe, per,
                                                  _stream(output_glwe_ciphertext)))


class CompressedModulusSwitchedGlweCiphertext128:
    """A batch of modulus-switched, bit-packed u128 GLWE ciphertexts
    (compressed_modulus_switched_glwe_ciphertext.rs:100-257): ``packed_integers`` is a device tensor
    (..., words, 2), ``words = ceil((k N + bodies_count) log_modulus / 128)`` u128 per GLWE."""

    def __init__(self, packed_integers, glwe_dimension: int, polynomial_size: int, bodies_count: int,
                 log_modulus: int):
        self.packed_integers = packed_integers
        self.glwe_dimension, self.polynomial_size = glwe_dimension, polynomial_size
        self.bodies_count, self.log_modulus = bodies_count, log_modulus

    @staticmethod
    def packed_words(glwe_dimension: int, polynomial_size: int, bodies_count: int, log_modulus: int) -> int:
        _check_compress_params(polynomial_size, bodies_count, log_modulus)
        out = ctypes.c_size_t()
        check(lib().mi_glwe_compressed_words128(polynomial_size, glwe_dimension, bodies_count, log_modulus,
                                                ctypes.byref(out)))
        return out.value

    @classmethod
    def compress(cls, ct, log_modulus: int, bodies_count: int):
        """``compress`` (:169-220) of every GLWE of ``ct`` (..., k + 1, N, 2), native u128 modulus."""
        import torch

        if ct.dim() < 3 or ct.shape[-3] < 2 or ct.shape[-1] != 2:
            raise ValueError(f"assertion failed: glwe shape {tuple(ct.shape)} != (..., k + 1, N, 2)")
        kp1, n = int(ct.shape[-3]), int(ct.shape[-2])
        words = cls.packed_words(kp1 - 1, n, bodies_count, log_modulus)
        batch = ct.numel() // (kp1 * n * 2)
        packed = torch.empty(tuple(ct.shape[:-3]) + (words, 2), dtype=ct.dtype, device=ct.device)
        check(lib().mi_glwe_compress128_batch(_dev(packed, "packed"), _dev(ct, "ct"), n, kp1 - 1, bodies_count,
                                              log_modulus, batch, ct.device.index or 0, _stream(ct)))
        return cls(packed, kp1 - 1, n, bodies_count, log_modulus)

    def extract(self, out=None):
        """``extract`` (:226-256): the GLWEs (..., k + 1, N, 2) at the native modulus, the body polynomial zero past
        ``bodies_count``."""
        import torch

        p = self.packed_integers
        k, n = self.glwe_dimension, self.polynomial_size
        words = self.packed_words(k, n, self.bodies_count, self.log_modulus)
        if p.dim() < 2 or p.shape[-1] != 2 or p.shape[-2] != words:
            raise ValueError(f"assertion failed: Mismatch between actual(={tuple(p.shape)}) and maximal(={words}) "
                             "CompressedModulusSwitchedGlweCiphertext packed_coeffs size")
        shape = tuple(p.shape[:-2]) + (k + 1, n, 2)
        if out is None:
            out = torch.empty(shape, dtype=p.dtype, device=p.device)
        elif tuple(out.shape) != shape:
            raise ValueError(f"assertion failed: out shape {tuple(out.shape)} != {shape}")
        batch = p.numel() // (words * 2) if words else 0
        check(lib().mi_glwe_extract128_batch(_dev(out, "out"), _dev(p, "packed_integers"), n, k, self.bodies_count,
                                             self.log_modulus, batch, p.device.index or 0, _stream(p)))
        return out


def _check_compress_params(polynomial_size: int, bodies_count: int, log_modulus: int) -> None:
    if not 0 <= bodies_count <= polynomial_size:
        raise ValueError(f"assertion failed: Number of stored bodies (asked {bodies_count}) cannot be bigger than "
                         f"polynomial_size ={polynomial_size}")
    if not 1 <= log_modulus <= 128:
        raise ValueError(f"assertion failed: The log_modulus (={log_modulus}) for modulus switch compression must be "
                         "in [1, 128]")


def compress_noise_squashed_ciphertexts_into_list(lwe_pksk: LwePackingKeyswitchKey128, ciphertexts, lwe_per_glwe: int,
                                                  log_modulus: int = 128):
    """``compress_noise_squashed_ciphertexts_into_list`` (noise_squashing_compression.rs:23-118): ``ciphertexts``
    (n_lwe, in_dim + 1, 2) are packed in chunks of ``lwe_per_glwe`` and every GLWE is compressed with the number of
    bodies its chunk holds, ``log_modulus`` being the ciphertext modulus' (128 for the native one).  Returns the list
    of compressed batches in order: the full chunks as one ``CompressedModulusSwitchedGlweCiphertext128`` of
    ``lwe_per_glwe`` bodies each, then the remainder chunk (fewer bodies, fewer packed words) as a second one; an
    empty input gives an empty list."""
    import torch

    k = lwe_pksk
    n_lwe = _check_lwe(k, ciphertexts)
    if not 1 <= lwe_per_glwe <= k.output_key_polynomial_size:
        raise ValueError(f"assertion failed: Cannot pack more than polynomial_size(={k.output_key_polynomial_size}) "
                         f"elements per glwe, {lwe_per_glwe} requested")
    if n_lwe == 0:
        return []
    n_glwe = (n_lwe + lwe_per_glwe - 1) // lwe_per_glwe
    glwe = torch.empty((n_glwe, k.output_key_glwe_dimension + 1, k.output_key_polynomial_size, 2),
                       dtype=ciphertexts.dtype, device=ciphertexts.device)
    keyswitch_lwe_ciphertext_list_and_pack_in_glwe_ciphertext(k, ciphertexts, glwe, lwe_per_glwe)
    full, rest = divmod(n_lwe, lwe_per_glwe)
    C = CompressedModulusSwitchedGlweCiphertext128
    out = []
    if full:
        out.append(C.compress(glwe[:full], log_modulus, lwe_per_glwe))
    if rest:
        out.append(C.compress(glwe[full:], log_modulus, rest))
    return out


__all__ = ["LwePackingKeyswitchKey128", "keyswitch_lwe_ciphertext_into_glwe_ciphertext",
           "keyswitch_lwe_ciphertext_list_and_pack_in_glwe_ciphertext", "CompressedModulusSwitchedGlweCiphertext128",
           "compress_noise_squashed_ciphertexts_into_list"]
