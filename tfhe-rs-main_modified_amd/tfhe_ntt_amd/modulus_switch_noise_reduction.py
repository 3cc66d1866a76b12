"""Host-side mirror of the drift-technique modulus switch noise reduction over the C ABI (``mi_ms_noise_*``,
``mi_lwe_ms_noise_*``).

Reference (paths relative to the reference's tfhe/src):

* ``ModulusSwitchNoiseReductionKey``  shortint/server_key/modulus_switch_noise_reduction.rs:35-119
* ``measure_modulus_switch_noise_estimation_for_binary_key``, ``choose_candidate_to_improve_modulus_switch_noise_for_
  binary_key``, ``improve_lwe_ciphertext_modulus_switch_noise_for_binary_key``
  core_crypto/algorithms/modulus_switch_noise_reduction.rs:71-242

The reference handles one ciphertext per call; here a leading batch dimension is allowed (one launch, one wave per
ciphertext, csrc/ms_noise_reduction.hip).  The measures, the chosen candidates and the outputs are the reference's
bit for bit.  Shape mismatches raise ``ValueError`` carrying the reference's assert text.
"""
from __future__ import annotations

import ctypes

from ._lib import check, lib, release
from .ntt64_pbs import _dev, _stream

NO_ADDITION = -1  # Candidate::NoAddition in the `candidate` outputs


class ModulusSwitchNoiseReductionKey:
    """The encryptions of zero and the three constants of the drift technique (``mi_ms_noise_key``).

    ``modulus_switch_zeros``: device tensor (zeros_count, lwe_dimension + 1) of u64, the reference's LweCiphertextList.
    A private copy in the kernels' tile order is made; the tensor may be released afterwards."""

    def __init__(self, modulus_switch_zeros, ms_bound: float, ms_r_sigma_factor: float, ms_input_variance: float):
        z = modulus_switch_zeros
        if z.dim() != 2 or z.shape[1] < 2:
            raise ValueError(f"assertion failed: modulus_switch_zeros shape {tuple(z.shape)} != "
                             "(zeros_count, lwe_dimension + 1)")
        if z.shape[0] == 0:
            raise ValueError("Expected at least one encryption of zero")
        self.zeros_count, self.lwe_dimension = int(z.shape[0]), int(z.shape[1]) - 1
        self.ms_bound, self.ms_r_sigma_factor = float(ms_bound), float(ms_r_sigma_factor)
        self.ms_input_variance = float(ms_input_variance)
        self.device = z.device
        h = ctypes.c_void_p()
        check(lib().mi_ms_noise_key_create(_dev(z, "modulus_switch_zeros"), self.lwe_dimension, self.zeros_count,
                                           self.ms_bound, self.ms_r_sigma_factor, self.ms_input_variance,
                                           z.device.index or 0, _stream(z), ctypes.byref(h)))
        self._h = h

    def __del__(self):
        release(self, "mi_ms_noise_key_destroy")

    def improve_modulus_switch_noise(self, input, log_modulus: int) -> None:
        """``input`` (..., lwe_dimension + 1), in place (modulus_switch_noise_reduction.rs:85-100)."""
        improve_lwe_ciphertext_modulus_switch_noise_for_binary_key(self, input, log_modulus)

    def improve_noise_and_modulus_switch(self, input, switched_out, log_modulus: int) -> None:
        """``switched_out`` (same shape as ``input``) gets the improved ciphertexts through the standard modulus
        switch: values in [0, 2^log_modulus), the MI_MS_PRE_SWITCHED input of every blind rotation / PBS (:102-118)."""
        batch = _batch(self, input)
        if tuple(switched_out.shape) != tuple(input.shape):
            raise ValueError(f"assertion failed: shapes {tuple(input.shape)} != {tuple(switched_out.shape)}")
        check(lib().mi_lwe_ms_noise_improve_and_switch_batch(self._h, _dev(switched_out, "switched_out"),
                                                             _dev(input, "input"), batch, log_modulus,
                                                             _stream(input)))


def _batch(key: ModulusSwitchNoiseReductionKey, lwe) -> int:
    size = key.lwe_dimension + 1
    if lwe.dim() < 1 or lwe.shape[-1] != size:
        raise ValueError(f"input lwe size (=LweSize({lwe.shape[-1] if lwe.dim() else 0})) != encryptions of zero lwe "
                         f"size (=LweSize({size}))")
    return lwe.numel() // size


def measure_modulus_switch_noise_estimation_for_binary_key(key: ModulusSwitchNoiseReductionKey, lwe,
                                                           log_modulus: int, all_candidates: bool = False):
    """The measure of every ciphertext of the batch (modulus_switch_noise_reduction.rs:71-86): a float64 device tensor
    (batch,), or (batch, 1 + zeros_count) with ``all_candidates``, whose column 1 + c is the measure of lwe + zero[c]."""
    import torch

    batch = _batch(key, lwe)
    cols = 1 + key.zeros_count if all_candidates else 1
    out = torch.empty((batch, cols), dtype=torch.float64, device=lwe.device)
    check(lib().mi_lwe_ms_noise_measure_batch(key._h, ctypes.c_void_p(out.data_ptr()), _dev(lwe, "lwe"), batch,
                                              log_modulus, int(all_candidates), _stream(lwe)))
    return out if all_candidates else out.reshape(batch)


def choose_candidate_to_improve_modulus_switch_noise_for_binary_key(key: ModulusSwitchNoiseReductionKey, lwe,
                                                                    log_modulus: int):
    """(candidate, satisfied) of every ciphertext (:99-195): candidate int64, ``NO_ADDITION`` or the index of the
    encryption of zero; satisfied int32, 1 for SatisfyingBound and 0 for BestNotSatisfyingBound."""
    import torch

    batch = _batch(key, lwe)
    candidate = torch.empty(batch, dtype=torch.int64, device=lwe.device)
    satisfied = torch.empty(batch, dtype=torch.int32, device=lwe.device)
    check(lib().mi_lwe_ms_noise_choose_batch(key._h, ctypes.c_void_p(candidate.data_ptr()),
                                             ctypes.c_void_p(satisfied.data_ptr()), _dev(lwe, "lwe"), batch,
                                             log_modulus, _stream(lwe)))
    return candidate, satisfied


def improve_lwe_ciphertext_modulus_switch_noise_for_binary_key(key: ModulusSwitchNoiseReductionKey, lwe,
                                                               log_modulus: int, output=None,
                                                               return_candidates: bool = False):
    """lwe += the chosen encryption of zero, for every ciphertext (:202-242); in place as the reference, or into
    ``output`` (same shape).  With ``return_candidates`` the (candidate, satisfied) tensors of the choice."""
    import torch

    batch = _batch(key, lwe)
    out = lwe if output is None else output
    if tuple(out.shape) != tuple(lwe.shape):
        raise ValueError(f"assertion failed: shapes {tuple(lwe.shape)} != {tuple(out.shape)}")
    candidate = satisfied = None
    cp = sp = None
    if return_candidates:
        candidate = torch.empty(batch, dtype=torch.int64, device=lwe.device)
        satisfied = torch.empty(batch, dtype=torch.int32, device=lwe.device)
        cp, sp = ctypes.c_void_p(candidate.data_ptr()), ctypes.c_void_p(satisfied.data_ptr())
    check(lib().mi_lwe_ms_noise_improve_batch(key._h, _dev(out, "output"), _dev(lwe, "lwe"), batch, log_modulus, cp,
                                              sp, _stream(lwe)))
    return (candidate, satisfied) if return_candidates else None


__all__ = ["ModulusSwitchNoiseReductionKey", "NO_ADDITION", "measure_modulus_switch_noise_estimation_for_binary_key",
           "choose_candidate_to_improve_modulus_switch_noise_for_binary_key",
           "improve_lwe_ciphertext_modulus_switch_noise_for_binary_key"]
