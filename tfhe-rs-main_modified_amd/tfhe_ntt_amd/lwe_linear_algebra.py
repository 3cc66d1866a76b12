"""Host-side mirror of the core_crypto LWE linear algebra over the C ABI (``mi_lwe_linear_combination_batch``).

Reference (paths relative to tfhe/src/core_crypto): algorithms/lwe_linear_algebra.rs

* ``lwe_ciphertext_add`` / ``lwe_ciphertext_add_assign``                  :190 / :67
* ``lwe_ciphertext_sub`` / ``lwe_ciphertext_sub_assign``                  :789 / :702
* ``lwe_ciphertext_opposite_assign``                                      :490
* ``lwe_ciphertext_cleartext_mul`` / ``lwe_ciphertext_cleartext_mul_assign``   :624 / :555
* ``lwe_ciphertext_plaintext_add_assign`` / ``lwe_ciphertext_plaintext_sub_assign``   :275 / :383

The reference handles one ciphertext per call; here every operand is a device tensor (..., lwe_size) of u64 with a
leading batch, native modulus.  All of them are one launch of the gathered linear combination (csrc/
lwe_linear_algebra.hip); ``lwe_linear_combination`` is that call itself, which is also the CUDA backend's input / output
index arrays.  The kernel reads one input list, so a two-operand function first joins its operands into one list, and
an ``_assign`` form computes into a new tensor and copies back.  Cleartexts are Python ints or int64 tensors with one
entry per ciphertext; plaintexts likewise (u64 words).  Shape mismatches raise ``ValueError``.
"""
from __future__ import annotations

import ctypes

from ._lib import check, lib
from .ntt64_pbs import _dev, _stream

NO_TERM = 0xFFFFFFFF  # an index that is out of range for every list: the term contributes nothing


def lwe_linear_combination(output, input, index, coeff=None, plaintext=None) -> None:
    """output[i] = sum_t coeff[i, t] * input[index[i, t]] + (0, ..., 0, plaintext[i]), wrapping.

    ``input`` (n_in, lwe_size) or None with no terms; ``output`` (n_out, lwe_size); ``index`` (n_out, terms) int32 device
    tensor (an entry >= n_in, e.g. ``NO_TERM`` stored as -1, drops the term); ``coeff`` (n_out, terms) int64 or None
    (all ones); ``plaintext`` (n_out,) int64 / uint64 or None.  ``output`` may not overlap ``input``."""
    import torch

    if output.dim() != 2:
        raise ValueError(f"assertion failed: output shape {tuple(output.shape)} != (n_out, lwe_size)")
    n_out, size = int(output.shape[0]), int(output.shape[1])
    terms = 0 if index is None else (int(index.shape[1]) if index.dim() == 2 else -1)
    if terms < 0 or (index is not None and (index.shape[0] != n_out or index.dtype not in (torch.int32, torch.uint32)
                                            or not index.is_cuda or not index.is_contiguous())):
        raise ValueError(f"assertion failed: index must be a contiguous ({n_out}, terms) int32 device tensor")
    n_in = 0
    if terms:
        if input is None or input.dim() != 2 or input.shape[1] != size:
            raise ValueError(f"assertion failed: input shape != (n_in, {size})")
        n_in = int(input.shape[0])
    for name, t in (("coeff", coeff), ("plaintext", plaintext)):
        want = (n_out, terms) if name == "coeff" else (n_out,)
        if t is not None and (tuple(t.shape) != want or not t.is_cuda or not t.is_contiguous()
                              or t.dtype not in (torch.int64, torch.uint64)):
            raise ValueError(f"assertion failed: {name} must be a contiguous {want} 64-bit device tensor")
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    check(lib().mi_lwe_linear_combination_batch(_dev(output, "output"), _dev(input, "input") if terms else None,
                                                size - 1, n_in, n_out, terms, ptr(index) if terms else None,
                                                ptr(coeff) if terms else None, ptr(plaintext),
                                                output.device.index or 0, _stream(output)))


def _rows(t, name):
    if t.dim() < 1:
        raise ValueError(f"assertion failed: {name} shape {tuple(t.shape)} != (..., lwe_size)")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return t.reshape(-1, t.shape[-1])


def _per_row(v, batch, device):
    """A cleartext / plaintext argument as a (batch,) int64 tensor: an int is broadcast."""
    import torch

    if isinstance(v, int):
        v %= 1 << 64
        return torch.full((batch,), v - (1 << 64) if v >= (1 << 63) else v, dtype=torch.int64, device=device)
    if v.numel() != batch:
        raise ValueError(f"assertion failed: expected one value per ciphertext ({batch}), got {v.numel()}")
    return v.reshape(batch).contiguous().view(torch.int64)


def _combine(output, operands, coeffs, plaintext=None) -> None:
    """output = sum_t coeffs[t] * operands[t] + plaintext over same-shaped operands; coeffs[t] an int or a per-row
    tensor.  ``output`` may be one of the operands."""
    import torch

    out = _rows(output, "output")
    batch, size = int(out.shape[0]), int(out.shape[1])
    ops = [_rows(o, "operand") for o in operands]
    if any(tuple(o.shape) != (batch, size) for o in ops):
        raise ValueError("assertion failed: mismatched LweSize or batch between the operands and the output")
    dev = output.device
    src = ops[0] if len(ops) == 1 else torch.cat(ops, dim=0)
    aliased = len(ops) == 1 and src.data_ptr() == out.data_ptr()
    dst = torch.empty_like(out) if aliased else out
    ar = torch.arange(batch, dtype=torch.int32, device=dev)
    index = torch.stack([ar + t * batch for t in range(len(ops))], dim=1).contiguous()
    coeff = None
    if any(not (isinstance(c, int) and c == 1) for c in coeffs):
        coeff = torch.stack([_per_row(c, batch, dev) for c in coeffs], dim=1).contiguous()
    pt = None if plaintext is None else _per_row(plaintext, batch, dev)
    lwe_linear_combination(dst, src.contiguous(), index, coeff, pt)
    if dst is not out:
        out.copy_(dst)


def lwe_ciphertext_add(output, lhs, rhs) -> None:
    _combine(output, [lhs, rhs], [1, 1])


def lwe_ciphertext_add_assign(lhs, rhs) -> None:
    _combine(lhs, [lhs, rhs], [1, 1])


def lwe_ciphertext_sub(output, lhs, rhs) -> None:
    _combine(output, [lhs, rhs], [1, -1])


def lwe_ciphertext_sub_assign(lhs, rhs) -> None:
    _combine(lhs, [lhs, rhs], [1, -1])


def lwe_ciphertext_opposite_assign(ct) -> None:
    _combine(ct, [ct], [-1])


def lwe_ciphertext_cleartext_mul(output, input, cleartext) -> None:
    _combine(output, [input], [cleartext])


def lwe_ciphertext_cleartext_mul_assign(ct, cleartext) -> None:
    _combine(ct, [ct], [cleartext])


def lwe_ciphertext_plaintext_add_assign(ct, plaintext) -> None:
    _combine(ct, [ct], [1], plaintext)


def lwe_ciphertext_plaintext_sub_assign(ct, plaintext) -> None:
    import torch

    neg = -plaintext if isinstance(plaintext, int) else (0 - plaintext.view(torch.int64))
    _combine(ct, [ct], [1], neg)


__all__ = ["NO_TERM", "lwe_linear_combination", "lwe_ciphertext_add", "lwe_ciphertext_add_assign", "lwe_ciphertext_sub",
           "lwe_ciphertext_sub_assign", "lwe_ciphertext_opposite_assign", "lwe_ciphertext_cleartext_mul",
           "lwe_ciphertext_cleartext_mul_assign", "lwe_ciphertext_plaintext_add_assign",
           "lwe_ciphertext_plaintext_sub_assign"]
