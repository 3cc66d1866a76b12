"""Host-side mirror of the core_crypto bootstrap without padding bit (WoP-PBS) over the C ABI.

Reference (paths relative to tfhe/src/core_crypto):

* ``LwePrivateFunctionalPackingKeyswitchKeyList``   entities/lwe_private_functional_packing_keyswitch_key_list.rs
* ``private_functional_keyswitch_lwe_ciphertext_into_glwe_ciphertext``
                                                     algorithms/lwe_private_functional_packing_keyswitch.rs:20-88
* ``extract_bits_from_lwe_ciphertext_mem_optimized``  algorithms/lwe_wopbs.rs (fft_impl/fft64/crypto/wop_pbs/mod.rs:61-220)
* ``circuit_bootstrap_boolean``                       wop_pbs/mod.rs:238-435
* ``cmux_tree_memory_optimized``                      wop_pbs/mod.rs:459-583
* ``blind_rotate_assign``                             wop_pbs/mod.rs:838-863
* ``vertical_packing``                                wop_pbs/mod.rs:771-825
* ``circuit_bootstrap_boolean_vertical_packing_lwe_ciphertext_list_mem_optimized``
                                                     algorithms/lwe_wopbs.rs:644-698 (wop_pbs/mod.rs:638-732)

The reference evaluates one ciphertext per call; every function here takes a leading batch dimension of independent
evaluations.  GGSW lists are float64 device tensors (batch, n_ggsw, level, k+1, k+1, N/2, 2) in the ``Fft`` plan's
order, most significant bit first, as the reference's FourierGgswCiphertextList.  Shape mismatches raise
``ValueError`` where the reference panics on ``assert!``.
"""
from __future__ import annotations

import ctypes

from ._lib import check, lib, release
from .fft64 import Fft, FourierLweBootstrapKey, _fdev
from .lwe_keyswitch import LweKeyswitchKey
from .ntt64_pbs import _dev, _stream


class LwePrivateFunctionalPackingKeyswitchKeyList:
    """A device list of private functional packing keyswitch keys prepared for the keyswitch below
    (``mi_lwe_pfpksk_list``).

    ``pfpksk_list``: device tensor (n_keys, in_dim + 1, level, k + 1, N) of u64 in the reference layout (levels as
    generate_lwe_private_functional_packing_keyswitch_key stores them).  A private matrix-core copy is made; the
    tensor may be released afterwards."""

    def __init__(self, pfpksk_list, base_log: int, level: int):
        t = pfpksk_list
        if t.dim() != 5 or t.shape[2] != level or t.shape[3] < 2 or t.shape[1] < 2:
            raise ValueError(f"assertion failed: pfpksk list shape {tuple(t.shape)} != (n_keys, in_dim + 1, {level}, "
                             "k + 1, N)")
        self.lwe_pfpksk_count = int(t.shape[0])
        self.input_key_lwe_dimension = int(t.shape[1]) - 1
        self.output_key_glwe_dimension = int(t.shape[3]) - 1
        self.output_polynomial_size = int(t.shape[4])
        self.decomposition_base_log, self.decomposition_level_count = base_log, level
        self.device = t.device
        h = ctypes.c_void_p()
        check(lib().mi_lwe_pfpksk_list_create(_dev(t, "pfpksk_list"), self.lwe_pfpksk_count,
                                              self.input_key_lwe_dimension, self.output_key_glwe_dimension,
                                              self.output_polynomial_size, base_log, level, t.device.index or 0,
                                              _stream(t), ctypes.byref(h)))
        self._h = h

    def __del__(self):
        release(self, "mi_lwe_pfpksk_list_destroy")


def private_functional_keyswitch_lwe_ciphertext_into_glwe_ciphertext(
        lwe_pfpksk: LwePrivateFunctionalPackingKeyswitchKeyList, output_glwe_ciphertext, input_lwe_ciphertext) -> None:
    """output[b, j] = key j of the list applied to input[b]: input (..., in_dim + 1) -> output (..., n_keys, k + 1, N)."""
    k = lwe_pfpksk
    n_in = k.input_key_lwe_dimension + 1
    if input_lwe_ciphertext.dim() < 1 or input_lwe_ciphertext.shape[-1] != n_in:
        raise ValueError(f"assertion failed: Mismatched input LweDimension != {k.input_key_lwe_dimension}")
    want = (k.lwe_pfpksk_count, k.output_key_glwe_dimension + 1, k.output_polynomial_size)
    batch = input_lwe_ciphertext.numel() // n_in
    out = output_glwe_ciphertext
    if out.dim() < 3 or tuple(out.shape[-3:]) != want or out.numel() != batch * want[0] * want[1] * want[2]:
        raise ValueError(f"assertion failed: output shape {tuple(out.shape)} != (batch = {batch}, *{want})")
    check(lib().mi_lwe_pfpks_batch(k._h, _dev(out, "output_glwe_ciphertext"),
                                   _dev(input_lwe_ciphertext, "input_lwe_ciphertext"), batch, _stream(out)))


def extract_bits_from_lwe_ciphertext_mem_optimized(lwe_in, lwe_list_out, fourier_bsk: FourierLweBootstrapKey,
                                                   ksk: LweKeyswitchKey, delta_log: int,
                                                   number_of_bits_to_extract: int) -> None:
    """lwe_in (batch, k N + 1) -> lwe_list_out (batch, n_bits, n + 1), the most significant extracted bit first."""
    big1, small1 = fourier_bsk.output_lwe_size(), ksk.output_key_lwe_dimension + 1
    if lwe_in.dim() < 1 or lwe_in.shape[-1] != big1:
        raise ValueError(f"assertion failed: lwe_in needs to have an LWE size of {big1}, got {lwe_in.shape[-1]}")
    batch, nb = lwe_in.numel() // big1, int(number_of_bits_to_extract)
    if lwe_list_out.dim() < 2 or tuple(lwe_list_out.shape[-2:]) != (nb, small1) or lwe_list_out.numel() != batch * nb * small1:
        raise ValueError(f"assertion failed: lwe_list_out shape {tuple(lwe_list_out.shape)} != ({batch}, {nb}, {small1})")
    check(lib().mi_fft64_extract_bits_batch(fourier_bsk._h, ksk._h, _dev(lwe_list_out, "lwe_list_out"),
                                            _dev(lwe_in, "lwe_in"), delta_log, nb, batch, _stream(lwe_in)))


def circuit_bootstrap_boolean(fourier_bsk: FourierLweBootstrapKey, lwe_in, delta_log: int,
                              pfpksk_list: LwePrivateFunctionalPackingKeyswitchKeyList, base_log_cbs: int,
                              level_cbs: int, ggsw_out=None, fourier_ggsw_out=None, fft: Fft | None = None) -> None:
    """lwe_in (batch, n + 1) of boolean messages at bit ``delta_log`` -> ggsw_out (batch, level_cbs, k + 1, k + 1, N)
    u64 (output index 0 = decomposition level level_cbs) and / or fourier_ggsw_out (batch, level_cbs, k + 1, k + 1,
    N / 2, 2) float64 in ``fft``'s order."""
    p = pfpksk_list
    small1 = fourier_bsk.input_lwe_dimension + 1
    if lwe_in.dim() < 1 or lwe_in.shape[-1] != small1:
        raise ValueError(f"assertion failed: lwe_in needs to have an LWE size of {small1}, got {lwe_in.shape[-1]}")
    batch = lwe_in.numel() // small1
    kp1, n = p.output_key_glwe_dimension + 1, p.output_polynomial_size
    if ggsw_out is None and fourier_ggsw_out is None:
        raise ValueError("assertion failed: no output")
    if ggsw_out is not None and (tuple(ggsw_out.shape[-4:]) != (level_cbs, p.lwe_pfpksk_count, kp1, n)
                                 or ggsw_out.numel() != batch * level_cbs * p.lwe_pfpksk_count * kp1 * n):
        raise ValueError(f"assertion failed: ggsw_out shape {tuple(ggsw_out.shape)}")
    if fourier_ggsw_out is not None:
        fft = fft or Fft(n, lwe_in.device.index or 0)
        if (tuple(fourier_ggsw_out.shape[-5:]) != (level_cbs, p.lwe_pfpksk_count, kp1, n // 2, 2)
                or fourier_ggsw_out.numel() != batch * level_cbs * p.lwe_pfpksk_count * kp1 * n):
            raise ValueError(f"assertion failed: fourier_ggsw_out shape {tuple(fourier_ggsw_out.shape)}")
    check(lib().mi_fft64_circuit_bootstrap_boolean_batch(
        fourier_bsk._h, p._h, fft.handle if fft is not None else None,
        _dev(ggsw_out, "ggsw_out") if ggsw_out is not None else None,
        _fdev(fourier_ggsw_out, "fourier_ggsw_out") if fourier_ggsw_out is not None else None,
        _dev(lwe_in, "lwe_in"), batch, delta_log, base_log_cbs, level_cbs, _stream(lwe_in)))


def _ggsw_list(fft, ggsw_list, level, batch):
    """(batch, n_ggsw, level, k+1, k+1, N/2, 2) -> (n_ggsw, k)."""
    g = ggsw_list
    if g.dim() != 7 or g.shape[0] != batch or g.shape[2] != level or g.shape[3] != g.shape[4] \
            or tuple(g.shape[-2:]) != (fft.n // 2, 2):
        raise ValueError(f"assertion failed: fourier ggsw list shape {tuple(g.shape)} != ({batch}, n_ggsw, {level}, "
                         f"k + 1, k + 1, {fft.n // 2}, 2)")
    return int(g.shape[1]), int(g.shape[3]) - 1


def _luts(lut, n):
    """(n_outputs, n_polys, N) -> (n_outputs, n_polys)."""
    if lut.dim() != 3 or lut.shape[-1] != n:
        raise ValueError(f"assertion failed: lut shape {tuple(lut.shape)} != (n_outputs, n_polys, {n})")
    return int(lut.shape[0]), int(lut.shape[1])


def cmux_tree_memory_optimized(output_glwe, lut_per_layer, ggsw_list, base_log: int, level: int,
                               fft: Fft | None = None) -> None:
    """output_glwe (batch, n_outputs, k + 1, N) = the CMUX tree of lut_per_layer (n_outputs, 2^r, N), shared by the
    batch, selected by the r GGSWs of ggsw_list (batch, r, level, k+1, k+1, N/2, 2); the last GGSW selects the first
    layer."""
    fft = fft or Fft(int(lut_per_layer.shape[-1]), lut_per_layer.device.index or 0)
    n_out, n_polys = _luts(lut_per_layer, fft.n)
    batch = int(output_glwe.shape[0]) if output_glwe.dim() == 4 else -1
    r, k = _ggsw_list(fft, ggsw_list, level, batch)
    if n_polys != 1 << r:
        raise ValueError(f"assertion failed: lut_per_layer polynomial count {n_polys} != 1 << {r}")
    if tuple(output_glwe.shape) != (batch, n_out, k + 1, fft.n):
        raise ValueError(f"assertion failed: output_glwe shape {tuple(output_glwe.shape)}")
    check(lib().mi_fft64_cmux_tree_batch(fft.handle, _dev(output_glwe, "output_glwe"),
                                         _dev(lut_per_layer, "lut_per_layer"), n_polys, n_out,
                                         _fdev(ggsw_list, "ggsw_list") if r else None, r, 0, r, k, base_log, level, batch,
                                         _stream(output_glwe)))


def blind_rotate_assign(lut, ggsw_list, base_log: int, level: int, fft: Fft | None = None) -> None:
    """lut (batch, n_outputs, k + 1, N), in place: from the last GGSW of ggsw_list (batch, n, level, ...) to the first,
    ct1 = ct0 / X^d, d doubling from 1, ct0 = cmux(ct0, ct1)."""
    fft = fft or Fft(int(lut.shape[-1]), lut.device.index or 0)
    batch = int(lut.shape[0]) if lut.dim() == 4 else -1
    n_rot, k = _ggsw_list(fft, ggsw_list, level, batch)
    if tuple(lut.shape[2:]) != (k + 1, fft.n):
        raise ValueError(f"assertion failed: lut shape {tuple(lut.shape)}")
    check(lib().mi_fft64_wop_blind_rotate_batch(fft.handle, _dev(lut, "lut"), int(lut.shape[1]),
                                                _fdev(ggsw_list, "ggsw_list") if n_rot else None, n_rot, 0, n_rot, k,
                                                base_log, level, batch, _stream(lut)))


def vertical_packing(lut, lwe_out, ggsw_list, base_log: int, level: int, fft: Fft | None = None) -> None:
    """lwe_out (batch, n_outputs, k N + 1) = the vertical packing of lut (n_outputs, n_polys, N) by ggsw_list (batch,
    n_ggsw, level, ...), most significant bit first: CMUX tree, rotation, sample extraction."""
    fft = fft or Fft(int(lut.shape[-1]), lut.device.index or 0)
    n_out, n_polys = _luts(lut, fft.n)
    batch = int(lwe_out.shape[0]) if lwe_out.dim() == 3 else -1
    n_ggsw, k = _ggsw_list(fft, ggsw_list, level, batch)
    if tuple(lwe_out.shape) != (batch, n_out, k * fft.n + 1):
        raise ValueError(f"assertion failed: lwe_out shape {tuple(lwe_out.shape)} != ({batch}, {n_out}, {k * fft.n + 1})")
    check(lib().mi_fft64_vertical_packing_batch(fft.handle, _dev(lwe_out, "lwe_out"), _dev(lut, "lut"), n_polys, n_out,
                                                _fdev(ggsw_list, "ggsw_list") if n_ggsw else None, n_ggsw, k, base_log,
                                                level, batch, _stream(lwe_out)))


def circuit_bootstrap_boolean_vertical_packing_lwe_ciphertext_list_mem_optimized(
        lwe_list_in, lwe_list_out, big_lut_as_polynomial_list, fourier_bsk: FourierLweBootstrapKey,
        pfpksk_list: LwePrivateFunctionalPackingKeyswitchKeyList, base_log_cbs: int, level_cbs: int,
        fft: Fft | None = None) -> None:
    """lwe_list_in (batch, n_bits, n + 1) boolean LWEs (bit in the top bit, most significant first, as
    ``extract_bits`` writes them) -> lwe_list_out (batch, n_outputs, k N + 1): output o is big_lut[o] (n_outputs,
    n_polys, N) evaluated at the input bits."""
    p = pfpksk_list
    fft = fft or Fft(p.output_polynomial_size, lwe_list_in.device.index or 0)
    n_out, n_polys = _luts(big_lut_as_polynomial_list, fft.n)
    small1 = fourier_bsk.input_lwe_dimension + 1
    if lwe_list_in.dim() != 3 or lwe_list_in.shape[-1] != small1:
        raise ValueError(f"assertion failed: lwe_list_in shape {tuple(lwe_list_in.shape)} != (batch, n_bits, {small1})")
    batch, n_bits = int(lwe_list_in.shape[0]), int(lwe_list_in.shape[1])
    out1 = p.output_key_glwe_dimension * p.output_polynomial_size + 1
    if tuple(lwe_list_out.shape) != (batch, n_out, out1):
        raise ValueError(f"assertion failed: lwe_list_out shape {tuple(lwe_list_out.shape)} != ({batch}, {n_out}, {out1})")
    check(lib().mi_fft64_circuit_bootstrap_boolean_vertical_packing_batch(
        fourier_bsk._h, p._h, fft.handle, _dev(lwe_list_out, "lwe_list_out"), _dev(lwe_list_in, "lwe_list_in"), n_bits,
        _dev(big_lut_as_polynomial_list, "big_lut_as_polynomial_list"), n_polys, n_out, base_log_cbs, level_cbs, batch,
        _stream(lwe_list_out)))


__all__ = ["LwePrivateFunctionalPackingKeyswitchKeyList",
           "private_functional_keyswitch_lwe_ciphertext_into_glwe_ciphertext",
           "extract_bits_from_lwe_ciphertext_mem_optimized", "circuit_bootstrap_boolean", "cmux_tree_memory_optimized",
           "blind_rotate_assign", "vertical_packing",
           "circuit_bootstrap_boolean_vertical_packing_lwe_ciphertext_list_mem_optimized"]
