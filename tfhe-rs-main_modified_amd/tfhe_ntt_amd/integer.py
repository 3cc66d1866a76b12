"""Host-side mirror of the first slice of integer's radix server key over the C ABI (``mi_radix_*``).

Reference (paths relative to tfhe/src/integer/server_key):

* ``unchecked_add``                              radix/add.rs
* ``add_parallelized`` / ``unsigned_overflowing_add_parallelized``   radix_parallel/add.rs
* ``scalar_add_parallelized``                    radix_parallel/scalar_add.rs
* ``full_propagate_parallelized``                radix_parallel/mod.rs:228 (partial_propagate :91-201)
* ``propagate_single_carry_parallelized``        radix_parallel/add.rs (compute_prefix_sum_hillis_steele :1452-1487)
* ``bitand_parallelized`` / ``bitor_parallelized`` / ``bitxor_parallelized``   radix_parallel/bitwise_op.rs
* ``unchecked_sum_ciphertexts_vec_parallelized`` / ``sum_ciphertexts_parallelized``   radix_parallel/sum.rs:155-166, :183
* ``mul_parallelized``                           radix_parallel/mul.rs:599-608 (compute_terms_for_mul_low :333-400)

A ``RadixCiphertext`` is a batch of unsigned integers: a device tensor (n_integers, n_blocks, k N + 1) of shortint
blocks, least significant first, and one degree per block position on the host (the largest value a block at that
position may hold, shared by the integers of the batch), as the reference's ``Ciphertext::degree``.  An unchecked
operation whose degree would pass m c - 1 raises ``ValueError`` where the reference's checked form would refuse.
"""
from __future__ import annotations

from ._lib import check, lib
from .ntt64_pbs import _dev, _stream
from .shortint import ShortintServerKey


class RadixCiphertext:
    def __init__(self, blocks, degrees):
        if blocks.dim() != 3:
            raise ValueError(f"assertion failed: blocks shape {tuple(blocks.shape)} != (n_integers, n_blocks, lwe_size)")
        if len(degrees) != blocks.shape[1]:
            raise ValueError(f"assertion failed: {len(degrees)} degrees for {blocks.shape[1]} blocks")
        self.blocks, self.degrees = blocks, [int(d) for d in degrees]

    @property
    def n_integers(self) -> int:
        return int(self.blocks.shape[0])

    @property
    def n_blocks(self) -> int:
        return int(self.blocks.shape[1])

    def clone(self) -> "RadixCiphertext":
        return RadixCiphertext(self.blocks.clone(), self.degrees)


class ServerKey:
    """``integer::ServerKey`` over a ``ShortintServerKey``."""

    def __init__(self, key: ShortintServerKey):
        self.key = key

    # ---- checks ----
    def _same_shape(self, a: RadixCiphertext, b: RadixCiphertext):
        if tuple(a.blocks.shape) != tuple(b.blocks.shape) or a.blocks.shape[2] != self.key.lwe_size:
            raise ValueError(f"assertion failed: radix shapes {tuple(a.blocks.shape)} and {tuple(b.blocks.shape)}")

    def _guard(self, degrees):
        if max(degrees) > self.key.max_degree:
            raise ValueError(f"degree {max(degrees)} would pass message_modulus * carry_modulus - 1 = "
                             f"{self.key.max_degree}: propagate the carries first")
        return degrees

    def _clean(self, ct: RadixCiphertext) -> bool:
        return max(ct.degrees) < self.key.message_modulus

    def _propagate_single_carry(self, blocks, carry=None) -> None:
        check(lib().mi_radix_propagate_single_carry_batch(self.key._h, _dev(blocks, "blocks"),
                                                          _dev(carry, "carry") if carry is not None else None,
                                                          int(blocks.shape[1]), int(blocks.shape[0]), _stream(blocks)))

    # ---- operations ----
    def unchecked_add(self, lhs: RadixCiphertext, rhs: RadixCiphertext) -> RadixCiphertext:
        self._same_shape(lhs, rhs)
        degrees = self._guard([a + b for a, b in zip(lhs.degrees, rhs.degrees)])
        return RadixCiphertext(self.key.unchecked_add(lhs.blocks, rhs.blocks), degrees)

    def full_propagate_parallelized(self, ct: RadixCiphertext) -> None:
        """In place: blocks of any value below m c -> clean blocks (the carry out of the top block is dropped)."""
        self._guard(ct.degrees)
        b = ct.blocks
        check(lib().mi_radix_full_propagate_batch(self.key._h, _dev(b, "blocks"), ct.n_blocks, ct.n_integers,
                                                  _stream(b)))
        ct.degrees = [self.key.message_modulus - 1] * ct.n_blocks

    def _add(self, lhs, rhs, want_carry):
        import torch

        self._same_shape(lhs, rhs)
        for ct in (lhs, rhs):  # the reference propagates operands that carry carries first (a clone: &self inputs)
            if not self._clean(ct):
                raise ValueError("add_parallelized takes clean operands here: call full_propagate_parallelized first")
        out = torch.empty_like(lhs.blocks)
        carry = None
        if want_carry:
            carry = torch.empty((lhs.n_integers, self.key.lwe_size), dtype=lhs.blocks.dtype, device=lhs.blocks.device)
        check(lib().mi_radix_add_batch(self.key._h, _dev(out, "out"), _dev(lhs.blocks, "lhs"), _dev(rhs.blocks, "rhs"),
                                       _dev(carry, "carry") if want_carry else None, lhs.n_blocks, lhs.n_integers,
                                       _stream(out)))
        return RadixCiphertext(out, [self.key.message_modulus - 1] * lhs.n_blocks), carry

    def add_parallelized(self, lhs: RadixCiphertext, rhs: RadixCiphertext) -> RadixCiphertext:
        return self._add(lhs, rhs, False)[0]

    def unsigned_overflowing_add_parallelized(self, lhs: RadixCiphertext, rhs: RadixCiphertext):
        """(lhs + rhs mod m^B, the overflow flag): the flag is one shortint block per integer holding 0 or 1."""
        return self._add(lhs, rhs, True)

    def scalar_add_parallelized(self, ct: RadixCiphertext, scalar: int) -> RadixCiphertext:
        """ct + scalar mod m^B for a clean ``ct``: the scalar's radix digits on the bodies, one carry propagation."""
        import torch

        if not self._clean(ct):
            raise ValueError("scalar_add_parallelized takes a clean operand here: call full_propagate_parallelized first")
        m, n_blocks = self.key.message_modulus, ct.n_blocks
        scalar %= m ** n_blocks
        digits = [(scalar // m ** b) % m for b in range(n_blocks)]
        pts = torch.tensor(digits * ct.n_integers, dtype=torch.int64, device=ct.blocks.device)
        out = self.key.unchecked_scalar_add(ct.blocks, pts)
        self._propagate_single_carry(out)
        return RadixCiphertext(out, [m - 1] * n_blocks)

    def unchecked_sum_ciphertexts_vec_parallelized(self, ciphertexts, first_block=None):
        """The sum mod m^B of a list of clean ``RadixCiphertext`` of one shape (``mi_radix_sum_batch``); ``None`` for an
        empty list, as the reference.  ``first_block[t]``: term t is identically zero below that block (the blocks the
        reference skips by ``degree == 0``) and its rows there are not read."""
        import ctypes

        import torch

        ciphertexts = list(ciphertexts)
        if not ciphertexts:
            return None
        for ct in ciphertexts:
            self._same_shape(ciphertexts[0], ct)
            if not self._clean(ct):
                raise ValueError("sum_ciphertexts_parallelized takes clean operands here: call "
                                 "full_propagate_parallelized first")
        if first_block is not None and len(first_block) != len(ciphertexts):
            raise ValueError(f"assertion failed: {len(first_block)} first blocks for {len(ciphertexts)} terms")
        first = ciphertexts[0]
        terms = torch.stack([ct.blocks for ct in ciphertexts]).contiguous()
        out = torch.empty_like(first.blocks)
        fb = (ctypes.c_uint32 * len(ciphertexts))(*[int(f) for f in first_block]) if first_block is not None else None
        check(lib().mi_radix_sum_batch(self.key._h, _dev(out, "out"), _dev(terms, "terms"), len(ciphertexts), fb,
                                       first.n_blocks, first.n_integers, _stream(out)))
        return RadixCiphertext(out, [self.key.message_modulus - 1] * first.n_blocks)

    def sum_ciphertexts_parallelized(self, ciphertexts):
        """``sum_ciphertexts_parallelized`` (radix_parallel/sum.rs:183) on clean operands."""
        return self.unchecked_sum_ciphertexts_vec_parallelized(ciphertexts)

    def mul_parallelized(self, lhs: RadixCiphertext, rhs: RadixCiphertext) -> RadixCiphertext:
        """lhs * rhs mod m^B for clean operands (``mi_radix_mul_batch``; radix_parallel/mul.rs:599-608)."""
        import torch

        self._same_shape(lhs, rhs)
        for ct in (lhs, rhs):
            if not self._clean(ct):
                raise ValueError("mul_parallelized takes clean operands here: call full_propagate_parallelized first")
        out = torch.empty_like(lhs.blocks)
        check(lib().mi_radix_mul_batch(self.key._h, _dev(out, "out"), _dev(lhs.blocks, "lhs"), _dev(rhs.blocks, "rhs"),
                                       lhs.n_blocks, lhs.n_integers, _stream(out)))
        return RadixCiphertext(out, [self.key.message_modulus - 1] * lhs.n_blocks)

    def _bitwise(self, lhs, rhs, name, f):
        self._same_shape(lhs, rhs)
        m = self.key.message_modulus
        for ct in (lhs, rhs):
            if not self._clean(ct):
                raise ValueError(f"bit{name}_parallelized takes clean operands here: call full_propagate_parallelized "
                                 "first")
        lut = self.key._cached_lut("bit" + name, f, bivariate=True)
        size = self.key.lwe_size
        out = self.key.unchecked_apply_lookup_table_bivariate(lhs.blocks.reshape(-1, size), rhs.blocks.reshape(-1, size),
                                                              lut)
        return RadixCiphertext(out.reshape(lhs.blocks.shape), [m - 1] * lhs.n_blocks)

    def bitand_parallelized(self, lhs: RadixCiphertext, rhs: RadixCiphertext) -> RadixCiphertext:
        return self._bitwise(lhs, rhs, "and", lambda a, b: a & b)

    def bitor_parallelized(self, lhs: RadixCiphertext, rhs: RadixCiphertext) -> RadixCiphertext:
        return self._bitwise(lhs, rhs, "or", lambda a, b: a | b)

    def bitxor_parallelized(self, lhs: RadixCiphertext, rhs: RadixCiphertext) -> RadixCiphertext:
        return self._bitwise(lhs, rhs, "xor", lambda a, b: a ^ b)


__all__ = ["RadixCiphertext", "ServerKey"]
