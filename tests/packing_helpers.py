"""References for the LWE packing keyswitch and the GLWE compression tests (numpy / plain Python, host only).

Reference paths are relative to tfhe/src/core_crypto.

* ``packing_keyswitch_ref``: keyswitch_lwe_ciphertext_list_and_pack_in_glwe_ciphertext
  (algorithms/lwe_packing_keyswitch.rs:296-379) composed from the oracle's pinned pieces: the LWE keyswitch over the
  pre-rounded mask (the packing keyswitch decomposes closest_representable(a_i), :173-174, whose balanced-rounding
  tie differs from decompose(a_i)'s), the body added at column k N (:161), one oracle.poly_monomial_mul per
  polynomial and wrapping adds (:369-378).
* ``packing_keyswitch_transcription``: the same two functions line by line on Python integers (tiny shapes only),
  the check of the composition.
* ``pack_ref`` / ``compress_ref`` / ``extract_ref``: PackedIntegers::pack / unpack (entities/packed_integers.rs:39-222)
  restated on one big integer (the values concatenated log_modulus bits each, little end first, cut into 64-bit
  words) around oracle.modulus_switch; ``pack_loop`` is the Rust's own loop, the check of the restatement.
* ``pksk_gen``: a packing keyswitch key with the semantics of generate_lwe_packing_keyswitch_key
  (algorithms/lwe_packing_keyswitch_key_generation.rs:129-156), our own random stream.
"""
import numpy as np

import tfhe_helpers as H

M64 = (1 << 64) - 1


def pre_round(a, base_log, level):
    """native_closest_representable (commons/math/decomposition/decomposer.rs:25-49) of every word of a u64 array."""
    shift = np.uint64(63 - base_log * level)
    with np.errstate(over="ignore"):
        return (((np.asarray(a, np.uint64) >> shift) + np.uint64(1)) & ~np.uint64(1)) << shift


def tie_words(base_log, level):
    """Mask words around the rounding corners: 0, 2^64 - 1, 2^63, 2^63 - 1, and the ends of the interval whose
    pre-rounded state 2^(rep-1) is not balanced where decompose(a_i) would balance it."""
    step = 1 << (63 - base_log * level)
    return [0, M64, 1 << 63, (1 << 63) - 1, (1 << 63) - step, (1 << 63) - step - 1]


def single_keyswitch_rows(oracle, pksk, lwe, k, n, base_log, level, rounded=True):
    """keyswitch_lwe_ciphertext_into_glwe_ciphertext (:102-187) of every ciphertext of lwe (batch, in_dim + 1):
    (batch, (k + 1) N).  rounded=False composes it from decompose(a_i) instead (the LWE keyswitch's digits): wrong on
    the tie, kept to pin that the two differ."""
    in_dim, size = lwe.shape[-1] - 1, (k + 1) * n
    x = np.ascontiguousarray(lwe, dtype=np.uint64).copy()
    if rounded:
        x[:, :in_dim] = pre_round(x[:, :in_dim], base_log, level)
    x[:, in_dim] = 0
    key = np.ascontiguousarray(pksk, dtype=np.uint64).reshape(in_dim, level, size)
    rows = oracle.lwe_keyswitch(key, x, size - 1, base_log, level)
    with np.errstate(over="ignore"):
        rows[:, k * n] += np.asarray(lwe, np.uint64)[:, in_dim]
    return rows


def packing_keyswitch_ref(oracle, pksk, lwe, k, n, base_log, level, lwe_per_glwe, rounded=True):
    """lwe (n_lwe, in_dim + 1) -> (ceil(n_lwe / lwe_per_glwe), k + 1, N): every chunk of lwe_per_glwe ciphertexts
    packed into one GLWE (:296-379)."""
    assert lwe_per_glwe <= n
    rows = single_keyswitch_rows(oracle, pksk, lwe, k, n, base_log, level, rounded).reshape(-1, k + 1, n)
    n_lwe = rows.shape[0]
    out = np.zeros(((n_lwe + lwe_per_glwe - 1) // lwe_per_glwe, k + 1, n), np.uint64)
    with np.errstate(over="ignore"):
        for i in range(n_lwe):
            g, d = divmod(i, lwe_per_glwe)
            for p in range(k + 1):
                out[g, p] += oracle.poly_monomial_mul(rows[i, p], d)
    return out


def _closest_representable(x, base_log, level):
    shift = 64 - base_log * level - 1
    res = ((x >> shift) + 1) & M64
    res &= M64 - 1
    return (res << shift) & M64


def packing_keyswitch_transcription(oracle, pksk, lwe_list, k, n, base_log, level):
    """lwe_packing_keyswitch.rs:296-379 calling :102-187, statement by statement on Python integers; the decomposer's
    state machine is the oracle's (decomposer.rs:156-185, iter.rs:131-151), already pinned against the reference.
    pksk (in_dim, level, (k + 1) N), lwe_list (count, in_dim + 1) -> one GLWE ((k + 1) N,)."""
    size = (k + 1) * n
    key = [[[int(v) for v in row] for row in block] for block in np.asarray(pksk).reshape(-1, level, size)]
    assert len(lwe_list) <= n
    output = [0] * size                                                   # :361
    for degree, ct in enumerate(lwe_list):                                # :369
        ct = [int(v) for v in ct]
        buffer = [0] * size                                               # :160
        buffer[k * n] = ct[-1]                                            # :161
        for block, a in zip(key, ct[:-1]):                                # :169-171
            rounded = _closest_representable(a, base_log, level)          # :173
            state = oracle.decomp_init_native(rounded, base_log, level)   # :174
            for row in block:                                             # :179
                digit, state = oracle.decompose_one_level(base_log, state)
                for c in range(size):                                     # :180-184 slice_wrapping_sub_scalar_mul_assign
                    buffer[c] = (buffer[c] - row[c] * digit) & M64
        for p in range(k + 1):                                            # :371-376, X^degree mod X^N + 1
            poly = buffer[p * n:(p + 1) * n]
            poly = poly[n - degree:] + poly[:n - degree] if degree else poly
            buffer[p * n:(p + 1) * n] = [(-v) & M64 if j < degree else v for j, v in enumerate(poly)]
        output = [(o + b) & M64 for o, b in zip(output, buffer)]          # :377
    return np.array(output, dtype=np.uint64)


def pack_ref(values, log_modulus):
    """PackedIntegers::pack (packed_integers.rs:39-130): values < 2^log_modulus -> ceil(len * log_modulus / 64) u64."""
    big = 0
    for j, v in enumerate(values):
        big |= int(v) << (j * log_modulus)
    words = (len(values) * log_modulus + 63) // 64
    return np.array([(big >> (64 * i)) & M64 for i in range(words)], dtype=np.uint64)


def pack_loop(values, log_modulus):
    """The reference's own loop (packed_integers.rs:89-121), for checking pack_ref."""
    values = [int(v) for v in values]
    out = []
    for i in range((len(values) * log_modulus + 63) // 64):
        j = 64 * i // log_modulus
        value = values[j] >> (i * 64 - j * log_modulus)
        j += 1
        while j * log_modulus < (i + 1) * 64 and j < len(values):
            value |= (values[j] << (j * log_modulus - i * 64)) & M64
            j += 1
        out.append(value)
    return np.array(out, dtype=np.uint64)


def unpack_ref(packed, count, log_modulus):
    """PackedIntegers::unpack (packed_integers.rs:132-222)."""
    big = 0
    for i, w in enumerate(packed):
        big |= int(w) << (64 * i)
    mask = (1 << log_modulus) - 1
    return [(big >> (j * log_modulus)) & mask for j in range(count)]


def compress_ref(oracle, glwe, k, n, bodies_count, log_modulus):
    """CompressedModulusSwitchedGlweCiphertext::compress (compressed_modulus_switched_glwe_ciphertext.rs:169-220) of
    one GLWE (k + 1, N): the packed words."""
    flat = np.asarray(glwe, np.uint64).reshape(-1)[:k * n + bodies_count]
    return pack_ref([oracle.modulus_switch(int(v), log_modulus) for v in flat], log_modulus)


def extract_ref(packed, k, n, bodies_count, log_modulus):
    """::extract (:226-256): (k + 1, N), the body polynomial zero past bodies_count."""
    vals = unpack_ref(packed, k * n + bodies_count, log_modulus)
    out = np.zeros((k + 1) * n, np.uint64)
    out[:len(vals)] = [(v << (64 - log_modulus)) & M64 for v in vals]
    return out.reshape(k + 1, n)


def pksk_gen(g, in_sk, glwe_sk, base_log, level, noise_log2):
    """LwePackingKeyswitchKey (in_dim, level, k + 1, N): block i, entry li is a GLWE encryption under glwe_sk of the
    constant polynomial s_in[i] << (64 - base_log * (level - li))
    (lwe_packing_keyswitch_key_generation.rs:129-156: levels level_count down to 1)."""
    k, n = glwe_sk.shape
    rows = in_sk.size * level
    mask = H.uniform_u64(g, (rows, k, n))
    with np.errstate(over="ignore"):
        body = H.tuniform(g, (rows, n), noise_log2)
        for i in range(k):
            body += H.negacyclic_mul_binary(mask[:, i], glwe_sk[i])
        body[:, 0] += np.array([(int(s) << (64 - base_log * (level - li))) & M64 for s in in_sk for li in range(level)],
                               dtype=np.uint64)
    return np.concatenate([mask, body[:, None, :]], axis=1).reshape(in_sk.size, level, k + 1, n)
