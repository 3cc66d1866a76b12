"""References for the 128-bit LWE packing keyswitch and GLWE compression tests (numpy / plain Python, host only): the
u128 twins of packing_helpers.py, built on pbs128_helpers.py (to_words, closest_representable, py_decompose,
corner_words, monomial_mul, glwe_encrypt / glwe_decrypt).

Reference paths are relative to tfhe/src/core_crypto.

* ``packing_keyswitch128_transcription``: keyswitch_lwe_ciphertext_list_and_pack_in_glwe_ciphertext
  (algorithms/lwe_packing_keyswitch.rs:296-379) calling keyswitch_lwe_ciphertext_into_glwe_ciphertext (:102-187),
  statement by statement on Python integers at Scalar = u128 (tiny shapes only).
* ``single_keyswitch_rows128`` / ``packing_keyswitch128_ref``: the vectorised reference for larger shapes.  Every key
  row ((k + 1) N u128) is packed into one big integer, 256-bit slots, so that one ciphertext's sum
  sum_i d_i KEY[i] is in_dim level multiplications of a big integer by a digit; the rotate-and-sum is numpy on
  (lo, hi) words with explicit carries.
* ``pack128_ref`` / ``compress128_ref`` / ``extract128_ref``: PackedIntegers<u128>::pack / unpack
  (entities/packed_integers.rs:39-222) restated on one big integer cut into 128-bit words, around modulus_switch
  (fft_impl/common.rs:10-23) at 128 bits; ``pack128_loop`` is the Rust's own loop, the check of the restatement.
* ``pksk128_gen``: a packing keyswitch key with the semantics of generate_lwe_packing_keyswitch_key
  (algorithms/lwe_packing_keyswitch_key_generation.rs:129-156), our own random stream.
* ``tie_words128``: the mask words around the rounding corners of the pre-rounded decomposition.
* ``signed_bytes`` / ``from_signed_bytes``: the signed-byte recoding of the GEMM (x = sum_t s_t 2^(8t) mod 2^(8 count),
  s_t in [-128, 127]) and its inverse.
"""
import numpy as np

import pbs128_helpers as R

M128, MASK128, MASK64 = R.M128, R.MASK128, R.MASK64


def tie_words128(base_log, level):
    """0, 2^128 - 1, 2^127, 2^127 - 1, and the ends of the interval whose pre-rounded state 2^(rep-1) is not balanced
    where decompose(a_i) would balance it."""
    step = 1 << (127 - base_log * level)
    return [0, MASK128, 1 << 127, (1 << 127) - 1, (1 << 127) - step, (1 << 127) - step - 1]


def digits128(a, base_log, level, rounded=True):
    """The packing keyswitch's digits of one mask word, least significant first (lwe_packing_keyswitch.rs:173-174:
    decompose(closest_representable(a))).  rounded=False: decompose(a), the LWE keyswitch's digits: wrong on the tie,
    kept to pin that the two differ."""
    return R.py_decompose(R.closest_representable(a, base_log, level) if rounded else a, base_log, level)


def packing_keyswitch128_transcription(pksk, lwe_list, k, n, base_log, level, rounded=True):
    """lwe_packing_keyswitch.rs:296-379 calling :102-187, statement by statement on Python integers.
    pksk: in_dim blocks of `level` rows of (k + 1) N ints; lwe_list: `count` lists of in_dim + 1 ints -> one GLWE,
    (k + 1) N ints."""
    size = (k + 1) * n
    assert len(lwe_list) <= n                                                 # :358-360
    output = [0] * size                                                       # :361
    for degree, ct in enumerate(lwe_list):                                    # :369
        buffer = [0] * size                                                   # :160
        buffer[k * n] = ct[-1]                                                # :161
        for block, a in zip(pksk, ct[:-1]):                                   # :169-171
            terms = digits128(a, base_log, level, rounded)                    # :173-174
            for row, digit in zip(block, terms):                              # :179
                for c in range(size):                                         # :180-184 slice_wrapping_sub_scalar_mul_assign
                    buffer[c] = (buffer[c] - row[c] * digit) & MASK128
        for p in range(k + 1):                                                # :371-376, X^degree mod X^N + 1
            buffer[p * n:(p + 1) * n] = R.monomial_mul(buffer[p * n:(p + 1) * n], degree)
        output = [(o + b) & MASK128 for o, b in zip(output, buffer)]          # :377
    return output


# ---- the vectorised reference ------------------------------------------------------------------------------------------

_SLOT = 32  # bytes per packed key word: 128 bits + 62 digit bits + 24 bits of row count + a sign bit fit 256


def _pack_rows(key_words):
    """(rows, size, 2) uint64 -> one big integer per row, 256-bit slots."""
    rows, size, _ = key_words.shape
    padded = np.zeros((rows, size, _SLOT // 8), "<u8")
    padded[:, :, :2] = key_words
    return [int.from_bytes(padded[r].tobytes(), "little") for r in range(rows)]


def single_keyswitch_rows128(pksk, lwe, k, n, base_log, level, rounded=True, block=256):
    """keyswitch_lwe_ciphertext_into_glwe_ciphertext (:102-187) of every ciphertext: pksk (in_dim, level, k + 1, N, 2)
    uint64 words, lwe (batch, in_dim + 1, 2) -> (batch, (k + 1) N, 2)."""
    size = (k + 1) * n
    lwe = np.asarray(lwe, np.uint64)
    batch, in_dim = lwe.shape[0], lwe.shape[1] - 1
    assert base_log <= 63 and in_dim * level < 1 << 24  # what a 256-bit slot holds
    key = np.asarray(pksk, np.uint64).reshape(in_dim * level, size, 2)
    digits = [[d for a in ct[:-1] for d in digits128(a, base_log, level, rounded)] for ct in R.from_words(lwe)]
    sums = [0] * batch
    for r0 in range(0, in_dim * level, block):  # a block of key rows at a time: the packed rows are twice the key
        for j, row in enumerate(_pack_rows(key[r0:r0 + block])):
            for b in range(batch):
                d = digits[b][r0 + j]
                if d:
                    sums[b] += d * row
    # T = -sum mod 2^128 per slot: 2^255 - sum keeps every slot in [0, 2^256), so no borrow crosses slots
    offset = int.from_bytes(bytes([0] * (_SLOT - 1) + [0x80]) * size, "little")
    out = np.empty((batch, size, 2), np.uint64)
    for b in range(batch):
        raw = (offset - sums[b]).to_bytes(size * _SLOT, "little")
        out[b] = np.frombuffer(raw, "<u8").reshape(size, _SLOT // 8)[:, :2]
    body = np.zeros((batch, size, 2), np.uint64)
    body[:, k * n] = lwe[:, in_dim]
    return add128(out, body)


def add128(a, b):
    """(..., 2) uint64 (lo, hi) + (..., 2) mod 2^128."""
    with np.errstate(over="ignore"):
        lo = a[..., 0] + b[..., 0]
        hi = a[..., 1] + b[..., 1] + (lo < a[..., 0]).astype(np.uint64)
    return np.stack([lo, hi], axis=-1)


def neg128(a):
    with np.errstate(over="ignore"):
        lo = ~a[..., 0] + np.uint64(1)
        hi = ~a[..., 1] + (lo == 0).astype(np.uint64)
    return np.stack([lo, hi], axis=-1)


def monomial_mul128(poly, degree):
    """(N, 2) words * X^degree mod X^N + 1, 0 <= degree < N."""
    out = np.roll(poly, degree, axis=0)
    out[:degree] = neg128(out[:degree])
    return out


def packing_keyswitch128_ref(pksk, lwe, k, n, base_log, level, lwe_per_glwe, rounded=True):
    """lwe (n_lwe, in_dim + 1, 2) -> (ceil(n_lwe / lwe_per_glwe), k + 1, N, 2): every chunk of lwe_per_glwe
    ciphertexts packed into one GLWE (:296-379)."""
    return pack_rows128(single_keyswitch_rows128(pksk, lwe, k, n, base_log, level, rounded), k, n, lwe_per_glwe)


def pack_rows128(rows, k, n, lwe_per_glwe):
    """The list form's rotate-and-sum (:369-378) of keyswitched rows (n_lwe, (k + 1) N, 2)."""
    assert lwe_per_glwe <= n
    rows = rows.reshape(-1, k + 1, n, 2)
    n_lwe = rows.shape[0]
    out = np.zeros(((n_lwe + lwe_per_glwe - 1) // lwe_per_glwe, k + 1, n, 2), np.uint64)
    for i in range(n_lwe):
        g, d = divmod(i, lwe_per_glwe)
        for p in range(k + 1):
            out[g, p] = add128(out[g, p], monomial_mul128(rows[i, p], d))
    return out


# ---- compression -------------------------------------------------------------------------------------------------------

def modulus_switch128(x, log_modulus):
    """fft_impl/common.rs:10-23 at Scalar = u128: the identity at log_modulus = 128."""
    if log_modulus == 128:
        return x
    return ((x + (1 << (128 - log_modulus - 1))) & MASK128) >> (128 - log_modulus)


def pack128_ref(values, log_modulus):
    """PackedIntegers::<u128>::pack (packed_integers.rs:39-130): values < 2^log_modulus -> ceil(len * log_modulus /
    128) u128, as Python ints."""
    big = 0
    for j, v in enumerate(values):
        big |= int(v) << (j * log_modulus)
    return [(big >> (128 * i)) & MASK128 for i in range((len(values) * log_modulus + 127) // 128)]


def pack128_loop(values, log_modulus):
    """The reference's own loop (packed_integers.rs:89-121) at Scalar::BITS = 128, for checking pack128_ref."""
    values = [int(v) for v in values]
    out = []
    for i in range((len(values) * log_modulus + 127) // 128):
        j = 128 * i // log_modulus
        value = values[j] >> (i * 128 - j * log_modulus)
        j += 1
        while j * log_modulus < (i + 1) * 128 and j < len(values):
            value |= (values[j] << (j * log_modulus - i * 128)) & MASK128
            j += 1
        out.append(value)
    return out


def unpack128_ref(packed, count, log_modulus):
    """PackedIntegers::<u128>::unpack (packed_integers.rs:132-222)."""
    big = 0
    for i, w in enumerate(packed):
        big |= int(w) << (128 * i)
    mask = (1 << log_modulus) - 1
    return [(big >> (j * log_modulus)) & mask for j in range(count)]


def compress128_ref(glwe, k, n, bodies_count, log_modulus):
    """CompressedModulusSwitchedGlweCiphertext::compress (compressed_modulus_switched_glwe_ciphertext.rs:169-220) of
    one GLWE ((k + 1) N ints): the packed u128 words as ints."""
    return pack128_ref([modulus_switch128(v, log_modulus) for v in glwe[:k * n + bodies_count]], log_modulus)


def extract128_ref(packed, k, n, bodies_count, log_modulus):
    """::extract (:226-256): (k + 1) N ints, the body polynomial zero past bodies_count."""
    vals = unpack128_ref(packed, k * n + bodies_count, log_modulus)
    return [(v << (128 - log_modulus)) & MASK128 for v in vals] + [0] * (n - bodies_count)


# ---- keys, recodings -----------------------------------------------------------------------------------------------------

def pksk128_gen(g, in_sk, glwe_sk, base_log, level, noise_log2):
    """LwePackingKeyswitchKey<u128> as nested lists (in_dim, level, k + 1, N): block i, entry li is a GLWE encryption
    under glwe_sk of the constant polynomial s_in[i] << (128 - base_log * (level - li))
    (lwe_packing_keyswitch_key_generation.rs:129-156: levels level_count down to 1)."""
    n = len(glwe_sk[0])
    return [[R.glwe_encrypt(g, [(s << (128 - base_log * (level - li))) & MASK128] + [0] * (n - 1), glwe_sk, noise_log2)
             for li in range(level)] for s in in_sk]


def lwe_encrypt_u128(g, pt, lwe_sk, noise_log2=None):
    """A native-modulus u128 LWE (list of ints) of plaintext pt; noise-free when noise_log2 is None."""
    a = R.uniform_u128(g, len(lwe_sk))
    e = int(g.integers(-(1 << noise_log2), (1 << noise_log2) + 1)) if noise_log2 is not None else 0
    return a + [(sum(x for x, s in zip(a, lwe_sk) if s) + pt + e) & MASK128]


def signed_bytes(x, count):
    """The GEMM's recoding: x = sum_t s_t 2^(8t) mod 2^(8 count), s_t in [-128, 127]."""
    out, carry = [], 0
    for t in range(count):
        v = ((x >> (8 * t)) & 255) + carry
        carry = 1 if v >= 128 else 0
        out.append(v - 256 * carry)
    return out


def from_signed_bytes(bytes_, bits=128):
    return sum(s << (8 * t) for t, s in enumerate(bytes_)) & ((1 << bits) - 1)
