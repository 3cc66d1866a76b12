"""The multi-bit 128-bit programmable bootstrap on integers (host only, test infrastructure).

Built on ``pbs128_helpers`` (SignedDecomposer<u128>, the exact product, seeded u128 keys) and ``multi_bit_helpers`` (the
selection bits and key-bit products of a multi-bit key), both unchanged.  Reference paths relative to
tfhe/src/core_crypto/algorithms/lwe_multi_bit_programmable_bootstrapping.rs:

* ``subset_degrees``   modulus_switch_multi_bit :30-51 (StandardMultiBitModulusSwitchedCt): the standard switch of the
                       wrapping sum of the mask elements GGSW ``idx`` selects; ``per_element_degrees`` is the mutant
                       that switches each element before summing
* ``bundle``           std_prepare_multi_bit_ggsw :1849-2255 on Python integers: G_0 + sum_idx X^(d_idx) G_idx mod 2^128
                       (``monomial_mul`` and wrapping adds); ``bundle_words`` the same on (lo, hi) uint64 words in numpy,
                       pinned to it by tests/test_pbs128_multi_bit_helpers.py
* ``step``             acc <- 0 + bundle (.) acc: ``external_product`` into zeros (not a CMUX)
* ``blind_rotate`` / ``pbs``  multi_bit_f128_deterministic_blind_rotate_assign /
                       multi_bit_programmable_bootstrap_f128_lwe_ciphertext :2257-2700 with the exact product in place of
                       the reference's f128 FFT
* ``bsk_gen`` / ``gadget_key``  a multi-bit key at u128: ``ggsw_encrypt`` (or the noise-free gadget GGSW) of the key-bit
                       products
* ``limb_rule``        the limb rule of mi_pbs128_multi_bit_limb_plan in big integers

A key is a nested list [group][idx] of GGSWs (level, k + 1, k + 1, N lists of ints) or, for the word forms, a uint64
array (n / g, 2^g, level, k + 1, k + 1, N, 2).
"""
import numpy as np

import multi_bit_helpers as MB
import pbs128_helpers as R

U64 = np.uint64


# ---- degrees ----------------------------------------------------------------------------------------------------------

def subset_degrees(mask_group, g, log_mod):
    """2^g degrees in [0, 2^log_mod) of one group's g mask elements (ints): entry idx is the switch of the wrapping sum
    of the elements idx selects; entry 0 is 0 (GGSW 0 is not rotated)."""
    out = [0] * (1 << g)
    for idx in range(1, 1 << g):
        s = sum(a for a, bit in zip(mask_group, MB.selection_bits(idx, g)) if bit) & R.MASK64
        out[idx] = R.modulus_switch(s, log_mod) % (1 << log_mod)
    return out


def per_element_degrees(mask_group, g, log_mod):
    """The mutant: every element switched on its own, the switched values summed mod 2^log_mod."""
    sw = [R.modulus_switch(a, log_mod) for a in mask_group]
    return [sum(v for v, bit in zip(sw, MB.selection_bits(idx, g)) if bit) % (1 << log_mod) for idx in range(1 << g)]


def selected_index(key_bits):
    """The GGSW of a group whose key-bit product is 1: bit_m(idx) = s[m]."""
    g = len(key_bits)
    return sum(int(b) << (g - 1 - m) for m, b in enumerate(key_bits))


# ---- the bundle ---------------------------------------------------------------------------------------------------------

def bundle(group, degrees):
    """G_0 + sum_idx X^(degrees[idx]) G_idx mod 2^128 over a group of 2^g GGSWs (nested lists), on Python integers."""
    out = [[[list(p) for p in row] for row in lvl] for lvl in group[0]]
    for idx in range(1, len(group)):
        for li, lvl in enumerate(group[idx]):
            for r, row in enumerate(lvl):
                for c, poly in enumerate(row):
                    rot = R.monomial_mul(poly, degrees[idx])
                    out[li][r][c] = [(x + y) & R.MASK128 for x, y in zip(out[li][r][c], rot)]
    return out


def _neg_words(w):
    lo = ~w[..., 0] + U64(1)
    hi = ~w[..., 1] + (lo == 0).astype(U64)
    return np.stack([lo, hi], axis=-1)


def _add_words(a, b):
    lo = a[..., 0] + b[..., 0]
    hi = a[..., 1] + b[..., 1] + (lo < a[..., 0]).astype(U64)
    return np.stack([lo, hi], axis=-1)


def monomial_mul_words(p, d):
    """X^d p mod (X^N + 1, 2^128) on words: p (..., N, 2) uint64, d in [0, 2N)."""
    n = p.shape[-2]
    src = (np.arange(n) - int(d)) % (2 * n)
    sel = p[..., src % n, :]
    with np.errstate(over="ignore"):
        return np.where((src >= n)[:, None], _neg_words(sel), sel)


def bundle_words(group_words, degrees):
    """``bundle`` on a (2^g, level, k + 1, k + 1, N, 2) uint64 array."""
    out = group_words[0].copy()
    with np.errstate(over="ignore"):
        for idx in range(1, group_words.shape[0]):
            out = _add_words(out, monomial_mul_words(group_words[idx], degrees[idx]))
    return out


def packed_bundle(group_words, degrees, base_log):
    """The bundle as a pbs128_helpers.PackedGgsw, its word form already in place."""
    words = np.ascontiguousarray(bundle_words(group_words, degrees))
    packed = R.PackedGgsw(R.from_words(words), base_log)
    packed._words = words
    return packed


# ---- the step, blind rotation and PBS -------------------------------------------------------------------------------------

def step(acc, mask_group, group_words, base_log, level, g, degrees=subset_degrees):
    """One multi-bit step: 0 + bundle (.) acc for acc (k + 1 lists of N u128) and the group's g mask elements."""
    n = len(acc[0])
    deg = degrees(mask_group, g, n.bit_length())
    out = [[0] * n for _ in acc]
    R.external_product(out, packed_bundle(group_words, deg, base_log), acc, level)
    return out


def blind_rotate(acc, lwe, key_words, base_log, level, g, degrees=subset_degrees):
    """acc / X^ms(body), then one step per group; lwe: n + 1 u64 ints at the native modulus, key_words
    (n / g, 2^g, level, k + 1, k + 1, N, 2)."""
    n = len(acc[0])
    assert (len(lwe) - 1) == g * key_words.shape[0] and key_words.shape[1] == 1 << g
    body = R.modulus_switch(lwe[-1], n.bit_length()) % (2 * n)
    acc = [R.monomial_div(p, body) for p in acc]
    for i in range(key_words.shape[0]):
        acc = step(acc, lwe[i * g:(i + 1) * g], key_words[i], base_log, level, g, degrees)
    return acc


def pbs(lut, lwe, key_words, base_log, level, g):
    """The extracted LWE (k N + 1 u128) of the rotated LUT."""
    return R.sample_extract(blind_rotate([list(p) for p in lut], lwe, key_words, base_log, level, g))


# ---- keys ---------------------------------------------------------------------------------------------------------------

def uniform_key_words(rng, n_groups, g, k, n, level):
    """A key of uniform u128 GGSWs, as words."""
    return rng.integers(0, R.M64, size=(n_groups, 1 << g, level, k + 1, k + 1, n, 2), dtype=U64)


def bsk_gen(rng, lwe_sk, glwe_sk, base_log, level, noise_log2, g):
    """[group][idx] = ggsw_encrypt of prod_m (s[i g + m] XOR NOT bit_m(idx))."""
    bits = MB.combined_key_bits(lwe_sk, g)
    return [[R.ggsw_encrypt(rng, int(m), glwe_sk, base_log, level, noise_log2) for m in row] for row in bits]


def gadget_key(lwe_sk, k, n, base_log, level, g):
    """The noise-free multi-bit key whose GGSWs are gadget GGSWs of the key-bit products."""
    bits = MB.combined_key_bits(lwe_sk, g)
    return [[R.gadget_ggsw(int(m), k, n, base_log, level) for m in row] for row in bits]


def key_words(key):
    return np.ascontiguousarray(R.to_words(key))


# ---- the corner corpus of the degrees ---------------------------------------------------------------------------------------

def edge_words(t, log_mod):
    """The smallest and the largest u64 that the standard switch sends to degree t."""
    unit = 1 << (64 - log_mod)
    return (t * unit - unit // 2) & R.MASK64, (t * unit + unit // 2 - 1) & R.MASK64


def corner_mask_groups(g, n, rng):
    """Mask groups (lists of g u64 ints) for a group's degrees: for each of the degrees 0, 1, N - 1, N, N + 1, 2N - 1 and
    each rounding edge, one group whose first element sits on that edge and whose full sum sits on the same edge of the
    next degree of the list (the elements between are random, the last one makes the sum); then the groups where every
    element lies just under half a switching unit, so that each switches to 0 and every sum of two or more does not.
    Returns (groups, the index of the first half-unit group)."""
    log_mod = n.bit_length()
    unit = 1 << (64 - log_mod)
    targets = [0, 1, n - 1, n, n + 1, 2 * n - 1]
    groups = []
    for j, t in enumerate(targets):
        for edge in (0, 1):
            first = edge_words(t, log_mod)[edge]
            total = edge_words(targets[(j + 1) % len(targets)], log_mod)[edge]
            mid = [int(v) for v in rng.integers(0, R.M64, size=g - 2, dtype=U64)]
            groups.append([first] + mid + [(total - first - sum(mid)) & R.MASK64])
    first_half = len(groups)
    groups.append([unit // 2 - 1] * g)
    groups.append([unit // 2 - 1 - m for m in range(g)])
    return groups, first_half


# ---- the limb rule ------------------------------------------------------------------------------------------------------

def limb_rule(n, k, base_log, level, g):
    """(w, n_limbs): the largest w with 2^g R N 2^(B-1) (2^w - 1) <= (p - 1) / 2, R = (k + 1) level; n_limbs =
    ceil(128 / w), (0, 0) when no width fits."""
    d = (1 << g) * (k + 1) * level * n * (1 << (base_log - 1))
    w = 0
    while d * ((1 << (w + 1)) - 1) <= (R.P - 1) // 2:
        w += 1
    return (w, -(-128 // w)) if w else (0, 0)
