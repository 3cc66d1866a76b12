"""References for the WoP-PBS tests (numpy, host only): the private functional packing keyswitch, its circuit-bootstrap
key list, and the whole bootstrap without padding bit in f64 over oracle/fft_oracle.py.

Reference paths are relative to tfhe/src/core_crypto.

* ``pfpks_ref``: private_functional_keyswitch_lwe_ciphertext_into_glwe_ciphertext
  (algorithms/lwe_private_functional_packing_keyswitch.rs:20-88) on wrapping uint64 arrays, against a key list.
* ``pfpks_ref_oracle``: the same composed from the C oracle's pinned LWE keyswitch (every word of the row, the body
  included, pre-rounded and fed as a mask word; a zero body), fast enough for the large GPU shapes;
  tests/test_wopbs_ref.py pins the two against each other.
* ``pfpksk_gen``: generate_circuit_bootstrap_lwe_pfpksk_list (algorithms/lwe_wopbs.rs:81-155 over
  lwe_private_functional_packing_keyswitch_key_generation.rs:98-130), our own random stream.
* ``extract_bits_ref`` .. ``wop_ref``: fft_impl/fft64/crypto/wop_pbs/mod.rs:61-220, 238-435, 459-583, 771-825, 838-863
  restated on batches.
* ``Shape`` / ``SHAPE_A`` / ``SHAPE_N512`` / ``keys``: the parameter sets and seeded keys the CPU and GPU tests share.
"""
import functools
from collections import namedtuple

import numpy as np

import fft_oracle as F
import packing_helpers as P
import tfhe_helpers as H

U64 = np.uint64


# ---- the private functional packing keyswitch ----------------------------------------------------------------------
def pfpks_ref(key_list, lwe, base_log, level):
    """key_list (n_keys, in_dim + 1, level, k + 1, N), lwe (rows, in_dim + 1) -> (rows, n_keys, k + 1, N):
    out = - sum_i sum_l digit_l(closest_representable(lwe[i])) key[i][l], the body word decomposed like the mask."""
    key_list = np.asarray(key_list, U64)
    n_keys, blocks = key_list.shape[:2]
    lwe = np.asarray(lwe, U64)
    assert lwe.shape[-1] == blocks
    terms = F.decompose(P.pre_round(lwe, base_log, level), base_log, level)   # least significant level first
    digits = np.stack(terms, axis=-1).reshape(lwe.shape[0], blocks * level)   # (rows, (i, l))
    out = np.zeros((lwe.shape[0], n_keys) + key_list.shape[3:], U64)
    with np.errstate(over="ignore"):
        for j in range(n_keys):
            mat = key_list[j].reshape(blocks * level, -1)
            out[:, j] = (U64(0) - digits @ mat).reshape((lwe.shape[0],) + key_list.shape[3:])
    return out


def pfpks_ref_oracle(oracle, key_list, lwe, base_log, level):
    """pfpks_ref through oracle.lwe_keyswitch: the row's in_dim + 1 words pre-rounded as the mask of an LWE of
    dimension in_dim + 1 with a zero body; the keyswitch then subtracts exactly the digit products."""
    key_list = np.asarray(key_list, U64)
    n_keys, blocks = key_list.shape[:2]
    size = int(np.prod(key_list.shape[3:]))
    x = np.zeros((lwe.shape[0], blocks + 1), U64)
    x[:, :blocks] = P.pre_round(np.asarray(lwe, U64), base_log, level)
    out = np.zeros((lwe.shape[0], n_keys, size), U64)
    for j in range(n_keys):
        out[:, j] = oracle.lwe_keyswitch(key_list[j].reshape(blocks, level, size), x, size - 1, base_log, level,
                                         threads=16)
    return out.reshape((lwe.shape[0], n_keys) + key_list.shape[3:])


def pfpksk_gen(g, in_sk, glwe_sk, base_log, level, noise_log2):
    """(k + 1, in_dim + 1, level, k + 1, N): key j < k encrypts, in block i and entry li, the polynomial
    S_j * (-s_i) * 2^(64 - base_log (level - li)); the body block has key bit -1 (so +S_j * 2^..); key k takes the
    constant polynomial -1 for S_j (f = x -> -x)."""
    k, n = glwe_sk.shape
    in_dim = in_sk.size
    bits = np.concatenate([in_sk.astype(U64), np.array([H.M64], U64)])        # the body block: -1
    polys = np.concatenate([glwe_sk.astype(U64), np.zeros((1, n), U64)])
    polys[k, 0] = H.M64
    out = np.zeros((k + 1, in_dim + 1, level, k + 1, n), U64)
    with np.errstate(over="ignore"):
        for j in range(k + 1):
            for li in range(level):
                scale = U64(1 << (64 - base_log * (level - li)))
                pt = (U64(0) - bits)[:, None] * scale * polys[j][None, :]     # f(1) * key bit = -bit
                mask = H.uniform_u64(g, (in_dim + 1, k, n))
                body = pt + H.tuniform(g, (in_dim + 1, n), noise_log2)
                for c in range(k):
                    body += H.negacyclic_mul_binary(mask[:, c], glwe_sk[c])
                out[j, :, li, :k] = mask
                out[j, :, li, k] = body
    return out


# ---- the stages, batched -------------------------------------------------------------------------------------------
def lwe_keyswitch_ref(ksk, lwe, base_log, level):
    """keyswitch_lwe_ciphertext (lwe_keyswitch.rs:137-227): ksk (in_dim, level, out + 1), lwe (rows, in_dim + 1)."""
    in_dim = ksk.shape[0]
    digits = np.stack(F.decompose(lwe[:, :in_dim], base_log, level), axis=-1).reshape(lwe.shape[0], -1)
    with np.errstate(over="ignore"):
        out = U64(0) - digits @ np.asarray(ksk, U64).reshape(in_dim * level, -1)
        out[:, -1] += lwe[:, in_dim]
    return out


def trivial_acc(k, n, value):
    acc = np.zeros((k + 1, n), U64)
    acc[k] = U64(value % 2**64)
    return acc


def extract_bits_ref(lwe_in, ksk, ks_base_log, ks_level, fbsk, base_log, level, k, n, delta_log, n_bits):
    """wop_pbs/mod.rs:61-220 over a batch: (batch, k N + 1) -> (batch, n_bits, small + 1), MSB first."""
    cur = np.asarray(lwe_in, U64).copy()
    out = np.zeros((cur.shape[0], n_bits, ksk.shape[2]), U64)
    with np.errstate(over="ignore"):
        for bit in range(n_bits):
            ks = lwe_keyswitch_ref(ksk, cur << U64(64 - delta_log - bit - 1), ks_base_log, ks_level)
            out[:, n_bits - 1 - bit] = ks
            if bit == n_bits - 1:
                break
            ks[:, -1] += U64(1 << 62)
            boot = F.pbs(ks, trivial_acc(k, n, -(1 << (delta_log - 1 + bit))), fbsk, base_log, level)
            boot[:, -1] += U64(1 << (delta_log + bit - 1))
            cur -= boot
    return out


def circuit_bootstrap_ref(lwe_in, fbsk, base_log, level, k, n, pfpksk, pf_base_log, pf_level, delta_log, base_log_cbs,
                          level_cbs):
    """:238-435 over a batch: (batch, small + 1) -> (batch, level_cbs, n_keys, k' + 1, N') u64, output index 0 =
    decomposition level level_cbs."""
    lwe_in = np.asarray(lwe_in, U64)
    with np.errstate(over="ignore"):
        shifted = lwe_in << U64(63 - delta_log)
        shifted[:, -1] += U64(1 << 62)
    out = []
    for i in range(level_cbs):
        alpha = 1 << (63 - base_log_cbs * (level_cbs - i))
        boot = F.pbs(shifted, trivial_acc(k, n, -alpha), fbsk, base_log, level)
        with np.errstate(over="ignore"):
            boot[:, -1] += U64(alpha)
        out.append(pfpks_ref(pfpksk, boot, pf_base_log, pf_level))
    return np.stack(out, axis=1)


def ext_product_items(glwe, fggsw, base_log, level):
    """F.external_product with one Fourier GGSW per item: glwe (B, k+1, N), fggsw (B, level, k+1, k+1, N/2)."""
    acc = 0
    for li, term in enumerate(F.decompose(glwe, base_log, level)):
        acc = acc + np.einsum("brm,brcm->bcm", F.forward_as_integer(term), fggsw[:, li])
    return F.backward_as_torus(acc)


def cmux_items(ct0, ct1, fggsw, base_log, level):
    with np.errstate(over="ignore"):
        return ct0 + ext_product_items(ct1 - ct0, fggsw, base_log, level)


def cmux_tree_ref(luts, fggsw, base_log, level, k):
    """:459-583: luts (2^r, N) shared, fggsw (B, r, level, k+1, k+1, N/2): the last GGSW selects the first layer."""
    bsz, r = fggsw.shape[0], fggsw.shape[1]
    n = luts.shape[-1]
    nodes = np.zeros((bsz, luts.shape[0], k + 1, n), U64)
    nodes[:, :, k] = luts
    for j in range(r):
        g = fggsw[:, r - 1 - j]
        half = nodes.shape[1] // 2
        t0, t1 = nodes[:, 0::2].reshape(-1, k + 1, n), nodes[:, 1::2].reshape(-1, k + 1, n)
        gg = np.repeat(g[:, None], half, axis=1).reshape((-1,) + g.shape[1:])
        nodes = cmux_items(t0, t1, gg, base_log, level).reshape(bsz, half, k + 1, n)
    return nodes[:, 0]


def monomial_div(p, d):
    """polynomial_wrapping_monic_monomial_div_assign of every polynomial of p (..., N) by X^d (full-cycle rule)."""
    n = p.shape[-1]
    d %= 2 * n
    full, rem = d // n, d % n
    out = np.roll(p, -rem, axis=-1).copy()
    with np.errstate(over="ignore"):
        if rem:
            out[..., n - rem:] = U64(0) - out[..., n - rem:]
        if full:
            out = U64(0) - out
    return out


def blind_rotate_ref(glwe, fggsw, base_log, level):
    """:838-863: glwe (B, k+1, N), fggsw (B, n_rot, level, ...)."""
    d = 1
    for i in reversed(range(fggsw.shape[1])):
        glwe = cmux_items(glwe, monomial_div(glwe, d), fggsw[:, i], base_log, level)
        d <<= 1
    return glwe


def sample_extract0(glwe):
    """extract_lwe_sample_from_glwe_ciphertext at degree 0: (B, k+1, N) -> (B, k N + 1)."""
    bsz, kp1, n = glwe.shape
    out = np.zeros((bsz, (kp1 - 1) * n + 1), U64)
    with np.errstate(over="ignore"):
        for c in range(kp1 - 1):
            out[:, c * n] = glwe[:, c, 0]
            out[:, c * n + 1:(c + 1) * n] = U64(0) - glwe[:, c, :0:-1]
    out[:, -1] = glwe[:, kp1 - 1, 0]
    return out


def vertical_packing_ref(luts, fggsw, base_log, level, k):
    """:771-825 for one output: luts (n_polys, N), fggsw (B, n_ggsw, level, ...) -> (B, k N + 1)."""
    n_polys, n_ggsw = luts.shape[0], fggsw.shape[1]
    r = n_polys.bit_length() - 1
    if r > n_ggsw:
        r = 0
    assert n_polys == 1 << r
    acc = cmux_tree_ref(luts, fggsw[:, :r], base_log, level, k)
    return sample_extract0(blind_rotate_ref(acc, fggsw[:, r:], base_log, level))


# ---- the fixed inputs of tests/golden/ks_before_pfpks.npz ------------------------------------------------------------
# The outputs of mi_lwe_keyswitch_batch and mi_lwe_packing_keyswitch_batch on these inputs were recorded from the
# library as it was before the shared GEMM core learnt the private functional packing keyswitch; the core must still
# give the same bits.  (in_dim, out_dim, base_log, level, batch) and (in_dim, k, N, base_log, level, lwe_per_glwe, n_lwe)
GOLDEN_KS = [(70, 33, 4, 2, 300), (45, 20, 7, 3, 17), (20, 40, 23, 2, 5)]
GOLDEN_PKS = [(50, 1, 64, 6, 2, 64, 320), (33, 1, 32, 10, 2, 32, 40)]


def golden_ks_inputs(i):
    in_dim, out_dim, base_log, level, batch = GOLDEN_KS[i]
    g = H.rng(0x601d + i)
    lwe = H.uniform_u64(g, (batch, in_dim + 1))
    ties = P.tie_words(base_log, level)[:in_dim]
    lwe[0, :len(ties)] = ties
    return H.uniform_u64(g, (in_dim, level, out_dim + 1)), lwe


def golden_pks_inputs(i):
    in_dim, k, n, base_log, level, _, n_lwe = GOLDEN_PKS[i]
    g = H.rng(0x901d + i)
    lwe = H.uniform_u64(g, (n_lwe, in_dim + 1))
    ties = P.tie_words(base_log, level)[:in_dim]
    lwe[0, :len(ties)] = ties
    return H.uniform_u64(g, (in_dim, level, k + 1, n)), lwe


# ---- parameter sets and seeded keys --------------------------------------------------------------------------------
Shape = namedtuple("Shape", "name n k N pbs ks pfks cbs noise_log2 seed")
# shape A of the tests; PBS / KS / pfks / cbs are (base_log, level)
SHAPE_A = Shape("A", 8, 1, 256, (9, 4), (4, 7), (15, 2), (6, 4), 10, 0xA0)
# FFT_WOPBS_N512_PARAMS (fft_impl/fft64/crypto/wop_pbs/tests.rs)
SHAPE_N512 = Shape("N512", 4, 2, 512, (9, 4), (4, 7), (15, 2), (6, 4), 10, 0xA1)
# the one-wave engine: N = 2048, k = 1, n = 8
SHAPE_N2048 = Shape("N2048", 8, 1, 2048, (9, 4), (4, 7), (15, 2), (6, 4), 10, 0xA2)

N_INPUT_BITS = 10
MESSAGES_SEED = 0x5eed


@functools.lru_cache(maxsize=None)
def keys(shape):
    """The seeded keys of a shape: small / GLWE secret keys, the standard bootstrap key (n, level, k+1, k+1, N), the
    keyswitch key big -> small, the circuit-bootstrap pfpksk list."""
    g = H.rng(shape.seed)
    small_sk = H.binary_key(g, shape.n)
    glwe_sk = H.binary_key(g, (shape.k, shape.N))
    big_sk = H.glwe_sk_as_lwe_sk(glwe_sk)
    bsk = H.bsk_gen(g, small_sk, glwe_sk, shape.pbs[0], shape.pbs[1], shape.noise_log2)
    ksk = H.ksk_gen(g, big_sk, small_sk, shape.ks[0], shape.ks[1], shape.noise_log2)
    pfpksk = pfpksk_gen(g, big_sk, glwe_sk, shape.pfks[0], shape.pfks[1], shape.noise_log2)
    return {"small_sk": small_sk, "glwe_sk": glwe_sk, "big_sk": big_sk, "bsk": bsk, "ksk": ksk, "pfpksk": pfpksk}


def messages(count=8):
    return [int(v) for v in H.rng(MESSAGES_SEED).integers(0, 1 << N_INPUT_BITS, size=count)]


def add_one_lut(n, n_bits=N_INPUT_BITS, add=1):
    """test_wop_add_one's LUT (tests.rs:852-862): i -> ((i + add) mod 2^n_bits) << (64 - n_bits), as polynomials."""
    size = max(1 << n_bits, n)
    vals = [((i + add) % (1 << n_bits)) << (64 - n_bits) for i in range(size)]
    return np.array(vals, U64).reshape(-1, n)


def encrypt_messages(shape, msgs, n_bits=N_INPUT_BITS):
    """Each message at delta_log = 64 - n_bits under the big key: (len, k N + 1)."""
    ks = keys(shape)
    g = H.rng(shape.seed + 1000)
    return H.lwe_encrypt_batch(g, [m << (64 - n_bits) for m in msgs], ks["big_sk"], shape.noise_log2)


def decode_output(ct, big_sk, n_bits=N_INPUT_BITS):
    """closest_representable(decrypt) >> delta_log (tests.rs:893-902)."""
    pt = H.lwe_decrypt_batch(ct, big_sk)
    with np.errstate(over="ignore"):
        return [int(v) for v in ((pt + U64(1 << (63 - n_bits))) >> U64(64 - n_bits))]


LEAF_BITS = 4  # every leaf of the selection case carries a 4-bit message: half a step is 2^59


def leaf_lut(r, n):
    """(2^r, N): lut[p][c] = ((7 p + c) mod 16) << 60; any two leaves differ in every coefficient while r <= 4."""
    p, c = np.arange(1 << r, dtype=U64)[:, None], np.arange(n, dtype=U64)[None, :]
    return ((U64(7) * p + c) % U64(1 << LEAF_BITS)) << U64(64 - LEAF_BITS)


def leaf_selector_lwes(shape, r):
    """For every m < 2^r its r bits, most significant first, encrypted at delta_log 63 under the small key:
    (2^r * r, n + 1), item m's bits in rows m r .. m r + r - 1.  The tree's last GGSW selects the first layer, so these
    bits select leaf m."""
    bits = [((m >> (r - 1 - j)) & 1) << 63 for m in range(1 << r) for j in range(r)]
    return H.lwe_encrypt_batch(H.rng(shape.seed + 2000 + r), bits, keys(shape)["small_sk"], shape.noise_log2)


def decode_leaves(glwe, glwe_sk):
    """glwe (2^r, k+1, N) -> what each coefficient decodes to at LEAF_BITS bits, (2^r, N), and the largest absolute
    error against leaf m for item m."""
    r = glwe.shape[0].bit_length() - 1
    lut = leaf_lut(r, glwe.shape[-1])
    pt = np.stack([H.glwe_decrypt(g, glwe_sk) for g in glwe])
    with np.errstate(over="ignore"):
        err = int(np.abs((pt - lut).view(np.int64)).max())
        return (pt + U64(1 << (63 - LEAF_BITS))) >> U64(64 - LEAF_BITS), err


def wop_ref(shape, lwe_in, luts_per_output, n_bits=N_INPUT_BITS):
    """Extract bits, circuit bootstrap every bit at delta_log 63, vertical packing of every output's LUT:
    (batch, k N + 1) -> (batch, n_outputs, k N + 1), and the extracted bits."""
    ks = keys(shape)
    fbsk = F.forward_as_torus(ks["bsk"])
    bits = extract_bits_ref(lwe_in, ks["ksk"], *shape.ks, fbsk, *shape.pbs, shape.k, shape.N, 64 - n_bits, n_bits)
    flat = bits.reshape(-1, bits.shape[-1])
    ggsw = circuit_bootstrap_ref(flat, fbsk, *shape.pbs, shape.k, shape.N, ks["pfpksk"], *shape.pfks, 63, *shape.cbs)
    fggsw = F.forward_as_torus(ggsw).reshape((lwe_in.shape[0], n_bits) + ggsw.shape[1:-1] + (shape.N // 2,))
    outs = [vertical_packing_ref(l, fggsw, *shape.cbs, shape.k) for l in luts_per_output]
    return np.stack(outs, axis=1), bits
