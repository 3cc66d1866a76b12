"""The modulus switch and the negacyclic monomial rotation on big integers, and the corner corpus every rotation test
feeds (host only).

Reference paths are relative to tfhe/src/core_crypto.

* ``py_modulus_switch`` (fft_impl/common.rs:10-23), ``py_ms_non_native`` (algorithms/lwe_programmable_bootstrapping/
  ntt64_pbs.rs:540-549 with algorithms/misc.rs:6-18 divide_round), ``py_centered_correction`` (algorithms/
  modulus_switch.rs:60-104), ``py_monomial_mul`` / ``py_monomial_div`` (algorithms/polynomial_algorithms.rs:395-507),
  ``py_sample_extract`` (algorithms/glwe_sample_extraction.rs:89-160 at degree 0) and ``py_blind_rotate`` (the blind
  rotation under a noiseless key): statement by statement on Python integers, written from the reference's text and
  independent of oracle/.
* ``degrees`` / ``native_words`` / ``nonnative_words`` / ``centered_mask`` / ``centered_bodies``: the inputs at which a
  rotation can go wrong and a uniform random word lands with probability about 1 / 2N: both rounding edges of the degrees
  0, 1, N - 1, N, N + 1, 2N - 1, the words that round past the top, the parities and signs of the centered correction's two
  truncating divisions, and bodies on both sides of a cell edge after the correction.
* ``roll_batch``: item b's mask is the mask corpus rolled by b, so every key position meets every special word.

The native switch adds the half unit with wrapping_add, so the word 2^64 - u/2 (the low edge of degree 0) switches to 0:
the native switch never returns 2^log.  The non-native switch does return 2N for the top words of [0, q), and
``py_monomial_mul`` / ``py_monomial_div`` accept it (X^2N = 1).
"""
import numpy as np

M64 = 1 << 64
P = 0xFFFFFFFF00000001
KINDS = ("hed_zero", "hed_odd_positive", "hed_odd_negative", "sum_half_wraps")


def _signed(v, bits=64):
    return v - (1 << bits) if v >> (bits - 1) else v


def trunc_div2(v):
    """Rust's signed `v / 2`: rounds toward zero (Python's // floors)."""
    return -((-v) // 2) if v < 0 else v // 2


# ---- reference functions -------------------------------------------------------------------------------------------
def py_modulus_switch(x, log, bits=64):
    """modulus_switch of a `bits`-bit word: (x wrapping_add 2^(bits - log - 1)) >> (bits - log), in [0, 2^log)."""
    if log == bits:
        return x
    return ((x + (1 << (bits - log - 1))) % (1 << bits)) >> (bits - log)


def py_ms_non_native(x, n, q):
    """pbs_modulus_switch_non_native: divide_round(x * 2N, q), in [0, 2N] (2N is kept, the rotation folds it)."""
    div, rem = divmod(x * 2 * n, q)
    return div + (1 if rem >= (q >> 1) else 0)


def centered_sums(mask, log, bits=64):
    """(sum_half_mask_round_errors before the halving fix, as a wrapping word; sum_halving_errors_doubled, signed)."""
    mod = 1 << bits
    sum_half, hed = 0, 0
    for a in mask:
        rounded = (py_modulus_switch(a, log, bits) << (bits - log)) % mod
        err = _signed((rounded - a) % mod, bits)
        half = trunc_div2(err)
        hed += 2 * half - err
        sum_half = (sum_half + half) % mod
    return sum_half, hed


def py_centered_correction(mask, log, bits=64):
    """centered_binary_ms_body_correction_to_add: the word added to the body before it is switched."""
    sum_half, hed = centered_sums(mask, log, bits)
    return (sum_half - trunc_div2(hed) - (1 << (bits - log - 1))) % (1 << bits)


def py_switch_lwe(lwe, log, centered=False, bits=64):
    """The switched mask and body as the lazy switched ciphertext reads them (entities/
    modulus_switched_lwe_ciphertext.rs:150-172)."""
    mask, body = list(lwe[:-1]), lwe[-1]
    corr = py_centered_correction(mask, log, bits) if centered else 0
    return [py_modulus_switch(a, log, bits) for a in mask] + [py_modulus_switch((body + corr) % (1 << bits), log, bits)]


def _neg(v, q):
    return (-v) % (q or M64)


def py_monomial_mul(poly, d, q=0):
    """polynomial_wrapping_monic_monomial_mul: poly * X^d mod (X^N + 1) for d in [0, 2N]; q = 0 means 2^64."""
    n = len(poly)
    full, rem = (d // n) % 2, d % n
    return [_neg(poly[(e - rem) % n], q) if full ^ (e < rem) else poly[(e - rem) % n] for e in range(n)]


def py_monomial_div(poly, d, q=0):
    """polynomial_wrapping_monic_monomial_div: poly / X^d for d in [0, 2N]."""
    n = len(poly)
    full, rem = (d // n) % 2, d % n
    return [_neg(poly[(m + rem) % n], q) if full ^ (m >= n - rem) else poly[(m + rem) % n] for m in range(n)]


def py_sample_extract(glwe, q=0):
    """extract_lwe_sample_from_glwe_ciphertext at MonomialDegree(0): glwe is k + 1 lists of N; returns k N + 1 words."""
    out = []
    for poly in glwe[:-1]:
        n = len(poly)
        out += [poly[0]] + [_neg(poly[n - j], q) for j in range(1, n)]
    return out + [glwe[-1][0]]


def py_steps_non_native(mask, n, q):
    """The CMUX steps blind_rotate_ntt64_assign runs (ntt64_pbs.rs:257): [(index, degree)] of every mask word that is not
    raw 0.  A non-zero word that switches to 0 (x = 1) is a step with ct1 - ct0 = 0, not a skip."""
    return [(i, py_ms_non_native(x, n, q)) for i, x in enumerate(mask) if x != 0]


def py_steps_native(mask, log):
    """The steps of blind_rotate_ntt64_bnf_assign (ntt64_bnf_pbs.rs:241): the switched value decides the skip."""
    return [(i, py_modulus_switch(x, log)) for i, x in enumerate(mask) if py_modulus_switch(x, log) != 0]


def py_rotation_degree(switched, bits, n):
    """The exponent of the blind rotation under secret bits `bits`: sum bits_i a_i - body mod 2N."""
    return (sum(a for a, s in zip(switched[:-1], bits) if s) - switched[-1]) % (2 * n)


def py_blind_rotate(acc, switched, bits, q=0):
    """The blind rotation of acc (k + 1 lists of N) by the switched LWE under a noiseless key of secret bits `bits`:
    acc * X^(sum bits_i a_i - body), every CMUX step selecting exactly (one multiplication by the total degree;
    test_rotation_corners.py checks it against the step-by-step divisions and multiplications)."""
    d = py_rotation_degree(switched, bits, len(acc[0]))
    return [py_monomial_mul(p, d, q) for p in acc]


def py_blind_rotate_stepwise(acc, switched, bits, q=0):
    """The same, as the reference runs it: the division by X^body, then one multiplication per set bit."""
    acc = [py_monomial_div(p, switched[-1], q) for p in acc]
    for a, s in zip(switched[:-1], bits):
        if s:
            acc = [py_monomial_mul(p, a, q) for p in acc]
    return acc


# ---- the corpus ----------------------------------------------------------------------------------------------------
def degrees(n):
    """0, 1, N - 1, N, N + 1, 2N - 1, one seeded value inside (1, N - 1) and one inside (N + 1, 2N - 1)."""
    g = np.random.default_rng(n)
    return [0, 1, n - 1, n, n + 1, 2 * n - 1, int(g.integers(2, n - 1)), int(g.integers(n + 2, 2 * n - 1))]


def unit(n, bits=64):
    """The distance between two words that switch to neighbouring degrees: 2^(bits - log2(2N))."""
    return 1 << (bits - n.bit_length())


def native_words(n, bits=64):
    """[(word, degree it switches to, kind)] for every degree: the grid point d u, the low edge d u - u/2 (the tie,
    which rounds up; for d = 0 it is 2^bits - u/2, which wraps to 0) and the high edge d u + u/2 - 1."""
    u, mod = unit(n, bits), 1 << bits
    out = []
    for d in degrees(n):
        out += [(d * u, d, "grid"), ((d * u - u // 2) % mod, d, "low"), (d * u + u // 2 - 1, d, "high")]
    return out


def nonnative_range(d, n, q):
    """The smallest and largest x in [0, q) with divide_round(x 2N, q) == d (d in [0, 2N]), from the formula: the result
    is d iff d q - ceil(q / 2) <= x 2N < d q + (q >> 1)... with divide_round's own tie (rem >= q >> 1 rounds up)."""
    lo = max(0, -((-(d * q - (q - (q >> 1)))) // (2 * n)))          # ceil((d q - (q - q >> 1)) / 2N)
    hi = min(q - 1, (d * q + (q >> 1) - 1) // (2 * n))               # floor((d q + (q >> 1) - 1) / 2N)
    return lo, hi


def nonnative_words(n, q=P):
    """[(x, value the switch returns, kind)]: both ends of every degree's interval; x = 0 (the step is skipped);
    x = 1 (switches to 0 but is not skipped: ct1 - ct0 = 0); the top of [0, q), which switches to 2N = 0 mod 2N."""
    out = [(0, 0, "zero"), (1, 0, "one")]
    for d in degrees(n):
        lo, hi = nonnative_range(d, n, q)
        out += [(max(lo, 1) if d == 0 else lo, d, "low"), (hi, d, "high")]
    lo, hi = nonnative_range(2 * n, n, q)
    out += [(lo, 2 * n, "low"), (hi, 2 * n, "high")]
    return out


def centered_mask(n, length, kind, seed=0, corner_words=(), bits=64):
    """A mask of `length` words for the centered switch at log2(2N).  All but `corner_words` (placed at seeded positions)
    have |a| <= u/2 - 2 and switch to 0 (on BNF their steps are skipped, so a long mask is cheap).  With a = +t the
    rounding error is -t, with a = -t it is +t; an odd t contributes +1 resp. -1 to sum_halving_errors_doubled.  The small
    words' parities are then set so that the total is
      hed_zero: 0      hed_odd_positive: +3 (+1 at length < 8)      hed_odd_negative: -3 (-1): truncation != floor
      sum_half_wraps: 0, the small words positive, so their half errors are negative and the u64 sum wraps below 0
    (hed_zero has the small words negative: the sum stays in [0, 2^63)); the few words that fix the parity take the
    sign the fix needs."""
    assert kind in KINDS
    g = np.random.default_rng([n, length, KINDS.index(kind), seed])
    u, mod = unit(n, bits), 1 << bits
    log = n.bit_length()
    corner_words = list(corner_words) if length >= len(corner_words) + 8 else []
    t = [2 * int(x) for x in g.integers(1, u // 4 - 1, size=length)]           # even, in [2, u/2 - 4]
    if kind == "sum_half_wraps":
        sign = [1] * length
    elif kind == "hed_zero":
        sign = [-1] * length
    else:
        sign = [int(s) for s in g.choice([-1, 1], size=length)]
    slots = [int(i) for i in g.permutation(length)]
    mask = [(s * x) % mod for s, x in zip(sign, t)]
    for w in corner_words:
        mask[slots.pop()] = w
    want = {"hed_zero": 0, "sum_half_wraps": 0, "hed_odd_positive": 3 if length >= 8 else 1,
            "hed_odd_negative": -3 if length >= 8 else -1}[kind]
    need = want - centered_sums(mask, log, bits)[1]
    for _ in range(abs(need)):                                              # at most a few words, sign as needed
        i = slots.pop()
        tt = t[i] + 1
        mask[i] = tt if need > 0 else mod - tt                              # +t adds +1, -t adds -1
    assert centered_sums(mask, log, bits)[1] == want
    return mask


def centered_bodies(n, corr, bits=64):
    """[(body, degree)] around every cell edge after the correction: body + corr = d u - u/2 is the tie and switches to
    d; one less switches to d - 1.  d = 0 is the edge at 2^bits: 2^bits - u/2 wraps to 0, one less gives 2N - 1."""
    u, mod = unit(n, bits), 1 << bits
    out = []
    for d in degrees(n):
        edge = (d * u - u // 2 - corr) % mod
        out += [(edge, d), ((edge - 1) % mod, (d - 1) % (2 * n))]
    return out


def roll_batch(mask_words, body_words):
    """(len(body_words), len(mask_words) + 1) u64: item b's mask is the mask corpus rolled by b, its body is body word b."""
    m = len(mask_words)
    rows = [[mask_words[(i + b) % m] for i in range(m)] + [body] for b, body in enumerate(body_words)]
    return np.array(rows, dtype=np.uint64)


def standard_batch(n, q=0, extra_bodies=0):
    """The corpus batch of the standard switch: masks and bodies are the native words (q = 0) or the non-native words."""
    words = [w for w, _, _ in (nonnative_words(n, q) if q else native_words(n))]
    bodies = words + words[:extra_bodies]
    return roll_batch(words, bodies)


def centered_batch(n, kind, seed=0):
    """The corpus batch of the centered switch: the mask is the native words plus twelve small words of the given kind;
    the bodies are centered_bodies for that mask's correction (the correction is a sum, so every rolled item shares it),
    then the native grid words."""
    corners = [w for w, _, _ in native_words(n)]
    mask = centered_mask(n, len(corners) + 12, kind, seed, corners)
    corr = py_centered_correction(mask, n.bit_length())
    bodies = [b for b, _ in centered_bodies(n, corr)] + [w for w, _, k in native_words(n) if k == "grid"]
    return roll_batch(mask, bodies)


def corner4(n, bits=64):
    """Four words that do not switch to 0, for the long centered masks: the tie below N, the high edge of N, the tie
    past the top (wraps to 0 after rounding, error + u/2) and the grid point N - 1."""
    u, mod = unit(n, bits), 1 << bits
    return [(n * u - u // 2) % mod, n * u + u // 2 - 1, mod - u // 2, (n - 1) * u]


def centered_length_batch(n, length, bits=64):
    """Sixteen ciphertexts of mask length `length` for the strided reduction of a device copy of the correction: item b
    has a centered_mask of kind b % 4 (with corner4 once the mask is long enough) and a body on one side of a cell edge
    after its own correction, degrees and sides cycling against the kinds."""
    rows_ = []
    for b in range(16):
        mask = centered_mask(n, length, KINDS[b % 4], b // 4, corner4(n, bits), bits)
        bodies = centered_bodies(n, py_centered_correction(mask, n.bit_length(), bits), bits)
        rows_.append(mask + [bodies[(b + b // 4) % len(bodies)][0]])
    return np.array(rows_, dtype=np.uint64)


def length_cases(width):
    """The mask lengths around a reduction of `width` threads: one pass, the last lane idle, exact, one lane twice,
    every lane twice and three lanes three times."""
    return [1, width - 1, width, width + 1, 2 * width + 3]


def pre_switched_batch(n):
    """Switched values given directly: every corner degree as mask and body (the header's contract for PRE_SWITCHED is
    [0, 2N), so 2N itself is not sent), three of each so that the mask has the corpus' length."""
    ds = degrees(n)
    mask = [ds[i % len(ds)] for i in range(3 * len(ds))]
    return roll_batch(mask, [ds[(b // 3) % len(ds)] for b in range(3 * len(ds) + 1)])


# ---- the noiseless gadget key and its LUT ----------------------------------------------------------------------------
def gadget_key(bits, k, n, base_log, level):
    """A standard-domain bootstrap key (n_lwe, level, k + 1, k + 1, N) whose GGSW i is the trivial (zero mask, zero
    noise) encryption of bits[i]: the gadget matrix for 1, zero for 0 (level row li holds 2^(64 - B (level - li)))."""
    key = np.zeros((len(bits), level, k + 1, k + 1, n), np.uint64)
    for i, s in enumerate(bits):
        if s:
            for li in range(level):
                for r in range(k + 1):
                    key[i, li, r, r, 0] = np.uint64(1 << (64 - base_log * (level - li)))
    return key


def gadget_lut(k, n, base_log, level, seed, q=0):
    """(k + 1, N) LUT: seeded signed values with magnitude in [2^60, 2^62), rounded to multiples of 2^(64 - B l), so the
    decomposition of every X^a acc - acc (magnitude < 2^63) is exact; modulo q for the non-native modulus."""
    g = np.random.default_rng([seed, n, k, base_log, level])
    step = 1 << (64 - base_log * level)
    mag = g.integers(1 << 60, 1 << 62, size=(k + 1, n), dtype=np.uint64)
    neg = g.integers(0, 2, size=(k + 1, n)).astype(bool)
    rows = []
    for c in range(k + 1):
        row = []
        for m, s in zip(mag[c].tolist(), neg[c].tolist()):
            v = m // step * step                                            # step divides 2^60: still >= 2^60
            row.append((-v if s else v) % (q or M64))
        rows.append(row)
    return np.array(rows, dtype=np.uint64)


def secret_bits(n_lwe, seed):
    """Seeded secret bits with both values present (alternating start, then seeded)."""
    g = np.random.default_rng([seed, n_lwe])
    bits = [int(b) for b in g.integers(0, 2, size=n_lwe)]
    if n_lwe >= 2:
        bits[0], bits[1] = 1, 0
    else:
        bits[0] = 1
    return bits


def rows(a):
    """A (k + 1, N) array as k + 1 lists of Python integers."""
    return [[int(x) for x in r] for r in np.asarray(a)]


def expected_rotation(lut, switched, bits, q=0):
    """(rotated GLWE (k + 1, N), extracted LWE (k N + 1)) as u64 arrays."""
    acc = py_blind_rotate(rows(lut), [int(x) for x in switched], bits, q)
    return np.array(acc, dtype=np.uint64), np.array(py_sample_extract(acc, q), dtype=np.uint64)
