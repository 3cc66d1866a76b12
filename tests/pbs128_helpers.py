"""The 128-bit programmable bootstrap on Python integers (host only, test infrastructure).

Reference paths are relative to tfhe/src/core_crypto.

* ``init_decomposer_state`` / ``decompose_one_level`` / ``py_decompose``: SignedDecomposer<u128> in its generic form
  (commons/math/decomposition/decomposer.rs:156-185, iter.rs:131-151); ``split_one_level`` / ``py_decompose_split``:
  the form the u128 path really runs, on (lo, hi) words (fft_impl/fft128_u128/crypto/ggsw.rs:517-567
  collect_next_term_split_scalar, fft128_u128/math/fft/mod.rs:12-60, 192-201).  Both written from the reference's text.
* ``negacyclic_mul``: the exact product in Z_{2^128}[X]/(X^N + 1): the coefficients packed into one big integer each
  (through ``bytes``), one multiplication, then the fold.  No transform anywhere.
* ``external_product`` / ``cmux`` / ``blind_rotate`` / ``pbs``: add_external_product_assign_split, cmux_split
  (fft128_u128/crypto/ggsw.rs:17, :621-675), blind_rotate_assign_split and blind_rotate_u128
  (fft128_u128/crypto/bootstrap.rs:60-247) with that exact product in place of the reference's f128 FFT.
* ``accelerator``: tests/cpp/pbs128_ref.c, the decomposition loop and the schoolbook column sums compiled (unsigned
  __int128, still no transform), which ``external_product`` uses when a C compiler is present so that expected values
  at N = 2048 cost milliseconds; pinned to the Python-integer forms by tests/test_pbs128_oracle.py.
* seeded u128 GLWE / GGSW / bootstrap-key generation and decryption in the manner of tests/tfhe_helpers.py (our own
  random streams: only functional results and parity on identical inputs are compared).
* ``corner_words``: the corner corpus of SignedDecomposer<u128>(base_log, level).

A u128 polynomial is a list of Python ints; ``to_words`` / ``from_words`` convert to the (..., 2) uint64 (lo, hi)
arrays that cross the ABI.
"""
import numpy as np

M64 = 1 << 64
M128 = 1 << 128
MASK64 = M64 - 1
MASK128 = M128 - 1
P = 0xFFFFFFFF00000001


# ---- words ---------------------------------------------------------------------------------------------------------

def to_words(values):
    """Nested lists of u128 ints -> uint64 array (..., 2) of little-endian words."""
    a = np.array(values, dtype=object)
    out = np.empty(a.shape + (2,), np.uint64)
    out[..., 0] = (a & MASK64).astype(np.uint64)
    out[..., 1] = (a >> 64).astype(np.uint64)
    return out


def from_words(words):
    """uint64 array (..., 2) -> nested lists of u128 ints."""
    w = np.asarray(words).astype(np.uint64)
    lo = w[..., 0].astype(object)
    hi = w[..., 1].astype(object)
    return (lo | (hi << 64)).tolist()


# ---- the decomposer, generic form ----------------------------------------------------------------------------------

def _signed128(v):
    return v - M128 if v >> 127 else v


def closest_representable(x, base_log, level):
    """native_closest_representable (decomposer.rs:25-49) of a u128."""
    shift = 128 - base_log * level - 1
    return ((((x >> shift) + 1) & (M128 - 2)) << shift) & MASK128


def init_decomposer_state(x, base_log, level):
    """SignedDecomposer::<u128>::init_decomposer_state (decomposer.rs:156-185)."""
    rep = base_log * level
    res = x >> (128 - rep - 1)
    rounding_bit = res & 1
    res = (res + 1) & MASK128
    res >>= 1
    res &= MASK128 >> (128 - rep)
    need_balance = ((((res - 1) & MASK128) | (rounding_bit << (rep - 1))) & res) >> (rep - 1)
    return (res - (need_balance << rep)) & MASK128


def decompose_one_level(base_log, state):
    """decompose_one_level (iter.rs:131-151) on a u128 state: (term as a u128, next state)."""
    res = state & ((1 << base_log) - 1)
    state = (_signed128(state) >> base_log) & MASK128
    carry = ((((res - 1) & MASK128) | state) & res) >> (base_log - 1)
    state = (state + carry) & MASK128
    return (res - (carry << base_log)) & MASK128, state


def py_decompose(x, base_log, level):
    """The signed digits of a u128, least significant level first (the order the GGSW's level matrices pair with)."""
    state = init_decomposer_state(x, base_log, level)
    terms = []
    for _ in range(level):
        t, state = decompose_one_level(base_log, state)
        terms.append(_signed128(t))
    return terms


# ---- the decomposer, split form (what fft128_u128 runs) ------------------------------------------------------------

def _zeroing_shl(x, s):
    return 0 if s >= 64 else (x << s) & MASK64


def _zeroing_shr(x, s):
    return 0 if s >= 64 else x >> s


def _arithmetic_shr64(x, s):
    sx = x - M64 if x >> 63 else x
    if s >= 64:
        return 0 if sx >= 0 else MASK64
    return (sx >> s) & MASK64


def _arithmetic_shr_split(lo, hi, s):
    """arithmetic_shr_split_u128 (fft128_u128/math/fft/mod.rs:32-58)."""
    res_hi = _arithmetic_shr64(hi, s)
    if s < 64:
        res_lo = _zeroing_shl(hi, 64 - s) | _zeroing_shr(lo, s)
    else:
        res_lo = _arithmetic_shr64(hi, s - 64)
    return res_lo, res_hi


def _wrapping_add(a, b):
    s = a[0] + b[0]
    return s & MASK64, (a[1] + b[1] + (s >> 64)) & MASK64


def _wrapping_sub(a, b):
    borrow = 1 if a[0] < b[0] else 0
    return (a[0] - b[0]) & MASK64, (a[1] - b[1] - borrow) & MASK64


def split_one_level(base_log, state_lo, state_hi):
    """One step of collect_next_term_split_scalar (ggsw.rs:517-567): ((term_lo, term_hi), (state_lo, state_hi))."""
    mask = (1 << base_log) - 1
    res_lo, res_hi = state_lo & (mask & MASK64), state_hi & (mask >> 64)
    state_lo, state_hi = _arithmetic_shr_split(state_lo, state_hi, base_log)
    overflow = 1 if res_lo == 0 else 0
    res_sub1_lo = (res_lo - 1) & MASK64
    res_sub1_hi = (res_hi - overflow) & MASK64
    carry_lo = (res_sub1_lo | state_lo) & res_lo
    carry_hi = (res_sub1_hi | state_hi) & res_hi
    shift = base_log - 1
    if shift < 64:
        carry_lo = _zeroing_shl(carry_hi, 64 - shift) | _zeroing_shr(carry_lo, shift)
        carry_hi = _zeroing_shr(carry_hi, shift)
    else:
        carry_lo = _zeroing_shr(carry_hi, shift - 64)
        carry_hi = 0
    state_lo, state_hi = _wrapping_add((state_lo, state_hi), (carry_lo, carry_hi))
    if base_log < 64:
        carry_hi = _zeroing_shl(carry_hi, base_log) | _zeroing_shr(carry_lo, 64 - base_log)
        carry_lo = _zeroing_shl(carry_lo, base_log)
    else:
        carry_hi = _zeroing_shl(carry_lo, base_log - 64)
        carry_lo = 0
    return _wrapping_sub((res_lo, res_hi), (carry_lo, carry_hi)), (state_lo, state_hi)


def py_decompose_split(x, base_log, level):
    """The same digits through the split form: the state of init_decomposer_state as (lo, hi) words (ggsw.rs:90-101),
    then one split step per level."""
    state = init_decomposer_state(x, base_log, level)
    lo, hi = state & MASK64, state >> 64
    terms = []
    for _ in range(level):
        (t_lo, t_hi), (lo, hi) = split_one_level(base_log, lo, hi)
        terms.append(_signed128(t_lo | (t_hi << 64)))
    return terms


def recompose(terms, base_log, level):
    """sum_l term_l 2^(128 - B (level - l)) mod 2^128 (terms least significant first)."""
    return sum(t << (128 - base_log * (level - j)) for j, t in enumerate(terms)) & MASK128


# ---- the corner corpus ----------------------------------------------------------------------------------------------

def corner_words(base_log, level):
    """The words at which SignedDecomposer<u128>(base_log, level) can go wrong and a uniform word almost never lands
    (in the manner of decomp_corners.corner_words): rounding ties, a digit of exactly +-2^(B-1) at every level, the
    carry through every level, 0, 2^127, 2^128 - 1; values whose rounding carry crosses bit 64; states whose digit
    straddles the word boundary."""
    rep = base_log * level
    step = 1 << (128 - rep)          # distance between representable values
    half = step >> 1                 # the rounding tie
    pos = [128 - rep + j * base_log for j in range(level)]  # bit position of field j (0 = least significant)
    top = 1 << (base_log - 1)        # the field value that ties between +2^(B-1) and -2^(B-1)
    words = [0, MASK128, 1 << 127, (1 << 127) - 1, 1, 1 << 64, MASK64, (1 << 64) + 1]
    for c in (0, 1 << 127, 1 << 64, 1 << 126):
        words += [c + half, c + half - 1, c - half, c - half - 1, c + 1, c + half + 1, c - half + 1, c + step, c - step,
                  c + step + half, c + step + half - 1, c - step - half, c - step - half - 1]
    lows = [0, half, half - 1, -1, -half, -half - 1, step, -step]
    for j in range(level):
        w = top << pos[j]
        nexts = [0, top << pos[j + 1]] if j + 1 < level else [0]
        words += [w + nb + low for nb in nexts for low in lows]
        words += [-w + low for low in lows]
    chain = sum(top << q for q in pos)  # every field 2^(B-1): the carry runs through all levels
    words += [chain, chain + 1, chain - 1, chain + half, chain + half - 1, chain - half, chain - half - 1,
              -chain, -chain + 1, -chain - 1, -chain - half, -chain + half - 1]
    # the rounding carry crosses bit 64: every bit from the tie up to bit 64 (and beyond) set, so that the +1 of the
    # rounding ripples across the word boundary; only meaningful when the tie lies in the low word
    ones_to_64 = (1 << 64) - half if half < M64 else 0
    ones_to_100 = (1 << 100) - half if half < (1 << 100) else 0
    words += [ones_to_64, ones_to_64 - 1, ones_to_64 + (1 << 127), ones_to_100, MASK128 - half + 1, MASK128 - half]
    # states whose digit straddles the word boundary: the field that holds bit 64 at its extremes, the fields around it
    # full, so that the state's arithmetic shift and the carry both move bits between the words
    for j in range(level):
        lo_bit, hi_bit = pos[j], pos[j] + base_log
        if lo_bit < 64 < hi_bit or lo_bit <= 64 <= hi_bit:
            field_max = ((1 << base_log) - 1) << lo_bit
            words += [field_max, field_max + half, field_max - half, top << lo_bit, (top << lo_bit) - 1,
                      (top << lo_bit) + field_max, MASK128 ^ field_max, (1 << 64) - (1 << lo_bit),
                      (1 << 64) + (top << lo_bit), ((top - 1) << lo_bit) | ((1 << lo_bit) - 1)]
    seen, out = set(), []
    for w in words:
        w &= MASK128
        if w not in seen:
            seen.add(w)
            out.append(w)
    return out


def saturating_digits(base_log, level, negative):
    """The digit vector of largest magnitude a u128 can decompose into, least significant level first.  Two adjacent
    levels cannot both be +-2^(B-1): +2^(B-1) needs the next field's top bit clear (no carry), which bounds the next
    digit by 2^(B-1) - 1; -2^(B-1) needs it set and carries into the next field, which then yields at most
    -2^(B-1) + 1.  So the extreme vectors are (2^(B-1), 2^(B-1) - 1, ...) and (-2^(B-1), -2^(B-1) + 1, ...): exactly
    +-2^(B-1) at level count 1."""
    top = 1 << (base_log - 1)
    return [-top] + [-top + 1] * (level - 1) if negative else [top] + [top - 1] * (level - 1)


def saturating_word(base_log, level, negative):
    """A u128 whose decomposition is saturating_digits(base_log, level, negative) (the tests assert that it is)."""
    top = 1 << (base_log - 1)
    pos = [128 - base_log * level + j * base_log for j in range(level)]
    fields = [top] * level if negative else [top] + [top - 1] * (level - 1)
    # negative: every field at the tie and the word just below the rounding tie, so that the lowest field balances
    # downwards (at level count 1 that is the rounding bit of init_decomposer_state)
    tie = (1 << (128 - base_log * level - 1)) if negative else 0
    return (sum(f << q for f, q in zip(fields, pos)) - tie) & MASK128


def saturating_poly(base_log, level, n, kind):
    """N coefficients that put the saturating digits where a column sum is largest: "plus" / "minus": every digit
    positive / negative (coefficient N - 1 of a product with a non-negative polynomial adds every term); "index0": the
    first coefficient positive and the rest negative (coefficient 0 adds every term, the wrapped ones negated)."""
    plus, minus = (saturating_word(base_log, level, neg) for neg in (False, True))
    if kind == "index0":
        return [plus] + [minus] * (n - 1)
    return [plus if kind == "plus" else minus] * n


def corner_poly(words, n, rng, roll=0):
    """n coefficients: the corpus (rolled) on even repetitions, seeded random u128 on odd ones."""
    m = len(words)
    assert n >= m, "the polynomial must hold the whole corpus"
    rnd = uniform_u128(rng, n)
    return [words[(i + roll) % m] if (i // m) % 2 == 0 else rnd[i] for i in range(n)]


# ---- the exact product ----------------------------------------------------------------------------------------------

def _pack(coeffs, slot_bytes):
    """sum_i coeffs[i] 2^(8 slot_bytes i) for non-negative coefficients below 2^(8 slot_bytes)."""
    return int.from_bytes(b"".join(c.to_bytes(slot_bytes, "little") for c in coeffs), "little")


def _unpack(value, count, slot_bytes):
    raw = value.to_bytes(count * slot_bytes, "little")
    return [int.from_bytes(raw[i * slot_bytes:(i + 1) * slot_bytes], "little") for i in range(count)]


def negacyclic_mul(a, b):
    """(a * b) mod (X^N + 1, 2^128) for two lists of N u128: one big-integer multiplication, then the fold."""
    n = len(a)
    slot = (256 + n.bit_length() + 7) // 8
    c = _unpack(_pack(a, slot) * _pack(b, slot), 2 * n, slot)
    return [(c[i] - c[i + n]) & MASK128 for i in range(n)]


def _pack_signed(coeffs, slot_bytes):
    return (_pack([c if c > 0 else 0 for c in coeffs], slot_bytes)
            - _pack([-c if c < 0 else 0 for c in coeffs], slot_bytes))


class PackedGgsw:
    """A standard-domain u128 GGSW (level, k + 1, k + 1, N nested lists) with every polynomial packed once, for
    products with digit polynomials (|d| <= 2^(base_log - 1)).  Slots are wide enough for the signed sum of a whole
    column: 128 + base_log - 1 + log2(R N) bits, a sign bit and a spare one."""

    def __init__(self, ggsw, base_log):
        self.level = len(ggsw)
        self.kp1 = len(ggsw[0])
        self.n = len(ggsw[0][0][0])
        self.base_log = base_log
        rows = self.level * self.kp1
        bits = 128 + base_log - 1 + (rows * self.n).bit_length() + 2
        self.slot = (bits + 7) // 8
        self.offset = _pack([1 << (8 * self.slot - 1)] * (2 * self.n), self.slot)
        self.ggsw = ggsw
        self._packed = self._words = None

    @property
    def packed(self):
        if self._packed is None:
            self._packed = [[[_pack(self.ggsw[li][r][c], self.slot) for c in range(self.kp1)]
                             for r in range(self.kp1)] for li in range(self.level)]
        return self._packed

    def words(self):
        """The GGSW as a contiguous (level, k + 1, k + 1, N, 2) uint64 array (what the ABI takes)."""
        if self._words is None:
            self._words = np.ascontiguousarray(to_words(self.ggsw))
        return self._words

    def column_sums(self, digits):
        """digits[li][r] = a list of N signed digits; returns the k + 1 polynomials
        sum_{li, r} digits[li][r] * ggsw[li][r][c] mod (X^N + 1, 2^128)."""
        n, slot = self.n, self.slot
        dp = [[_pack_signed(digits[li][r], slot) for r in range(self.kp1)] for li in range(self.level)]
        bias = 1 << (8 * slot - 1)
        out = []
        for c in range(self.kp1):
            total = self.offset
            for li in range(self.level):
                for r in range(self.kp1):
                    total += dp[li][r] * self.packed[li][r][c]
            v = _unpack(total, 2 * n, slot)
            out.append([(v[i] - v[i + n]) & MASK128 for i in range(n)])  # the biases cancel in the fold
        return out


def decompose_glwe(glwe, base_log, level):
    """digits[li][r][e] of a GLWE (k + 1 lists of N u128), least significant level first."""
    digits = [[[0] * len(glwe[0]) for _ in glwe] for _ in range(level)]
    for r, poly in enumerate(glwe):
        for e, x in enumerate(poly):
            for li, t in enumerate(py_decompose(x, base_log, level)):
                digits[li][r][e] = t
    return digits


_ACCEL = []


def accelerator():
    """tests/cpp/pbs128_ref.c through ctypes: the decomposition loop and the schoolbook column sums in unsigned __int128,
    so that expected values at N = 2048 take milliseconds.  Built once per process into a temporary directory that
    lives as long as the process; tests/test_pbs128_oracle.py pins it to the Python-integer forms above.  None only
    where there is no `cc` to run at all (the Python-integer forms then serve, slowly); a compiler that is there and
    fails on the committed file, or a library that does not load, is an error."""
    if not _ACCEL:
        import ctypes
        import os
        import shutil
        import subprocess
        import tempfile

        if shutil.which("cc") is None:
            _ACCEL.append(None)
            return None
        src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "pbs128_ref.c")
        tmp = tempfile.TemporaryDirectory(prefix="pbs128_ref_")  # removed when the process ends
        so = os.path.join(tmp.name, "pbs128_ref.so")
        built = subprocess.run(["cc", "-O2", "-fopenmp", "-shared", "-fPIC", src, "-o", so], capture_output=True,
                               text=True)
        if built.returncode != 0:
            raise RuntimeError(f"tests/cpp/pbs128_ref.c does not build:\n{built.stderr}")
        lib = ctypes.CDLL(so)
        vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
        lib.pbs128_decompose.argtypes = [vp, vp, i64, i32, i32, i32]
        lib.pbs128_column_sums.argtypes = [vp, vp, vp, i32, i32, i32, i32]
        lib.pbs128_decompose.restype = lib.pbs128_column_sums.restype = None
        lib._directory = tmp
        _ACCEL.append(lib)
    return _ACCEL[0]


def _threads():
    import os
    return max(1, min(16, len(os.sched_getaffinity(0))))


def fast_external_sums(ggsw, glwe, level):
    """The k + 1 column polynomials of GGSW (.) glwe through the compiled loops; ggsw a PackedGgsw, base_log <= 63."""
    lib = accelerator()
    words = np.ascontiguousarray(to_words(glwe))
    count = ggsw.kp1 * ggsw.n
    digits = np.empty((level, count), np.int64)
    lib.pbs128_decompose(digits.ctypes.data, words.ctypes.data, count, ggsw.base_log, level, _threads())
    out = np.empty((ggsw.kp1, ggsw.n, 2), np.uint64)
    lib.pbs128_column_sums(out.ctypes.data, digits.ctypes.data, ggsw.words().ctypes.data, level * ggsw.kp1, ggsw.kp1,
                           ggsw.n, _threads())
    return from_words(out)


def external_product(out, ggsw, glwe, level, fast=True):
    """add_external_product_assign_split: out += GGSW (.) glwe, in place; ggsw a PackedGgsw.  fast: through the
    compiled loops when they are available (the same integers; pinned by tests/test_pbs128_oracle.py)."""
    if fast and ggsw.base_log <= 63 and accelerator() is not None:
        sums = fast_external_sums(ggsw, glwe, level)
    else:
        sums = ggsw.column_sums(decompose_glwe(glwe, ggsw.base_log, level))
    for c, col in enumerate(sums):
        out[c] = [(x + y) & MASK128 for x, y in zip(out[c], col)]


def cmux(ct0, ct1, ggsw, level):
    """cmux_split: ct1 -= ct0, then ct0 += GGSW (.) ct1; both in place."""
    for c in range(len(ct0)):
        ct1[c] = [(x - y) & MASK128 for x, y in zip(ct1[c], ct0[c])]
    external_product(ct0, ggsw, ct1, level)


# ---- monomials, modulus switches, blind rotation ---------------------------------------------------------------------

def monomial_mul(poly, degree):
    """polynomial_wrapping_monic_monomial_mul: poly * X^degree mod (X^N + 1), degree in [0, 2N)."""
    n = len(poly)
    full, rem = (degree // n) & 1, degree % n
    out = [0] * n
    for e in range(n):
        v = poly[(e - rem) % n]
        if full ^ (e < rem):
            v = -v
        out[e] = v & MASK128
    return out


def monomial_div(poly, degree):
    """polynomial_wrapping_monic_monomial_div: poly / X^degree = poly * X^(2N - degree)."""
    n = len(poly)
    return monomial_mul(poly, (2 * n - degree % (2 * n)) % (2 * n))


def modulus_switch(x, log_modulus):
    """fft_impl/common.rs:10-23 at Scalar = u64."""
    return ((x + (1 << (64 - log_modulus - 1))) & MASK64) >> (64 - log_modulus)


def _trunc_div2(v):
    return -((-v) // 2) if v < 0 else v // 2


def centered_body_correction(mask, log_modulus):
    """centered_binary_ms_body_correction_to_add (algorithms/modulus_switch.rs:56-102) at Scalar = u64."""
    sum_half, sum_doubled = 0, 0
    for a in mask:
        error = ((modulus_switch(a, log_modulus) << (64 - log_modulus)) - a) & MASK64
        signed_error = error - M64 if error >> 63 else error
        half_error = _trunc_div2(signed_error)
        sum_half = (sum_half + half_error) & MASK64
        sum_doubled += 2 * half_error - signed_error
    sum_half = (sum_half - _trunc_div2(sum_doubled)) & MASK64
    return (sum_half - (1 << (64 - log_modulus - 1))) & MASK64


def switch_lwe(lwe, log_modulus, centered=False):
    """The switched mask and body of a u64 LWE (list of ints), values in [0, 2^log_modulus)."""
    mask, body = lwe[:-1], lwe[-1]
    corr = centered_body_correction(mask, log_modulus) if centered else 0
    return [modulus_switch(a, log_modulus) for a in mask] + [modulus_switch((body + corr) & MASK64, log_modulus)]


def blind_rotate(acc, switched, bsk, level):
    """blind_rotate_assign_split (bootstrap.rs:60-150): acc (k + 1 lists of N u128) / X^body, then one CMUX per
    non-zero switched mask element; bsk a list of PackedGgsw.  Returns the rotated accumulator."""
    acc = [monomial_div(p, switched[-1]) for p in acc]
    for a, ggsw in zip(switched[:-1], bsk):
        if a != 0:
            ct1 = [monomial_mul(p, a) for p in acc]
            cmux(acc, ct1, ggsw, level)
    return acc


def sample_extract(glwe):
    """extract_lwe_sample_from_glwe_ciphertext at MonomialDegree(0) (glwe_sample_extraction.rs:89-160)."""
    out = []
    for poly in glwe[:-1]:
        out += [poly[0]] + [(-poly[len(poly) - j]) & MASK128 for j in range(1, len(poly))]
    return out + [glwe[-1][0]]


def pbs(lut, switched, bsk, level):
    """blind_rotate_u128 (bootstrap.rs:152-247, native modulus): the extracted LWE, k N + 1 u128."""
    return sample_extract(blind_rotate([list(p) for p in lut], switched, bsk, level))


# ---- seeded keys and ciphertexts --------------------------------------------------------------------------------------

def rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def uniform_u128(g, count):
    w = g.integers(0, M64, size=(count, 2), dtype=np.uint64).astype(object)
    return (w[:, 0] | (w[:, 1] << 64)).tolist()


def uniform_glwe(g, k, n):
    return [uniform_u128(g, n) for _ in range(k + 1)]


def binary_key(g, size):
    return [int(b) for b in g.integers(0, 2, size=size)]


def _mul_binary(a, s):
    """(a * s) mod (X^N + 1, 2^128) for a binary polynomial s."""
    n = len(a)
    slot = (128 + n.bit_length() + 7) // 8
    c = _unpack(_pack(a, slot) * _pack(s, slot), 2 * n, slot)
    return [(c[i] - c[i + n]) & MASK128 for i in range(n)]


def glwe_encrypt(g, plaintext, glwe_sk, noise_log2):
    """plaintext (N u128) -> GLWE (k + 1 lists) under glwe_sk (k binary lists): b = sum a_i s_i + m + e mod 2^128; the
    noise is uniform in [-2^noise_log2, 2^noise_log2] (TUniform's support), none when noise_log2 is None."""
    n = len(plaintext)
    mask = [uniform_u128(g, n) for _ in glwe_sk]
    body = list(plaintext)
    for a, s in zip(mask, glwe_sk):
        body = [(x + y) & MASK128 for x, y in zip(body, _mul_binary(a, s))]
    if noise_log2 is not None:
        e = g.integers(-(1 << noise_log2), (1 << noise_log2) + 1, size=n)
        body = [(x + int(v)) & MASK128 for x, v in zip(body, e)]
    return mask + [body]


def glwe_decrypt(ct, glwe_sk):
    body = list(ct[-1])
    for a, s in zip(ct[:-1], glwe_sk):
        body = [(x - y) & MASK128 for x, y in zip(body, _mul_binary(a, s))]
    return body


def ggsw_encrypt(g, m, glwe_sk, base_log, level, noise_log2):
    """GGSW(m) as (level, k + 1, k + 1, N) nested lists, the level matrices in storage order (index li holds
    DecompositionLevel(level - li), the order ggsw.into_levels() yields): factor = -m 2^(128 - B j); row r < k encrypts
    s_r * factor, the last row -factor at X^0 (ggsw_encryption.rs:20-45, 318-375)."""
    k, n = len(glwe_sk), len(glwe_sk[0])
    out = []
    for li in range(level):
        j = level - li
        factor = (-m * (1 << (128 - base_log * j))) & MASK128
        rows = []
        for r in range(k + 1):
            if r < k:
                pt = [(s * factor) & MASK128 for s in glwe_sk[r]]
            else:
                pt = [(-factor) & MASK128] + [0] * (n - 1)
            rows.append(glwe_encrypt(g, pt, glwe_sk, noise_log2))
        out.append(rows)
    return out


def gadget_ggsw(m, k, n, base_log, level):
    """The noise-free GGSW of message m whose masks carry the gadget: row r of level matrix li is m 2^(128 - B j) at
    X^0 of polynomial r.  Its external product with a GLWE is m * closest_representable of every coefficient."""
    out = []
    for li in range(level):
        f = (m << (128 - base_log * (level - li))) & MASK128
        out.append([[[f if (c == r and e == 0) else 0 for e in range(n)] for c in range(k + 1)]
                    for r in range(k + 1)])
    return out


def uniform_ggsw(g, k, n, level):
    return [[uniform_glwe(g, k, n) for _ in range(k + 1)] for _ in range(level)]


def bsk_gen(g, lwe_sk, glwe_sk, base_log, level, noise_log2):
    return [ggsw_encrypt(g, b, glwe_sk, base_log, level, noise_log2) for b in lwe_sk]


def lwe_encrypt_u64(g, pt, lwe_sk, noise_log2=None):
    """A native-modulus u64 LWE (list of ints) of plaintext pt; noise-free when noise_log2 is None."""
    a = [int(v) for v in g.integers(0, M64, size=len(lwe_sk), dtype=np.uint64)]
    e = int(g.integers(-(1 << noise_log2), (1 << noise_log2) + 1)) if noise_log2 is not None else 0
    return a + [(sum(x for x, s in zip(a, lwe_sk) if s) + pt + e) & MASK64]


def lwe_decrypt_u128(ct, lwe_sk):
    return (ct[-1] - sum(x for x, s in zip(ct[:-1], lwe_sk) if s)) & MASK128


def pbs_lut(n, k, msg_mod, delta, f):
    """generate_programmable_bootstrap_glwe_lut (lwe_programmable_bootstrapping/mod.rs:24-75) over u128."""
    box = n // msg_mod
    acc = []
    for i in range(msg_mod):
        acc += [(f(i) * delta) & MASK128] * box
    half = box // 2
    acc = [(-v) & MASK128 for v in acc[:half]] + acc[half:]
    acc = acc[half:] + acc[:half]
    return [[0] * n for _ in range(k)] + [acc]


def decode(pt, delta, msg_mod):
    """divide_round(pt, delta) mod 2 msg_mod (the padding bit kept)."""
    return ((pt + delta // 2) // delta) % (2 * msg_mod)


# ---- the limb rule ----------------------------------------------------------------------------------------------------

def limb_rule(n, k, base_log, level):
    """(w, n_limbs): the largest w with R N 2^(B-1) (2^w - 1) <= (p - 1) / 2, R = (k + 1) level; n_limbs =
    ceil(128 / w), (0, 0) when no width fits."""
    d = (k + 1) * level * n * (1 << (base_log - 1))
    w = 0
    while d * ((1 << (w + 1)) - 1) <= (P - 1) // 2:
        w += 1
    return (w, -(-128 // w)) if w else (0, 0)
