"""The limb-corner corpus every modular-arithmetic test feeds (host only: numpy and Python integers, seeded).

The engine's integer results rest on three families of modular arithmetic written for 32-bit ALUs (csrc/mi_arith.hpp:
Goldilocks, Montgomery, Shoup32) and on the same arithmetic as asm in the generated N = 2048 bodies.  Each primitive
has a correction arm that uniform operands take with probability about 2^-32 (the borrow fix of reduce128, the
"no carry but >= p" arm of a canonical add, ...).  The corpus puts operands whose 32-bit limbs (16-bit limbs below
2^32) sit on 0, 1, 2, 2^31 - 1, 2^31, 2^32 - 2 and 2^32 - 1 in front of every primitive and every butterfly slot.

* ``values(p)``: the limb-corner residues of a modulus and their negations (73 for the Solinas prime).
* ``grid(p)``: the operand grid values x values as two flat arrays (the pointwise tests' operands).
* ``accumulate_operand(p, a, b, k)``: the c that makes c + a b a corner (mul_accumulate's add on its own corners).
* ``montgomery_wrap_pairs(p)``: operands that reach the ``t < s`` arm of Montgomery::mul.  REDC computes
  u = (a b + m p) / 2^64 = thi + mhi + c with c = [tlo != 0] and u < 2 p.  The arm needs thi + mhi = 2^64 - 1 without
  its own wrap and c = 1, i.e. u = 2^64 exactly: impossible for p < 2^63 (u < 2 p <= 2^64 there), reachable above:
  a b + m p = 2^128 has, for any a < p, the solution m = 2^128 p^-1 mod a, b = (2^128 - m p) / a, valid when b < p.
* ``rows(n, p, oracle, inverse)``: at most 64 polynomials per (n, p): spikes, first-stage butterfly pairs whose sum /
  difference lands on 0, p - 1, p, p + 1, 2^w - 1, 2^w (w the word width, 64, or 32 below 2^32), dense corner rows
  and rows built backwards from a corner-valued (or small-valued) spectrum.
"""
import numpy as np

LIMBS32 = (0, 1, 2, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF)
LIMBS16 = (0, 1, 2, 0x7FFF, 0x8000, 0xFFFE, 0xFFFF)
SOLINAS_P = 0xFFFFFFFF00000001
MAX_ROWS = 64


def word_bits(p):
    """Width of the machine word the modulus' arithmetic is written on."""
    return 32 if p < (1 << 32) else 64


def values(p):
    """Distinct residues (h << w/2 | l) mod p for corner limbs h, l, then their negations mod p."""
    half = word_bits(p) // 2
    limbs = LIMBS16 if half == 16 else LIMBS32
    base = [((h << half) | l) % p for h in limbs for l in limbs]
    seen, out = set(), []
    for v in base + [(p - v) % p for v in base]:
        if v not in seen:
            seen.add(v)
            out.append(v)
    return out


def grid(p):
    """(a, b): every ordered pair of values(p), as two uint64 arrays of len(values)^2."""
    v = np.array(values(p), dtype=np.uint64)
    return np.repeat(v, v.size), np.tile(v, v.size)


def sum_targets(p):
    """Where a canonical add / sub changes arm: the sums 0, p - 1, p, p + 1, 2^w - 1 and 2^w."""
    w = 1 << word_bits(p)
    return [0, p - 1, p, p + 1, w - 1, w]


def accumulate_operand(p, a, b, k):
    """c < p with c + (a b mod p) equal (as integers, where possible) to the k-th sum target, else c = target - a b mod p."""
    t = sum_targets(p)[k % 6]
    c = t - (a * b) % p
    return c if 0 <= c < p else c % p


def _inv(a, m):
    return pow(a, -1, m)


def montgomery_wrap_pairs(p, count=8, seed=0x6d77):
    """(a, b) < p with a b + m p = 2^128 for m = -a b p^-1 mod 2^64: REDC's thi + mhi = 2^64 - 1 with a carry in."""
    if p < (1 << 63):
        return []
    rng = np.random.default_rng(seed)
    out, cand = [], [p - 1, p - 2, (1 << 63) + 1, 0xFFFFFFFF00000001 % p]
    while len(out) < count:
        a = cand.pop(0) if cand else int(rng.integers(1 << 62, 1 << 63)) * 2 + 1
        if a >= p or a < 2:
            continue
        m = ((1 << 128) * _inv(p % a, a)) % a
        t = (1 << 128) - m * p
        if t <= 0 or t % a:
            continue
        b = t // a
        if b < p and (a * b) & ((1 << 64) - 1):
            out.append((a, b))
    return out


# ---- rows ------------------------------------------------------------------------------------------------------

def _lead(p):
    """The values a spike row carries: the corners first whose products and sums sit nearest the correction arms."""
    w = word_bits(p)
    half = w // 2
    top = (1 << half) - 1
    first = [p - 1, (1 << half) % p, top % p, ((top - 1) << half | top) % p, (1 << (w - 1)) % p, (top << half) % p,
             ((1 << (w - 1)) | (1 << (half - 1))) % p, (p - top) % p, 2, (p + 1) // 2]
    seen, out = set(), []
    for v in first + values(p):
        if v not in seen:
            seen.add(v)
            out.append(v)
    return out


def _pairs(p):
    """(a, b), a, b < p, whose integer sum a + b or wrapped difference a - b mod 2^w is a sum target."""
    w = 1 << word_bits(p)
    eps = w % p
    anchors = [0, 1, eps, (p - 1) // 2, p - 1, p - eps, (w - 1) % p, 1 << (word_bits(p) - 1)]
    out, seen = [], set()
    for a in anchors:                           # anchor-major: every target comes early (small n keeps a prefix)
        a %= p
        for t in sum_targets(p):
            for b in (t - a, (a - t) % w):      # a + b = t; a - b = t (mod 2^w)
                if 0 <= b < p and (a, b) not in seen:
                    seen.add((a, b))
                    out.append((a, b))
    return out


def rows(n, p, oracle, inverse=False, limit=MAX_ROWS):
    """The corner batch of one (n, p): a uint64 array (rows <= limit <= 64, n) of canonical residues.  `oracle` is the
    oracle module (its plan supplies the first twiddle and builds the backward rows); inverse selects the rows built
    for the inverse transform.  Deterministic in (n, p, inverse); a limit below the family's size keeps an evenly
    spaced subset (every family keeps its share) and builds only those rows."""
    assert limit <= MAX_ROWS
    plan = oracle.Plan.try_new(n, p)
    vals = values(p)
    varr = np.array(vals, dtype=np.uint64)
    lead = _lead(p)
    makers = []  # (built backwards?, function of the row's own generator -> the row, or its spectrum)

    def rng_of(k):
        return np.random.default_rng([n % (1 << 31), p % (1 << 63), int(inverse), k])

    # spikes: one corner value alone at 0, 1, n/2 - 1, n/2, n - 1: every twiddle of its cone multiplies it
    spots = [0, 1, n // 2 - 1, n // 2, n - 1]

    def spike(k):
        def make(_):
            r = np.zeros(n, dtype=np.uint64)
            r[spots[k % 5]] = lead[k]
            return r
        return make
    makers += [(False, spike(k)) for k in range(15)]
    # pairs: the first-stage partners (j, j + n/2) of the forward's decimation and (j, j + 1) of the inverse's, every
    # pair row holding several pairs at distinct j; then with b w^-1 in b's place so that the twiddle product is b
    w_f, w_i = int(plan.twid[1]), int(plan.inv_twid[n // 2])
    pairs = _pairs(p)
    per_row = min(len(pairs), n // 2)

    def pair_row(dist, winv, start):
        def make(_):
            r = np.zeros(n, dtype=np.uint64)
            for q, (a, b) in enumerate(pairs[start:start + per_row]):
                j = 2 * q if dist == 1 else q
                r[j], r[j + dist] = a, (b * winv) % p
            return r
        return make
    for dist, winv in ((n // 2, 1), (1, 1), (n // 2, _inv(w_f, p)), (1, _inv(w_i, p))):
        for start in range(0, min(len(pairs), 6 * per_row), per_row):  # n = 16 keeps the first 48 pairs
            makers.append((False, pair_row(dist, winv, start)))
    # dense: every slot a corner value, and the all-(p - 1) row
    idx = np.arange(n)
    draw = lambda g: varr[g.integers(0, varr.size, size=n)]
    makers += [(False, draw)] * 4
    makers.append((False, lambda _: varr[idx % varr.size]))
    makers.append((False, lambda _: np.full(n, p - 1, dtype=np.uint64)))
    # backward-built: the transform's OUTPUT is dense over the corners / over small values (a last-stage sum below
    # 2^w mod p can only leave the "no carry but >= p" arm of a canonical add)
    small_hi = min(p, (1 << (word_bits(p) // 2)) - 1)
    makers += [(True, draw)] * 4
    makers += [(True, lambda g: g.integers(0, small_hi, size=n, dtype=np.uint64))] * 4
    makers.append((True, lambda _: varr[(3 * idx + 1) % varr.size]))
    makers.append((True, lambda _: (idx % min(p, 7)).astype(np.uint64)))
    assert len(makers) <= MAX_ROWS
    keep = range(len(makers))
    if len(makers) > limit:
        keep = sorted(set(np.linspace(0, len(makers) - 1, limit).round().astype(int).tolist()))
    out = []
    for k in keep:
        backward, make = makers[k]
        r = make(rng_of(k))
        if backward:
            r = plan.normalize(plan.fwd(r) if inverse else plan.inv(r))
        out.append(r)
    out = np.stack(out)
    assert (out < np.uint64(p)).all()
    return out


# ---- the body corpus of the N = 2048 asm bodies (tests/test_tw_body_corners.py, tests/test_arith_corners_gpu.py) ------
# rows(2048, P) plus targeted rows: seeded candidates the carry recorder of tools/asm_emu.py kept because they set a
# carry no earlier row had set (BODY_SEEDS), and rows constructed backwards through the transform so that the operand
# of a general multiply takes the reduction's borrow against that element's own table twiddle.
P = SOLINAS_P
FAMILIES = 10
L32 = np.array(LIMBS32, dtype=np.uint64)


def _limb_words(g, n, mix):
    """words whose two 32-bit limbs are corner limbs or (with probability mix) random"""
    def limb():
        c = L32[g.integers(0, L32.size, size=n)]
        r = g.integers(0, 1 << 32, size=n, dtype=np.uint64)
        return np.where(g.random(n) < mix, r, c)
    return (limb() << np.uint64(32)) | limb()


def _near(g, n):
    """residues next to the arithmetic's own thresholds: p - d, 2^32 k - d, 2^32 k + d, (2^32 - 1) k for small d, k"""
    k = g.integers(0, 1 << 32, size=n, dtype=np.uint64)
    d = g.integers(0, 4, size=n, dtype=np.uint64)
    kind = g.integers(0, 5, size=n)
    hi = k << np.uint64(32)
    v = np.select([kind == 0, kind == 1, kind == 2, kind == 3],
                  [np.uint64(P - 1) - d, hi - d, hi + d, k * np.uint64(0xFFFFFFFF) + d], (hi | np.uint64(0xFFFFFFFF)) - d)
    return v


def candidate(k, plan, inverse, raw=False):
    g = np.random.default_rng([0xB0D7, int(inverse), int(raw), k])
    n = 2048
    fam = k % FAMILIES
    vals = np.array(values(P), dtype=np.uint64)
    if fam in (0, 1):
        y = vals[g.integers(0, vals.size, size=n)]
    elif fam in (2, 3):
        y = _limb_words(g, n, 0.25)
    elif fam in (4, 5):
        y = _near(g, n)
    elif fam in (6, 7):
        y = np.zeros(n, dtype=np.uint64)
        m = int(2 ** g.integers(0, 8))
        pos = g.choice(n, size=m, replace=False)
        src = _near(g, m) if g.random() < 0.5 else vals[g.integers(0, vals.size, size=m)]
        y[pos] = src
    else:
        y = g.integers(0, (1 << 32) - 1, size=n, dtype=np.uint64) << np.uint64(int(g.integers(0, 33)))
    if raw:
        return y
    y = y % np.uint64(P)
    if fam % 2 == 1:  # built backwards: y is the transform's output
        y = plan.normalize(plan.fwd(y) if inverse else plan.inv(y))
    return y


def ms64_rows():
    g = np.random.default_rng(0x6D73)
    w = [(h << 32) | l for h in LIMBS32 for l in LIMBS32] + [P, P + 1, P - 1]
    w = np.array(w, dtype=np.uint64)
    return np.stack([w[g.integers(0, w.size, size=2048)] for _ in range(4)] + [_limb_words(g, 2048, 0.3) for _ in range(4)])


def borrow_operand(w, g):
    """x < p whose product with w takes the reduction's borrow: the low 64 bits of x w (below 2^32) are less than the
    top 32 bits of its high half.  w = 2^k u, u odd: x = l u^-1 mod 2^(64 - k) plus any multiple of 2^(64 - k)."""
    if w == 0:
        return 0
    k = (w & -w).bit_length() - 1
    u = w >> k
    if k >= 32:  # the low half is a multiple of 2^k >= 2^32 unless it is 0: x = t 2^(64 - k), x w = t u 2^64, t u >= 2^32
        for _ in range(64):
            t = int(g.integers(1, 1 << k, dtype=np.uint64))
            if (t << (64 - k)) < P and t * u >= (1 << 32):
                return t << (64 - k)
        return 0
    mod = 1 << (64 - k)
    uinv = pow(u, -1, mod)
    for _ in range(64):
        l = int(g.integers(1, 1 << 8))
        x = (l * uinv) % mod + (int(g.integers(0, 1 << k)) << (64 - k) if k else 0)
        t = x * w
        if x < P and (t & ((1 << 64) - 1)) < (t >> 96):
            return x
    return int(g.integers(0, 1 << 32))


def fwd_borrow_row(plan, tf, g1_out, seed=0):
    """Input whose value in front of the forward body's twist multiply (after the 5 block stages, carrying the scale
    2^g1_out[block]) is borrow_operand of that element's twist-table entry."""
    g = np.random.default_rng([0xB0220, seed])
    n = 2048
    half = (P + 1) // 2
    z = [borrow_operand(int(tf[e]), g) * pow(2, (-g1_out[e // 64]) % 192, P) % P for e in range(n)]
    tw = [int(v) for v in plan.twid]
    m = 16
    while m >= 1:       # undo the reference's CT stages m = 16 ... 1
        t = n // (2 * m)
        for i in range(m):
            winv = pow(tw[m + i], P - 2, P)
            for j in range(2 * i * t, 2 * i * t + t):
                a, b = z[j], z[j + t]
                z[j], z[j + t] = (a + b) * half % P, (a - b) * half % P * winv % P
        m //= 2
    return np.array(z, dtype=np.uint64)


def inv_borrow_row(plan, ti, seed=0):
    """Input of the inverse whose value in front of the untwist multiply (after the 6 stages inside the 64-blocks) is
    borrow_operand of that element's untwist-table entry."""
    g = np.random.default_rng([0xB0221, seed])
    n = 2048
    half = (P + 1) // 2
    z = [borrow_operand(int(ti[e]), g) * int(ti[e]) % P for e in range(n)]
    tw = [int(v) for v in plan.inv_twid]
    m = 32
    while m <= n // 2:  # undo the reference's GS stages m = 32 ... 1024 (the last of its first six first)
        t = n // (2 * m)
        for i in range(m):
            winv = pow(tw[m + i], P - 2, P)
            for j in range(2 * i * t, 2 * i * t + t):
                s, d = z[j], z[j + t] * winv % P
                z[j], z[j + t] = (s + d) * half % P, (s - d) * half % P
        m *= 2
    return np.array(z, dtype=np.uint64)


def _br(x, b):
    return int(format(x, f"0{b}b")[::-1], 2)


def fwd_pair_borrow_row(plan, lane_tw, seed=0):
    """Input whose last-stage multiplicand, in the body's lane-pair stage (pair k of a 64-block times lane_tw[k]),
    is borrow_operand(lane_tw[k]): the product v is the reference's x[2 k + 1] twid[1024 + k], the partner is random."""
    g = np.random.default_rng([0xB0222, seed])
    n = 2048
    y = [0] * n
    for k in range(n // 2):
        w = int(lane_tw[k % 32])
        v = borrow_operand(w, g) * w % P
        a = int(g.integers(0, P, dtype=np.uint64))
        y[2 * k], y[2 * k + 1] = (a + v) % P, (a - v) % P
    return plan.normalize(plan.inv(np.array(y, dtype=np.uint64)))


def inv_pair_borrow_row(lane_tw_inv, seed=0):
    """Input of the inverse whose last decimation-in-time stage inside each 64-block multiplies
    O_j = borrow_operand(omega^-j) by omega^-j (lane_tw_inv[j] = omega^-j, omega = 8): O is the unnormalised 32-point
    inverse transform (root omega^2) of the block's second half read in bit-reversed order; the first half is random."""
    g = np.random.default_rng([0xB0223, seed])
    n = 2048
    inv32 = pow(32, P - 2, P)
    out = [0] * n
    for b in range(32):
        O = [borrow_operand(int(lane_tw_inv[j]), g) for j in range(32)]
        for k in range(32):  # c_k = (1/32) sum_j O_j omega^(2 j k)
            c = sum(O[j] * pow(8, (2 * j * k) % 64 * 1, P) for j in range(32)) % P * inv32 % P
            out[64 * b + 32 + _br(k, 5)] = c
        for j in range(32):
            out[64 * b + j] = int(g.integers(0, P, dtype=np.uint64))
    return np.array(out, dtype=np.uint64)


def ms64_preimage(x):
    """A native word v with (v p + 2^63) >> 64 = x for every canonical x of the array (the key conversion's switch)."""
    out = []
    for r in np.asarray(x, dtype=np.uint64).reshape(-1):
        r = int(r)
        v = max(0, -((-(r << 64) + (1 << 63)) // P))  # ceil((r 2^64 - 2^63) / p)
        assert v < (1 << 64) and (v * P + (1 << 63)) >> 64 == r
        out.append(v)
    return np.array(out, dtype=np.uint64).reshape(np.shape(x))


def body_tables(oracle):
    """(plan, forward body table, inverse body table) as the library builds them for the N = 2048 asm bodies: the twist
    rows rho_b^j with the forward's scale plan folded in, then the 32 lane-pair twiddles; the inverse's untwist rows
    and the twiddles omega^-(2 m + par) of its last decimation-in-time stage."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import gen_tw_kernel as G
    plan = oracle.Plan.try_new(2048, P)
    psi = int(plan.twid[_br(1, 11)])
    omega = pow(psi, 64, P)
    tabs = G.load_tables()
    g1_out, cyc_in = tabs["TW_G1_OUT_SCALE"][0], tabs["TW_CYC_IN_SCALE"][0]
    f, i = [], []
    for blk in range(32):
        rho = pow(psi, 2 * _br(blk, 5) + 1, P)
        rinv = pow(rho, P - 2, P)
        f += [pow(rho, j, P) * pow(2, (cyc_in[j >> 1] - g1_out[blk]) % 192, P) % P for j in range(64)]
        i += [pow(rinv, j, P) for j in range(64)]
    f += [pow(omega, _br(g, 5), P) for g in range(32)]
    omega_inv = pow(omega, P - 2, P)
    i += [pow(omega_inv, 2 * (e % 16) + e // 16, P) for e in range(32)]
    return plan, f, i, g1_out


# candidates the recorder kept (found once with the search loop of tests/test_tw_body_corners.py's docstring)
BODY_SEEDS = {
    "fwd": [1, 6, 7, 17, 37, 40, 46, 47, 56, 86, 276, 306],
    "inv": [0, 6, 7, 10, 16, 17, 26, 27, 36, 45, 66, 76, 87, 106, 126, 127, 147, 157, 167, 176, 177, 196, 207, 216, 251,
            256, 266, 326, 366],
    "fwd_ms64": [],
}


def body_rows(oracle, name):
    """The body corpus of one asm body ("fwd", "inv", "fwd_ms64"): rows(2048, P), the kept candidates and the
    constructed borrow rows; for the key-conversion body the forward's corpus as native words that switch to it, and
    raw limb-corner words for the switch's own carries."""
    plan, tf, ti, g1_out = body_tables(oracle)
    inverse = name == "inv"
    base = "inv" if inverse else "fwd"
    out = list(rows(2048, P, oracle, inverse))
    out += [candidate(k, plan, inverse) for k in BODY_SEEDS[base]]
    if inverse:
        omega_inv = pow(8, P - 2, P)
        out += [inv_borrow_row(plan, ti), inv_pair_borrow_row([pow(omega_inv, j, P) for j in range(32)]),
                inv_stage_carry_row(plan, 16, -1), inv_stage_carry_row(plan, 4, -1),
                inv_dit_carry_row(3), inv_dit_carry_row(5)]
    else:
        out += [fwd_borrow_row(plan, tf, g1_out), fwd_pair_borrow_row(plan, tf[2048:2080])]
    out = np.stack(out)
    if name == "fwd_ms64":
        out = np.concatenate([ms64_preimage(out), ms64_rows(),
                              np.stack([candidate(k, plan, False, raw=True) for k in BODY_SEEDS[name]] or
                                       [np.zeros(2048, np.uint64)])])
    return out


def shift_carry_operand(e):
    """x < p whose product with 2^e sets the carry of the first fold of the bodies' shift multiply (tmul): with
    r = e mod 32 (r = 32 at e = 32) the fold adds the top r bits h of x, times 2^32 - 1, to the low bits shifted up by
    r, which carries for h = 1 and all lower bits set: x = 2^(65 - r) - 1.  None where no canonical x carries (r < 2:
    the carry needs x >= 2^64 - 2^31 + 1 at r = 1) or the multiply takes another path (e >= 64)."""
    e %= 96
    r = e if e <= 32 else e - 32
    if e >= 64 or r < 2 or r > 31:
        return None
    return (1 << (65 - r)) - 1


_LOG2 = {}


def inv_stage_carry_row(plan, m, sign, seed=0):
    """Input of the inverse whose differences at the reference's stage of m groups (one of its last five: the twiddles
    are powers of two) are sign times shift_carry_operand of the group's twiddle exponent; the partners are random."""
    if not _LOG2:
        _LOG2.update({pow(2, s, P): s for s in range(192)})
    g = np.random.default_rng([0xB0224, m, sign + 1, seed])
    n = 2048
    half = (P + 1) // 2
    tw = [int(v) for v in plan.inv_twid]
    z = [int(v) for v in g.integers(0, P, size=n, dtype=np.uint64)]
    t = n // (2 * m)
    for i in range(m):
        x = shift_carry_operand(_LOG2[tw[m + i]])
        if x is not None:
            for j in range(2 * i * t, 2 * i * t + t):
                z[j] = (z[j + t] + sign * x) % P
    mm = 2 * m
    while mm <= n // 2:  # undo the stages before it
        t = n // (2 * mm)
        for i in range(mm):
            winv = pow(tw[mm + i], P - 2, P)
            for j in range(2 * i * t, 2 * i * t + t):
                s, d = z[j], z[j + t] * winv % P
                z[j], z[j + t] = (s + d) * half % P, (s - d) * half % P
        mm *= 2
    return np.array(z, dtype=np.uint64)


def inv_dit_carry_row(s, seed=0):
    """Input of the inverse whose multiplicands at decimation-in-time stage s inside every 64-block (position
    base + j + 2^s times omega^(-j 32 / 2^s), omega = 8 = 2^3) are shift_carry_operand of that exponent."""
    g = np.random.default_rng([0xB0225, s, seed])
    half = (P + 1) // 2
    out = []
    for _ in range(32):
        v = [int(x) for x in g.integers(0, P, size=64, dtype=np.uint64)]
        d = 1 << s
        for base in range(0, 64, 2 * d):
            for j in range(d):
                x = shift_carry_operand((-3 * j * (32 >> s)) % 192)
                if x is not None:
                    v[base + j + d] = x
        for q in range(s - 1, -1, -1):  # undo the stages before it
            d = 1 << q
            for base in range(0, 64, 2 * d):
                for j in range(d):
                    winv = pow(8, (j * (32 >> q)) % 64, P)
                    a, b = v[base + j], v[base + j + d]
                    v[base + j], v[base + j + d] = (a + b) * half % P, (a - b) * half % P * winv % P
        out += v
    return np.array(out, dtype=np.uint64)
