"""numpy / pure-Python restatement of the shortint lookup tables and the radix carry propagation (host only, test
infrastructure).  Reference paths relative to tfhe/src:

* ``lut_fill``                  shortint/engine/mod.rs:80-141 (fill_accumulator_with_encoding)
* ``bivariate_table``           shortint/server_key/bivariate_pbs.rs:57-108 (generate_lookup_table_bivariate_with_factor)
* ``propagate_single_carry``    integer/server_key/radix_parallel/add.rs:1452-1487 (compute_prefix_sum_hillis_steele), as
                                the library's mi_radix_propagate_single_carry_batch sequences it
* ``full_propagate``            integer/server_key/radix_parallel/mod.rs:140-158, :187-199

The radix functions work on cleartext block values: a lookup is ``table[x]`` and refuses x >= m c (the value would
reach the padding bit).  ``Rule`` carries the three one-off mutants the tests tell from the true rule.
"""
import numpy as np

NONE, GENERATED, PROPAGATED = 0, 1, 2


def lut_fill(n, k, m, c, table):
    """The accumulator (k + 1, N): boxes of N / (m c) holding table[i] 2^63 / (m c), the first half box negated, rotated
    left by half a box."""
    sup = m * c
    assert len(table) == sup
    box, delta = n // sup, (1 << 63) // sup
    body = np.zeros(n, np.uint64)
    for i in range(sup):
        body[i * box:(i + 1) * box] = np.uint64((int(table[i]) * delta) % 2**64)
    half = box // 2
    with np.errstate(over="ignore"):
        body[:half] = np.uint64(0) - body[:half]
    body = np.roll(body, -half)
    acc = np.zeros((k + 1, n), np.uint64)
    acc[k] = body
    return acc


def bivariate_table(m, c, f, factor=None):
    factor = factor or m
    return [f((x // factor) % m, (x % factor) % m) for x in range(m * c)]


class Rule:
    """The true propagation rule; each flag is one mutant."""

    def __init__(self, scan_offset=0, block0_propagated=False, drop_last_scan_round=False):
        self.scan_offset, self.block0_propagated, self.drop_last_scan_round = scan_offset, block0_propagated, \
            drop_last_scan_round


def single_carry_supported(m, c):
    return m * c >= 16 and c <= m and 2 * m + 2 < m * c


def _lookup(f, x, m, c):
    if not 0 <= x < m * c:
        raise OverflowError(f"lookup of {x} with m c = {m * c}")
    return f(x)


def state(x, m, first, rule):
    if x >= m:
        return GENERATED
    if x == m - 1 and (not first or rule.block0_propagated):
        return PROPAGATED
    return NONE


def scan_rounds(n_blocks):
    return 0 if n_blocks <= 1 else (n_blocks - 1).bit_length()


def propagate_single_carry(blocks, m, c, rule=None):
    """blocks (values <= 2 (m - 1), least significant first) -> (clean blocks, carry out, bootstrap rounds)."""
    rule = rule or Rule()
    b = len(blocks)
    msg = [_lookup(lambda x: x % m, x, m, c) for x in blocks]
    st = [_lookup(lambda x, i=i: state(x, m, i == 0, rule), x, m, c) for i, x in enumerate(blocks)]
    if b == 1:
        return msg, st[0], 1
    steps = scan_rounds(b) - (1 if rule.drop_last_scan_round else 0)
    space = 1
    for _ in range(steps):
        new = list(st)
        for i in range(space, b):
            prev = st[i - space + rule.scan_offset] if 0 <= i - space + rule.scan_offset < b else 0
            packed = m * st[i] + prev
            new[i] = _lookup(lambda x: (x % m) if (x // m) % m == PROPAGATED else (x // m) % m, packed, m, c)
        st = new
        space *= 2
    out = [_lookup(lambda x: x % m, msg[i] + (st[i - 1] if i else 0), m, c) for i in range(b)]
    return out, st[b - 1], 2 + scan_rounds(b)


def extract_and_add(blocks, m, c):
    msg = [_lookup(lambda x: x % m, x, m, c) for x in blocks]
    carry = [_lookup(lambda x: x // m, x, m, c) for x in blocks]
    return [msg[i] + (carry[i - 1] if i else 0) for i in range(len(blocks))]


def full_propagate(blocks, m, c):
    """blocks of any value below m c -> clean blocks (the top carry is dropped)."""
    b = len(blocks)
    cur = extract_and_add(blocks, m, c)
    if b == 1 or single_carry_supported(m, c):
        return propagate_single_carry(cur, m, c)[0] if b > 1 else cur
    for _ in range(b - 1):
        cur = extract_and_add(cur, m, c)
    return cur


def add(lhs, rhs, m, c):
    return propagate_single_carry([a + b for a, b in zip(lhs, rhs)], m, c)


def value(blocks, m):
    return sum(int(x) * m**i for i, x in enumerate(blocks))


def digits(v, m, n_blocks):
    return [(v // m**i) % m for i in range(n_blocks)]
