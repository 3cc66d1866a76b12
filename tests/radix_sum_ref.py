"""Pure-Python model of the radix sum of ciphertexts and of the radix multiplication (host only, test infrastructure),
written from the reference's loop.  Paths relative to tfhe/src/integer/server_key/radix_parallel:

* ``run_rounds`` / ``partial_sum`` / ``sum_terms``   sum.rs:14-147 (unchecked_partial_sum_ciphertexts_vec_parallelized),
                                                     :155-166 (unchecked_sum_ciphertexts_vec_parallelized)
* ``mul_terms`` / ``mul``                            mul.rs:333-400 (compute_terms_for_mul_low), :437-460
* ``max_sum_size``                                   shortint/server_key/mod.rs

A row is whatever the caller puts into the columns: a block value (the value model: ``partial_sum``, ``sum_terms``,
``mul``) or a label (the schedule model: ``schedule``, which the written GPU sequences and the index-array tests
drive).  ``Rule`` carries the four one-off mutants the tests tell from the true rule.  A lookup refuses x >= m c (the
value would reach the padding bit).
"""
import shortint_ref as R


class Rule:
    """The true schedule; each flag is one mutant."""

    def __init__(self, chunk_extra=0, last_column_carry=False, rest_from_front=False, skip_exact=False):
        self.chunk_extra, self.last_column_carry, self.rest_from_front, self.skip_exact = \
            chunk_extra, last_column_carry, rest_from_front, skip_exact


def max_sum_size(m, c):
    """max_sum_size(Degree(m - 1)): how many rows of value <= m - 1 a block holds."""
    return (m * c - 1) // (m - 1)


def supported(m, c):
    return m >= 2 and 2 <= c <= m


def initial_columns(terms, first_block, n_blocks):
    """terms[t][b] -> columns[b] = block b of every term that lives there (first_block[t] <= b: the blocks the
    reference skips by degree == 0), in term order."""
    first_block = first_block or [0] * len(terms)
    return [[terms[t][b] for t in range(len(terms)) if first_block[t] <= b] for b in range(n_blocks)]


def run_rounds(columns, m, c, on_chunk, rule=None):
    """The while loop of sum.rs:75-126.  on_chunk(rows, column, want_carry, round) -> (message row, carry row or None),
    called column by column and, in a column, chunk by chunk.  Returns (final columns, rounds); a round is the list over
    columns of (length before the round, chunks)."""
    rule = rule or Rule()
    s = max_sum_size(m, c) + rule.chunk_extra
    n = len(columns)
    columns = [list(col) for col in columns]
    rounds = []
    while any(len(col) > s for col in columns):
        shape, outputs, rests = [], [], []
        for b, col in enumerate(columns):
            if len(col) < s or (rule.skip_exact and len(col) == s):  # sum.rs:81-83
                shape.append((len(col), 0))
                outputs.append([])
                rests.append(list(col))
                continue
            q = len(col) // s
            want_carry = b < n - 1 or rule.last_column_carry  # sum.rs:92 with output_carries = None
            outputs.append([on_chunk(col[k * s:(k + 1) * s], b, want_carry, len(rounds)) for k in range(q)])
            rest = len(col) % s
            rests.append(col[:rest] if rule.rest_from_front else col[len(col) - rest:])  # rotate_right + truncate
            shape.append((len(col), q))
        columns = rests
        for i, out in enumerate(outputs):  # sum.rs:113-125, in its visiting order
            for msg, carry in out:
                columns[i].append(msg)
                if carry is not None:
                    columns[min(i + 1, n - 1)].append(carry)  # only the mutant has a carry in the last column
        rounds.append(shape)
    return columns, rounds


def _value_chunk(m, c):
    def on_chunk(rows, column, want_carry, rnd):
        x = sum(rows)
        msg = R._lookup(lambda v: v % m, x, m, c)
        return msg, (R._lookup(lambda v: v // m, x, m, c) if want_carry else None)
    return on_chunk


def partial_sum(terms, first_block, n_blocks, m, c, rule=None):
    """Block values with unpropagated carries (each refused at >= m c), and the rounds."""
    columns, rounds = run_rounds(initial_columns(terms, first_block, n_blocks), m, c, _value_chunk(m, c), rule)
    blocks = [R._lookup(lambda v: v, sum(col), m, c) for col in columns]
    return blocks, rounds


def sum_terms(terms, first_block, n_blocks, m, c, rule=None):
    """unchecked_sum_ciphertexts_vec_parallelized: the partial sum, then the full propagation."""
    if not terms:
        return [0] * n_blocks
    return R.full_propagate(partial_sum(terms, first_block, n_blocks, m, c, rule)[0], m, c)


def mul_first_block(n_blocks, m):
    """first_block of the terms of compute_terms_for_mul_low in its chain order: the lsb term of every rhs block, then
    (m > 2) the msb term of every rhs block but the last."""
    return list(range(n_blocks)) + ([j + 1 for j in range(n_blocks - 1)] if m > 2 else [])


def mul_pairs(n_blocks, m):
    """Per term of mul_first_block, per block b >= first_block: (lhs block, rhs block, msb)."""
    n = n_blocks
    terms = [[(b - j, j, False) for b in range(j, n)] for j in range(n)]
    if m > 2:
        terms += [[(b - j - 1, j, True) for b in range(j + 1, n)] for j in range(n - 1)]
    return terms


def mul_terms(lhs, rhs, m, c):
    """The dense terms (zeros below first_block) of lhs * rhs, and their first_block.  The products are taken on the
    block values; the library's bivariate lookup packs m x + y, which fits under m c only at c >= m
    (``mul_supported``)."""
    n = len(lhs)
    first = mul_first_block(n, m)
    terms = [[0] * f + [(lhs[x] * rhs[y]) // m if msb else (lhs[x] * rhs[y]) % m for x, y, msb in row]
             for f, row in zip(first, mul_pairs(n, m))]
    return terms, first


def mul_supported(m, c):
    return supported(m, c) and c == m


def mul(lhs, rhs, m, c, rule=None):
    terms, first = mul_terms(lhs, rhs, m, c)
    return sum_terms(terms, first, len(lhs), m, c, rule)


def schedule(n_blocks, first_block, m, c):
    """The data-independent schedule on labels.  Initial rows are labelled ("t", term, block); round r's outputs
    ("m", r, chunk) and ("c", r, chunk), chunks numbered in the order run_rounds makes them (columns ascending).
    Returns a dict: s; rounds = per round the list over chunks of (column, rows, want_carry); lens = the column lengths
    before every round and, last, at the end; chunks = the chunk counts per round and column; final = the final
    columns."""
    labels = [[("t", t, b) for b in range(n_blocks)] for t in range(len(first_block))]
    made = []

    def on_chunk(rows, column, want_carry, rnd):
        while len(made) <= rnd:
            made.append([])
        k = len(made[rnd])
        made[rnd].append((column, list(rows), want_carry))
        return ("m", rnd, k), (("c", rnd, k) if want_carry else None)

    columns, rounds = run_rounds(initial_columns(labels, first_block, n_blocks), m, c, on_chunk)
    return {"s": max_sum_size(m, c), "rounds": made, "lens": [[l for l, _ in r] for r in rounds] + [[len(x) for x in columns]],
            "chunks": [[q for _, q in r] for r in rounds], "final": columns}
