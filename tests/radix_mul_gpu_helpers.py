"""The written sequences of the radix sum and multiplication (public calls only, driven by the schedule of the Python
model tests/radix_sum_ref.py), which mi_radix_sum_batch and mi_radix_mul_batch are defined to equal bit for bit, and the
library's documented slot numbering restated for the index-array test."""
import ctypes

import numpy as np

import radix_sum_ref as S
import shortint_gpu_helpers as G

NONE = G.NONE
LUT_MSG, LUT_CARRY, LUT_MUL_LSB, LUT_MUL_MSB = 0, 1, 5, 6


def key_luts(sk):
    """The seven lookup tables of the key: the five of the propagation, then (x y) mod m and (x y) / m on m x + y."""
    import torch
    m = sk.message_modulus
    mul = [sk.generate_lookup_table_bivariate(lambda x, y: (x * y) % m),
           sk.generate_lookup_table_bivariate(lambda x, y: (x * y) // m)]
    return torch.cat([G.key_luts(sk), torch.stack(mul)]).contiguous()


def c_stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def c_sum(engine, sk, out, terms, n_terms, first_block, blocks, n_int):
    fb = (ctypes.c_uint32 * max(n_terms, 1))(*first_block) if first_block is not None else None
    return engine._lib.lib().mi_radix_sum_batch(sk._h, out.data_ptr(), terms.data_ptr() if terms is not None else None,
                                                n_terms, fb, blocks, n_int, c_stream())


def c_mul(engine, sk, out, lhs, rhs, blocks, n_int):
    return engine._lib.lib().mi_radix_mul_batch(sk._h, out.data_ptr(), lhs.data_ptr(), rhs.data_ptr(), blocks, n_int,
                                                c_stream())


def seq_sum(engine, sk, out, terms, first_block=None):
    """mi_radix_sum_batch as LC / APPLY / full-propagate calls.  terms (T, I, B, size) or None; out (I, B, size)."""
    import torch
    LA = engine.lwe_linear_algebra
    n_int, blocks, size = out.shape
    flat_out = out.reshape(n_int * blocks, size)
    n_terms = 0 if terms is None else int(terms.shape[0])
    if n_terms == 0:
        LA.lwe_linear_combination(flat_out, None, None)
        return
    m, c = sk.message_modulus, sk.carry_modulus
    sched = S.schedule(blocks, list(first_block) if first_block is not None else [0] * n_terms, m, c)
    s = sched["s"]
    pool = terms.reshape(n_terms * n_int * blocks, size)
    luts = key_luts(sk)
    i = np.arange(n_int)

    base = {}  # label -> (row of integer 0, stride over the integers)
    for t in range(n_terms):
        for b in range(blocks):
            base[("t", t, b)] = (t * n_int * blocks + b, blocks)

    def rows(label):
        r0, stride = base[label]
        return r0 + i * stride

    for rnd, chunks in enumerate(sched["rounds"]):
        index = np.stack([np.stack([rows(l) for l in chunk_rows], axis=1) for _, chunk_rows, _ in chunks])  # (C, I, s)
        sums = G.zeros((len(chunks) * n_int, size))
        LA.lwe_linear_combination(sums, pool, G.i32(index.reshape(-1, s)))
        items = []
        for k, (_, _, want_carry) in enumerate(chunks):
            items.append((("m", rnd, k), k, LUT_MSG))
            if want_carry:
                items.append((("c", rnd, k), k, LUT_CARRY))
        outs = G.zeros((len(items) * n_int, size))
        in_index = np.concatenate([k * n_int + i for _, k, _ in items])
        lut_index = np.concatenate([np.full(n_int, lut) for _, _, lut in items])
        sk.apply_lookup_table_batch(outs, sums, luts, G.i32(lut_index), G.i32(in_index))
        for j, (label, _, _) in enumerate(items):
            base[label] = (int(pool.shape[0]) + j * n_int, 1)
        pool = torch.cat([pool, outs]).contiguous()
    index = np.full((n_int, blocks, s), NONE, dtype=np.int64)
    for b, col in enumerate(sched["final"]):
        for p, label in enumerate(col):
            index[:, b, p] = rows(label)
    LA.lwe_linear_combination(flat_out, pool, G.i32(index.reshape(-1, s)))
    engine.integer.ServerKey(sk).full_propagate_parallelized(
        engine.integer.RadixCiphertext(out, [sk.max_degree] * blocks))


def mul_dense_terms(engine, sk, lhs, rhs, fill=0):
    """The pack, the lookup and the scatter of mi_radix_mul_batch: the dense terms (T, I, B, size) of lhs * rhs, rows
    below first_block holding `fill` words, and their first_block."""
    import torch
    LA = engine.lwe_linear_algebra
    n_int, blocks, size = lhs.shape
    m = sk.message_modulus
    total = n_int * blocks
    both = torch.cat([lhs.reshape(total, size), rhs.reshape(total, size)]).contiguous()
    pairs = [(d - y, y) for d in range(blocks) for y in range(d + 1)]
    pair_id = {p: k for k, p in enumerate(pairs)}
    i = np.arange(n_int)
    index = np.stack([np.stack([i * blocks + x, total + i * blocks + y], axis=1) for x, y in pairs])  # (P, I, 2)
    pack = G.zeros((len(pairs) * n_int, size))
    coeff = G.dev(np.tile(np.array([m, 1], np.int64), (len(pairs) * n_int, 1)))
    LA.lwe_linear_combination(pack, both, G.i32(index.reshape(-1, 2)), coeff)
    first = S.mul_first_block(blocks, m)
    items = [(t, f + k, x, y, msb) for t, (f, row) in enumerate(zip(first, S.mul_pairs(blocks, m)))
             for k, (x, y, msb) in enumerate(row)]
    in_index = np.concatenate([pair_id[(x, y)] * n_int + i for _, _, x, y, _ in items])
    lut_index = np.concatenate([np.full(n_int, LUT_MUL_MSB if msb else LUT_MUL_LSB) for *_, msb in items])
    prods = G.zeros((len(items) * n_int, size))
    sk.apply_lookup_table_batch(prods, pack, key_luts(sk), G.i32(lut_index), G.i32(in_index))
    dense = torch.full((len(first), n_int, blocks, size), fill, dtype=torch.int64, device="cuda")
    dst = np.concatenate([(t * n_int + i) * blocks + b for t, b, *_ in items])
    dense.reshape(-1, size)[torch.from_numpy(dst).cuda()] = prods
    return dense, first


def seq_mul(engine, sk, out, lhs, rhs):
    """mi_radix_mul_batch as its definition: pack, lookup, scatter into dense terms (the rows below first_block hold a
    sentinel, which nothing reads), the sum of those terms."""
    dense, first = mul_dense_terms(engine, sk, lhs, rhs, fill=int(G.SENTINEL))
    seq_sum(engine, sk, out, dense, first)


def model_index_arrays(blocks, n_int, m, c):
    """What mi_radix_mul_index_arrays documents, from the model's schedule: per step a dict of numpy arrays (index,
    coeff, in_index, lut_index; absent ones None).  Slots: the products column-major in chain order, then every
    round's outputs column by column, the carries of column b - 1's chunks before the messages of column b's."""
    i = np.arange(n_int)
    first = S.mul_first_block(blocks, m)
    sched = S.schedule(blocks, first, m, c)
    s = sched["s"]
    pairs = [(d - y, y) for d in range(blocks) for y in range(d + 1)]
    pair_id = {p: k for k, p in enumerate(pairs)}
    what = {("t", t, f + k): p for t, (f, row) in enumerate(zip(first, S.mul_pairs(blocks, m))) for k, p in enumerate(row)}
    slot = {}
    columns = S.initial_columns([[("t", t, b) for b in range(blocks)] for t in range(len(first))], first, blocks)
    for col in columns:
        for label in col:
            slot[label] = len(slot)
    steps = []
    # step 0: the pack and the product round
    index = np.stack([np.stack([i * blocks + x, n_int * blocks + i * blocks + y], axis=1) for x, y in pairs])
    order = sorted(slot, key=slot.get)
    in_index = np.concatenate([pair_id[what[l][:2]] * n_int + i for l in order])
    lut_index = np.concatenate([np.full(n_int, LUT_MUL_MSB if what[l][2] else LUT_MUL_LSB) for l in order])
    steps.append({"index": index.reshape(-1), "coeff": np.tile(np.array([m, 1], np.int64), len(pairs) * n_int),
                  "in_index": in_index, "lut_index": lut_index})
    for rnd, chunks in enumerate(sched["rounds"]):
        index = np.stack([np.stack([slot[l] * n_int + i for l in rows], axis=1) for _, rows, _ in chunks])
        items = []
        for b in range(blocks):
            items += [(("c", rnd, k), k, LUT_CARRY) for k, (col, _, w) in enumerate(chunks) if col == b - 1 and w]
            items += [(("m", rnd, k), k, LUT_MSG) for k, (col, _, _) in enumerate(chunks) if col == b]
        for label, _, _ in items:
            slot[label] = len(slot)
        steps.append({"index": index.reshape(-1), "coeff": None,
                      "in_index": np.concatenate([k * n_int + i for _, k, _ in items]),
                      "lut_index": np.concatenate([np.full(n_int, lut) for _, _, lut in items])})
    index = np.full((n_int, blocks, s), NONE, dtype=np.int64)
    for b, col in enumerate(sched["final"]):
        for p, label in enumerate(col):
            index[:, b, p] = slot[label] * n_int + i
    steps.append({"index": index.reshape(-1), "coeff": None, "in_index": None, "lut_index": None})
    return steps
