"""The stream contract of the radix sum and multiplication, through the delayed-operand harness of
tests/stream_order.py (its docstring says what a run shows):

  mi_radix_sum_batch    test_async_entries[sum]   H, test_hand_over[sum]  O
  mi_radix_mul_batch    test_async_entries[mul]   H, test_hand_over[mul]  O

H: the entry on a non-blocking stream behind the delay reads the true operands and returns while the delay is pending
(its schedule is made on the host and reaches the index kernels as arguments: nothing is copied, nothing waits);
O: two non-blocking streams take turns on the entry's scratch.  Uniform key words at N = 1024, n = 16, the NTT engine
with the drift key; 4 blocks (a round of the schedule and the block sums), the sum over 7 ragged terms.  Both are
compared with a quiescent run of the same call."""
import pytest

import radix_mul_gpu_helpers as RM
import shortint_gpu_helpers as G
import stream_order as SO
import tfhe_helpers as H

pytestmark = pytest.mark.gpu

ENTRIES = ["sum", "mul"]
BLOCKS = 4
FIRST = [0, 0, 1, 2, 2, 0, 1]


def two(make):
    return make(), make()


def build(engine, oracle, entry, batch, g):
    """(call, operands, outputs) of one entry at `batch` integers."""
    ks = G.key_set(engine, oracle, "u1024")
    sk = ks.server("ntt", drift=True)
    u = lambda shape: H.uniform_u64(g, shape)
    out = G.zeros((batch, BLOCKS, ks.size))
    if entry == "sum":
        terms = G.zeros((len(FIRST), batch, BLOCKS, ks.size))

        def call():
            engine._lib.check(RM.c_sum(engine, sk, out, terms, len(FIRST), FIRST, BLOCKS, batch))
        return call, [(terms, *two(lambda: u(tuple(terms.shape))))], [out]
    lhs, rhs = G.zeros((batch, BLOCKS, ks.size)), G.zeros((batch, BLOCKS, ks.size))

    def call():
        engine._lib.check(RM.c_mul(engine, sk, out, lhs, rhs, BLOCKS, batch))
    return call, [(lhs, *two(lambda: u(tuple(lhs.shape)))), (rhs, *two(lambda: u(tuple(rhs.shape))))], [out]


@pytest.mark.parametrize("entry", ENTRIES)
def test_async_entries(engine, oracle, entry):
    call, operands, outputs = build(engine, oracle, entry, 3, H.rng(0x5f10 + ENTRIES.index(entry)))
    SO.check_case(engine, SO.Case("radix-" + entry, call, operands, outputs, None))


@pytest.mark.parametrize("entry", ENTRIES)
def test_hand_over(engine, oracle, entry):
    """Two non-blocking streams take turns on the entry's scratch: eight calls in four rounds, the first of a round
    behind the delay, the second (the other stream, other inputs, same size) right away.  The second call of a round
    completes only behind the first one, the pool ends up holding what the same calls leave on one stream, and every
    call equals a quiescent run of the same call."""
    import torch

    sizes = [3, 1, 4, 2]
    built = {}

    def fill():
        for call, operands, outputs in built.values():
            for buf, true, _ in operands:
                buf.copy_(SO.to_dev(true))
            for t in outputs:
                SO.sentinel_fill(t)
        torch.cuda.synchronize()

    for side in "AB":
        for r, size in list(enumerate(sizes)) + [(-1, sizes[0])]:
            seed = 0x5f40 + 64 * ENTRIES.index(entry) + 16 * "AB".index(side) + r + 1
            built[(side, r)] = build(engine, oracle, entry, size, H.rng(seed))
    fill()
    single, shared, first_done = SO.hand_over(engine, lambda side, r, size: built[(side, r)][0](), sizes, fill)
    assert single > 0, "this entry took no scratch"
    assert shared == single, f"the pool holds {shared} bytes after the two-stream run, {single} after the same calls on one"
    assert all(first_done), f"rounds {[r for r, d in enumerate(first_done) if not d]}: the second call finished before " \
                            "the first one: it did not wait for the scratch block's last user"
    torch.cuda.synchronize()
    got = {key: [t.clone() for t in outputs] for key, (_, _, outputs) in built.items() if key[1] >= 0}
    fill()
    for key, (call, _, outputs) in built.items():  # the same calls on an idle device
        if key[1] >= 0:
            call()
            torch.cuda.synchronize()
            for a, b in zip(got[key], outputs):
                assert torch.equal(a, b), f"stream {key[0]}, round {key[1]} differs from the quiescent run"
