"""The stream contract of the shortint / radix entries, through the delayed-operand harness of tests/stream_order.py
(its docstring says what a run shows):

  mi_lwe_linear_combination_batch            test_async_entries[lincomb]          H
  mi_shortint_apply_lut_batch                test_async_entries[apply, apply-fft] H, test_hand_over O
  mi_radix_propagate_single_carry_batch      test_async_entries[propagate]        H, test_hand_over O
                                             test_async_propagate_on_the_lane_driver  H (N = 8192, forked lanes)
  mi_radix_full_propagate_batch              test_async_entries[full-propagate]   H, test_hand_over O
  mi_radix_add_batch                         test_async_entries[add]              H, test_hand_over O

H: the entry on a non-blocking stream behind the delay reads the true operands and returns while the delay is pending;
O: two non-blocking streams take turns on the entry's scratch.  Uniform key words at N = 1024, n = 16 (the stream contract
does not need encryptions); "apply" runs the NTT engine with the drift key and both index arrays, the radix entries
the NTT engine with the drift key, "apply-fft" the f64 engine.  The linear combination is compared with numpy, the
others with a quiescent run of the same call."""
import numpy as np
import pytest

import shortint_gpu_helpers as G
import stream_order as SO
import tfhe_helpers as H

pytestmark = pytest.mark.gpu

ENTRIES = ["lincomb", "apply", "apply-fft", "propagate", "full-propagate", "add"]
BLOCKS = 3


def two(make):
    return make(), make()


def build(engine, oracle, entry, batch, g):
    """(call, operands, outputs, want) of one entry at `batch` items / integers."""
    ks = G.key_set(engine, oracle, "u1024")
    u = lambda shape: H.uniform_u64(g, shape)
    size = ks.size
    if entry == "lincomb":
        LA = engine.lwe_linear_algebra
        src, out = G.zeros((batch + 1, size)), G.zeros((batch, size))
        index = np.stack([np.arange(batch), np.arange(batch) + 1], axis=1).astype(np.uint32)
        coeff = np.tile(np.array([3, -1], np.int64), (batch, 1))
        d_index, d_coeff = G.i32(index), G.dev(coeff)
        call = lambda: LA.lwe_linear_combination(out, src, d_index, d_coeff)

        def want(v):
            with np.errstate(over="ignore"):
                return [np.uint64(3) * v[0][:-1] - v[0][1:]]
        return call, [(src, *two(lambda: u((batch + 1, size))))], [out], want
    if entry in ("apply", "apply-fft"):
        sk = ks.server("ntt", drift=True) if entry == "apply" else ks.server("fft")
        lwe, luts, out = G.zeros((batch, size)), G.zeros((2, 2, ks.n)), G.zeros((2 * batch, size))
        in_index, lut_index = G.i32(np.arange(2 * batch) % batch), G.i32(np.arange(2 * batch) // batch)
        call = lambda: sk.apply_lookup_table_batch(out, lwe, luts, lut_index, in_index)
        return call, [(lwe, *two(lambda: u((batch, size)))), (luts, *two(lambda: u((2, 2, ks.n))))], [out], None
    I = engine.integer.ServerKey(ks.server("ntt", drift=True))
    radix = G.zeros((batch, BLOCKS, size))
    if entry == "propagate":
        carry = G.zeros((batch, size))
        call = lambda: I._propagate_single_carry(radix, carry)
        return call, [(radix, *two(lambda: u((batch, BLOCKS, size))))], [radix, carry], None
    if entry == "full-propagate":
        call = lambda: I.full_propagate_parallelized(engine.integer.RadixCiphertext(radix, [15] * BLOCKS))
        return call, [(radix, *two(lambda: u((batch, BLOCKS, size))))], [radix], None
    rhs, out, carry = G.zeros((batch, BLOCKS, size)), G.zeros((batch, BLOCKS, size)), G.zeros((batch, size))
    lib, key = engine._lib.lib(), I.key
    import ctypes
    import torch

    def call():
        s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        engine._lib.check(lib.mi_radix_add_batch(key._h, out.data_ptr(), radix.data_ptr(), rhs.data_ptr(),
                                                 carry.data_ptr(), BLOCKS, batch, s))
    return call, [(radix, *two(lambda: u((batch, BLOCKS, size)))), (rhs, *two(lambda: u((batch, BLOCKS, size))))], \
        [out, carry], None


@pytest.mark.parametrize("entry", ENTRIES)
def test_async_entries(engine, oracle, entry):
    call, operands, outputs, want = build(engine, oracle, entry, 3, H.rng(0x5d10 + ENTRIES.index(entry)))
    SO.check_case(engine, SO.Case("shortint-" + entry, call, operands, outputs, want))


@pytest.mark.parametrize("entry", [e for e in ENTRIES if e != "lincomb"])
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
                if not any(t is o[0] for o in operands):
                    SO.sentinel_fill(t)
        torch.cuda.synchronize()

    for side in "AB":
        for r, size in list(enumerate(sizes)) + [(-1, sizes[0])]:
            seed = 0x5e00 + 64 * ENTRIES.index(entry) + 16 * "AB".index(side) + r + 1
            built[(side, r)] = build(engine, oracle, entry, size, H.rng(seed))[:3]
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


def test_async_propagate_on_the_lane_driver(engine, oracle):
    """H for mi_radix_propagate_single_carry_batch where the bootstrap is the multi-pass one: N = 8192 (pbs_large.hip) at
    m = c = 8, 8 integers of 5 blocks.  Round 1 is 80 items, which the chunk-and-lane driver runs on side streams
    (pbs_passes.hpp lanes_wanted), the scan rounds 40 items with kept blocks on the caller's stream alone: the
    composite's scratch and the forked lanes keep the contract together."""
    ks = G.key_set(engine, oracle, "u8192")
    I = engine.integer.ServerKey(ks.server("ntt", m=8, c=8))
    g = H.rng(0x5d20)
    n_int, blocks = 8, 5
    radix, carry = G.zeros((n_int, blocks, ks.size)), G.zeros((n_int, ks.size))
    call = lambda: I._propagate_single_carry(radix, carry)
    operands = [(radix, *two(lambda: H.uniform_u64(g, (n_int, blocks, ks.size))))]
    SO.check_case(engine, SO.Case("shortint-propagate-8192", call, operands, [radix, carry], None))
