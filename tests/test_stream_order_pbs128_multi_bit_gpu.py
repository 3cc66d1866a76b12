"""The stream contract of the multi-bit 128-bit bootstrap (``mi_pbs128_multi_bit_*``), through the delayed-operand
harness of tests/stream_order.py (its docstring says what a run shows):

  mi_pbs128_multi_bit_blind_rotate_batch     test_async_entries[blind_rotate]   H
  mi_pbs128_multi_bit_batch                  test_async_entries[pbs]            H, test_hand_over   O
  mi_pbs128_multi_bit_key_create             test_key_create                    S

H: the entry on a non-blocking stream behind the delay reads the true operands and returns while the delay is pending;
O: two non-blocking streams take turns on one scratch block; S: the entry synchronises the stream and builds the key from
the delayed operands.  Shapes: tests/test_pbs128_multi_bit_gpu.py's smallest (N = 256, k = 1, base 2^23, 1 level, g = 2),
two groups."""
import numpy as np
import pytest

import pbs128_helpers as R
import pbs128_multi_bit_helpers as H
import stream_order as SO

pytestmark = pytest.mark.gpu

N, K, BASE_LOG, LEVEL, G, GROUPS = 256, 1, 23, 1, 2, 2
N_LWE = G * GROUPS


def zeros(shape):
    import torch
    return torch.zeros(shape, dtype=torch.int64, device="cuda")


def host(t):
    return t.cpu().numpy().view(np.uint64)


def u64s(rng, shape):
    return rng.integers(0, R.M64, size=shape, dtype=np.uint64)


def glwes(rng, count):
    return tuple(R.to_words([R.uniform_glwe(rng, K, N) for _ in range(count)]) for _ in range(2))


def rotated(accs, lwes, words):
    return [H.blind_rotate(acc, [int(x) for x in lwe], words, BASE_LOG, LEVEL, G) for acc, lwe in zip(accs, lwes)]


@pytest.mark.parametrize("entry", ["blind_rotate", "pbs"])
def test_async_entries(engine, entry):
    M = engine.pbs128
    batch = 2
    rng = R.rng(0x1280 + len(entry))
    words = H.uniform_key_words(rng, GROUPS, G, K, N, LEVEL)
    key = M.LweMultiBitBootstrapKey128(SO.to_dev(words), BASE_LOG, LEVEL, G)
    lwes = (u64s(rng, (batch, N_LWE + 1)), u64s(rng, (batch, N_LWE + 1)))
    lwe = zeros((batch, N_LWE + 1))
    if entry == "blind_rotate":
        a = zeros((batch, K + 1, N, 2))
        case = SO.Case("pbs128-multi-bit-blind-rotate", lambda: M.multi_bit_blind_rotate_assign(key, a, lwe),
                       [(a, *glwes(rng, batch)), (lwe, *lwes)], [a],
                       lambda v: [R.to_words(rotated(R.from_words(v[0]), v[1], words))])
    else:
        lut, out = zeros((K + 1, N, 2)), zeros((batch, K * N + 1, 2))
        v_lut = tuple(x[0] for x in glwes(rng, 1))
        case = SO.Case("pbs128-multi-bit-pbs",
                       lambda: M.multi_bit_programmable_bootstrap_f128_lwe_ciphertext(lwe, out, lut, key),
                       [(lut, *v_lut), (lwe, *lwes)], [out],
                       lambda v: [R.to_words([R.sample_extract(acc)
                                              for acc in rotated([R.from_words(v[0])] * batch, v[1], words)])])
    SO.check_case(engine, case)


def test_key_create(engine):
    """_create prepares a private copy on `stream` and synchronises it: the key is built from the true operands that
    arrive behind the delay, and the delay has drained when the call returns.  The key is then used once, on the same
    stream."""
    import torch

    M = engine.pbs128
    batch = 2
    rng = R.rng(0x1291)
    vals = (H.uniform_key_words(rng, GROUPS, G, K, N, LEVEL), H.uniform_key_words(rng, GROUPS, G, K, N, LEVEL))
    acc_h = R.to_words([R.uniform_glwe(rng, K, N) for _ in range(batch)])
    lwe_h = u64s(rng, (batch, N_LWE + 1))
    acc0, lwe = SO.to_dev(acc_h), SO.to_dev(lwe_h)
    src, out = zeros(vals[0].shape), zeros(acc_h.shape)
    made = []  # the keys stay alive until the streams are idle

    def call():
        made.append(M.LweMultiBitBootstrapKey128(src, BASE_LOG, LEVEL, G))
        out.copy_(acc0)
        M.multi_bit_blind_rotate_assign(made[-1], out, lwe)

    want = lambda v: [R.to_words(rotated(R.from_words(acc_h), lwe_h, v[0]))]
    SO.check_case(engine, SO.Case("create-pbs128-multi-bit-key", call, [(src, *vals)], [out], want, sync=True))
    torch.cuda.synchronize()
    made.clear()


def test_hand_over(engine):
    """Two non-blocking streams take turns on one scratch block (accumulators, digits and limb products of a chunk):
    eight calls in four rounds, the first of a round behind the delay, the second (the other stream, other inputs, same
    size) right away.  Every call equals the helper, the second call of a round completes only behind the first one, and
    the pool ends up holding what the same calls leave on one stream."""
    M = engine.pbs128
    sizes = [3, 1, 4, 2]
    rng = R.rng(0x12A2)
    words = H.uniform_key_words(rng, GROUPS, G, K, N, LEVEL)
    key = M.LweMultiBitBootstrapKey128(SO.to_dev(words), BASE_LOG, LEVEL, G)
    lut = {s: R.uniform_glwe(rng, K, N) for s in "AB"}
    lwe = {s: u64s(rng, (max(sizes), N_LWE + 1)) for s in "AB"}
    dt, dl = {s: SO.to_dev(R.to_words(lut[s])) for s in "AB"}, {s: SO.to_dev(lwe[s]) for s in "AB"}
    outs = {}

    def reset():
        outs.clear()
        outs.update({(s, r): zeros((b, K * N + 1, 2)) for r, b in enumerate(sizes) for s in "AB"})
        outs.update({(s, -1): zeros((sizes[0], K * N + 1, 2)) for s in "AB"})

    def issue(side, r, size):
        M.multi_bit_programmable_bootstrap_f128_lwe_ciphertext(dl[side][:size], outs[(side, r)], dt[side], key)

    reset()
    single, shared, first_done = SO.hand_over(engine, issue, sizes, reset)
    assert single > 0, "this entry took no scratch"
    assert shared == single, f"the pool holds {shared} bytes after the two-stream run, {single} after the same calls on one"
    assert all(first_done), f"rounds {[r for r, d in enumerate(first_done) if not d]}: the second call finished before " \
                            "the first one: it did not wait for the scratch block's last user"
    want = {s: R.to_words([R.sample_extract(acc) for acc in rotated([lut[s]] * max(sizes), lwe[s], words)]) for s in "AB"}
    for (s, r), out in outs.items():
        if r >= 0:
            assert np.array_equal(host(out), want[s][:sizes[r]]), f"stream {s}, round {r} differs from the helper"
