"""The stream contract of the WoP-PBS entries, through the delayed-operand harness of tests/stream_order.py (its
docstring says what a run shows):

  mi_lwe_pfpks_batch                                            test_async_entries[pfpks]          H, test_hand_over O
  mi_fft64_ext_product_batch_indexed                            test_async_entries[ext-indexed]    H
  mi_fft64_cmux_batch_indexed                                   test_async_entries[cmux-indexed]   H, test_hand_over O
  mi_fft64_extract_bits_batch                                   test_async_entries[extract-bits]   H, test_hand_over O
  mi_fft64_circuit_bootstrap_boolean_batch                      test_async_entries[cbs]            H, test_hand_over O
  mi_fft64_cmux_tree_batch                                      test_async_entries[tree]           H, test_hand_over O
  mi_fft64_wop_blind_rotate_batch                               test_async_entries[rotate]         H, test_hand_over O
  mi_fft64_vertical_packing_batch                               test_async_entries[packing]        H, test_hand_over O
  mi_fft64_circuit_bootstrap_boolean_vertical_packing_batch     test_async_entries[cbs-packing]    H, test_hand_over O
  mi_lwe_pfpksk_list_create                                     test_key_create                    S

H: the entry on a non-blocking stream behind the delay reads the true operands and returns while the delay is pending;
O: two non-blocking streams take turns on the entry's scratch; S: the entry synchronises the stream and builds the key
from the delayed operands.  Shape A of tests/wopbs_helpers.py (N = 256: the generic f64 engine, whose external product
takes scratch) with uniform key words: the f64 entries are compared with a quiescent run of the same call."""
import pytest

import stream_order as SO
import tfhe_helpers as H
import wopbs_helpers as W

pytestmark = pytest.mark.gpu

S = W.SHAPE_A
K, N, SMALL1, BIG1 = S.k, S.N, S.n + 1, S.k * S.N + 1
LEVEL = S.cbs[1]
N_BITS, N_OUT, N_POLYS = 3, 2, 4   # 3 GGSWs per item: a tree of 2 layers and 1 rotation step
ENTRIES = ["pfpks", "ext-indexed", "cmux-indexed", "extract-bits", "cbs", "tree", "rotate", "packing", "cbs-packing"]
_keys = {}


def zeros(shape):
    import torch
    return torch.zeros(shape, dtype=torch.int64, device="cuda")


def fzeros(shape):
    import torch
    return torch.zeros(shape, dtype=torch.float64, device="cuda")


def keys(engine):
    """Uniform key words (the stream contract does not need encryptions), made once."""
    if not _keys:
        X, KS, M = engine.fft64, engine.lwe_keyswitch, engine.lwe_wopbs
        g = H.rng(0x5700)
        fft = X.Fft(N)
        fbsk = fzeros((S.n, S.pbs[1], K + 1, K + 1, N // 2, 2))
        X.convert_standard_lwe_bootstrap_key_to_fourier(SO.to_dev(H.uniform_u64(g, (S.n, S.pbs[1], K + 1, K + 1, N))),
                                                        fbsk, fft)
        pf = H.uniform_u64(g, (K + 1, K * N + 1, S.pfks[1], K + 1, N))
        _keys.update(fft=fft, bsk=X.FourierLweBootstrapKey(fbsk, *S.pbs, fft), pf_words=pf,
                     ksk=KS.LweKeyswitchKey(SO.to_dev(H.uniform_u64(g, (K * N, S.ks[1], SMALL1))), *S.ks),
                     pfpksk=M.LwePrivateFunctionalPackingKeyswitchKeyList(SO.to_dev(pf), *S.pfks))
    return _keys


def fourier_ggsws(engine, g, batch, count):
    """Host float64 (batch, count, level, k+1, k+1, N/2, 2) Fourier GGSWs in the plan's order."""
    out = fzeros((batch, count, LEVEL, K + 1, K + 1, N // 2, 2))
    keys(engine)["fft"].forward_as_torus(out, SO.to_dev(H.uniform_u64(g, (batch, count, LEVEL, K + 1, K + 1, N))))
    return out.cpu().numpy()


def two(make):
    return make(), make()


def build(engine, entry, batch, g):
    """(call, operands, outputs, want) of one entry at `batch` items; operands hold (buffer, true values, decoys)."""
    X, M = engine.fft64, engine.lwe_wopbs
    ks = keys(engine)
    u = lambda shape: H.uniform_u64(g, shape)
    if entry == "pfpks":
        lwe, out = zeros((batch, BIG1)), zeros((batch, K + 1, K + 1, N))
        call = lambda: M.private_functional_keyswitch_lwe_ciphertext_into_glwe_ciphertext(ks["pfpksk"], out, lwe)
        return call, [(lwe, *two(lambda: u((batch, BIG1))))], [out], lambda v: [W.pfpks_ref(ks["pf_words"], v[0], *S.pfks)]
    if entry in ("ext-indexed", "cmux-indexed"):
        import torch
        n_ggsw = 3
        fg = SO.to_dev(fourier_ggsws(engine, g, 1, n_ggsw)[0])
        index = torch.tensor([(2 * b + 1) % n_ggsw for b in range(batch)], dtype=torch.int32, device="cuda")
        acc, glwe = zeros((batch, K + 1, N)), zeros((batch, K + 1, N))
        if entry == "cmux-indexed":
            call = lambda: X.cmux_assign(acc, glwe, fg, *S.cbs, ks["fft"], ggsw_index=index)
            outs = [acc, glwe]
        else:
            call = lambda: X.add_external_product_assign(acc, fg, glwe, *S.cbs, ks["fft"], ggsw_index=index)
            outs = [acc]
        return call, [(acc, *two(lambda: u((batch, K + 1, N)))), (glwe, *two(lambda: u((batch, K + 1, N))))], outs, None
    if entry == "extract-bits":
        lwe, out = zeros((batch, BIG1)), zeros((batch, N_BITS, SMALL1))
        call = lambda: M.extract_bits_from_lwe_ciphertext_mem_optimized(lwe, out, ks["bsk"], ks["ksk"], 60, N_BITS)
        return call, [(lwe, *two(lambda: u((batch, BIG1))))], [out], None
    if entry == "cbs":
        lwe = zeros((batch, SMALL1))
        std, four = zeros((batch, LEVEL, K + 1, K + 1, N)), fzeros((batch, LEVEL, K + 1, K + 1, N // 2, 2))
        call = lambda: M.circuit_bootstrap_boolean(ks["bsk"], lwe, 60, ks["pfpksk"], *S.cbs, std, four, ks["fft"])
        return call, [(lwe, *two(lambda: u((batch, SMALL1))))], [std, four], None
    luts = zeros((N_OUT, N_POLYS, N))
    v_luts = two(lambda: u((N_OUT, N_POLYS, N)))
    if entry == "cbs-packing":
        bits, out = zeros((batch, N_BITS, SMALL1)), zeros((batch, N_OUT, K * N + 1))
        call = lambda: M.circuit_bootstrap_boolean_vertical_packing_lwe_ciphertext_list_mem_optimized(
            bits, out, luts, ks["bsk"], ks["pfpksk"], *S.cbs, ks["fft"])
        return call, [(bits, *two(lambda: u((batch, N_BITS, SMALL1)))), (luts, *v_luts)], [out], None
    count = {"tree": 2, "rotate": 3, "packing": N_BITS}[entry]
    ggsw = fzeros((batch, count, LEVEL, K + 1, K + 1, N // 2, 2))
    v_ggsw = two(lambda: fourier_ggsws(engine, g, batch, count))
    if entry == "tree":
        out = zeros((batch, N_OUT, K + 1, N))
        call = lambda: M.cmux_tree_memory_optimized(out, luts, ggsw, *S.cbs, ks["fft"])
        return call, [(luts, *v_luts), (ggsw, *v_ggsw)], [out], None
    if entry == "rotate":
        glwe = zeros((batch, N_OUT, K + 1, N))
        call = lambda: M.blind_rotate_assign(glwe, ggsw, *S.cbs, ks["fft"])
        return call, [(glwe, *two(lambda: u((batch, N_OUT, K + 1, N)))), (ggsw, *v_ggsw)], [glwe], None
    out = zeros((batch, N_OUT, K * N + 1))
    call = lambda: M.vertical_packing(luts, out, ggsw, *S.cbs, ks["fft"])
    return call, [(luts, *v_luts), (ggsw, *v_ggsw)], [out], None


@pytest.mark.parametrize("entry", ENTRIES)
def test_async_entries(engine, entry):
    call, operands, outputs, want = build(engine, entry, 3, H.rng(0x5710 + ENTRIES.index(entry)))
    SO.check_case(engine, SO.Case("wopbs-" + entry, call, operands, outputs, want))


def test_key_create(engine):
    """mi_lwe_pfpksk_list_create prepares a private copy on `stream` and synchronises it: the key is built from the true
    words that arrive behind the delay, and the delay has drained when the call returns.  The key is then used once, on
    the same stream."""
    import torch

    M = engine.lwe_wopbs
    g = H.rng(0x5720)
    shape = (K + 1, K * N + 1, S.pfks[1], K + 1, N)
    vals = (H.uniform_u64(g, shape), H.uniform_u64(g, shape))
    lwe_h = H.uniform_u64(g, (3, BIG1))
    lwe, src, out = SO.to_dev(lwe_h), zeros(shape), zeros((3, K + 1, K + 1, N))
    made = []  # the keys stay alive until the streams are idle

    def call():
        made.append(M.LwePrivateFunctionalPackingKeyswitchKeyList(src, *S.pfks))
        M.private_functional_keyswitch_lwe_ciphertext_into_glwe_ciphertext(made[-1], out, lwe)

    want = lambda v: [W.pfpks_ref(v[0], lwe_h, *S.pfks)]
    SO.check_case(engine, SO.Case("create-pfpksk-list", call, [(src, *vals)], [out], want, sync=True))
    torch.cuda.synchronize()
    made.clear()


@pytest.mark.parametrize("entry", [e for e in ENTRIES if e != "ext-indexed"])
def test_hand_over(engine, entry):
    """Two non-blocking streams take turns on the entry's scratch: eight calls in four rounds, the first of a round
    behind the delay, the second (the other stream, other inputs, same size) right away.  The second call of a round
    completes only behind the first one, the pool ends up holding what the same calls leave on one stream, and every
    call equals a quiescent run of the same call."""
    import torch

    sizes = [3, 1, 4, 2]
    built = {}

    def make():
        built.clear()
        for side in "AB":
            for r, size in list(enumerate(sizes)) + [(-1, sizes[0])]:
                call, operands, outputs, _ = build(engine, entry, size, H.rng(0x5800 + 64 * ENTRIES.index(entry) + 16 * "AB".index(side) + r + 1))
                for buf, true, _ in operands:
                    buf.copy_(SO.to_dev(true))
                built[(side, r)] = (call, operands, outputs)
        torch.cuda.synchronize()

    def reset():
        for call, operands, outputs in built.values():
            for buf, true, _ in operands:
                buf.copy_(SO.to_dev(true))
            for t in outputs:
                if not any(t is o[0] for o in operands):
                    SO.sentinel_fill(t)
        torch.cuda.synchronize()

    make()
    single, shared, first_done = SO.hand_over(engine, lambda side, r, size: built[(side, r)][0](), sizes, reset)
    assert single > 0, "this entry took no scratch"
    assert shared == single, f"the pool holds {shared} bytes after the two-stream run, {single} after the same calls on one"
    assert all(first_done), f"rounds {[r for r, d in enumerate(first_done) if not d]}: the second call finished before " \
                            "the first one: it did not wait for the scratch block's last user"
    torch.cuda.synchronize()
    got = {key: [t.clone() for t in outputs] for key, (_, _, outputs) in built.items() if key[1] >= 0}
    reset()
    for key, (call, _, outputs) in built.items():  # the same calls on an idle device
        if key[1] >= 0:
            call()
            torch.cuda.synchronize()
            for a, b in zip(got[key], outputs):
                assert torch.equal(a, b), f"stream {key[0]}, round {key[1]} differs from the quiescent run"
