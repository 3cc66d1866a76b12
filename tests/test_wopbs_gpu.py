"""GPU tests of the bootstrap without padding bit (`-m gpu`; references in tests/wopbs_helpers.py).

1. the private functional packing keyswitch, bit-exact against the restatement, with the decomposition's corner words
   in mask positions and in the body position, across the 256-row block of the GEMM; and the keyswitches that share
   the GEMM core still give the bits recorded before it changed (tests/golden/ks_before_pfpks.npz);
2. the f64 external product / CMUX with one GGSW per item: equal to the shared-GGSW call bit for bit, untouched items,
   and the project's accuracy criterion (tests/fft_accuracy.py);
3. every composite equals the sequence of public stages it is defined as, bit for bit;
4. decryption: extracted bits, the circuit bootstrap's GGSW, and test_wop_add_one end to end.
"""
import functools
import os

import numpy as np
import pytest

import decomp_corners as D
import fft_accuracy as A
import fft_oracle as F
import tfhe_helpers as H
import wopbs_helpers as W
from conftest import GOLDEN
from wopbs_gpu_helpers import (cbs_by_stages, dev, device_keys, extract_bits_by_stages, fzeros, host, idev, lut_polys,
                               random_fourier_ggsws, rotate_by_steps, same, tree_by_layers, zeros)

pytestmark = pytest.mark.gpu


# ---- 1. the private functional packing keyswitch -------------------------------------------------------------------
PFPKS_SHAPES = [(7, 1, 32, 15, 2, 2), (600, 2, 512, 4, 9, 3), (2048, 1, 2048, 15, 2, 2), (33, 1, 64, 63, 1, 1),
                (16, 1, 32, 1, 9, 2)]
MAX_ROWS = 300


@functools.lru_cache(maxsize=2)
def pfpks_case(oracle, shape):
    """Key words, MAX_ROWS input rows and their reference, once per shape.  Row r carries corner word r in the body
    position and the corpus rolled by r in every other mask position; the rows past the corpus are random."""
    in_dim, k, n, base_log, level, n_keys = shape
    g = H.rng(0x9F00 + in_dim + n + base_log)
    key = H.uniform_u64(g, (n_keys, in_dim + 1, level, k + 1, n))
    lwe = H.uniform_u64(g, (MAX_ROWS, in_dim + 1))
    words = D.corner_words(base_log, level)
    for r in range(min(MAX_ROWS, len(words))):
        lwe[r, in_dim] = words[r]
        for j in range(0, in_dim, 2):
            lwe[r, j] = words[(r + 1 + j // 2) % len(words)]
    return key, lwe, W.pfpks_ref_oracle(oracle, key, lwe, base_log, level)


@pytest.mark.parametrize("rows", [1, 3, MAX_ROWS])
@pytest.mark.parametrize("shape", PFPKS_SHAPES)
def test_pfpks_matches_restatement(engine, oracle, shape, rows):
    M = engine.lwe_wopbs
    in_dim, k, n, base_log, level, n_keys = shape
    key, lwe, want = pfpks_case(oracle, shape)
    if rows == 1 and in_dim <= 33:  # the numpy restatement itself, where it is cheap
        assert np.array_equal(want[:3], W.pfpks_ref(key, lwe[:3], base_log, level))
    dkey = M.LwePrivateFunctionalPackingKeyswitchKeyList(dev(key), base_log, level)
    out = zeros((rows, n_keys, k + 1, n), -1)  # every word must be written
    M.private_functional_keyswitch_lwe_ciphertext_into_glwe_ciphertext(dkey, out, dev(lwe[:rows]))
    assert np.array_equal(host(out), want[:rows])


def test_keyswitches_sharing_the_gemm_core_are_unchanged(engine):
    """mi_lwe_keyswitch_batch and mi_lwe_packing_keyswitch_batch on fixed inputs give the bits the library gave before
    the core learnt the key list (tests/golden/ks_before_pfpks.npz, recorded from the parent commit's library)."""
    gold = np.load(os.path.join(GOLDEN, "ks_before_pfpks.npz"))
    KS, PK = engine.lwe_keyswitch, engine.lwe_packing_keyswitch
    for i, (in_dim, out_dim, base_log, level, batch) in enumerate(W.GOLDEN_KS):
        ksk, lwe = W.golden_ks_inputs(i)
        out = zeros((batch, out_dim + 1), -1)
        KS.keyswitch_lwe_ciphertext(KS.LweKeyswitchKey(dev(ksk), base_log, level), dev(lwe), out)
        assert np.array_equal(host(out), gold[f"ks{i}"]), ("keyswitch", i)
    for i, (in_dim, k, n, base_log, level, per, n_lwe) in enumerate(W.GOLDEN_PKS):
        pksk, lwe = W.golden_pks_inputs(i)
        out = zeros(((n_lwe + per - 1) // per, k + 1, n), -1)
        PK.keyswitch_lwe_ciphertext_list_and_pack_in_glwe_ciphertext(PK.LwePackingKeyswitchKey(dev(pksk), base_log, level),
                                                                     dev(lwe), out, per)
        assert np.array_equal(host(out), gold[f"pks{i}"]), ("packing keyswitch", i)


# ---- 2. the external product / CMUX with one GGSW per item ---------------------------------------------------------
N_GGSW, INDEX = 3, [2, 0, 7, 1, 2]  # batch 5 over 3 GGSWs; 7 is out of range


@pytest.mark.parametrize("level,base_log", [(1, 23), (3, 8)])
@pytest.mark.parametrize("n,k", [(2048, 1), (2048, 2), (32, 1), (32, 3), (512, 1), (512, 3), (4096, 1), (4096, 3)])
def test_indexed_external_product_and_cmux(engine, oracle, n, k, level, base_log):
    X = engine.fft64
    fft = X.Fft(n)
    batch = len(INDEX)
    g = H.rng(0x1D00 + n + 16 * k + level)
    ggsw = H.uniform_u64(g, (N_GGSW, level, k + 1, k + 1, n))
    glwe, acc = H.uniform_u64(g, (batch, k + 1, n)), H.uniform_u64(g, (batch, k + 1, n))
    fg = fzeros((N_GGSW, level, k + 1, k + 1, n // 2, 2))
    fft.forward_as_torus(fg, dev(ggsw))
    d_glwe, d_acc = dev(glwe), dev(acc)

    def shared(cmux, gi):
        out, inp = d_acc.clone(), d_glwe.clone()
        (X.cmux_assign if cmux else X.add_external_product_assign)(out, *((inp, fg[gi]) if cmux else (fg[gi], inp)),
                                                                    base_log, level, fft)
        return out, inp

    def indexed(cmux, index):
        out, inp = d_acc.clone(), d_glwe.clone()
        if cmux:
            X.cmux_assign(out, inp, fg, base_log, level, fft, ggsw_index=idev(index))
        else:
            X.add_external_product_assign(out, fg, inp, base_log, level, fft, ggsw_index=idev(index))
        return out, inp

    for cmux in (False, True):
        per_ggsw = [shared(cmux, gi) for gi in range(N_GGSW)]
        for gi in range(N_GGSW):  # every index equal to gi: the shared call on GGSW gi, bit for bit
            out, inp = indexed(cmux, [gi] * batch)
            assert same(out, per_ggsw[gi][0]) and same(inp, per_ggsw[gi][1]), (cmux, gi)
        out, inp = indexed(cmux, INDEX)
        for b, gi in enumerate(INDEX):
            if gi < N_GGSW:  # item b equals the shared call on its own GGSW
                assert same(out[b], per_ggsw[gi][0][b]) and same(inp[b], per_ggsw[gi][1][b]), (cmux, b)
            else:            # untouched, ct1 of the CMUX included
                assert same(out[b], d_acc[b]) and same(inp[b], d_glwe[b]), (cmux, b)

    # accuracy: the project's criterion, on the mixed indices from a zero accumulator
    out = zeros((batch, k + 1, n))
    X.add_external_product_assign(out, fg, d_glwe, base_log, level, fft, ggsw_index=idev(INDEX))
    live = [b for b, gi in enumerate(INDEX) if gi < N_GGSW]
    want = np.stack([A.exact_ext_product(oracle, glwe[b], ggsw[INDEX[b]], base_log, level) for b in live])
    rest = np.stack([F.external_product(glwe[b], F.forward_as_torus(ggsw[INDEX[b]]), base_log, level) for b in live])
    ref, gpu = A.word_error_stats(rest, want), A.word_error_stats(host(out)[live], want)
    print(f"\nindexed ext product N={n} k={k} B={base_log} l={level}: numpy rms {ref[0]:.2e} max {ref[1]:.2e} | "
          f"gpu rms {gpu[0]:.2e} max {gpu[1]:.2e}", end="")
    assert A.within_margin(gpu, ref), (n, k, level, A.ratios(gpu, ref))


# ---- 3. structure, bit for bit --------------------------------------------------------------------------------------
STRUCT_SHAPES = [W.SHAPE_A, W.SHAPE_N2048]


@pytest.mark.parametrize("r", [0, 1, 3])
@pytest.mark.parametrize("shape", STRUCT_SHAPES, ids=lambda s: s.name)
def test_tree_equals_layered_cmux(engine, shape, r):
    M = engine.lwe_wopbs
    batch, n_out = 3, 2
    luts = lut_polys(shape, n_out, 1 << r, 0x7E00 + r)
    ggsw = random_fourier_ggsws(engine, shape, batch, r, 0x7E10 + r)
    out = zeros((batch, n_out, shape.k + 1, shape.N), -1)
    M.cmux_tree_memory_optimized(out, luts, ggsw, *shape.cbs)
    assert same(out, tree_by_layers(engine, shape, luts, ggsw, batch))


@pytest.mark.parametrize("n_rot", [1, 8, "log2(2N)+1"])
@pytest.mark.parametrize("shape", STRUCT_SHAPES, ids=lambda s: s.name)
def test_rotation_equals_stepwise_cmux(engine, shape, n_rot):
    M = engine.lwe_wopbs
    n_rot = shape.N.bit_length() + 1 if isinstance(n_rot, str) else n_rot  # the degree passes 2N
    batch, n_out = 3, 2
    glwe = dev(H.uniform_u64(H.rng(0x7F00 + n_rot), (batch, n_out, shape.k + 1, shape.N)))
    ggsw = random_fourier_ggsws(engine, shape, batch, n_rot, 0x7F10 + n_rot)
    want = rotate_by_steps(engine, shape, glwe, ggsw)
    M.blind_rotate_assign(glwe, ggsw, *shape.cbs)
    assert same(glwe, want)


@pytest.mark.parametrize("n_polys,n_ggsw", [(1, 3), (4, 2), (4, 5)], ids=["rotation-only", "tree-only", "both"])
@pytest.mark.parametrize("shape", STRUCT_SHAPES, ids=lambda s: s.name)
def test_vertical_packing_equals_its_stages(engine, shape, n_polys, n_ggsw):
    M, P = engine.lwe_wopbs, engine.ntt64_pbs
    batch, n_out = 3, 2
    r = n_polys.bit_length() - 1
    luts = lut_polys(shape, n_out, n_polys, 0x8000 + n_ggsw)
    ggsw = random_fourier_ggsws(engine, shape, batch, n_ggsw, 0x8010 + n_ggsw)
    out = zeros((batch, n_out, shape.k * shape.N + 1), -1)
    M.vertical_packing(luts, out, ggsw, *shape.cbs)
    acc = zeros((batch, n_out, shape.k + 1, shape.N), -1)
    M.cmux_tree_memory_optimized(acc, luts, ggsw[:, :r].contiguous(), *shape.cbs)
    M.blind_rotate_assign(acc, ggsw[:, r:].contiguous(), *shape.cbs)
    want = zeros((batch * n_out, shape.k * shape.N + 1), -1)
    P.extract_lwe_sample_from_glwe_ciphertext(acc.reshape(batch * n_out, shape.k + 1, shape.N), want)
    assert same(out.reshape(want.shape), want)


def test_vertical_packing_rejects_what_the_reference_panics_on(engine):
    M = engine.lwe_wopbs
    shape = W.SHAPE_A
    out = zeros((1, 1, shape.k * shape.N + 1))
    for n_polys, n_ggsw in [(3, 2), (4, 1)]:  # not a power of two; no tree but more than one polynomial
        with pytest.raises(engine.MiError) as e:
            M.vertical_packing(lut_polys(shape, 1, n_polys, 1), out, random_fourier_ggsws(engine, shape, 1, n_ggsw, 2),
                               *shape.cbs)
        assert e.value.status == 1
    with pytest.raises(ValueError):
        M.cmux_tree_memory_optimized(zeros((1, 1, shape.k + 1, shape.N)), lut_polys(shape, 1, 3, 1),
                                     random_fourier_ggsws(engine, shape, 1, 2, 2), *shape.cbs)


@pytest.mark.parametrize("shape", STRUCT_SHAPES, ids=lambda s: s.name)
def test_circuit_bootstrap_equals_its_stages(engine, shape):
    M = engine.lwe_wopbs
    dk = device_keys(engine, shape, shape is W.SHAPE_A)
    batch, delta_log = 5, 60
    lwe = dev(H.uniform_u64(H.rng(0x8100), (batch, shape.n + 1)))
    level, k, n = shape.cbs[1], shape.k, shape.N
    std, four = zeros((batch, level, k + 1, k + 1, n), -1), fzeros((batch, level, k + 1, k + 1, n // 2, 2))
    M.circuit_bootstrap_boolean(dk["bsk"], lwe, delta_log, dk["pfpksk"], *shape.cbs, std, four, dk["fft"])
    want_std, want_four = cbs_by_stages(engine, shape, dk, lwe, delta_log)
    assert same(std, want_std) and same(four, want_four)
    only_f = fzeros(four.shape)  # either output alone
    M.circuit_bootstrap_boolean(dk["bsk"], lwe, delta_log, dk["pfpksk"], *shape.cbs, None, only_f, dk["fft"])
    only_s = zeros(std.shape, -1)
    M.circuit_bootstrap_boolean(dk["bsk"], lwe, delta_log, dk["pfpksk"], *shape.cbs, only_s, None)
    assert same(only_f, four) and same(only_s, std)
    one = zeros((1,) + tuple(std.shape[1:]), -1)  # one item alone equals the same item inside the batch of 5
    M.circuit_bootstrap_boolean(dk["bsk"], lwe[3:4].contiguous(), delta_log, dk["pfpksk"], *shape.cbs, one, None)
    assert same(one[0], std[3])


@pytest.mark.parametrize("shape", STRUCT_SHAPES, ids=lambda s: s.name)
def test_extract_bits_equals_its_stages(engine, shape):
    KS, M = engine.lwe_keyswitch, engine.lwe_wopbs
    dk = device_keys(engine, shape, shape is W.SHAPE_A)
    batch, n_bits, delta_log = 5, 4, 56
    big1, small1 = shape.k * shape.N + 1, shape.n + 1
    lwe = dev(H.uniform_u64(H.rng(0x8200), (batch, big1)))
    out = zeros((batch, n_bits, small1), -1)
    M.extract_bits_from_lwe_ciphertext_mem_optimized(lwe, out, dk["bsk"], dk["ksk"], delta_log, n_bits)
    want, cur = extract_bits_by_stages(engine, shape, dk, lwe, delta_log, n_bits)
    assert same(out, want)
    last = zeros((batch, small1), -1)  # the last output: the keyswitch of the shifted running input
    KS.keyswitch_lwe_ciphertext(dk["ksk"], (cur << (64 - delta_log - n_bits)).contiguous(), last)
    assert same(out[:, 0], last)
    one = zeros((1, n_bits, small1), -1)  # one item alone equals the same item inside the batch of 5
    M.extract_bits_from_lwe_ciphertext_mem_optimized(lwe[2:3].contiguous(), one, dk["bsk"], dk["ksk"], delta_log, n_bits)
    assert same(one[0], out[2])


@pytest.mark.parametrize("shape", STRUCT_SHAPES, ids=lambda s: s.name)
def test_cbs_vertical_packing_equals_its_stages(engine, shape):
    M = engine.lwe_wopbs
    dk = device_keys(engine, shape, shape is W.SHAPE_A)
    batch, n_bits, n_out, n_polys = 5, 4, 2, 4
    level, k, n = shape.cbs[1], shape.k, shape.N
    bits = dev(H.uniform_u64(H.rng(0x8300), (batch, n_bits, shape.n + 1)))
    luts = lut_polys(shape, n_out, n_polys, 0x8301)
    out = zeros((batch, n_out, k * n + 1), -1)
    M.circuit_bootstrap_boolean_vertical_packing_lwe_ciphertext_list_mem_optimized(bits, out, luts, dk["bsk"],
                                                                                   dk["pfpksk"], *shape.cbs, dk["fft"])
    four = fzeros((batch, n_bits, level, k + 1, k + 1, n // 2, 2))
    M.circuit_bootstrap_boolean(dk["bsk"], bits.reshape(batch * n_bits, -1), 63, dk["pfpksk"], *shape.cbs, None,
                                four.reshape((batch * n_bits,) + tuple(four.shape[2:])), dk["fft"])
    want = zeros(tuple(out.shape), -1)
    M.vertical_packing(luts, want, four, *shape.cbs, dk["fft"])
    assert same(out, want)
    one = zeros((1, n_out, k * n + 1), -1)  # one item alone equals the same item inside the batch of 5
    M.circuit_bootstrap_boolean_vertical_packing_lwe_ciphertext_list_mem_optimized(
        bits[1:2].contiguous(), one, luts, dk["bsk"], dk["pfpksk"], *shape.cbs, dk["fft"])
    assert same(one[0], out[1])


# ---- 4. decryption --------------------------------------------------------------------------------------------------
DECRYPT_SHAPES = [W.SHAPE_A, W.SHAPE_N512]


@pytest.mark.parametrize("shape", DECRYPT_SHAPES, ids=lambda s: s.name)
def test_extracted_bits_decrypt_to_the_message_bits(engine, shape):
    """tests.rs:94-252: each output decrypts to the message's bit in the top bit."""
    M = engine.lwe_wopbs
    dk, ks = device_keys(engine, shape, True), W.keys(shape)
    msgs = W.messages(8)
    out = zeros((len(msgs), W.N_INPUT_BITS, shape.n + 1), -1)
    M.extract_bits_from_lwe_ciphertext_mem_optimized(dev(W.encrypt_messages(shape, msgs)), out, dk["bsk"], dk["ksk"],
                                                     64 - W.N_INPUT_BITS, W.N_INPUT_BITS)
    with np.errstate(over="ignore"):
        got = (H.lwe_decrypt_batch(host(out), ks["small_sk"]) + np.uint64(1 << 62)) >> np.uint64(63)
    for b, m in enumerate(msgs):
        assert [int(v) for v in got[b]] == [(m >> (W.N_INPUT_BITS - 1 - j)) & 1 for j in range(W.N_INPUT_BITS)], (b, m)


@pytest.mark.parametrize("shape", DECRYPT_SHAPES, ids=lambda s: s.name)
def test_circuit_bootstrap_decrypts_to_the_ggsw_of_the_bit(engine, shape):
    """tests.rs:254-446: GLWE (i, j) of the output decodes, at base_log * (level_cbs - i) bits, to bit * (-S_j) for
    j < k and to bit at X^0 for the last row."""
    M = engine.lwe_wopbs
    dk, ks = device_keys(engine, shape, True), W.keys(shape)
    base_log, level = shape.cbs
    k, n, delta_log = shape.k, shape.N, 60
    bits = [0, 1, 1, 0, 1]
    lwe = H.lwe_encrypt_batch(H.rng(0x8400), [b << delta_log for b in bits], ks["small_sk"], shape.noise_log2)
    std = zeros((len(bits), level, k + 1, k + 1, n), -1)
    M.circuit_bootstrap_boolean(dk["bsk"], dev(lwe), delta_log, dk["pfpksk"], base_log, level, std, None)
    got = host(std)
    for b, bit in enumerate(bits):
        for i in range(level):
            rep = base_log * (level - i)
            for j in range(k + 1):
                pt = H.glwe_decrypt(got[b, i, j], ks["glwe_sk"])
                with np.errstate(over="ignore"):
                    dec = (pt + np.uint64(1 << (63 - rep))) >> np.uint64(64 - rep)
                want = np.zeros(n, np.uint64)
                if j < k:
                    want[:] = [((-bit * int(s)) % 2**64) >> (64 - rep) for s in ks["glwe_sk"][j]]
                else:
                    want[0] = bit
                assert np.array_equal(dec, want), (b, i, j)


@pytest.mark.parametrize("shape", DECRYPT_SHAPES, ids=lambda s: s.name)
def test_wop_add_one_end_to_end(engine, shape):
    """All 8 seeded messages of the CPU test: extract bits, then circuit bootstrap + vertical packing with two outputs,
    (m + 1) mod 2^10 and (m + 3) mod 2^10."""
    M = engine.lwe_wopbs
    dk, ks = device_keys(engine, shape, True), W.keys(shape)
    msgs, nb = W.messages(8), W.N_INPUT_BITS
    bits = zeros((len(msgs), nb, shape.n + 1), -1)
    M.extract_bits_from_lwe_ciphertext_mem_optimized(dev(W.encrypt_messages(shape, msgs)), bits, dk["bsk"], dk["ksk"],
                                                     64 - nb, nb)
    luts = dev(np.stack([W.add_one_lut(shape.N), W.add_one_lut(shape.N, add=3)]))
    out = zeros((len(msgs), 2, shape.k * shape.N + 1), -1)
    M.circuit_bootstrap_boolean_vertical_packing_lwe_ciphertext_list_mem_optimized(bits, out, luts, dk["bsk"],
                                                                                   dk["pfpksk"], *shape.cbs, dk["fft"])
    got = host(out)
    assert W.decode_output(got[:, 0], ks["big_sk"]) == [(m + 1) % 1024 for m in msgs]
    assert W.decode_output(got[:, 1], ks["big_sk"]) == [(m + 3) % 1024 for m in msgs]
