"""GPU tests of the shortint atomic pattern and the radix drivers, bit for bit (`-m gpu`).

* mi_shortint_apply_lut_batch on the NTT engine against oracle.lwe_keyswitch followed by the oracle's PBS: each
  modulus switch, the drift key, shared inputs through in_index, per-item and out-of-range LUT indices, the in-place
  form.  N = 2048 runs the hand-scheduled engine, N = 1024 the fused generic one.
* every composite against its written sequence of public calls (tests/shortint_gpu_helpers.py seq_*), on all three
  engines: the composites are deterministic functions of their input words, so uniform words serve.

Key words are uniform (n = 16): nothing here decrypts; tests/test_integer_gpu.py does, under real keys."""
import numpy as np
import pytest

import ms_noise_helpers as MN
import shortint_gpu_helpers as G
import tfhe_helpers as H

pytestmark = pytest.mark.gpu

SENTINEL = G.SENTINEL
oracle_apply = G.oracle_apply


@pytest.mark.parametrize("which", ["u2048", "u1024"])
@pytest.mark.parametrize("mode", ["standard", "centered", "drift"])
def test_apply_lut_matches_oracle(engine, oracle, which, mode):
    import torch
    ks = G.key_set(engine, oracle, which)
    drift, ms_mode = mode == "drift", int(mode == "centered")
    sk = ks.server("ntt", False, ms_mode)
    g = H.rng(0x5100 + len(which + mode))
    n_in, n_lut = 5, 3
    lwe = H.uniform_u64(g, (n_in, ks.size))
    luts = H.uniform_u64(g, (n_lut, 2, ks.n))
    params = None
    if drift:  # a bound that three of the five inputs meet: the drift step adds candidates to some and not to others
        log2n = (2 * ks.n).bit_length() - 1
        small = oracle.lwe_keyswitch(ks.ksk_words, lwe, ks.small, G.KS_BL, G.KS_L)
        base = MN.measures_np(small, np.zeros((1, ks.small + 1), np.uint64), MN.Params(0.0, 1.0, 0.0, log2n))[:, 0]
        params = (float(np.sort(base)[2]), 1.0, 0.0)
        cand, _ = MN.choose_np(small, ks.zeros_words, MN.Params(*params, log2n))
        assert (cand >= 0).any() and (cand < 0).sum() >= 3, cand
        msk = engine.modulus_switch_noise_reduction.ModulusSwitchNoiseReductionKey(G.dev(ks.zeros_words), *params)
        sk = engine.shortint.ShortintServerKey(ks.ksk, ks.pbs["ntt"], G.MSG, G.CARRY, msk)
    # one input feeding several tables, an input no item uses, out-of-range inputs and tables
    in_index = [0, 0, 3, 1, G.NONE, 4, n_in, 2, 2]
    lut_index = [0, 2, 1, n_lut, 0, 2, 1, G.NONE, 1]
    out = torch.full((len(in_index), ks.size), int(SENTINEL), dtype=torch.int64, device="cuda")
    sk.apply_lookup_table_batch(out, G.dev(lwe), G.dev(luts), G.i32(lut_index), G.i32(in_index))
    want, live = oracle_apply(oracle, ks, lwe, luts, lut_index, in_index, ms_mode, drift, params)
    assert live.tolist() == [True, True, True, False, False, True, False, False, True]
    assert np.array_equal(G.host(out), want)
    # no index arrays: item j is input j through table j; then a table per item, in place
    out = torch.full((n_lut, ks.size), int(SENTINEL), dtype=torch.int64, device="cuda")
    sk.apply_lookup_table_batch(out, G.dev(lwe[:n_lut]), G.dev(luts))
    want, _ = oracle_apply(oracle, ks, lwe[:n_lut], luts, list(range(n_lut)), None, ms_mode, drift, params)
    assert np.array_equal(G.host(out), want)
    ct = G.dev(lwe)
    per_item = [2, 0, 1, 1, 2]
    sk.apply_lookup_table_assign(ct, G.dev(luts), G.i32(per_item))
    want, _ = oracle_apply(oracle, ks, lwe, luts, per_item, None, ms_mode, drift, params)
    assert np.array_equal(G.host(ct), want)
    assert np.array_equal(G.host(sk.apply_lookup_table(G.dev(lwe), G.dev(luts[1]))),
                          oracle_apply(oracle, ks, lwe, luts, [1] * n_in, None, ms_mode, drift, params)[0])


def servers(engine, oracle):
    """(id, server key) over the three engines, with and without the drift key, and the centered switch."""
    ks = G.key_set(engine, oracle, "u2048")
    yield "ntt", ks, ks.server("ntt")
    yield "ntt-drift", ks, ks.server("ntt", drift=True)
    yield "ntt-centered", ks, ks.server("ntt", ms_mode=1)
    yield "fft", ks, ks.server("fft")
    yield "fft-drift", ks, ks.server("fft", drift=True)
    yield "multi-bit", ks, ks.server("multi-bit")
    small = G.key_set(engine, oracle, "u1024")
    yield "ntt-1024", small, small.server("ntt")
    yield "fft-1024", small, small.server("fft", drift=True)


SERVER_IDS = ["ntt", "ntt-drift", "ntt-centered", "fft", "fft-drift", "multi-bit", "ntt-1024", "fft-1024"]


def server(engine, oracle, name):
    return next((ks, sk) for n, ks, sk in servers(engine, oracle) if n == name)


@pytest.mark.parametrize("name", SERVER_IDS)
def test_apply_lut_equals_its_stages(engine, oracle, name):
    import torch
    ks, sk = server(engine, oracle, name)
    g = H.rng(0x5200 + SERVER_IDS.index(name))
    lwe, luts = G.dev(H.uniform_u64(g, (4, ks.size))), G.dev(H.uniform_u64(g, (3, 2, ks.n)))
    for in_index, lut_index in [([1, 1, 3, G.NONE, 0, 4, 2], [0, 1, 2, 0, 3, 1, 2]), (None, [2, 2, 0, 1]),
                                ([0, 1, 2], None)]:
        items = len(in_index or lut_index)
        got = torch.full((items, ks.size), int(SENTINEL), dtype=torch.int64, device="cuda")
        want = got.clone()
        ii = None if in_index is None else G.i32(in_index)
        li = None if lut_index is None else G.i32(lut_index)
        sk.apply_lookup_table_batch(got, lwe, luts, li, ii)
        G.seq_apply(engine, sk, want, lwe, luts, li, ii)
        assert torch.equal(got, want), (name, in_index, lut_index)


@pytest.mark.parametrize("name", SERVER_IDS)
def test_radix_composites_equal_their_sequences(engine, oracle, name):
    """Propagation at B = 1 (with and without the carry), 2, 3, 5 and 9 blocks (a last partial scan round), full
    propagation and addition: the C drivers against the same LC / APPLY calls issued from Python."""
    import torch
    ks, sk = server(engine, oracle, name)
    I = engine.integer.ServerKey(sk)
    g = H.rng(0x5300 + SERVER_IDS.index(name))
    shapes = [(3, 1), (2, 2), (2, 3), (3, 5), (2, 9)] if name in ("ntt", "fft", "multi-bit") else [(2, 1), (2, 3)]
    for n_int, blocks in shapes:
        words = H.uniform_u64(g, (2, n_int, blocks, ks.size))
        for with_carry in (True, False):
            got, want = G.dev(words[0]), G.dev(words[0])
            c_got = torch.full((n_int, ks.size), int(SENTINEL), dtype=torch.int64, device="cuda")
            c_want = c_got.clone()
            I._propagate_single_carry(got, c_got if with_carry else None)
            G.seq_propagate(engine, sk, want, c_want if with_carry else None)
            assert torch.equal(got, want) and torch.equal(c_got, c_want), (name, n_int, blocks, with_carry)
            assert with_carry == bool((G.host(c_got) != SENTINEL).any())
        ct = engine.integer.RadixCiphertext(G.dev(words[0]), [15] * blocks)
        want = G.dev(words[0])
        I.full_propagate_parallelized(ct)
        G.seq_full_propagate(engine, sk, want)
        assert torch.equal(ct.blocks, want), (name, n_int, blocks, "full")
        a = engine.integer.RadixCiphertext(G.dev(words[0]), [3] * blocks)
        b = engine.integer.RadixCiphertext(G.dev(words[1]), [3] * blocks)
        got, carry = I.unsigned_overflowing_add_parallelized(a, b)
        want, c_want = G.zeros((n_int, blocks, ks.size)), G.zeros((n_int, ks.size))
        G.seq_add(engine, sk, want, a.blocks, b.blocks, c_want)
        assert torch.equal(got.blocks, want) and torch.equal(carry, c_want), (name, n_int, blocks, "add")
        assert torch.equal(I.add_parallelized(a, b).blocks, want)


def test_full_propagate_without_the_single_carry_form(engine, oracle):
    """m = c = 2 has no single-carry form: full propagation is the extract-and-add round n_blocks times, and the
    single-carry calls answer MI_ERR_UNSUPPORTED."""
    import torch
    ks = G.key_set(engine, oracle, "u2048")
    sk = ks.server("ntt", m=2, c=2)
    I = engine.integer.ServerKey(sk)
    g = H.rng(0x5400)
    words = H.uniform_u64(g, (2, 3, ks.size))
    ct = engine.integer.RadixCiphertext(G.dev(words), [3] * 3)
    want = G.dev(words)
    I.full_propagate_parallelized(ct)
    G.seq_full_propagate(engine, sk, want)
    assert torch.equal(ct.blocks, want)
    clean = engine.integer.RadixCiphertext(G.dev(words), [1] * 3)
    with pytest.raises(engine.MiError) as e:
        I.add_parallelized(clean, clean)
    assert e.value.status == 6
