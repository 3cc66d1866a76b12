"""The WoP-PBS drivers at their chunk, index and shift corners (`-m gpu`; restatements in tests/wopbs_gpu_helpers.py).

A. the CMUX tree across the chunks of its scratch cap: a boundary inside an item on both engines, one tree above the
   cap, the straddling item alone, and the pool's size as the witness that the call did chunk;
B. ggsw_first != 0 and ggsw_stride > count on the tree and the rotation, through the C entry;
C. the ends of the shift and exponent ranges of the word-wise passes, against the staged restatements; the argument
   rules and the no-ops next to them;
D. the empty ends of vertical packing against plain numpy;
E. every leaf of a tree of depth 3 and 4 selected by encrypted bits, decrypted.
"""
import ctypes

import numpy as np
import pytest

import tfhe_helpers as H
import wopbs_helpers as W
from wopbs_gpu_helpers import (cbs_by_stages, dev, device_keys, device_uniform, extract_bits_by_stages, fzeros, host,
                               lut_polys, random_fourier_ggsws, same, tree_by_layers, zeros)

pytestmark = pytest.mark.gpu

STRUCT_SHAPES = [W.SHAPE_A, W.SHAPE_N2048]
MIB = 1 << 20


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def current_stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def last_message(L):
    return L.mi_last_error_message().decode()


# ---- A. the tree across chunks --------------------------------------------------------------------------------------
# WOP_TREE_CAP_BYTES of csrc/c_api_wopbs.cpp.  It is a constant of that file and not of the ABI, so it is restated
# here: whoever changes it moves the shapes below so that each still chunks as its comment says (the test checks that
# arithmetic before it runs anything, and on the one-wave engine it checks the scratch pool after the call).
TREE_CAP = 256 * MIB
# (shape, r, batch, n_outputs); a tree is 2^r GLWEs of (k + 1) N words of 8 bytes
CHUNKED = [
    # 2^10 * 2 * 2048 * 8 B = 32 MiB per tree, 256 / 32 = 8 trees per chunk; 4 * 3 = 12 trees = 8 + 4; the boundary
    # t0 = 8 is item 2, output 2: inside item 2, and the last chunk is shorter
    pytest.param(W.SHAPE_N2048, 10, 4, 3, 8, id="one-wave-8+4"),
    # 2^10 * 2 * 256 * 8 B = 4 MiB per tree, 256 / 4 = 64 trees per chunk; 23 * 3 = 69 trees = 64 + 5; t0 = 64 is
    # item 21, output 1
    pytest.param(W.SHAPE_A, 10, 23, 3, 64, id="generic-64+5"),
    # 2^14 * 2 * 2048 * 8 B = 512 MiB per tree, above the cap: the chunk is clamped to one tree, two chunks of one.
    # About 3 GiB of device memory: 1 GiB of reference nodes, their two halves, 512 MiB of the library's scratch
    pytest.param(W.SHAPE_N2048, 14, 2, 1, 1, id="one-wave-tree-above-cap"),
]


@pytest.mark.parametrize("shape,r,batch,n_out,chunk", CHUNKED)
def test_tree_across_chunks(engine, shape, r, batch, n_out, chunk):
    import torch
    M, P = engine.lwe_wopbs, engine.ntt64_pbs
    k, n = shape.k, shape.N
    tree_bytes, total = ((k + 1) * n * 8) << r, batch * n_out
    assert max(1, TREE_CAP // tree_bytes) == chunk and total > chunk  # more than one chunk, as the table says
    luts = device_uniform((n_out, 1 << r, n), 0x9A00 + r + n)
    ggsw = random_fourier_ggsws(engine, shape, batch, r, 0x9A10 + r + n, on_device=True)
    out = zeros((batch, n_out, k + 1, n), -1)  # every word must be written
    P.scratch_trim(0)
    M.cmux_tree_memory_optimized(out, luts, ggsw, *shape.cbs)
    held = P.scratch_bytes(0)
    assert same(out, tree_by_layers(engine, shape, luts, ggsw, batch))
    if n == 2048:
        # The one-wave indexed CMUX takes no scratch of its own (csrc/fft64.hip allocates none), so after a trim the pool
        # holds what the tree took: chunk trees of nodes and the index array (chunk * 2^(r-1) u32, rounded up to the
        # pool's 1 MiB grain).  All the trees at once would be total * tree_bytes: had the call not chunked, the pool
        # would hold at least that.
        assert chunk * tree_bytes <= held < total * tree_bytes, (held // MIB, total * tree_bytes // MIB)
    if chunk % n_out:  # the boundary falls inside this item: alone, it gives what it gave in the chunked call
        item = chunk // n_out
        one = zeros((1, n_out, k + 1, n), -1)
        M.cmux_tree_memory_optimized(one, luts, ggsw[item:item + 1].contiguous(), *shape.cbs)
        assert same(one[0], out[item])
    del luts, ggsw, out
    torch.cuda.empty_cache()
    P.scratch_trim(0)


# ---- B. ggsw_first and ggsw_stride ----------------------------------------------------------------------------------
STRIDE = 5
RANGE = "the GGSW range exceeds the GGSWs of an item"


@pytest.mark.parametrize("shape", STRUCT_SHAPES, ids=lambda s: s.name)
def test_tree_reads_its_range_of_a_longer_list(engine, shape):
    """GGSWs [2, 5) of 5 per item: the call on the contiguous slice, bit for bit."""
    from tfhe_ntt_amd import _lib
    L, M = _lib.lib(), engine.lwe_wopbs
    batch, n_out, first, r = 3, 2, 2, 3
    fft = engine.fft64.Fft(shape.N)
    luts = lut_polys(shape, n_out, 1 << r, 0x9B00)
    ggsw = random_fourier_ggsws(engine, shape, batch, STRIDE, 0x9B10)
    out = zeros((batch, n_out, shape.k + 1, shape.N), -1)
    assert L.mi_fft64_cmux_tree_batch(fft.handle, ptr(out), ptr(luts), 1 << r, n_out, ptr(ggsw), STRIDE, first, r,
                                      shape.k, *shape.cbs, batch, current_stream()) == _lib.MI_OK, last_message(L)
    want = zeros(tuple(out.shape), -1)
    M.cmux_tree_memory_optimized(want, luts, ggsw[:, first:first + r].contiguous(), *shape.cbs)
    assert same(out, want)


@pytest.mark.parametrize("shape", STRUCT_SHAPES, ids=lambda s: s.name)
def test_rotation_reads_its_range_of_a_longer_list(engine, shape):
    """GGSWs [1, 4) of 5 per item: the call on the contiguous slice, bit for bit."""
    from tfhe_ntt_amd import _lib
    L, M = _lib.lib(), engine.lwe_wopbs
    batch, n_out, first, n_rot = 3, 2, 1, 3
    fft = engine.fft64.Fft(shape.N)
    glwe = dev(H.uniform_u64(H.rng(0x9B20), (batch, n_out, shape.k + 1, shape.N)))
    ggsw = random_fourier_ggsws(engine, shape, batch, STRIDE, 0x9B30)
    want = glwe.clone()
    M.blind_rotate_assign(want, ggsw[:, first:first + n_rot].contiguous(), *shape.cbs)
    assert L.mi_fft64_wop_blind_rotate_batch(fft.handle, ptr(glwe), n_out, ptr(ggsw), STRIDE, first, n_rot, shape.k,
                                             *shape.cbs, batch, current_stream()) == _lib.MI_OK, last_message(L)
    assert same(glwe, want)


def test_ggsw_range_rejections(engine):
    """first + count > stride, before any buffer is read (the buffers are NULL)."""
    from tfhe_ntt_amd import _lib
    L = _lib.lib()
    shape = W.SHAPE_A
    fft = engine.fft64.Fft(shape.N)
    for first, count in [(3, 3), (5, 1), (6, 0), (0, 6)]:
        assert L.mi_fft64_cmux_tree_batch(fft.handle, None, None, 1 << count, 2, None, STRIDE, first, count, shape.k,
                                          *shape.cbs, 1, None) == _lib.MI_ERR_INVALID_ARG, (first, count)
        assert last_message(L) == RANGE
        assert L.mi_fft64_wop_blind_rotate_batch(fft.handle, None, 2, None, STRIDE, first, count, shape.k, *shape.cbs, 1,
                                                 None) == _lib.MI_ERR_INVALID_ARG, (first, count)
        assert last_message(L) == RANGE
    # the whole list and the empty range at its end are inside: the next rule answers (NULL buffers)
    for first, count in [(0, 5), (5, 0)]:
        assert L.mi_fft64_wop_blind_rotate_batch(fft.handle, None, 2, None, STRIDE, first, count, shape.k, *shape.cbs,
                                                 1, None) == (_lib.MI_ERR_INVALID_ARG if count else _lib.MI_OK)
        assert not count or last_message(L) == "buffer is NULL"


# ---- C. shift and exponent corners ----------------------------------------------------------------------------------
# (delta_log, n_bits, batch).  The shift of bit b is 63 - delta_log - b and the accumulator's exponent delta_log - 1 + b:
# (0, 1) shifts by 63; (63, 1) by 0; (1, 63) by 62 .. 0 with exponents 0 .. 61 (62 bootstraps per item); (32, 32) starts
# in the middle and ends at shift 0, exponent 61
EXTRACT_CORNERS = [(0, 1, 5), (63, 1, 5), (1, 63, 2), (32, 32, 3)]


@pytest.mark.parametrize("delta_log,n_bits,batch", EXTRACT_CORNERS)
@pytest.mark.parametrize("shape", STRUCT_SHAPES, ids=lambda s: s.name)
def test_extract_bits_corners_equal_the_stages(engine, shape, delta_log, n_bits, batch):
    M = engine.lwe_wopbs
    dk = device_keys(engine, shape, shape is W.SHAPE_A)
    lwe = dev(H.uniform_u64(H.rng(0x9C00 + delta_log), (batch, shape.k * shape.N + 1)))
    out = zeros((batch, n_bits, shape.n + 1), -1)
    M.extract_bits_from_lwe_ciphertext_mem_optimized(lwe, out, dk["bsk"], dk["ksk"], delta_log, n_bits)
    want, _ = extract_bits_by_stages(engine, shape, dk, lwe, delta_log, n_bits)
    assert same(out, want)


# (delta_log, (base_log_cbs, level_cbs) or the shape's).  The input shift is 63 - delta_log: 63 and 0.  The exponents of
# the accumulators are 63 - base_log_cbs (level_cbs - i): (63, 1) gives 0; (9, 7) gives 0, 9, .., 54 over the most
# levels a product of 63 leaves room for with base_log > 1; (1, 1) gives 62
CBS_CORNERS = [(0, None), (63, None), (60, (63, 1)), (60, (9, 7)), (60, (1, 1))]


@pytest.mark.parametrize("delta_log,cbs", CBS_CORNERS)
@pytest.mark.parametrize("shape", STRUCT_SHAPES, ids=lambda s: s.name)
def test_circuit_bootstrap_corners_equal_the_stages(engine, shape, delta_log, cbs):
    M = engine.lwe_wopbs
    dk = device_keys(engine, shape, shape is W.SHAPE_A)
    cbs = cbs or shape.cbs
    batch, level, k, n = 3, cbs[1], shape.k, shape.N
    lwe = dev(H.uniform_u64(H.rng(0x9D00 + delta_log + cbs[0]), (batch, shape.n + 1)))
    std, four = zeros((batch, level, k + 1, k + 1, n), -1), fzeros((batch, level, k + 1, k + 1, n // 2, 2))
    M.circuit_bootstrap_boolean(dk["bsk"], lwe, delta_log, dk["pfpksk"], *cbs, std, four, dk["fft"])
    want_std, want_four = cbs_by_stages(engine, shape, dk, lwe, delta_log, cbs)
    assert same(std, want_std) and same(four, want_four)
    if cbs == (63, 1):
        # What this corner can and cannot show.  The accumulator is the constant -2^0.  Every CMUX of the bootstrap
        # multiplies the GGSW by X^a acc - acc, whose coefficients are 0 or +-2: below what the (9, 4) decomposition
        # keeps (multiples of 2^28), so the digits are zero and the accumulator stays trivial.  The bootstrapped LWE
        # has a zero mask and the body -+1 + 1, and the pfpks, which keeps the top 30 bits, rounds that to zero: the
        # GGSW is exactly zero, here and for any exponent near 0.  So this case holds the shift to its range (a stray
        # large constant would show), and (9, 7), whose exp0 is 0 as well, shows exp0 itself through its levels from
        # exponent 27 on.
        assert not bool(std.any()) and not bool(four.any())


EXTRACT_RULE = "delta_log + n_bits must be <= 64 (delta_log >= 1 for more than one bit)"
CBS_RULE, DELTA_RULE = "circuit bootstrap base_log * level must be in [1, 63]", "delta_log must be in [0, 63]"


def test_corner_rejections_and_no_ops(engine):
    """One step past every corner above is MI_ERR_INVALID_ARG with the rule's message, before any buffer is read (the
    buffers are NULL); n_bits = 0 and batch = 0 are MI_OK and write nothing."""
    import torch
    from tfhe_ntt_amd import _lib
    L, INVALID, OK = _lib.lib(), _lib.MI_ERR_INVALID_ARG, _lib.MI_OK
    shape = W.SHAPE_A
    dk = device_keys(engine, shape, True)
    bsk, ksk, pf, plan = dk["bsk"]._h, dk["ksk"]._h, dk["pfpksk"]._h, dk["fft"].handle
    for delta_log, n_bits in [(60, 5), (64, 1), (1, 64), (0, 65), (0, 2), (0, 64), (-1, 1)]:
        assert L.mi_fft64_extract_bits_batch(bsk, ksk, None, None, delta_log, n_bits, 1, None) == INVALID, (delta_log, n_bits)
        assert last_message(L) == EXTRACT_RULE
    for delta_log, base_log, level, message in [(60, 8, 8, CBS_RULE), (60, 64, 1, CBS_RULE), (60, 6, 0, CBS_RULE),
                                                (60, 0, 4, CBS_RULE), (64, 6, 4, DELTA_RULE), (-1, 6, 4, DELTA_RULE)]:
        assert L.mi_fft64_circuit_bootstrap_boolean_batch(bsk, pf, plan, None, None, None, 1, delta_log, base_log, level,
                                                          None) == INVALID, (delta_log, base_log, level)
        assert last_message(L) == message
    # the no-ops, on buffers that a write would show in
    s = current_stream()
    lwe = dev(H.uniform_u64(H.rng(0x9E00), (3, shape.k * shape.N + 1)))
    out = zeros((3, 4, shape.n + 1), -1)
    assert L.mi_fft64_extract_bits_batch(bsk, ksk, ptr(out), ptr(lwe), 60, 0, 3, s) == OK
    assert L.mi_fft64_extract_bits_batch(bsk, ksk, ptr(out), ptr(lwe), 64, 0, 3, s) == OK  # 64 + 0 <= 64
    assert L.mi_fft64_extract_bits_batch(bsk, ksk, ptr(out), ptr(lwe), 60, 4, 0, s) == OK
    level = shape.cbs[1]
    std = zeros((3, level, shape.k + 1, shape.k + 1, shape.N), -1)
    four = torch.full((3, level, shape.k + 1, shape.k + 1, shape.N // 2, 2), -1.0, dtype=torch.float64, device="cuda")
    small = dev(H.uniform_u64(H.rng(0x9E01), (3, shape.n + 1)))
    assert L.mi_fft64_circuit_bootstrap_boolean_batch(bsk, pf, plan, ptr(std), ptr(four), ptr(small), 0, 60,
                                                      *shape.cbs, s) == OK
    torch.cuda.synchronize()
    assert bool((out == -1).all()) and bool((std == -1).all()) and bool((four == -1.0).all())


# ---- D. the empty ends, against plain numpy -------------------------------------------------------------------------
@pytest.mark.parametrize("shape", STRUCT_SHAPES, ids=lambda s: s.name)
def test_empty_ends_extract_the_trivial_glwe(engine, shape):
    """No GGSW and one polynomial per output: a tree of depth 0, no rotation, sample extraction; and the composite with
    no input bit, which runs no circuit bootstrap and passes a NULL list.  Output (b, o) is the LWE with a zero mask and
    body lut[o, 0, 0]: no f64 arithmetic is in it, so the reference is numpy alone and the comparison exact."""
    M = engine.lwe_wopbs
    dk = device_keys(engine, shape, shape is W.SHAPE_A)
    batch, n_out, k, n = 3, 2, shape.k, shape.N
    lut = H.uniform_u64(H.rng(0x9F00 + n), (n_out, 1, n))
    glwe = np.zeros((n_out, k + 1, n), np.uint64)
    glwe[:, k] = lut[:, 0]
    want = np.broadcast_to(W.sample_extract0(glwe), (batch, n_out, k * n + 1))
    assert not want[..., :-1].any() and np.array_equal(want[1, :, -1], lut[:, 0, 0]) and lut[:, 0, 0].all()
    out = zeros((batch, n_out, k * n + 1), -1)
    M.vertical_packing(dev(lut), out, random_fourier_ggsws(engine, shape, batch, 0, 1), *shape.cbs)
    assert np.array_equal(host(out), want)
    out = zeros((batch, n_out, k * n + 1), -1)
    M.circuit_bootstrap_boolean_vertical_packing_lwe_ciphertext_list_mem_optimized(
        zeros((batch, 0, shape.n + 1)), out, dev(lut), dk["bsk"], dk["pfpksk"], *shape.cbs, dk["fft"])
    assert np.array_equal(host(out), want)


# ---- E. every leaf through real GGSWs -------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,r", [(W.SHAPE_A, 4), (W.SHAPE_N512, 3)], ids=["A-r4", "N512-r3"])
def test_every_leaf_is_selected_by_its_encrypted_bits(engine, shape, r):
    """For every m < 2^r: m's bits encrypted at delta_log 63 under the seeded keys, circuit-bootstrapped to a Fourier
    GGSW list, the tree over W.leaf_lut; all N coefficients of item m decode to leaf m at 4 bits (margin 2^59;
    tests/test_wopbs_ref.py holds the numpy restatement to the same, worst error 2^42.7 at A and 2^43.1 at N512).  The
    bit-reversed leaf order equals the natural one at r = 1 and swaps two leaves at r = 2; from r = 3 on a tree that
    did not reverse would select other leaves."""
    M = engine.lwe_wopbs
    dk, ks = device_keys(engine, shape, True), W.keys(shape)
    level, k, n = shape.cbs[1], shape.k, shape.N
    four = fzeros((1 << r, r, level, k + 1, k + 1, n // 2, 2))
    M.circuit_bootstrap_boolean(dk["bsk"], dev(W.leaf_selector_lwes(shape, r)), 63, dk["pfpksk"], *shape.cbs, None,
                                four.reshape((r << r,) + tuple(four.shape[2:])), dk["fft"])
    lut = W.leaf_lut(r, n)
    out = zeros((1 << r, 1, k + 1, n), -1)
    M.cmux_tree_memory_optimized(out, dev(lut[None]), four, *shape.cbs, dk["fft"])
    got, err = W.decode_leaves(host(out)[:, 0], ks["glwe_sk"])
    print(f"\nleaf selection {shape.name} r={r}: gpu worst error 2^{np.log2(max(err, 1)):.1f}", end="")
    assert np.array_equal(got, lut >> np.uint64(60))
