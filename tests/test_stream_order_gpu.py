"""The stream contract of the asynchronous entry points, pinned on non-blocking streams (`-m gpu`).

include/tfhe_ntt_amd.h promises that every `_batch` call is asynchronous on `stream`, that plans and keys may be shared
by any number of streams and host threads, and (csrc/scratch.hpp) that a scratch block is reissued only behind the last
kernel that used it, on any stream, with no call blocking the host.  The rest of the GPU suite runs on the legacy null
stream, where a kernel on the wrong stream, a scratch block released on the wrong stream or an unjoined side lane
still gives the right values.  Here every entry runs through the delayed-operand harness of tests/stream_order.py on a
`torch.cuda.Stream()` (hipStreamNonBlocking); the expected values are the oracle's (the f64-FFT entries: a quiescent
run of the same call, shown to repeat bit for bit; test_fft_accuracy_gpu.py and the decryption tests tie those values
to the reference).

Entry point -> test (H = through the harness, S = synchronises by design: operand half only, O = scratch hand-over,
T = host threads):

  mi_ntt64_{fwd,inv,normalize,mul_assign_normalize,mul_accumulate}_batch   test_plan_ops[solinas2048 (asm bodies),
                                                                           solinas4096 (split), solinas1024 (generic),
                                                                           prime1024]                              H
  mi_ntt32_{fwd,inv,normalize,mul_assign_normalize,mul_accumulate}_batch   test_plan_ops[prime32-*]                 H
  mi_fill_uniform                                                          test_fill_uniform                        H
  mi_ntt64_forward[_normalized|_from_power_of_two_modulus|_from_decomp]_batch,
  mi_ntt64_add_backward[_on_power_of_two_modulus]_batch                    test_view_ops[2048 (fused), 1024]        H
  mi_native_polymul_batch                                                  test_native_polymul H, test_hand_over[native] O
  mi_bsk_to_ntt64                                                          test_key_conversion[ntt-2048-w64 (fused
                                                                           twisted), ntt-1024]                      H
  mi_bsk_to_fourier64                                                      test_key_conversion[fourier-*]           H
  mi_ext_product_ntt64_batch, mi_cmux_ntt64_batch, their _indexed and
  _prepared forms                                                          test_ntt_ext_product (both variants, the
                                                                           twisted shape and N = 1024, k = 2, l = 2) H,
                                                                           test_hand_over[tw_ext] O
  mi_ntt64_ggsw_create                                                     test_synchronising_entries[ggsw]         S
  mi_pbs_ntt64_batch, _batch_lut_indexed, mi_blind_rotate_ntt64_batch      test_ntt_pbs (BNF / Solinas x STANDARD /
                                                                           PRE_SWITCHED: the sw and lifted scratch) H,
                                                                           test_hand_over[pbs_sw, pbs_lifted] O,
                                                                           test_host_threads T
  mi_sample_extract_batch                                                  test_sample_extract                      H
  mi_pbs_ntt64_key_create                                                  test_synchronising_entries[pbs_key]      S
  mi_fft64_{forward,backward}_torus_batch, mi_fft64_ext_product_batch,
  mi_fft64_cmux_batch, mi_fft64_pbs_batch, _batch_lut_indexed,
  mi_fft64_blind_rotate_batch                                              test_fft64[2048 (one wave), 256 (generic)] H,
                                                                           test_hand_over[fft_ext, fft_pbs] O,
                                                                           test_host_threads T
  mi_fft64_multi_bit_pbs_batch, mi_fft64_multi_bit_blind_rotate_batch      test_fft64_multi_bit (grouping factor 2) H
  mi_lwe_keyswitch_batch                                                   test_keyswitch H (one and two bytes per
                                                                           digit), test_hand_over[keyswitch] O,
                                                                           test_host_threads T
  mi_lwe_keyswitch32_batch                                                 test_keyswitch32                         H
  mi_lwe_modulus_switch32_batch, mi_lwe_modulus_switch_batch               test_modulus_switch (standard, centered) H
  mi_lwe_ksk_create, mi_lwe_ksk32_create                                   test_synchronising_entries[ksk, ksk32]   S
  mi_lwe_ms_noise_{measure,choose,improve,improve_and_switch}_batch        test_ms_noise_reduction                  H
  mi_ms_noise_key_create                                                   test_synchronising_entries[ms_noise_key] S
  mi_lwe_packing_keyswitch_batch                                           test_packing_keyswitch H (one and two bytes
                                                                           per digit), test_hand_over[pks] O
  mi_glwe_compress_batch, mi_glwe_extract_batch                            test_glwe_compression                    H
  mi_lwe_pksk_create                                                       test_synchronising_entries[pksk]         S
  mi_lwe_packing_keyswitch128_batch, mi_glwe_compress128_batch,
  mi_glwe_extract128_batch                                                 test_noise_squashing_compression H,
                                                                           test_hand_over[pks128] O
  mi_lwe_pksk128_create                                                    test_synchronising_entries[pksk128]      S
  mi_ext_product128_batch, mi_cmux128_batch, mi_blind_rotate128_batch,
  mi_pbs128_batch                                                          test_pbs128 H, test_hand_over[pbs128] O
  mi_pbs128_key_create                                                     test_synchronising_entries[pbs128_key]   S
  the forked lanes of run_blind_rotation (pbs_large.hip,
  fft64_generic.hip)                                                       test_forked_lanes H + O; test_hand_over[large]
                                                                           is pbs_large.hip's one-lane scratch

Left out, with the file that covers them on the null stream (their stream order is not pinned yet):
  the lanes of pbs128.hip: it asks run_blind_rotation for one lane (its
  default lane count is 1, pbs128.hip launch_blind_rotate128), so no batch
  forks there; its chunk loop                                              test_pbs128_gpu.py::test_two_chunks
  the piecewise path of mi_lwe_packing_keyswitch_batch (rows beyond the
  64 MiB scratch bound: a large call)                                      test_packing_ks_gpu.py
  mi_fft64_multi_bit_pbs_batch_lut_indexed                                 test_multi_bit_gpu.py
  mi_fft64_{to,from}_standard_order, mi_fft64_pbs_key_{load,write},
  mi_pbs_ntt64_key_load                                                    test_fft_gpu.py, test_ntt_bsk_format.py
  the `_host` entries                                                      test_host_path_gpu.py
  the mi_multi_gpu_* and *_multi_gpu[_ordered] entries                     test_multi_gpu_engine.py
"""
import threading

import numpy as np
import pytest

import ms_noise_helpers as MS
import native_oracle as NO
import packing128_helpers as Q
import packing_helpers as PH
import pbs128_helpers as R
import stream_order as SO
import tfhe_helpers as H

pytestmark = pytest.mark.gpu

P = 0xFFFFFFFF00000001
M32 = 2**32


def zeros(shape, dtype="int64"):
    import torch
    return torch.zeros(shape, dtype=getattr(torch, dtype), device="cuda")


def host(t):
    a = t.cpu().numpy()
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize]) if a.dtype.kind == "i" else a


def two(g, shape, q=0):
    """A true and a decoy value set: uniform below q (0: the whole u64 range)."""
    return H.uniform_q(g, shape, q), H.uniform_q(g, shape, q)


def two32(g, shape, hi=M32):
    return tuple(g.integers(0, hi, size=shape, dtype=np.uint64).astype(np.uint32) for _ in range(2))


# ---- the negative controls: the harness must see a call on another stream and a late overwrite ------------------------
def _control_case(engine, oracle, mode):
    """One entry per mode: an in-place transform, an out-of-place integer entry with scratch, an f64 entry."""
    g = H.rng(0xC0 + len(mode))
    if mode == "in_place":
        plan, ref = engine.Plan.cached(2048, P), oracle.Plan.try_new(2048, P)
        x = zeros((3, 2048))
        return SO.Case("control-fwd", lambda: plan.fwd(x), [(x, *two(g, (3, 2048), P))], [x], lambda v: [ref.fwd(v[0])])
    if mode == "out_of_place":
        return _keyswitch_case(engine, oracle, 40, 24, 4, 4, 5, g)
    return _fft_case(engine, "forward_torus", 2048, g)


@pytest.mark.parametrize("mode", ["in_place", "out_of_place", "f64"])
def test_operand_control_reports_a_call_on_another_stream(engine, oracle, mode):
    """The call issued on a second non-blocking stream is not ordered behind the operands that arrive on `s`: it reads
    the decoys, and the harness must report the mismatch (it reads valid data, so it is harmless)."""
    case = _control_case(engine, oracle, mode)
    bad = SO.check_case(engine, case, call_stream=SO.stream("other"))
    assert bad, "the harness did not notice a call that ran ahead of its operands"


@pytest.mark.parametrize("mode", ["out_of_place", "f64"])
def test_output_control_reports_a_late_overwrite(engine, oracle, mode):
    """The sentinel fill issued on another stream behind a longer delay of its own lands after the call wrote its
    results: the harness must report the overwrite (the mechanism that catches a stage writing early)."""
    case = _control_case(engine, oracle, mode)
    bad = SO.check_case(engine, case, fill_stream=SO.stream("other"))
    assert bad, "the harness did not notice the outputs being overwritten"


# ---- prime64 / prime32 plan ops -----------------------------------------------------------------------------------------
def _plans(oracle):
    generic = oracle.largest_prime_in_arithmetic_progression64(1 << 16, 1, 1 << 63, 2**64 - 1)
    return {"solinas2048": (64, 2048, P), "solinas4096": (64, 4096, P), "solinas1024": (64, 1024, P),
            "prime1024": (64, 1024, generic), "prime32": (32, 1024, 1062862849)}


@pytest.mark.parametrize("op", ["fwd", "inv", "normalize", "mul_assign_normalize", "mul_accumulate"])
@pytest.mark.parametrize("which", ["solinas2048", "solinas4096", "solinas1024", "prime1024", "prime32"])
def test_plan_ops(engine, oracle, which, op):
    bits, n, p = _plans(oracle)[which]
    plan = (engine.Plan if bits == 64 else engine.prime32.Plan).try_new(n, p)
    ref = oracle.Plan.try_new(n, p)
    g = H.rng(sum(map(ord, which + op)))
    cast = (lambda a: a) if bits == 64 else (lambda a: a.astype(np.uint32))
    arity = {"mul_assign_normalize": 2, "mul_accumulate": 3}.get(op, 1)
    bufs = [zeros((3, n), "int64" if bits == 64 else "int32") for _ in range(arity)]
    vals = [tuple(cast(v) for v in two(g, (3, n), p)) for _ in range(arity)]
    want = lambda v: [cast(getattr(ref, op)(*[a.astype(np.uint64) for a in v]))]
    case = SO.Case(f"{which}-{op}", lambda: getattr(plan, op)(*bufs), [(b, *v) for b, v in zip(bufs, vals)], bufs[:1], want)
    SO.check_case(engine, case)


def test_fill_uniform(engine, oracle):
    """No operand buffer (the seed is an argument): the output half only, a fill that ran early is overwritten."""
    out = zeros((3, 1024))
    case = SO.Case("fill_uniform", lambda: engine.fill_uniform(out, 0x5EED, P), [], [out],
                   lambda v: [oracle.fill_uniform(0x5EED, P, 3 * 1024).reshape(3, 1024)])
    SO.check_case(engine, case)


# ---- Ntt64View --------------------------------------------------------------------------------------------------------
VIEW_OPS = ["forward", "forward_normalized", "forward_from_power_of_two_modulus", "forward_from_decomp", "add_backward",
            "add_backward_on_power_of_two_modulus"]


@pytest.mark.parametrize("op", VIEW_OPS)
@pytest.mark.parametrize("n", [2048, 1024])
def test_view_ops(engine, oracle, n, op):
    view = engine.ntt64.Ntt64(P, n).as_view()
    ctx = oracle.NttContext(n, P)
    g = H.rng(n + VIEW_OPS.index(op))
    a, b = zeros((3, n)), zeros((3, n))
    if op.startswith("forward"):
        if op == "forward_from_decomp":
            src = tuple(g.integers(-(1 << 22), (1 << 22) + 1, size=(3, n), dtype=np.int64).astype(np.uint64)
                        for _ in range(2))
        else:
            src = two(g, (3, n), 0 if "power_of_two" in op else P)
        lead = (64,) if "power_of_two" in op else ()
        case = SO.Case(f"view{n}-{op}", lambda: getattr(view, op)(*lead, a, b), [(b, *src)], [a],
                       lambda v: [getattr(ctx, op)(*lead, v[0])])
    else:
        lead = (64,) if "power_of_two" in op else ()
        st, y = two(g, (3, n), 0 if lead else P), two(g, (3, n), P)
        case = SO.Case(f"view{n}-{op}", lambda: getattr(view, op)(*lead, a, b), [(a, *st), (b, *y)], [a, b],
                       lambda v: list(getattr(ctx, op)(*lead, v[0], v[1])))
    SO.check_case(engine, case)


# ---- the native product (a scratch user) --------------------------------------------------------------------------------
def _native_want(lhs, rhs):
    return np.array([NO.schoolbook([int(x) for x in l], [int(x) for x in r], 64) for l, r in zip(lhs, rhs)], np.uint64)


def test_native_polymul(engine):
    n = 32  # the smallest size native64::Plan32 accepts (its prime32 components need N >= 32)
    plan = engine.native64.Plan32.try_new(n)
    g = H.rng(0x4E41)
    prod, lhs, rhs = zeros((2, n)), zeros((2, n)), zeros((2, n))
    case = SO.Case("native64-plan32", lambda: plan.negacyclic_polymul(prod, lhs, rhs),
                   [(lhs, *two(g, (2, n))), (rhs, *two(g, (2, n)))], [prod], lambda v: [_native_want(v[0], v[1])])
    SO.check_case(engine, case)


# ---- key conversion -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n,normalize", [("ntt", 2048, False), ("ntt", 1024, True), ("fourier", 2048, False),
                                              ("fourier", 256, False)])
def test_key_conversion(engine, oracle, kind, n, normalize):
    """mi_bsk_to_ntt64: the fused twisted conversion (N = 2048, width 64) and the generic one; mi_bsk_to_fourier64."""
    import torch
    g = H.rng(n + normalize)
    shape = (3, 1, 2, 2, n)
    src = zeros(shape)
    if kind == "ntt":
        M = engine.ntt64_pbs
        plan, ctx = engine.Plan.cached(n, P), oracle.NttContext(n, P)
        dst = zeros(shape)
        case = SO.Case(f"bsk_to_ntt64-{n}", lambda: M.convert_standard_lwe_bootstrap_key_to_ntt64(plan, src, dst, normalize),
                       [(src, *two(g, shape))], [dst], lambda v: [ctx.bsk_to_ntt(v[0], 64, normalize)])
    else:
        F = engine.fft64
        fft = F.Fft(n)
        dst = torch.zeros(shape[:-1] + (n // 2, 2), dtype=torch.float64, device="cuda")
        case = SO.Case(f"bsk_to_fourier64-{n}", lambda: F.convert_standard_lwe_bootstrap_key_to_fourier(src, dst, fft),
                       [(src, *two(g, shape))], [dst])
    SO.check_case(engine, case)


# ---- NTT external product and CMUX ----------------------------------------------------------------------------------------
def _ext_want(oracle, n, k, base_log, level, bnf, cmux):
    ctx = oracle.NttContext(n, P)
    q = 0 if bnf else P

    def want(out, glwe, ggsws, index):
        res = np.stack([(ctx.cmux if cmux else ctx.ext_product)(out[b], *((glwe[b], ggsws[index[b]]) if cmux else
                                                                         (ggsws[index[b]], glwe[b])),
                                                                k, base_log, level, bnf) for b in range(out.shape[0])])
        return [res, H.sub_q(glwe, out, q)] if cmux else [res]
    return want


@pytest.mark.parametrize("form", ["plain", "indexed", "prepared", "prepared_indexed"])
@pytest.mark.parametrize("cmux", [False, True], ids=["ext", "cmux"])
@pytest.mark.parametrize("bnf", [True, False], ids=["bnf", "solinas"])
@pytest.mark.parametrize("n,k,base_log,level", [(2048, 1, 23, 1), (1024, 2, 12, 2)])
def test_ntt_ext_product(engine, oracle, n, k, base_log, level, bnf, cmux, form):
    """Both variants in every form at the twisted shape (whose raw-pointer calls permute the GGSW into per-call scratch)
    and at N = 1024, k = 2, level 2.  A prepared list is made beforehand (its creation synchronises: see
    test_synchronising_entries), so there the GLWEs and the indices are the delayed operands."""
    M = engine.ntt64_pbs
    plan = engine.Plan.cached(n, P)
    g = H.rng(n + 2 * bnf + cmux + 7 * len(form))
    q = 0 if bnf else P
    batch, n_ggsw = 3, 2
    variant = M.BNF if bnf else M.SOLINAS
    ref = _ext_want(oracle, n, k, base_log, level, bnf, cmux)
    out, glwe = zeros((batch, k + 1, n)), zeros((batch, k + 1, n))
    v_out, v_glwe = two(g, (batch, k + 1, n), q), two(g, (batch, k + 1, n), q)
    ggsw_shape = (n_ggsw, level, k + 1, k + 1, n)
    v_ggsw = two(g, ggsw_shape, P)
    v_idx = (np.array([1, 0, 1], np.uint32), np.array([0, 1, 0], np.uint32))
    idx = zeros((batch,), "int32")
    if cmux:  # cmux(plan, ct0, ct1, ggsw, ...): the same (plan, out, ggsw, glwe, ...) order for both below
        raw = M.cmux_ntt64_bnf_assign if bnf else M.cmux_ntt64_assign
        fn = lambda plan, ct0, ggsw, ct1, *a, **kw: raw(plan, ct0, ct1, ggsw, *a, **kw)
    else:
        fn = M.add_external_product_ntt64_bnf_assign if bnf else M.add_external_product_ntt64_assign
    outs = [out, glwe] if cmux else [out]
    name = f"ntt-{'cmux' if cmux else 'ext'}-{n}-{'bnf' if bnf else 'sol'}-{form}"
    if form == "plain":
        ggsw = zeros(ggsw_shape[1:])
        case = SO.Case(name, lambda: fn(plan, out, ggsw, glwe, base_log, level),
                       [(out, *v_out), (glwe, *v_glwe), (ggsw, v_ggsw[0][0], v_ggsw[1][0])], outs,
                       lambda v: ref(v[0], v[1], v[2][None], [0] * batch))
    elif form == "indexed":
        ggsw = zeros(ggsw_shape)
        case = SO.Case(name, lambda: fn(plan, out, ggsw, glwe, base_log, level, ggsw_index=idx),
                       [(out, *v_out), (glwe, *v_glwe), (ggsw, *v_ggsw), (idx, *v_idx)], outs,
                       lambda v: ref(v[0], v[1], v[2], v[3]))
    else:
        pg = M.NttGgswList(plan, SO.to_dev(v_ggsw[0]), base_log, level, variant)
        if form == "prepared":
            case = SO.Case(name, lambda: fn(plan, out, pg, glwe, base_log, level), [(out, *v_out), (glwe, *v_glwe)], outs,
                           lambda v: ref(v[0], v[1], v_ggsw[0], [0] * batch))
        else:
            case = SO.Case(name, lambda: fn(plan, out, pg, glwe, base_log, level, ggsw_index=idx),
                           [(out, *v_out), (glwe, *v_glwe), (idx, *v_idx)], outs,
                           lambda v: ref(v[0], v[1], v_ggsw[0], v[2]))
    SO.check_case(engine, case)


# ---- NTT PBS ----------------------------------------------------------------------------------------------------------------
N_LWE, BATCH = 8, 3


def _pbs_want(oracle, n, k, base_log, level, bnf, ms_mode):
    """lwe_out[b] = SampleExtract_0(BlindRotate(lut of item b, lwe_in[b])), through the oracle's batched rotation."""
    ctx = oracle.NttContext(n, P)
    q = 0 if bnf else P

    def rotate(acc, lwe, bsk):
        return ctx.blind_rotate_batch(acc, lwe, bsk, k, base_log, level, bnf=bnf, ms_mode=ms_mode, threads=4)

    def pbs(luts, lwe, bsk):
        return np.stack([oracle.sample_extract(r, n, k, q) for r in rotate(luts, lwe, bsk)])
    return rotate, pbs


def _lwe_values(g, shape, bnf, ms_mode, n):
    if ms_mode == 2:
        return two(g, shape, 2 * n)  # already switched: [0, 2N)
    return two(g, shape, 0 if bnf else P)


@pytest.mark.parametrize("entry", ["pbs", "lut_indexed", "per_item", "blind_rotate"])
@pytest.mark.parametrize("ms_mode", [0, 2], ids=["standard", "pre_switched"])
@pytest.mark.parametrize("bnf", [True, False], ids=["bnf", "solinas"])
@pytest.mark.parametrize("n,k,base_log,level", [(2048, 1, 23, 1), (1024, 2, 12, 2)])
def test_ntt_pbs(engine, oracle, n, k, base_log, level, bnf, ms_mode, entry):
    """n_lwe = 8, batch 3.  At the twisted shape Solinas / STANDARD switches the mask into scratch (`sw`); PRE_SWITCHED
    lifts the input into scratch (`lifted`) everywhere but on the Solinas twisted engine (c_api_pbs.cpp pbs_common)."""
    M = engine.ntt64_pbs
    plan = engine.Plan.cached(n, P)
    g = H.rng(n + 2 * bnf + ms_mode + 11 * len(entry))
    q = 0 if bnf else P
    bsk = H.uniform_q(g, (N_LWE, level, k + 1, k + 1, n), P)
    bsk_dev = SO.to_dev(bsk)
    key = M.NttBootstrapKey(plan, bsk_dev, base_log, level, M.BNF if bnf else M.SOLINAS)
    rotate, pbs = _pbs_want(oracle, n, k, base_log, level, bnf, ms_mode)
    lwe = zeros((BATCH, N_LWE + 1))
    v_lwe = _lwe_values(g, (BATCH, N_LWE + 1), bnf, ms_mode, n)
    fn = (M.programmable_bootstrap_ntt64_bnf_lwe_ciphertext_mem_optimized if bnf else
          M.programmable_bootstrap_ntt64_lwe_ciphertext_mem_optimized)
    name = f"ntt-pbs-{n}-{'bnf' if bnf else 'sol'}-ms{ms_mode}-{entry}"
    out = zeros((BATCH, k * n + 1))
    if entry == "pbs":
        lut = zeros((k + 1, n))
        case = SO.Case(name, lambda: fn(lwe, out, lut, key, ms_mode), [(lwe, *v_lwe), (lut, *two(g, (k + 1, n), q))],
                       [out], lambda v: [pbs(np.broadcast_to(v[1], (BATCH, k + 1, n)), v[0], bsk)])
    elif entry == "lut_indexed":
        luts, idx = zeros((2, k + 1, n)), zeros((BATCH,), "int32")
        v_idx = (np.array([1, 0, 1], np.uint32), np.array([0, 1, 0], np.uint32))
        case = SO.Case(name, lambda: fn(lwe, out, luts, key, ms_mode, lut_index=idx),
                       [(lwe, *v_lwe), (luts, *two(g, (2, k + 1, n), q)), (idx, *v_idx)], [out],
                       lambda v: [pbs(v[1][v[2]], v[0], bsk)])
    elif entry == "per_item":  # lut_index NULL: item b bootstraps through GLWE b
        import ctypes
        from tfhe_ntt_amd._lib import check, lib
        luts = zeros((BATCH, k + 1, n))
        call = lambda: check(lib().mi_pbs_ntt64_batch_lut_indexed(
            key._h, ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(lwe.data_ptr()), ctypes.c_void_p(luts.data_ptr()),
            None, BATCH, BATCH, ms_mode, M._stream(out)))
        case = SO.Case(name, call, [(lwe, *v_lwe), (luts, *two(g, (BATCH, k + 1, n), q))], [out],
                       lambda v: [pbs(v[1], v[0], bsk)])
    else:
        acc = zeros((BATCH, k + 1, n))
        rot = M.blind_rotate_ntt64_bnf_assign if bnf else M.blind_rotate_ntt64_assign
        case = SO.Case(name, lambda: rot(lwe, acc, key, ms_mode), [(lwe, *v_lwe), (acc, *two(g, (BATCH, k + 1, n), q))],
                       [acc], lambda v: [rotate(v[1], v[0], bsk)])
    SO.check_case(engine, case)


@pytest.mark.parametrize("modulus", [0, P], ids=["native", "solinas"])
def test_sample_extract(engine, oracle, modulus):
    M = engine.ntt64_pbs
    n, k, nth, stride, count = 1024, 2, 5, 300, 3
    g = H.rng(0x5E + (modulus != 0))
    glwe, out = zeros((BATCH, k + 1, n)), zeros((BATCH, count, k * n + 1))
    want = lambda v: [np.stack([[oracle.sample_extract_nth(v[0][b], n, k, nth + j * stride, modulus) for j in range(count)]
                                for b in range(BATCH)])]
    case = SO.Case(f"sample_extract-{modulus != 0}",
                   lambda: M.extract_lwe_sample_from_glwe_ciphertext(glwe, out, nth, stride, count, modulus),
                   [(glwe, *two(g, (BATCH, k + 1, n), modulus))], [out], want)
    SO.check_case(engine, case)


# ---- f64 FFT ---------------------------------------------------------------------------------------------------------------
def _fourier_of(engine, fft, std):
    """forward_as_torus of a host array, run on an idle device (setup: valid Fourier operands for the entries below)."""
    import torch
    src = SO.to_dev(std)
    dst = torch.zeros(std.shape[:-1] + (fft.n // 2, 2), dtype=torch.float64, device="cuda")
    fft.forward_as_torus(dst, src)
    torch.cuda.synchronize()
    return dst.cpu().numpy()


def _fft_case(engine, entry, n, g):
    import torch
    F = engine.fft64
    fft = F.Fft(n)
    k, base_log, level = (1, 23, 1) if n == 2048 else (2, 15, 1)
    fz = lambda shape: torch.zeros(shape + (n // 2, 2), dtype=torch.float64, device="cuda")
    name = f"fft64-{n}-{entry}"
    if entry == "forward_torus":
        std, fo = zeros((BATCH, n)), fz((BATCH,))
        return SO.Case(name, lambda: fft.forward_as_torus(fo, std), [(std, *two(g, (BATCH, n)))], [fo])
    if entry == "backward_torus":
        std, fo = zeros((BATCH, n)), fz((BATCH,))
        vals = tuple(_fourier_of(engine, fft, v) for v in two(g, (BATCH, n)))
        return SO.Case(name, lambda: fft.backward_as_torus(std, fo), [(fo, *vals)], [std])
    if entry in ("ext_product", "cmux"):
        out, glwe, ggsw = zeros((BATCH, k + 1, n)), zeros((BATCH, k + 1, n)), fz((level, k + 1, k + 1))
        v_ggsw = tuple(_fourier_of(engine, fft, v) for v in two(g, (level, k + 1, k + 1, n)))
        fn = ((lambda ct0, gg, ct1, *a: F.cmux_assign(ct0, ct1, gg, *a)) if entry == "cmux" else
              F.add_external_product_assign)
        return SO.Case(name, lambda: fn(out, ggsw, glwe, base_log, level, fft),
                       [(out, *two(g, (BATCH, k + 1, n))), (glwe, *two(g, (BATCH, k + 1, n))), (ggsw, *v_ggsw)],
                       [out, glwe] if entry == "cmux" else [out])
    # the bootstraps: the key references the caller's Fourier tensor, so the key data is a delayed operand too
    fbsk = fz((N_LWE, level, k + 1, k + 1))
    v_bsk = tuple(_fourier_of(engine, fft, v) for v in two(g, (N_LWE, level, k + 1, k + 1, n)))
    key = F.FourierLweBootstrapKey(fbsk, base_log, level, fft)
    lwe, out = zeros((BATCH, N_LWE + 1)), zeros((BATCH, k * n + 1))
    ops = [(lwe, *two(g, (BATCH, N_LWE + 1))), (fbsk, *v_bsk)]
    if entry == "pbs":
        lut = zeros((k + 1, n))
        case = SO.Case(name, lambda: F.programmable_bootstrap_lwe_ciphertext(lwe, out, lut, key),
                       ops + [(lut, *two(g, (k + 1, n)))], [out])
    elif entry == "pbs_lut_indexed":
        luts, idx = zeros((2, k + 1, n)), zeros((BATCH,), "int32")
        v_idx = (np.array([1, 0, 1], np.uint32), np.array([0, 1, 0], np.uint32))
        case = SO.Case(name, lambda: F.programmable_bootstrap_lwe_ciphertext(lwe, out, luts, key, lut_index=idx),
                       ops + [(luts, *two(g, (2, k + 1, n))), (idx, *v_idx)], [out])
    else:
        assert entry == "blind_rotate"
        acc = zeros((BATCH, k + 1, n))
        case = SO.Case(name, lambda: F.blind_rotate_assign(lwe, acc, key, F.MS_STANDARD),
                       ops + [(acc, *two(g, (BATCH, k + 1, n)))], [acc])
    case.keep = key
    return case


@pytest.mark.parametrize("entry", ["forward_torus", "backward_torus", "ext_product", "cmux", "pbs", "pbs_lut_indexed",
                                   "blind_rotate"])
@pytest.mark.parametrize("n", [2048, 256], ids=["one_wave", "generic"])
def test_fft64(engine, n, entry):
    """The one-wave engine (N = 2048) and the shape-generic one (N = 256, k = 2: its digit spectra live in scratch).
    Expected values: the quiescent run of the same call, which must repeat bit for bit."""
    SO.check_case(engine, _fft_case(engine, entry, n, H.rng(n + len(entry))))


@pytest.mark.parametrize("entry", ["pbs", "blind_rotate"])
def test_fft64_multi_bit(engine, entry):
    """The multi-bit bootstrap at grouping factor 2 (N = 2048, k = 1): 8 mask elements in 4 groups of 4 GGSWs."""
    import torch
    F = engine.fft64
    n, k, base_log, level, gf = 2048, 1, 23, 1, 2
    fft = F.Fft(n)
    g = H.rng(0xB17 + len(entry))
    shape = (N_LWE // gf, 1 << gf, level, k + 1, k + 1)
    fbsk = torch.zeros(shape + (n // 2, 2), dtype=torch.float64, device="cuda")
    v_bsk = tuple(_fourier_of(engine, fft, v) for v in two(g, shape + (n,)))
    key = F.FourierLweMultiBitBootstrapKey(fbsk, base_log, level, gf, fft)
    lwe = zeros((BATCH, N_LWE + 1))
    ops = [(lwe, *two(g, (BATCH, N_LWE + 1))), (fbsk, *v_bsk)]
    if entry == "pbs":
        lut, out = zeros((k + 1, n)), zeros((BATCH, k * n + 1))
        case = SO.Case("fft64-multi-bit-pbs", lambda: F.multi_bit_programmable_bootstrap_lwe_ciphertext(lwe, out, lut, key),
                       ops + [(lut, *two(g, (k + 1, n)))], [out])
    else:
        acc = zeros((BATCH, k + 1, n))
        case = SO.Case("fft64-multi-bit-blind-rotate", lambda: F.multi_bit_blind_rotate_assign(lwe, acc, key),
                       ops + [(acc, *two(g, (BATCH, k + 1, n)))], [acc])
    SO.check_case(engine, case)


# ---- keyswitch family ---------------------------------------------------------------------------------------------------------
def _keyswitch_case(engine, oracle, in_dim, out_dim, base_log, level, batch, g):
    K = engine.lwe_keyswitch
    ksk = H.uniform_u64(g, (in_dim, level, out_dim + 1))
    key = K.LweKeyswitchKey(SO.to_dev(ksk), base_log, level)
    lwe, out = zeros((batch, in_dim + 1)), zeros((batch, out_dim + 1))
    case = SO.Case(f"keyswitch-{in_dim}-{out_dim}-{base_log}-{level}", lambda: K.keyswitch_lwe_ciphertext(key, lwe, out),
                   [(lwe, *two(g, (batch, in_dim + 1)))], [out],
                   lambda v: [oracle.lwe_keyswitch(ksk, v[0], out_dim, base_log, level)])
    case.keep = key
    return case


@pytest.mark.parametrize("in_dim,out_dim,base_log,level,batch", [
    (40, 24, 4, 4, 5),     # one byte per digit
    (33, 17, 10, 2, 3),    # digits wider than a signed byte: two bytes per digit
])
def test_keyswitch(engine, oracle, in_dim, out_dim, base_log, level, batch):
    SO.check_case(engine, _keyswitch_case(engine, oracle, in_dim, out_dim, base_log, level, batch, H.rng(in_dim)))


@pytest.mark.parametrize("in_dim,out_dim,base_log,level,w", [(40, 24, 2, 8, 21), (33, 17, 16, 2, 32)])
def test_keyswitch32(engine, oracle, in_dim, out_dim, base_log, level, w):
    K = engine.lwe_keyswitch
    g = H.rng(in_dim + w)
    ksk = two32(g, (in_dim, level, out_dim + 1))[0]
    key = K.LweKeyswitchKey32(SO.to_dev(ksk), base_log, level, w)
    lwe, out = zeros((5, in_dim + 1)), zeros((5, out_dim + 1), "int32")
    case = SO.Case(f"keyswitch32-{in_dim}-{w}", lambda: K.keyswitch_lwe_ciphertext_with_scalar_change(key, lwe, out),
                   [(lwe, *two(g, (5, in_dim + 1)))], [out],
                   lambda v: [oracle.lwe_keyswitch32(ksk, v[0], out_dim, base_log, level, w)])
    SO.check_case(engine, case)


@pytest.mark.parametrize("centered", [False, True], ids=["standard", "centered"])
@pytest.mark.parametrize("bits", [32, 64])
def test_modulus_switch(engine, oracle, bits, centered):
    K = engine.lwe_keyswitch
    g = H.rng(bits + centered)
    dim, batch, log_mod = 40, 5, 12
    out = zeros((batch, dim + 1))
    if bits == 32:
        lwe = zeros((batch, dim + 1), "int32")
        case = SO.Case(f"ms32-{centered}", lambda: K.lwe_ciphertext_modulus_switch32(lwe, out, log_mod, centered),
                       [(lwe, *two32(g, (batch, dim + 1)))], [out], lambda v: [oracle.lwe_ms32(v[0], log_mod, centered)])
    else:
        lwe = zeros((batch, dim + 1))
        case = SO.Case(f"ms64-{centered}", lambda: K.lwe_ciphertext_modulus_switch(lwe, out, log_mod, centered),
                       [(lwe, *two(g, (batch, dim + 1)))], [out], lambda v: [oracle.lwe_ms64(v[0], log_mod, centered)])
    SO.check_case(engine, case)


def _packing_case(engine, oracle, in_dim, k, n, base_log, level, n_lwe, per, g):
    K = engine.lwe_packing_keyswitch
    pksk = H.uniform_u64(g, (in_dim, level, k + 1, n))
    key = K.LwePackingKeyswitchKey(SO.to_dev(pksk), base_log, level)
    lwe, out = zeros((n_lwe, in_dim + 1)), zeros(((n_lwe + per - 1) // per, k + 1, n))
    case = SO.Case(f"packing-ks-{in_dim}-{base_log}-{level}",
                   lambda: K.keyswitch_lwe_ciphertext_list_and_pack_in_glwe_ciphertext(key, lwe, out, per),
                   [(lwe, *two(g, (n_lwe, in_dim + 1)))], [out],
                   lambda v: [PH.packing_keyswitch_ref(oracle, pksk, v[0], k, n, base_log, level, per)])
    case.keep = key
    return case


@pytest.mark.parametrize("base_log,level", [(4, 3), (10, 2)], ids=["one_byte", "two_bytes"])
def test_packing_keyswitch(engine, oracle, base_log, level):
    """mi_lwe_packing_keyswitch_batch (keyswitched rows and their digits in scratch): 5 ciphertexts, 2 per GLWE, the last
    GLWE holding the remainder.  The piecewise path (rows beyond the 64 MiB scratch bound) needs a large call and stays
    with test_packing_ks_gpu.py."""
    SO.check_case(engine, _packing_case(engine, oracle, 40, 1, 32, base_log, level, 5, 2, H.rng(base_log)))


@pytest.mark.parametrize("entry", ["compress", "extract"])
def test_glwe_compression(engine, oracle, entry):
    import ctypes
    from tfhe_ntt_amd._lib import check, lib
    K = engine.lwe_packing_keyswitch
    C = K.CompressedModulusSwitchedGlweCiphertext
    k, n, bodies, log_modulus, batch = 1, 32, 20, 12, 3
    g = H.rng(0xC0DE + len(entry))
    words = C.packed_words(k, n, bodies, log_modulus)
    glwe, packed = zeros((batch, k + 1, n)), zeros((batch, words))
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    compress = lambda v: np.stack([PH.compress_ref(oracle, v[b], k, n, bodies, log_modulus) for b in range(batch)])
    if entry == "compress":
        call = lambda: check(lib().mi_glwe_compress_batch(ptr(packed), ptr(glwe), n, k, bodies, log_modulus, batch, 0,
                                                         engine.ntt64_pbs._stream(glwe)))
        case = SO.Case("glwe-compress", call, [(glwe, *two(g, (batch, k + 1, n)))], [packed], lambda v: [compress(v[0])])
    else:
        vals = tuple(compress(v) for v in two(g, (batch, k + 1, n)))
        ct = C(packed, k, n, bodies, log_modulus)
        case = SO.Case("glwe-extract", lambda: ct.extract(glwe), [(packed, *vals)], [glwe],
                       lambda v: [np.stack([PH.extract_ref(v[0][b], k, n, bodies, log_modulus) for b in range(batch)])])
    SO.check_case(engine, case)


def _words128(g, shape):
    return tuple(g.integers(0, 1 << 64, size=tuple(shape) + (2,), dtype=np.uint64) for _ in range(2))


@pytest.mark.parametrize("entry", ["packing_keyswitch", "compress", "extract"])
def test_noise_squashing_compression(engine, entry):
    """The 128-bit counterparts: mi_lwe_packing_keyswitch128_batch (a scratch user; 5 ciphertexts, 2 per GLWE),
    mi_glwe_compress128_batch and mi_glwe_extract128_batch; mi_lwe_pksk128_create is in test_synchronising_entries."""
    import ctypes
    from tfhe_ntt_amd._lib import check, lib
    K = engine.noise_squashing_compression
    C = K.CompressedModulusSwitchedGlweCiphertext128
    g = R.rng(0x9128 + len(entry))
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    if entry == "packing_keyswitch":
        in_dim, k, n, base_log, level, n_lwe, per = 20, 1, 8, 24, 3, 5, 2
        pksk = _words128(g, (in_dim, level, k + 1, n))[0]
        key = K.LwePackingKeyswitchKey128(SO.to_dev(pksk), base_log, level)
        lwe, out = zeros((n_lwe, in_dim + 1, 2)), zeros((3, k + 1, n, 2))
        case = SO.Case("packing-ks128", lambda: K.keyswitch_lwe_ciphertext_list_and_pack_in_glwe_ciphertext(key, lwe, out, per),
                       [(lwe, *_words128(g, (n_lwe, in_dim + 1)))], [out],
                       lambda v: [Q.packing_keyswitch128_ref(pksk, v[0], k, n, base_log, level, per)])
    else:
        k, n, bodies, log_modulus, batch = 1, 8, 5, 100, 3
        words = C.packed_words(k, n, bodies, log_modulus)
        glwe, packed = zeros((batch, k + 1, n, 2)), zeros((batch, words, 2))
        compress = lambda v: R.to_words([Q.compress128_ref(R.from_words(v[b].reshape(-1, 2)), k, n, bodies, log_modulus)
                                         for b in range(batch)])
        st = lambda: engine.ntt64_pbs._stream(glwe)
        if entry == "compress":
            call = lambda: check(lib().mi_glwe_compress128_batch(ptr(packed), ptr(glwe), n, k, bodies, log_modulus,
                                                                batch, 0, st()))
            case = SO.Case("glwe-compress128", call, [(glwe, *_words128(g, (batch, k + 1, n)))], [packed],
                           lambda v: [compress(v[0])])
        else:
            vals = tuple(compress(v) for v in _words128(g, (batch, k + 1, n)))
            call = lambda: check(lib().mi_glwe_extract128_batch(ptr(glwe), ptr(packed), n, k, bodies, log_modulus,
                                                               batch, 0, st()))
            extract = lambda v: R.to_words([Q.extract128_ref(R.from_words(v[b]), k, n, bodies, log_modulus)
                                            for b in range(batch)]).reshape(batch, k + 1, n, 2)
            case = SO.Case("glwe-extract128", call, [(packed, *vals)], [glwe], lambda v: [extract(v[0])])
    SO.check_case(engine, case)


@pytest.mark.parametrize("entry", ["measure", "measure_all", "choose", "improve", "improve_and_switch"])
def test_ms_noise_reduction(engine, entry):
    """The four drift-technique entries (measure with and without the candidates' table).  The bound is 0, so no
    candidate satisfies it and every item takes the encryption of zero with the smallest measure: the choice depends on
    the data of every item.  `satisfied` is then 0 for the true and the decoy set alike, the one output that cannot
    differ; it is still compared."""
    import ctypes
    import torch
    from tfhe_ntt_amd._lib import check, lib
    K = engine.modulus_switch_noise_reduction
    dim, count, batch, log_modulus = 33, 5, 4, 12
    p = MS.Params(0.0, MS.TEST_PARAM.r_sigma, MS.TEST_PARAM.input_variance, log_modulus)
    g = H.rng(0x35 + len(entry))
    zeros_h = H.uniform_u64(g, (count, dim + 1))
    key = K.ModulusSwitchNoiseReductionKey(SO.to_dev(zeros_h), p.bound, p.r_sigma, p.input_variance)
    lwe = zeros((batch, dim + 1))
    ops = [(lwe, *two(g, (batch, dim + 1)))]
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    st = lambda: engine.ntt64_pbs._stream(lwe)
    chosen = lambda v: MS.choose_np(v, zeros_h, p)
    same_ok = ()
    if entry.startswith("measure"):
        every = entry == "measure_all"
        out = torch.zeros((batch, 1 + count if every else 1), dtype=torch.float64, device="cuda")
        call = lambda: check(lib().mi_lwe_ms_noise_measure_batch(key._h, ptr(out), ptr(lwe), batch, log_modulus,
                                                                 int(every), st()))
        outs, want = [out], lambda v: [MS.all_measures_np(v[0], zeros_h, p)[:, :out.shape[1]]]
    elif entry == "choose":
        cand, sat = zeros((batch,)), zeros((batch,), "int32")
        call = lambda: check(lib().mi_lwe_ms_noise_choose_batch(key._h, ptr(cand), ptr(sat), ptr(lwe), batch,
                                                                log_modulus, st()))
        outs, want, same_ok = [cand, sat], lambda v: list(chosen(v[0])), (1,)
    elif entry == "improve":
        out = zeros((batch, dim + 1))
        call = lambda: check(lib().mi_lwe_ms_noise_improve_batch(key._h, ptr(out), ptr(lwe), batch, log_modulus, None,
                                                                 None, st()))
        outs, want = [out], lambda v: [MS.improve_np(v[0], zeros_h, chosen(v[0])[0])]
    else:
        out = zeros((batch, dim + 1))
        call = lambda: key.improve_noise_and_modulus_switch(lwe, out, log_modulus)
        outs, want = [out], lambda v: [MS.switch_np(MS.improve_np(v[0], zeros_h, chosen(v[0])[0]), log_modulus)]
    case = SO.Case(f"ms-noise-{entry}", call, ops, outs, want)
    case.decoy_may_match = same_ok
    SO.check_case(engine, case)


# ---- the 128-bit bootstrap --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["ext_product", "cmux", "blind_rotate", "pbs"])
def test_pbs128(engine, entry):
    """The four entries at test_pbs128_gpu.py's smallest shape (N = 256, k = 1, base 2^23, 1 level), two GGSWs, batch 2
    (digits, limb products and u128 accumulators in scratch), against pbs128_helpers' integer reference."""
    M = engine.pbs128
    n, k, base_log, level, n_ggsw, batch = 256, 1, 23, 1, 2, 2
    g = R.rng(0x128 + len(entry))
    bsk = [R.uniform_ggsw(g, k, n, level) for _ in range(n_ggsw)]
    key = M.LweBootstrapKey128(SO.to_dev(R.to_words(bsk)), base_log, level)
    packed = [R.PackedGgsw(x, base_log) for x in bsk]
    glwes = lambda count=batch: tuple(R.to_words([R.uniform_glwe(g, k, n) for _ in range(count)]) for _ in range(2))
    lwes = two(g, (batch, n_ggsw + 1))
    log = n.bit_length()  # log2(2N)
    switched = lambda lwe: [R.switch_lwe([int(x) for x in row], log) for row in lwe]
    a, b = zeros((batch, k + 1, n, 2)), zeros((batch, k + 1, n, 2))
    lwe = zeros((batch, n_ggsw + 1))

    def ext(v):
        out = R.from_words(v[0])
        for i in range(batch):
            R.external_product(out[i], packed[1], R.from_words(v[1][i]), level)
        return [R.to_words(out)]

    def cmux(v):
        ct0, ct1 = R.from_words(v[0]), R.from_words(v[1])
        for i in range(batch):
            R.cmux(ct0[i], ct1[i], packed[1], level)
        return [R.to_words(ct0), R.to_words(ct1)]

    if entry == "ext_product":
        case = SO.Case("pbs128-ext", lambda: M.add_external_product_assign(a, key, 1, b), [(a, *glwes()), (b, *glwes())],
                       [a], ext)
    elif entry == "cmux":
        case = SO.Case("pbs128-cmux", lambda: M.cmux_assign(a, b, key, 1), [(a, *glwes()), (b, *glwes())], [a, b], cmux)
    elif entry == "blind_rotate":
        case = SO.Case("pbs128-blind-rotate", lambda: M.blind_rotate_assign(key, a, lwe, 0), [(a, *glwes()), (lwe, *lwes)],
                       [a], lambda v: [R.to_words([R.blind_rotate(acc, sw, packed, level)
                                                   for acc, sw in zip(R.from_words(v[0]), switched(v[1]))])])
    else:
        lut, out = zeros((k + 1, n, 2)), zeros((batch, k * n + 1, 2))
        v_lut = tuple(x[0] for x in glwes(1))
        case = SO.Case("pbs128-pbs", lambda: M.programmable_bootstrap_f128_lwe_ciphertext(lwe, out, lut, key, 0),
                       [(lut, *v_lut), (lwe, *lwes)], [out],
                       lambda v: [R.to_words([R.pbs(R.from_words(v[0]), sw, packed, level) for sw in switched(v[1])])])
    SO.check_case(engine, case)


# ---- entries that synchronise `stream` before they return: the operand half only ------------------------------------------------
@pytest.mark.parametrize("entry", ["ksk", "ksk32", "pksk", "pksk128", "ms_noise_key", "pbs128_key", "pbs_key", "ggsw"])
def test_synchronising_entries(engine, oracle, entry):
    """The *_create calls prepare a private copy on `stream` and synchronise it (the header says so): the key must be
    built from the true operands that arrive on `s` behind the delay, and the delay has drained when the call returns.
    The key made from the delayed buffer is then used once, on `s`, and that result is what is compared."""
    M, K = engine.ntt64_pbs, engine.lwe_keyswitch
    g = H.rng(0x5C + len(entry))
    made = []  # the keys stay alive until the streams are idle
    if entry in ("ksk", "ksk32"):
        in_dim, out_dim, batch = 40, 24, 5
        base_log, level = (4, 4) if entry == "ksk" else (2, 8)
        lwe_h = H.uniform_u64(g, (batch, in_dim + 1))
        lwe = SO.to_dev(lwe_h)
        if entry == "ksk":
            src, out = zeros((in_dim, level, out_dim + 1)), zeros((batch, out_dim + 1))
            vals = two(g, (in_dim, level, out_dim + 1))
            want = lambda v: [oracle.lwe_keyswitch(v[0], lwe_h, out_dim, base_log, level)]

            def call():
                made.append(K.LweKeyswitchKey(src, base_log, level))
                K.keyswitch_lwe_ciphertext(made[-1], lwe, out)
        else:
            src, out = zeros((in_dim, level, out_dim + 1), "int32"), zeros((batch, out_dim + 1), "int32")
            vals = two32(g, (in_dim, level, out_dim + 1))
            want = lambda v: [oracle.lwe_keyswitch32(v[0], lwe_h, out_dim, base_log, level, 21)]

            def call():
                made.append(K.LweKeyswitchKey32(src, base_log, level, 21))
                K.keyswitch_lwe_ciphertext_with_scalar_change(made[-1], lwe, out)
    elif entry == "pksk":
        PK = engine.lwe_packing_keyswitch
        in_dim, k, n, base_log, level, n_lwe, per = 40, 1, 32, 4, 3, 5, 2
        lwe_h = H.uniform_u64(g, (n_lwe, in_dim + 1))
        lwe = SO.to_dev(lwe_h)
        src, out = zeros((in_dim, level, k + 1, n)), zeros((3, k + 1, n))
        vals = two(g, (in_dim, level, k + 1, n))
        want = lambda v: [PH.packing_keyswitch_ref(oracle, v[0], lwe_h, k, n, base_log, level, per)]

        def call():
            made.append(PK.LwePackingKeyswitchKey(src, base_log, level))
            PK.keyswitch_lwe_ciphertext_list_and_pack_in_glwe_ciphertext(made[-1], lwe, out, per)
    elif entry == "pksk128":
        PK = engine.noise_squashing_compression
        in_dim, k, n, base_log, level, n_lwe, per = 20, 1, 8, 24, 3, 5, 2
        r = R.rng(0x9129)
        lwe_h = _words128(r, (n_lwe, in_dim + 1))[0]
        lwe = SO.to_dev(lwe_h)
        src, out = zeros((in_dim, level, k + 1, n, 2)), zeros((3, k + 1, n, 2))
        vals = _words128(r, (in_dim, level, k + 1, n))
        want = lambda v: [Q.packing_keyswitch128_ref(v[0], lwe_h, k, n, base_log, level, per)]

        def call():
            made.append(PK.LwePackingKeyswitchKey128(src, base_log, level))
            PK.keyswitch_lwe_ciphertext_list_and_pack_in_glwe_ciphertext(made[-1], lwe, out, per)
    elif entry == "ms_noise_key":
        N = engine.modulus_switch_noise_reduction
        dim, count, batch, log_modulus = 33, 5, 4, 12
        p = MS.Params(0.0, MS.TEST_PARAM.r_sigma, MS.TEST_PARAM.input_variance, log_modulus)
        lwe_h = H.uniform_u64(g, (batch, dim + 1))
        lwe = SO.to_dev(lwe_h)
        src, out = zeros((count, dim + 1)), zeros((batch, dim + 1))
        vals = two(g, (count, dim + 1))
        want = lambda v: [MS.switch_np(MS.improve_np(lwe_h, v[0], MS.choose_np(lwe_h, v[0], p)[0]), log_modulus)]

        def call():
            made.append(N.ModulusSwitchNoiseReductionKey(src, p.bound, p.r_sigma, p.input_variance))
            made[-1].improve_noise_and_modulus_switch(lwe, out, log_modulus)
    elif entry == "pbs128_key":
        B = engine.pbs128
        n, k, base_log, level = 256, 1, 23, 1
        r = R.rng(0x129)
        vals = tuple(R.to_words([R.uniform_ggsw(r, k, n, level)]) for _ in range(2))
        acc_h, glwe_h = (R.to_words([R.uniform_glwe(r, k, n) for _ in range(2)]) for _ in range(2))
        acc0, glwe = SO.to_dev(acc_h), SO.to_dev(glwe_h)
        src, out = zeros(vals[0].shape), zeros(acc_h.shape)

        def want(v):
            res, packed = R.from_words(acc_h), R.PackedGgsw(R.from_words(v[0])[0], base_log)
            for i in range(2):
                R.external_product(res[i], packed, R.from_words(glwe_h[i]), level)
            return [R.to_words(res)]

        def call():
            made.append(B.LweBootstrapKey128(src, base_log, level))
            out.copy_(acc0)
            B.add_external_product_assign(out, made[-1], 0, glwe)
    elif entry == "pbs_key":  # BNF keys are copied with N^-1 folded in; the twisted shape re-orders the copy
        n, k, base_log, level = 2048, 1, 23, 1
        plan = engine.Plan.cached(n, P)
        _, pbs = _pbs_want(oracle, n, k, base_log, level, True, 0)
        lwe_h, lut_h = H.uniform_u64(g, (BATCH, N_LWE + 1)), H.uniform_u64(g, (k + 1, n))
        lwe, lut = SO.to_dev(lwe_h), SO.to_dev(lut_h)
        src, out = zeros((N_LWE, level, k + 1, k + 1, n)), zeros((BATCH, k * n + 1))
        vals = two(g, (N_LWE, level, k + 1, k + 1, n), P)
        want = lambda v: [pbs(np.broadcast_to(lut_h, (BATCH, k + 1, n)), lwe_h, v[0])]

        def call():
            made.append(M.NttBootstrapKey(plan, src, base_log, level, M.BNF))
            M.programmable_bootstrap_ntt64_bnf_lwe_ciphertext_mem_optimized(lwe, out, lut, made[-1])
    else:  # the twisted shape's prepared GGSW list: permuted once into a private copy
        n, k, base_log, level = 2048, 1, 23, 1
        plan = engine.Plan.cached(n, P)
        ref = _ext_want(oracle, n, k, base_log, level, True, False)
        acc_h, glwe_h = H.uniform_u64(g, (BATCH, k + 1, n)), H.uniform_u64(g, (BATCH, k + 1, n))
        glwe = SO.to_dev(glwe_h)
        src, out = zeros((2, level, k + 1, k + 1, n)), zeros((BATCH, k + 1, n))
        vals = two(g, (2, level, k + 1, k + 1, n), P)
        want = lambda v: ref(acc_h, glwe_h, v[0], [1] * BATCH)
        acc0, ones = SO.to_dev(acc_h), SO.to_dev(np.ones(BATCH, np.uint32))

        def call():
            made.append(M.NttGgswList(plan, src, base_log, level, M.BNF))
            out.copy_(acc0)
            M.add_external_product_ntt64_bnf_assign(plan, out, made[-1], glwe, base_log, level, ggsw_index=ones)
    SO.check_case(engine, SO.Case(f"create-{entry}", call, [(src, *vals)], [out], want, sync=True))
    import torch
    torch.cuda.synchronize()
    made.clear()


# ---- scratch hand-over between two streams --------------------------------------------------------------------------------------
class Site:
    """One scratch user for the hand-over test: per side ("A" / "B") inputs of its own for the largest batch, one
    output per call, the call on the first `size` items, and the expected rows."""

    def __init__(self, sizes, new_out, issue, want):
        self.sizes, self.new_out, self._issue, self.want = sizes, new_out, issue, want
        self.reset()

    def reset(self):
        self.outs = {(side, r): self.new_out(side, size) for r, size in enumerate(self.sizes) for side in "AB"}
        self.outs.update({(side, -1): self.new_out(side, self.sizes[0]) for side in "AB"})

    def issue(self, side, r, size):
        self._issue(side, size, self.outs[(side, r)])


def _site(engine, oracle, user):
    import torch
    M, K, F = engine.ntt64_pbs, engine.lwe_keyswitch, engine.fft64
    g = H.rng(0x0A + len(user))
    sizes = [4, 2, 9, 5]  # per round; the third round outgrows the blocks of the first two
    top = max(sizes)
    if user == "keyswitch":
        in_dim, out_dim, base_log, level = 40, 24, 4, 4
        sizes = [300, 100, 70000, 500]  # 70000 x 160 digit bytes outgrow the 1 MiB block: grow-and-supersede
        top = max(sizes)
        ksk = H.uniform_u64(g, (in_dim, level, out_dim + 1))
        key = K.LweKeyswitchKey(SO.to_dev(ksk), base_log, level)
        lwe = {s: H.uniform_u64(g, (top, in_dim + 1)) for s in "AB"}
        dev = {s: SO.to_dev(lwe[s]) for s in "AB"}
        return Site(sizes, lambda s, b: zeros((b, out_dim + 1)),
                    lambda s, b, out: K.keyswitch_lwe_ciphertext(key, dev[s][:b], out),
                    lambda s: oracle.lwe_keyswitch(ksk, lwe[s], out_dim, base_log, level, threads=16))
    if user == "pks":
        PK = engine.lwe_packing_keyswitch
        in_dim, k, n, base_log, level = 40, 1, 32, 4, 3
        pksk = H.uniform_u64(g, (in_dim, level, k + 1, n))
        key = PK.LwePackingKeyswitchKey(SO.to_dev(pksk), base_log, level)
        lwe = {s: H.uniform_u64(g, (top, in_dim + 1)) for s in "AB"}
        dev = {s: SO.to_dev(lwe[s]) for s in "AB"}
        return Site(sizes, lambda s, b: zeros((b, k + 1, n)),  # one ciphertext per GLWE: item b is row b
                    lambda s, b, out: PK.keyswitch_lwe_ciphertext_into_glwe_ciphertext(key, dev[s][:b], out),
                    lambda s: PH.packing_keyswitch_ref(oracle, pksk, lwe[s], k, n, base_log, level, 1))
    if user == "pks128":
        PK = engine.noise_squashing_compression
        in_dim, k, n, base_log, level = 20, 1, 8, 24, 3
        r = R.rng(0x912A)
        pksk = _words128(r, (in_dim, level, k + 1, n))[0]
        key = PK.LwePackingKeyswitchKey128(SO.to_dev(pksk), base_log, level)
        lwe = {s: _words128(r, (top, in_dim + 1))[0] for s in "AB"}
        dev = {s: SO.to_dev(lwe[s]) for s in "AB"}
        return Site(sizes, lambda s, b: zeros((b, k + 1, n, 2)),
                    lambda s, b, out: PK.keyswitch_lwe_ciphertext_list_and_pack_in_glwe_ciphertext(key, dev[s][:b], out, 1),
                    lambda s: Q.packing_keyswitch128_ref(pksk, lwe[s], k, n, base_log, level, 1))
    if user == "pbs128":  # digits, limb products and u128 accumulators of a chunk in one block (pbs128.hip)
        B = engine.pbs128
        n, k, base_log, level = 256, 1, 23, 1
        sizes = [3, 1, 4, 2]
        r = R.rng(0x12A)
        bsk = [R.uniform_ggsw(r, k, n, level)]
        key = B.LweBootstrapKey128(SO.to_dev(R.to_words(bsk)), base_log, level)
        packed = [R.PackedGgsw(bsk[0], base_log)]
        lut = {s: R.uniform_glwe(r, k, n) for s in "AB"}
        lwe = {s: H.uniform_u64(g, (max(sizes), 2)) for s in "AB"}
        dt, dl = {s: SO.to_dev(R.to_words(lut[s])) for s in "AB"}, {s: SO.to_dev(lwe[s]) for s in "AB"}
        site = Site(sizes, lambda s, b: zeros((b, k * n + 1, 2)),
                    lambda s, b, out: B.programmable_bootstrap_f128_lwe_ciphertext(dl[s][:b], out, dt[s], key, 0),
                    lambda s: R.to_words([R.pbs(lut[s], R.switch_lwe([int(x) for x in row], n.bit_length()), packed, level)
                                          for row in lwe[s]]))
        site.keep = key
        return site
    if user == "native":
        n = 32
        plan = engine.native64.Plan32.try_new(n)
        vals = {s: two(g, (top, n)) for s in "AB"}
        dev = {s: tuple(SO.to_dev(v) for v in vals[s]) for s in "AB"}
        return Site(sizes, lambda s, b: zeros((b, n)),
                    lambda s, b, out: plan.negacyclic_polymul(out, dev[s][0][:b], dev[s][1][:b]),
                    lambda s: _native_want(*vals[s]))
    if user == "tw_ext":  # the raw-pointer call at the twisted shape permutes its GGSW into per-call scratch
        n, k, base_log, level = 2048, 1, 23, 1
        plan = engine.Plan.cached(n, P)
        ref = _ext_want(oracle, n, k, base_log, level, True, False)
        ggsw = {s: H.uniform_q(g, (level, k + 1, k + 1, n), P) for s in "AB"}
        glwe = {s: H.uniform_u64(g, (top, k + 1, n)) for s in "AB"}
        dg, dl = {s: SO.to_dev(ggsw[s]) for s in "AB"}, {s: SO.to_dev(glwe[s]) for s in "AB"}
        return Site(sizes, lambda s, b: zeros((b, k + 1, n)),
                    lambda s, b, out: M.add_external_product_ntt64_bnf_assign(plan, out, dg[s], dl[s][:b], base_log, level),
                    lambda s: ref(np.zeros_like(glwe[s]), glwe[s], ggsw[s][None], [0] * top)[0])
    if user in ("pbs_sw", "pbs_lifted", "large"):
        # sw: Solinas / STANDARD on the twisted engine; lifted: BNF / PRE_SWITCHED; large: pbs_large.hip's accumulators
        # (N = 8192, its smallest size), at batches below the 64 items that fork lanes (test_forked_lanes has those)
        bnf, ms_mode = (False, 0) if user == "pbs_sw" else (True, 2) if user == "pbs_lifted" else (True, 0)
        n, k, base_log, level, n_lwe = (8192, 1, 15, 2, 3) if user == "large" else (2048, 1, 23, 1, N_LWE)
        plan = engine.Plan.cached(n, P)
        q = 0 if bnf else P
        bsk = H.uniform_q(g, (n_lwe, level, k + 1, k + 1, n), P)
        key = M.NttBootstrapKey(plan, SO.to_dev(bsk), base_log, level, M.BNF if bnf else M.SOLINAS)
        _, pbs = _pbs_want(oracle, n, k, base_log, level, bnf, ms_mode)
        lut = {s: H.uniform_q(g, (k + 1, n), q) for s in "AB"}
        lwe = {s: _lwe_values(g, (top, n_lwe + 1), bnf, ms_mode, n)[0] for s in "AB"}
        dt, dl = {s: SO.to_dev(lut[s]) for s in "AB"}, {s: SO.to_dev(lwe[s]) for s in "AB"}
        fn = (M.programmable_bootstrap_ntt64_bnf_lwe_ciphertext_mem_optimized if bnf else
              M.programmable_bootstrap_ntt64_lwe_ciphertext_mem_optimized)
        site = Site(sizes, lambda s, b: zeros((b, k * n + 1)),
                    lambda s, b, out: fn(dl[s][:b], out, dt[s], key, ms_mode),
                    lambda s: pbs(np.broadcast_to(lut[s], (top, k + 1, n)), lwe[s], bsk))
        site.keep = key
        return site
    assert user in ("fft_ext", "fft_pbs")  # the generic f64 engine: digit spectra / accumulators in scratch
    n, k, base_log, level = 256, 2, 15, 1
    fft = F.Fft(n)
    if user == "fft_ext":
        ggsw = {s: SO.to_dev(_fourier_of(engine, fft, H.uniform_u64(g, (level, k + 1, k + 1, n)))) for s in "AB"}
        glwe = {s: SO.to_dev(H.uniform_u64(g, (top, k + 1, n))) for s in "AB"}
        issue = lambda s, b, out: F.add_external_product_assign(out, ggsw[s], glwe[s][:b], base_log, level, fft)
        new_out = lambda s, b: zeros((b, k + 1, n))
    else:
        fbsk = SO.to_dev(_fourier_of(engine, fft, H.uniform_u64(g, (N_LWE, level, k + 1, k + 1, n))))
        key = F.FourierLweBootstrapKey(fbsk, base_log, level, fft)
        lut = {s: SO.to_dev(H.uniform_u64(g, (k + 1, n))) for s in "AB"}
        lwe = {s: SO.to_dev(H.uniform_u64(g, (top, N_LWE + 1))) for s in "AB"}
        issue = lambda s, b, out: F.programmable_bootstrap_lwe_ciphertext(lwe[s][:b], out, lut[s], key)
        new_out = lambda s, b: zeros((b, k * n + 1))
    # f64: the expected rows are a quiescent run at the largest batch (every item is computed on its own)
    quiet = {}
    for s in "AB":
        out = new_out(s, top)
        torch.cuda.synchronize()
        issue(s, top, out)
        torch.cuda.synchronize()
        quiet[s] = host(out)
    return Site(sizes, new_out, issue, lambda s: quiet[s])


@pytest.mark.parametrize("user", ["keyswitch", "pks", "pks128", "pbs128", "native", "tw_ext", "pbs_sw", "pbs_lifted", "large", "fft_ext", "fft_pbs"])
def test_hand_over(engine, oracle, user):
    """Two non-blocking streams take turns on one scratch block: eight calls in four rounds, the first of a round behind
    the delay, the second (the other stream, other inputs, same size) right away; the batch changes between rounds, so
    the snug-fit reuse and the grow-and-supersede path both run.  Every call must equal the oracle, the second call of
    a round may complete only behind the first one (it waits on the event of the block it takes over), and the pool
    must end up holding what the same eight calls leave on one stream: shared, not doubled."""
    site = _site(engine, oracle, user)
    single, shared, first_done = SO.hand_over(engine, site.issue, site.sizes, site.reset)
    assert single > 0, "this entry took no scratch: it is not a scratch user at this shape"
    assert shared == single, f"the pool holds {shared} bytes after the two-stream run, {single} after the same calls on one"
    assert all(first_done), f"rounds {[r for r, d in enumerate(first_done) if not d]}: the second call finished before " \
                            "the first one: it did not wait for the scratch block's last user"
    want = {s: site.want(s) for s in "AB"}
    for (s, r), out in site.outs.items():
        if r >= 0:
            b = site.sizes[r]
            assert np.array_equal(host(out), want[s][:b]), f"stream {s}, round {r} (batch {b}) differs from the oracle"


# ---- forked lanes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine_name", ["pbs_large", "fft64_generic"])
def test_forked_lanes(engine, oracle, engine_name):
    """run_blind_rotation (pbs_passes.hpp) splits a chunk of >= 64 items over the caller's stream and pooled side
    streams: 70 items are two lanes of 35 (the shapes of test_pbs_large_gpu.py and test_fft_generic_gpu.py's lane
    tests, n_lwe = 3).  Through the harness the side lanes must be ordered behind the operands that arrive on `s` and the
    copy-out on `s` behind every lane; every row is compared, so both sides of the lane boundary (rows 34 / 35) are.
    Then the hand-over: the scratch is freed on `s`, so a same-size call on another stream may reuse it only behind the
    join."""
    import torch
    M, F = engine.ntt64_pbs, engine.fft64
    batch, n_lwe = 70, 3
    g = H.rng(0xF0 + len(engine_name))
    if engine_name == "pbs_large":
        n, k, base_log, level = 8192, 1, 15, 2
        plan = engine.Plan.cached(n, P)
        bsk = H.uniform_q(g, (n_lwe, level, k + 1, k + 1, n), P)
        key = M.NttBootstrapKey(plan, SO.to_dev(bsk), base_log, level, M.BNF)
        _, pbs = _pbs_want(oracle, n, k, base_log, level, True, 0)
        want = lambda v: [pbs(np.broadcast_to(v[1], (batch, k + 1, n)), v[0], bsk)]
        fn = lambda lwe, out, lut: M.programmable_bootstrap_ntt64_bnf_lwe_ciphertext_mem_optimized(lwe, out, lut, key)
    else:
        n, k, base_log, level = 4096, 1, 12, 2
        fft = F.Fft(n)
        fbsk = SO.to_dev(_fourier_of(engine, fft, H.uniform_u64(g, (n_lwe, level, k + 1, k + 1, n))))
        key = F.FourierLweBootstrapKey(fbsk, base_log, level, fft)
        want = None
        fn = lambda lwe, out, lut: F.programmable_bootstrap_lwe_ciphertext(lwe, out, lut, key)
    lwe, lut, out = zeros((batch, n_lwe + 1)), zeros((k + 1, n)), zeros((batch, k * n + 1))
    case = SO.Case(f"lanes-{engine_name}", lambda: fn(lwe, out, lut), [(lwe, *two(g, (batch, n_lwe + 1))),
                                                                      (lut, *two(g, (k + 1, n)))], [out], want)
    SO.check_case(engine, case)
    expected = case.expected(0)[0]
    assert expected.shape[0] == batch and not np.array_equal(expected[34], expected[35])

    # hand-over: a forked call on A behind the delay, then the same-size call on B
    true_lwe, true_lut = case.staged[0]
    other_lwe, other_lut = case.staged[1]
    outs = {}

    def reset():
        outs.clear()

    def issue(side, r, size):
        outs[(side, r)] = o = zeros((batch, k * n + 1))
        fn(true_lwe if side == "A" else other_lwe, o, true_lut if side == "A" else other_lut)

    single, shared, first_done = SO.hand_over(engine, issue, [batch, batch], reset)
    assert shared == single and all(first_done), (single, shared, first_done)
    torch.cuda.synchronize()
    want_side = {"A": expected, "B": case.expected(1)[0]}
    for (side, r), o in outs.items():
        assert np.array_equal(host(o).view(np.uint8), np.ascontiguousarray(want_side[side]).view(np.uint8)), (side, r)


# ---- host threads ---------------------------------------------------------------------------------------------------------------
def test_host_threads(engine, oracle):
    """Four host threads, each with a non-blocking stream and inputs of its own, share one keyswitch key, one N = 2048
    NTT bootstrap key and one f64 bootstrap key (and with them the scratch pool's mutex): released from a barrier, each
    makes eight calls of varying batch per entry and compares with the oracle (the f64 bootstrap: with the quiescent
    rows computed beforehand)."""
    import torch
    M, K, F = engine.ntt64_pbs, engine.lwe_keyswitch, engine.fft64
    g = H.rng(0x7EAD)
    threads, batches = 4, [3, 1, 5, 2, 7, 4, 8, 6]
    top = max(batches)
    in_dim, out_dim, ks_bl, ks_l = 40, 24, 4, 4
    n, k, base_log, level = 2048, 1, 23, 1
    ksk = H.uniform_u64(g, (in_dim, ks_l, out_dim + 1))
    ks_key = K.LweKeyswitchKey(SO.to_dev(ksk), ks_bl, ks_l)
    bsk = H.uniform_q(g, (N_LWE, level, k + 1, k + 1, n), P)
    ntt_key = M.NttBootstrapKey(engine.Plan.cached(n, P), SO.to_dev(bsk), base_log, level, M.SOLINAS)  # the sw scratch
    fft = F.Fft(n)
    fbsk = SO.to_dev(_fourier_of(engine, fft, H.uniform_u64(g, (N_LWE, level, k + 1, k + 1, n))))
    fft_key = F.FourierLweBootstrapKey(fbsk, base_log, level, fft)
    _, pbs = _pbs_want(oracle, n, k, base_log, level, False, 0)
    work = []
    for t in range(threads):
        big, small, lut = H.uniform_u64(g, (top, in_dim + 1)), H.uniform_q(g, (top, N_LWE + 1), P), H.uniform_q(g, (k + 1, n), P)
        d_big, d_small, d_lut = SO.to_dev(big), SO.to_dev(small), SO.to_dev(lut)
        quiet = zeros((top, k * n + 1))
        torch.cuda.synchronize()
        F.programmable_bootstrap_lwe_ciphertext(d_small, quiet, d_lut, fft_key)
        torch.cuda.synchronize()
        work.append(dict(big=d_big, small=d_small, lut=d_lut, stream=SO.stream(f"thread{t}"),
                         want_ks=oracle.lwe_keyswitch(ksk, big, out_dim, ks_bl, ks_l),
                         want_ntt=pbs(np.broadcast_to(lut, (top, k + 1, n)), small, bsk), want_fft=host(quiet),
                         outs=[(zeros((b, out_dim + 1)), zeros((b, k * n + 1)), zeros((b, k * n + 1))) for b in batches]))
    torch.cuda.synchronize()
    barrier = threading.Barrier(threads)
    errors = []

    def run(w):
        try:
            barrier.wait(timeout=60)
            with torch.cuda.stream(w["stream"]):
                for b, (o_ks, o_ntt, o_fft) in zip(batches, w["outs"]):
                    K.keyswitch_lwe_ciphertext(ks_key, w["big"][:b], o_ks)
                    M.programmable_bootstrap_ntt64_lwe_ciphertext_mem_optimized(w["small"][:b], o_ntt, w["lut"], ntt_key)
                    F.programmable_bootstrap_lwe_ciphertext(w["small"][:b], o_fft, w["lut"], fft_key)
            w["stream"].synchronize()
            for i, (b, (o_ks, o_ntt, o_fft)) in enumerate(zip(batches, w["outs"])):
                assert np.array_equal(host(o_ks), w["want_ks"][:b]), f"keyswitch, call {i}"
                assert np.array_equal(host(o_ntt), w["want_ntt"][:b]), f"NTT PBS, call {i}"
                assert np.array_equal(host(o_fft), w["want_fft"][:b]), f"f64 PBS, call {i}"
        except BaseException as e:  # noqa: BLE001  (reported by the main thread)
            errors.append(e)

    pool = [threading.Thread(target=run, args=(w,)) for w in work]
    for t in pool:
        t.start()
    for t in pool:
        t.join()
    torch.cuda.synchronize()
    assert not errors, errors
