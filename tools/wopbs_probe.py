#!/usr/bin/env python3
"""Times of the WoP-PBS stages at LEGACY_WOPBS_PARAM_MESSAGE_2_CARRY_2_KS_PBS (not a test).

shortint/parameters/parameters_wopbs_message_carry.rs:400-422: n = 769, k = 1, N = 2048, PBS (15, 2), KS (6, 2),
pfks (15, 2), cbs (5, 3).  Load: 64 evaluations of 8 input bits.  Keys and inputs are uniform words resident on the
device (times do not depend on the values); HIP events on the launching stream around a loop of at least 0.3 s of GPU
work after one untimed call, as bench.py's legs.  Every time is set beside an existing entry point run in the same
process:

* mi_lwe_pfpks_batch beside mi_lwe_packing_keyswitch_batch at the same GEMM depth and column count (in_dim 2049,
  k = 3, N = 2048: 8192 columns, one ciphertext per GLWE), and its fraction of the int8 peak (all 8 byte planes counted);
* the circuit bootstrap, and its three stages run through the public calls, beside mi_fft64_pbs_batch alone on the same
  number of bootstraps;
* the rotation (8 GGSWs per item) and a 3-layer tree beside the same CMUX counts through the shared-GGSW
  mi_fft64_cmux_batch;
* extract bits + circuit bootstrap + vertical packing per evaluation.

Writes profiles/wopbs/probe.json and prints it.
"""
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tfhe-rs-main_modified_amd"))

N_LWE, K, N = 769, 1, 2048
PBS, KS, PFKS, CBS = (15, 2), (6, 2), (15, 2), (5, 3)
EVALS, BITS = 64, 8
I8_PEAK_TOPS, MIN_SECONDS = 5000.0, 0.3  # bench.py's constants


def timed(run, torch):
    """kernel ms per call: one untimed call sizes the loop to >= MIN_SECONDS, events bracket it."""
    run()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run()
    torch.cuda.synchronize()
    steps = max(2, math.ceil(MIN_SECONDS / max(time.perf_counter() - t0, 1e-6)))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def alternate(runs, torch, reps=3):
    """Times the named calls `reps` times, taking turns (so that a drift of the clock or a neighbour's load hits every
    call alike): name -> (median ms, [every ms])."""
    got = {name: [] for name in runs}
    for _ in range(reps):
        for name, run in runs.items():
            got[name].append(timed(run, torch))
    return {name: (sorted(v)[len(v) // 2], v) for name, v in got.items()}


def main():
    import torch
    import tfhe_ntt_amd as eng

    X, KSW, PK, M = eng.fft64, eng.lwe_keyswitch, eng.lwe_packing_keyswitch, eng.lwe_wopbs
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(device=dev))
    seed = [0x776f70]

    def words(shape):
        t = torch.empty(shape, dtype=torch.int64, device=dev)
        seed[0] += 1
        eng.fill_uniform(t, seed[0], 0)
        return t

    def fourier(shape):  # uniform standard polynomials through forward_as_torus
        out = torch.zeros(shape[:-1] + (N // 2, 2), dtype=torch.float64, device=dev)
        fft.forward_as_torus(out, words(shape))
        return out

    fft = X.Fft(N)
    big, big1, small1 = K * N, K * N + 1, N_LWE + 1
    bsk = X.FourierLweBootstrapKey(fourier((N_LWE, PBS[1], K + 1, K + 1, N)), *PBS, fft)
    ksk = KSW.LweKeyswitchKey(words((big, KS[1], small1)), *KS)
    pfpksk = M.LwePrivateFunctionalPackingKeyswitchKeyList(words((K + 1, big1, PFKS[1], K + 1, N)), *PFKS)
    res = {"probe": "wopbs_probe", "shape": {"n": N_LWE, "k": K, "N": N, "pbs": PBS, "ks": KS, "pfks": PFKS, "cbs": CBS,
                                             "evaluations": EVALS, "input_bits": BITS}}

    # ---- the private functional packing keyswitch beside the packing keyswitch ----
    rows = EVALS * BITS * CBS[1]
    boot = words((rows, big1))
    ggsw_std = torch.empty((rows, K + 1, K + 1, N), dtype=torch.int64, device=dev)
    cols = (K + 1) * (K + 1) * N
    pkey = PK.LwePackingKeyswitchKey(words((big1, PFKS[1], cols // N, N)), *PFKS)
    plwe, pout = words((rows, big1 + 1)), torch.empty((rows, cols // N, N), dtype=torch.int64, device=dev)
    t = alternate({"pfpks": lambda: M.private_functional_keyswitch_lwe_ciphertext_into_glwe_ciphertext(pfpksk, ggsw_std, boot),
                   "pks": lambda: PK.keyswitch_lwe_ciphertext_list_and_pack_in_glwe_ciphertext(pkey, plwe, pout, 1)}, torch)
    pf_ms, pk_ms = t["pfpks"][0], t["pks"][0]
    nd = (PFKS[0] + 1 + 7) // 8
    ops = 2.0 * rows * 8 * cols * big1 * PFKS[1] * nd
    res["pfpks"] = {"rows": rows, "columns": cols, "depth_digits": big1 * PFKS[1] * nd, "ms": pf_ms,
                    "rows_per_s": rows / (pf_ms * 1e-3), "int8_tops": ops / (pf_ms * 1e-3) / 1e12,
                    "frac_of_int8_peak": ops / (pf_ms * 1e-3) / 1e12 / I8_PEAK_TOPS,
                    "packing_keyswitch_same_depth_and_columns_ms": pk_ms, "runs_ms": {k: v[1] for k, v in t.items()}}

    # ---- the circuit bootstrap and its stages beside the PBS alone ----
    n_in = EVALS * BITS
    bits = words((n_in, small1))
    four = torch.zeros((n_in, CBS[1], K + 1, K + 1, N // 2, 2), dtype=torch.float64, device=dev)
    lwes, lut, luts3 = words((rows, small1)), words((K + 1, N)), words((CBS[1], K + 1, N))
    lut_idx = torch.arange(rows, dtype=torch.int32, device=dev) % CBS[1]
    pbs_out = torch.empty((rows, big1), dtype=torch.int64, device=dev)
    t = alternate({"cbs": lambda: M.circuit_bootstrap_boolean(bsk, bits, 63, pfpksk, *CBS, None, four, fft),
                   "pbs": lambda: X.programmable_bootstrap_lwe_ciphertext(lwes, pbs_out, lut, bsk),
                   "pbs_lut_indexed": lambda: X.programmable_bootstrap_lwe_ciphertext(lwes, pbs_out, luts3, bsk,
                                                                                      lut_index=lut_idx)}, torch)
    cbs_ms, pbs_ms, pbs_idx_ms = t["cbs"][0], t["pbs"][0], t["pbs_lut_indexed"][0]
    four_ms = timed(lambda: X.convert_standard_lwe_bootstrap_key_to_fourier(
        ggsw_std.view(rows, 1, K + 1, K + 1, N), four.view(rows, 1, K + 1, K + 1, N // 2, 2), fft), torch)
    res["circuit_bootstrap"] = {"inputs": n_in, "bootstraps": rows, "ms": cbs_ms, "pbs_batch_alone_ms": pbs_ms,
                                "pbs_batch_lut_indexed_alone_ms": pbs_idx_ms, "pfpks_ms": pf_ms, "fourier_ms": four_ms,
                                "remainder_ms": cbs_ms - pbs_idx_ms - pf_ms - four_ms,  # shifts, constants, accumulators
                                "runs_ms": {k: v[1] for k, v in t.items()}}

    # ---- rotation and tree beside the same CMUX counts with one shared GGSW ----
    ggsw = four  # (EVALS * BITS, ...) = (EVALS, BITS, ...)
    lists = ggsw.view(EVALS, BITS, CBS[1], K + 1, K + 1, N // 2, 2)
    acc = words((EVALS, 1, K + 1, N))
    ct0, ct1 = words((EVALS, K + 1, N)), words((EVALS, K + 1, N))
    idx = torch.arange(EVALS, dtype=torch.int32, device=dev) * BITS
    flat = ggsw.view(EVALS * BITS, CBS[1], K + 1, K + 1, N // 2, 2)
    t = alternate({"rotation": lambda: M.blind_rotate_assign(acc, lists, *CBS, fft),
                   "cmux_shared": lambda: X.cmux_assign(ct0, ct1, ggsw[0], *CBS, fft),
                   "cmux_indexed": lambda: X.cmux_assign(ct0, ct1, flat, *CBS, fft, ggsw_index=idx)}, torch)
    rot_ms, one_ms, one_idx_ms = t["rotation"][0], t["cmux_shared"][0], t["cmux_indexed"][0]
    ggsw_bytes = CBS[1] * (K + 1) ** 2 * (N // 2) * 16
    res["rotation"] = {"items": EVALS, "ggsw_per_item": BITS, "cmuxes": EVALS * BITS, "ms": rot_ms,
                       "shared_cmux_batch_same_count_ms": BITS * one_ms, "cmux_batch_indexed_one_step_ms": one_idx_ms,
                       "cmux_batch_shared_one_step_ms": one_ms, "ggsw_bytes_per_item": ggsw_bytes,
                       "extra_ggsw_read_mb_per_step": (EVALS - 1) * ggsw_bytes / 1e6,
                       "runs_ms": {k: v[1] for k, v in t.items()}}
    r = 3
    luts = words((1, 1 << r, N))
    tree_out = torch.empty((EVALS, 1, K + 1, N), dtype=torch.int64, device=dev)
    tree_lists = lists[:, :r].contiguous()
    tree_ms = timed(lambda: M.cmux_tree_memory_optimized(tree_out, luts, tree_lists, *CBS, fft), torch)
    layer_ms = 0.0
    for j in range(r):
        items = EVALS << (r - 1 - j)
        a, b = words((items, K + 1, N)), words((items, K + 1, N))
        layer_ms += timed(lambda: X.cmux_assign(a, b, ggsw[0], *CBS, fft), torch)
    res["tree"] = {"items": EVALS, "layers": r, "cmuxes": EVALS * ((1 << r) - 1), "ms": tree_ms,
                   "shared_cmux_batch_same_counts_ms": layer_ms}

    # ---- end to end ----
    lwe_in = words((EVALS, big1))
    ext = torch.empty((EVALS, BITS, small1), dtype=torch.int64, device=dev)
    lut1 = words((1, 1, N))
    out = torch.empty((EVALS, 1, big1), dtype=torch.int64, device=dev)
    ext_ms = timed(lambda: M.extract_bits_from_lwe_ciphertext_mem_optimized(lwe_in, ext, bsk, ksk, 64 - BITS, BITS), torch)
    vp_ms = timed(lambda: M.circuit_bootstrap_boolean_vertical_packing_lwe_ciphertext_list_mem_optimized(
        ext, out, lut1, bsk, pfpksk, *CBS, fft), torch)
    res["end_to_end"] = {"evaluations": EVALS, "extract_bits_ms": ext_ms, "cbs_vertical_packing_ms": vp_ms,
                         "ms_per_evaluation": (ext_ms + vp_ms) / EVALS}

    os.makedirs(os.path.join(ROOT, "profiles", "wopbs"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "wopbs", "probe.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
