#!/usr/bin/env python3
"""Times of radix addition at the PARAM_MESSAGE_2_CARRY_2 shape (not a test).

n = 918, k = 1, N = 2048, PBS (23, 1) on the NTT engine (BNF), KS (4, 4), m = c = 4; with and without the drift key
(1449 encryptions of zero).  Load: mi_radix_add_batch on 64-bit integers (32 blocks) at 1, 16 and 128 integers per
call.  Keys and inputs are uniform words resident on the device (times do not depend on the values); HIP events on the
launching stream around a loop of at least 0.3 s of GPU work after one untimed call, as bench.py's legs.

Beside every addition, in the same process and taking turns with it: the keyswitch, drift and bootstrap calls of the
same rounds alone, on the same row counts (round 1: T keyswitches and 2 T bootstraps; the scan round at distance s:
I (32 - s) of each; the last round: T of each), so that the share the glue adds (index rules, packing, gathers, the
blockwise add and its staging copies, skipped items) reads off as 1 - baseline / add.

Also: the achieved fraction of HBM bandwidth of the linear-combination kernel at 4096 x 2049 words, two terms (two rows
read and one written per output row).

Writes profiles/radix/probe.json and prints it.
"""
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tfhe-rs-main_modified_amd"))

N_LWE, K, N = 918, 1, 2048
PBS, KS = (23, 1), (4, 4)
MSG = CARRY = 4
BLOCKS, INTEGERS = 32, (1, 16, 128)
ZEROS, MS_BOUND, MS_R_SIGMA, MS_VARIANCE = 1449, 288230376151711744.0, 13.179852282053789, 2.63039184094559e-7
HBM_PEAK_GBS, MIN_SECONDS = 8000.0, 0.3  # bench.py's constants


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
    """name -> (median ms, [every ms]), the calls taking turns."""
    got = {name: [] for name in runs}
    for _ in range(reps):
        for name, run in runs.items():
            got[name].append(timed(run, torch))
    return {name: (sorted(v)[len(v) // 2], v) for name, v in got.items()}


def main():
    import torch
    import tfhe_ntt_amd as eng

    M, KSW, NR, LA = eng.ntt64_pbs, eng.lwe_keyswitch, eng.modulus_switch_noise_reduction, eng.lwe_linear_algebra
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(device=dev))
    seed = [0x726478]

    def words(shape, p=0):
        t = torch.empty(shape, dtype=torch.int64, device=dev)
        seed[0] += 1
        eng.fill_uniform(t, seed[0], p)
        return t

    plan = eng.Plan.try_new(N, eng.SOLINAS_P)
    big1, small1 = K * N + 1, N_LWE + 1
    bsk = M.NttBootstrapKey(plan, words((N_LWE, PBS[1], K + 1, K + 1, N), eng.SOLINAS_P), *PBS, M.BNF)
    ksk = KSW.LweKeyswitchKey(words((K * N, KS[1], small1)), *KS)
    msk = NR.ModulusSwitchNoiseReductionKey(words((ZEROS, small1)), MS_BOUND, MS_R_SIGMA, MS_VARIANCE)
    luts = words((5, K + 1, N))
    res = {"probe": "radix_probe",
           "shape": {"n": N_LWE, "k": K, "N": N, "pbs": PBS, "ks": KS, "message_modulus": MSG, "carry_modulus": CARRY,
                     "blocks": BLOCKS, "bits": 64, "drift_zeros": ZEROS, "engine": "ntt64-bnf"}, "add": []}

    for drift in (False, True):
        sk = eng.shortint.ShortintServerKey(ksk, bsk, MSG, CARRY, msk if drift else None)
        server = eng.integer.ServerKey(sk)
        for n_int in INTEGERS:
            total = n_int * BLOCKS
            a = eng.integer.RadixCiphertext(words((n_int, BLOCKS, big1)), [MSG - 1] * BLOCKS)
            b = eng.integer.RadixCiphertext(words((n_int, BLOCKS, big1)), [MSG - 1] * BLOCKS)
            # the rounds: (keyswitched rows, bootstrapped rows)
            rounds = [(total, 2 * total)]
            s = 1
            while s < BLOCKS:
                rounds.append((n_int * (BLOCKS - s),) * 2)
                s *= 2
            rounds.append((total, total))
            big_in, small = words((2 * total, big1)), torch.empty((2 * total, small1), dtype=torch.int64, device=dev)
            sw, out = torch.empty_like(small), torch.empty((2 * total, big1), dtype=torch.int64, device=dev)
            idx = torch.arange(2 * total, dtype=torch.int32, device=dev) % 5
            # the bootstraps read buffers of their own: native words, or switched values in [0, 2 N) after the drift step
            pbs_in = words((2 * total, small1))
            if drift:
                pbs_in &= 2 * N - 1

            def baseline():
                for ks_rows, pbs_rows in rounds:
                    KSW.keyswitch_lwe_ciphertext(ksk, big_in[:ks_rows], small[:ks_rows])
                    mode = M.MS_STANDARD
                    if drift:
                        msk.improve_noise_and_modulus_switch(small[:ks_rows], sw[:ks_rows], 12)
                        mode = M.MS_PRE_SWITCHED
                    M.programmable_bootstrap_ntt64_bnf_lwe_ciphertext_mem_optimized(pbs_in[:pbs_rows], out[:pbs_rows],
                                                                                    luts, bsk, mode, idx[:pbs_rows])

            t = alternate({"add": lambda: server.add_parallelized(a, b), "baseline": baseline}, torch)
            add_ms, base_ms = t["add"][0], t["baseline"][0]
            res["add"].append({"drift": drift, "integers": n_int, "bootstrap_rounds": len(rounds),
                               "bootstraps": sum(r[1] for r in rounds), "keyswitches": sum(r[0] for r in rounds),
                               "ms_per_call": add_ms, "us_per_addition": add_ms * 1e3 / n_int,
                               "ks_drift_pbs_alone_ms": base_ms, "glue_share": 1.0 - base_ms / add_ms,
                               "runs_ms": {k: v[1] for k, v in t.items()}})

    rows, size = 4096, 2049
    src, dst = words((rows, size)), torch.empty((rows, size), dtype=torch.int64, device=dev)
    ar = torch.arange(rows, dtype=torch.int32, device=dev)
    index = torch.stack([ar, (ar * 7 + 1) % rows], dim=1).contiguous()
    coeff = torch.tensor([[MSG, 1]], dtype=torch.int64, device=dev).repeat(rows, 1).contiguous()
    lc_ms = timed(lambda: LA.lwe_linear_combination(dst, src, index, coeff), torch)
    moved = 3 * rows * size * 8
    res["linear_combination"] = {"rows": rows, "words": size, "terms": 2, "ms": lc_ms, "bytes_moved": moved,
                                 "gb_per_s": moved / (lc_ms * 1e-3) / 1e9,
                                 "frac_of_hbm_peak": moved / (lc_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                 "note": "two rows read and one written per output row; the 67 MB source fits the "
                                         "256 MB Infinity Cache, so reads may be served from it"}

    os.makedirs(os.path.join(ROOT, "profiles", "radix"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "radix", "probe.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
