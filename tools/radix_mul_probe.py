#!/usr/bin/env python3
"""Times of radix multiplication at the PARAM_MESSAGE_2_CARRY_2 shape (not a test; no threshold).

n = 918, k = 1, N = 2048, PBS (23, 1) on the NTT engine (BNF), KS (4, 4), m = c = 4, no drift key.  Load:
mi_radix_mul_batch on 64-bit integers (32 blocks) at 1, 4 and 16 integers per call.  Keys and inputs are uniform words
resident on the device (times do not depend on the values); HIP events on the launching stream around a loop of at
least 0.3 s of GPU work after one untimed call, as tools/radix_probe.py and bench.py's legs; medians of three, the
calls taking turns in one process.

Beside every multiplication: the keyswitch and bootstrap calls of the same rounds alone, on the same row counts and in
the same passes (the product round: B (B + 1) / 2 keyswitches and B^2 bootstraps per integer; a round of the schedule:
one keyswitch per chunk, one bootstrap per message and carry; then the rounds of the full propagation), so that the
share the glue adds (index kernels, the staging copies, packing, chunk and block sums, gathers) reads off as
1 - baseline / mul; and mi_radix_add_batch on the same integers, for the ratio.

Writes profiles/radix_mul/probe.json and prints it.
"""
import ctypes
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
BLOCKS, INTEGERS = 32, (1, 4, 16)
MIN_SECONDS = 0.3


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


def mul_schedule(lib):
    """Per round of the multiplication's sum at BLOCKS blocks: (chunks, output rows) per integer."""
    first = list(range(BLOCKS)) + [j + 1 for j in range(BLOCKS - 1)]
    fb = (ctypes.c_uint32 * len(first))(*first)
    rounds = ctypes.c_size_t()
    assert lib.mi_radix_sum_schedule(BLOCKS, len(first), fb, MSG, CARRY, ctypes.byref(rounds), None, None, 0) == 0
    r = rounds.value
    lens, chunks = (ctypes.c_uint32 * ((r + 1) * BLOCKS))(), (ctypes.c_uint32 * (r * BLOCKS))()
    assert lib.mi_radix_sum_schedule(BLOCKS, len(first), fb, MSG, CARRY, ctypes.byref(rounds), lens, chunks, r) == 0
    out = []
    for i in range(r):
        q = list(chunks[i * BLOCKS:(i + 1) * BLOCKS])
        out.append((sum(q), 2 * sum(q) - q[-1]))  # no carry out of the last column
    return out


def main():
    import torch
    import tfhe_ntt_amd as eng

    M, KSW = eng.ntt64_pbs, eng.lwe_keyswitch
    lib = eng._lib.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(device=dev))
    seed = [0x726d75]

    def words(shape, p=0):
        t = torch.empty(shape, dtype=torch.int64, device=dev)
        seed[0] += 1
        eng.fill_uniform(t, seed[0], p)
        return t

    plan = eng.Plan.try_new(N, eng.SOLINAS_P)
    big1, small1 = K * N + 1, N_LWE + 1
    bsk = M.NttBootstrapKey(plan, words((N_LWE, PBS[1], K + 1, K + 1, N), eng.SOLINAS_P), *PBS, M.BNF)
    ksk = KSW.LweKeyswitchKey(words((K * N, KS[1], small1)), *KS)
    luts = words((7, K + 1, N))
    sk = eng.shortint.ShortintServerKey(ksk, bsk, MSG, CARRY, None)
    server = eng.integer.ServerKey(sk)
    sum_rounds = mul_schedule(lib)
    pairs = BLOCKS * (BLOCKS + 1) // 2
    # per integer: (keyswitched rows, bootstrapped rows) of every round of one multiplication
    per_int = [(pairs, BLOCKS * BLOCKS)] + sum_rounds + [(BLOCKS, 2 * BLOCKS)]
    scan = []  # the single-carry propagation that ends the full propagation: first round, scan rounds, last round
    s = 1
    while s < BLOCKS:
        scan.append((BLOCKS - s, BLOCKS - s))
        s *= 2
    per_int += [(BLOCKS, 2 * BLOCKS)] + scan + [(BLOCKS, BLOCKS)]
    res = {"probe": "radix_mul_probe",
           "shape": {"n": N_LWE, "k": K, "N": N, "pbs": PBS, "ks": KS, "message_modulus": MSG, "carry_modulus": CARRY,
                     "blocks": BLOCKS, "bits": 64, "engine": "ntt64-bnf", "drift": False},
           "per_integer": {"bootstraps": sum(r[1] for r in per_int), "keyswitches": sum(r[0] for r in per_int),
                           "bootstrap_rounds": len(per_int), "sum_rounds": len(sum_rounds),
                           "product_round": per_int[0], "sum_round_rows": sum_rounds},
           "mul": []}

    for n_int in INTEGERS:
        n = ctypes.c_size_t()
        assert lib.mi_radix_mul_pass_integers(sk._h, BLOCKS, n_int, ctypes.byref(n)) == 0
        passes = [min(n.value, n_int - i0) for i0 in range(0, n_int, n.value)]
        a = eng.integer.RadixCiphertext(words((n_int, BLOCKS, big1)), [MSG - 1] * BLOCKS)
        b = eng.integer.RadixCiphertext(words((n_int, BLOCKS, big1)), [MSG - 1] * BLOCKS)
        top = max(passes) * BLOCKS * BLOCKS
        big_in, small = words((top, big1)), torch.empty((top, small1), dtype=torch.int64, device=dev)
        out = torch.empty((top, big1), dtype=torch.int64, device=dev)
        idx = torch.arange(top, dtype=torch.int32, device=dev) % 7
        pbs_in = words((top, small1))

        def baseline():
            for ints in passes:
                for ks_rows, pbs_rows in per_int:
                    KSW.keyswitch_lwe_ciphertext(ksk, big_in[:ks_rows * ints], small[:ks_rows * ints])
                    M.programmable_bootstrap_ntt64_bnf_lwe_ciphertext_mem_optimized(
                        pbs_in[:pbs_rows * ints], out[:pbs_rows * ints], luts, bsk, M.MS_STANDARD, idx[:pbs_rows * ints])

        t = alternate({"mul": lambda: server.mul_parallelized(a, b), "baseline": baseline,
                       "add": lambda: server.add_parallelized(a, b)}, torch)
        mul_ms, base_ms, add_ms = t["mul"][0], t["baseline"][0], t["add"][0]
        res["mul"].append({"integers": n_int, "passes": passes, "ms_per_call": mul_ms,
                           "ms_per_multiplication": mul_ms / n_int, "ks_pbs_alone_ms": base_ms,
                           "glue_share": 1.0 - base_ms / mul_ms, "add_ms_per_call": add_ms,
                           "mul_over_add": mul_ms / add_ms, "bootstraps_per_second": res["per_integer"]["bootstraps"] *
                           n_int / (mul_ms * 1e-3), "runs_ms": {k: v[1] for k, v in t.items()}})

    os.makedirs(os.path.join(ROOT, "profiles", "radix_mul"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "radix_mul", "probe.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
