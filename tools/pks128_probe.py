#!/usr/bin/env python3
"""Cost of the 128-bit packing keyswitch and compression at the noise-squashing shape, in one process (not a test).

V1_4_NOISE_SQUASHING_COMP_PARAM_MESSAGE_2_CARRY_2_KS_PBS_TUNIFORM_2M128: in_dim 4096, k = 6, N = 1024, base 2^61, one
level, 128 ciphertexts per GLWE; 2048 ciphertexts (16 GLWEs) per call, key and inputs resident (filled by
mi_fill_uniform: the rate does not depend on their content), HIP events on the launching stream around a loop of at
least 0.3 s of GPU work, three repeats, the best kept.  It records

  pack        mi_lwe_packing_keyswitch128_batch at 128 per GLWE: digit pass + int8 GEMM mod 2^128 + rotate-and-sum.
  digits+GEMM there is no entry that stops after the GEMM.  The pack call runs it in four launches of 512 rows (the
              64 MiB cap on the rows in flight: four GLWEs' rows), so the single keyswitch (1 per GLWE) of 512
              ciphertexts is timed: the same digit pass and GEMM launch, then a rotate-and-sum pass that degenerates
              to one copy of the keyswitched rows; a device copy of that size, timed alone, is taken off and the
              rest counted four times.  rotate-and-sum = pack - (digits + GEMM).
  the GEMM's useful int8 op rate: rows * in_dim * level * pairs * (k + 1) N * 2 with pairs = sum_{s < nd} (16 - s)
              byte products per digit and key word (100 at nd = 8), against the 5 PF dense peak pks_probe.py uses.
  compress    mi_glwe_compress128_batch at log_modulus 128 of the 16 GLWEs (and extract).
  u64         the u64 packing keyswitch at pks_probe.py's shape and by its method, the yardstick of the GEMM rate.
  pbs128      mi_pbs128_batch of the same 2048 ciphertexts at its production shape (k = 2, N = 2048, base 2^24, 3
              levels, n = 918), the bootstrap whose outputs the packing consumes: pack + compress as a share of it.

Prints one JSON object and, with --out FILE, writes it there too (profiles/pks128/probe.json).
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tfhe-rs-main_modified_amd"))

IN_DIM, K, N, BASE_LOG, LEVEL, PER, N_LWE, LOG_MODULUS = 4096, 6, 1024, 61, 1, 128, 2048, 128
U64 = dict(in_dim=2048, k=4, n=256, base_log=4, level=3, per=256, n_lwe=6400)  # tools/pks_probe.py
PBS = dict(n=2048, k=2, base_log=24, level=3, n_lwe=918)                       # tools/pbs128_probe.py
I8_PEAK_TOPS, MIN_SECONDS, REPEATS = 5000.0, 0.3, 3


def timed(run, torch):
    """(calls, ms per call): one untimed call sizes the loop to >= MIN_SECONDS, events bracket it."""
    run()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run()
    torch.cuda.synchronize()
    calls = max(2, math.ceil(MIN_SECONDS / max(time.perf_counter() - t0, 1e-6)))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        run()
    e1.record()
    torch.cuda.synchronize()
    return calls, e0.elapsed_time(e1) / calls


def best(run, torch):
    runs = [timed(run, torch)[1] for _ in range(REPEATS)]
    return min(runs), runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import tfhe_ntt_amd as eng

    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(device=dev))

    def filled(shape, seed, p=0):
        t = torch.empty(shape, dtype=torch.int64, device=dev)
        eng.fill_uniform(t, seed, p)
        return t

    # ---- the 128-bit packing keyswitch and compression
    Q = eng.noise_squashing_compression
    size = (K + 1) * N
    raw = filled((IN_DIM, LEVEL, K + 1, N, 2), 0x706b3132)
    key = Q.LwePackingKeyswitchKey128(raw, BASE_LOG, LEVEL)
    del raw
    lwe = filled((N_LWE, IN_DIM + 1, 2), 0x706b3133)
    n_glwe = N_LWE // PER
    glwe = torch.empty((n_glwe, K + 1, N, 2), dtype=torch.int64, device=dev)
    launches, chunk = 4, N_LWE // 4  # the pack call's GEMM launches (pks_plan_rows: 64 MiB / (128 * 112 KiB) = 4 GLWEs)
    rows = torch.empty((chunk, K + 1, N, 2), dtype=torch.int64, device=dev)
    rows2 = torch.empty_like(rows)
    pack_ms, pack_runs = best(
        lambda: Q.keyswitch_lwe_ciphertext_list_and_pack_in_glwe_ciphertext(key, lwe, glwe, PER), torch)
    single_ms, single_runs = best(
        lambda: Q.keyswitch_lwe_ciphertext_into_glwe_ciphertext(key, lwe[:chunk], rows), torch)
    copy_ms, _ = best(lambda: rows2.copy_(rows), torch)
    C = Q.CompressedModulusSwitchedGlweCiphertext128
    comp_ms, _ = best(lambda: C.compress(glwe, LOG_MODULUS, PER), torch)
    ct = C.compress(glwe, LOG_MODULUS, PER)
    extract_ms, _ = best(lambda: ct.extract(glwe), torch)
    del rows, rows2
    nd = (BASE_LOG + 1 + 7) // 8
    pairs = sum(16 - s for s in range(nd))
    gemm_ms = launches * max(single_ms - copy_ms, 1e-6)
    ops = 2.0 * N_LWE * IN_DIM * LEVEL * pairs * size
    frac128 = ops / (gemm_ms * 1e-3) / 1e12 / I8_PEAK_TOPS

    # ---- the u64 packing keyswitch, by pks_probe.py's method
    P, KS = eng.lwe_packing_keyswitch, eng.lwe_keyswitch
    u = U64
    usize = (u["k"] + 1) * u["n"]
    raw = filled((u["in_dim"], u["level"], u["k"] + 1, u["n"]), 0x706b73)
    pkey = P.LwePackingKeyswitchKey(raw, u["base_log"], u["level"])
    kkey = KS.LweKeyswitchKey(raw.view(u["in_dim"], u["level"], usize), u["base_log"], u["level"])
    del raw
    ulwe = filled((u["n_lwe"], u["in_dim"] + 1), 0x706b74)
    uglwe = torch.empty(((u["n_lwe"] + u["per"] - 1) // u["per"], u["k"] + 1, u["n"]), dtype=torch.int64, device=dev)
    urows = torch.empty((u["n_lwe"], usize), dtype=torch.int64, device=dev)
    upack_ms, _ = best(
        lambda: P.keyswitch_lwe_ciphertext_list_and_pack_in_glwe_ciphertext(pkey, ulwe, uglwe, u["per"]), torch)
    ugemm_ms, _ = best(lambda: KS.keyswitch_lwe_ciphertext(kkey, ulwe, urows), torch)
    uops = 2.0 * u["n_lwe"] * 8 * usize * u["in_dim"] * u["level"]  # all 8 recoded byte planes, as bench.py counts
    frac64 = uops / (ugemm_ms * 1e-3) / 1e12 / I8_PEAK_TOPS
    del pkey, kkey, ulwe, uglwe, urows

    # ---- the bootstrap that produces the inputs
    M = eng.pbs128
    b = PBS
    plan = eng.Plan.cached(b["n"], eng.SOLINAS_P, 0)
    std = filled((b["n_lwe"], b["level"], b["k"] + 1, b["k"] + 1, b["n"], 2), 0x313238)
    bkey = M.LweBootstrapKey128(std, b["base_log"], b["level"], plan=plan)
    del std
    lut = filled((b["k"] + 1, b["n"], 2), 0x313239)
    blwe = filled((N_LWE, b["n_lwe"] + 1), 0x31323a)
    bout = torch.zeros((N_LWE, b["k"] * b["n"] + 1, 2), dtype=torch.int64, device=dev)
    pbs_ms, pbs_runs = best(
        lambda: M.programmable_bootstrap_f128_lwe_ciphertext(blwe, bout, lut, bkey, M.MS_CENTERED), torch)
    torch.cuda.synchronize()

    result = {
        "probe": "pks128_probe",
        "shape": {"in_dim": IN_DIM, "glwe_dim": K, "polynomial_size": N, "base_log": BASE_LOG, "level": LEVEL,
                  "lwe_per_glwe": PER, "n_lwe": N_LWE, "log_modulus": LOG_MODULUS},
        "device": torch.cuda.get_device_name(0), "source_hash": eng._lib.build_provenance()["so_source_hash"],
        "pack_ms": pack_ms, "pack_ms_runs": pack_runs, "ciphertexts_per_s": N_LWE / (pack_ms * 1e-3),
        "gemm_launches": launches, "single_keyswitch_rows": chunk, "single_keyswitch_ms": single_ms,
        "single_keyswitch_ms_runs": single_runs, "rows_copy_ms": copy_ms,
        "digits_gemm_ms": gemm_ms, "rotate_sum_ms": max(pack_ms - gemm_ms, 0.0),
        "digit_bytes": nd, "byte_pairs": pairs, "gemm_int8_tops": ops / (gemm_ms * 1e-3) / 1e12,
        "gemm_frac_of_int8_peak": frac128,
        "compress_ms": comp_ms, "extract_ms": extract_ms,
        "u64": {"shape": u, "pack_ms": upack_ms, "digits_gemm_ms": ugemm_ms,
                "gemm_int8_tops": uops / (ugemm_ms * 1e-3) / 1e12, "gemm_frac_of_int8_peak": frac64},
        "gemm_frac_over_u64_frac": frac128 / frac64,
        "pbs128": {"shape": b, "batch": N_LWE, "ms_per_batch": pbs_ms, "ms_per_batch_runs": pbs_runs},
        "pack_plus_compress_share_of_pbs128": (pack_ms + comp_ms) / pbs_ms,
    }
    text = json.dumps(result)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
