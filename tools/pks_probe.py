#!/usr/bin/env python3
"""Throughput of the LWE packing keyswitch at the COMP_PARAM_MESSAGE_2_CARRY_2 shape (not a test).

2048 -> k = 4, N = 256, base 2^4, 3 levels, 256 ciphertexts per GLWE, 6,400 ciphertexts (25 GLWEs) per call, key and
inputs resident, HIP events on the launching stream around a loop of at least 0.3 s of GPU work, as bench.py's legs.

The call is digit pass + int8 GEMM + rotate-and-sum.  The LWE keyswitch 2048 -> 1279 with the same decomposition runs
the identical digit pass and GEMM (same depth, same 1,280 columns; only the body column and the rounding flag differ),
so it is timed beside the packing call: its time gives the GEMM's fraction of the int8 MFMA peak, computed as
bench.py's keyswitch leg does (all 8 recoded byte planes counted), and the difference of the two is the rotate-and-sum
pass, reported as the bytes it moves (the keyswitched rows read once, the GLWEs written, partial sums written and
read) per second against the HBM peak.  Compress + extract at 12 bits is timed too.  Prints one JSON line.
"""
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tfhe-rs-main_modified_amd"))

IN_DIM, K, N, BASE_LOG, LEVEL, PER, LOG_MODULUS = 2048, 4, 256, 4, 3, 256, 12
I8_PEAK_TOPS, HBM_PEAK_GBS, MIN_SECONDS = 5000.0, 8000.0, 0.3  # bench.py's constants


def timed(run, torch):
    """(steps, kernel ms per step): one untimed step sizes the loop to >= MIN_SECONDS, events bracket it."""
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
    return steps, e0.elapsed_time(e1) / steps


def main():
    import torch
    import tfhe_ntt_amd as eng

    n_lwe = int(sys.argv[1]) if len(sys.argv) > 1 else 6400
    P, KS = eng.lwe_packing_keyswitch, eng.lwe_keyswitch
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(device=dev))
    size = (K + 1) * N
    raw = torch.empty((IN_DIM, LEVEL, K + 1, N), dtype=torch.int64, device=dev)
    eng.fill_uniform(raw, 0x706b73, 0)
    pkey = P.LwePackingKeyswitchKey(raw, BASE_LOG, LEVEL)
    kkey = KS.LweKeyswitchKey(raw.view(IN_DIM, LEVEL, size), BASE_LOG, LEVEL)
    del raw
    lwe = torch.empty((n_lwe, IN_DIM + 1), dtype=torch.int64, device=dev)
    eng.fill_uniform(lwe, 0x706b74, 0)
    n_glwe = (n_lwe + PER - 1) // PER
    glwe = torch.empty((n_glwe, K + 1, N), dtype=torch.int64, device=dev)
    rows = torch.empty((n_lwe, size), dtype=torch.int64, device=dev)
    pack = lambda: P.keyswitch_lwe_ciphertext_list_and_pack_in_glwe_ciphertext(pkey, lwe, glwe, PER)
    steps, pack_ms = timed(pack, torch)
    _, gemm_ms = timed(lambda: KS.keyswitch_lwe_ciphertext(kkey, lwe, rows), torch)
    C = P.CompressedModulusSwitchedGlweCiphertext
    _, comp_ms = timed(lambda: C.compress(glwe, LOG_MODULUS, PER).extract(glwe), torch)
    ops = 2.0 * n_lwe * 8 * size * IN_DIM * LEVEL  # int8 MACs x 2 over the 8 byte planes
    rot_ms = max(pack_ms - gemm_ms, 1e-6)
    # slices of the d range (packing_keyswitch.hip pks_plan): ~1024 workgroups, slices of at least 8 rows
    blocks = n_glwe * ((size + 255) // 256)
    part = max(1, min(math.ceil(1024 / blocks), (PER + 7) // 8))
    part = math.ceil(PER / math.ceil(PER / part))
    rot_bytes = 8.0 * size * (n_lwe + n_glwe + (2 * n_glwe * part if part > 1 else 0))
    print(json.dumps({
        "probe": "pks_probe", "shape": {"in_dim": IN_DIM, "glwe_dim": K, "polynomial_size": N, "base_log": BASE_LOG,
                                        "level": LEVEL, "lwe_per_glwe": PER, "n_lwe": n_lwe},
        "steps": steps, "pack_ms": pack_ms, "ciphertexts_per_s": n_lwe / (pack_ms * 1e-3),
        "digits_gemm_ms": gemm_ms, "gemm_int8_tops": ops / (gemm_ms * 1e-3) / 1e12,
        "gemm_frac_of_int8_peak": ops / (gemm_ms * 1e-3) / 1e12 / I8_PEAK_TOPS,
        "rotate_sum_ms": rot_ms, "rotate_sum_slices": part, "rotate_sum_gbytes_per_s": rot_bytes / (rot_ms * 1e-3) / 1e9,
        "rotate_sum_frac_of_hbm_peak": rot_bytes / (rot_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
        "compress_extract_ms": comp_ms, "compress_log_modulus": LOG_MODULUS,
    }))


if __name__ == "__main__":
    main()
