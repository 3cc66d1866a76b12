#!/usr/bin/env python3
"""Cost of the drift-technique modulus switch noise reduction in front of the classic PBS, in one process (not a test).

Batch 4096, n = 918, 1449 encryptions of zero, log modulus 12, bound / r_sigma / input variance of the reference's
TEST_PARAM (core_crypto/algorithms/test/modulus_switch_noise_reduction.rs:32-44); k = 1, N = 2048, level 1, B = 2^23.
Keys and inputs resident, HIP events on the launching stream around a loop of at least 0.3 s of GPU work (as bench.py's
legs), three repeats each:

  (a) improve_and_switch   mi_lwe_ms_noise_improve_and_switch_batch alone
  (b) pbs_standard         mi_fft64_pbs_batch with its on-device standard switch
  (c) improve_then_pbs     (a) followed by mi_fft64_pbs_batch at MI_MS_PRE_SWITCHED

The inputs and the zeros are uniform random words: the measure reads rounding errors of sums of mask words, which are
uniform for real encryptions too, so the candidates are walked as they would be (the walk is recorded).  The Fourier
key is uniform random as in tools/multi_bit_probe.py.  Condition: (c) <= 1.03 x (b).  Prints one JSON object and, with
--out FILE, writes it there too (profiles/ms_noise/probe.json).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tfhe-rs-main_modified_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from multi_bit_probe import REPEATS, timed  # noqa: E402

N, K, BATCH, N_LWE, ZEROS, LOG_MODULUS, BASE_LOG = 2048, 1, 4096, 918, 1449, 12, 23
BOUND, R_SIGMA, INPUT_VARIANCE = 288230376151711744.0, 13.179852282053789, 2.63039184094559e-7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=BATCH)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import tfhe_ntt_amd as eng

    F, MS = eng.fft64, eng.modulus_switch_noise_reduction
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(device=dev))
    fft = F.Fft(N, 0)
    batch = args.batch

    def uniform(shape, seed):
        t = torch.empty(shape, dtype=torch.int64, device=dev)
        eng.fill_uniform(t, seed, 0)
        return t

    std = uniform((N_LWE, 1, K + 1, K + 1, N), 0x6d63)
    fbsk = torch.empty((N_LWE, 1, K + 1, K + 1, N // 2, 2), dtype=torch.float64, device=dev)
    F.convert_standard_lwe_bootstrap_key_to_fourier(std, fbsk, fft)
    torch.cuda.synchronize()
    del std
    key = F.FourierLweBootstrapKey(fbsk, BASE_LOG, 1, fft)
    ms_key = MS.ModulusSwitchNoiseReductionKey(uniform((ZEROS, N_LWE + 1), 0x6d65), BOUND, R_SIGMA, INPUT_VARIANCE)
    lwe = uniform((batch, N_LWE + 1), 0x6d64)
    lut = uniform((K + 1, N), 0x6d62)
    switched = torch.zeros_like(lwe)
    out = torch.zeros((batch, K * N + 1), dtype=torch.int64, device=dev)

    def improve():
        ms_key.improve_noise_and_modulus_switch(lwe, switched, LOG_MODULUS)

    def pbs_standard():
        F.programmable_bootstrap_lwe_ciphertext(lwe, out, lut, key, F.MS_STANDARD)

    def improve_then_pbs():
        improve()
        F.programmable_bootstrap_lwe_ciphertext(switched, out, lut, key, F.MS_PRE_SWITCHED)

    legs = []
    for name, run in (("improve_and_switch", improve), ("pbs_standard", pbs_standard),
                      ("improve_then_pbs", improve_then_pbs)):
        ms = []
        for _ in range(REPEATS):
            steps, t = timed(run, torch)
            ms.append(t)
        legs.append({"leg": name, "steps": steps, "ms_per_batch": ms, "spread": (max(ms) - min(ms)) / min(ms)})

    cand, sat = MS.choose_candidate_to_improve_modulus_switch_noise_for_binary_key(ms_key, lwe, LOG_MODULUS)
    cand = cand.cpu()
    a, b, c = (min(leg["ms_per_batch"]) for leg in legs)
    result = {"probe": "ms_noise_probe", "batch": batch, "lwe_dimension": N_LWE, "zeros_count": ZEROS,
              "log_modulus": LOG_MODULUS, "polynomial_size": N, "glwe_dimension": K, "level": 1, "base_log": BASE_LOG,
              "device": torch.cuda.get_device_name(0), "source_hash": eng._lib.build_provenance()["so_source_hash"],
              "legs": legs,
              "walk": {"average_number_checks": float((cand + 2).double().mean()), "largest_index": int(cand.max()),
                       "within_first_tile": float((cand < 64).double().mean()),
                       "not_satisfied": int((sat == 0).sum())},
              "improve_share_of_pbs": a / b, "improve_then_pbs_over_pbs": c / b,
              "condition_c_le_1p03_b": bool(c <= 1.03 * b)}
    text = json.dumps(result)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
