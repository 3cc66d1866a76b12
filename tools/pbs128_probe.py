#!/usr/bin/env python3
"""Rate of the exact 128-bit PBS at the noise-squashing shape, against its transform floor, in one process (not a test).

k = 2, N = 2048, base 2^24, 3 levels, n = 918 (V1_4_NOISE_SQUASHING_PARAM_MESSAGE_2_CARRY_2_KS_PBS_TUNIFORM_2M128), the
key filled by mi_fill_uniform (the rate does not depend on key content), batch 256 and 2048, keys and inputs resident,
HIP events on the launching stream, three repeats each.  Per batch it records:

  pbs          mi_pbs128_batch: PBS/s and ms per CMUX step
  transforms   mi_ntt64_fwd_batch / mi_ntt64_inv_batch alone over the same transform count (per item and step
               R = 9 forward and (k + 1) n_limbs = 18 inverse), times n: the floor this design cannot beat
  the ratio of the two (what the three streaming passes cost), and the bytes the five passes move per item and step by
  the model below, as a fraction of 8 TB/s at the measured step time.

Prints one JSON object and, with --out FILE, writes it there too (profiles/pbs128/probe.json).
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tfhe-rs-main_modified_amd"))

N, K, BASE_LOG, LEVEL, N_LWE = 2048, 2, 24, 3, 918
BATCHES, MIN_SECONDS, REPEATS, HBM_BYTES_PER_S = (256, 2048), 0.3, 3, 8e12


def timed(run, torch):
    """(calls, ms per call): one untimed call sizes the loop to >= MIN_SECONDS, events bracket it."""
    run()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run()
    torch.cuda.synchronize()
    calls = max(1, math.ceil(MIN_SECONDS / max(time.perf_counter() - t0, 1e-6)))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        run()
    e1.record()
    torch.cuda.synchronize()
    return calls, e0.elapsed_time(e1) / calls


def step_bytes(n_limbs):
    """HBM bytes one item moves in one CMUX step through the five passes (the step's GGSW, shared by the chunk and
    re-read from cache, left out): the u128 accumulator is read by the decomposition and read and written by the
    recombination; the R digit polynomials are written, transformed in place and read by the mac; the (k + 1) n_limbs
    limb products are written, transformed in place and read back."""
    kp1, rows = K + 1, (K + 1) * LEVEL
    acc = 3 * kp1 * N * 16
    digits = 4 * rows * N * 8
    products = 4 * kp1 * n_limbs * N * 8
    return acc + digits + products


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import tfhe_ntt_amd as eng

    M = eng.pbs128
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(device=dev))
    plan = eng.Plan.cached(N, eng.SOLINAS_P, 0)

    def filled(shape, seed, p=0):
        t = torch.empty(shape, dtype=torch.int64, device=dev)
        eng.fill_uniform(t, seed, p)
        return t

    std = filled((N_LWE, LEVEL, K + 1, K + 1, N, 2), 0x313238)
    key = M.LweBootstrapKey128(std, BASE_LOG, LEVEL, plan=plan)
    del std
    rows, products = (K + 1) * LEVEL, (K + 1) * key.n_limbs
    lut = filled((K + 1, N, 2), 0x313239)
    legs = []
    for batch in BATCHES:
        lwe = filled((batch, N_LWE + 1), 0x31323a + batch)
        out = torch.zeros((batch, K * N + 1, 2), dtype=torch.int64, device=dev)
        # canonical residues, as the transforms' domain asks
        fwd_buf = filled((batch * rows, N), 0x31323b, eng.SOLINAS_P)
        inv_buf = filled((batch * products, N), 0x31323c, eng.SOLINAS_P)

        def run_pbs():
            M.programmable_bootstrap_f128_lwe_ciphertext(lwe, out, lut, key, M.MS_CENTERED)

        def run_transforms():  # one step's transforms of the whole batch
            plan.fwd(fwd_buf)
            plan.inv(inv_buf)

        pbs_ms, tr_ms = [], []
        for _ in range(REPEATS):
            calls, t = timed(run_pbs, torch)
            pbs_ms.append(t)
            tr_calls, t = timed(run_transforms, torch)
            tr_ms.append(t * N_LWE)  # the same transform count as one PBS call
        best, floor = min(pbs_ms), min(tr_ms)
        step_s = best * 1e-3 / N_LWE
        moved = step_bytes(key.n_limbs)
        legs.append({"batch": batch, "calls": calls, "ms_per_batch": pbs_ms,
                     "pbs_per_s": [batch / (t * 1e-3) for t in pbs_ms], "spread": (max(pbs_ms) - best) / best,
                     "ms_per_cmux_step": best / N_LWE,
                     "transforms_only_ms_per_batch": tr_ms, "transforms_only_pbs_per_s": batch / (floor * 1e-3),
                     "transforms_spread": (max(tr_ms) - floor) / floor, "pbs_over_transforms_time": best / floor,
                     "model_bytes_per_item_step": moved,
                     "model_fraction_of_8_tb_per_s": moved * batch / step_s / HBM_BYTES_PER_S})
        del lwe, out, fwd_buf, inv_buf
    torch.cuda.synchronize()
    result = {"probe": "pbs128_probe", "polynomial_size": N, "glwe_dimension": K, "base_log": BASE_LOG,
              "level": LEVEL, "n_lwe": N_LWE, "limb_bits": key.limb_bits, "n_limbs": key.n_limbs,
              "forward_per_item_step": rows, "inverse_per_item_step": products,
              "device": torch.cuda.get_device_name(0), "source_hash": eng._lib.build_provenance()["so_source_hash"],
              "legs": legs}
    text = json.dumps(result)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
