#!/usr/bin/env python3
"""Rate of the multi-bit 128-bit PBS against the classic one, in one process (not a test).

Multi-bit: k = 2, N = 2048, base 2^23, 3 levels, grouping factor 4, n = 920
(V1_3_NOISE_SQUASHING_PARAM_GPU_MULTI_BIT_GROUP_4_MESSAGE_2_CARRY_2_KS_PBS_TUNIFORM_2M128); classic: base 2^24, n = 918
(tools/pbs128_probe.py's shape).  Keys filled by mi_fill_uniform (the rate does not depend on key content), batch 256 and
2048, keys and inputs resident, HIP events on the launching stream, each loop warmed and at least 0.3 s long, three
repeats.  Per batch it records:

  multi_bit    mi_pbs128_multi_bit_batch: PBS/s and ms per step (230 steps)
  classic      mi_pbs128_batch, standard switch: PBS/s and ms per CMUX step (918 steps)
  transforms   mi_ntt64_fwd_batch / mi_ntt64_inv_batch alone over the multi-bit step's transform count (per item and
               step R = 9 forward and (k + 1) n_limbs = 18 inverse), times the 230 steps
  the ratio multi-bit over classic (time per batch), and the multi-bit step over its transforms

and once the size of the two prepared keys and, with --resources FILE (the compiler's -Rpass-analysis=kernel-resource-usage
remarks of csrc/pbs128_multi_bit.hip), the registers and spills of the mac kernel at (k + 1, n_limbs, g) = (3, 6, 4).

Prints one JSON object and, with --out FILE, writes it there too (profiles/pbs128_multi_bit/probe.json).
"""
import argparse
import json
import math
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tfhe-rs-main_modified_amd"))

N, K, LEVEL = 2048, 2, 3
MB_BASE_LOG, G, MB_N_LWE = 23, 4, 920
CL_BASE_LOG, CL_N_LWE = 24, 918
BATCHES, MIN_SECONDS, REPEATS = (256, 2048), 0.3, 3
MAC_KERNEL = "multi_bit_macILi3ELi6ELi4ELb0EE"  # multi_bit_mac<3, 6, 4, false>


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


def mac_resources(path):
    """The resource remarks of the mac kernel: {"vgprs", "agprs", "sgprs", "vgpr_spill", "sgpr_spill",
    "scratch_bytes_per_lane", "occupancy_waves_per_simd"}."""
    text = open(path).read()
    at = text.find(MAC_KERNEL)
    if at < 0:
        return None
    nxt = text.find("Function Name:", at)
    block = text[at:nxt if nxt > 0 else len(text)]
    names = {"vgprs": r" VGPRs: (\d+)", "agprs": r"AGPRs: (\d+)", "sgprs": r"TotalSGPRs: (\d+)",
             "vgpr_spill": r"VGPRs Spill: (\d+)", "sgpr_spill": r"SGPRs Spill: (\d+)",
             "scratch_bytes_per_lane": r"ScratchSize \[bytes/lane\]: (\d+)",
             "occupancy_waves_per_simd": r"Occupancy \[waves/SIMD\]: (\d+)"}
    return {k: int(m.group(1)) for k, pat in names.items() if (m := re.search(pat, block))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--resources", default=None)
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

    std = filled((MB_N_LWE // G, 1 << G, LEVEL, K + 1, K + 1, N, 2), 0x6d6231)
    mb_key = M.LweMultiBitBootstrapKey128(std, MB_BASE_LOG, LEVEL, G, plan=plan)
    del std
    std = filled((CL_N_LWE, LEVEL, K + 1, K + 1, N, 2), 0x6d6232)
    cl_key = M.LweBootstrapKey128(std, CL_BASE_LOG, LEVEL, plan=plan)
    del std
    ggsw_bytes = lambda key: LEVEL * (K + 1) * (K + 1) * key.n_limbs * N * 8
    steps = MB_N_LWE // G
    rows, products = (K + 1) * LEVEL, (K + 1) * mb_key.n_limbs
    lut = filled((K + 1, N, 2), 0x6d6233)
    legs = []
    for batch in BATCHES:
        mb_lwe = filled((batch, MB_N_LWE + 1), 0x6d6234 + batch)
        cl_lwe = filled((batch, CL_N_LWE + 1), 0x6d6235 + batch)
        out = torch.zeros((batch, K * N + 1, 2), dtype=torch.int64, device=dev)
        fwd_buf = filled((batch * rows, N), 0x6d6236, eng.SOLINAS_P)  # canonical residues
        inv_buf = filled((batch * products, N), 0x6d6237, eng.SOLINAS_P)

        def run_multi_bit():
            M.multi_bit_programmable_bootstrap_f128_lwe_ciphertext(mb_lwe, out, lut, mb_key)

        def run_classic():
            M.programmable_bootstrap_f128_lwe_ciphertext(cl_lwe, out, lut, cl_key, M.MS_STANDARD)

        def run_transforms():  # one multi-bit step's transforms of the whole batch
            plan.fwd(fwd_buf)
            plan.inv(inv_buf)

        mb_ms, cl_ms, tr_ms = [], [], []
        for _ in range(REPEATS):
            mb_calls, t = timed(run_multi_bit, torch)
            mb_ms.append(t)
            cl_calls, t = timed(run_classic, torch)
            cl_ms.append(t)
            _, t = timed(run_transforms, torch)
            tr_ms.append(t * steps)  # the transform count of one multi-bit PBS call
        mb, cl, tr = min(mb_ms), min(cl_ms), min(tr_ms)
        legs.append({"batch": batch,
                     "multi_bit": {"calls": mb_calls, "ms_per_batch": mb_ms, "pbs_per_s": batch / (mb * 1e-3),
                                   "ms_per_step": mb / steps, "spread": (max(mb_ms) - mb) / mb},
                     "classic": {"calls": cl_calls, "ms_per_batch": cl_ms, "pbs_per_s": batch / (cl * 1e-3),
                                 "ms_per_cmux_step": cl / CL_N_LWE, "spread": (max(cl_ms) - cl) / cl},
                     "transforms_only": {"ms_per_batch": tr_ms, "ms_per_step": tr / steps,
                                         "spread": (max(tr_ms) - tr) / tr},
                     "multi_bit_over_classic_time": mb / cl, "multi_bit_over_transforms_time": mb / tr})
        del mb_lwe, cl_lwe, out, fwd_buf, inv_buf
    torch.cuda.synchronize()
    result = {"probe": "pbs128_multi_bit_probe", "polynomial_size": N, "glwe_dimension": K, "level": LEVEL,
              "multi_bit": {"base_log": MB_BASE_LOG, "grouping_factor": G, "n_lwe": MB_N_LWE, "steps": steps,
                            "limb_bits": mb_key.limb_bits, "n_limbs": mb_key.n_limbs,
                            "prepared_key_bytes": (steps << G) * ggsw_bytes(mb_key),
                            "group_bytes": ggsw_bytes(mb_key) << G},
              "classic": {"base_log": CL_BASE_LOG, "n_lwe": CL_N_LWE, "limb_bits": cl_key.limb_bits,
                          "n_limbs": cl_key.n_limbs, "prepared_key_bytes": CL_N_LWE * ggsw_bytes(cl_key)},
              "forward_per_item_step": rows, "inverse_per_item_step": products,
              "mac_kernel": "multi_bit_mac<3, 6, 4, false>",
              "mac_resources": mac_resources(args.resources) if args.resources else None,
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
