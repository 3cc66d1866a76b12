#!/usr/bin/env python3
"""Rate of the multi-bit PBS against the classic PBS on the f64-FFT path, in one process (not a test).

Batch 4096, k = 1, N = 2048, level 1, keys and inputs resident, HIP events on the launching stream around a loop of
at least 0.3 s of GPU work (as bench.py's legs), three repeats each:

  classic    mi_fft64_pbs_batch            n = 918, B = 2^23
  g = 4      mi_fft64_multi_bit_pbs_batch  n = 920, B = 2^22   (the GPU parameter sets' shape)
  g = 2      mi_fft64_multi_bit_pbs_batch  n = 920, B = 2^22
  g = 3      mi_fft64_multi_bit_pbs_batch  n = 918, B = 2^22

The keys are uniform random (the standard key filled on the device, then converted): the rate does not depend on key
content.  Prints one JSON object and, with --out FILE, writes it there too (profiles/multi_bit/probe.json).
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tfhe-rs-main_modified_amd"))

N, K, BATCH, MIN_SECONDS, REPEATS = 2048, 1, 4096, 0.3, 3


def timed(run, torch):
    """(steps, ms per call): one untimed call sizes the loop to >= MIN_SECONDS, events bracket it."""
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
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=BATCH)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import tfhe_ntt_amd as eng

    F = eng.fft64
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(device=dev))
    fft = F.Fft(N, 0)
    batch = args.batch

    def fourier(shape, seed):
        std = torch.empty(shape + (N,), dtype=torch.int64, device=dev)
        eng.fill_uniform(std, seed, 0)
        out = torch.empty(shape + (N // 2, 2), dtype=torch.float64, device=dev)
        F.convert_standard_lwe_bootstrap_key_to_fourier(std, out, fft)
        torch.cuda.synchronize()
        return out

    def inputs(n_lwe, seed):
        lwe = torch.empty((batch, n_lwe + 1), dtype=torch.int64, device=dev)
        eng.fill_uniform(lwe, seed, 0)
        return lwe

    lut = torch.empty((K + 1, N), dtype=torch.int64, device=dev)
    eng.fill_uniform(lut, 0x6d62, 0)
    out = torch.zeros((batch, K * N + 1), dtype=torch.int64, device=dev)
    legs = []

    def leg(name, n_lwe, base_log, g, run):
        ms = []
        for _ in range(REPEATS):
            steps, t = timed(run, torch)
            ms.append(t)
        best = min(ms)
        legs.append({"leg": name, "n_lwe": n_lwe, "base_log": base_log, "grouping_factor": g, "steps": steps,
                     "ms_per_batch": ms, "pbs_per_s": [batch / (t * 1e-3) for t in ms],
                     "spread": (max(ms) - best) / best})

    n_lwe, base_log = 918, 23
    key = F.FourierLweBootstrapKey(fourier((n_lwe, 1, K + 1, K + 1), 0x6d63), base_log, 1, fft)
    lwe = inputs(n_lwe, 0x6d64)
    leg("classic", n_lwe, base_log, 1, lambda: F.programmable_bootstrap_lwe_ciphertext(lwe, out, lut, key))
    del key
    for g, n_lwe in ((4, 920), (2, 920), (3, 918)):
        base_log = 22
        fbsk = fourier((n_lwe // g, 1 << g, 1, K + 1, K + 1), 0x6d70 + g)
        mkey = F.FourierLweMultiBitBootstrapKey(fbsk, base_log, 1, g, fft)
        lwe = inputs(n_lwe, 0x6d80 + g)
        leg(f"multi_bit_g{g}", n_lwe, base_log, g,
            lambda: F.multi_bit_programmable_bootstrap_lwe_ciphertext(lwe, out, lut, mkey))
        del mkey, fbsk
    torch.cuda.synchronize()

    by = {l["leg"]: l for l in legs}
    classic, g4 = min(by["classic"]["ms_per_batch"]), min(by["multi_bit_g4"]["ms_per_batch"])
    result = {"probe": "multi_bit_probe", "batch": batch, "polynomial_size": N, "glwe_dimension": K, "level": 1,
              "device": torch.cuda.get_device_name(0), "source_hash": eng._lib.build_provenance()["so_source_hash"],
              "legs": legs, "g4_over_classic_time": g4 / classic,
              "g4_no_slower_than_classic": bool(g4 <= classic * (1.0 + by["classic"]["spread"]))}
    text = json.dumps(result)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
