"""The f64-FFT engines' accuracy against a high-precision reference (`-m gpu`; the helper is tests/fft_accuracy.py).

For identical inputs the error of the numpy restatement (oracle/fft_oracle.py) and the error of the GPU result are both
taken against the long-double spectrum or the exact integers, as rms and max normalised by the rms of the true result;
the GPU may be at most 4 times worse in either (why 4: tests/fft_accuracy.py).  tests/test_fft_accuracy.py shows that
this bar rejects table errors 100 times below what the 1e-13 max|want| bar of tests/test_fft_gpu.py lets through.

Sizes: the one-wave engine (N = 2048); the generic engine at N = 32, 64, 128 (its row pass's three radix remainders)
and N = 32768 .. 262144 (the column pass with R = 2, 4, 8, 16).  Every measured pair is printed (`-s`); DESIGN.md holds
the table of the first run.
"""
import numpy as np
import pytest

import fft_accuracy as A
import fft_oracle as F
import tfhe_helpers as H

pytestmark = pytest.mark.gpu

SIZES = [2048, 32, 64, 128, 32768, 65536, 131072, 262144]


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


def fdev(z):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.stack([z.real, z.imag], axis=-1))).cuda()


def from_engine(t, order):
    a = t.cpu().numpy()
    z = a[..., 0] + 1j * a[..., 1]
    out = np.empty_like(z)
    out[..., order] = z
    return out


def report(what, n, ref, gpu):
    r = A.ratios(gpu, ref)
    print(f"\n{what:<28} N={n:<6} numpy rms {ref[0]:.2e} max {ref[1]:.2e} | gpu rms {gpu[0]:.2e} max {gpu[1]:.2e} | "
          f"gpu/numpy rms {r[0]:.2f} max {r[1]:.2f}", end="")
    return r


@pytest.mark.parametrize("n", SIZES)
def test_transform_accuracy(engine, n):
    """forward_as_torus against the long-double spectrum; backward_as_torus, fed that spectrum rounded to f64, against
    the integers it came from; the GPU round trip against the integers."""
    import torch
    m = n // 2
    batch = 8 if n <= 128 else 4 if n <= 32768 else 2
    fft = engine.fft64.Fft(n)
    order = fft.fourier_order().astype(np.int64)
    x = H.uniform_u64(H.rng(9000 + n), (batch, n))
    true = A.forward_as_torus_ld(x)
    failed = []

    four = torch.zeros((batch, m, 2), dtype=torch.float64, device="cuda")
    fft.forward_as_torus(four, dev(x))
    ref = A.error_stats(F.forward_as_torus(x), true)
    gpu = A.error_stats(from_engine(four, order), true)
    report("forward_as_torus", n, ref, gpu)
    if not A.within_margin(gpu, ref):
        failed.append("forward")

    spec = true.astype(np.complex128)
    out = torch.zeros((batch, n), dtype=torch.int64, device="cuda")
    fft.backward_as_torus(out, fdev(spec[..., order]))
    ref = A.word_error_stats(F.backward_as_torus(spec), x)
    gpu = A.word_error_stats(host(out), x)
    report("backward_as_torus", n, ref, gpu)
    if not A.within_margin(gpu, ref):
        failed.append("backward")

    back = torch.zeros((batch, n), dtype=torch.int64, device="cuda")
    fft.backward_as_torus(back, four)
    ref = A.word_error_stats(F.backward_as_torus(F.forward_as_torus(x)), x)
    gpu = A.word_error_stats(host(back), x)
    report("round trip", n, ref, gpu)
    if not A.within_margin(gpu, ref):
        failed.append("round trip")
    assert not failed, (n, failed)


@pytest.mark.parametrize("n,k,base_log,level", [(2048, 1, 23, 1), (2048, 1, 10, 2), (2048, 2, 8, 3), (32, 1, 10, 2),
                                                (128, 1, 10, 2), (32768, 1, 10, 2)])
def test_external_product_accuracy(engine, oracle, n, k, base_log, level):
    """add_external_product_assign against the exact integer product, next to the restatement's external product on the
    same inputs (each through its own forward transform of the same standard GGSW)."""
    import torch
    m = n // 2
    batch = 2
    fft = engine.fft64.Fft(n)
    g = H.rng(9500 + n + 10 * k + base_log)
    ggsw = H.uniform_u64(g, (level, k + 1, k + 1, n))
    glwe = H.uniform_u64(g, (batch, k + 1, n))
    fg = torch.zeros((level, k + 1, k + 1, m, 2), dtype=torch.float64, device="cuda")
    fft.forward_as_torus(fg, dev(ggsw))
    out = dev(np.zeros((batch, k + 1, n), np.uint64))
    engine.fft64.add_external_product_assign(out, fg, dev(glwe), base_log, level, fft)
    got = host(out)
    want = np.stack([A.exact_ext_product(oracle, glwe[b], ggsw, base_log, level) for b in range(batch)])
    rest = F.external_product(glwe, F.forward_as_torus(ggsw), base_log, level)
    ref, gpu = A.word_error_stats(rest, want), A.word_error_stats(got, want)
    report(f"ext product k={k} B={base_log} l={level}", n, ref, gpu)
    rb, gb = A.word_error_bits(rest, want), A.word_error_bits(got, want)
    print(f" | error bits numpy rms {rb[0]:.1f} max {rb[1]:.1f}, gpu rms {gb[0]:.1f} max {gb[1]:.1f}", end="")
    assert A.within_margin(gpu, ref), (n, k, base_log, level, A.ratios(gpu, ref))
