"""The f64 <-> torus conversions of csrc/fft64_device.hpp on the device, bit for bit at their corners (`-m gpu`): the
real kernels are driven through the public API so that one coefficient sees an exactly known double (see
tests/torus_corners.py for the method, the contract in numbers and the map of device copies).

Every test runs on the one-wave engine (N = 2048), on the generic engine at N = 32, 64, 128 (the three radix remainders
of its row pass) and at N = 32768 (the smallest size with a column pass, R = 2).  Each also asserts the words the
transform must leave zero (or unchanged): that the transform added no rounding is checked, not assumed.
"""
import numpy as np
import pytest

import torus_corners as C

pytestmark = pytest.mark.gpu

ENGINES = [2048, 32, 64, 128, 32768]
ROWS = 256


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


def u64s(vals):
    return np.array([v % C.M64 for v in vals], dtype=np.uint64)


def chunks(seq):
    return [seq[i:i + ROWS] for i in range(0, len(seq), ROWS)]


@pytest.fixture(scope="module")
def forward_case():
    words = C.forward_words()
    want = np.array([C.ref_s64_to_f64(x) for x in words], np.float64) * 2.0 ** -64   # a power of two: exact
    return words, want


@pytest.fixture(scope="module")
def backward_case():
    vals = C.backward_values()
    shifted = vals[7:] + vals[:7]   # every value is seen by the real and by the imaginary part
    exp = {t: C.expected_backward(t) for t in vals}
    for t in vals:   # the contract of from_torus_scaled against the reference, class by class
        ref = C.ref_from_torus(t)
        if C.fract_is_plus_half(t):
            assert exp[t] == 1 << 63 and ref == (1 << 63) - 1
        elif C.is_half(t):
            assert exp[t] % 2 == 0 and C.word_distance(exp[t], ref) <= 1
        else:
            assert exp[t] == ref
    return vals, shifted, exp


@pytest.fixture(scope="module")
def add_case():
    vals = C.add_torus_values()
    return vals, {t: (C.add_torus_class(t), C.expected_add_torus(t), C.ref_from_torus(t)) for t in vals}


@pytest.mark.parametrize("n", ENGINES)
def test_forward_conversion_exact(engine, forward_case, n):
    """x at coefficient 0 (N/2): every frequency's real (imaginary) part is f64(i64(x)) 2^-64 bit for bit, the other
    part a zero (the sign of a zero is no part of the contract)."""
    import torch
    words, want = forward_case
    m = n // 2
    fft = engine.fft64.Fft(n)
    for pos, part in ((0, 0), (m, 1)):
        for lo in range(0, len(words), ROWS):
            w = words[lo:lo + ROWS]
            x = np.zeros((len(w), n), np.uint64)
            x[:, pos] = u64s(w)
            four = torch.full((len(w), m, 2), float("nan"), dtype=torch.float64, device="cuda")
            fft.forward_as_torus(four, dev(x))
            got = four.cpu().numpy()
            exp = np.broadcast_to(want[lo:lo + len(w), None], (len(w), m))
            bad = np.nonzero(got[..., part].view(np.int64) != exp.view(np.int64))
            assert bad[0].size == 0, (n, pos, hex(w[bad[0][0]]), got[bad[0][0], bad[1][0], part], exp[bad[0][0], 0])
            assert np.all(got[..., 1 - part] == 0.0), (n, pos)


@pytest.mark.parametrize("n", ENGINES)
def test_backward_conversion_exact(engine, backward_case, n):
    """A constant spectrum (t_re, t_im): coefficient 0 is from_torus(t_re), coefficient N/2 from_torus(t_im), every
    other word zero; stored, and added to the accumulators 0, 2^64 - 1 and 2^63 (wrapping)."""
    import torch
    vals, shifted, exp = backward_case
    m = n // 2
    fft = engine.fft64.Fft(n)
    for lo in range(0, len(vals), ROWS):
        tre, tim = vals[lo:lo + ROWS], shifted[lo:lo + ROWS]
        b = len(tre)
        c = torch.tensor(np.stack([tre, tim], axis=-1), dtype=torch.float64, device="cuda")
        four = c.view(b, 1, 2).expand(b, m, 2).contiguous()
        ere, eim = u64s([exp[t] for t in tre]), u64s([exp[t] for t in tim])
        for add, acc in ((False, 0x5A5A5A5A5A5A5A5A),) + tuple((True, a) for a in C.ACCUMULATORS):
            out = dev(np.full((b, n), acc, np.uint64))
            fft.backward_as_torus(out, four, add=add)
            got = host(out)
            base = np.uint64(acc if add else 0)
            with np.errstate(over="ignore"):
                want = np.full((b, n), base, np.uint64)
                want[:, 0] += ere
                want[:, m] += eim
            bad = np.nonzero(got != want)
            if bad[0].size:
                i, j = int(bad[0][0]), int(bad[1][0])
                t = tre[i] if j == 0 else tim[i] if j == m else None
                pytest.fail(f"N={n} add={add} acc={acc:#x} row {i} coefficient {j}: t={t!r} "
                            f"got {int(got[i, j]):#x} want {int(want[i, j]):#x} ({bad[0].size} words differ)")


@pytest.mark.parametrize("n", ENGINES)
def test_add_torus_contract(engine, add_case, n):
    """add_external_product_assign at level 1 with the digit polynomial 1 and the Fourier GGSW a constant c at
    [0, 0, w]: out[b, w, 0] += from_torus(c.re), out[b, w, N/2] += from_torus(c.im), every other word unchanged.
    Four values per call (w = 0, 1; re, im), the accumulators down the batch.  The device equals the host model bit
    for bit, and the contract of fft64_device.hpp in numbers: exact where it says exact, 2^32 below the reference on
    the dropped carry, within 2^11 elsewhere (2^10 outside the clamp, one unit on the rounded fraction)."""
    import torch
    vals, info = add_case
    m = n // 2
    base_log = 23
    fft = engine.fft64.Fft(n)
    accs = C.ACCUMULATORS + (0x00000000FFFFFFFF, 0x123456789ABCDEF0)
    bsz = len(accs)
    glwe = np.zeros((bsz, 2, n), np.uint64)
    glwe[:, 0, 0] = np.uint64(1 << (64 - base_log))
    glwe_d = dev(glwe)
    out0 = np.empty((bsz, 2, n), np.uint64)
    for b, a in enumerate(accs):
        out0[b] = np.uint64(a)
    vals = vals + vals[:(-len(vals)) % 4]
    failures = []
    for lo in range(0, len(vals), 4):
        quad = vals[lo:lo + 4]   # [w = 0 re, w = 0 im, w = 1 re, w = 1 im]
        fg = torch.zeros((1, 2, 2, m, 2), dtype=torch.float64, device="cuda")
        for w in range(2):
            fg[0, 0, w, :, 0] = quad[2 * w]
            fg[0, 0, w, :, 1] = quad[2 * w + 1]
        out = dev(out0)
        engine.fft64.add_external_product_assign(out, fg, glwe_d, base_log, 1, fft)
        got = host(out)
        touched = np.zeros((bsz, 2, n), bool)
        touched[:, :, 0] = touched[:, :, m] = True
        if not np.array_equal(got[~touched], out0[~touched]):
            failures.append((quad, "a word outside coefficients 0 and N/2 changed"))
            continue
        for q, t in enumerate(quad):
            w, pos = q // 2, (0 if q % 2 == 0 else m)
            cls, (word, slack), ref = info[t]
            for b, a in enumerate(accs):
                d = (int(got[b, w, pos]) - a) % C.M64
                why = None
                if (C.model_add_torus(a, t) - a) % C.M64 != d:
                    why = "differs from the host model"
                elif C.word_distance(d, word) > slack:
                    why = "outside the contract"
                elif cls == "carry" and (ref - d) % C.M64 != 1 << 32:
                    why = "carry class not 2^32 below the reference"
                elif cls != "carry" and C.word_distance(d, ref) > 1 << 11:
                    why = "more than 2^11 from the reference"
                elif cls == "exact" and d != ref:
                    why = "not exact"
                if why:
                    failures.append((t.hex(), cls, hex(a), hex(d), hex(word), slack, why))
    assert not failures, (n, len(failures), failures[:12])
