"""GPU parity of mi_lwe_linear_combination_batch and the lwe_linear_algebra mirror against numpy wrapping u64 arithmetic
(`-m gpu`), bit for bit.  Shapes: lwe_dim 1 and 7 (rows shorter than a wave), 918 (the small LWE of 2_2: four chunks of
256 words, the last ragged) and 2048 (the big LWE: nine chunks, one word in the last); 0 to 3 terms; indices out of range;
coefficients -1 and INT64_MIN; more outputs than inputs; a NULL plaintext; more rows than the grid's cap."""
import numpy as np
import pytest

import tfhe_helpers as H

pytestmark = pytest.mark.gpu

INT64_MIN = -(1 << 63)


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype)
    return torch.from_numpy(a.view(view) if view else a).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


def reference(lwe_in, index, coeff, plaintext, n_out, size):
    out = np.zeros((n_out, size), np.uint64)
    with np.errstate(over="ignore"):
        for i in range(n_out):
            for t in range(index.shape[1]):
                if index[i, t] < lwe_in.shape[0]:
                    c = np.uint64(1) if coeff is None else np.uint64(int(coeff[i, t]) % 2**64)
                    out[i] += c * lwe_in[index[i, t]]
            if plaintext is not None:
                out[i, -1] += plaintext[i]
    return out


@pytest.mark.parametrize("lwe_dim", [1, 7, 918, 2048])
@pytest.mark.parametrize("terms", [0, 1, 2, 3])
def test_linear_combination_matches_numpy(engine, lwe_dim, terms):
    import torch
    LA = engine.lwe_linear_algebra
    g = H.rng(0x11a0 + 4 * lwe_dim + terms)
    n_in, n_out, size = 5, 13, lwe_dim + 1  # n_out > n_in
    lwe_in = H.uniform_u64(g, (n_in, size))
    index = g.integers(0, n_in + 2, size=(n_out, terms), dtype=np.uint32)  # n_in and n_in + 1 are out of range
    if terms:
        index[0, 0] = 0xFFFFFFFF
        index[1, :] = n_in  # every term of the row dropped: a trivial ciphertext
    coeff = g.integers(-8, 9, size=(n_out, terms), dtype=np.int64)
    coeff.reshape(-1)[::3] = -1
    coeff.reshape(-1)[1::5] = INT64_MIN
    plaintext = H.uniform_u64(g, n_out)
    for cf in (coeff, None):
        for pt in (plaintext, None):
            out = torch.full((n_out, size), 0x5E, dtype=torch.int64, device="cuda")
            LA.lwe_linear_combination(out, dev(lwe_in) if terms else None, dev(index) if terms else None,
                                      dev(cf) if cf is not None and terms else None, dev(pt) if pt is not None else None)
            assert np.array_equal(host(out), reference(lwe_in, index, cf, pt, n_out, size)), (cf is None, pt is None)


def test_more_rows_than_the_grid(engine):
    """4100 x 9 tiles at lwe_dim 2048 is more than the 4096 workgroups the launch is capped at: the stride loop."""
    import torch
    LA = engine.lwe_linear_algebra
    g = H.rng(0x11b0)
    n_in, n_out, size = 3, 4100 // 9 + 20, 2049
    lwe_in = H.uniform_u64(g, (n_in, size))
    index = g.integers(0, n_in, size=(n_out, 2), dtype=np.uint32)
    coeff = g.integers(-3, 4, size=(n_out, 2), dtype=np.int64)
    out = torch.zeros((n_out, size), dtype=torch.int64, device="cuda")
    LA.lwe_linear_combination(out, dev(lwe_in), dev(index), dev(coeff))
    assert np.array_equal(host(out), reference(lwe_in, index, coeff, None, n_out, size))


def test_overlap_and_empty_batch(engine):
    import torch
    LA = engine.lwe_linear_algebra
    buf = torch.zeros((4, 8), dtype=torch.int64, device="cuda")
    idx = torch.zeros((2, 1), dtype=torch.int32, device="cuda")
    with pytest.raises(engine.MiError) as e:
        LA.lwe_linear_combination(buf[1:3], buf[0:2], idx)
    assert e.value.status == 1 and "overlaps" in str(e.value)
    LA.lwe_linear_combination(buf[2:4], buf[0:2], idx)  # disjoint halves of one tensor
    LA.lwe_linear_combination(buf[0:0], buf[0:2], idx[0:0])  # n_out = 0
    with pytest.raises(ValueError):
        LA.lwe_linear_combination(buf[2:4], buf[0:2, :7], idx)


def test_mirrored_reference_functions(engine):
    """Every function of lwe_linear_algebra.rs that the mirror carries, over a batch, against wrapping numpy."""
    import torch
    LA = engine.lwe_linear_algebra
    g = H.rng(0x11c0)
    a, b = H.uniform_u64(g, (2, 3, 919)), H.uniform_u64(g, (2, 3, 919))
    scal = g.integers(-5, 6, size=6, dtype=np.int64)
    pts = H.uniform_u64(g, 6)
    body = lambda x, p: np.concatenate([x[..., :-1], (x[..., -1] + p.reshape(x.shape[:-1]))[..., None]], axis=-1)
    with np.errstate(over="ignore"):
        out = torch.zeros((2, 3, 919), dtype=torch.int64, device="cuda")
        LA.lwe_ciphertext_add(out, dev(a), dev(b))
        assert np.array_equal(host(out), a + b)
        LA.lwe_ciphertext_sub(out, dev(a), dev(b))
        assert np.array_equal(host(out), a - b)
        LA.lwe_ciphertext_cleartext_mul(out, dev(a), 7)
        assert np.array_equal(host(out), a * np.uint64(7))
        LA.lwe_ciphertext_cleartext_mul(out, dev(a), dev(scal))
        assert np.array_equal(host(out), a * scal.astype(np.uint64).reshape(2, 3, 1))
        t = dev(a)
        LA.lwe_ciphertext_add_assign(t, dev(b))
        assert np.array_equal(host(t), a + b)
        t = dev(a)
        LA.lwe_ciphertext_sub_assign(t, dev(b))
        assert np.array_equal(host(t), a - b)
        t = dev(a)
        LA.lwe_ciphertext_opposite_assign(t)
        assert np.array_equal(host(t), np.uint64(0) - a)
        t = dev(a)
        LA.lwe_ciphertext_cleartext_mul_assign(t, INT64_MIN)
        assert np.array_equal(host(t), a * np.uint64(1 << 63))
        t = dev(a)
        LA.lwe_ciphertext_plaintext_add_assign(t, dev(pts))
        assert np.array_equal(host(t), body(a, pts))
        t = dev(a)
        LA.lwe_ciphertext_plaintext_sub_assign(t, dev(pts))
        assert np.array_equal(host(t), body(a, np.uint64(0) - pts))
        t = dev(a)
        LA.lwe_ciphertext_plaintext_add_assign(t, (1 << 64) - 3)
        assert np.array_equal(host(t), body(a, np.full(6, (1 << 64) - 3, np.uint64)))
    with pytest.raises(ValueError):
        LA.lwe_ciphertext_add(out, dev(a), dev(b[:1]))
