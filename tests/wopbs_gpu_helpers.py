"""What the WoP-PBS GPU tests share (tests/test_wopbs_gpu.py, tests/test_wopbs_corners_gpu.py): device tensors, the
device keys of a shape, and every composite restated as the sequence of public stages it is defined as.  The references
themselves are in tests/wopbs_helpers.py."""
import functools

import numpy as np

import tfhe_helpers as H
import wopbs_helpers as W


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()


def idev(a):
    import torch
    return torch.tensor(list(a), dtype=torch.int32, device="cuda")


def host(t):
    return t.cpu().numpy().view(np.uint64)


def zeros(shape, fill=0):
    import torch
    return torch.full(shape, fill, dtype=torch.int64, device="cuda")


def fzeros(shape):
    import torch
    return torch.zeros(shape, dtype=torch.float64, device="cuda")


def same(a, b):
    import torch
    return bool(torch.equal(a, b))


def device_uniform(shape, seed):
    """Uniform 64-bit words drawn on the device (two 32-bit halves), for inputs too large to draw on the host."""
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    out = torch.randint(0, 1 << 32, shape, dtype=torch.int64, device="cuda", generator=g)
    out <<= 32
    out |= torch.randint(0, 1 << 32, shape, dtype=torch.int64, device="cuda", generator=g)
    return out


@functools.lru_cache(maxsize=None)
def device_keys(engine, shape, real):
    """The device keys of a shape: seeded encryptions (decryption tests) or uniform words (the structure tests compare
    bits only, and the N = 2048 keys would take minutes to encrypt on the host)."""
    X, KS, M = engine.fft64, engine.lwe_keyswitch, engine.lwe_wopbs
    big = shape.k * shape.N
    if real:
        ks = W.keys(shape)
        bsk, ksk, pf = ks["bsk"], ks["ksk"], ks["pfpksk"]
    else:
        g = H.rng(shape.seed + 7)
        bsk = H.uniform_u64(g, (shape.n, shape.pbs[1], shape.k + 1, shape.k + 1, shape.N))
        ksk = H.uniform_u64(g, (big, shape.ks[1], shape.n + 1))
        pf = H.uniform_u64(g, (shape.k + 1, big + 1, shape.pfks[1], shape.k + 1, shape.N))
    fft = X.Fft(shape.N)
    fbsk = fzeros(bsk.shape[:-1] + (shape.N // 2, 2))
    X.convert_standard_lwe_bootstrap_key_to_fourier(dev(bsk), fbsk, fft)
    return {"fft": fft, "bsk": X.FourierLweBootstrapKey(fbsk, *shape.pbs, fft),
            "ksk": KS.LweKeyswitchKey(dev(ksk), *shape.ks),
            "pfpksk": M.LwePrivateFunctionalPackingKeyswitchKeyList(dev(pf), *shape.pfks)}


def random_fourier_ggsws(engine, shape, batch, count, seed, on_device=False):
    """(batch, count, level_cbs, k+1, k+1, N/2, 2): distinct GGSWs per item (uniform words, transformed)."""
    fft = engine.fft64.Fft(shape.N)
    level = shape.cbs[1]
    dims = (batch, count, level, shape.k + 1, shape.k + 1, shape.N)
    out = fzeros(dims[:-1] + (shape.N // 2, 2))
    if count:
        fft.forward_as_torus(out, device_uniform(dims, seed) if on_device else dev(H.uniform_u64(H.rng(seed), dims)))
    return out


def trivial(luts, k):
    """(..., N) polynomials as trivial GLWEs (..., k+1, N)."""
    import torch
    out = torch.zeros(luts.shape[:-1] + (k + 1, luts.shape[-1]), dtype=luts.dtype, device=luts.device)
    out[..., k, :] = luts
    return out


def tree_by_layers(engine, shape, luts, ggsw, batch):
    """The layered mi_fft64_cmux_batch_indexed loop: luts (n_out, 2^r, N) device, ggsw (batch, r, ...) -> (batch, n_out,
    k+1, N)."""
    import torch
    X = engine.fft64
    r, k, n = int(ggsw.shape[1]), shape.k, shape.N
    n_out = int(luts.shape[0])
    nodes = trivial(luts, k).unsqueeze(0).repeat(batch, 1, 1, 1, 1)  # (batch, n_out, 2^r, k+1, N)
    items = torch.arange(batch, dtype=torch.int32, device="cuda")
    for j in range(r):
        t0, t1 = nodes[:, :, 0::2].contiguous(), nodes[:, :, 1::2].contiguous()
        per_item = t0.shape[2]
        index = (items * r + (r - 1 - j)).repeat_interleave(n_out * per_item)  # item b's GGSW r-1-j, for all its nodes
        X.cmux_assign(t0, t1, ggsw.reshape((batch * r,) + tuple(ggsw.shape[2:])), *shape.cbs, X.Fft(n),
                      ggsw_index=index)
        nodes = t0
    return nodes[:, :, 0].contiguous()


def div_monomial(t, d):
    """polynomial_wrapping_monic_monomial_div_assign of every polynomial of a device tensor (..., N)."""
    import torch
    n = t.shape[-1]
    d %= 2 * n
    full, rem = d // n, d % n
    out = torch.roll(t, -rem, dims=-1)
    if rem:
        out[..., n - rem:] = -out[..., n - rem:]
    return -out if full else out


def rotate_by_steps(engine, shape, glwe, ggsw):
    """The Python loop of rotate + mi_fft64_cmux_batch_indexed: glwe (batch, n_out, k+1, N), ggsw (batch, n_rot, ...)."""
    X = engine.fft64
    batch, n_out, n_rot = int(glwe.shape[0]), int(glwe.shape[1]), int(ggsw.shape[1])
    ct0, d = glwe.clone(), 1
    flat = ggsw.reshape((batch * n_rot,) + tuple(ggsw.shape[2:]))
    for i in reversed(range(n_rot)):
        ct1 = div_monomial(ct0, d).contiguous()
        d <<= 1
        X.cmux_assign(ct0, ct1, flat, *shape.cbs, X.Fft(shape.N),
                      ggsw_index=idev([b * n_rot + i for b in range(batch) for _ in range(n_out)]))
    return ct0


def lut_polys(shape, n_out, n_polys, seed):
    return dev(H.uniform_u64(H.rng(seed), (n_out, n_polys, shape.N)))


def cbs_by_stages(engine, shape, dk, lwe, delta_log, cbs=None):
    """mi_fft64_pbs_batch per level (items in the order b * level + i) -> mi_lwe_pfpks_batch -> mi_bsk_to_fourier64;
    (base_log_cbs, level_cbs) = cbs, the shape's by default."""
    import torch
    X, M = engine.fft64, engine.lwe_wopbs
    base_log, level = cbs or shape.cbs
    batch, k, n = int(lwe.shape[0]), shape.k, shape.N
    shifted = lwe << (63 - delta_log)
    shifted[:, -1] += 1 << 62
    boot = zeros((batch, level, k * n + 1), -1)
    for i in range(level):
        alpha = 1 << (63 - base_log * (level - i))
        acc = zeros((k + 1, n))
        acc[k] = -alpha
        one = zeros((batch, k * n + 1), -1)
        X.programmable_bootstrap_lwe_ciphertext(shifted.contiguous(), one, acc, dk["bsk"])
        one[:, -1] += alpha
        boot[:, i] = one
    std = zeros((batch, level, k + 1, k + 1, n), -1)
    M.private_functional_keyswitch_lwe_ciphertext_into_glwe_ciphertext(dk["pfpksk"], std, boot.reshape(batch * level, -1))
    four = fzeros((batch, level, k + 1, k + 1, n // 2, 2))
    X.convert_standard_lwe_bootstrap_key_to_fourier(std.reshape(batch * level, 1, k + 1, k + 1, n),
                                                    four.reshape(batch * level, 1, k + 1, k + 1, n // 2, 2), dk["fft"])
    torch.cuda.synchronize()
    return std, four


def extract_bits_by_stages(engine, shape, dk, lwe, delta_log, n_bits):
    """Per bit: shift, mi_lwe_keyswitch_batch, store; then q/4 on the body, mi_fft64_pbs_batch on the trivial accumulator
    -2^(delta_log - 1 + bit), its constant back on the body, subtract.  lwe (batch, k N + 1) -> the outputs (batch,
    n_bits, n + 1), most significant bit first, and the running input the last keyswitch read."""
    X, KS = engine.fft64, engine.lwe_keyswitch
    batch = int(lwe.shape[0])
    k, n, big1, small1 = shape.k, shape.N, shape.k * shape.N + 1, shape.n + 1
    cur, want = lwe.clone(), zeros((batch, n_bits, small1), -1)
    for bit in range(n_bits):
        ks = zeros((batch, small1), -1)
        KS.keyswitch_lwe_ciphertext(dk["ksk"], (cur << (64 - delta_log - bit - 1)).contiguous(), ks)
        want[:, n_bits - 1 - bit] = ks
        if bit == n_bits - 1:
            break
        ks[:, -1] += 1 << 62
        acc = zeros((k + 1, n))
        acc[k] = -(1 << (delta_log - 1 + bit))
        boot = zeros((batch, big1), -1)
        X.programmable_bootstrap_lwe_ciphertext(ks, boot, acc, dk["bsk"])
        boot[:, -1] += 1 << (delta_log + bit - 1)
        cur -= boot
    return want, cur
