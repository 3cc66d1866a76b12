"""Shared setup of the shortint / radix GPU tests: key sets made once per process, the written sequences of public calls
that each composite is defined as (csrc/c_api_shortint.cpp's header comment, restated with the Python mirror), and radix
encryption / decryption under real keys."""
import numpy as np

import multi_bit_helpers as MB
import tfhe_helpers as H

ENGINES = ("ntt", "fft", "multi-bit")
PBS_BL, PBS_L, KS_BL, KS_L = 23, 1, 4, 4
MSG = CARRY = 4
DELTA = (1 << 63) // (MSG * CARRY)
NONE = 0xFFFFFFFF
_sets = {}


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype)
    return torch.from_numpy(a.view(view) if view else a).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


def zeros(shape):
    import torch
    return torch.zeros(shape, dtype=torch.int64, device="cuda")


def i32(values):
    """Index values (0xFFFFFFFF allowed) as an int32 device tensor."""
    return dev(np.asarray(values, dtype=np.uint32))


class KeySet:
    """The three bootstrap keys of one (N, k, n) shape over one small secret key, a keyswitch key and the drift key.
    ``device=False`` stops after the host words (the CPU noise measurement needs no more)."""

    def __init__(self, engine, oracle, n, small, real, seed, k=1, ks_level=KS_L, device=True):
        g = H.rng(seed)
        self.n, self.small, self.k, self.real, self.ks_l = n, small, k, real, ks_level
        self.size = k * n + 1
        if real:
            assert k == 1, "the real key generation is the k = 1 one"
            glwe_sk = H.binary_key(g, (1, n))
            self.big_sk, self.small_sk = H.glwe_sk_as_lwe_sk(glwe_sk), H.binary_key(g, small)
            self.ksk_words = H.ksk_gen(g, self.big_sk, self.small_sk, KS_BL, ks_level, noise_log2=12)
            bsk_std = H.bsk_gen_native_l1(g, self.small_sk, glwe_sk, PBS_BL, 10)
            mb_std = MB.multi_bit_bsk_gen(g, oracle, self.small_sk, glwe_sk, PBS_BL, PBS_L, 10, 2) if n == 2048 else None
            self.zeros_words = H.lwe_encrypt_batch(g, np.zeros(32, np.uint64), self.small_sk, 12)
        else:
            self.ksk_words = H.uniform_u64(g, (k * n, ks_level, small + 1))
            bsk_std = H.uniform_u64(g, (small, PBS_L, k + 1, k + 1, n))
            mb_std = H.uniform_u64(g, (small // 2, 4, PBS_L, k + 1, k + 1, n))
            self.zeros_words = H.uniform_u64(g, (16, small + 1))
            mb_std = mb_std if n == 2048 else None
        self.ctx = oracle.NttContext(n)
        self.bsk_ntt = self.ctx.bsk_to_ntt(bsk_std, 64, False)  # Raw: what the oracle's BNF PBS reads
        # a bound that some ciphertexts meet and some do not, so that the drift step does add candidates
        self.ms_params = (2.0**52 * 1.5 if real else 2.0**53 * 1.2, 1.0, 0.0)
        self._server = {}
        self.engine = engine
        if device:
            self._to_device(bsk_std, mb_std)

    def _to_device(self, bsk_std, mb_std):
        import torch
        engine, n = self.engine, self.n
        M, X, KS, NR = engine.ntt64_pbs, engine.fft64, engine.lwe_keyswitch, engine.modulus_switch_noise_reduction
        self.plan = engine.Plan.try_new(n, engine.SOLINAS_P)
        self._bsk_dev = dev(self.bsk_ntt)
        fb = torch.zeros(bsk_std.shape[:-1] + (n // 2, 2), dtype=torch.float64, device="cuda")
        X.convert_standard_lwe_bootstrap_key_to_fourier(dev(bsk_std), fb)
        self.pbs = {"ntt": M.NttBootstrapKey(self.plan, self._bsk_dev, PBS_BL, PBS_L, M.BNF),
                    "fft": X.FourierLweBootstrapKey(fb, PBS_BL, PBS_L)}
        if mb_std is not None:  # N = 2048, the multi-bit engine's one polynomial size
            fm = torch.zeros(mb_std.shape[:-1] + (n // 2, 2), dtype=torch.float64, device="cuda")
            X.convert_standard_lwe_multi_bit_bootstrap_key_to_fourier(dev(mb_std), fm)
            self.pbs["multi-bit"] = X.FourierLweMultiBitBootstrapKey(fm, PBS_BL, PBS_L, 2)
        self.ksk = KS.LweKeyswitchKey(dev(self.ksk_words), KS_BL, self.ks_l)
        self.msk = NR.ModulusSwitchNoiseReductionKey(dev(self.zeros_words), *self.ms_params)

    def server(self, which, drift=False, ms_mode=0, m=MSG, c=CARRY):
        key = (which, drift, ms_mode, m, c)
        if key not in self._server:
            self._server[key] = self.engine.shortint.ShortintServerKey(self.ksk, self.pbs[which], m, c,
                                                                       self.msk if drift else None, ms_mode)
        return self._server[key]


# name: (N, n, real, seed, k, keyswitch levels)
SETS = {"real": (2048, 64, True, 0x51a0, 1, KS_L), "u1024": (1024, 16, False, 0x51a1, 1, KS_L),
        "u2048": (2048, 16, False, 0x51a2, 1, KS_L), "u1024k2": (1024, 16, False, 0x51a3, 2, KS_L),
        "u2048k2": (2048, 16, False, 0x51a4, 2, KS_L), "u8192": (8192, 16, False, 0x51a5, 1, KS_L),
        "real4096": (4096, 64, True, 0x51a7, 1, 6), "real2048n16": (2048, 16, True, 0x51a8, 1, 6)}
# The real set that meets the noise condition of tests/test_shortint_corners_gpu.py at each (m, c), for the NTT and
# f64 engines; the multi-bit engine has N = 2048 only and takes REAL_MULTI_BIT_8_8 at (8, 8).
REAL_FOR = {(4, 4): "real", (8, 4): "real", (4, 8): "real", (2, 2): "real", (8, 8): "real4096"}
REAL_MULTI_BIT_8_8 = "real2048n16"


def key_set(engine, oracle, name, device=True):
    """"real": N = 2048, n = 64 under real keys, keyswitch 2^4 x 4; "real4096": N = 4096, n = 64, keyswitch 2^4 x 6;
    "real2048n16": N = 2048, n = 16, keyswitch 2^4 x 6; "u<N>[k2]": uniform key words at n = 16 (k = 1, or 2 with
    the suffix) for the bit-exact tests.  device=False: the host words only, made again at every call."""
    if not device:
        return KeySet(engine, oracle, *SETS[name], device=False)
    if name not in _sets:
        _sets[name] = KeySet(engine, oracle, *SETS[name])
    return _sets[name]


SENTINEL = np.uint64(0x5E5E5E5E5E5E5E5E)


def oracle_apply(oracle, ks, lwe, luts, lut_index, in_index, mode, drift, ms_params=None, k=1):
    """mi_shortint_apply_lut_batch through oracle.lwe_keyswitch and the oracle's PBS at GLWE dimension k: the expected
    output rows (SENTINEL where nothing is written), and which rows are written at all."""
    import ms_noise_helpers as MN
    n, small = ks.n, ks.small
    cur = oracle.lwe_keyswitch(ks.ksk_words, lwe, small, KS_BL, ks.ks_l)
    ms = mode
    if drift:
        log2n = (2 * n).bit_length() - 1
        p = MN.Params(*(ms_params or ks.ms_params), log2n)
        cand, _ = MN.choose_np(cur, ks.zeros_words, p)
        cur, ms = MN.switch_np(MN.improve_np(cur, ks.zeros_words, cand), log2n), 2
    n_items = len(lut_index)
    src = np.arange(n_items) if in_index is None else np.asarray(in_index)
    live = (src < lwe.shape[0]) & (np.asarray(lut_index) < luts.shape[0])
    out = np.full((n_items, k * n + 1), SENTINEL, np.uint64)
    rows = np.flatnonzero(live)
    if rows.size:
        if ms == 2:
            acc = luts[np.asarray(lut_index)[rows]]
            rot = ks.ctx.blind_rotate_batch(acc, cur[src[rows]], ks.bsk_ntt, k, PBS_BL, PBS_L, bnf=True, ms_mode=2)
            out[rows] = np.stack([oracle.sample_extract(r, n, k) for r in rot])
        else:
            for l in set(np.asarray(lut_index)[rows].tolist()):
                sel = rows[np.asarray(lut_index)[rows] == l]
                out[sel] = ks.ctx.pbs_batch_bnf(cur[src[sel]], luts[l], ks.bsk_ntt, k, PBS_BL, PBS_L,
                                                centered=(ms == 1))
    return out, live


# ---- the written sequences (public calls only) ----

def seq_pbs(sk, out, small_in, luts, lut_index, ms_mode):
    X, M = sk.bootstrapping_key, None
    from tfhe_ntt_amd import fft64, ntt64_pbs
    if sk.pbs_engine == 0:
        ntt64_pbs.programmable_bootstrap_ntt64_bnf_lwe_ciphertext_mem_optimized(small_in, out, luts, X, ms_mode, lut_index)
    elif sk.pbs_engine == 1:
        fft64.programmable_bootstrap_lwe_ciphertext(small_in, out, luts, X, ms_mode, lut_index)
    else:
        fft64.multi_bit_programmable_bootstrap_lwe_ciphertext(small_in, out, luts, X, lut_index)


def seq_apply(engine, sk, out, inp, luts, lut_index, in_index=None):
    """mi_shortint_apply_lut_batch as its stages: KS, DRIFT, LC gather with the masked LUT index, PBS."""
    import torch
    LA, KS = engine.lwe_linear_algebra, engine.lwe_keyswitch
    n_in, n_items = int(inp.shape[0]), int(out.shape[0])
    small1 = sk.key_switching_key.output_key_lwe_dimension + 1
    if n_in == 0 or n_items == 0:
        return
    cur = zeros((n_in, small1))
    KS.keyswitch_lwe_ciphertext(sk.key_switching_key, inp, cur)
    mode = sk.ms_mode
    if sk.modulus_switch_noise_reduction_key is not None:
        sw = zeros((n_in, small1))
        log2n = (2 * sk.polynomial_size).bit_length() - 1
        sk.modulus_switch_noise_reduction_key.improve_noise_and_modulus_switch(cur, sw, log2n)
        cur, mode = sw, engine.ntt64_pbs.MS_PRE_SWITCHED
    if lut_index is None:
        lut_index = torch.arange(n_items, dtype=torch.int32, device="cuda")
    if in_index is not None:
        gathered = zeros((n_items, small1))
        LA.lwe_linear_combination(gathered, cur, in_index.reshape(n_items, 1).contiguous())
        in_range = (in_index.to(torch.int64) & 0xFFFFFFFF) < n_in
        lut_index = torch.where(in_range, lut_index, torch.full_like(lut_index, -1))
        cur = gathered
    seq_pbs(sk, out, cur, luts, lut_index.contiguous(), mode)


def key_luts(sk):
    """The five lookup tables mi_shortint_key_create builds: MSG, CARRY, STATE0, STATE, SCAN."""
    import torch
    m = sk.message_modulus
    fs = [lambda x: x % m, lambda x: x // m, lambda x: int(x >= m),
          lambda x: 1 if x >= m else (2 if x == m - 1 else 0),
          lambda x: (x % m) if (x // m) % m == 2 else (x // m) % m]
    return torch.stack([sk.generate_lookup_table(f) for f in fs]).contiguous()


def _add_previous(engine, out, work, total, blocks):
    j = np.arange(total)
    prev = np.where(j % blocks >= 1, total + j - 1, NONE)
    engine.lwe_linear_algebra.lwe_linear_combination(out, work, i32(np.stack([j, prev], axis=1)))


def seq_propagate(engine, sk, radix, carry_out=None):
    """mi_radix_propagate_single_carry_batch as LC / APPLY calls; radix (I, B, size) in place."""
    LA = engine.lwe_linear_algebra
    n_int, blocks, size = radix.shape
    total, m = n_int * blocks, sk.message_modulus
    flat = radix.reshape(total, size)
    luts = key_luts(sk)
    j = np.arange(2 * total)
    want_state = blocks > 1 or carry_out is not None
    items = 2 * total if want_state else total
    work = zeros((2 * total, size))
    lut1 = np.where(j < total, 0, np.where((j - total) % blocks == 0, 2, 3))
    seq_apply(engine, sk, work[:items], flat, luts, i32(lut1[:items]), i32((j % total)[:items]))
    if blocks == 1:
        LA.lwe_linear_combination(flat, work, i32(np.arange(total).reshape(total, 1)))
        if carry_out is not None:
            LA.lwe_linear_combination(carry_out, work, i32((total + np.arange(total)).reshape(total, 1)))
        return
    msg_st = work
    st = work[total:]
    sp = 1
    while sp < blocks:
        cnt = n_int * (blocks - sp)
        c = np.arange(cnt)
        cur = total + (c // (blocks - sp)) * blocks + sp + c % (blocks - sp)
        pack = zeros((cnt, size))
        coeff = dev(np.tile(np.array([m, 1], np.int64), (cnt, 1)))
        LA.lwe_linear_combination(pack, msg_st, i32(np.stack([cur, cur - sp], axis=1)), coeff)
        t = np.arange(total)
        in_index = np.where(t % blocks >= sp, (t // blocks) * (blocks - sp) + t % blocks - sp, NONE)
        seq_apply(engine, sk, st, pack, luts, i32(np.full(total, 4)), i32(in_index))
        sp *= 2
    summed = zeros((total, size))
    _add_previous(engine, summed, msg_st, total, blocks)
    seq_apply(engine, sk, flat, summed, luts, i32(np.full(total, 0)))
    if carry_out is not None:
        top = total + np.arange(n_int) * blocks + blocks - 1
        LA.lwe_linear_combination(carry_out, msg_st, i32(top.reshape(n_int, 1)))


def seq_full_propagate(engine, sk, radix):
    import shortint_ref as R
    n_int, blocks, size = radix.shape
    total = n_int * blocks
    flat = radix.reshape(total, size)
    luts = key_luts(sk)
    j = np.arange(2 * total)
    single = blocks == 1 or R.single_carry_supported(sk.message_modulus, sk.carry_modulus)
    for _ in range(1 if single else blocks):
        work = zeros((2 * total, size))
        seq_apply(engine, sk, work, flat, luts, i32(np.where(j < total, 0, 1)), i32(j % total))
        _add_previous(engine, flat, work, total, blocks)
    if single and blocks > 1:
        seq_propagate(engine, sk, radix)


def seq_add(engine, sk, out, lhs, rhs, carry_out=None):
    import torch
    n_int, blocks, size = lhs.shape
    total = n_int * blocks
    both = torch.cat([lhs.reshape(total, size), rhs.reshape(total, size)]).contiguous()
    j = np.arange(total)
    engine.lwe_linear_algebra.lwe_linear_combination(out.reshape(total, size), both, i32(np.stack([j, total + j], axis=1)))
    seq_propagate(engine, sk, out, carry_out)


# ---- radix integers under the real key set ----

def delta_of(m=MSG, c=CARRY):
    return (1 << 63) // (m * c)


def encrypt_blocks(ks, g, values, m=MSG, c=CARRY):
    """values (...,) block values -> LWEs (..., size) under the big key, noise 2^10."""
    v = np.asarray(values, dtype=np.uint64)
    cts = H.lwe_encrypt_batch(g, v.reshape(-1) * np.uint64(delta_of(m, c)), ks.big_sk, noise_log2=10)
    return cts.reshape(v.shape + (ks.size,))


def decrypt_blocks(ks, cts, m=MSG, c=CARRY):
    """LWEs (..., size) -> block values mod 2 m c (the padding bit kept, so that an overflow shows)."""
    dec = H.lwe_decrypt_batch(np.asarray(cts, dtype=np.uint64), ks.big_sk)
    return np.vectorize(lambda d: H.decode(int(d), delta_of(m, c), m * c))(dec)


def phase_errors(cts, sk, values, m=MSG, c=CARRY):
    """The signed phase errors of LWEs (..., dim + 1) that should hold values * 2^63 / (m c) under sk."""
    dec = H.lwe_decrypt_batch(np.asarray(cts, dtype=np.uint64), sk)
    with np.errstate(over="ignore"):
        return (dec - np.asarray(values, dtype=np.uint64) * np.uint64(delta_of(m, c))).view(np.int64)


def radix_digits(values, blocks, m=MSG, c=CARRY):
    return np.array([[(int(v) // m**b) % m for b in range(blocks)] for v in values], dtype=np.uint64)


def radix_values(digits, m=MSG, c=CARRY):
    return [sum(int(x) * m**i for i, x in enumerate(row)) for row in digits]


def measure_noise(oracle, ks, m, c, seed, multi_bit=False):
    """Every value 0 .. m c - 1 through oracle.lwe_keyswitch, the standard modulus switch to 2 N and the oracle's
    bootstrap through the identity table, under the real keys of ks, on the host -> the worst absolute phase error of
    the keyswitched-and-switched input (under the small key) and of the output (under the big key).  multi_bit: the
    input error is that of the multi-bit engine's switch at grouping factor 2 (multi_bit_helpers.group_degrees: one
    rounding per group, of the sum of the mask elements the group's key bits select)."""
    import shortint_ref as R
    values = np.arange(m * c, dtype=np.uint64)
    cts = encrypt_blocks(ks, H.rng(seed), values, m, c)
    small = oracle.lwe_keyswitch(ks.ksk_words, cts, ks.small, KS_BL, ks.ks_l)
    log2n = (2 * ks.n).bit_length() - 1
    up = np.uint64(64 - log2n)
    if multi_bit:
        deg = MB.group_degrees(small[:, :-1].reshape(len(values), ks.small // 2, 2), 2, log2n)  # (items, groups, 4)
        pick = (2 * ks.small_sk[0::2] + ks.small_sk[1::2]).astype(np.int64)  # the GGSW whose selection bits are the key's
        mask = np.take_along_axis(deg, pick[None, :, None], axis=2)[:, :, 0].sum(axis=1)
        body = oracle.lwe_ms64(small, log2n, False)[:, -1].astype(np.int64)
        with np.errstate(over="ignore"):
            phase = ((body - mask) % (1 << log2n)).astype(np.uint64) << up
            e_in = (phase - values * np.uint64(delta_of(m, c))).view(np.int64)
    else:
        e_in = phase_errors(oracle.lwe_ms64(small, log2n, False) << up, ks.small_sk, values, m, c)
    out = ks.ctx.pbs_batch_bnf(small, R.lut_fill(ks.n, 1, m, c, list(range(m * c))), ks.bsk_ntt, 1, PBS_BL, PBS_L)
    return int(np.abs(e_in).max()), int(np.abs(phase_errors(out, ks.big_sk, values, m, c)).max())
