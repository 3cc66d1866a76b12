"""The exact 128-bit bootstrap (csrc/pbs128.hip) against plain integer arithmetic (tests/pbs128_helpers.py): every
output word of the external product, the CMUX, the blind rotation and the PBS is compared bit for bit.

* random keys and inputs at the smallest shapes that reach each path: the generic transform (N = 256), k = 3, the
  N = 2048 bodies with the production limb plan (w = 25, 6 limbs), base_log above 32 with 16 limbs;
* the decomposer's corner corpus as the input GLWE, against a random GGSW and against the noise-free gadget GGSW of
  message 1 (the product is then closest_representable of the input);
* saturation: the digit vectors of largest magnitude against key coefficients of 2^128 - 1 (every limb full) and of one
  full limb, signs arranged so that coefficient N - 1 and coefficient 0 add every term: the input for which a limb one
  bit too wide wraps silently.  Two adjacent levels cannot both decompose to +-2^(B-1) (pbs128_helpers.
  saturating_digits), so at 3 levels the extreme reachable vectors are (2^23, 2^23 - 1, 2^23 - 1) and its negative
  twin; at 1 level they are exactly +-2^(B-1).  The tests assert the digits the helper decomposes;
* blind rotation and PBS over masks that switch to 0, 1, N - 1, N, 2N - 1, in the three ms modes, and in two chunks;
* a real key at the noise-squashing shape: every message decodes, and the output equals the helper's."""
import ctypes

import numpy as np
import pytest

import pbs128_helpers as H

pytestmark = pytest.mark.gpu

P = 0xFFFFFFFF00000001
PRODUCTION = (2048, 2, 24, 3)
EXT_SHAPES = [(256, 1, 23, 1), (512, 3, 16, 4), PRODUCTION, (2048, 1, 42, 3)]  # (N, k, base_log, level)
ROTATE_SHAPES = [PRODUCTION, (256, 1, 23, 1)]
N_GGSW, BATCH = 6, 5
STANDARD, CENTERED, PRE_SWITCHED = 0, 1, 2


def dev(words):
    import torch
    return torch.from_numpy(np.ascontiguousarray(words, dtype=np.uint64).view(np.int64)).cuda()


def dev128(values):
    return dev(H.to_words(values))


def host128(t):
    return H.from_words(t.cpu().numpy().view(np.uint64))


def make_key(engine, ggsws, base_log, level):
    return engine.pbs128.LweBootstrapKey128(dev128(ggsws), base_log, level)


# ---- external product and CMUX ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,k,base_log,level", EXT_SHAPES)
def test_external_product_and_cmux(engine, n, k, base_log, level):
    g = H.rng(n + 7 * k + base_log)
    ggsws = [H.uniform_ggsw(g, k, n, level) for _ in range(2)]
    key = make_key(engine, ggsws, base_log, level)
    assert (key.limb_bits, key.n_limbs) == H.limb_rule(n, k, base_log, level)
    packed = [H.PackedGgsw(x, base_log) for x in ggsws]
    batch = 3
    glwe = [H.uniform_glwe(g, k, n) for _ in range(batch)]
    out0 = [H.uniform_glwe(g, k, n) for _ in range(batch)]
    for index in (1, 0):
        want = [[list(p) for p in x] for x in out0]
        for b in range(batch):
            H.external_product(want[b], packed[index], glwe[b], level)
        out, inp = dev128(out0), dev128(glwe)
        engine.pbs128.add_external_product_assign(out, key, index, inp)
        assert host128(out) == want, ("ext", index)
        assert host128(inp) == glwe, "the input is left as it was"
    want0 = [[list(p) for p in x] for x in out0]
    want1 = [[list(p) for p in x] for x in glwe]
    for b in range(batch):
        H.cmux(want0[b], want1[b], packed[1], level)
    ct0, ct1 = dev128(out0), dev128(glwe)
    engine.pbs128.cmux_assign(ct0, ct1, key, 1)
    assert host128(ct0) == want0
    assert host128(ct1) == want1, "ct1 is left holding ct1 - ct0"


@pytest.mark.parametrize("n,k,base_log,level", EXT_SHAPES)
def test_corner_corpus(engine, n, k, base_log, level):
    g = H.rng(1000 + n + base_log)
    batch = 3
    words = H.corner_words(base_log, level)
    flat = H.corner_poly(words, batch * (k + 1) * n, g)
    assert set(words) <= set(flat)
    glwe = [[flat[(b * (k + 1) + c) * n:(b * (k + 1) + c + 1) * n] for c in range(k + 1)] for b in range(batch)]
    ggsws = [H.uniform_ggsw(g, k, n, level), H.gadget_ggsw(1, k, n, base_log, level)]
    key = make_key(engine, ggsws, base_log, level)
    packed = H.PackedGgsw(ggsws[0], base_log)
    out0 = [H.uniform_glwe(g, k, n) for _ in range(batch)]
    want = [[list(p) for p in x] for x in out0]
    for b in range(batch):
        H.external_product(want[b], packed, glwe[b], level)
    out = dev128(out0)
    engine.pbs128.add_external_product_assign(out, key, 0, dev128(glwe))
    assert host128(out) == want
    zero = dev128([[[0] * n] * (k + 1)] * batch)
    engine.pbs128.add_external_product_assign(zero, key, 1, dev128(glwe))
    assert host128(zero) == [[[H.closest_representable(x, base_log, level) for x in p] for p in ct] for ct in glwe]


@pytest.mark.parametrize("n,k,base_log,level", [PRODUCTION, (2048, 1, 23, 1)])
def test_saturation(engine, n, k, base_log, level):
    w, n_limbs = H.limb_rule(n, k, base_log, level)
    kinds = ("plus", "minus", "index0")
    glwe = [[H.saturating_poly(base_log, level, n, kind)] * (k + 1) for kind in kinds]
    plus, minus = (H.saturating_digits(base_log, level, neg) for neg in (False, True))
    for kind, ct in zip(kinds, glwe):  # the digits the helper decomposes are the extreme ones
        for e in (0, 1, n - 1):
            want = plus if kind == "plus" or (kind == "index0" and e == 0) else minus
            assert H.py_decompose(ct[0][e], base_log, level) == want
    # on this input a limb one bit wider would leave (-p/2, p/2): the sum the widest limb then sees at coefficient N - 1
    rows_sum = (k + 1) * n * sum(plus)
    assert rows_sum * ((1 << w) - 1) <= (P - 1) // 2 < rows_sum * ((1 << (w + 1)) - 1)
    full = [[[[H.MASK128] * n] * (k + 1)] * (k + 1)] * level
    one_limb = [[[[((1 << w) - 1) << w] * n] * (k + 1)] * (k + 1)] * level
    ggsws = [full, one_limb]
    key = make_key(engine, ggsws, base_log, level)
    assert (key.limb_bits, key.n_limbs) == (w, n_limbs)
    for index in (0, 1):
        packed = H.PackedGgsw(ggsws[index], base_log)
        want = [[[0] * n for _ in range(k + 1)] for _ in kinds]
        for b in range(len(kinds)):
            H.external_product(want[b], packed, glwe[b], level)
        out = dev128([[[0] * n] * (k + 1)] * len(kinds))
        engine.pbs128.add_external_product_assign(out, key, index, dev128(glwe))
        assert host128(out) == want, index


# ---- blind rotation and PBS -------------------------------------------------------------------------------------------

class RotateCase:
    """One shape's key, LUT, accumulators and LWEs, with the helper's results cached by the switched values."""

    def __init__(self, engine, n, k, base_log, level):
        self.shape = (n, k, base_log, level)
        g = H.rng(31 * n + base_log)
        self.log = n.bit_length()  # log2(2N)
        bsk = [H.uniform_ggsw(g, k, n, level) for _ in range(N_GGSW)]
        self.key = make_key(engine, bsk, base_log, level)
        self.packed = [H.PackedGgsw(x, base_log) for x in bsk]
        self.lut = H.uniform_glwe(g, k, n)
        self.accs = [H.uniform_glwe(g, k, n) for _ in range(BATCH)]
        unit = 1 << (64 - self.log)

        def word(v):  # a u64 that the standard switch sends to v: off the grid by less than half a unit
            return (v * unit + int(g.integers(-(unit // 2) + 1, unit // 2))) % H.M64

        bodies = [0, n, 2 * n - 1, int(g.integers(0, 2 * n)), int(g.integers(0, 2 * n))]
        self.lwes = []
        for b in range(BATCH):
            masks = [0, 1, n - 1, n, 2 * n - 1, int(g.integers(1, 2 * n))]
            masks = masks[b:] + masks[:b]  # every GGSW meets every special value
            self.lwes.append([word(v) for v in masks + [bodies[b]]])
        assert all(H.switch_lwe(lwe, self.log)[-1] == v for lwe, v in zip(self.lwes, bodies))
        self._rotated = {}

    def switched(self, centered):
        return [H.switch_lwe(lwe, self.log, centered) for lwe in self.lwes]

    def rotated(self, b, switched, shared_lut):
        """The helper's blind rotation of the LUT (or of item b's own accumulator) by the switched values."""
        key = (b if not shared_lut else -1, tuple(switched))
        if key not in self._rotated:
            acc = self.lut if shared_lut else self.accs[b]
            self._rotated[key] = H.blind_rotate([list(p) for p in acc], switched, self.packed, self.shape[3])
        return self._rotated[key]

    def lwe_input(self, engine, mode):
        """(device tensor, the mode to call with, the helper's switched values) of one of the test's five modes."""
        raw = dev(np.array(self.lwes, dtype=np.uint64))
        if mode in ("standard", "centered"):
            return raw, STANDARD if mode == "standard" else CENTERED, self.switched(mode == "centered")
        centered = mode == "pre_switched_centered"
        out = dev(np.zeros((BATCH, N_GGSW + 1), np.uint64))
        engine.lwe_keyswitch.lwe_ciphertext_modulus_switch(raw, out, self.log, centered=centered)
        want = self.switched(centered)
        assert out.cpu().numpy().view(np.uint64).tolist() == want
        return out, PRE_SWITCHED, want


_CASES = {}


@pytest.fixture
def rotate_case(engine, request):
    shape = request.param
    if shape not in _CASES:
        _CASES[shape] = RotateCase(engine, *shape)
    return _CASES[shape]


MODES = ["standard", "centered", "pre_switched", "pre_switched_centered"]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("rotate_case", ROTATE_SHAPES, indirect=True)
def test_pbs(engine, rotate_case, mode):
    import torch

    case = rotate_case
    n, k, _, _ = case.shape
    lwe, ms_mode, switched = case.lwe_input(engine, mode)
    out = torch.zeros((BATCH, k * n + 1, 2), dtype=torch.int64, device="cuda")
    engine.pbs128.programmable_bootstrap_f128_lwe_ciphertext(lwe, out, dev128(case.lut), case.key, ms_mode)
    want = [H.sample_extract(case.rotated(b, switched[b], True)) for b in range(BATCH)]
    assert host128(out) == want


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("rotate_case", ROTATE_SHAPES, indirect=True)
def test_blind_rotate(engine, rotate_case, mode):
    case = rotate_case
    n = case.shape[0]
    # one accumulator per item; at N = 2048 the items' own accumulators are rotated in the standard mode and the LUT
    # (whose rotations test_pbs shares) in the others: the per-item path does not depend on the mode
    own = n < 2048 or mode == "standard"
    lwe, ms_mode, switched = case.lwe_input(engine, mode)
    acc = dev128(case.accs if own else [case.lut] * BATCH)
    engine.pbs128.blind_rotate_assign(case.key, acc, lwe, ms_mode)
    assert host128(acc) == [case.rotated(b, switched[b], not own) for b in range(BATCH)]


@pytest.mark.parametrize("rotate_case", ROTATE_SHAPES, indirect=True)
def test_two_chunks(engine, rotate_case, monkeypatch):
    """The chunk bound forced below the batch (MI_PBS128_CHUNK, read per call): 5 items run as chunks of 3 and 2."""
    import torch

    case = rotate_case
    n, k, base_log, level = case.shape
    monkeypatch.setenv("MI_PBS128_CHUNK", "3")
    lwe, ms_mode, switched = case.lwe_input(engine, "standard")
    out = torch.zeros((BATCH, k * n + 1, 2), dtype=torch.int64, device="cuda")
    lut = dev128(case.lut)

    # That the bound took effect is read off the scratch pool: emptied first, it then holds the one block the call
    # asked for, a chunk's items (digits, limb products, u128 accumulator, body correction) in whole MiB.  At the
    # production shape 3 items round to 2 MiB and all 5 to 3 MiB, so one chunk of 5 would show.
    per = (k + 1) * n
    item_bytes = 8 * (per * level + per * case.key.n_limbs + 2 * per + 1)

    def mib(items):
        return -(-items * item_bytes // (1 << 20)) << 20

    if case.shape == PRODUCTION:
        assert mib(3) < mib(BATCH)
    torch.cuda.synchronize()
    engine.ntt64_pbs.scratch_trim(0)
    assert engine.ntt64_pbs.scratch_bytes(0) == 0  # nothing idle is left to serve the request
    engine.pbs128.programmable_bootstrap_f128_lwe_ciphertext(lwe, out, lut, case.key, ms_mode)
    torch.cuda.synchronize()
    assert engine.ntt64_pbs.scratch_bytes(0) == mib(3)
    assert host128(out) == [H.sample_extract(case.rotated(b, switched[b], True)) for b in range(BATCH)]
    acc = dev128([case.lut] * BATCH)
    engine.pbs128.blind_rotate_assign(case.key, acc, lwe, ms_mode)
    assert host128(acc) == [case.rotated(b, switched[b], True) for b in range(BATCH)]
    # and the external product: 5 GLWEs as chunks of 3 and 2
    g = H.rng(77)
    glwe = [H.uniform_glwe(g, k, n) for _ in range(BATCH)]
    want = [[[0] * n for _ in range(k + 1)] for _ in range(BATCH)]
    for b in range(BATCH):
        H.external_product(want[b], case.packed[2], glwe[b], level)
    o = dev128([[[0] * n] * (k + 1)] * BATCH)
    engine.pbs128.add_external_product_assign(o, case.key, 2, dev128(glwe))
    assert host128(o) == want


# ---- a real key at the noise-squashing shape ----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def real_key(engine):
    """V1_4_NOISE_SQUASHING_PARAM_MESSAGE_2_CARRY_2_KS_PBS_TUNIFORM_2M128's GLWE side (k 2, N 2048, base 2^24, 3
    levels, TUniform(30)) over an LWE key of dimension 8."""
    n, k, base_log, level = PRODUCTION
    g = H.rng(2024)
    lwe_sk = H.binary_key(g, 8)
    glwe_sk = [H.binary_key(g, n) for _ in range(k)]
    bsk = H.bsk_gen(g, lwe_sk, glwe_sk, base_log, level, 30)
    return {"g": g, "lwe_sk": lwe_sk, "glwe_sk": glwe_sk, "key": make_key(engine, bsk, base_log, level),
            "packed": [H.PackedGgsw(x, base_log) for x in bsk]}


def test_real_key_every_message(engine, real_key):
    import torch

    n, k, base_log, level = PRODUCTION
    msg_mod = 16  # 4 message bits and the padding bit
    delta64, delta128 = 1 << 59, 1 << 123
    lut = H.pbs_lut(n, k, msg_mod, delta128, lambda m: m)
    lwes = [H.lwe_encrypt_u64(real_key["g"], m * delta64, real_key["lwe_sk"]) for m in range(msg_mod)]
    out = torch.zeros((msg_mod, k * n + 1, 2), dtype=torch.int64, device="cuda")
    engine.pbs128.programmable_bootstrap_f128_lwe_ciphertext(dev(np.array(lwes, dtype=np.uint64)), out, dev128(lut),
                                                             real_key["key"], CENTERED)
    got = host128(out)
    flat_sk = [s for poly in real_key["glwe_sk"] for s in poly]
    assert [H.decode(H.lwe_decrypt_u128(ct, flat_sk), delta128, msg_mod) for ct in got] == list(range(msg_mod))
    want = [H.pbs(lut, H.switch_lwe(lwe, n.bit_length(), centered=True), real_key["packed"], level) for lwe in lwes]
    assert got == want


# ---- errors --------------------------------------------------------------------------------------------------------------

def test_errors(engine):
    import torch
    from tfhe_ntt_amd import _lib

    n, k, base_log, level = 256, 1, 23, 1
    g = H.rng(9)
    bsk = dev128([H.uniform_ggsw(g, k, n, level) for _ in range(2)])
    M = engine.pbs128
    with pytest.raises(engine.MiError) as err:  # a plan of another prime
        M.LweBootstrapKey128(bsk, base_log, level, plan=engine.Plan.try_new(n, 0x3F5A0001))
    assert err.value.status == _lib.MI_ERR_UNSUPPORTED
    with pytest.raises(engine.MiError) as err:  # the Goldilocks plan of another N
        M.LweBootstrapKey128(bsk, base_log, level, plan=engine.Plan.try_new(2 * n, P))
    assert err.value.status == _lib.MI_ERR_UNSUPPORTED
    assert "Goldilocks plan of the key's polynomial size" in str(err.value)
    key = M.LweBootstrapKey128(bsk, base_log, level)
    info = [ctypes.c_size_t(), ctypes.c_int(), ctypes.c_size_t(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int(),
            ctypes.c_int()]
    assert _lib.lib().mi_pbs128_key_info(key._h, *[ctypes.byref(x) for x in info]) == _lib.MI_OK
    assert [x.value for x in info] == [2, k, n, base_log, level, 32, 4]
    glwe = H.uniform_glwe(g, k, n)
    before = H.uniform_glwe(g, k, n)
    for entry in (M.add_external_product_assign, None):
        out, inp = dev128([before]), dev128([glwe])
        with pytest.raises(engine.MiError) as err:  # an index past the key: nothing is written
            if entry:
                entry(out, key, 2, inp)
            else:
                M.cmux_assign(out, inp, key, 2)
        assert err.value.status == _lib.MI_ERR_INVALID_ARG and "ggsw_index must be < n_ggsw" in str(err.value)
        torch.cuda.synchronize()
        assert host128(out) == [before] and host128(inp) == [glwe]
    both = dev128([before, glwe])
    L = _lib.lib()
    base, item = both.data_ptr(), (k + 1) * n * 16
    # the same buffer, half an item apart, and two items one item apart (rejected before any pointer is used)
    for out_p, in_p, batch in ((base, base, 1), (base, base + item // 2, 1), (base + item, base, 2)):
        for entry in (L.mi_ext_product128_batch, L.mi_cmux128_batch):  # overlapping operands: nothing is written
            assert entry(key._h, 0, out_p, in_p, batch, None) == _lib.MI_ERR_INVALID_ARG
            assert L.mi_last_error_message() == b"buffers overlap"
    torch.cuda.synchronize()
    assert host128(both) == [before, glwe]
    assert L.mi_ext_product128_batch(key._h, 0, None, None, 0, None) == _lib.MI_OK
    assert L.mi_cmux128_batch(key._h, 0, None, None, 0, None) == _lib.MI_OK
    assert L.mi_blind_rotate128_batch(key._h, None, None, 0, STANDARD, None) == _lib.MI_OK
    assert L.mi_pbs128_batch(key._h, None, None, None, 0, STANDARD, None) == _lib.MI_OK
    assert L.mi_pbs128_batch(key._h, None, None, None, 1, STANDARD, None) == _lib.MI_ERR_INVALID_ARG
    assert L.mi_last_error_message() == b"buffer is NULL"
    assert L.mi_pbs128_batch(key._h, None, None, None, 0, 7, None) == _lib.MI_ERR_INVALID_ARG
    assert L.mi_last_error_message() == b"unknown ms_mode"
