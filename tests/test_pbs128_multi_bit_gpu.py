"""The exact multi-bit 128-bit bootstrap (csrc/pbs128_multi_bit.hip) against plain integer arithmetic
(tests/pbs128_multi_bit_helpers.py): every output word of the blind rotation and the PBS is compared bit for bit.

* the limb plan of every grouping factor against the big-integer rule, and what the key reports;
* one step (a single-group key of uniform u128 GGSWs) at the smallest shapes that reach each path: the generic transform
  (N = 256), k = 3, the N = 2048 body with the production limb plan (w = 22, 6 limbs) and base_log above 32, bodies that
  switch to 0, N and 2N - 1;
* every subset degree: mask groups whose subset sums switch to 0, 1, N - 1, N, N + 1, 2N - 1 on both rounding edges, and
  groups whose elements each lie just under half a switching unit, where switching each element first gives other
  degrees and another result;
* saturation: an all-zero mask group (every degree 0, so the 2^g GGSWs add up without a rotation) over keys whose
  coefficients have every limb full / one limb full and accumulators that decompose to the digits of largest magnitude:
  the input on which a limb one bit wider would wrap silently;
* several groups in two chunks, the PBS with its shared LUT, the full-length production key in closed form, real keys
  at every grouping factor, and the argument errors."""
import ctypes

import numpy as np
import pytest

import pbs128_helpers as R
import pbs128_multi_bit_helpers as H

pytestmark = pytest.mark.gpu

P = 0xFFFFFFFF00000001
PRODUCTION = (2048, 2, 23, 3, 4)  # N, k, base_log, level, grouping factor
STEP_SHAPES = [(256, 1, 23, 1, 2), (512, 3, 16, 4, 3), PRODUCTION, (2048, 1, 42, 3, 2)]
ROTATE_SHAPES = [PRODUCTION, (256, 1, 23, 1, 2)]
BATCH = 5


def dev(words):
    import torch
    return torch.from_numpy(np.ascontiguousarray(words, dtype=np.uint64).view(np.int64)).cuda()


def dev128(values):
    return dev(R.to_words(values))


def host128(t):
    return R.from_words(t.cpu().numpy().view(np.uint64))


def make_key(engine, words, base_log, level, g):
    return engine.pbs128.LweMultiBitBootstrapKey128(dev(words), base_log, level, g)


def word_for(rng, v, log_mod):
    """A u64 that the standard switch sends to v: off the grid by less than half a unit."""
    unit = 1 << (64 - log_mod)
    return (v * unit + int(rng.integers(-(unit // 2) + 1, unit // 2))) % R.M64


def random_mask(rng, count):
    return [int(v) for v in rng.integers(0, R.M64, size=count, dtype=np.uint64)]


def rotate(engine, key, accs, lwes):
    acc = dev128(accs)
    engine.pbs128.multi_bit_blind_rotate_assign(key, acc, dev(np.array(lwes, dtype=np.uint64)))
    return host128(acc)


# ---- the limb plan ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("g", [2, 3, 4])
def test_limb_plan(engine, g):
    from tfhe_ntt_amd import _lib

    n, k, base_log, level, _ = PRODUCTION
    want = H.limb_rule(n, k, base_log, level, g)
    assert engine.pbs128.multi_bit_limb_plan(n, k, base_log, level, g) == want
    if g == 4:
        assert want == (22, 6)
    key = make_key(engine, H.uniform_key_words(R.rng(g), 1, g, k, n, level), base_log, level, g)
    assert (key.limb_bits, key.n_limbs) == want
    info = [ctypes.c_size_t(), ctypes.c_int(), ctypes.c_size_t(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int(),
            ctypes.c_int(), ctypes.c_int()]
    assert _lib.lib().mi_pbs128_multi_bit_key_info(key._h, *[ctypes.byref(x) for x in info]) == _lib.MI_OK
    assert [x.value for x in info] == [g, k, n, base_log, level, g, *want]


# ---- one step -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,k,base_log,level,g", STEP_SHAPES)
def test_one_step(engine, n, k, base_log, level, g):
    rng = R.rng(n + 7 * k + base_log + g)
    log_mod = n.bit_length()
    words = H.uniform_key_words(rng, 1, g, k, n, level)
    key = make_key(engine, words, base_log, level, g)
    assert (key.limb_bits, key.n_limbs) == H.limb_rule(n, k, base_log, level, g)
    bodies = [0, n, 2 * n - 1, int(rng.integers(0, 2 * n)), int(rng.integers(0, 2 * n))]
    lwes = [random_mask(rng, g) + [word_for(rng, v, log_mod)] for v in bodies]
    assert [R.modulus_switch(lwe[-1], log_mod) % (2 * n) for lwe in lwes] == bodies
    accs = [R.uniform_glwe(rng, k, n) for _ in bodies]
    want = [H.blind_rotate(acc, lwe, words, base_log, level, g) for acc, lwe in zip(accs, lwes)]
    assert rotate(engine, key, accs, lwes) == want


# ---- every subset degree ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("g", [2, 3, 4])
def test_every_subset_degree(engine, g):
    n, k, base_log, level = 256, 1, 23, 1
    rng = R.rng(300 + g)
    log_mod = n.bit_length()
    groups, first_half = H.corner_mask_groups(g, n, rng)
    # the prescribed degrees are reached, on both rounding edges: a word on the lower edge is the smallest that switches
    # to its degree, one on the upper edge the largest
    reached = set()
    for mask in groups:
        for idx, d in enumerate(H.subset_degrees(mask, g, log_mod)):
            if idx:
                s = sum(a for a, bit in zip(mask, H.MB.selection_bits(idx, g)) if bit) & R.MASK64
                reached |= {(d, edge) for edge in (0, 1) if H.edge_words(d, log_mod)[edge] == s}
    assert {(t, edge) for t in (0, 1, n - 1, n, n + 1, 2 * n - 1) for edge in (0, 1)} <= reached
    words = H.uniform_key_words(rng, 1, g, k, n, level)
    key = make_key(engine, words, base_log, level, g)
    lwes = [mask + [word_for(rng, int(rng.integers(0, 2 * n)), log_mod)] for mask in groups]
    accs = [R.uniform_glwe(rng, k, n) for _ in groups]
    want = [H.blind_rotate(acc, lwe, words, base_log, level, g) for acc, lwe in zip(accs, lwes)]
    for b in range(first_half, len(groups)):  # the sum's switch differs from the sum of switches, and so does the result
        assert H.subset_degrees(groups[b], g, log_mod) != H.per_element_degrees(groups[b], g, log_mod)
        mutant = H.blind_rotate(accs[b], lwes[b], words, base_log, level, g, degrees=H.per_element_degrees)
        assert mutant != want[b]
    assert rotate(engine, key, accs, lwes) == want


# ---- saturation ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,k,base_log,level,g", [PRODUCTION, (2048, 1, 23, 1, 2)])
def test_saturation(engine, n, k, base_log, level, g):
    w, n_limbs = H.limb_rule(n, k, base_log, level, g)
    kinds = ("plus", "minus", "index0")
    glwe = [[R.saturating_poly(base_log, level, n, kind)] * (k + 1) for kind in kinds]
    plus, minus = (R.saturating_digits(base_log, level, neg) for neg in (False, True))
    for kind, ct in zip(kinds, glwe):  # the digits the helper decomposes are the extreme ones
        for e in (0, 1, n - 1):
            want = plus if kind == "plus" or (kind == "index0" and e == 0) else minus
            assert R.py_decompose(ct[0][e], base_log, level) == want
    # every degree is 0, so the 2^g GGSWs of the group add up in one column: on this input w holds and a limb one bit
    # wider would leave (-p/2, p/2)
    rows_sum = (1 << g) * (k + 1) * n * sum(plus)
    assert rows_sum * ((1 << w) - 1) <= (P - 1) // 2 < rows_sum * ((1 << (w + 1)) - 1)
    lwes = [[0] * (g + 1)] * len(kinds)  # an all-zero mask group and body: nothing is rotated
    assert H.subset_degrees([0] * g, g, n.bit_length()) == [0] * (1 << g)
    shape = (1, 1 << g, level, k + 1, k + 1, n, 2)
    full = np.full(shape, R.MASK64, np.uint64)
    one_limb = np.broadcast_to(R.to_words([((1 << w) - 1) << w])[0], shape).copy()
    for words in (full, one_limb):
        key = make_key(engine, words, base_log, level, g)
        assert (key.limb_bits, key.n_limbs) == (w, n_limbs)
        want = [H.blind_rotate(ct, lwe, words, base_log, level, g) for ct, lwe in zip(glwe, lwes)]
        assert rotate(engine, key, glwe, lwes) == want


# ---- several groups, two chunks, the PBS ----------------------------------------------------------------------------------------

class RotateCase:
    """One shape's key of three groups, LUT and LWEs, with the helper's rotation of the LUT computed once."""

    def __init__(self, engine, n, k, base_log, level, g):
        self.shape = (n, k, base_log, level, g)
        rng = R.rng(31 * n + base_log + g)
        log_mod = n.bit_length()
        self.words = H.uniform_key_words(rng, 3, g, k, n, level)
        self.key = make_key(engine, self.words, base_log, level, g)
        self.lut = R.uniform_glwe(rng, k, n)
        bodies = [0, n, 2 * n - 1, int(rng.integers(0, 2 * n)), int(rng.integers(0, 2 * n))]
        special = [0, 1, n - 1, n, 2 * n - 1]
        self.lwes = []
        for b in range(BATCH):
            mask = random_mask(rng, 3 * g)
            mask[b % (3 * g)] = word_for(rng, special[b], log_mod)
            self.lwes.append(mask + [word_for(rng, bodies[b], log_mod)])
        self._rotated = None

    def rotated(self):
        if self._rotated is None:
            _, _, base_log, level, g = self.shape
            self._rotated = [H.blind_rotate([list(p) for p in self.lut], lwe, self.words, base_log, level, g)
                             for lwe in self.lwes]
        return self._rotated


_CASES = {}


@pytest.fixture
def rotate_case(engine, request):
    shape = request.param
    if shape not in _CASES:
        _CASES[shape] = RotateCase(engine, *shape)
    return _CASES[shape]


@pytest.mark.parametrize("rotate_case", ROTATE_SHAPES, indirect=True)
def test_pbs(engine, rotate_case):
    import torch

    case = rotate_case
    n, k = case.shape[:2]
    lwe_h = np.array(case.lwes, dtype=np.uint64)
    lwe = dev(lwe_h)
    out = torch.zeros((BATCH, k * n + 1, 2), dtype=torch.int64, device="cuda")
    engine.pbs128.multi_bit_programmable_bootstrap_f128_lwe_ciphertext(lwe, out, dev128(case.lut), case.key)
    assert host128(out) == [R.sample_extract(acc) for acc in case.rotated()]
    assert np.array_equal(lwe.cpu().numpy().view(np.uint64), lwe_h), "the input LWEs are left as they were"


@pytest.mark.parametrize("rotate_case", ROTATE_SHAPES, indirect=True)
def test_several_groups_two_chunks(engine, rotate_case, monkeypatch):
    """n_lwe = 3 g, and the chunk bound forced below the batch (MI_PBS128_CHUNK, read per call): 5 items run as chunks
    of 2, 2 and 1.  Both runs equal the helper, so they equal each other."""
    import torch

    case = rotate_case
    n, k = case.shape[:2]
    lwe = dev(np.array(case.lwes, dtype=np.uint64))
    whole = rotate(engine, case.key, [case.lut] * BATCH, case.lwes)
    monkeypatch.setenv("MI_PBS128_CHUNK", "2")
    # that the bound took effect is read off the scratch pool, as tests/test_pbs128_gpu.py::test_two_chunks reads it
    per = (k + 1) * n
    item_bytes = 8 * (per * case.shape[3] + per * case.key.n_limbs + 2 * per + 1)

    def mib(items):
        return -(-items * item_bytes // (1 << 20)) << 20

    torch.cuda.synchronize()
    engine.ntt64_pbs.scratch_trim(0)
    assert engine.ntt64_pbs.scratch_bytes(0) == 0
    chunked = rotate(engine, case.key, [case.lut] * BATCH, case.lwes)
    torch.cuda.synchronize()
    assert engine.ntt64_pbs.scratch_bytes(0) == mib(2)
    if case.shape == PRODUCTION:
        assert mib(2) < mib(BATCH)
    out = torch.zeros((BATCH, k * n + 1, 2), dtype=torch.int64, device="cuda")
    engine.pbs128.multi_bit_programmable_bootstrap_f128_lwe_ciphertext(lwe, out, dev128(case.lut), case.key)
    assert chunked == whole
    assert whole == case.rotated()
    assert host128(out) == [R.sample_extract(acc) for acc in case.rotated()]


# ---- the full length, in closed form ----------------------------------------------------------------------------------------------

def test_full_length_gadget_key(engine):
    """n_lwe = 920 at the production shape: noise-free gadget GGSWs of known key bits, built on the device.  A step then
    multiplies the accumulator by X^(degree of the set-bit subset) (closest_representable is the identity on a LUT that
    keeps only the bits the decomposition represents), so the PBS is one monomial rotation of the LUT."""
    import torch

    n, k, base_log, level, g = PRODUCTION
    n_lwe, batch = 920, 2
    rng = R.rng(920)
    log_mod = n.bit_length()
    sk = R.binary_key(rng, n_lwe)
    groups = n_lwe // g
    sel = [H.selected_index(sk[i * g:(i + 1) * g]) for i in range(groups)]
    bsk = torch.zeros((groups, 1 << g, level, k + 1, k + 1, n, 2), dtype=torch.int64, device="cuda")
    gi, si = torch.arange(groups, device="cuda"), torch.tensor(sel, device="cuda")
    for li in range(level):
        f = R.to_words([1 << (128 - base_log * (level - li))])[0].view(np.int64)
        for r in range(k + 1):
            for word in (0, 1):
                bsk[gi, si, li, r, r, 0, word] = int(f[word])
    key = engine.pbs128.LweMultiBitBootstrapKey128(bsk, base_log, level, g)
    del bsk
    assert (key.limb_bits, key.n_limbs, key.input_lwe_dimension) == (22, 6, n_lwe)
    keep = R.MASK128 ^ ((1 << (128 - base_log * level)) - 1)
    lut = [[x & keep for x in p] for p in R.uniform_glwe(rng, k, n)]
    assert all(R.closest_representable(x, base_log, level) == x for x in lut[0][:64])
    lwes = [random_mask(rng, n_lwe + 1) for _ in range(batch)]
    want = []
    for lwe in lwes:
        exponent = -(R.modulus_switch(lwe[-1], log_mod) % (2 * n))
        for i in range(groups):
            s = sum(a for a, bit in zip(lwe[i * g:(i + 1) * g], sk[i * g:(i + 1) * g]) if bit) & R.MASK64
            assert H.subset_degrees(lwe[i * g:(i + 1) * g], g, log_mod)[sel[i]] == R.modulus_switch(s, log_mod) % (2 * n)
            exponent += R.modulus_switch(s, log_mod)
        want.append(R.sample_extract([R.monomial_mul(p, exponent % (2 * n)) for p in lut]))
    out = torch.zeros((batch, k * n + 1, 2), dtype=torch.int64, device="cuda")
    engine.pbs128.multi_bit_programmable_bootstrap_f128_lwe_ciphertext(dev(np.array(lwes, dtype=np.uint64)), out,
                                                                       dev128(lut), key)
    assert host128(out) == want


# ---- real keys ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("g", [2, 3, 4])
def test_real_key_every_message(engine, g):
    """A real multi-bit key (TUniform(30) noise) over an LWE key of dimension 12 at N = 512, k = 1, base 2^23, 3 levels:
    every message of the 4-bit space and its padding bit decrypts through the PBS to itself, and the output is the
    helper's."""
    import torch

    n, k, base_log, level, n_lwe = 512, 1, 23, 3, 12
    rng = R.rng(2025 + g)
    lwe_sk = R.binary_key(rng, n_lwe)
    glwe_sk = [R.binary_key(rng, n) for _ in range(k)]
    words = H.key_words(H.bsk_gen(rng, lwe_sk, glwe_sk, base_log, level, 30, g))
    key = make_key(engine, words, base_log, level, g)
    msg_mod = 16  # 4 message bits and the padding bit
    delta64, delta128 = 1 << 59, 1 << 123
    lut = R.pbs_lut(n, k, msg_mod, delta128, lambda m: m)
    lwes = [R.lwe_encrypt_u64(rng, m * delta64, lwe_sk) for m in range(msg_mod)]
    out = torch.zeros((msg_mod, k * n + 1, 2), dtype=torch.int64, device="cuda")
    engine.pbs128.multi_bit_programmable_bootstrap_f128_lwe_ciphertext(dev(np.array(lwes, dtype=np.uint64)), out,
                                                                       dev128(lut), key)
    got = host128(out)
    flat_sk = [s for poly in glwe_sk for s in poly]
    assert [R.decode(R.lwe_decrypt_u128(ct, flat_sk), delta128, msg_mod) for ct in got] == list(range(msg_mod))
    assert got == [H.pbs(lut, lwe, words, base_log, level, g) for lwe in lwes]


# ---- errors -----------------------------------------------------------------------------------------------------------------------

def test_errors(engine):
    import torch
    from tfhe_ntt_amd import _lib

    n, k, base_log, level, g = 256, 1, 23, 1, 2
    rng = R.rng(11)
    M, L = engine.pbs128, _lib.lib()
    words = H.uniform_key_words(rng, 2, g, k, n, level)
    bsk = dev(words)
    plan = engine.Plan.cached(n, P)

    def create(plan_h, ptr, n_lwe, kk, nn, b, l, gg, out=True):
        h = ctypes.c_void_p(0x5E5E)
        st = L.mi_pbs128_multi_bit_key_create(plan_h, ptr, n_lwe, kk, nn, b, l, gg, None, ctypes.byref(h) if out else None)
        assert not out or h.value is None or st == _lib.MI_OK, "a failed create leaves *out_key NULL"
        return st, (L.mi_last_error_message() or b"").decode(), h

    ptr = bsk.data_ptr()
    assert create(plan.handle, ptr, 4, k, n, base_log, level, g, out=False)[:2] == (_lib.MI_ERR_INVALID_ARG, "out_key is NULL")
    assert create(None, ptr, 4, k, n, base_log, level, g)[:2] == (_lib.MI_ERR_INVALID_ARG, "plan is NULL")
    assert create(plan.handle, None, 4, k, n, base_log, level, g)[:2] == (_lib.MI_ERR_INVALID_ARG, "bsk_std is NULL")
    for bad in (0, 1, 5):
        assert create(plan.handle, ptr, 4 if bad != 5 else 5, k, n, base_log, level, bad)[:2] == \
            (_lib.MI_ERR_INVALID_ARG, "grouping factor must be 2, 3 or 4")
    for bad in (0, 3, 5):
        st, msg, _ = create(plan.handle, ptr, bad, k, n, base_log, level, g)
        assert st == _lib.MI_ERR_INVALID_ARG and "lwe dimension" in msg
    assert create(plan.handle, ptr, 4, k, n, 64, 2, g)[0] == _lib.MI_ERR_INVALID_ARG
    st, msg, _ = create(plan.handle, ptr, 4, k, n, 50, 1, g)  # 43 limbs of 3 bits
    assert st == _lib.MI_ERR_UNSUPPORTED and "32 limbs" in msg and H.limb_rule(n, k, 50, 1, g)[1] > 32
    assert create(plan.handle, ptr, 4, 4, n, base_log, level, g)[0] == _lib.MI_ERR_UNSUPPORTED
    with pytest.raises(engine.MiError) as err:  # a plan of another prime
        M.LweMultiBitBootstrapKey128(bsk, base_log, level, g, plan=engine.Plan.try_new(n, 0x3F5A0001))
    assert err.value.status == _lib.MI_ERR_UNSUPPORTED
    with pytest.raises(engine.MiError) as err:  # the Goldilocks plan of another N
        M.LweMultiBitBootstrapKey128(bsk, base_log, level, g, plan=engine.Plan.try_new(2 * n, P))
    assert err.value.status == _lib.MI_ERR_UNSUPPORTED
    assert "Goldilocks plan of the key's polynomial size" in str(err.value)
    with pytest.raises(ValueError):  # 2^g GGSWs per group
        M.LweMultiBitBootstrapKey128(bsk, base_log, level, 3)

    key = M.LweMultiBitBootstrapKey128(bsk, base_log, level, g)
    n_lwe = 2 * g
    assert L.mi_pbs128_multi_bit_key_info(None, *[None] * 8) == _lib.MI_ERR_INVALID_ARG
    assert L.mi_pbs128_multi_bit_key_destroy(None) == _lib.MI_OK
    # overlapping buffers: nothing is written.  One block holds an accumulator and, inside it, what is passed as lwe_in
    acc_h = R.to_words([R.uniform_glwe(rng, k, n) for _ in range(2)])
    block = dev(acc_h)
    base, item = block.data_ptr(), (k + 1) * n * 16
    for acc_p, in_p, batch in ((base, base, 1), (base, base + item - 8, 1), (base, base + 2 * item - 8, 2),
                               (base + 16, base, 1)):
        assert L.mi_pbs128_multi_bit_blind_rotate_batch(key._h, acc_p, in_p, batch, None) == _lib.MI_ERR_INVALID_ARG
        assert L.mi_last_error_message() == b"buffers overlap"
    lwe = dev(np.array([random_mask(rng, n_lwe + 1)], dtype=np.uint64))
    for out_p, in_p, lut_p in ((base, base, base + item), (base, lwe.data_ptr(), base), (base, lwe.data_ptr(), base + 4096)):
        assert L.mi_pbs128_multi_bit_batch(key._h, out_p, in_p, lut_p, 1, None) == _lib.MI_ERR_INVALID_ARG
        assert L.mi_last_error_message() == b"buffers overlap"
    assert L.mi_pbs128_multi_bit_blind_rotate_batch(key._h, base + 8, lwe.data_ptr(), 1, None) == _lib.MI_ERR_INVALID_ARG
    assert L.mi_last_error_message() == b"u128 buffers must be 16-byte aligned"
    torch.cuda.synchronize()
    assert np.array_equal(block.cpu().numpy().view(np.uint64), acc_h)
    # NULL arguments and the empty batch
    assert L.mi_pbs128_multi_bit_blind_rotate_batch(None, base, lwe.data_ptr(), 1, None) == _lib.MI_ERR_INVALID_ARG
    assert L.mi_last_error_message() == b"key is NULL"
    assert L.mi_pbs128_multi_bit_batch(None, None, None, None, 0, None) == _lib.MI_ERR_INVALID_ARG
    assert L.mi_pbs128_multi_bit_blind_rotate_batch(key._h, None, None, 0, None) == _lib.MI_OK
    assert L.mi_pbs128_multi_bit_batch(key._h, None, None, None, 0, None) == _lib.MI_OK
    assert L.mi_pbs128_multi_bit_blind_rotate_batch(key._h, None, lwe.data_ptr(), 1, None) == _lib.MI_ERR_INVALID_ARG
    assert L.mi_last_error_message() == b"acc_glwe is NULL"
    assert L.mi_pbs128_multi_bit_blind_rotate_batch(key._h, base, None, 1, None) == _lib.MI_ERR_INVALID_ARG
    assert L.mi_last_error_message() == b"buffer is NULL"
    for args in ((None, lwe.data_ptr(), base), (base, None, base + item), (base, lwe.data_ptr(), None)):
        assert L.mi_pbs128_multi_bit_batch(key._h, *args, 1, None) == _lib.MI_ERR_INVALID_ARG
        assert L.mi_last_error_message() == b"buffer is NULL"
    torch.cuda.synchronize()
    assert np.array_equal(block.cpu().numpy().view(np.uint64), acc_h)
    # the tensor checks of the Python layer
    acc = dev(acc_h)
    with pytest.raises(ValueError):
        M.multi_bit_blind_rotate_assign(key, acc, dev(np.zeros((2, n_lwe), np.uint64)))
    with pytest.raises(ValueError):
        M.multi_bit_blind_rotate_assign(key, acc[:, :, : n // 2], dev(np.zeros((2, n_lwe + 1), np.uint64)))
    out = torch.zeros((2, k * n + 1, 2), dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError):  # one accumulator is shared by the batch
        M.multi_bit_programmable_bootstrap_f128_lwe_ciphertext(dev(np.zeros((2, n_lwe + 1), np.uint64)), out, acc, key)
