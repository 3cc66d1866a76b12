"""The modular arithmetic of every GPU transform and pointwise path on its carry corners (`-m gpu`), bit-exact against
the oracle.

Every other GPU test of these paths feeds uniform random residues, which take the correction arms of the 32-bit-limb
arithmetic (csrc/mi_arith.hpp: the borrow fix of Goldilocks::reduce128, the "no carry but >= p" arms of add and
reduce128, Montgomery's wrapped sums, Shoup32's r = p) with probability about 2^-32.  Here the operands come from the
limb-corner corpus of tests/arith_corners.py:

* pointwise ops at N = 64 on the whole operand grid values(p) x values(p): the direct window onto mul and add, on the
  three access paths (contiguous, odd stride, even stride > N), with mul_accumulate's c placed so that c + a b is
  itself a corner; Solinas, p64 (plus the operands that reach Montgomery's `t < s` arm), p62, p30 and prime32 plans;
* transforms on rows(n, p), forward and inverse: Solinas 2^4 ... 2^17 (every window kernel, the one-launch split
  transform also on a padded stride, the tile passes of 2^15 / 2^16, the two plain top passes of 2^17) and 2^19 / 2^20
  (the K = 4 / K = 5 top passes off stage 0), generic primes at 2^4, 2^5, 2^10, 2^11, 2^12 and 2^15 (the large-N
  passes in Montgomery and Shoup32 form), prime32 plans at 32, 1024, 2048, 32768;
* N = 2048 Solinas (the asm bodies) as its own batch and inside a ragged batch of 2051 rows;
* the Ntt64View bodies at N = 2048: forward, forward_normalized, add_backward, forward_from_power_of_two_modulus(64).

Mutants (one-line edits of mi_arith.hpp, the library rebuilt for each; "old" = tests/test_ntt_gpu.py +
tests/test_native_gpu.py as they were, "new" = this file, "host" = tests/test_arith_host.py's program):

| mutant of mi_arith.hpp                          | host check | old GPU files          | this file  |
|-------------------------------------------------|------------|------------------------|------------|
| 1 Goldilocks::add without `|| s >= P`           | fails      | pass (106)             | 28 fail    |
| 2 reduce128 without the `t0 - GL_EPS` fix       | fails      | 26 fail (a)            | 39 fail    |
| 3 reduce128 without `|| r >= P`                 | fails      | pass (106)             | 39 fail    |
| 4 Montgomery::mul without `ov1 ||`              | fails      | 8 fail (b)             | 15 fail    |
| 5 Shoup32::mul `r > p` for `r >= p`             | fails      | pass (106)             | 2 fail (c) |

(a) mul_pow2 feeds reduce128 a low half whose low f bits are clear, so large shifts take the borrow at a rate near
    2^-16 and the tower-twiddle stages of uniform data find it; through mul the rate is 2^-33.
(b) ov1 is taken by about a quarter of uniform products at p64.
(c) On canonical operands mutant 5 computes the same function: r = p needs x w = 0 mod p.  It shows only on the
    product's wider domain x < 2^32, through the word p (test_shoup32_product_of_the_word_p).
"""
import numpy as np
import pytest

import arith_corners as AC

pytestmark = pytest.mark.gpu

P = AC.SOLINAS_P
M64 = (1 << 64) - 1


def _primes(oracle):
    f = oracle.largest_prime_in_arithmetic_progression64
    return {"solinas": P, "p64": f(1 << 16, 1, 1 << 63, 2**64 - 1), "p62": f(1 << 16, 1, 1 << 61, 1 << 62),
            "p30": 1062862849, "lo31": f(1 << 16, 1, 1 << 31, 1 << 32)}


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


def dev32(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.uint32).view(np.int32)).cuda()


def host32(t):
    return t.cpu().numpy().view(np.uint32).astype(np.uint64)


_CACHE = {}


def _operands(oracle, p, n):
    """(a, b, c) of shape (batch, n): the operand grid (for p > 2^63 also the pairs of Montgomery's `t < s` arm),
    padded to whole rows by repeating it, and the c that puts c + a b on the sum targets in turn."""
    key = ("ops", p, n)
    if key not in _CACHE:
        a, b = AC.grid(p)
        extra = AC.montgomery_wrap_pairs(p)
        a = np.concatenate([a, np.array([x for x, _ in extra], dtype=np.uint64)])
        b = np.concatenate([b, np.array([y for _, y in extra], dtype=np.uint64)])
        batch = -(-a.size // n)
        a, b = np.resize(a, batch * n), np.resize(b, batch * n)
        c = np.array([AC.accumulate_operand(p, int(x), int(y), k) for k, (x, y) in enumerate(zip(a, b))],
                     dtype=np.uint64)
        _CACHE[key] = tuple(v.reshape(batch, n) for v in (a, b, c))
    return _CACHE[key]


def _rows(oracle, n, p, inverse, limit=AC.MAX_ROWS):
    """rows(n, p) and its oracle transform, computed once per shape."""
    key = ("rows", n, p, inverse, limit)
    if key not in _CACHE:
        ora = oracle.Plan.try_new(n, p)
        # N = 2048 Solinas runs the asm bodies: their corpus (tests/test_tw_body_corners.py) holds rows(2048, P)
        x = AC.body_rows(oracle, "inv" if inverse else "fwd") if (n, p) == (2048, P) else \
            AC.rows(n, p, oracle, inverse, limit)
        _CACHE[key] = (x, (ora.inv if inverse else ora.fwd)(x, threads=8))
    return _CACHE[key]


def _padded(a, pad):
    """The rows of `a` inside a wider device buffer (row stride N + pad, the gap filled with 5): (buffer, view)."""
    full = np.concatenate([a, np.full((a.shape[0], pad), 5, np.uint64)], axis=1)
    t = dev(full)
    return t, t[:, :a.shape[1]]


@pytest.mark.parametrize("pad", [0, 1, 2], ids=["contiguous", "odd_stride", "even_stride"])
@pytest.mark.parametrize("name", ["solinas", "p64", "p62", "p30"])
def test_pointwise_operand_grid(engine, oracle, name, pad):
    p = _primes(oracle)[name]
    n = 64
    a, b, c = _operands(oracle, p, n)
    assert a.shape[0] >= 84 or p < (1 << 32)
    plan, ora = engine.Plan.try_new(n, p), oracle.Plan.try_new(n, p)
    tb, vb = _padded(b, pad)
    ta, va = _padded(a, pad)
    plan.normalize(va)
    assert np.array_equal(host(ta)[:, :n], ora.normalize(a))
    ta, va = _padded(a, pad)
    plan.mul_assign_normalize(va, vb)
    assert np.array_equal(host(ta)[:, :n], ora.mul_assign_normalize(a, b))
    ta, va = _padded(a, pad)
    tc, vc = _padded(c, pad)
    plan.mul_accumulate(vc, va, vb)
    assert np.array_equal(host(tc)[:, :n], ora.mul_accumulate(c, a, b))
    assert (host(tc)[:, n:] == 5).all() and np.array_equal(host(ta)[:, :n], a) and np.array_equal(host(tb)[:, :n], b)


@pytest.mark.parametrize("name", ["p30", "lo31"])
def test_pointwise_operand_grid_prime32(engine, oracle, name):
    p = _primes(oracle)[name]
    n = 64
    a, b, c = _operands(oracle, p, n)
    plan, ora = engine.prime32.Plan.try_new(n, p), oracle.Plan.try_new(n, p)
    t = dev32(a)
    plan.normalize(t)
    assert np.array_equal(host32(t), ora.normalize(a))
    t = dev32(a)
    plan.mul_assign_normalize(t, dev32(b))
    assert np.array_equal(host32(t), ora.mul_assign_normalize(a, b))
    t = dev32(c)
    plan.mul_accumulate(t, dev32(a), dev32(b))
    assert np.array_equal(host32(t), ora.mul_accumulate(c, a, b))


def _limit(logn):
    return AC.MAX_ROWS if logn <= 14 else 16 if logn <= 17 else 3


def _check_transform(engine, oracle, n, p, inverse, limit, pad=0):
    plan = engine.Plan.try_new(n, p)
    x, want = _rows(oracle, n, p, inverse, limit)
    full, view = _padded(x, pad)
    (plan.inv if inverse else plan.fwd)(view)
    got = host(full)
    assert np.array_equal(got[:, :n], want)
    assert (got[:, n:] == 5).all()


@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("logn", list(range(4, 18)) + [19, 20])
def test_transform_corner_rows_solinas(engine, oracle, logn, inverse):
    """2^11 runs the asm bodies, 2^12 ... 2^14 the one-launch split transform, 2^15 / 2^16 the K = 4 / 5 tile pass,
    2^17 two K = 3 passes (power-of-two twiddles at stage 0, table twiddles after it), 2^19 / 2^20 the K = 4 / 5 table
    passes."""
    _check_transform(engine, oracle, 1 << logn, P, inverse, _limit(logn))


@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("logn", [11, 12, 13, 14])
def test_transform_corner_rows_solinas_padded_stride(engine, oracle, logn, inverse):
    _check_transform(engine, oracle, 1 << logn, P, inverse, _limit(logn), pad=64)


@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("logn", [4, 5, 10, 11, 12, 15])
@pytest.mark.parametrize("name", ["p64", "p62", "p30"])
def test_transform_corner_rows_generic_primes(engine, oracle, name, logn, inverse):
    """Montgomery (p64, p62) and Shoup32 (p30, u64 buffers) window kernels; 2^15: their large-N passes."""
    _check_transform(engine, oracle, 1 << logn, _primes(oracle)[name], inverse, _limit(logn))


@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("n", [32, 1024, 2048, 32768])
@pytest.mark.parametrize("name", ["p30", "lo31"])
def test_transform_corner_rows_prime32(engine, oracle, name, n, inverse):
    p = _primes(oracle)[name]
    plan = engine.prime32.Plan.try_new(n, p)
    x, want = _rows(oracle, n, p, inverse, AC.MAX_ROWS if n <= 2048 else 8)
    t = dev32(x)
    (plan.inv if inverse else plan.fwd)(t)
    assert np.array_equal(host32(t), want)


@pytest.mark.parametrize("name", ["p30", "lo31"])
def test_shoup32_product_of_the_word_p(engine, oracle, name):
    """Shoup32::mul is exact for any x < 2^32 (r = x w - floor(x w' / 2^32) p < 2 p does not need x < p), and its
    r >= p comparison meets r = p only at x = p: for canonical x, r = p would need x w = 0 mod p.  The forward's first
    stage multiplies the upper half of the input by its twiddle before anything else touches it, so the word p there
    (and 2 p, p + 1 where they fit) is the one way to put r = p in front of the kernels; every later operand is
    canonical again.  u32 buffers (prime32 plans) and u64 buffers (the prime64 plan of the same modulus)."""
    p = _primes(oracle)[name]
    for n in (32, 1024):
        ora = oracle.Plan.try_new(n, p)
        x = AC.rows(n, p, oracle, False, 8)
        words = [w for w in (p, p + 1, 2 * p, 2 * p - 1, (1 << 32) - 1) if w < (1 << 32)]
        for r in range(x.shape[0]):
            x[r, n // 2 + r::7] = words[r % len(words)]
        want = ora.fwd(x)
        assert np.array_equal(want, ora.fwd(np.where(np.arange(n) >= n // 2, x % np.uint64(p), x))), \
            "the oracle reduces the product's operand"
        t = dev32(x)
        engine.prime32.Plan.try_new(n, p).fwd(t)
        assert np.array_equal(host32(t), want)
        t = dev(x)
        engine.Plan.try_new(n, p).fwd(t)
        assert np.array_equal(host(t), want)
        # In the forward a product p is indistinguishable from 0 (add and sub treat the word p as 0).  The inverse
        # stores its products: the word p at index 0 and zeros elsewhere stays the minuend of a zero at every stage,
        # d = p - 0 = p, and the product d w = 0 is what moves on (to index N - 1 in the end): all zeros out.
        e0 = np.zeros((2, n), dtype=np.uint64)
        e0[0, 0] = p
        e0[1, ::2] = p
        want = ora.inv(e0)
        assert not want[0].any()
        t = dev32(e0)
        engine.prime32.Plan.try_new(n, p).inv(t)
        assert np.array_equal(host32(t), want)
        t = dev(e0)
        engine.Plan.try_new(n, p).inv(t)
        assert np.array_equal(host(t), want)


def test_asm_bodies_corner_rows_in_a_ragged_batch(engine, oracle):
    """N = 2048 Solinas: the body corpus inside 2051 rows (not a multiple of the polynomials per workgroup), the rest
    random; the corpus sits at the batch's start, across its middle and at its very end."""
    n, batch = 2048, 2051
    plan, ora = engine.Plan.try_new(n, P), oracle.Plan.try_new(n, P)
    for inverse in (False, True):
        x, _ = _rows(oracle, n, P, inverse)
        full = oracle.fill_uniform(0xC0A7 + inverse, P, batch * n).reshape(batch, n)
        k = x.shape[0]
        third = k // 3
        full[:third] = x[:third]
        full[1021:1021 + third] = x[third:2 * third]
        full[batch - (k - 2 * third):] = x[2 * third:]
        t = dev(full)
        (plan.inv if inverse else plan.fwd)(t)
        assert np.array_equal(host(t), (ora.inv if inverse else ora.fwd)(full, threads=8))


def test_view_bodies_on_the_corpus(engine, oracle):
    """The Ntt64View bodies at N = 2048: forward / forward_normalized of rows(2048, P), add_backward of the inverse
    rows onto a standard operand placed so that standard + inv(ntt) lands on the sum targets, and
    forward_from_power_of_two_modulus(64) of the limb-corner words (any u64)."""
    n = 2048
    view = engine.ntt64.Ntt64(P, n).as_view()
    ctx = oracle.NttContext(n, P)
    x, _ = _rows(oracle, n, P, False)
    for fn, want in ((view.forward, ctx.forward(x)), (view.forward_normalized, ctx.forward_normalized(x))):
        dst = dev(np.zeros_like(x))
        fn(dst, dev(x))
        assert np.array_equal(host(dst), want)
    y, back = _rows(oracle, n, P, True)
    targets = AC.sum_targets(P)
    st = np.array([(targets[k % 6] - int(v)) % P for k, v in enumerate(back.reshape(-1))],
                  dtype=np.uint64).reshape(back.shape)  # st + v is the target itself wherever that leaves st < p
    want_st, want_y = ctx.add_backward(st, y)
    ts, ty = dev(st), dev(y)
    view.add_backward(ts, ty)
    assert np.array_equal(host(ty), want_y) and np.array_equal(host(ts), want_st)
    w = AC.body_rows(oracle, "fwd_ms64")  # limb-corner words, and native words that switch to the forward's corpus
    dst = dev(np.zeros_like(w))
    view.forward_from_power_of_two_modulus(64, dst, dev(w))
    assert np.array_equal(host(dst), ctx.forward_from_power_of_two_modulus(64, w))
