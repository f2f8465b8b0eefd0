"""Worst-case limb-range model of smartbft_amd/csrc/ed25519_f25.hpp, in the manner of
tests/test_f29_bounds.py but by interval propagation: every limb is an interval [lo, hi], every
operation of the header is restated on intervals, and each 64-bit column accumulator (the sum of
the magnitudes of its terms, so any summation order is covered) and each 32-bit limb is checked
against the width the GPU computes in. The classes are the ones the header's comments state
(T: limbs 0..7 in [-2^17, 2^29 + 2^17], limb 8 in [-2^17, 2^23 + 2^17]); the compositions are the
ones the kernel runs: the doubling, both additions, ge_complete, the table build, the
exponentiation chains, the square-root ratio, decoding and encoding. Stored point coordinates
are taken as T or its negative (the kernel negates A and table entries), i.e. symmetric."""
import os
import re

from conftest import ROOT

I64 = 1 << 63
I32 = 1 << 31
M29 = (1 << 29) - 1
M23 = (1 << 23) - 1
T_HI = [2**29 + 2**17] * 8 + [2**23 + 2**17]
T = [(-2**17, h) for h in T_HI]                # a product's class
S = [(-h, h) for h in T_HI]                    # T or its negative
C = [(0, M29)] * 8 + [(0, M23)]                # canonical limbs (constants, decoded bytes)


def fits32(iv):
    assert -I32 <= iv[0] and iv[1] < I32, ("32-bit limb overflow", iv)
    return iv


def mag(iv):
    return max(abs(iv[0]), abs(iv[1]))


def within(a, cls):
    for x, c in zip(a, cls):
        assert c[0] <= x[0] and x[1] <= c[1], ("outside the stated class", x, c)
    return a


def prod(x, y):
    c = [x[0] * y[0], x[0] * y[1], x[1] * y[0], x[1] * y[1]]
    return (min(c), max(c))


def isum(ivs):
    return (sum(i[0] for i in ivs), sum(i[1] for i in ivs))


def add(a, b):
    return [fits32((x[0] + y[0], x[1] + y[1])) for x, y in zip(a, b)]


def sub(a, b):
    return [fits32((x[0] - y[1], x[1] - y[0])) for x, y in zip(a, b)]


def neg(a):
    return [(-x[1], -x[0]) for x in a]


def column(acc, terms):
    """acc + sum(terms) as an interval, with |acc| + sum |term| checked against int64."""
    assert mag(acc) + sum(mag(t) for t in terms) < I64, "64-bit accumulator overflow"
    return isum([acc] + terms)


def shr(iv, n):
    return (iv[0] >> n, iv[1] >> n)


def finish(acc):
    """fe_finish: limbs 0..7 in [0, 2^29) below column 8's accumulator."""
    t = shr(acc, 23)
    z = (19 * t[0], M29 + 19 * t[1])
    c = shr(z, 29)
    out = [(0, M29), fits32((c[0], M29 + c[1]))] + [(0, M29)] * 6 + [(0, M23)]
    return within(out, T)


def mul(a, b, sq=False):
    """fe_mul / fe_sqr: columns 9..16 carried into h, then columns 0..8 with 1216 h[k]."""
    for x in a + b:
        fits32(x)
    if sq:
        for x in a:
            fits32((2 * x[0], 2 * x[1]))  # the doubled operand
    acc = (0, 0)
    h = []
    for k in range(9, 17):
        acc = column(acc, [prod(a[i], b[k - i]) for i in range(k - 8, 9)])
        h.append((0, M29))
        acc = shr(acc, 29)
    h.append(fits32(acc))
    acc = (0, 0)
    for k in range(9):
        acc = column(acc, [prod(a[i], b[k - i]) for i in range(k + 1)] + [prod(h[k], (1216, 1216))])
        if k < 8:
            acc = shr(acc, 29)
    return finish(acc)


def sqr(a):
    return mul(a, a, sq=True)


def weak(a):
    for x in a:
        fits32(x)
    c = [shr(x, 29) for x in a[:8]] + [shr(a[8], 23)]
    out = [fits32((19 * c[8][0], M29 + 19 * c[8][1]))]
    out += [(c[i - 1][0], M29 + c[i - 1][1]) for i in range(1, 8)]
    out.append((c[7][0], M23 + c[7][1]))
    return within(out, T)


def complete(p, want_t=True):
    x, y, z, t = p
    out = [mul(x, t), mul(y, z), mul(z, t)]
    if want_t:
        out.append(mul(x, y))
    return out


def dbl(p):
    x, y, z = p[:3]
    xx, yy, zz = sqr(x), sqr(y), sqr(z)
    s = sqr(weak(add(x, y)))
    ry = add(yy, xx)
    rz = sub(yy, xx)
    rx = weak(sub(s, ry))
    rt = weak(sub(add(zz, zz), rz))
    return [rx, ry, rz, rt]


def add_tail(a, b, c, d2):
    return [sub(a, b), add(a, b), weak(add(d2, c)), sub(d2, c)]


def madd(p, q):
    x, y, z, t = p
    ypx, ymx, xy2d = q
    return add_tail(mul(add(y, x), ypx), mul(sub(y, x), ymx), mul(xy2d, t), add(z, z))


def gadd(p, q):
    x, y, z, t = p
    ypx, ymx, qz, t2d = q
    zz = mul(z, qz)
    return add_tail(mul(add(y, x), ypx), mul(sub(y, x), ymx), mul(t2d, t), add(zz, zz))


def to_cached(p):
    x, y, z, t = p
    return [weak(add(y, x)), weak(sub(y, x)), z, mul(t, C)]


def test_header_states_the_classes_modelled_here():
    src = open(os.path.join(ROOT, "smartbft_amd", "csrc", "ed25519_f25.hpp")).read()
    assert re.search(r"T\s+\(tight\):\s+v\[0\.\.7\] in \[-2\^17, 2\^29 \+ 2\^17\], v\[8\] in \[-2\^17, 2\^23 \+ 2\^17\]", src)
    assert re.search(r"C\s+\(canonical limbs\): v\[0\.\.7\] in \[0, 2\^29\), v\[8\] in \[0, 2\^23\)", src)
    assert "sum_{i+j=k} |a[i]| |b[j]| + 2^42" in src


def test_products_of_the_stated_classes():
    two_t = add(S, S)
    for a, b in ((T, T), (S, S), (two_t, S), (two_t, C), (S, two_t)):
        mul(a, b)
    sqr(S)
    try:
        mul(two_t, two_t)  # the header says this one does not hold: the model must agree
    except AssertionError:
        pass
    else:
        raise AssertionError("2T x 2T passed: the model is weaker than the header's contract")


def test_doubling_and_additions_stay_in_range():
    p = [S, S, S, S]
    for want_t in (False, True):
        for q in complete(dbl(p), want_t):
            within(q, T)
    pre = [C, C, [(-x[1], x[1]) for x in C]]  # an affine entry or its negative
    for q in complete(madd(p, pre)):
        within(q, T)
    cached = [S, S, S, S]  # entries as stored (T) or negated on load
    for q in complete(gadd(p, cached)):
        within(q, T)
    for q in to_cached(p):
        within(q, S)


def test_table_build_and_ladder_compose():
    """tab_build (additions of the cached P to a running point) and one ladder step (four
    doublings, a mixed addition, an addition), each fed what the previous one produced."""
    p = [S, S, [(1, 1)] + [(0, 0)] * 8, S]  # the decoded, negated A: Z = 1
    c1 = to_cached(p)
    cur = p
    for _ in range(7):
        cur = complete(gadd(cur, c1))
        to_cached(cur)
    r = [[(0, 0)] * 9, [(1, 1)] + [(0, 0)] * 8, [(1, 1)] + [(0, 0)] * 8, [(0, 0)] * 9]  # identity
    pre = [C, C, [(-x[1], x[1]) for x in C]]
    for _ in range(3):
        for _ in range(4):
            r = complete(dbl(r))
        r = complete(madd(r, pre))
        r = complete(gadd(r, [S, S, S, S]))
        for q in r:
            within(q, T)


def test_chains_decode_and_encode():
    # the exponentiation chains square and multiply products only: T is closed under both
    within(sqr(T), T)
    within(mul(T, T), T)
    # ge_frombytes: y (C), u = y^2 - 1, v = d y^2 + 1; fe_sqrt_ratio brings both to T first
    one = [(1, 1)] + [(0, 0)] * 8
    y2 = sqr(C)
    u, v = weak(sub(y2, one)), weak(add(mul(y2, C), one))
    v3 = mul(sqr(v), v)
    v7 = mul(sqr(v3), v)
    mul(u, v7)
    r = mul(mul(u, v3), T)
    mul(v, sqr(r))
    mul(neg(u), C)
    r = mul(r, C)
    x = [(-a[1], a[1]) for a in r]  # negated when odd, and again for -A
    mul(x, C)                       # T = X Y
    # fe_tobytes takes anything below 2^31 - 2^24 in magnitude: the widest value it is given is
    # a difference of products (check = v r^2 against -u)
    for a in (T, S, sub(T, T), neg(u)):
        for lim in a:
            assert mag(lim) < I32 - (1 << 24)
    # unmasked self-test operands: limb 8 holds 24 bits
    full = [(0, M29)] * 8 + [(0, (1 << 24) - 1)]
    within(mul(full, full), T)
    within(sqr(full), T)
