"""Pure-Python restatement of Go 1.24's crypto/ed25519.Verify (big integers + hashlib.sha512),
plus key generation and signing for test data. This is the reference every Ed25519 test of
the engine is checked against; tests/test_ed25519_cpu.py pins it to OpenSSL and Node.

The five rules (include/sbft_gpuverify.h carries the same text):
 1. A = decode(pub): y = low 255 bits reduced mod p (y >= p accepted), x from the square-root
    ratio of (y^2 - 1) / (d y^2 + 1) (no root: reject), the non-negative root, negated if bit
    255 is set (x = 0 with the sign bit set is accepted and stays 0). No small-order check.
 2. S = sig[32:64] little-endian must be < L.
 3. k = SHA-512(sig[0:32] || pub || msg) as a little-endian integer mod L.
 4. R' = [S]B - [k]A, no cofactor multiplication.
 5. encode(R') == sig[0:32] as bytes (R is never decoded).
"""
import hashlib

P = 2**255 - 19
L = 2**252 + 27742317777372353535851937790883648493
D = -121665 * pow(121666, -1, P) % P
SQRT_M1 = pow(2, (P - 1) // 4, P)
IDENT = (0, 1, 1, 0)


def sqrt_ratio(u, v):
    """(r, was_square) as Go's field.Element.SqrtRatio: r = sqrt(u/v) non-negative if u/v is a
    square, else sqrt(i u/v)."""
    v3 = v * v % P * v % P
    v7 = v3 * v3 % P * v % P
    r = u * v3 % P * pow(u * v7 % P, (P - 5) // 8, P) % P
    check = v * r % P * r % P
    u %= P
    ok = True
    if check == u:
        pass
    elif check == (-u) % P:
        r = r * SQRT_M1 % P
    elif check == (-u) * SQRT_M1 % P:
        r = r * SQRT_M1 % P
        ok = False
    else:
        ok = False
    if r & 1:
        r = P - r
    return r, ok


def decode(b):
    """Point.SetBytes: extended coordinates, or None."""
    y = (int.from_bytes(b, "little") & ((1 << 255) - 1)) % P
    y2 = y * y % P
    x, ok = sqrt_ratio((y2 - 1) % P, (D * y2 + 1) % P)
    if not ok:
        return None
    if b[31] >> 7:
        x = (-x) % P
    return (x, y, 1, x * y % P)


def add(p, q):
    x1, y1, z1, t1 = p
    x2, y2, z2, t2 = q
    a = (y1 - x1) * (y2 - x2) % P
    b = (y1 + x1) * (y2 + x2) % P
    c = 2 * D * t1 * t2 % P
    d = 2 * z1 * z2 % P
    e, f, g, h = b - a, d - c, d + c, b + a
    return (e * f % P, g * h % P, f * g % P, e * h % P)


def neg(p):
    return ((-p[0]) % P, p[1], p[2], (-p[3]) % P)


def mul(k, p):
    q = IDENT
    while k:
        if k & 1:
            q = add(q, p)
        p = add(p, p)
        k >>= 1
    return q


def encode(p):
    zi = pow(p[2], -1, P)
    x, y = p[0] * zi % P, p[1] * zi % P
    return (y | (x & 1) << 255).to_bytes(32, "little")


BY = 4 * pow(5, -1, P) % P
B = decode(BY.to_bytes(32, "little"))
assert B[0] == 15112221349535400772501151409588531511454012693041857206046113283949847762202


_B_POW2 = []


def mul_base(k):
    """[k]B from a cached table of 2^i B (half the work of mul for test-data generation)."""
    if not _B_POW2:
        p = B
        for _ in range(256):
            _B_POW2.append(p)
            p = add(p, p)
    q = IDENT
    i = 0
    while k:
        if k & 1:
            q = add(q, _B_POW2[i])
        k >>= 1
        i += 1
    return q


def verify(pub, msg, sig):
    if len(pub) != 32 or len(sig) != 64:
        return False
    a = decode(pub)
    if a is None:
        return False
    s = int.from_bytes(sig[32:], "little")
    if s >= L:
        return False
    k = int.from_bytes(hashlib.sha512(sig[:32] + pub + msg).digest(), "little") % L
    r = add(mul_base(s), neg(mul(k, a)))
    return encode(r) == sig[:32]


def _expand(seed):
    h = hashlib.sha512(seed).digest()
    a = int.from_bytes(h[:32], "little")
    a &= (1 << 254) - 8
    a |= 1 << 254
    return a, h[32:]


def public_key(seed):
    return encode(mul_base(_expand(seed)[0] % L))


def sign(seed, msg, pub=None):
    """RFC 8032 signing. pub overrides the key bytes that are hashed (for crafted records)."""
    a, prefix = _expand(seed)
    pub = pub or encode(mul_base(a % L))
    r = int.from_bytes(hashlib.sha512(prefix + msg).digest(), "little") % L
    rb = encode(mul_base(r))
    k = int.from_bytes(hashlib.sha512(rb + pub + msg).digest(), "little") % L
    return rb + ((r + k * a) % L).to_bytes(32, "little")
