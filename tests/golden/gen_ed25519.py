#!/usr/bin/env python3
"""Seeded generator of tests/golden/ed25519_vectors.bin and ed25519_categories.json.

Record: pub32 | sig64 | u16 len (little-endian) | msg | verdict | category. The verdict is the
reference's (tests/ed25519_ref.py, Go's crypto/ed25519.Verify restated); tests/test_ed25519_cpu.py
pins every record to OpenSSL and Node as well. Each category's first 15 records take the message
lengths that straddle SHA-512's padding boundaries behind the 64-byte R || A prefix; the rest
use short messages so the file stays below 200 KB.

Run: python3 tests/golden/gen_ed25519.py   (rewrites both files in place; --check compares)
"""
import hashlib
import json
import os
import random
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ed25519_ref as ref  # noqa: E402

CATEGORIES = ["valid", "flip_sig_r", "flip_sig_s", "flip_key", "flip_msg", "s_plus_l", "s_eq_l",
              "small_order_key", "noncanonical_key_sign0", "noncanonical_key_sign1",
              "r_identity_canonical", "r_identity_noncanonical", "r_identity_signbit",
              "mixed_order_key", "wrong_key"]
LENGTHS = [0, 1, 31, 32, 47, 48, 64, 111, 112, 113, 200, 239, 240, 241, 500]
SHORT = [0, 1, 31, 32]
PER_CATEGORY = 90
N_VALID = 150
P, L = ref.P, ref.L


def small_order_points(rng):
    """The eight points of order dividing 8, as multiples of one of order exactly 8."""
    while True:
        q = ref.decode(rng.randbytes(32))
        if q is None:
            continue
        t = ref.mul(L, q)
        if ref.encode(ref.mul(4, t)) != ref.encode(ref.IDENT):
            return [ref.mul(j, t) for j in range(8)]


def hash_k(rb, pub, msg):
    return int.from_bytes(hashlib.sha512(rb + pub + msg).digest(), "little") % L


def main():
    rng = random.Random(0x25519)
    out = []

    def msg_for(i):
        n = LENGTHS[i] if i < len(LENGTHS) else SHORT[i % len(SHORT)]
        return rng.randbytes(n)

    def emit(cat, pub, sig, msg):
        v = 1 if ref.verify(pub, msg, sig) else 0
        out.append((pub, sig, msg, v, CATEGORIES.index(cat)))
        return v

    def keypair():
        seed = rng.randbytes(32)
        return seed, ref.public_key(seed)

    def flip(b, lo, hi):
        i = rng.randrange(8 * lo, 8 * hi)
        x = bytearray(b)
        x[i // 8] ^= 1 << (i % 8)
        return bytes(x)

    # RFC 8032 section 7.1 TEST 1: the anchor
    seed = bytes.fromhex("9d61b19deffd5a60ba844af492ec2cc44449c5697b326919703bac031cae7f60")
    pub = ref.public_key(seed)
    sig = ref.sign(seed, b"")
    assert pub.hex() == "d75a980182b10ab7d54bfed3c964073a0ee172f3daa62325af021a68f707511a"
    assert sig.hex().startswith("e5564300c360ac72")
    assert emit("valid", pub, sig, b"") == 1
    for i in range(N_VALID - 1):
        seed, pub = keypair()
        m = msg_for(i)
        assert emit("valid", pub, ref.sign(seed, m), m) == 1

    for cat, lo, hi, what in (("flip_sig_r", 0, 32, "sig"), ("flip_sig_s", 32, 64, "sig"),
                              ("flip_key", 0, 32, "key"), ("flip_msg", 0, 0, "msg")):
        for i in range(PER_CATEGORY):
            seed, pub = keypair()
            m = msg_for(i)
            sig = ref.sign(seed, m)
            if what == "sig":
                sig = flip(sig, lo, hi)
            elif what == "key":
                pub = flip(pub, lo, hi)
            elif len(m):
                m = flip(m, 0, len(m))
            else:
                m = b"\x00"  # an empty message has no bit to flip: one byte appended
            emit(cat, pub, sig, m)

    for i in range(PER_CATEGORY):
        seed, pub = keypair()
        m = msg_for(i)
        sig = ref.sign(seed, m)
        s = int.from_bytes(sig[32:], "little") + L
        assert emit("s_plus_l", pub, sig[:32] + s.to_bytes(32, "little"), m) == 0
    for i in range(PER_CATEGORY):
        seed, pub = keypair()
        m = msg_for(i)
        sig = ref.sign(seed, m)
        rb = sig[:32] if i % 2 else ref.encode(ref.IDENT)
        assert emit("s_eq_l", pub, rb + L.to_bytes(32, "little"), m) == 0

    def craft_small(pub, a, m, want_accept):
        """A signature under a key a of small order: R = [s]B - j a accepts when k = j (mod 8)."""
        for _ in range(200):
            s = rng.randrange(L)
            sb = ref.mul_base(s)
            if not want_accept:  # R = [s]B - j a but S = s + 1: off by B, which has large order
                rb = ref.encode(ref.add(sb, ref.neg(ref.mul(rng.randrange(8), a))))
                return rb + ((s + 1) % L).to_bytes(32, "little")
            for j in range(8):
                rb = ref.encode(ref.add(sb, ref.neg(ref.mul(j, a))))
                if (ref.verify(pub, m, rb + s.to_bytes(32, "little"))) == want_accept:
                    return rb + s.to_bytes(32, "little")
        raise AssertionError("no signature found")

    small = small_order_points(rng)
    keys = [ref.encode(q) for q in small]
    ident_sign = bytes([1] + [0] * 30 + [0x80])          # y = 1, sign bit set: x = -0 = 0, accepted
    minus1_sign = (P - 1 | 1 << 255).to_bytes(32, "little")  # y = -1, sign bit set
    y0 = [bytes(32), bytes(31) + b"\x80"]
    assert y0[0] in keys and y0[1] in keys and bytes([1] + [0] * 31) in keys
    keys += [ident_sign, minus1_sign]
    for i in range(PER_CATEGORY):
        pub = keys[i % len(keys)]
        m = msg_for(i)
        emit("small_order_key", pub, craft_small(pub, ref.decode(pub), m, i % 3 != 2), m)

    for sign_bit, cat in ((0, "noncanonical_key_sign0"), (1, "noncanonical_key_sign1")):
        for i in range(PER_CATEGORY):
            y = i % 19
            pub = (y + P | sign_bit << 255).to_bytes(32, "little")
            m = msg_for(i)
            a = ref.decode(pub)
            if a is not None and ref.encode(ref.mul(8, a)) == ref.encode(ref.IDENT):
                sig = craft_small(pub, a, m, i % 3 != 2)
            else:  # off the curve, or a point of unknown discrete logarithm: nothing can verify
                seed, _ = keypair()
                sig = ref.sign(seed, m, pub=pub)
            emit(cat, pub, sig, m)

    # R' = identity: S = k a for the key A = a B
    forms = {"r_identity_canonical": bytes([1] + [0] * 31),
             "r_identity_noncanonical": (1 + P).to_bytes(32, "little"),
             "r_identity_signbit": ident_sign}
    for cat, rb in forms.items():
        for i in range(PER_CATEGORY):
            seed, pub = keypair()
            a = ref._expand(seed)[0]
            m = msg_for(i)
            s = hash_k(rb, pub, m) * a % L
            if cat == "r_identity_canonical" and i % 3 == 2:
                s = (s + 1) % L
            v = emit(cat, pub, rb + s.to_bytes(32, "little"), m)
            assert v == (1 if cat == "r_identity_canonical" and i % 3 != 2 else 0)

    # A' = A + T8: the honest signature under a verifies only when 8 | k
    acc = 0
    for i in range(PER_CATEGORY):
        seed, pub = keypair()
        mixed = ref.encode(ref.add(ref.decode(pub), small[1 + i % 7]))
        m = msg_for(i)
        acc += emit("mixed_order_key", mixed, ref.sign(seed, m, pub=mixed), m)
    assert 0 < acc < PER_CATEGORY

    for i in range(PER_CATEGORY):
        seed, _ = keypair()
        _, other = keypair()
        m = msg_for(i)
        assert emit("wrong_key", other, ref.sign(seed, m), m) == 0

    blob = b"".join(pub + sig + struct.pack("<H", len(m)) + m + bytes([v, c]) for pub, sig, m, v, c in out)
    cats = json.dumps({"categories": CATEGORIES}, indent=1) + "\n"
    assert len(blob) < 200_000, len(blob)
    bin_path = os.path.join(HERE, "ed25519_vectors.bin")
    json_path = os.path.join(HERE, "ed25519_categories.json")
    if "--check" in sys.argv:
        same = open(bin_path, "rb").read() == blob and open(json_path).read() == cats
        print("identical" if same else "DIFFERENT")
        sys.exit(0 if same else 1)
    open(bin_path, "wb").write(blob)
    open(json_path, "w").write(cats)
    per = [sum(1 for r in out if r[4] == c) for c in range(len(CATEGORIES))]
    ok = [sum(r[3] for r in out if r[4] == c) for c in range(len(CATEGORIES))]
    print(f"{len(out)} records, {len(blob)} bytes; per category (accepted/total):",
          ", ".join(f"{n}:{a}/{t}" for n, a, t in zip(CATEGORIES, ok, per)))


if __name__ == "__main__":
    main()
