// ed25519_f25.hpp — Ed25519 verification arithmetic: GF(2^255 - 19), scalars mod L, points of
// edwards25519 and the double-scalar multiplication of crypto/ed25519.Verify. One header for
// the device (ed25519_verify.hip) and the host (tests/native/ed25519_test.cpp compiles it with
// g++ -O2 -Wall -Werror and runs the kernel's algorithm on the CPU).
//
// Field. x = sum v[i] 2^(29 i), nine signed 32-bit limbs (radix 2^29, the shapes of
// p256_f29.hpp). Chosen by counting: a product is 81 multiply-adds (v_mad_i64_i32, 64-bit
// column accumulators) plus 9 for the fold 2^261 = 1216 (mod p) and one for 2^255 = 19, against
// 100 plus 19 pre-scalings for ten limbs of 25.5 bits. There is no Montgomery domain.
//
// Limb classes (tests/test_ed25519_bounds.py propagates them through every composition below):
//   T  (tight):  v[0..7] in [-2^17, 2^29 + 2^17], v[8] in [-2^17, 2^23 + 2^17]
//                every fe_mul / fe_sqr / fe_weak / fe_mul_small result is T
//   C  (canonical limbs): v[0..7] in [0, 2^29), v[8] in [0, 2^23)  (constants, fe_frombytes)
//   nT: the limb-wise sum or difference of n values of class T (|v[i]| <= n (2^29 + 2^17))
// Contract of fe_mul(a, b) and fe_sqr(a): for every column k, sum_{i+j=k} |a[i]| |b[j]| + 2^42
// < 2^63. T x T, 2T x T and 2T x C hold it; 2T x 2T does not (9 x 2^60), so sums are brought
// back to T with fe_weak (a carry step of 27 32-bit operations, no multiply) where two of them
// would meet. Every limb stays inside int32 (at most 3T < 2^31 before a fe_weak).
//
// Verification handles public data only: branches and memory addresses depend on it freely.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "sha512_dev.hpp"  // SBFT_ED_HD, SBFT_ED_UNROLL, ed25519_tables.inc

namespace sbft {
namespace ed {

typedef int32_t i32;
typedef int64_t i64;
typedef uint32_t u32;
typedef uint64_t u64;

#define SBFT_ED_M29 0x1FFFFFFF
#define SBFT_ED_M23 0x007FFFFF

struct fe {
    i32 v[9];
};

// acc + a b (signed 32 x 32 + 64): one v_mad_i64_i32 on the device. The empty asm keeps the
// accumulation a chain of mads (p256_f29.hpp's smad); the host form is the portable fallback.
SBFT_ED_HD i64 mac(i64 acc, i32 a, i32 b) {
    i64 r = (i64)a * (i64)b + acc;
#if defined(__HIP_DEVICE_COMPILE__)
    asm("" : "+v"(r));
#endif
    return r;
}
// low 29 bits as a limb whose range the compiler cannot see (p256_f29.hpp's lo29)
SBFT_ED_HD i32 lo29(i64 acc) {
    i32 t = (i32)((u32)acc & SBFT_ED_M29);
#if defined(__HIP_DEVICE_COMPILE__)
    asm("" : "+v"(t));
#endif
    return t;
}
// 2^261 mod p, in a register the compiler cannot turn into shifts and adds
SBFT_ED_HD i32 fold_const() {
    i32 c = 1216;
#if defined(__HIP_DEVICE_COMPILE__)
    asm("" : "+s"(c));
#endif
    return c;
}

// Shared tail of fe_mul / fe_sqr: acc is column 8's accumulator (|acc| < 2^63), o[0..7] the
// limbs below it in [0, 2^29). Bits 23 and up of column 8 weigh 2^255 = 19: t = acc >> 23,
// |t| <= 2^40, z = o[0] + 19 t, |z| < 2^44.3, so o[1] gains |z >> 29| < 2^15.3. Result: T.
SBFT_ED_HD void fe_finish(fe& r, i32 o[9], i64 acc) {
    o[8] = (i32)(acc & SBFT_ED_M23);
    const i64 z = (i64)o[0] + 19 * (acc >> 23);
    o[0] = lo29(z);
    o[1] += (i32)(z >> 29);
    SBFT_ED_UNROLL
    for (int i = 0; i < 9; ++i) r.v[i] = o[i];
}

// r = a b mod p. In: the contract above. Out: T (r[0], r[2..7] in [0, 2^29), r[1] within 2^15.3
// of that, r[8] in [0, 2^23)). Columns 9..16 are summed and carried first into h[0..8] (h[0..7]
// in [0, 2^29), |h[8]| < 2^31 since |column 16 + carry| < 2^60), then column k takes 1216 h[k]
// (< 2^42) with its own products. r may alias a or b.
SBFT_ED_HD void fe_mul(fe& r, const fe& a, const fe& b) {
    const i32 c1216 = fold_const();
    i32 h[9], o[9];
    i64 acc = 0;
    SBFT_ED_UNROLL
    for (int k = 9; k < 17; ++k) {
        SBFT_ED_UNROLL
        for (int i = k - 8; i < 9; ++i) acc = mac(acc, a.v[i], b.v[k - i]);
        h[k - 9] = lo29(acc);
        acc >>= 29;
    }
    h[8] = (i32)acc;
    acc = 0;
    SBFT_ED_UNROLL
    for (int k = 0; k < 9; ++k) {
        SBFT_ED_UNROLL
        for (int i = 0; i <= k; ++i) acc = mac(acc, a.v[i], b.v[k - i]);
        acc = mac(acc, h[k], c1216);
        if (k < 8) {
            o[k] = lo29(acc);
            acc >>= 29;
        }
    }
    fe_finish(r, o, acc);
}

// r = a^2 mod p: the off-diagonal products against the doubled operand (45 + 10 multiply-adds).
// In: fe_mul's contract with b = a, and |a[i]| < 2^30 (the doubled limb is an int32). Out: T.
SBFT_ED_HD void fe_sqr(fe& r, const fe& a) {
    const i32 c1216 = fold_const();
    i32 d[9], h[9], o[9];
    SBFT_ED_UNROLL
    for (int i = 0; i < 9; ++i) d[i] = 2 * a.v[i];
    i64 acc = 0;
    SBFT_ED_UNROLL
    for (int k = 9; k < 17; ++k) {
        SBFT_ED_UNROLL
        for (int i = k - 8; 2 * i < k; ++i) acc = mac(acc, a.v[i], d[k - i]);
        if (!(k & 1)) acc = mac(acc, a.v[k / 2], a.v[k / 2]);
        h[k - 9] = lo29(acc);
        acc >>= 29;
    }
    h[8] = (i32)acc;
    acc = 0;
    SBFT_ED_UNROLL
    for (int k = 0; k < 9; ++k) {
        SBFT_ED_UNROLL
        for (int i = 0; 2 * i < k; ++i) acc = mac(acc, a.v[i], d[k - i]);
        if (!(k & 1)) acc = mac(acc, a.v[k / 2], a.v[k / 2]);
        acc = mac(acc, h[k], c1216);
        if (k < 8) {
            o[k] = lo29(acc);
            acc >>= 29;
        }
    }
    fe_finish(r, o, acc);
}

// r = c a mod p for a small constant: |c| |a[i]| < 2^62. Out: T.
SBFT_ED_HD void fe_mul_small(fe& r, const fe& a, i32 c) {
    i32 o[9];
    i64 acc = 0;
    SBFT_ED_UNROLL
    for (int k = 0; k < 9; ++k) {
        acc = mac(acc, a.v[k], c);
        if (k < 8) {
            o[k] = lo29(acc);
            acc >>= 29;
        }
    }
    fe_finish(r, o, acc);
}

// limb-wise: nT + mT -> (n + m)T, no carries, no reduction
SBFT_ED_HD void fe_add(fe& r, const fe& a, const fe& b) {
    SBFT_ED_UNROLL
    for (int i = 0; i < 9; ++i) r.v[i] = a.v[i] + b.v[i];
}
SBFT_ED_HD void fe_sub(fe& r, const fe& a, const fe& b) {
    SBFT_ED_UNROLL
    for (int i = 0; i < 9; ++i) r.v[i] = a.v[i] - b.v[i];
}
SBFT_ED_HD void fe_neg(fe& r, const fe& a) {
    SBFT_ED_UNROLL
    for (int i = 0; i < 9; ++i) r.v[i] = -a.v[i];
}
// One parallel carry step. In: any int32 limbs. Out: r[0] in [-4864, 2^29 + 4864) (19 times the
// top carry, |carry| <= 2^8), r[1..7] in [-4, 2^29 + 4), r[8] in [-4, 2^23 + 4): T.
SBFT_ED_HD void fe_weak(fe& r, const fe& a) {
    i32 c[9];
    SBFT_ED_UNROLL
    for (int i = 0; i < 8; ++i) c[i] = a.v[i] >> 29;
    c[8] = a.v[8] >> 23;
    i32 o[9];
    o[0] = (a.v[0] & SBFT_ED_M29) + 19 * c[8];
    SBFT_ED_UNROLL
    for (int i = 1; i < 8; ++i) o[i] = (a.v[i] & SBFT_ED_M29) + c[i - 1];
    o[8] = (a.v[8] & SBFT_ED_M23) + c[7];
    SBFT_ED_UNROLL
    for (int i = 0; i < 9; ++i) r.v[i] = o[i];
}
SBFT_ED_HD void fe_set(fe& r, i32 x) {
    SBFT_ED_UNROLL
    for (int i = 0; i < 9; ++i) r.v[i] = 0;
    r.v[0] = x;
}
SBFT_ED_HD void fe_const(fe& r, const i32 (&c)[9]) {
    SBFT_ED_UNROLL
    for (int i = 0; i < 9; ++i) r.v[i] = c[i];
}

// Decode 8 little-endian words. mask_top: drop bit 255 (a point encoding's y); otherwise all
// 256 bits are taken (limb 8 then holds 24 bits). The value is not reduced: any residue will
// do, so y >= p is accepted as Go's SetBytes accepts it. Out: C (limb 8 < 2^24 unmasked).
SBFT_ED_HD void fe_frombytes(fe& r, const u32 w[8], bool mask_top) {
    SBFT_ED_UNROLL
    for (int i = 0; i < 9; ++i) {
        const int bit = 29 * i, j = bit >> 5, s = bit & 31;
        u32 x = w[j] >> s;
        if (s > 3 && j < 7) x |= w[j + 1] << (32 - s);
        r.v[i] = (i32)(x & SBFT_ED_M29);
    }
    if (mask_top) r.v[8] &= SBFT_ED_M23;
}

// sequential carry of limbs 0..7 into the next (no wrap): limbs 0..7 end in [0, 2^29)
SBFT_ED_HD void fe_carry_seq(i32 v[9]) {
    SBFT_ED_UNROLL
    for (int i = 0; i < 8; ++i) {
        v[i + 1] += v[i] >> 29;
        v[i] &= SBFT_ED_M29;
    }
}
// Canonical encoding: the unique value in [0, p) as 8 little-endian words. In: any limbs with
// |v[i]| < 2^31 - 2^24. Steps: one carry pass with the 19-wrap leaves x1 = x (mod p) in
// (-2^14, 2^255 + 2^14); adding p makes it positive and below 2^256; a second pass leaves y in
// [0, 2^255 + 19); y >= p exactly when y + 19 carries into bit 255.
SBFT_ED_HD void fe_tobytes(u32 w[8], const fe& a) {
    i32 v[9];
    SBFT_ED_UNROLL
    for (int i = 0; i < 9; ++i) v[i] = a.v[i];
    fe_carry_seq(v);
    v[0] += 19 * (v[8] >> 23);
    v[8] &= SBFT_ED_M23;
    v[0] -= 19;  // + p = 2^255 - 19
    v[8] += 1 << 23;
    fe_carry_seq(v);
    v[0] += 19 * (v[8] >> 23);
    v[8] &= SBFT_ED_M23;
    fe_carry_seq(v);  // v[8] <= 2^23 now, value y
    i32 t[9];
    SBFT_ED_UNROLL
    for (int i = 0; i < 9; ++i) t[i] = v[i];
    t[0] += 19;
    fe_carry_seq(t);
    const bool ge_p = (t[8] >> 23) != 0;
    t[8] &= SBFT_ED_M23;
    SBFT_ED_UNROLL
    for (int i = 0; i < 9; ++i) v[i] = ge_p ? t[i] : v[i];
    SBFT_ED_UNROLL
    for (int j = 0; j < 8; ++j) {
        const int i = (32 * j) / 29, s = 32 * j - 29 * i;  // word j starts at bit s of limb i
        u32 x = (u32)v[i] >> s;
        if (i < 8) x |= (u32)v[i + 1] << (29 - s);
        if (s > 26 && i < 7) x |= (u32)v[i + 2] << (58 - s);
        w[j] = x;
    }
}
SBFT_ED_HD bool words_eq(const u32 a[8], const u32 b[8]) {
    u32 x = 0;
    SBFT_ED_UNROLL
    for (int i = 0; i < 8; ++i) x |= a[i] ^ b[i];
    return x == 0;
}

SBFT_ED_HD void fe_sqr_n(fe& r, const fe& a, int n) {
    fe_sqr(r, a);
    SBFT_ED_UNROLL1
    for (int i = 1; i < n; ++i) fe_sqr(r, r);
}
// t250 = z^(2^250 - 1), z11 = z^11: the common head of the two exponentiation chains
// (249 squarings + 4 for z11's, 10 products). All operands T.
SBFT_ED_HD void fe_pow250(fe& t250, fe& z11, const fe& z) {
    fe t0, t1, t2, t3;
    fe_sqr(t0, z);            // 2
    fe_sqr_n(t1, t0, 2);      // 8
    fe_mul(t1, z, t1);        // 9
    fe_mul(t0, t0, t1);       // 11
    fe_sqr(t2, t0);           // 22
    fe_mul(t1, t1, t2);       // 2^5 - 1
    fe_sqr_n(t2, t1, 5);
    fe_mul(t1, t2, t1);       // 2^10 - 1
    fe_sqr_n(t2, t1, 10);
    fe_mul(t2, t2, t1);       // 2^20 - 1
    fe_sqr_n(t3, t2, 20);
    fe_mul(t2, t3, t2);       // 2^40 - 1
    fe_sqr_n(t2, t2, 10);
    fe_mul(t1, t2, t1);       // 2^50 - 1
    fe_sqr_n(t2, t1, 50);
    fe_mul(t2, t2, t1);       // 2^100 - 1
    fe_sqr_n(t3, t2, 100);
    fe_mul(t2, t3, t2);       // 2^200 - 1
    fe_sqr_n(t2, t2, 50);
    fe_mul(t250, t2, t1);     // 2^250 - 1
    z11 = t0;
}
// r = z^(p - 2) = z^(2^255 - 21) (0 for z = 0). In: T. Out: T. 254 squarings, 11 products.
SBFT_ED_HD void fe_invert(fe& r, const fe& z) {
    fe t, z11;
    fe_pow250(t, z11, z);
    fe_sqr_n(t, t, 5);
    fe_mul(r, t, z11);
}
// r = z^((p - 5) / 8) = z^(2^252 - 3). 251 squarings, 11 products.
SBFT_ED_HD void fe_pow22523(fe& r, const fe& z) {
    fe t, z11;
    fe_pow250(t, z11, z);
    fe_sqr_n(t, t, 2);
    fe_mul(r, t, z);
}

// Go's field.Element.SqrtRatio: r = the non-negative square root of u / v and true, or (u / v
// not a square) r = sqrt(i u / v) and false. In: u, v of class 2T at most (they meet only T
// operands below). Out: T with |r| the even canonical representative.
SBFT_ED_HD bool fe_sqrt_ratio(fe& r, const fe& u_in, const fe& v_in) {
    const i32 sm1[9] = SBFT_ED_SQRTM1;
    fe u, v, v3, v7, t, rr, check, i_;
    fe_weak(u, u_in);
    fe_weak(v, v_in);
    fe_const(i_, sm1);
    fe_sqr(t, v);
    fe_mul(v3, t, v);
    fe_sqr(t, v3);
    fe_mul(v7, t, v);
    fe_mul(t, u, v7);
    fe_pow22523(t, t);
    fe_mul(rr, u, v3);
    fe_mul(rr, rr, t);
    fe_sqr(t, rr);
    fe_mul(check, v, t);
    fe nu, nui;
    fe_neg(nu, u);
    fe_mul(nui, nu, i_);
    u32 wc[8], wu[8], wn[8], wi[8];
    fe_tobytes(wc, check);
    fe_tobytes(wu, u);
    fe_tobytes(wn, nu);
    fe_tobytes(wi, nui);
    const bool correct = words_eq(wc, wu), flipped = words_eq(wc, wn), flipped_i = words_eq(wc, wi);
    if (flipped || flipped_i) fe_mul(rr, rr, i_);
    u32 wr[8];
    fe_tobytes(wr, rr);
    if (wr[0] & 1) fe_neg(rr, rr);
    r = rr;
    return correct || flipped;
}

// ------------------------------------------------------------------ scalars mod L
// L = 2^252 + c, c = 27742317777372353535851937790883648493 (125 bits), little-endian words
#define SBFT_ED_L {0x5cf5d3edu, 0x5812631au, 0xa2f79cd6u, 0x14def9deu, 0u, 0u, 0u, 0x10000000u}
#define SBFT_ED_LC {0x5cf5d3edu, 0x5812631au, 0xa2f79cd6u, 0x14def9deu}

// s < L (8 little-endian words)
SBFT_ED_HD bool sc_is_canonical(const u32 s[8]) {
    const u32 l[8] = SBFT_ED_L;
    bool lt = false, decided = false;
    SBFT_ED_UNROLL
    for (int i = 7; i >= 0; --i) {
        if (!decided && s[i] != l[i]) {
            lt = s[i] < l[i];
            decided = true;
        }
    }
    return lt;
}
// out[0 .. NA + 4) = a[0 .. NA) * c (schoolbook, 64-bit column carries)
template <int NA>
SBFT_ED_HD void sc_mul_c(u32* out, const u32* a) {
    const u32 c[4] = SBFT_ED_LC;
    SBFT_ED_UNROLL
    for (int i = 0; i < NA + 4; ++i) out[i] = 0;
    SBFT_ED_UNROLL
    for (int i = 0; i < NA; ++i) {
        u64 carry = 0;
        SBFT_ED_UNROLL
        for (int j = 0; j < 4; ++j) {
            const u64 t = (u64)a[i] * c[j] + out[i + j] + carry;
            out[i + j] = (u32)t;
            carry = t >> 32;
        }
        out[i + 4] = (u32)carry;
    }
}
// hi = x >> 252 (NH words), x of NX words
template <int NX, int NH>
SBFT_ED_HD void sc_hi252(u32* hi, const u32* x) {
    SBFT_ED_UNROLL
    for (int j = 0; j < NH; ++j) {
        u32 v = (7 + j < NX) ? x[7 + j] >> 28 : 0;
        if (8 + j < NX) v |= x[8 + j] << 4;
        hi[j] = v;
    }
}
// r (9 words) += / -= the low 252 bits of x (8 words) -- or all of x if full
SBFT_ED_HD void sc_acc(u32 r[9], const u32* x, int nx, bool sub, bool low252) {
    i64 carry = 0;
    SBFT_ED_UNROLL
    for (int i = 0; i < 9; ++i) {
        u32 v = i < nx ? x[i] : 0;
        if (low252 && i == 7) v &= 0x0fffffffu;
        if (low252 && i > 7) v = 0;
        const i64 t = (i64)r[i] + (sub ? -(i64)v : (i64)v) + carry;
        r[i] = (u32)t;
        carry = t >> 32;
    }
}
// out = x mod L for a 512-bit x (16 little-endian words). With 2^252 = -c (mod L):
//   x  = lo + 2^252 hi,  t1 = c hi  (385 bits) = lo1 + 2^252 hi1,  t2 = c hi1 (258 bits) =
//   lo2 + 2^252 hi2,  hi2 < 2^6:   x = lo - lo1 + lo2 - c hi2 (mod L),
// a value in (-2^252 - 2^131, 2^253). Adding 2 L makes it positive and below 4 L; at most three
// subtractions of L finish.
SBFT_ED_HD void sc_reduce(u32 out[8], const u32 x[16]) {
    const u32 l[8] = SBFT_ED_L;
    u32 hi[9], t1[13], hi1[5], t2[9], hi2[1], t3[5];
    sc_hi252<16, 9>(hi, x);
    sc_mul_c<9>(t1, hi);
    sc_hi252<13, 5>(hi1, t1);
    sc_mul_c<5>(t2, hi1);
    sc_hi252<9, 1>(hi2, t2);
    sc_mul_c<1>(t3, hi2);
    u32 r[9];
    SBFT_ED_UNROLL
    for (int i = 0; i < 9; ++i) r[i] = 0;
    sc_acc(r, l, 8, false, false);
    sc_acc(r, l, 8, false, false);
    sc_acc(r, x, 8, false, true);
    sc_acc(r, t2, 8, false, true);
    sc_acc(r, t1, 8, true, true);
    sc_acc(r, t3, 5, true, false);
    SBFT_ED_UNROLL
    for (int rep = 0; rep < 3; ++rep) {
        if (r[8] || !sc_is_canonical(r)) sc_acc(r, l, 8, true, false);
    }
    SBFT_ED_UNROLL
    for (int i = 0; i < 8; ++i) out[i] = r[i];
}

// Signed radix-16 recoding of a scalar s < 2^253: with the bias 0x88..8 (8 in every nibble)
// added once, digit i is nibble i of the biased value minus 8, in [-8, 7], and
// sum digit_i 16^i = s. The biased value stays below 2^256 (no carry out). The loop below takes
// the digits from the top by shifting the eight words left, so no array is indexed at run time.
SBFT_ED_HD void sc_bias(u32 s[8]) {
    u64 carry = 0;
    SBFT_ED_UNROLL
    for (int i = 0; i < 8; ++i) {
        const u64 t = (u64)s[i] + 0x88888888u + carry;
        s[i] = (u32)t;
        carry = t >> 32;
    }
}
SBFT_ED_HD int sc_pop_digit(u32 s[8]) {
    const int d = (int)(s[7] >> 28) - 8;
    SBFT_ED_UNROLL
    for (int i = 7; i > 0; --i) s[i] = (s[i] << 4) | (s[i - 1] >> 28);
    s[0] <<= 4;
    return d;
}

// ------------------------------------------------------------------ points
// Extended coordinates (X : Y : Z : T), x = X / Z, y = Y / Z, x y = T / Z, curve
// -x^2 + y^2 = 1 + d x^2 y^2. Every stored coordinate is T.
struct ge {
    fe X, Y, Z, T;
};
// The "completed" result of an addition or doubling: (X : Z) x (Y : T), i.e. x = X / Z,
// y = Y / T. X, Z of class T; Y, T of class 2T at most (see each producer).
struct ge_p1p1 {
    fe X, Y, Z, T;
};
// A table entry for additions: Y + X, Y - X, Z, 2 d T, all T.
struct ge_cached {
    fe YpX, YmX, Z, T2d;
};
// An affine table entry (Z = 1): y + x, y - x, 2 d x y, class C.
struct ge_precomp {
    fe ypx, ymx, xy2d;
};

#if defined(__HIPCC__)
__device__ __constant__ const i32 kBtab_dev[8 * 27] = SBFT_ED_BTAB;
#endif
static const i32 kBtab_host[8 * 27] = SBFT_ED_BTAB;
// j B for j in [1, 8], negated if neg (swap y + x and y - x, negate 2 d x y)
SBFT_ED_HD void btab_load(ge_precomp& p, int j, bool neg) {
#if defined(__HIP_DEVICE_COMPILE__)
    const i32* t = kBtab_dev + 27 * (j - 1);
#else
    const i32* t = kBtab_host + 27 * (j - 1);
#endif
    SBFT_ED_UNROLL
    for (int i = 0; i < 9; ++i) {
        const i32 a = t[i], b = t[9 + i], c = t[18 + i];
        p.ypx.v[i] = neg ? b : a;
        p.ymx.v[i] = neg ? a : b;
        p.xy2d.v[i] = neg ? -c : c;
    }
}

SBFT_ED_HD void ge_identity(ge& r) {
    fe_set(r.X, 0);
    fe_set(r.Y, 1);
    fe_set(r.Z, 1);
    fe_set(r.T, 0);
}
// p1p1 -> extended. Products: X T (T x 2T), Y Z (2T x T), Z T (T x 2T), X Y (T x 2T); the
// fourth only when the next operation is an addition (a doubling does not read T).
SBFT_ED_HD void ge_complete(ge& r, const ge_p1p1& p, bool want_t) {
    fe x, y, z;
    fe_mul(x, p.X, p.T);
    fe_mul(y, p.Y, p.Z);
    fe_mul(z, p.Z, p.T);
    if (want_t) fe_mul(r.T, p.X, p.Y);
    r.X = x;
    r.Y = y;
    r.Z = z;
}
// Dedicated doubling (dbl-2008-hwcd, a = -1), 4 squarings here + 3 or 4 products in
// ge_complete. In: X, Y, Z of class T. XX, YY, ZZ, S = (X + Y)^2 (the sum brought to T first).
// Out: X = weak(S - YY - XX) T, Y = YY + XX 2T, Z = YY - XX (|limb| <= 2^29 + 2^18, within the
// 2T x T products of ge_complete), T = weak(2 ZZ - Z) T (3T < 2^31 before the carry).
SBFT_ED_HD void ge_dbl(ge_p1p1& r, const ge& p) {
    fe xx, yy, zz, s, t;
    fe_sqr(xx, p.X);
    fe_sqr(yy, p.Y);
    fe_sqr(zz, p.Z);
    fe_add(t, p.X, p.Y);
    fe_weak(t, t);
    fe_sqr(s, t);
    fe_add(r.Y, yy, xx);
    fe_sub(r.Z, yy, xx);
    fe_sub(t, s, r.Y);
    fe_weak(r.X, t);
    fe_add(t, zz, zz);
    fe_sub(t, t, r.Z);
    fe_weak(r.T, t);
}
// Shared tail of the two additions: a = (Y1 + X1)(Y2 + X2), b = (Y1 - X1)(Y2 - X2), c = 2 d T1
// T2 (all T), d2 = 2 Z1 Z2 (2T). Out: X = a - b (|limb| <= 2^29 + 2^18), Y = a + b 2T,
// Z = weak(d2 + c) T, T = d2 - c (2T in magnitude): X T, Y Z, Z T, X Y in ge_complete are
// T x 2T at most.
SBFT_ED_HD void ge_add_tail(ge_p1p1& r, const fe& a, const fe& b, const fe& c, const fe& d2) {
    fe t;
    fe_sub(r.X, a, b);
    fe_add(r.Y, a, b);
    fe_add(t, d2, c);
    fe_weak(r.Z, t);
    fe_sub(r.T, d2, c);
}
// The complete unified addition (add-2008-hwcd-3, a = -1; it holds for the identity, P + P and
// small-order points), mixed with an affine table entry: 3 products + ge_complete.
// (Y1 + X1), (Y1 - X1): 2T x C.
SBFT_ED_HD void ge_madd(ge_p1p1& r, const ge& p, const ge_precomp& q) {
    fe a, b, c, d2, t;
    fe_add(t, p.Y, p.X);
    fe_mul(a, t, q.ypx);
    fe_sub(t, p.Y, p.X);
    fe_mul(b, t, q.ymx);
    fe_mul(c, q.xy2d, p.T);
    fe_add(d2, p.Z, p.Z);
    ge_add_tail(r, a, b, c, d2);
}
// The same with a projective table entry: 4 products + ge_complete. 2T x T.
SBFT_ED_HD void ge_add(ge_p1p1& r, const ge& p, const ge_cached& q) {
    fe a, b, c, d2, t;
    fe_add(t, p.Y, p.X);
    fe_mul(a, t, q.YpX);
    fe_sub(t, p.Y, p.X);
    fe_mul(b, t, q.YmX);
    fe_mul(c, q.T2d, p.T);
    fe_mul(t, p.Z, q.Z);
    fe_add(d2, t, t);
    ge_add_tail(r, a, b, c, d2);
}
SBFT_ED_HD void ge_to_cached(ge_cached& r, const ge& p) {
    const i32 d2[9] = SBFT_ED_2D;
    fe k, t;
    fe_const(k, d2);
    fe_add(t, p.Y, p.X);
    fe_weak(r.YpX, t);
    fe_sub(t, p.Y, p.X);
    fe_weak(r.YmX, t);
    r.Z = p.Z;
    fe_mul(r.T2d, p.T, k);
}

// Go's Point.SetBytes (rule 1 of the header comment of include/sbft_gpuverify.h): y = the low
// 255 bits, not checked against p; x = sqrt((y^2 - 1) / (d y^2 + 1)), none: false; the
// non-negative root, negated if bit 255 is set (-0 = 0 is accepted).
SBFT_ED_HD bool ge_frombytes(ge& r, const u32 w[8]) {
    const i32 dl[9] = SBFT_ED_D;
    fe d, y2, u, v, one;
    fe_const(d, dl);
    fe_set(one, 1);
    fe_frombytes(r.Y, w, true);
    fe_sqr(y2, r.Y);
    fe_sub(u, y2, one);
    fe_mul(v, y2, d);
    fe_add(v, v, one);
    const bool ok = fe_sqrt_ratio(r.X, u, v);
    if (w[7] >> 31) fe_neg(r.X, r.X);
    fe_set(r.Z, 1);
    fe_mul(r.T, r.X, r.Y);
    return ok;
}
// canonical 32-byte encoding: y with x's low bit in bit 255 (one inversion)
SBFT_ED_HD void ge_tobytes(u32 w[8], const ge& p) {
    fe zi, x, y;
    fe_invert(zi, p.Z);
    fe_mul(x, p.X, zi);
    fe_mul(y, p.Y, zi);
    u32 wx[8];
    fe_tobytes(w, y);
    fe_tobytes(wx, x);
    w[7] |= (wx[0] & 1) << 31;
}

// The per-signature table j P, j = 1..8, in cached form: 8 x 36 words behind an accessor, so
// the device keeps it in a strided workspace (word i of a lane at base[i * stride]) and the host
// in a plain array. No per-lane array is indexed at run time.
struct TabHost {
    i32 w[8 * 36];
    i32 get(int i) const { return w[i]; }
    void put(int i, i32 x) { w[i] = x; }
};
struct TabStrided {
    i32* base;
    size_t stride;
    SBFT_ED_HDM i32 get(int i) const { return base[(size_t)i * stride]; }
    SBFT_ED_HDM void put(int i, i32 x) { base[(size_t)i * stride] = x; }
};
template <class Tab>
SBFT_ED_HD void tab_store(Tab& tab, int e, const ge_cached& c) {
    SBFT_ED_UNROLL
    for (int i = 0; i < 9; ++i) {
        tab.put(36 * e + i, c.YpX.v[i]);
        tab.put(36 * e + 9 + i, c.YmX.v[i]);
        tab.put(36 * e + 18 + i, c.Z.v[i]);
        tab.put(36 * e + 27 + i, c.T2d.v[i]);
    }
}
template <class Tab>
SBFT_ED_HD void tab_load(ge_cached& c, const Tab& tab, int e, bool neg) {
    SBFT_ED_UNROLL
    for (int i = 0; i < 9; ++i) {
        const i32 a = tab.get(36 * e + i), b = tab.get(36 * e + 9 + i);
        c.YpX.v[i] = neg ? b : a;
        c.YmX.v[i] = neg ? a : b;
        c.Z.v[i] = tab.get(36 * e + 18 + i);
        const i32 t = tab.get(36 * e + 27 + i);
        c.T2d.v[i] = neg ? -t : t;
    }
}
// tab[j - 1] = j P for j = 1..8 (7 unified additions; P + P goes through the same formula)
template <class Tab>
SBFT_ED_HD void tab_build(Tab& tab, const ge& p) {
    ge_cached c1, c;
    ge_to_cached(c1, p);
    tab_store(tab, 0, c1);
    ge cur = p;
    SBFT_ED_UNROLL1
    for (int j = 1; j < 8; ++j) {
        ge_p1p1 t;
        ge_add(t, cur, c1);
        ge_complete(cur, t, true);
        ge_to_cached(c, cur);
        tab_store(tab, j, c);
    }
}

// r = [s] B + [k] P for the P whose multiples tab holds; s, k < 2^253 (8 little-endian words).
// Interleaved signed 4-bit windows: 64 steps of four doublings, one mixed addition from B's
// static table and one addition from P's table (a zero digit skips its addition). T is
// computed only where the next operation reads it.
template <class Tab>
SBFT_ED_HD void double_scalar_vartime(ge& r, const u32 s_in[8], const u32 k_in[8], const Tab& tab) {
    u32 s[8], k[8];
    SBFT_ED_UNROLL
    for (int i = 0; i < 8; ++i) {
        s[i] = s_in[i];
        k[i] = k_in[i];
    }
    sc_bias(s);
    sc_bias(k);
    ge_identity(r);
    SBFT_ED_UNROLL1
    for (int step = 0; step < 64; ++step) {
        const int ds = sc_pop_digit(s), dk = sc_pop_digit(k);
        ge_p1p1 t;
        if (step) {
            SBFT_ED_UNROLL1
            for (int d = 0; d < 4; ++d) {
                ge_dbl(t, r);
                ge_complete(r, t, d == 3 && (ds | dk) != 0);
            }
        }
        if (ds) {
            ge_precomp q;
            btab_load(q, ds < 0 ? -ds : ds, ds < 0);
            ge_madd(t, r, q);
            ge_complete(r, t, dk != 0);
        }
        if (dk) {
            ge_cached q;
            tab_load(q, tab, (dk < 0 ? -dk : dk) - 1, dk < 0);
            ge_add(t, r, q);
            ge_complete(r, t, false);
        }
    }
}

// The 512-bit digest (SHA-512 state words) as 16 little-endian words of the integer Go reads.
SBFT_ED_HD void digest_words(u32 x[16], const u64 h[8]) {
    SBFT_ED_UNROLL
    for (int i = 0; i < 8; ++i) {
        x[2 * i] = sha512::bswap32((u32)(h[i] >> 32));
        x[2 * i + 1] = sha512::bswap32((u32)h[i]);
    }
}

// crypto/ed25519.Verify after the hash: pub, R (sig[0:32]) and S (sig[32:64]) as little-endian
// words, h = SHA-512(R || pub || msg). 1 = accept. Order of the checks is free (all five rules
// must hold); the cheap ones come first.
template <class Tab>
SBFT_ED_HD int verify_core(const u32 pub[8], const u32 rw[8], const u32 sw[8], const u64 h[8], Tab& tab) {
    if (!sc_is_canonical(sw)) return 0;
    ge a;
    if (!ge_frombytes(a, pub)) return 0;
    fe_neg(a.X, a.X);
    fe_neg(a.T, a.T);
    u32 x[16], k[8];
    digest_words(x, h);
    sc_reduce(k, x);
    tab_build(tab, a);
    ge r;
    double_scalar_vartime(r, sw, k, tab);
    u32 enc[8];
    ge_tobytes(enc, r);
    return words_eq(enc, rw) ? 1 : 0;
}

}  // namespace ed
}  // namespace sbft
