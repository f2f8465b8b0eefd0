// sha512_dev.hpp — SHA-512 (FIPS 180-4) of one message per lane, for the Ed25519 verify kernel
// (k = SHA-512(R || A || M)) and sha512_kernel. Compiles for the device and, unchanged, for the
// host (tests/native/ed25519_test.cpp runs the same code under g++).
//
// The hashed stream is an optional 64-byte prefix held in registers (R || A as 16 little-endian
// words) followed by the message msg[0, len) at any byte alignment. Message bytes are fetched
// as aligned 4-byte words, and only words that hold at least one message byte are read: a blob
// sized exactly to its messages is safe (its allocation is 4-byte aligned at both ends: every
// device allocation is). Padding is for an arbitrary length.
//
// The state is 8 x 64 bits and the schedule a rolling window of 16 x 64 bits, all indexed by
// constants (the 16 rounds of a pass are unrolled), so nothing goes to scratch. 64-bit rotates
// are two v_alignbit on the 32-bit halves; the adds are the compiler's v_add_co / v_addc pairs.
// A wavefront's lanes may hash different lengths: each lane loops over its own block count, so
// the hardware runs the loop to the longest and masks the lanes that are done.
#pragma once
#include <stdint.h>

#include "ed25519_tables.inc"
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SBFT_ED_HD __host__ __device__ __forceinline__
#define SBFT_ED_HDM __host__ __device__ __forceinline__  // member functions
#define SBFT_ED_UNROLL _Pragma("unroll")
#define SBFT_ED_UNROLL1 _Pragma("unroll 1")
#else
#define SBFT_ED_HD static inline
#define SBFT_ED_HDM inline
#define SBFT_ED_UNROLL
#define SBFT_ED_UNROLL1
#endif

namespace sbft {
namespace sha512 {

#if defined(__HIPCC__)
__device__ __constant__ const uint64_t kK_dev[80] = SBFT_SHA512_K;
#endif
static const uint64_t kK_host[80] = SBFT_SHA512_K;

SBFT_ED_HD uint64_t round_k(int i) {
#if defined(__HIP_DEVICE_COMPILE__)
    return kK_dev[i];
#else
    return kK_host[i];
#endif
}

SBFT_ED_HD uint64_t rotr(uint64_t x, int n) {  // 0 < n < 64, n != 32
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
    if (n > 32) {
        const uint32_t t = lo;
        lo = hi;
        hi = t;
        n -= 32;
    }
    const uint32_t rl = __builtin_amdgcn_alignbit(hi, lo, n), rh = __builtin_amdgcn_alignbit(lo, hi, n);
    return ((uint64_t)rh << 32) | rl;
#else
    return (x >> n) | (x << (64 - n));
#endif
}

SBFT_ED_HD uint32_t bswap32(uint32_t x) {
    return (x >> 24) | ((x >> 8) & 0xff00u) | ((x << 8) & 0xff0000u) | (x << 24);
}

SBFT_ED_HD void init(uint64_t h[8]) {
    const uint64_t iv[8] = SBFT_SHA512_IV;
    SBFT_ED_UNROLL
    for (int i = 0; i < 8; ++i) h[i] = iv[i];
}

// one 128-byte block: w holds its 16 big-endian words and is consumed
SBFT_ED_HD void compress(uint64_t h[8], uint64_t w[16]) {
    uint64_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
    SBFT_ED_UNROLL1
    for (int pass = 0; pass < 5; ++pass) {
        SBFT_ED_UNROLL
        for (int j = 0; j < 16; ++j) {
            if (pass) {
                const uint64_t w15 = w[(j + 1) & 15], w2 = w[(j + 14) & 15];
                const uint64_t s0 = rotr(w15, 1) ^ rotr(w15, 8) ^ (w15 >> 7);
                const uint64_t s1 = rotr(w2, 19) ^ rotr(w2, 61) ^ (w2 >> 6);
                w[j] += s0 + w[(j + 9) & 15] + s1;
            }
            const uint64_t S1 = rotr(e, 14) ^ rotr(e, 18) ^ rotr(e, 41);
            const uint64_t ch = (e & f) ^ (~e & g);
            const uint64_t t1 = hh + S1 + ch + round_k(16 * pass + j) + w[j];
            const uint64_t S0 = rotr(a, 28) ^ rotr(a, 34) ^ rotr(a, 39);
            const uint64_t maj = (a & b) ^ (a & c) ^ (b & c);
            const uint64_t t2 = S0 + maj;
            hh = g;
            g = f;
            f = e;
            e = d + t1;
            d = c;
            c = b;
            b = a;
            a = t1 + t2;
        }
    }
    h[0] += a;
    h[1] += b;
    h[2] += c;
    h[3] += d;
    h[4] += e;
    h[5] += f;
    h[6] += g;
    h[7] += hh;
}

// Message bytes m .. m+3 (m a multiple of 4) as a big-endian word, bytes at or past len read
// as zero, with the 0x80 padding byte placed at position len. q is msg rounded down to a
// 4-byte boundary and a = msg - q, so the four bytes straddle two aligned words when a != 0.
// cur = q[m / 4], nxt = q[m / 4 + 1] (each 0 where not loaded, see aligned_word).
SBFT_ED_HD uint32_t msg_word(uint32_t cur, uint32_t nxt, uint32_t a, uint64_t m, uint32_t len) {
    if (m > len) return 0;
    uint32_t v = bswap32(a ? (cur >> (8 * a)) | (nxt << (32 - 8 * a)) : cur);
    const uint64_t left = len - m;  // message bytes from m on (may exceed 4)
    if (left < 4) {
        v &= ~(0xffffffffu >> (8 * (uint32_t)left));
        v |= 0x80000000u >> (8 * (uint32_t)left);
    }
    return v;
}
// q[i] if that word holds a message byte (4 i < a + len; its last byte is at or past a for
// every i >= 0), else 0 without a load
SBFT_ED_HD uint32_t aligned_word(const uint32_t* q, uint64_t i, uint64_t end) { return 4 * i < end ? q[i] : 0; }

// h = SHA-512(prefix || msg[0, len)) as 8 big-endian 64-bit words. pre: 16 little-endian words
// (the 64 prefix bytes as loaded from memory), used when npre = 64; npre = 0: no prefix.
SBFT_ED_HD void hash_prefixed(uint64_t h[8], const uint32_t pre[16], uint32_t npre, const uint8_t* msg,
                              uint32_t len) {
    const uint32_t a = (uint32_t)((uintptr_t)msg & 3u);
    const uint32_t* q = (const uint32_t*)(msg - a);
    const uint64_t total = (uint64_t)npre + len;
    const uint64_t nblocks = (total + 17 + 127) >> 7;
    const uint64_t end = len ? (uint64_t)a + len : 0;  // an empty message has no word to read
    init(h);
    SBFT_ED_UNROLL1
    for (uint64_t b = 0; b < nblocks; ++b) {
        // the block's message words are consecutive aligned words: one load each, carried along
        uint64_t i = b ? (128 * b - npre) >> 2 : 0;
        uint32_t cur = aligned_word(q, i, end);
        uint64_t w[16];
        SBFT_ED_UNROLL
        for (int j = 0; j < 16; ++j) {
            uint32_t x[2];
            SBFT_ED_UNROLL
            for (int t = 0; t < 2; ++t) {
                if (j < 8 && b == 0 && npre) {
                    x[t] = bswap32(pre[2 * (j & 7) + t]);
                } else {
                    const uint32_t nxt = aligned_word(q, i + 1, end);
                    x[t] = msg_word(cur, nxt, a, 4 * i, len);
                    cur = nxt;
                    ++i;
                }
            }
            w[j] = ((uint64_t)x[0] << 32) | x[1];
        }
        if (b == nblocks - 1) {
            w[14] |= total >> 61;
            w[15] |= total << 3;
        }
        compress(h, w);
    }
}

}  // namespace sha512
}  // namespace sbft
