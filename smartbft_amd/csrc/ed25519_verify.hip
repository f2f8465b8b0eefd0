// ed25519_verify.hip — batched Ed25519 verification with the semantics of Go's
// crypto/ed25519.Verify (include/sbft_gpuverify.h states the five rules), one lane per
// signature: decode A, k = SHA-512(R || A || M) mod L, S < L, R' = [S]B - [k]A by interleaved
// signed 4-bit windows, encode R', compare with sig[0:32], one verdict byte. One launch per
// batch, no second pass: the unified a = -1 addition is complete, so there are no exceptional
// cases to hand to another kernel. The arithmetic is ed25519_f25.hpp / sha512_dev.hpp, which
// the host tests compile unchanged.
//
// Each lane's table of multiples j (-A), j = 1..8 (288 words) lives in a device workspace, word
// i of lane t at work[i * lanes + t], so a wavefront's loads of one entry coalesce and no
// per-lane array is indexed at run time. At most kEdMaxLanes lanes are launched (every wave
// slot of an MI355X at 128 VGPRs); a larger batch is walked with that stride, which also bounds
// the workspace (288 x 4 B per lane, 302 MB at the cap).
#include "ed25519_f25.hpp"
#include "sbft_kernels.h"

namespace sbft {

// Waves per SIMD the verify kernel is compiled for (its register budget: 512 / waves VGPRs).
// Measured on 1M tuples (profiles/ed25519/waves_ab.txt): 1 wave 51.7, 2 waves 58.7, 3 waves
// 61.4 M verifies/s -- the third wave pays for the 468 B of spills it costs.
#ifndef SBFT_ED_WAVES
#define SBFT_ED_WAVES 3
#endif
constexpr uint32_t kEdBlock = 256;
constexpr uint32_t kEdMaxLanes = 262144;
constexpr uint32_t kEdTabWords = 8 * 36;

__device__ __forceinline__ void load_words8(uint32_t w[8], const uint8_t* p) {  // p 4-byte aligned
    const uint32_t* q = (const uint32_t*)p;
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i] = q[i];
}
__device__ __forceinline__ void store_words8(uint8_t* p, const uint32_t w[8]) {
    uint32_t* q = (uint32_t*)p;
#pragma unroll
    for (int i = 0; i < 8; ++i) q[i] = w[i];
}

__global__ __launch_bounds__(kEdBlock, SBFT_ED_WAVES) void ed25519_verify_kernel(
    const uint8_t* __restrict__ blob, const uint64_t* __restrict__ off, const uint32_t* __restrict__ len,
    const uint8_t* __restrict__ sig, const uint8_t* __restrict__ pub, uint8_t* __restrict__ ok, uint32_t n,
    int32_t* __restrict__ work, uint32_t lanes) {
    const uint32_t tid = blockIdx.x * kEdBlock + threadIdx.x;
    if (tid >= lanes) return;
    ed::TabStrided tab = {work + tid, lanes};
#pragma unroll 1
    for (uint32_t k = tid; k < n; k += lanes) {
        uint32_t pre[16], a[8];
        load_words8(pre, sig + 64ull * k);
        load_words8(a, pub + 32ull * k);
#pragma unroll
        for (int i = 0; i < 8; ++i) pre[8 + i] = a[i];
        uint64_t h[8];
        sha512::hash_prefixed(h, pre, 64, blob + off[k], len[k]);
        uint32_t s[8];
        load_words8(s, sig + 64ull * k + 32);
        ok[k] = (uint8_t)ed::verify_core(a, pre, s, h, tab);
    }
}

__global__ __launch_bounds__(kEdBlock) void sha512_kernel(const uint8_t* __restrict__ blob,
                                                          const uint64_t* __restrict__ off,
                                                          const uint32_t* __restrict__ len,
                                                          uint8_t* __restrict__ dig, uint32_t n) {
    const uint32_t k = blockIdx.x * kEdBlock + threadIdx.x;
    if (k >= n) return;
    uint64_t h[8];
    sha512::hash_prefixed(h, nullptr, 0, blob + off[k], len[k]);
    uint32_t* out = (uint32_t*)(dig + 64ull * k);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        out[2 * i] = sha512::bswap32((uint32_t)(h[i] >> 32));
        out[2 * i + 1] = sha512::bswap32((uint32_t)h[i]);
    }
}

// Element-wise self-test (sbft_gv_selftest_ed25519). a, b, out: n x 32 bytes little-endian.
//   0  a b mod p          1  a^2 mod p          2  a^-1 mod p (0 for a = 0 mod p)
//   3  point decode of a: the canonical encoding of x, or all-ones if a is not a point
//   4  (a + 2^256 b) mod L
//   5  [a]B encoded       6  [a]B + [b]P0 encoded (P0: ed25519_tables.inc; a, b taken mod L)
__global__ __launch_bounds__(kEdBlock) void ed25519_selftest_kernel(int op, const uint8_t* __restrict__ a_in,
                                                                    const uint8_t* __restrict__ b_in,
                                                                    uint8_t* __restrict__ out, uint32_t n,
                                                                    int32_t* __restrict__ work) {
    const uint32_t k = blockIdx.x * kEdBlock + threadIdx.x;
    if (k >= n) return;
    uint32_t a[8], b[8], r[8];
    load_words8(a, a_in + 32ull * k);
    load_words8(b, b_in + 32ull * k);
#pragma unroll
    for (int i = 0; i < 8; ++i) r[i] = 0xffffffffu;
    if (op <= 2) {
        ed::fe x, y, z;
        ed::fe_frombytes(x, a, false);
        ed::fe_frombytes(y, b, false);
        if (op == 0) ed::fe_mul(z, x, y);
        else if (op == 1) ed::fe_sqr(z, x);
        else ed::fe_invert(z, x);
        ed::fe_tobytes(r, z);
    } else if (op == 3) {
        ed::ge p;
        if (ed::ge_frombytes(p, a)) ed::fe_tobytes(r, p.X);
    } else if (op == 4) {
        uint32_t x[16];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            x[i] = a[i];
            x[8 + i] = b[i];
        }
        ed::sc_reduce(r, x);
    } else {
        const uint32_t p0w[8] = SBFT_ED_P0;
        uint32_t x[16], s[8], t[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            x[i] = a[i];
            x[8 + i] = 0;
        }
        ed::sc_reduce(s, x);
#pragma unroll
        for (int i = 0; i < 8; ++i) x[i] = op == 6 ? b[i] : 0;
        ed::sc_reduce(t, x);
        ed::TabStrided tab = {work + k, n};
        ed::ge p0, q;
        (void)ed::ge_frombytes(p0, p0w);
        ed::tab_build(tab, p0);
        ed::double_scalar_vartime(q, s, t, tab);
        ed::ge_tobytes(r, q);
    }
    store_words8(out + 32ull * k, r);
}

static uint32_t ed_lanes(size_t n) {
    const size_t up = (n + kEdBlock - 1) / kEdBlock * kEdBlock;
    return (uint32_t)(up < kEdMaxLanes ? up : kEdMaxLanes);
}

}  // namespace sbft

extern "C" size_t sbft_ed25519_work_bytes(size_t n) {
    return (size_t)sbft::ed_lanes(n) * sbft::kEdTabWords * sizeof(int32_t);
}
extern "C" size_t sbft_ed25519_selftest_work_bytes(size_t n) { return n * sbft::kEdTabWords * sizeof(int32_t); }

extern "C" int sbft_launch_ed25519_verify(const uint8_t* d_blob, const uint64_t* d_off, const uint32_t* d_len,
                                          const uint8_t* d_sig, const uint8_t* d_pub, uint8_t* d_ok, uint32_t n,
                                          void* d_work, hipStream_t stream) {
    if (sbft_fault_hit(2)) return -1;  // SBFT_GV_FAULT_LAUNCH (tests only)
    if (n == 0) return 0;
    const uint32_t lanes = sbft::ed_lanes(n);
    hipLaunchKernelGGL(sbft::ed25519_verify_kernel, dim3(lanes / sbft::kEdBlock), dim3(sbft::kEdBlock), 0, stream,
                       d_blob, d_off, d_len, d_sig, d_pub, d_ok, n, (int32_t*)d_work, lanes);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int sbft_launch_sha512(const uint8_t* d_blob, const uint64_t* d_off, const uint32_t* d_len,
                                  uint8_t* d_dig, uint32_t n, hipStream_t stream) {
    if (sbft_fault_hit(2)) return -1;
    if (n == 0) return 0;
    hipLaunchKernelGGL(sbft::sha512_kernel, dim3((n + sbft::kEdBlock - 1) / sbft::kEdBlock), dim3(sbft::kEdBlock), 0,
                       stream, d_blob, d_off, d_len, d_dig, n);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int sbft_launch_ed25519_selftest(int op, const uint8_t* d_a, const uint8_t* d_b, uint8_t* d_out,
                                            uint32_t n, void* d_work, hipStream_t stream) {
    if (sbft_fault_hit(2)) return -1;
    if (n == 0) return 0;
    hipLaunchKernelGGL(sbft::ed25519_selftest_kernel, dim3((n + sbft::kEdBlock - 1) / sbft::kEdBlock),
                       dim3(sbft::kEdBlock), 0, stream, op, d_a, d_b, d_out, n, (int32_t*)d_work);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
