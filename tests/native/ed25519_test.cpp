// Host driver for smartbft_amd/csrc/ed25519_f25.hpp and sha512_dev.hpp: the header the
// Ed25519 kernel includes, compiled with g++ and checked by tests/test_ed25519_cpu.py against
// Python big integers. Numbers cross the pipe as big-endian hex of the integer.
//   field   lines "a b" (256-bit)        -> "mul sqr inv(a) sqrt_ratio(a,b) was_square"
//   limbs   lines of 18 signed limbs     -> "mul sqr" (canonical) of the two limb vectors
//   small   lines "a c"                  -> a * c (c a signed 32-bit decimal)
//   sc      lines of a 512-bit value     -> "x mod L"
//   digits  lines of a 256-bit value     -> the 64 signed radix-16 digits, least significant first
//   sha512  lines "<shift> <hex bytes>"  -> digest (message placed at byte offset shift of a buffer)
//   verify  <fixture file>               -> one character '0' / '1' per record
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../smartbft_amd/csrc/ed25519_f25.hpp"

using namespace sbft::ed;

static bool parse_hex(const char* s, u32* w, int nw) {
    const size_t n = strlen(s);
    for (int i = 0; i < nw; ++i) w[i] = 0;
    for (size_t i = 0; i < n; ++i) {
        const char c = s[n - 1 - i];
        int v = c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1;
        if (v < 0 || i / 8 >= (size_t)nw) return false;
        w[i / 8] |= (u32)v << (4 * (i % 8));
    }
    return true;
}
static void print_words(const u32* w, int nw) {
    for (int i = nw - 1; i >= 0; --i) printf("%08x", w[i]);
}
static void print_fe(const fe& a) {
    u32 w[8];
    fe_tobytes(w, a);
    print_words(w, 8);
}

static int run_verify(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) return 2;
    std::vector<uint8_t> buf;
    uint8_t tmp[4096];
    size_t got;
    while ((got = fread(tmp, 1, sizeof tmp, f)) > 0) buf.insert(buf.end(), tmp, tmp + got);
    fclose(f);
    size_t p = 0;
    std::string out;
    while (p < buf.size()) {
        if (p + 98 > buf.size()) return 3;
        u32 pub[8], sig[16], pre[16];
        memcpy(pub, &buf[p], 32);
        memcpy(sig, &buf[p + 32], 64);
        const uint32_t len = buf[p + 96] | (uint32_t)buf[p + 97] << 8;
        p += 98;
        if (p + len + 2 > buf.size()) return 3;
        // the message in an allocation of exactly its size (a sanitizer build sees any over-read
        // past the last aligned word that holds a message byte)
        const size_t words = (len + 3) / 4;
        uint32_t* msg = new uint32_t[words ? words : 1];
        memcpy(msg, &buf[p], len);
        p += len + 2;
        for (int i = 0; i < 8; ++i) {
            pre[i] = sig[i];
            pre[8 + i] = pub[i];
        }
        u64 h[8];
        sbft::sha512::hash_prefixed(h, pre, 64, (const uint8_t*)msg, len);
        TabHost tab;
        out.push_back(verify_core(pub, sig, sig + 8, h, tab) ? '1' : '0');
        delete[] msg;
    }
    printf("%s\n", out.c_str());
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string mode = argv[1];
    if (mode == "verify") return argc < 3 ? 2 : run_verify(argv[2]);
    static char line[1 << 16];
    while (fgets(line, sizeof line, stdin)) {
        std::vector<char*> tok;
        for (char* t = strtok(line, " \n"); t; t = strtok(nullptr, " \n")) tok.push_back(t);
        if (tok.empty()) continue;
        if (mode == "field") {
            u32 a[8], b[8];
            if (tok.size() != 2 || !parse_hex(tok[0], a, 8) || !parse_hex(tok[1], b, 8)) return 2;
            fe x, y, r;
            fe_frombytes(x, a, false);
            fe_frombytes(y, b, false);
            fe_mul(r, x, y);
            print_fe(r);
            printf(" ");
            fe_sqr(r, x);
            print_fe(r);
            printf(" ");
            fe_invert(r, x);
            print_fe(r);
            printf(" ");
            const bool sq = fe_sqrt_ratio(r, x, y);
            print_fe(r);
            printf(" %d\n", sq ? 1 : 0);
        } else if (mode == "limbs") {
            if (tok.size() != 18) return 2;
            fe x, y, r;
            for (int i = 0; i < 9; ++i) {
                x.v[i] = (i32)atol(tok[i]);
                y.v[i] = (i32)atol(tok[9 + i]);
            }
            fe_mul(r, x, y);
            print_fe(r);
            printf(" ");
            fe_sqr(r, x);
            print_fe(r);
            printf(" ");
            print_fe(x);  // fe_tobytes of the raw limbs
            printf("\n");
        } else if (mode == "small") {
            u32 a[8];
            if (tok.size() != 2 || !parse_hex(tok[0], a, 8)) return 2;
            fe x, r;
            fe_frombytes(x, a, false);
            fe_mul_small(r, x, (i32)atol(tok[1]));
            print_fe(r);
            printf("\n");
        } else if (mode == "sc") {
            u32 x[16], r[8];
            if (!parse_hex(tok[0], x, 16)) return 2;
            sc_reduce(r, x);
            print_words(r, 8);
            printf(" %d\n", sc_is_canonical(x) && !(x[8] | x[9] | x[10] | x[11] | x[12] | x[13] | x[14] | x[15]));
        } else if (mode == "digits") {
            u32 s[8];
            if (!parse_hex(tok[0], s, 8)) return 2;
            sc_bias(s);
            int d[64];
            for (int i = 63; i >= 0; --i) d[i] = sc_pop_digit(s);
            for (int i = 0; i < 64; ++i) printf("%d ", d[i]);
            printf("\n");
        } else if (mode == "sha512") {
            if (tok.size() < 1) return 2;
            const int shift = atoi(tok[0]);
            const char* hex = tok.size() > 1 ? tok[1] : "";
            const size_t len = strlen(hex) / 2;
            const size_t words = (shift + len + 3) / 4;
            uint32_t* buf = new uint32_t[words ? words : 1];
            uint8_t* m = (uint8_t*)buf + shift;
            for (size_t i = 0; i < len; ++i) {
                unsigned v;
                sscanf(hex + 2 * i, "%2x", &v);
                m[i] = (uint8_t)v;
            }
            u64 h[8];
            sbft::sha512::hash_prefixed(h, nullptr, 0, m, (uint32_t)len);
            for (int i = 0; i < 8; ++i) printf("%016llx", (unsigned long long)h[i]);
            printf("\n");
            delete[] buf;
        } else {
            return 2;
        }
    }
    return 0;
}
