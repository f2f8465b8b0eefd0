/* OpenSSL cross-check of Ed25519 verdicts (tests/test_ed25519_cpu.py, tests/test_gpu_ed25519.py).
 * verify (default): stdin records pub32 | sig64 | u16 len (little-endian) | msg | 2 trailing
 *   bytes (ignored); stdout one character '0' / '1' per record.
 * sign (argv[1] = "sign"): stdin records seed32 | u16 len | msg; stdout pub32 | sig64 per record
 *   (test data in bulk: RFC 8032 signing is deterministic).
 * Build: cc -O2 ed25519_xcheck.c -lcrypto */
#include <openssl/evp.h>
#include <stdio.h>
#include <string.h>

static unsigned char h[98], msg[65536 + 2];

static int sign_all(void) {
    while (fread(h, 1, 34, stdin) == 34) {
        const size_t len = h[32] | (size_t)h[33] << 8;
        unsigned char out[96];
        size_t publen = 32, siglen = 64;
        if (len && fread(msg, 1, len, stdin) != len) return 2;
        EVP_PKEY* key = EVP_PKEY_new_raw_private_key(EVP_PKEY_ED25519, NULL, h, 32);
        EVP_MD_CTX* md = EVP_MD_CTX_new();
        if (!key || !md || EVP_PKEY_get_raw_public_key(key, out, &publen) != 1 ||
            EVP_DigestSignInit(md, NULL, NULL, NULL, key) != 1 ||
            EVP_DigestSign(md, out + 32, &siglen, msg, len) != 1)
            return 3;
        EVP_MD_CTX_free(md);
        EVP_PKEY_free(key);
        fwrite(out, 1, 96, stdout);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "sign")) return sign_all();
    while (fread(h, 1, 98, stdin) == 98) {
        const size_t len = h[96] | (size_t)h[97] << 8;
        if (fread(msg, 1, len + 2, stdin) != len + 2) return 2;
        int ok = 0;
        EVP_PKEY* key = EVP_PKEY_new_raw_public_key(EVP_PKEY_ED25519, NULL, h, 32);
        EVP_MD_CTX* md = EVP_MD_CTX_new();
        if (key && md && EVP_DigestVerifyInit(md, NULL, NULL, NULL, key) == 1)
            ok = EVP_DigestVerify(md, h + 32, 64, msg, len) == 1;
        EVP_MD_CTX_free(md);
        EVP_PKEY_free(key);
        putchar(ok ? '1' : '0');
    }
    putchar('\n');
    return 0;
}
