#!/usr/bin/env python3
"""Throughput of the device-resident Ed25519 verify (sbft_gv_verify_ed25519_dev).

1,000,000 tuples with distinct keys and 32-byte messages, about 10% corrupted, resident on the
GPU; three warm-up calls, then 20 timed steps between two events on one stream; the verdicts of
the last step are checked against the generator's expectation. Prints one JSON line: verifies/s,
ms per step, 32 x 32 -> 64 products per verify by the design's own count (DESIGN.md, Ed25519
section) and that count x rate as a fraction of the measured v_mad_i64_i32 peak of 38.0 T/s
(profiles/r01g_valu_peak.txt).

The test data is made with the engine's own [a]B (the self-test's base-point op, checked
against Python in tests/test_gpu_ed25519.py): A = [a]B, R = [r]B, S = r + SHA-512(R || A || M) a.
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

L = 2**252 + 27742317777372353535851937790883648493
MAD_PEAK = 38.0e12

# Products per verify, counted on this kernel's own work. M = one fe_mul = 81 + 9 (the fold by
# 1216), S = one fe_sqr = 45 + 9.
M, S = 90, 54
POW250 = (249, 10)                       # squarings, products of z^(2^250 - 1)
DECODE = (1 + 2 + POW250[0] + 2 + 1,     # y^2; v^3, v^7; the chain; r^2
          1 + 2 + 1 + POW250[1] + 1 + 2 + 1 + 1 + 1 + 1)  # d y^2; v^3, v^7; u v^7; chain; u v^3 t; check; -u i; r i; X Y
TABLE = (0, 8 + 7 * 8)                   # eight cached forms (2 d T), seven additions of 4 + 4
DOUBLINGS = (252 * 4, 252 * 3 + 63)      # 63 steps of four; T where an addition follows
ADDS_B = (0, 60 * 6 + 56)                # 64 x 15/16 mixed additions of 3 + 3, T when A's digit is not 0
ADDS_A = (0, 60 * 7)                     # 64 x 15/16 additions of 4 + 3
ENCODE = (POW250[0] + 5, POW250[1] + 1 + 2)
PARTS = (DECODE, TABLE, DOUBLINGS, ADDS_B, ADDS_A, ENCODE)
PRODUCTS_PER_VERIFY = sum(s for s, _ in PARTS) * S + sum(m for _, m in PARTS) * M


def make_tuples(gv, n, seed):
    from smartbft_amd import gpuverify as g
    rng = np.random.default_rng(seed)
    sc = rng.integers(0, 256, size=(2 * n, 32), dtype=np.uint8)
    sc[:, 31] &= 0x0F  # below 2^252 < L
    zero = np.zeros((65536, 32), dtype=np.uint8)
    pts = np.concatenate([gv.selftest_ed25519(g.ED_OP_BASE_MULT, sc[i:i + 65536], zero[:len(sc[i:i + 65536])])
                          for i in range(0, 2 * n, 65536)])
    pub, rb = pts[:n], pts[n:]
    assert len(set(map(bytes, pub))) == n, "keys are not distinct"
    msg = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    sig = np.empty((n, 64), dtype=np.uint8)
    sig[:, :32] = rb
    for i in range(n):
        k = int.from_bytes(hashlib.sha512(rb[i].tobytes() + pub[i].tobytes() + msg[i].tobytes()).digest(), "little")
        s = (int.from_bytes(sc[n + i].tobytes(), "little") + k * int.from_bytes(sc[i].tobytes(), "little")) % L
        sig[i, 32:] = np.frombuffer(s.to_bytes(32, "little"), dtype=np.uint8)
    want = np.ones(n, dtype=np.uint8)
    bad = np.arange(3, n, 10)  # one in ten: a bit flipped in the key, the signature or the message
    which = rng.integers(0, 3, size=len(bad))
    for arr, w in ((pub, 0), (sig, 1), (msg, 2)):
        rows = bad[which == w]
        arr[rows, rng.integers(0, arr.shape[1], size=len(rows))] ^= (1 << rng.integers(0, 8, size=len(rows))).astype(np.uint8)
    want[bad] = 0
    return msg, sig, pub, want


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=25519)
    args = ap.parse_args()
    import torch
    from smartbft_amd import GpuVerifier
    assert torch.cuda.is_available(), "needs a GPU"
    gv = GpuVerifier(device_mask=1)
    n = args.n
    msg, sig, pub, want = make_tuples(gv, n, args.seed)
    dev = torch.device("cuda:0")
    d_blob = torch.from_numpy(msg.reshape(-1)).to(dev)
    d_off = (torch.arange(n, dtype=torch.int64) * 32).to(dev)
    d_len = torch.full((n,), 32, dtype=torch.int32, device=dev)
    d_sig, d_pub = torch.from_numpy(sig).to(dev), torch.from_numpy(pub).to(dev)
    d_ok = torch.zeros(n, dtype=torch.uint8, device=dev)
    st = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    for _ in range(args.warmup):
        gv.verify_ed25519_dev(d_blob, d_off, d_len, d_sig, d_pub, d_ok, stream=st, check=False)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(args.steps):
        gv.verify_ed25519_dev(d_blob, d_off, d_len, d_sig, d_pub, d_ok, stream=st, check=False)
    e1.record(st)
    e1.synchronize()
    ms = e0.elapsed_time(e1) / args.steps
    got = d_ok.cpu().numpy()
    rate = n / (ms * 1e-3)
    print(json.dumps({
        "bench": "ed25519_verify_dev", "n": n, "steps": args.steps, "warmup": args.warmup,
        "verifies_per_s": round(rate, 1), "ms_per_step": round(ms, 4),
        "products_per_verify": PRODUCTS_PER_VERIFY,
        "fraction_of_mad_peak": round(PRODUCTS_PER_VERIFY * rate / MAD_PEAK, 4),
        "accepted": int(got.sum()), "expected_accepted": int(want.sum()),
        "verdicts_ok": bool(np.array_equal(got, want)),
    }))
    gv.close()
    if not np.array_equal(got, want):
        sys.exit(1)


if __name__ == "__main__":
    main()
