"""Shared helpers of the Ed25519 tests: the golden fixture, batch packing, and the OpenSSL / Node
checkers (tests/native/ed25519_xcheck.*)."""
import json
import os
import shutil
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
BIN = os.path.join(GOLDEN, "ed25519_vectors.bin")


def load_fixture():
    """[(pub, sig, msg, verdict, category)], category names."""
    raw = open(BIN, "rb").read()
    names = json.load(open(os.path.join(GOLDEN, "ed25519_categories.json")))["categories"]
    recs, p = [], 0
    while p < len(raw):
        n = raw[p + 96] | raw[p + 97] << 8
        recs.append((raw[p:p + 32], raw[p + 32:p + 96], raw[p + 98:p + 98 + n], raw[p + 98 + n], raw[p + 99 + n]))
        p += 100 + n
    assert p == len(raw)
    return recs, names


def pack_records(recs):
    """The checkers' input stream: pub | sig | u16 len | msg | two bytes."""
    return b"".join(r[0] + r[1] + len(r[2]).to_bytes(2, "little") + r[2] + b"\0\0" for r in recs)


def pack_batch(recs, shift=0):
    """(blob, off, len, sig, pub, want) numpy arrays of a batch: the messages packed with no gaps
    behind `shift` leading bytes (so offsets take every alignment), the blob exactly that long."""
    blob = bytearray(shift)
    off, ln = [], []
    for r in recs:
        off.append(len(blob))
        ln.append(len(r[2]))
        blob += r[2]
    n = len(recs)
    sig = np.frombuffer(b"".join(r[1] for r in recs), dtype=np.uint8).reshape(n, 64).copy()
    pub = np.frombuffer(b"".join(r[0] for r in recs), dtype=np.uint8).reshape(n, 32).copy()
    want = np.array([r[3] for r in recs], dtype=np.uint8)
    return (np.frombuffer(bytes(blob), dtype=np.uint8).copy(), np.array(off, dtype=np.uint64),
            np.array(ln, dtype=np.uint32), sig, pub, want)


def by_category(recs, names, bad):
    """'category: count' summary of the records at indices `bad`."""
    out = {}
    for i in bad:
        out[names[recs[i][4]]] = out.get(names[recs[i][4]], 0) + 1
    return ", ".join(f"{k}: {v}" for k, v in sorted(out.items()))


def build_openssl_checker(dirname):
    """Path of the built OpenSSL checker, or None when the OpenSSL headers are absent."""
    if not os.path.exists("/usr/include/openssl/evp.h"):
        return None
    exe = os.path.join(str(dirname), "ed25519_xcheck")
    subprocess.run(["cc", "-O2", "-o", exe, os.path.join(HERE, "native", "ed25519_xcheck.c"), "-lcrypto"],
                   check=True)
    return exe


def run_checker(cmd, recs):
    out = subprocess.run(cmd, input=pack_records(recs), capture_output=True, check=True).stdout.decode().strip()
    assert len(out) == len(recs)
    return [int(c) for c in out]


def openssl_sign(exe, seeds, msgs):
    """[(pub, sig)] for seeds[i] over msgs[i], signed by the checker's sign mode."""
    data = b"".join(s + len(m).to_bytes(2, "little") + m for s, m in zip(seeds, msgs))
    out = subprocess.run([exe, "sign"], input=data, capture_output=True, check=True).stdout
    assert len(out) == 96 * len(seeds)
    return [(out[96 * i:96 * i + 32], out[96 * i + 32:96 * i + 96]) for i in range(len(seeds))]


def node_cmd():
    node = shutil.which("node")
    return [node, os.path.join(HERE, "native", "ed25519_xcheck.js")] if node else None
