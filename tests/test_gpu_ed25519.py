"""GPU tests of the Ed25519 path (smartbft_amd/csrc/ed25519_verify.hip) through the C ABI: the
SHA-512 kernel, every self-test op, the golden fixture through the host entry, batch sizes around
the wavefront and block sizes, the device-resident entry on caller streams, the split over two
slots, the error paths, and a differential run against the Python reference and OpenSSL."""
import ctypes
import hashlib
import importlib.util
import os
import random

import numpy as np
import pytest

from conftest import ROOT
import ed25519_fixture as fx
import ed25519_ref as ref

pytestmark = pytest.mark.gpu
P, L = ref.P, ref.L


@pytest.fixture(scope="module")
def fixture():
    return fx.load_fixture()


def _mixed(recs, n, seed):
    """n fixture records with accepted and rejected ones interleaved and the longest messages
    next to the empty ones (lengths mixed inside every wavefront)."""
    rng = random.Random(seed)
    acc = [r for r in recs if r[3] == 1]
    rej = [r for r in recs if r[3] == 0]
    rng.shuffle(acc)
    rng.shuffle(rej)
    long_ = [r for r in recs if len(r[2]) == 500]
    empty = [r for r in recs if len(r[2]) == 0]
    out = []
    for i in range(n):
        if i % 8 == 2:
            out.append(long_[i % len(long_)])
        elif i % 8 == 3:
            out.append(empty[i % len(empty)])
        else:
            out.append((acc if i % 2 else rej)[i % min(len(acc), len(rej))])
    return out


def _check(recs, names, got, want):
    bad = [i for i in range(len(recs)) if got[i] != want[i]]
    assert not bad, f"{len(bad)} wrong verdicts ({fx.by_category(recs, names, bad)}), first at {bad[:8]}"


def test_sha512_matches_hashlib(gpu):
    rng = random.Random(512)
    lens = [0, 1, 3, 55, 56, 63, 64, 111, 112, 113, 127, 128, 129, 239, 240, 255, 256, 1000]
    msgs = [rng.randbytes(lens[i % len(lens)]) for i in range(120)]
    rng.shuffle(msgs)
    off = np.cumsum([0] + [len(m) for m in msgs[:-1]]).astype(np.uint64)
    assert {int(o) % 4 for o in off} == {0, 1, 2, 3}
    blob = np.frombuffer(b"".join(msgs), dtype=np.uint8)  # packed with no gaps, no slack
    got = gpu.sha512(blob, off, np.array([len(m) for m in msgs], dtype=np.uint32))
    assert got.shape == (120, 64)
    for m, d in zip(msgs, got):
        assert bytes(d) == hashlib.sha512(m).digest(), len(m)


def _le(xs):
    return np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in xs), dtype=np.uint8).reshape(-1, 32)


def test_every_selftest_op_matches_python(gpu, fixture):
    from smartbft_amd import gpuverify as g
    spec = importlib.util.spec_from_file_location("gen_ed", os.path.join(ROOT, "tools", "gen_ed25519_tables.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    p0 = ref.mul_base(gen.P0_SCALAR % L)
    rng = random.Random(2048)
    edges = [0, 1, 2, P - 1, P, P + 18, 2**255 - 1, 2**256 - 1, L - 1, L, L + 1]
    n = 2048
    a = (edges + [rng.getrandbits(256) for _ in range(n)])[:n]
    b = (edges[::-1] + [rng.getrandbits(256) for _ in range(n)])[:n]
    A, B = _le(a), _le(b)

    def run(op, x=A, y=B):
        return [int.from_bytes(bytes(r), "little") for r in gpu.selftest_ed25519(op, x, y)]

    assert run(g.ED_OP_FE_MUL) == [x * y % P for x, y in zip(a, b)]
    assert run(g.ED_OP_FE_SQR) == [x * x % P for x in a]
    assert run(g.ED_OP_FE_INVERT) == [pow(x, P - 2, P) for x in a]
    assert run(g.ED_OP_SC_REDUCE) == [(x + (y << 256)) % L for x, y in zip(a, b)]
    # decode: fixture keys (weak and non-canonical ones among them), edges, random encodings
    recs, _ = fixture
    enc = [r[0] for r in recs[::3]] + [int(x).to_bytes(32, "little") for x in a]
    enc = enc[:n]
    want = []
    for e in enc:
        pt = ref.decode(e)
        want.append(2**256 - 1 if pt is None else pt[0])
    got = run(g.ED_OP_DECODE, np.frombuffer(b"".join(enc), dtype=np.uint8).reshape(-1, 32), B)
    assert got == want and 0 < sum(1 for w in want if w == 2**256 - 1) < n
    got = gpu.selftest_ed25519(g.ED_OP_BASE_MULT, A, B)
    assert [bytes(r) for r in got] == [ref.encode(ref.mul_base(x % L)) for x in a]
    # both tables; the Python side is the slow one here, so a quarter of the operands
    m = n // 4
    got = gpu.selftest_ed25519(g.ED_OP_DOUBLE_SCALAR, A[:m], B[:m])
    assert [bytes(r) for r in got] == [ref.encode(ref.add(ref.mul_base(x % L), ref.mul(y % L, p0)))
                                       for x, y in zip(a[:m], b[:m])]
    got = gpu.selftest_ed25519(g.ED_OP_DOUBLE_SCALAR, A, A)  # all 2,048 lanes: [a]B + [a]P0 = [a (1 + s0)]B
    assert [bytes(r) for r in got] == [ref.encode(ref.mul_base(x % L * (1 + gen.P0_SCALAR) % L)) for x in a]


def test_every_fixture_record_through_the_host_entry(gpu, fixture):
    recs, names = fixture
    blob, off, ln, sig, pub, want = fx.pack_batch(recs)
    _check(recs, names, gpu.verify_ed25519(blob, off, ln, sig, pub), want)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257])
def test_batch_sizes(gpu, fixture, n):
    recs, names = fixture
    sel = _mixed(recs, n, n)
    blob, off, ln, sig, pub, want = fx.pack_batch(sel, shift=n % 4)
    _check(sel, names, gpu.verify_ed25519(blob, off, ln, sig, pub), want)


def test_device_entry_on_caller_streams(gpu, fixture):
    import torch
    recs, names = fixture
    dev = torch.device("cuda:0")
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    calls = []
    for n, seed in ((300, 1), (40, 2), (200, 3)):
        sel = _mixed(recs, n, seed)
        blob, off, ln, sig, pub, want = fx.pack_batch(sel, shift=seed)
        t = [torch.from_numpy(x).to(dev) for x in (blob, off.astype(np.int64), ln.astype(np.int32), sig, pub)]
        assert t[0].numel() == seed + sum(len(r[2]) for r in sel)  # exactly the messages, no slack
        calls.append((sel, want, t, torch.full((n,), 0xAA, dtype=torch.uint8, device=dev)))
    torch.cuda.synchronize()
    # two calls of different n back to back on one stream, then one on a second stream
    for (sel, want, t, ok), st, chk in zip(calls, (s1, s1, s2), (False, False, True)):
        gpu.verify_ed25519_dev(*t, ok, stream=st, check=chk)
    torch.cuda.synchronize()
    for sel, want, t, ok in calls:
        _check(sel, names, ok.cpu().numpy(), want)


def test_split_over_two_slots(fixture):
    from smartbft_amd import GpuVerifier
    recs, names = fixture
    gv = GpuVerifier(slots_per_device=2, min_split=1)
    try:
        assert gv.device_count >= 2
        sel = _mixed(recs, 129, 129)
        blob, off, ln, sig, pub, want = fx.pack_batch(sel, shift=3)
        got = gv.verify_ed25519(blob, off, ln, sig, pub)
        _check(sel, names, got, want)
        assert 0 < int(want[65:].sum()) < 64 and np.array_equal(got[65:], want[65:])  # the second share's place
        dig = gv.sha512(blob, off, ln)
        assert [bytes(d) for d in dig] == [hashlib.sha512(r[2]).digest() for r in sel]
    finally:
        gv.close()


def test_errors(gpu, fixture):
    from smartbft_amd import gpuverify as g
    recs, names = fixture
    sel = _mixed(recs, 70, 7)
    blob, off, ln, sig, pub, want = fx.pack_batch(sel)
    u64p, u32p = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32)

    def raw(off_, ln_):
        ok = np.full(len(sel), 0xAA, dtype=np.uint8)
        rc = gpu.L.sbft_gv_verify_ed25519(gpu.ctx, g._p(blob), blob.size, off_.ctypes.data_as(u64p),
                                          ln_.ctypes.data_as(u32p), g._p(sig), g._p(pub), len(sel), g._p(ok))
        return rc, ok

    bad_ln = ln.copy()
    bad_ln[-1] += 1  # the last message ends one byte past the blob
    rc, ok = raw(off, bad_ln)
    assert rc == -1 and (ok == 0xAA).all()
    for big in ((1 << 63) - 1, (1 << 63) + 5, (1 << 64) - 1):  # off + len would wrap
        bad_off = off.copy()
        bad_off[3] = big
        rc, ok = raw(bad_off, np.maximum(ln, 2).astype(np.uint32))
        assert rc == -1 and (ok == 0xAA).all(), big
    assert gpu.L.sbft_gv_verify_ed25519(gpu.ctx, None, 0, None, None, None, None, 0, None) == 0  # n = 0
    assert gpu.L.sbft_gv_verify_ed25519(gpu.ctx, g._p(blob), blob.size, None, None, g._p(sig), g._p(pub), 3, None) == -1
    assert gpu.L.sbft_gv_selftest_ed25519(gpu.ctx, 7, g._p(pub), g._p(pub), 1, g._p(pub.copy())) == -1
    try:
        g.inject_fault(g.FAULT_LAUNCH, 1)
        with pytest.raises(g.GpuVerifyError, match=r"\(-4\)"):
            gpu.verify_ed25519(blob, off, ln, sig, pub)
    finally:
        g.inject_fault(g.FAULT_OFF, 0)
    _check(sel, names, gpu.verify_ed25519(blob, off, ln, sig, pub), want)


def _corrupt(rng, tuples, weak):
    """One in three corrupted in a random byte of key, signature or message; one in ten with its
    key replaced by a weak key of the fixture."""
    out = []
    for i, (pub, sig, msg) in enumerate(tuples):
        if i % 3 == 1:
            which = rng.randrange(3 if msg else 2)
            buf = bytearray((pub, sig, msg)[which])
            buf[rng.randrange(len(buf))] ^= 1 << rng.randrange(8)
            pub, sig, msg = [bytes(buf) if j == which else x for j, x in enumerate((pub, sig, msg))]
        if i % 10 == 7:
            pub = weak[i % len(weak)]
        out.append((pub, sig, msg))
    return out


def _weak_keys(fixture):
    recs, names = fixture
    return [r[0] for r in recs if names[r[4]] in ("small_order_key", "mixed_order_key")]


def test_differential_against_the_reference(gpu, fixture):
    rng = random.Random(500)
    tuples = []
    for i in range(500):
        seed, msg = rng.randbytes(32), rng.randbytes(rng.choice([0, 1, 32, 47, 48, 111, 112, 200]))
        tuples.append((ref.public_key(seed), ref.sign(seed, msg), msg))
    tuples = _corrupt(rng, tuples, _weak_keys(fixture))
    want = [int(ref.verify(p, m, s)) for p, s, m in tuples]  # the reference decides every tuple
    recs = [(p, s, m, w, 0) for (p, s, m), w in zip(tuples, want)]
    blob, off, ln, sig, pub, w = fx.pack_batch(recs, shift=1)
    got = gpu.verify_ed25519(blob, off, ln, sig, pub)
    assert 0 < sum(want) < len(want)
    bad = [i for i in range(len(want)) if got[i] != want[i]]
    assert not bad, bad[:8]


def test_differential_against_openssl(gpu, fixture, tmp_path):
    chk = fx.build_openssl_checker(tmp_path)
    if chk is None:
        pytest.skip("OpenSSL headers absent: cannot build tests/native/ed25519_xcheck.c")
    rng = random.Random(20000)
    n = 20000
    seeds = [rng.randbytes(32) for _ in range(n)]
    msgs = [rng.randbytes(rng.choice([0, 1, 31, 32, 48, 64, 111, 112, 113, 240])) for _ in range(n)]
    tuples = [(p, s, m) for (p, s), m in zip(fx.openssl_sign(chk, seeds, msgs), msgs)]
    tuples = _corrupt(rng, tuples, _weak_keys(fixture))
    recs = [(p, s, m, 0, 0) for p, s, m in tuples]
    want = fx.run_checker([chk], recs)  # OpenSSL decides every tuple
    blob, off, ln, sig, pub, _ = fx.pack_batch(recs, shift=2)
    got = gpu.verify_ed25519(blob, off, ln, sig, pub)
    assert 0 < sum(want) < n
    bad = [i for i in range(n) if got[i] != want[i]]
    assert not bad, (len(bad), bad[:8])
