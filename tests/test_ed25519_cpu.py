"""CPU tests of the Ed25519 path: the reference (tests/ed25519_ref.py) pinned to OpenSSL and Node
over the golden fixture, the device header (smartbft_amd/csrc/ed25519_f25.hpp, sha512_dev.hpp)
compiled for the host and checked against Python big integers -- including the kernel's whole
verify over every fixture record -- the same program under AddressSanitizer + UBSan, and the
argument plumbing of the Python wrappers. No device is needed."""
import hashlib
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import ed25519_fixture as fx
import ed25519_ref as ref

P, L = ref.P, ref.L
SRC = os.path.join(ROOT, "tests", "native", "ed25519_test.cpp")
EDGES = [0, 1, 2, P - 1, P, P + 18, 2**255 - 1, 2**256 - 1]


@pytest.fixture(scope="module")
def fixture():
    return fx.load_fixture()


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ed25519") / "ed25519_test")
    subprocess.run(["g++", "-O2", "-Wall", "-Werror", "-o", out, SRC], check=True)
    return out


def _run(exe, mode, lines):
    out = subprocess.run([exe, mode], input="".join(l + "\n" for l in lines), capture_output=True, text=True,
                         check=True).stdout.split("\n")
    assert len([l for l in out if l]) == len(lines)
    return out[:len(lines)]


# ---- 1. the fixture: three independent deciders and the committed verdict -------------------
def test_fixture_shape(fixture):
    recs, names = fixture
    assert len(names) == 15 and 1300 <= len(recs) <= 1700 and os.path.getsize(fx.BIN) < 200_000
    for c in range(15):
        assert sum(1 for r in recs if r[4] == c) >= 20, names[c]
    lens = {len(r[2]) for r in recs}
    assert lens == {0, 1, 31, 32, 47, 48, 64, 111, 112, 113, 200, 239, 240, 241, 500}
    anchor = recs[0]  # RFC 8032 section 7.1 TEST 1
    assert anchor[2] == b"" and anchor[3] == 1 and anchor[1].hex().startswith("e5564300c360ac72")
    assert anchor[0] == ref.public_key(bytes.fromhex(
        "9d61b19deffd5a60ba844af492ec2cc44449c5697b326919703bac031cae7f60"))


def test_reference_agrees_with_every_fixture_verdict(fixture):
    recs, names = fixture
    bad = [i for i, r in enumerate(recs) if int(ref.verify(r[0], r[2], r[1])) != r[3]]
    assert not bad, fx.by_category(recs, names, bad)


def test_openssl_agrees_with_every_fixture_verdict(fixture, tmp_path):
    recs, names = fixture
    chk = fx.build_openssl_checker(tmp_path)
    if chk is None:
        pytest.skip("OpenSSL headers absent: cannot build tests/native/ed25519_xcheck.c")
    got = fx.run_checker([chk], recs)
    bad = [i for i, r in enumerate(recs) if got[i] != r[3]]
    assert not bad, fx.by_category(recs, names, bad)


def test_node_agrees_with_every_fixture_verdict(fixture):
    recs, names = fixture
    cmd = fx.node_cmd()
    if cmd is None:
        pytest.skip("node absent")
    got = fx.run_checker(cmd, recs)
    bad = [i for i, r in enumerate(recs) if got[i] != r[3]]
    assert not bad, fx.by_category(recs, names, bad)


def test_generator_reproduces_the_committed_fixture():
    res = subprocess.run([sys.executable, os.path.join(fx.GOLDEN, "gen_ed25519.py"), "--check"],
                         capture_output=True, text=True)
    assert res.returncode == 0 and "identical" in res.stdout, res.stdout + res.stderr


def test_generated_constants_are_current():
    """smartbft_amd/csrc/ed25519_tables.inc is what tools/gen_ed25519_tables.py prints."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_ed25519_tables.py")],
                         capture_output=True, text=True, check=True).stdout
    assert out == open(os.path.join(ROOT, "smartbft_amd", "csrc", "ed25519_tables.inc")).read()


# ---- 2. the device header on the host ---------------------------------------------------------
def test_field_ops_match_python(exe):
    rng = random.Random(25519)
    pairs = [(a, b) for a in EDGES for b in EDGES]
    pairs += [(rng.getrandbits(256), rng.getrandbits(256)) for _ in range(20000)]
    # u / v a square, a non-square, and v = 0
    pairs += [(x * x * v % P, v) for x, v in ((rng.randrange(P), rng.randrange(1, P)) for _ in range(200))]
    out = _run(exe, "field", ["%064x %064x" % ab for ab in pairs])
    for (a, b), line in zip(pairs, out):
        f = line.split()
        r, ok = ref.sqrt_ratio(a % P, b % P)
        want = [a * b % P, a * a % P, pow(a, P - 2, P), r, int(ok)]
        assert [int(x, 16) for x in f[:4]] + [int(f[4])] == want, (hex(a), hex(b))


def test_field_ops_at_the_documented_limb_bounds(exe):
    """fe_mul / fe_sqr / fe_tobytes on limb vectors at the edges of the classes the header
    documents: T (tight), its negative, and 2T as fe_mul's second operand."""
    t_hi = [2**29 + 2**17] * 8 + [2**23 + 2**17]
    t_lo = [-2**17] * 9
    c_hi = [2**29 - 1] * 8 + [2**23 - 1]
    neg = [-x for x in t_hi]
    two = [2 * x for x in t_hi]
    rng = random.Random(3)
    rnd = [[rng.randint(lo, hi) for lo, hi in zip(t_lo, t_hi)] for _ in range(200)]
    xs = [t_hi, t_lo, c_hi, neg] + rnd
    ys = [t_hi, t_lo, c_hi, neg, two, [-x for x in two]] + rnd[:20]
    cases = [(x, y) for x in xs for y in ys]
    val = lambda v: sum(l << (29 * i) for i, l in enumerate(v))  # noqa: E731
    out = _run(exe, "limbs", [" ".join(str(l) for l in x + y) for x, y in cases])
    for (x, y), line in zip(cases, out):
        m, s, c = (int(t, 16) for t in line.split())
        assert (m, s, c) == (val(x) * val(y) % P, val(x) ** 2 % P, val(x) % P), (x, y)


def test_mul_small(exe):
    rng = random.Random(5)
    cases = [(a, c) for a in EDGES for c in (0, 1, -1, 2, 19, 121666, -121665, 2**30)]
    cases += [(rng.getrandbits(256), rng.randint(-2**30, 2**30)) for _ in range(2000)]
    out = _run(exe, "small", ["%064x %d" % ac for ac in cases])
    assert [int(l, 16) for l in out] == [a * c % P for a, c in cases]


def test_sc_reduce_and_range_check(exe):
    rng = random.Random(7)
    xs = [0, 1, L - 1, L, L + 1, 2 * L, 2**252, 2**253, 2**256 - 1, 2**256, 2**512 - 1, (2**260 - 1) << 252]
    xs += [rng.getrandbits(512) for _ in range(20000)] + [rng.getrandbits(253) for _ in range(2000)]
    out = _run(exe, "sc", ["%0128x" % x for x in xs])
    for x, line in zip(xs, out):
        r, lt = line.split()
        assert int(r, 16) == x % L and int(lt) == (x < L), hex(x)


def test_window_recoding_reconstructs_the_scalar(exe):
    rng = random.Random(9)
    ss = [0, 1, 7, 8, 9, 15, 16, L - 1, L, 2**252, 2**253 - 1] + [rng.getrandbits(253) for _ in range(5000)]
    out = _run(exe, "digits", ["%064x" % s for s in ss])
    for s, line in zip(ss, out):
        d = [int(t) for t in line.split()]
        assert len(d) == 64 and all(-8 <= t <= 7 for t in d)
        assert sum(t * 16**i for i, t in enumerate(d)) == s, hex(s)


def test_sha512_matches_hashlib_at_every_alignment(exe):
    rng = random.Random(11)
    cases = [(sh, rng.randbytes(n)) for n in (0, 1, 3, 55, 56, 63, 64, 111, 112, 113, 127, 128, 129, 239, 240,
                                              255, 256, 1000, 5000) for sh in range(4)]
    out = _run(exe, "sha512", ["%d %s" % (sh, m.hex()) for sh, m in cases])
    assert [l.strip() for l in out] == [hashlib.sha512(m).hexdigest() for _, m in cases]


def test_host_verify_matches_every_fixture_verdict(exe, fixture):
    """The kernel's algorithm (hash, decode, range check, double-scalar, encode, compare) on the
    CPU: a wrong verdict is found here before any GPU run."""
    recs, names = fixture
    got = subprocess.run([exe, "verify", fx.BIN], capture_output=True, text=True, check=True).stdout.strip()
    assert len(got) == len(recs)
    bad = [i for i, r in enumerate(recs) if int(got[i]) != r[3]]
    assert not bad, fx.by_category(recs, names, bad)


# ---- 3. the same program under the sanitizers (host code, its own main, no preload) ---------
def test_host_verify_is_clean_under_asan_and_ubsan(tmp_path, fixture):
    recs, _ = fixture
    out = str(tmp_path / "ed25519_test_san")
    subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                    "-Werror", "-o", out, SRC], check=True)
    res = subprocess.run([out, "verify", fx.BIN], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    assert res.stdout.strip() == "".join(str(r[3]) for r in recs)
    rng = random.Random(13)
    lines = "".join("%d %s\n" % (sh, rng.randbytes(n).hex()) for n in (0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129)
                    for sh in range(4))
    res = subprocess.run([out, "sha512"], input=lines, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]


# ---- 5. argument plumbing of the Python wrappers ----------------------------------------------
def test_python_wrappers_check_their_arguments():
    import torch
    from smartbft_amd import gpuverify
    from smartbft_amd.gpuverify import GpuVerifier
    for name in ("sbft_gv_verify_ed25519", "sbft_gv_verify_ed25519_dev", "sbft_gv_sha512", "sbft_gv_selftest_ed25519"):
        assert name in gpuverify.EXPORTS and hasattr(gpuverify.load_library(), name)
    assert (gpuverify.ED_OP_FE_MUL, gpuverify.ED_OP_DOUBLE_SCALAR) == (0, 6)
    sig, pub = np.zeros((3, 64), np.uint8), np.zeros((3, 32), np.uint8)
    s, p = GpuVerifier._ed_rows(sig[:, ::-1], pub, 3)  # a non-contiguous view is made contiguous
    assert s.flags.c_contiguous and s.dtype == np.uint8 and p.shape == (3, 32)
    with pytest.raises(ValueError):
        GpuVerifier._ed_rows(np.zeros((3, 32), np.uint8), pub, 3)
    with pytest.raises(ValueError):
        GpuVerifier._ed_rows(sig, np.zeros((2, 32), np.uint8), 3)
    gv = GpuVerifier.__new__(GpuVerifier)  # no context: every call below must fail before the C side
    with pytest.raises(ValueError):  # offsets and lengths of different counts
        gv.verify_ed25519(np.zeros(8, np.uint8), [0, 1], [1], sig[:2], pub[:2])
    with pytest.raises(ValueError):
        gv.verify_ed25519(np.zeros(8, np.uint8), [0, 1], [1, 1], sig, pub[:2])
    with pytest.raises(ValueError):
        gv.selftest_ed25519(0, np.zeros((2, 31), np.uint8), np.zeros((2, 32), np.uint8))
    ok = torch.zeros(2, dtype=torch.uint8)
    off, ln = torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int32)
    blob, dsig, dpub = torch.zeros(8, dtype=torch.uint8), torch.zeros(128, dtype=torch.uint8), torch.zeros(64, dtype=torch.uint8)
    with pytest.raises(ValueError, match="blob"):  # host tensors are refused
        gv.verify_ed25519_dev(blob, off, ln, dsig, dpub, ok)
    with pytest.raises(ValueError, match="blob"):
        gv.verify_ed25519_dev(blob.to(torch.int8), off, ln, dsig, dpub, ok)
    # the bounds predicate verify_ed25519_dev applies (shared with sha256_dev)
    bad = GpuVerifier._blob_bounds_bad(torch.tensor([0, 5, (1 << 63) - 2, -1]), torch.tensor([8, 4, 4, 0], dtype=torch.int32), 8)
    assert bad.tolist() == [False, True, True, True]
