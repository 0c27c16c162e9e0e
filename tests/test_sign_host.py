"""CPU: the signer's device functions (fd_ed25519_sign_dev.h, sc_muladd and
sc_reduce256 of fd_scalar_dev.h, ge_tobytes of fd_curve25519_dev.h) compiled
for the host and held to Python integers and hashlib; the Python mirror's
descriptor layout; the header and the library agree on the new symbols."""
import ctypes
import hashlib
import os
import random
import re
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 2**255 - 19
L = 2**252 + 27742317777372353535851937790883648493
D = -121665 * pow(121666, P - 2, P) % P
BY = 4 * pow(5, P - 2, P) % P
NEW_SYMBOLS = ["fd_ed25519_gpu_sign_batch", "fd_ed25519_gpu_sign_batch_dev",
               "fd_ed25519_gpu_public_from_private_batch", "fd_ed25519_gpu_public_from_private_batch_dev"]


def _xrecover(y):
    xx = (y * y - 1) * pow(D * y * y + 1, P - 2, P) % P
    x = pow(xx, (P + 3) // 8, P)
    if (x * x - xx) % P:
        x = x * pow(2, (P - 1) // 4, P) % P
    return P - x if x & 1 else x


B = (_xrecover(BY), BY)


def _add(p, q):
    (x1, y1), (x2, y2) = p, q
    t = D * x1 * x2 * y1 * y2 % P
    return ((x1 * y2 + x2 * y1) * pow(1 + t, P - 2, P) % P, (y1 * y2 + x1 * x2) * pow(1 - t, P - 2, P) % P)


def _mul(s, p):
    q = (0, 1)
    while s:
        if s & 1:
            q = _add(q, p)
        p = _add(p, p)
        s >>= 1
    return q


def _enc(p):
    return (p[1] | ((p[0] & 1) << 255)).to_bytes(32, "little")


def rfc8032_sign(seed, pub, msg):
    h = hashlib.sha512(seed).digest()
    a = int.from_bytes(h[:32], "little") & ~7 & ~(1 << 255) | (1 << 254)
    r = int.from_bytes(hashlib.sha512(h[32:] + msg).digest(), "little") % L
    R = _enc(_mul(r, B))
    k = int.from_bytes(hashlib.sha512(R + pub + msg).digest(), "little") % L
    return R + ((r + k * a) % L).to_bytes(32, "little")


@pytest.fixture(scope="module")
def lib():
    out = os.path.join(REPO, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "sign_host_check.so")
    src = os.path.join(REPO, "tests", "csrc", "sign_host_check.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, src])
    return ctypes.CDLL(so)


def words(x, n=8):
    return (ctypes.c_uint32 * n)(*[(x >> (32 * i)) & 0xffffffff for i in range(n)])


def ival(w):
    return sum(int(x) << (32 * i) for i, x in enumerate(w))


def test_sc_muladd(lib):
    rng = random.Random(3)
    amax = 2**255 - 8
    cases = [(L - 1, amax, L - 1), (0, 0, 0), (0, amax, 0), (L - 1, 0, L - 1), (L - 1, amax, 0), (0, amax, L - 1),
             (1, L - 1, 0), (L - 1, 2**254, L - 1), (L - 1, 2**254 + L - 8, 1)]
    cases += [(rng.randrange(L), rng.randrange(2**254, 2**255) & ~7, rng.randrange(L)) for _ in range(3000)]
    for k, a, r in cases:
        s = (ctypes.c_uint32 * 8)()
        lib.t_sc_muladd(s, words(k), words(a), words(r))
        assert ival(s) == (k * a + r) % L, (k, a, r)


def test_sc_reduce256_and_comb_digits(lib):
    rng = random.Random(4)
    q = [2**254 // L, 2**255 // L]
    xs = [0, 1, L - 1, L, L + 1, 2**252 - 1, 2**252, 2**254, 2**255 - 8, 2**255 - 1, 2**256 - 1, 15 * L, 15 * L - 1]
    # a mod l just below l (and just above 0) inside the clamped range [2^254, 2^255)
    for m in range(q[0] + 1, q[1] + 1):
        xs += [m * L - 1, m * L - 8, m * L, m * L + 7]
    xs += [rng.randrange(2**254, 2**255) & ~7 for _ in range(3000)] + [rng.randrange(2**256) for _ in range(1000)]
    for x in xs:
        r = (ctypes.c_uint32 * 8)()
        lib.t_sc_reduce256(r, words(x))
        assert ival(r) == x % L, x
        d = (ctypes.c_int * 11)()
        lib.t_reduce_comb_digits(d, words(x))
        d = list(d)
        assert sum(dk << (23 * k) for k, dk in enumerate(d)) == x % L, x
        assert all(-2**22 <= dk < 2**22 for dk in d[:10]) and 0 <= d[10] <= 2**22, (x, d)


def test_ge_tobytes(lib):
    rng = random.Random(5)
    for s in [1, 2, 8, L - 1, 2**252] + [rng.randrange(1, L) for _ in range(60)]:
        enc = (ctypes.c_uint32 * 8)()
        z1 = ctypes.c_int(0)
        lib.t_base_mul_tobytes(enc, words(s), ctypes.byref(z1))
        assert z1.value == 0                      # projective input, Z != 1
        assert bytes(enc) == _enc(_mul(s, B)), s


def test_seed_expand(lib):
    rng = random.Random(6)
    for _ in range(200):
        seed = rng.randbytes(32)
        a, pre = (ctypes.c_uint32 * 8)(), (ctypes.c_uint32 * 8)()
        lib.t_seed_expand(a, pre, words(int.from_bytes(seed, "little")))
        h = hashlib.sha512(seed).digest()
        assert ival(a) == int.from_bytes(h[:32], "little") & ~7 & ~(1 << 255) | (1 << 254)
        assert bytes(pre) == h[32:]


@pytest.mark.parametrize("hw", [8, 16])
def test_header_hash_every_padding_edge(lib, hw):
    """SHA-512( header || M ) for every length 0..300 (both headers' first-
    and second-block padding edges), 1232 and 65535, at the four byte
    alignments of the message, the message ending on the arena's last byte."""
    rng = random.Random(7 + hw)
    for n in list(range(0, 301)) + [1232, 65535]:
        for al in range(4) if n <= 300 else [n & 3]:
            hdr = rng.randbytes(4 * hw)
            msg = rng.randbytes(n)
            sz = al + n
            buf = np.zeros(((sz + 3) & ~3) + 8, np.uint8)
            buf[al:sz] = np.frombuffer(msg, np.uint8)
            buf[sz:] = 0xa5                        # bytes past the message must not reach the hash
            a32 = buf.view(np.uint32)
            dg = (ctypes.c_uint32 * 16)()
            lib.t_sign_hash(dg, hw, words(int.from_bytes(hdr, "little"), hw), a32.ctypes.data_as(ctypes.c_void_p),
                            al, n, ((sz + 3) >> 2) + 1)
            assert bytes(dg) == hashlib.sha512(hdr + msg).digest(), (hw, n, al)


def test_sign_sequence_matches_rfc8032(lib):
    """The sign kernel's sequence of device functions, [r]B by double-and-add."""
    rng = random.Random(8)
    for n in [0, 1, 31, 79, 80, 96, 97, 200, 1232]:
        seed, msg = rng.randbytes(32), rng.randbytes(n)
        h = hashlib.sha512(seed).digest()
        pub = _enc(_mul(int.from_bytes(h[:32], "little") & ~7 & ~(1 << 255) | (1 << 254), B))
        pad = rng.randrange(4)
        arena = b"\x11" * pad + seed + pub + msg
        sz = len(arena)
        buf = np.zeros(((sz + 3) & ~3) + 8, np.uint8)
        buf[:sz] = np.frombuffer(arena, np.uint8)
        sig = (ctypes.c_uint32 * 16)()
        lib.t_sign(sig, buf.view(np.uint32).ctypes.data_as(ctypes.c_void_p), sz, pad, pad + 32, pad + 64, n)
        assert bytes(sig) == rfc8032_sign(seed, pub, msg), n


def test_python_mirror_layout():
    import firedancer_amd as fa
    assert fa.SIGN_DESC_DTYPE.itemsize == 16
    assert fa.SIGN_DESC_DTYPE.names == ("prv_off", "pub_off", "msg_off", "msg_sz", "rsvd")
    recs = [(b"\1" * 32, b"\2" * 32, b"abc"), (b"\3" * 32, b"\4" * 32, b"")]
    arena, desc, sz = fa.pack_sign_batch(recs)
    assert sz == 64 + 3 + 64 and len(arena) >= ((sz + 3) & ~3) + 8
    for (prv, pub, msg), d in zip(recs, desc):
        assert arena[d["prv_off"]:d["prv_off"] + 32].tobytes() == prv
        assert arena[d["pub_off"]:d["pub_off"] + 32].tobytes() == pub
        assert arena[d["msg_off"]:d["msg_off"] + d["msg_sz"]].tobytes() == msg and d["rsvd"] == 0
    assert desc[1]["msg_off"] + desc[1]["msg_sz"] == sz      # the last message ends on the arena's last byte
    for name in ("sign_batch", "sign_batch_dev", "public_from_private_batch", "public_from_private_batch_dev"):
        assert callable(getattr(fa.Ed25519Gpu, name))


def test_header_and_library_agree_on_the_new_symbols():
    import firedancer_amd as fa
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "fd_ed25519_gpu.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(fd_\w+)\s*\(", src))
    assert "fd_ed25519_sign_desc_t" in src
    if not os.path.exists(fa.lib_path()):
        subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "firedancer_amd")])
    out = subprocess.check_output(["nm", "-D", "--defined-only", fa.lib_path()]).decode()
    exported = set(ln.split()[-1] for ln in out.splitlines() if " T " in ln)
    lib = fa.load_lib()
    for f in NEW_SYMBOLS:
        assert f in declared and f in exported, f
        assert getattr(lib, f).argtypes is not None, f
