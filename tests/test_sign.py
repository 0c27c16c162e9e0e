"""GPU: batch Ed25519 signing and key derivation (fd_ed25519_gpu_sign_batch,
fd_ed25519_gpu_public_from_private_batch and their device-resident forms)
against the reference's known answers (tests/golden/sign_kat.bin), a plain
RFC 8032 signer on Python integers and hashlib, the reference's own signer
where its build is present, and the library's verifier."""
import ctypes
import hashlib
import os
import struct

import numpy as np
import pytest

import firedancer_amd as fa

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -103          # FD_ED25519_GPU_ERR_ARG

# ---- RFC 8032 on Python integers (extended coordinates, a = -1) ----
P = 2**255 - 19
L = 2**252 + 27742317777372353535851937790883648493
D = -121665 * pow(121666, P - 2, P) % P


def _pt_add(p, q):
    x1, y1, z1, t1 = p
    x2, y2, z2, t2 = q
    a = (y1 - x1) * (y2 - x2) % P
    b = (y1 + x1) * (y2 + x2) % P
    c = 2 * D * t1 * t2 % P
    d = 2 * z1 * z2 % P
    e, f, g, h = b - a, d - c, d + c, b + a
    return e * f % P, g * h % P, f * g % P, e * h % P


def _base_powers():
    y = 4 * pow(5, P - 2, P) % P
    xx = (y * y - 1) * pow(D * y * y + 1, P - 2, P) % P
    x = pow(xx, (P + 3) // 8, P)
    if (x * x - xx) % P:
        x = x * pow(2, (P - 1) // 4, P) % P
    if x & 1:
        x = P - x
    pw = [(x, y, 1, x * y % P)]
    for _ in range(255):
        pw.append(_pt_add(pw[-1], pw[-1]))
    return pw


_BPOW = _base_powers()


def _base_mul_enc(s):
    q = (0, 1, 1, 0)
    for i in range(256):
        if (s >> i) & 1:
            q = _pt_add(q, _BPOW[i])
    zi = pow(q[2], P - 2, P)
    x, y = q[0] * zi % P, q[1] * zi % P
    return (y | ((x & 1) << 255)).to_bytes(32, "little")


def _expand(seed):
    h = hashlib.sha512(seed).digest()
    return int.from_bytes(h[:32], "little") & ~7 & ~(1 << 255) | (1 << 254), h[32:]


def py_public(seed):
    return _base_mul_enc(_expand(seed)[0])


def py_sign(seed, pub, msg):
    a, prefix = _expand(seed)
    r = int.from_bytes(hashlib.sha512(prefix + msg).digest(), "little") % L
    R = _base_mul_enc(r)
    k = int.from_bytes(hashlib.sha512(R + pub + msg).digest(), "little") % L
    return R + ((r + k * a) % L).to_bytes(32, "little")


# ---- fixtures ----

def read_sign_kat():
    """-> list of (prv, pub, sig, msg) of tests/golden/sign_kat.bin (format: make_sign_golden.py)."""
    data = open(os.path.join(REPO, "tests", "golden", "sign_kat.bin"), "rb").read()
    out, off = [], 0
    while off < len(data):
        (sz,) = struct.unpack_from("<I", data, off); off += 4
        prv, pub, sig = data[off:off + 32], data[off + 32:off + 64], data[off + 64:off + 128]; off += 128
        out.append((prv, pub, sig, data[off:off + sz])); off += sz
    return out


@pytest.fixture(scope="module")
def pool():
    """600 (prv, pub, msg, sig) with pub and sig from the Python signer, computed once: lengths 0 and
    1232 alternating over the first wave and a half, then mixed; records 0, 63 and 64 the same (key, msg)."""
    rng = np.random.default_rng(77)
    recs = []
    for i in range(600):
        n = (0 if i % 2 == 0 else 1232) if i < 96 else int(rng.integers(0, 400))
        recs.append((rng.bytes(32), rng.bytes(n)))
    recs[63] = recs[64] = recs[0]
    out = []
    for prv, msg in recs:
        pub = py_public(prv)
        out.append((prv, pub, msg, py_sign(prv, pub, msg)))
    return out


def _sign(g, recs):
    arena, desc, sz = fa.pack_sign_batch([(p, a, m) for p, a, m, _ in recs])
    return g.sign_batch(arena, sz, desc)


# ---- tests ----

def test_golden_known_answers(gpu):
    kat = read_sign_kat()
    assert len(kat) == 301 + 8 + 1 + 4
    pubs = gpu.public_from_private_batch(b"".join(k[0] for k in kat))
    arena, desc, sz = fa.pack_sign_batch([(prv, pub, msg) for prv, pub, _, msg in kat])
    sigs = gpu.sign_batch(arena, sz, desc)
    for i, (prv, pub, sig, msg) in enumerate(kat):
        assert pubs[i].tobytes() == pub, (i, len(msg))
        assert sigs[i].tobytes() == sig, (i, len(msg))


def test_independent_rfc8032_signer(gpu, pool):
    recs = pool[96:224]                                  # 128 random (seed, msg) pairs
    pubs = gpu.public_from_private_batch(np.frombuffer(b"".join(r[0] for r in recs), np.uint8))
    sigs = _sign(gpu, recs)
    for i, (prv, pub, msg, sig) in enumerate(recs):
        assert pubs[i].tobytes() == pub, i
        assert sigs[i].tobytes() == sig, (i, len(msg))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_counts(gpu, pool, n):
    """Partial waves and workgroups; the first 96 lanes alternate 0 and 1232 bytes (block counts diverge
    inside a wave); lanes 0, 63 and 64 carry the same (key, msg)."""
    sigs = _sign(gpu, pool[:n])
    pubs = gpu.public_from_private_batch(b"".join(r[0] for r in pool[:n]))
    for i in range(n):
        assert sigs[i].tobytes() == pool[i][3], (n, i)
        assert pubs[i].tobytes() == pool[i][1], (n, i)
    if n >= 65:
        assert sigs[0].tobytes() == sigs[63].tobytes() == sigs[64].tobytes()


def test_split_above_max_batch_and_round_trip(gpu, pool):
    """A context with max_batch 256 signs 600 in three launches; the signatures verify (code 0) and
    fail with ERR_MSG (-3) after one message bit is flipped."""
    g = fa.Ed25519Gpu(device_mask=1, max_batch=256)
    try:
        sigs = _sign(g, pool)
        pubs = g.public_from_private_batch(b"".join(r[0] for r in pool))
    finally:
        g.close()
    for i, (prv, pub, msg, sig) in enumerate(pool):
        assert sigs[i].tobytes() == sig, i
        assert pubs[i].tobytes() == pub, i
    arena, desc, sz = fa.pack_batch([(msg, sigs[i].tobytes(), pub) for i, (_, pub, msg, _) in enumerate(pool)])
    assert (gpu.verify_batch(arena, sz, desc) == 0).all()
    rng = np.random.default_rng(5)
    flipped = []
    for i, (_, pub, msg, _) in enumerate(pool):
        m = bytearray(msg) if msg else bytearray(b"\0")  # an empty message grows by one byte instead
        if msg:
            m[int(rng.integers(0, len(m)))] ^= 1 << int(rng.integers(0, 8))
        flipped.append((bytes(m), sigs[i].tobytes(), pub))
    arena, desc, sz = fa.pack_batch(flipped)
    assert (gpu.verify_batch(arena, sz, desc) == fa.FD_ED25519_ERR_MSG).all()


def test_message_alignment_and_arena_end(gpu, pool):
    """msg_off at each of the four byte alignments (keys too), the last message ending on the arena's last byte."""
    recs = [pool[1], pool[100], pool[101], pool[3]]
    for al in range(4):
        blob, desc = bytearray(b"\x5a" * al), np.zeros(len(recs), fa.SIGN_DESC_DTYPE)
        for i, (prv, pub, msg, _) in enumerate(recs):
            off = len(blob)
            blob += prv + pub + msg
            desc[i] = (off, off + 32, off + 64, len(msg), 0)
        assert desc[0]["msg_off"] % 4 == al
        sz = len(blob)
        assert desc[-1]["msg_off"] + desc[-1]["msg_sz"] == sz
        sigs = gpu.sign_batch(np.frombuffer(bytes(blob), np.uint8), sz, desc)
        for i, r in enumerate(recs):
            assert sigs[i].tobytes() == r[3], (al, i)
    seen = set()
    for al in range(4):                                   # and one message at every alignment on its own
        prv, pub, msg, sig = pool[97 + al]
        blob = b"\x5a" * al + msg + prv + pub
        desc = np.zeros(1, fa.SIGN_DESC_DTYPE)
        desc[0] = (al + len(msg), al + len(msg) + 32, al, len(msg), 0)
        seen.add(al % 4)
        assert gpu.sign_batch(np.frombuffer(blob, np.uint8), len(blob), desc)[0].tobytes() == sig, al
    assert seen == {0, 1, 2, 3}


def test_device_resident_forms(gpu, pool):
    import torch
    recs = pool[:300]
    arena, desc, sz = fa.pack_sign_batch([(p, a, m) for p, a, m, _ in recs])
    host_sigs = gpu.sign_batch(arena, sz, desc)
    host_pubs = gpu.public_from_private_batch(b"".join(r[0] for r in recs))
    dev = torch.device("cuda:0")
    pad = np.zeros(((sz + 3) & ~3) + 8, np.uint8); pad[:sz] = arena[:sz]
    d_arena = torch.from_numpy(pad).to(dev)
    d_desc = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
    d_sig = torch.full((len(recs) * 64,), 0xee, dtype=torch.uint8, device=dev)
    d_prv = torch.from_numpy(np.frombuffer(b"".join(r[0] for r in recs), np.uint8).copy()).to(dev)
    d_pub = torch.full((len(recs) * 32,), 0xee, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    gpu.sign_batch_dev(d_arena.data_ptr(), sz, d_desc.data_ptr(), len(recs), d_sig.data_ptr(), stream=st)
    gpu.public_from_private_batch_dev(d_prv.data_ptr(), len(recs), d_pub.data_ptr(), stream=st)
    torch.cuda.synchronize()
    assert np.array_equal(d_sig.cpu().numpy().reshape(-1, 64), host_sigs)
    assert np.array_equal(d_pub.cpu().numpy().reshape(-1, 32), host_pubs)
    assert np.array_equal(d_prv.cpu().numpy(), np.frombuffer(b"".join(r[0] for r in recs), np.uint8))   # left alone
    for i, r in enumerate(recs):
        assert host_sigs[i].tobytes() == r[3] and host_pubs[i].tobytes() == r[1], i


def test_arguments(gpu, pool):
    arena, desc, sz = fa.pack_sign_batch([(p, a, m) for p, a, m, _ in pool[:8]])
    lib = gpu.lib

    def call(d, n=None):
        out = np.full((len(d), 64), 0xcd, np.uint8)
        r = lib.fd_ed25519_gpu_sign_batch(gpu.ctx, arena.ctypes.data_as(ctypes.c_void_p), sz,
                                          d.ctypes.data_as(ctypes.c_void_p), len(d) if n is None else n,
                                          out.ctypes.data_as(ctypes.c_void_p))
        return r, out

    r, out = call(desc)
    assert r == 0 and out[0].tobytes() == pool[0][3]
    for field, val in [("prv_off", sz - 31), ("pub_off", sz - 31), ("prv_off", 0xfffffff0), ("pub_off", 0xffffffff),
                       ("msg_off", sz + 1), ("msg_off", 0xffffffff)]:
        d = desc.copy(); d[5][field] = val
        r, out = call(d)
        assert r == ERR_ARG and (out == 0xcd).all(), (field, val, r)
    d = desc.copy(); d[7]["msg_sz"] = d[7]["msg_sz"] + 1          # one byte past the arena's end
    r, out = call(d)
    assert r == ERR_ARG and (out == 0xcd).all()
    r, out = call(desc, n=0)
    assert r == 0 and (out == 0xcd).all()
    assert lib.fd_ed25519_gpu_public_from_private_batch(gpu.ctx, None, 0, None) == 0
    assert lib.fd_ed25519_gpu_sign_batch_dev(gpu.ctx, 0, None, 0, None, 0, None, None) == 0
    assert lib.fd_ed25519_gpu_public_from_private_batch_dev(gpu.ctx, 0, None, 0, None, None) == 0
    assert len(gpu.sign_batch(arena, sz, desc[:0])) == 0
    with pytest.raises(fa.GpuError):
        d = desc.copy(); d[0]["prv_off"] = sz
        gpu.sign_batch(arena, sz, d)


def test_reference_signer_where_present(gpu):
    path = os.path.join(REPO, "oracle", "_ref", "libfdref_avx512.so")
    if not os.path.exists(path):
        pytest.skip("oracle/_ref not built (dev container only)")
    ref = ctypes.CDLL(path)
    ref.fdref_public_from_private.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    ref.fdref_sign.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_ulong, ctypes.c_char_p, ctypes.c_char_p]
    rng = np.random.default_rng(2048)
    recs, exp = [], []
    for _ in range(2048):
        prv, msg = rng.bytes(32), rng.bytes(int(rng.integers(0, 1233)))
        pub = ctypes.create_string_buffer(32); ref.fdref_public_from_private(pub, prv)
        sig = ctypes.create_string_buffer(64); ref.fdref_sign(sig, msg, len(msg), pub.raw, prv)
        recs.append((prv, pub.raw, msg)); exp.append(sig.raw)
    arena, desc, sz = fa.pack_sign_batch(recs)
    sigs = gpu.sign_batch(arena, sz, desc)
    pubs = gpu.public_from_private_batch(b"".join(r[0] for r in recs))
    for i in range(len(recs)):
        assert pubs[i].tobytes() == recs[i][1], i
        assert sigs[i].tobytes() == exp[i], (i, len(recs[i][2]))
