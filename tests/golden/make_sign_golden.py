#!/usr/bin/env python3
"""Generates tests/golden/sign_kat.bin: known answers of the reference's signer.

Dev container only: pub and sig come from fd_ed25519_public_from_private and
fd_ed25519_sign of the reference's AVX-512 build (oracle/_ref/
libfdref_avx512.so, built by `make -C oracle ref`).  The keys are fresh, from
a fixed numpy seed.

Record:  u32 msg_sz, u8 prv[32], u8 pub[32], u8 sig[64], u8 msg[msg_sz]

Message lengths: every length 0..300 (the padding edges of both hashes:
79/80/95/96/97 for the 32-byte header of r's hash, 47/48/63/64/65 for the
64-byte header of k's, and the second-block edges of both), eight records at
1232, one at 65535, then the seeds of the reference's fuzz corpus
(corpus/fuzz_ed25519_sigverify: prv || msg, the inputs fuzz_seeds.bin was
made from, cross-checked against it).
"""
import ctypes
import os
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from golden_io import read_sigs  # noqa: E402
from make_golden import REF_SRC  # noqa: E402  (the reference's source tree, FD_REF_SRC)


def main():
    lib = ctypes.CDLL(os.path.join(REPO, "oracle", "_ref", "libfdref_avx512.so"))
    lib.fdref_sign.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_ulong, ctypes.c_char_p, ctypes.c_char_p]
    lib.fdref_public_from_private.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    assert lib.fdref_backend_avx512() == 1

    def record(prv, msg):
        pub = ctypes.create_string_buffer(32)
        lib.fdref_public_from_private(pub, prv)
        sig = ctypes.create_string_buffer(64)
        lib.fdref_sign(sig, msg, len(msg), pub.raw, prv)
        return struct.pack("<I", len(msg)) + prv + pub.raw + sig.raw + msg, sig.raw

    rng = np.random.default_rng(20250)
    out = []
    for n in list(range(0, 301)) + [1232] * 8 + [65535]:
        out.append(record(rng.bytes(32), rng.bytes(n))[0])
    d = os.path.join(os.path.dirname(REF_SRC), "corpus", "fuzz_ed25519_sigverify")
    seeds = [open(os.path.join(d, name), "rb").read() for name in sorted(os.listdir(d))]
    seeds = [s for s in seeds if len(s) >= 32]
    fz = read_sigs("fuzz_seeds.bin")
    assert len(seeds) == len(fz) == 4, (len(seeds), len(fz))
    for s, f in zip(seeds, fz):
        rec, sig = record(s[:32], s[32:])
        assert sig == f["sig"] and s[32:] == f["msg"]
        out.append(rec)
    blob = b"".join(out)
    assert len(blob) < 400 * 1000, len(blob)
    open(os.path.join(HERE, "sign_kat.bin"), "wb").write(blob)
    print("sign_kat.bin: %d records, %d bytes" % (len(out), len(blob)))


if __name__ == "__main__":
    main()
