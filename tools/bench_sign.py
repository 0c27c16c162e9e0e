#!/usr/bin/env python3
"""bench_sign.py -- batch Ed25519 signing and key derivation on device-resident
inputs (fd_ed25519_gpu_sign_batch_dev, fd_ed25519_gpu_public_from_private_batch_dev),
one JSON line per shape:

  c2   65,536 records x 200 B (bench.py config 2's shape)
  c3   1,048,576 records x 0-1232 B

The first records of each batch are the records of tests/golden/sign_kat.bin
up to 1232 B (313 of them), so a prefix of the output is held to the
reference's known answers; the rest is checked by verifying every signature
on the GPU.  Timing: warm launches, then back-to-back launches for at least
--min-s seconds between two device events.  Beside each line: the one-shot
fd_ed25519_verify_batch_gpu_dev rate of the same batch in the same process
and, where oracle/_ref is built, the reference's fd_ed25519_sign on one pinned
thread per allowed physical core (firedancer_amd.hostcpu.baseline_cpus, as
bench.py's cpu_baseline picks them).  Lines and the build id also go to --out."""
import argparse
import ctypes
import json
import os
import struct
import sys
import threading
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SHAPES = {"c2": (1 << 16, 200, 200), "c3": (1 << 20, 0, 1232)}


def read_kat(max_sz=1232):
    data = open(os.path.join(REPO, "tests", "golden", "sign_kat.bin"), "rb").read()
    out, off = [], 0
    while off < len(data):
        (sz,) = struct.unpack_from("<I", data, off); off += 4
        rec = (data[off:off + 32], data[off + 32:off + 64], data[off + 64:off + 128], data[off + 128:off + 128 + sz])
        off += 128 + sz
        if sz <= max_sz:
            out.append(rec)
    return out


def cpu_baseline(recs, budget_s=3.0):
    """fd_ed25519_sign of the reference over a sample of the batch, one pinned thread per allowed core."""
    path = os.path.join(REPO, "oracle", "_ref", "libfdref_avx512.so")
    if not os.path.exists(path):
        return None
    from firedancer_amd.hostcpu import baseline_cpus
    cpus, topo = baseline_cpus()
    lib = ctypes.CDLL(path)
    lib.fdref_sign.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_ulong, ctypes.c_char_p, ctypes.c_char_p]
    done = [0] * len(cpus)
    stop = time.perf_counter() + budget_s

    def work(t):
        try:
            os.sched_setaffinity(threading.get_native_id(), {cpus[t]})
        except OSError:
            pass
        sig = ctypes.create_string_buffer(64)
        i = t
        while time.perf_counter() < stop:
            for _ in range(64):
                prv, pub, msg = recs[i % len(recs)]
                lib.fdref_sign(sig, msg, len(msg), pub, prv)
                i += len(cpus)
            done[t] += 64

    t0 = time.perf_counter()
    th = [threading.Thread(target=work, args=(t,)) for t in range(len(cpus))]
    for x in th:
        x.start()
    for x in th:
        x.join()
    dt = time.perf_counter() - t0
    return {"value": sum(done) / dt, "unit": "sigs/s", "cores": len(cpus), "per_core": sum(done) / dt / len(cpus),
            "kind": "reference fd_ed25519_sign (ctypes call per signature)", "topology": topo}


def timed(torch, st, step, min_s):
    """Back-to-back launches of step() for at least min_s seconds between two device events -> (s per launch, launches)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(st); step(); b.record(st)
    torch.cuda.synchronize()
    reps = max(3, int(min_s * 1.15 / max(a.elapsed_time(b) * 1e-3, 1e-6)) + 1)
    a.record(st)
    for _ in range(reps):
        step()
    b.record(st)
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / reps, reps


def run_shape(fa, torch, g, name, min_s, warmup, no_cpu):
    n, lo, hi = SHAPES[name]
    rng = np.random.default_rng(11)
    kat = read_kat()
    lens = rng.integers(lo, hi + 1, n).astype(np.int64)
    lens[:len(kat)] = [len(k[3]) for k in kat]
    rec_off = np.concatenate([[0], np.cumsum(64 + lens)[:-1]]).astype(np.int64)
    sz = int(rec_off[-1] + 64 + lens[-1])
    base = (sz + 3) & ~3                                  # the signatures follow the sign arena (verify reads both)
    total = base + 64 * n
    arena = np.frombuffer(rng.bytes(total + 16), np.uint8).copy()
    for i, (prv, pub, _, msg) in enumerate(kat):
        o = int(rec_off[i])
        arena[o:o + 64 + len(msg)] = np.frombuffer(prv + pub + msg, np.uint8)
    sdesc = np.zeros(n, fa.SIGN_DESC_DTYPE)
    sdesc["prv_off"], sdesc["pub_off"], sdesc["msg_off"], sdesc["msg_sz"] = rec_off, rec_off + 32, rec_off + 64, lens
    vdesc = np.zeros(n, fa.DESC_DTYPE)
    vdesc["sig_off"], vdesc["pub_off"], vdesc["msg_off"] = base + 64 * np.arange(n), rec_off + 32, rec_off + 64
    vdesc["msg_sz"], vdesc["txn_idx"] = lens, np.arange(n) & 0xffff

    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(st)
    d_arena = torch.from_numpy(arena).to(dev)
    d_sdesc = torch.from_numpy(sdesc.view(np.uint8).copy()).to(dev)
    d_vdesc = torch.from_numpy(vdesc.view(np.uint8).copy()).to(dev)
    prv = arena[(rec_off[:, None] + np.arange(32)[None, :])].copy()          # [n, 32]
    d_prv = torch.from_numpy(prv.reshape(-1)).to(dev)
    d_pub = torch.zeros(32 * n, dtype=torch.uint8, device=dev)
    d_code = torch.zeros(n, dtype=torch.int8, device=dev)
    s = st.cuda_stream

    def pub_step():
        g.public_from_private_batch_dev(d_prv.data_ptr(), n, d_pub.data_ptr(), stream=s)

    def sign_step():
        g.sign_batch_dev(d_arena.data_ptr(), sz, d_sdesc.data_ptr(), n, d_arena.data_ptr() + base, stream=s)

    def verify_step():
        g.verify_batch_dev(d_arena.data_ptr(), total, d_vdesc.data_ptr(), n, d_code.data_ptr(), stream=s)

    # the public keys of the random records come from the key kernel (the golden prefix keeps the reference's)
    pub_step()
    torch.cuda.synchronize()
    pubs = d_pub.cpu().numpy().reshape(n, 32)
    for i, k in enumerate(kat):
        assert pubs[i].tobytes() == k[1], "public key %d differs from sign_kat.bin" % i
    idx = (rec_off[len(kat):, None] + 32 + np.arange(32)[None, :]).reshape(-1)
    d_arena[torch.from_numpy(idx).to(dev)] = d_pub[32 * len(kat):]
    torch.cuda.synchronize()

    for step in (pub_step, sign_step, verify_step):
        for _ in range(warmup):
            step()
    torch.cuda.synchronize()
    t_pub, r_pub = timed(torch, st, pub_step, min_s)
    t_sign, r_sign = timed(torch, st, sign_step, min_s)
    t_ver, r_ver = timed(torch, st, verify_step, min_s)

    # outputs: the golden prefix byte for byte, every signature through the GPU verifier
    sigs = d_arena[base:base + 64 * n].cpu().numpy().reshape(n, 64)
    for i, k in enumerate(kat):
        assert sigs[i].tobytes() == k[2], "signature %d differs from sign_kat.bin" % i
    verify_step()
    torch.cuda.synchronize()
    codes = d_code.cpu().numpy()
    assert (codes == 0).all(), "%d of %d signatures do not verify" % (int((codes != 0).sum()), n)

    cpu = None
    if not no_cpu:
        host = d_arena.cpu().numpy()
        m = min(n, 4096)
        cpu = cpu_baseline([(host[o:o + 32].tobytes(), host[o + 32:o + 64].tobytes(), host[o + 64:o + 64 + ln].tobytes())
                            for o, ln in zip(rec_off[:m].tolist(), lens[:m].tolist())])
    return {"metric": "Ed25519 signatures/sec (batched, device-resident)", "shape": name, "value": n / t_sign,
            "unit": "sigs/s", "n_gpus": 1, "higher_is_better": True, "data": "synthetic random keys and messages",
            "config": {"workload": "%d records x %s B, prv | pub | msg packed unaligned; first %d records = "
                                   "sign_kat.bin up to 1232 B" % (n, lo if lo == hi else "%d-%d" % (lo, hi), len(kat)),
                       "msg_bytes": int(lens.sum())},
            "sign_ms": t_sign * 1e3, "sign_launches": r_sign,
            "pubkey_per_s": n / t_pub, "pubkey_ms": t_pub * 1e3, "pubkey_launches": r_pub,
            "verify_oneshot_per_s": n / t_ver, "verify_oneshot_ms": t_ver * 1e3, "verify_launches": r_ver,
            "sign_over_verify": t_ver / t_sign,
            "checked": "golden prefix (%d) byte for byte, all %d through verify_batch_dev (code 0)" % (len(kat), n),
            "cpu_baseline": cpu, "build": fa.build_id()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c2,c3")
    ap.add_argument("--min-s", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r07", "sign"))
    args = ap.parse_args()
    import torch
    import firedancer_amd as fa
    os.makedirs(args.out, exist_ok=True)
    shapes = args.shapes.split(",")
    g = fa.Ed25519Gpu(device_mask=1, max_batch=max(SHAPES[s][0] for s in shapes))
    with open(os.path.join(args.out, "build_id.json"), "w") as f:
        json.dump({"build": fa.build_id(), "hip_version": fa.runtime_info().get("version")}, f)
    with open(os.path.join(args.out, "bench_sign.jsonl"), "w") as f:
        for name in shapes:
            line = json.dumps(run_shape(fa, torch, g, name, args.min_s, args.warmup, args.no_cpu))
            print(line, flush=True)
            f.write(line + "\n"); f.flush()
    g.close()


if __name__ == "__main__":
    main()
