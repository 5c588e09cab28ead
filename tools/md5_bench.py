#!/usr/bin/env python3
"""GPU MD5 of crypt files (one lane per object) vs the host: device-resident kernel rate for
N objects of one sealed 64 KiB block each (65 584-byte crypt files), and the end-to-end
batched cryptcheck call (host plaintext -> GPU seal -> GPU MD5 -> 16 B/object back) for
BASELINE configs[0]'s 1000 x 64 KiB.  CPU reference: hashlib.md5 on one core.  (The oracle is
test infrastructure and is not used here; the digests' parity is tests/test_md5_gpu.py.)

--hash sha1 reports the same three numbers for the SHA-1 of SHA-1-only remotes (xs_sha1,
hashlib.sha1, the batched call with hash_type="sha1"; parity: tests/test_sha1_gpu.py), plus the
lane rate the engine's host routing uses: at 1 k objects every object has a lane of its own, so
the kernel's time is one chain's and the lane rate is one object's bytes over it.

--hash quickxor measures OneDrive's QuickXorHash (xs_quickxor; parity: tests/test_quickxor_gpu.py),
whose kernel splits every object over many workgroups, in four shapes: 1 k and 100 k one-block
objects, one 1 GiB object, and a skewed batch of one ~4 GiB object with 2 000 objects of 1..4 096
bytes (in one launch, and as the engine launches it: the long object apart from the short ones).
The yardstick of each shape is a read-only pass over the same device bytes in the same process,
torch.sum of the buffer as int32, timed alternately with the kernel.  Then the batched cryptcheck
call with QuickXorHash against MD5, alternating in both orders, on the 1000 x 64 KiB tree and on
8 x 32 MiB objects."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rclone_amd import crypt, device  # noqa: E402
from rclone_amd.testdata import splitmix64_bytes  # noqa: E402

MD5_DESC = np.dtype([("off", "<u8"), ("len", "<u8"), ("prefix", "u1", (32,)), ("prefix_len", "<u4"),
                     ("res", "<u4", (3,))])


def kernel_rate(nobj, reps=5, hash_name="md5"):
    flen = 65552  # wire body of one full block; +32 header in the prefix
    stride = (flen + 15) & ~15
    src = torch.empty(nobj * stride, dtype=torch.uint8, device="cuda")
    device.fill_random(src, 1)
    d = np.zeros(nobj, dtype=MD5_DESC)
    d["off"] = np.arange(nobj, dtype=np.uint64) * stride
    d["len"] = flen
    d["prefix_len"] = 32
    dt = torch.from_numpy(np.frombuffer(d.tobytes(), dtype=np.uint8).copy()).cuda()
    run = device.md5_batch if hash_name == "md5" else (lambda d_, s_: device.hash_batch(hash_name, d_, s_))
    run(dt, src)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run(dt, src)
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ms = sorted(ts)[len(ts) // 2]
    return {"objects": nobj, "ms": round(ms, 3), "GB_s": round(nobj * (flen + 32) / (ms * 1e-3) / 1e9, 2)}


def _stats(ts):
    ts = sorted(ts)
    return {"ms": round(ts[len(ts) // 2], 4), "min_ms": round(ts[0], 4), "max_ms": round(ts[-1], 4)}


def quickxor_shape(name, lens, prefix_len, split_at=None, reps=9):
    """One batch of objects of the given wire lengths, device-resident: the kernel and the
    read-only yardstick over the same buffer, alternating, reps timings each after a warm-up.
    split_at: also time two launches, the objects longer than split_at apart from the rest."""
    lens = np.asarray(lens, dtype=np.uint64)
    strides = (lens + np.uint64(15)) & ~np.uint64(15)
    offs = np.concatenate([[0], np.cumsum(strides)[:-1]]).astype(np.uint64)
    total = int(strides.sum())
    src = torch.empty(total, dtype=torch.uint8, device="cuda")
    device.fill_random(src, 1)
    d = np.zeros(len(lens), dtype=MD5_DESC)
    d["off"], d["len"], d["prefix_len"] = offs, lens, prefix_len

    def dev(desc):
        return torch.from_numpy(np.frombuffer(desc.tobytes(), dtype=np.uint8).copy()).cuda()

    runs = {"kernel": [dev(d)]}
    if split_at is not None:
        runs["kernel_split"] = [dev(d[lens > split_at]), dev(d[lens <= split_at])]
    words = src.view(torch.int32)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    def hash_run(ds):
        for dt in ds:
            device.hash_batch("quickxor", dt, src)

    fns = {k: (lambda ds=ds: hash_run(ds)) for k, ds in runs.items()}
    fns["yardstick_sum_int32"] = lambda: torch.sum(words)
    for _ in range(3):  # warm the clock and every shape the timed window uses
        for fn in fns.values():
            timed(fn)
    ts = {k: [] for k in fns}
    order = list(fns)
    for r in range(reps):
        for k in (order if r % 2 == 0 else order[::-1]):
            ts[k].append(timed(fns[k]))
    hashed = int(lens.sum()) + prefix_len * len(lens)
    out = {"shape": name, "objects": len(lens), "hashed_bytes": hashed, "buffer_bytes": total}
    for k, v in ts.items():
        out[k] = _stats(v)
        out[k]["GB_s"] = round((hashed if k != "yardstick_sum_int32" else total) / (out[k]["ms"] * 1e-3) / 1e9, 1)
    for k in runs:
        out[k]["of_yardstick"] = round(out["yardstick_sum_int32"]["ms"] / out[k]["ms"], 3)
    del src, words
    torch.cuda.empty_cache()
    return out


def cryptcheck_ab(nobj, size, reps=5):
    """hash_batch_with_nonce with QuickXorHash against MD5 on the same objects in the same process,
    alternating, first one leading and then the other."""
    from tests.go_readers import Buffer
    c = crypt.Cipher("potato", "")
    plains = [splitmix64_bytes(1000 + i, size) for i in range(nobj)]
    nonces = [splitmix64_bytes(5000 + i, 24) for i in range(nobj)]

    def call(hn):
        t0 = time.perf_counter()
        c.hash_batch_with_nonce([(nonces[i], Buffer(plains[i])) for i in range(nobj)], hn)
        return (time.perf_counter() - t0) * 1e3

    for hn in ("md5", "quickxor"):
        call(hn)  # warm engine
    out = {"objects": nobj, "plain_bytes_each": size}
    for lead, order in (("quickxor_leads", ("quickxor", "md5")), ("md5_leads", ("md5", "quickxor"))):
        ts = {"md5": [], "quickxor": []}
        for _ in range(reps):
            for hn in order:
                ts[hn].append(call(hn))
        out[lead] = {hn: _stats(v) for hn, v in ts.items()}
        out[lead]["quickxor_over_md5"] = round(out[lead]["quickxor"]["ms"] / out[lead]["md5"]["ms"], 3)
    return out


def quickxor_main():
    one = 65552
    rng = np.random.default_rng(1)
    small = rng.integers(1, 4097, 2000)
    res = {"hash": "quickxor", "slice_bytes": int(_lib_slice()), "kernel": [
        quickxor_shape("1k one-block objects", [one] * 1000, 32),
        quickxor_shape("100k one-block objects", [one] * 100000, 32),
        quickxor_shape("one 1 GiB object", [1 << 30], 32),
        quickxor_shape("skewed: one 4 GiB object + 2000 objects of 1..4096 bytes",
                       list(small[:1000]) + [4 << 30] + list(small[1000:]), 32, split_at=1 << 20),
    ]}
    res["cryptcheck_1000x64KiB"] = cryptcheck_ab(1000, 65536)
    res["cryptcheck_8x32MiB"] = cryptcheck_ab(8, 32 << 20, reps=3)
    print(json.dumps(res))


def _lib_slice():
    from rclone_amd import _lib
    return _lib.lib().xs_quickxor_slice()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hash", choices=("md5", "sha1", "quickxor"), default="md5")
    hn = ap.parse_args().hash
    if hn == "quickxor":
        return quickxor_main()
    res = {"kernel": [kernel_rate(n, hash_name=hn) for n in (1000, 10000, 100000)]}
    if hn != "md5":
        res["hash"] = hn
        res["lane_MB_s"] = round((65552 + 32) / (res["kernel"][0]["ms"] * 1e-3) / 1e6, 2)
    # host single-core rate
    blob = splitmix64_bytes(2, 64 << 20)
    t0 = time.perf_counter()
    hashlib.new(hn, blob).digest()
    res[f"hashlib_{hn}_1core_GB_s"] = round(len(blob) / (time.perf_counter() - t0) / 1e9, 3)
    # end-to-end batched cryptcheck of configs[0]: 1000 x 64 KiB
    from tests.go_readers import Buffer
    c = crypt.Cipher("potato", "")
    plains = [splitmix64_bytes(1000 + i, 65536) for i in range(1000)]
    nonces = [splitmix64_bytes(5000 + i, 24) for i in range(1000)]
    c.hash_batch_with_nonce([(nonces[0], Buffer(plains[0]))], hn)  # warm engine
    t0 = time.perf_counter()
    c.hash_batch_with_nonce([(nonces[i], Buffer(plains[i])) for i in range(1000)], hn)
    el = time.perf_counter() - t0
    res["cryptcheck_1000x64KiB_gpu"] = {"s": round(el, 4), "GiB_s": round(1000 * 65536 / 2**30 / el, 3)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
