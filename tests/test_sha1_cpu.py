"""CPU-only checks of the SHA-1 ciphertext hash (no GPU): the host tier's one-shot digest
(xs_host_hash) against hashlib and the FIPS 180 vectors, the digest sizes, rejection of an unknown
hash type before anything is launched or read, and xs::HostSha1 fed in pieces -- a stand-alone
program (tests/native/sha1_host_main.cpp) built under AddressSanitizer + UBSan and run as its own
process, with the portable block function and, where the CPU has them, the SHA extensions.
"""
import ctypes
import hashlib
import os
import shutil
import subprocess

import pytest

from rclone_amd import _lib
from rclone_amd.testdata import splitmix64_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
XS_HASH_MD5, XS_HASH_SHA1 = 1, 2  # include/rclone_crypt_gpu.h (rclone's hash.Type values)
XS_ERR_INVALID, RC_ERR_INVALID = -1, -121


def _host_hash(ht, data: bytes) -> bytes:
    L = _lib.lib()
    out = ctypes.create_string_buffer(int(L.xs_hash_size(ht)))
    assert L.xs_host_hash(ht, data, len(data), out) == 0, _lib.last_error()
    return out.raw


def test_host_hash_vs_hashlib():
    data = splitmix64_bytes(41, (1 << 20) + 13)
    for n in list(range(0, 201)) + [(1 << 20) + 13]:
        assert _host_hash(XS_HASH_SHA1, data[:n]) == hashlib.sha1(data[:n]).digest(), n
        assert _host_hash(XS_HASH_MD5, data[:n]) == hashlib.md5(data[:n]).digest(), n


def test_fips_180_vectors():
    vectors = {
        b"": "da39a3ee5e6b4b0d3255bfef95601890afd80709",
        b"abc": "a9993e364706816aba3e25717850c26c9cd0d89d",
        b"abcdbcdecdefdefgefghfghighijhijkijkljklmklmnlmnomnopnopq": "84983e441c3bd26ebaae4aa1f95129e5e54670f1",
    }
    assert len(list(vectors)[2]) == 56
    for msg, want in vectors.items():
        assert _host_hash(XS_HASH_SHA1, msg).hex() == want


def test_hash_size():
    L = _lib.lib()
    assert [L.xs_hash_size(t) for t in (XS_HASH_MD5, XS_HASH_SHA1, 0, 3, 4, -1)] == [16, 20, 0, 0, 0, 0]


def test_unknown_hash_type_is_invalid():
    # the type is checked before any HIP call and before any source is read
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    assert L.xs_hash_batch_dev(3, buf, 1, buf, 64, buf, buf, None) == XS_ERR_INVALID
    assert "xs_hash_batch_dev" in _lib.last_error() and "3" in _lib.last_error()
    assert L.xs_host_hash(3, buf, 0, buf) == XS_ERR_INVALID
    from rclone_amd import crypt
    c = crypt.Cipher("", "")
    reads = []

    class Src:
        def read_go(self, n):
            reads.append(n)
            return b"", crypt.EOF

    bridge = crypt._ReaderBridge(Src(), closer=True)
    arr = (_lib.RcReader * 1)(bridge.c)
    dig = ctypes.create_string_buffer(20)
    errs = (ctypes.c_int32 * 1)()
    assert L.rc_hash_batch_with_nonce_type(c._h, 3, 1, arr, bytes(24), dig, errs) == RC_ERR_INVALID
    assert "rc_hash_batch_with_nonce_type" in _lib.last_error()
    assert L.rc_compute_hash_with_nonce_type(c._h, 3, bridge.c, bytes(24), dig) == RC_ERR_INVALID
    assert reads == []
    with pytest.raises(ValueError):
        c.hash_batch_with_nonce([(bytes(24), Src())], "sha256")


def test_host_sha1_incremental_standalone(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "sha1_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "sha1_host_main.cpp")])
    env = dict(os.environ)
    env.setdefault("ASAN_OPTIONS", "detect_leaks=1")
    p =subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    lens = [0, 1, 55, 56, 63, 64, 65, 119, 120, 128, 1000, 65584]
    want = {n: hashlib.sha1(bytes((131 * i + 7) & 255 for i in range(n))).hexdigest() for n in lens}
    seen = {}
    shani = None
    for line in p.stdout.splitlines():
        f = line.split()
        if f[0] == "shani" and len(f) == 2:
            shani = int(f[1])
            continue
        impl, n, piece, hexd = f[0], int(f[1]), int(f[2]), f[3]
        assert hexd == want[n], line
        seen.setdefault(impl, set()).add((n, piece))
    every = {(n, piece) for n in lens for piece in (1, 7, 64, 100, 0)}
    assert seen["portable"] == every
    assert shani in (0, 1)
    if shani:  # both block functions give the same digests
        assert seen["shani"] == every
    else:
        assert set(seen) == {"portable"}
