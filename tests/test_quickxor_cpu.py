"""CPU-only checks of the QuickXorHash ciphertext hash (no GPU): the host hasher's one-shot digest
(xs_host_hash) against the reference's 70 test vectors (tests/golden/quickxor_vectors.json, data
only) and against a restatement of the hash's bit rule kept in this file, the digest sizes, the
Python type tables, and xs::HostQuickXor fed in pieces with final() after every piece -- a
stand-alone program (tests/native/quickxor_host_main.cpp) built under AddressSanitizer + UBSan and
run as its own process.
"""
import base64
import ctypes
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from rclone_amd import _lib
from rclone_amd.testdata import splitmix64_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
XS_HASH_MD5, XS_HASH_SHA1, XS_HASH_QUICKXOR = 1, 2, 0x40000000  # include/rclone_crypt_gpu.h
RING = (1 << 160) - 1


def quickxor(data) -> bytes:
    """The rule, restated: stream byte i is XORed into a 160-bit ring at bit (11 i) mod 160, bits
    past 159 wrapping to bit 0; the ring is 20 little-endian bytes and the 64-bit little-endian
    length is XORed into bytes 12..19.  Bytes i and i + 160 meet the same bit (11 * 160 = 0 mod
    160), so the column-wise XOR of the stream in rows of 160 bytes is folded, 160 rotations."""
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    n = len(a)
    full = n - n % 160
    row = np.zeros(160, dtype=np.uint8)
    if full:
        row ^= np.bitwise_xor.reduce(a[:full].reshape(-1, 160), axis=0)
    row[:n - full] ^= a[full:]
    ring = 0
    for k in range(160):
        v = int(row[k]) << (11 * k % 160)
        ring ^= (v & RING) | (v >> 160)
    ring ^= n << 96  # bytes 12..19
    return ring.to_bytes(20, "little")


def _host_hash(data: bytes) -> bytes:
    L = _lib.lib()
    out = ctypes.create_string_buffer(int(L.xs_hash_size(XS_HASH_QUICKXOR)))
    assert L.xs_host_hash(XS_HASH_QUICKXOR, data, len(data), out) == 0, _lib.last_error()
    return out.raw


def _vectors():
    with open(os.path.join(ROOT, "tests", "golden", "quickxor_vectors.json")) as f:
        v = json.load(f)
    assert len(v) == 70 and v[0]["size"] == 0 and max(x["size"] for x in v) == 333
    return [(base64.b64decode(x["in"]), base64.b64decode(x["out"])) for x in v]


def test_restatement_equals_golden_vectors():
    for data, want in _vectors():
        assert quickxor(data) == want, len(data)


def test_host_hash_equals_golden_vectors():
    for data, want in _vectors():
        assert _host_hash(data) == want, len(data)


def test_host_hash_equals_restatement():
    data = splitmix64_bytes(43, (1 << 20) + 13)
    for n in list(range(0, 401)) + [(1 << 20) + 13]:
        assert _host_hash(data[:n]) == quickxor(data[:n]), n


def test_hash_size():
    L = _lib.lib()
    assert L.xs_hash_size(XS_HASH_QUICKXOR) == 20
    assert [L.xs_hash_size(t) for t in (XS_HASH_MD5, XS_HASH_SHA1, 0, 3, 4, -1)] == [16, 20, 0, 0, 0, 0]
    assert L.xs_quickxor_slice() % 160 == 0 and L.xs_quickxor_slice() > 0


def test_python_type_tables():
    from rclone_amd import crypt, cryptfs
    assert crypt.HASH_TYPES["quickxor"] == XS_HASH_QUICKXOR and crypt.HASH_SIZES[XS_HASH_QUICKXOR] == 20
    assert crypt.hash_type_id("quickxor") == XS_HASH_QUICKXOR
    with pytest.raises(ValueError):
        crypt.hash_type_id("sha256")
    data = splitmix64_bytes(44, 1000)
    r = cryptfs.MemoryRemote("quickxor")
    r.objects["a"] = data
    assert r.hashes == ("quickxor",) and r.hash("a") == quickxor(data).hex()
    with pytest.raises(ValueError):
        cryptfs.MemoryRemote("sha256")
    c = crypt.Cipher("", "")
    fs = cryptfs.CryptFs(r, c)
    assert fs.hash_type() == "quickxor"
    r.hashes = ("sha1", "quickxor")  # GetOne(): the lowest registered type
    assert fs.hash_type() == "sha1"
    r.hashes = ("crc32",)
    with pytest.raises(crypt.CryptError, match="none of md5, sha1, quickxor"):
        fs.hash_type()


def test_unknown_type_message_names_quickxor():
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    assert L.xs_host_hash(3, buf, 0, buf) == -1
    assert "XS_HASH_QUICKXOR" in _lib.last_error()


def test_host_quickxor_incremental_standalone(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "quickxor_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "quickxor_host_main.cpp")])
    env = dict(os.environ)
    env.setdefault("ASAN_OPTIONS", "detect_leaks=1")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    n = 4003
    data = bytes((131 * i + 7) & 255 for i in range(n))
    # the digest of every prefix, byte by byte (the rule itself, no rows)
    want, ring = {0: bytes(20)}, 0
    for i in range(n):
        v = data[i] << (11 * i % 160)
        ring ^= (v & RING) | (v >> 160)
        want[i + 1] = (ring ^ ((i + 1) << 96)).to_bytes(20, "little")
    assert want[n] == quickxor(data)
    seen = {}
    for line in p.stdout.splitlines():
        piece, fed, hexd = line.split()
        piece, fed = int(piece), int(fed)
        assert hexd == want[fed].hex(), line
        seen.setdefault(piece, []).append(fed)
    for piece in (1, 7, 16, 64, 100, 160, 1760):
        assert seen[piece] == [min(k, n) for k in range(piece, n + piece, piece)], piece
    assert seen[0] == [n]
