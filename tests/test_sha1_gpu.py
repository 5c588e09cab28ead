"""SHA-1 of crypt ciphertext for wrapped remotes whose Hashes().GetOne() is SHA-1 (Backblaze B2,
Box): Fs.put's ciphertext hash (crypt.go:516-533) and cryptcheck's computeHashWithNonce /
ComputeHash (crypt.go:784-852), through every layer the MD5 has -- the one-lane-per-stream kernel
(xs_sha1), the batched seal + hash of the engine and the pool with host routing of long objects,
the per-object streaming paths on host cores, the encrypter's tee, and the overlay.

Checker: Python's hashlib.sha1 (FIPS 180-4) over the oracle's crypt files (orc.encrypt_file).
"""
import ctypes
import hashlib
import threading

import numpy as np
import pytest

from oracle import pyoracle as orc
from rclone_amd.testdata import splitmix64_bytes
from tests.go_readers import Buffer, CloseDetector, ErrorReader, MultiReader, Potato

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

XS_HASH_MD5, XS_HASH_SHA1 = 1, 2
HASH_DESC = np.dtype([("off", "<u8"), ("len", "<u8"), ("prefix", "u1", (32,)), ("prefix_len", "<u4"),
                      ("res", "<u4", (3,))])


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _sizes():
    # plaintext sizes whose crypt-file length (32 + n + 16*blocks) hits every tail case (the
    # SHA-1 padding rule is MD5's: one tail block below 56 bytes mod 64, else two)
    out = [0, 1, 15, 16, 31, 32, 33, 63, 64, 65, 65535, 65536, 65537, 3 * 65536 + 7]
    for r in (0, 1, 55, 56, 57, 63):
        n = 100
        while (32 + n + 16) % 64 != r:
            n += 1
        out.append(n)
    return out


def _carry_nonce(i):
    return b"\xfd" + b"\xff" * 7 + splitmix64_bytes(i, 16)  # + block index carries across byte 8


def test_sha1_kernel_vs_hashlib():
    from rclone_amd import device
    assert HASH_DESC.itemsize == 64
    # every length 0..199 under each prefix length: 600 streams = 10 workgroups, the last partial,
    # and every total % 64 (55, 56, 63, 0 among them) with 0, 16 and 32 prefix bytes
    cases = [(n, plen) for n in range(200) for plen in (0, 16, 32)]
    cases += [(n, [0, 16, 32][i % 3]) for i, n in enumerate([1000, 4095, 4096, 65535, 65536, 65584, (1 << 20) + 13])]
    offs, pos = {}, 0
    for n in sorted({n for n, _ in cases}):
        offs[n] = pos
        pos += (n + 15) & ~15
    data = splitmix64_bytes(3, pos + 64)
    src = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    rng = np.random.default_rng(9)
    desc = np.zeros(len(cases) + 3, dtype=HASH_DESC)
    expect = []
    for i, (n, plen) in enumerate(cases):
        pre = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
        desc["off"][i], desc["len"][i], desc["prefix_len"][i] = offs[n], n, plen
        desc["prefix"][i] = np.frombuffer(pre, dtype=np.uint8)
        expect.append(hashlib.sha1(pre[:plen] + data[offs[n]:offs[n] + n]).digest())
    # invalid descriptors: misaligned offset, bad prefix length, out of bounds
    for k, (off_bad, len_bad, plen_bad) in enumerate(((8, 10, 0), (0, 10, 8), (len(data) - 16, 32, 0))):
        j = len(cases) + k
        desc["off"][j], desc["len"][j], desc["prefix_len"][j] = off_bad, len_bad, plen_bad
    assert (len(desc) + 63) // 64 == 10 and len(desc) % 64
    dig, ok = device.hash_batch("sha1", desc, src)
    md5_typed, ok_md5 = device.hash_batch("md5", desc, src)
    md5_plain, ok_plain = device.md5_batch(desc, src)
    torch.cuda.synchronize()
    dig, ok = dig.cpu().numpy(), ok.cpu().numpy()
    assert dig.shape == (len(desc), 20)
    assert list(ok) == [1] * len(cases) + [0, 0, 0]
    for i, c in enumerate(cases):
        assert dig[i].tobytes() == expect[i], (i, c)
    # the typed entry point's MD5 is xs_md5_batch_dev byte for byte
    assert torch.equal(ok_md5, ok_plain) and list(ok_md5.cpu().numpy()) == list(ok)
    assert torch.equal(md5_typed, md5_plain) and md5_typed.shape == (len(desc), 16)
    with pytest.raises(ValueError):
        device.hash_batch("sha256", desc, src)


def test_hash_batch_with_nonce_sha1_vs_oracle():
    from rclone_amd import crypt
    c = crypt.Cipher("", "")
    key = bytes(32)
    items, expect = [], []
    for i, n in enumerate(_sizes()):
        plain = splitmix64_bytes(100 + i, n)
        # every fourth object and the four-block one: nonce + 3 carries across byte 8
        nonce = _carry_nonce(i) if i % 4 == 0 or n > 3 * 65536 else splitmix64_bytes(200 + i, 24)
        items.append((nonce, Buffer(plain)))
        expect.append(hashlib.sha1(orc.encrypt_file(plain, nonce, key)).digest())
    got = c.hash_batch_with_nonce(items, "sha1")
    assert got == expect


def _stage(sizes, plains):
    offs, pos = [], 0
    for n in sizes:
        offs.append(pos)
        pos += (n + 15) & ~15
    stage = bytearray(pos + 16)
    for o, p in zip(offs, plains):
        stage[o:o + len(p)] = p
    return stage, offs


def test_put_batch_hash_sha1_bodies_and_digests_vs_oracle():
    from rclone_amd import _lib
    L = _lib.lib()
    key = splitmix64_bytes(77, 32)
    sizes = _sizes() + [2 * 65536, 5 * 65536 + 3, 1 << 20]
    plains = [splitmix64_bytes(300 + i, n) for i, n in enumerate(sizes)]
    nonces = b"".join(splitmix64_bytes(400 + i, 24) if i % 5 else b"\xff" * 8 + splitmix64_bytes(i, 16)
                      for i in range(len(sizes)))
    stage, offs = _stage(sizes, plains)
    n = len(sizes)
    u64s = ctypes.c_uint64 * n
    lens_c, offs_c = u64s(*sizes), u64s(*offs)
    total = L.xs_put_body_bytes(n, lens_c)
    body = (ctypes.c_uint8 * (total + 16))()
    sha = (ctypes.c_uint8 * (20 * n))()
    sha_seal = (ctypes.c_uint8 * (20 * n))()
    sha_pool = (ctypes.c_uint8 * (20 * n))()
    src = (ctypes.c_uint8 * len(stage)).from_buffer(stage)
    e = L.xs_engine_create(0, 64, 1)
    assert e
    try:
        assert L.xs_engine_put_batch_hash(e, XS_HASH_SHA1, key, n, nonces, offs_c, lens_c, src, body, sha) == 0, \
            _lib.last_error()
        assert L.xs_engine_seal_hash(e, XS_HASH_SHA1, key, n, nonces, offs_c, lens_c, src, sha_seal) == 0, \
            _lib.last_error()
        assert L.xs_engine_put_batch_hash(e, 3, key, n, nonces, offs_c, lens_c, src, body, sha) == -1
    finally:
        L.xs_engine_destroy(e)
    # a pool of two engines on device 0 splits the objects and returns the same digests
    p = L.xs_pool_create((ctypes.c_int * 2)(0, 0), 2, 64, 1)
    assert p
    try:
        assert L.xs_pool_size(p) == 2
        assert L.xs_pool_seal_hash(p, XS_HASH_SHA1, key, n, nonces, offs_c, lens_c, src, sha_pool) == 0, _lib.last_error()
    finally:
        L.xs_pool_destroy(p)
    raw, dig = bytes(body), bytes(sha)
    bpos = 0
    for i, pl in enumerate(plains):
        want = orc.encrypt_file(pl, nonces[24 * i:24 * i + 24], key)
        blen = len(want) - 32
        assert raw[bpos:bpos + blen] == want[32:], (i, sizes[i])
        assert dig[20 * i:20 * i + 20] == hashlib.sha1(want).digest(), (i, sizes[i])
        bpos += (blen + 15) & ~15
    assert bytes(sha_seal) == dig
    assert bytes(sha_pool) == dig


def test_long_object_is_hashed_on_the_host():
    # one 32 MiB object among 200 small ones: with host threads it leaves its GPU lane (exactly one
    # object routed), with none it stays; the digests are hashlib's either way
    from rclone_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(5)
    sizes = [int(x) for x in rng.integers(1, 131072, 200)]
    big = 77
    sizes[big] = 32 << 20
    sizes[17] = 0
    offs, pos = [], 0
    for n in sizes:
        offs.append(pos)
        pos += (n + 15) & ~15
    stage = rng.integers(0, 256, pos + 16, dtype=np.uint8)
    nonces = rng.integers(0, 256, 24 * len(sizes), dtype=np.uint8).tobytes()
    key = splitmix64_bytes(12, 32)
    want = b"".join(hashlib.sha1(orc.encrypt_file(stage[o:o + n].tobytes(), nonces[24 * i:24 * i + 24], key)).digest()
                    for i, (o, n) in enumerate(zip(offs, sizes)))
    n = len(sizes)
    u64s = ctypes.c_uint64 * n
    lens_c, offs_c = u64s(*sizes), u64s(*offs)
    src = ctypes.c_void_p(stage.ctypes.data)
    st0, st1, st2 = ((ctypes.c_uint64 * 3)() for _ in range(3))
    routed = (ctypes.c_uint8 * (20 * n))()
    lanes = (ctypes.c_uint8 * (20 * n))()
    e = L.xs_engine_create(0, 256, 1)
    assert e
    try:
        L.xs_engine_set_host_md5(e, 2)
        L.xs_engine_md5_stats(e, st0)
        assert L.xs_engine_seal_hash(e, XS_HASH_SHA1, key, n, nonces, offs_c, lens_c, src, routed) == 0, _lib.last_error()
        L.xs_engine_md5_stats(e, st1)
        L.xs_engine_set_host_md5(e, 0)
        assert L.xs_engine_seal_hash(e, XS_HASH_SHA1, key, n, nonces, offs_c, lens_c, src, lanes) == 0, _lib.last_error()
        L.xs_engine_md5_stats(e, st2)
    finally:
        L.xs_engine_destroy(e)
    assert bytes(routed) == want
    assert st1[0] - st0[0] == 1 and st1[2] - st0[2] == n, (list(st0), list(st1))
    assert bytes(lanes) == bytes(routed)
    assert st2[0] == st1[0] and st2[2] - st1[2] == n, (list(st1), list(st2))


def test_compute_hash_with_nonce_sha1_per_object():
    from rclone_amd import crypt
    c = crypt.Cipher("potato", "")
    c.batch_blocks = 4
    key = c.data_key
    cases = []
    for i, n in enumerate((0, 1, 65536, 3 * 65536 + 7, 9 * 65536 + 5)):  # the last crosses seal batches
        plain = splitmix64_bytes(500 + i, n)
        nonce = splitmix64_bytes(600 + i, 24) if i != 3 else _carry_nonce(i)
        cases.append((plain, nonce, hashlib.sha1(orc.encrypt_file(plain, nonce, key)).hexdigest()))
    for plain, nonce, want in cases:
        cd = CloseDetector(Buffer(plain))
        assert c.compute_hash_with_nonce(nonce, cd, "sha1") == want, len(plain)
        assert cd.closed == 1
    # the same five from 8 threads at once: their seals are group-committed by the engine
    got, errors = {}, []

    def checker(t):
        try:
            for k, (plain, nonce, _) in enumerate(cases):
                got[(t, k)] = c.compute_hash_with_nonce(nonce, Buffer(plain), "sha1")
        except BaseException as exc:  # noqa: BLE001 -- reported by the assertion below
            errors.append(exc)

    th = [threading.Thread(target=checker, args=(t,)) for t in range(8)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
    assert got == {(t, k): cases[k][2] for t in range(8) for k in range(len(cases))}
    # ComputeHash: the nonce comes from the stored object's header
    plain, nonce, want = cases[3]
    ct = orc.encrypt_file(plain, nonce, key)
    assert c.compute_hash(Buffer(ct), Buffer(plain), "sha1") == want == hashlib.sha1(ct).hexdigest()
    # the MD5 default is unchanged
    assert c.compute_hash_with_nonce(nonce, Buffer(plain)) == hashlib.md5(ct).hexdigest()


def test_hash_errors_pass_through_sha1():
    from rclone_amd import crypt
    c = crypt.Cipher("", "")
    key = bytes(32)
    good = splitmix64_bytes(5, 70000)
    n0 = splitmix64_bytes(6, 24)
    potato = Potato()

    class BadClose(Buffer):
        def close(self):
            raise potato

    def items():
        return [(n0, Buffer(good)),
                (n0, ErrorReader(potato)),                                     # error before data
                (n0, MultiReader(Buffer(good[:30000]), ErrorReader(potato))),  # data then error
                (n0, ErrorReader(crypt.ErrUnexpectedEOF())),
                (n0, BadClose(good)),                                          # fs.CheckClose error
                (n0, Buffer(good))]

    got = c.hash_batch_with_nonce(items(), "sha1")
    want = hashlib.sha1(orc.encrypt_file(good, n0, key)).digest()
    assert got[0] == want and got[5] == want
    assert got[1] is potato and got[2] is potato and got[4] is potato
    assert isinstance(got[3], crypt.ErrUnexpectedEOF)
    # sources are closed (defer fs.CheckClose(in, &err))
    cd = CloseDetector(Buffer(good))
    assert c.hash_batch_with_nonce([(n0, cd)], "sha1")[0] == want and cd.closed == 1
    # the per-object call: the reader's or the closer's error is raised
    for k, (_, src) in enumerate(items()):
        if k in (0, 5):
            assert c.compute_hash_with_nonce(n0, src, "sha1") == want.hex()
        elif k == 3:
            with pytest.raises(crypt.ErrUnexpectedEOF):
                c.compute_hash_with_nonce(n0, src, "sha1")
        else:
            with pytest.raises(Potato):
                c.compute_hash_with_nonce(n0, src, "sha1")


def test_encrypter_tee_sha1_after_every_read():
    from rclone_amd import crypt
    c = crypt.Cipher("potato", "")
    plain = splitmix64_bytes(77, 3 * 65536 + 99)
    nonce = splitmix64_bytes(78, 24)
    ct = orc.encrypt_file(plain, nonce, c.data_key)
    e = c.encrypt_data(Buffer(plain), nonce)
    e.set_hash("md5")
    e.set_hash("sha1")  # one type per encrypter: the second call replaces the first
    m = c.encrypt_data(Buffer(plain), nonce)
    m.set_md5(True)
    assert e.hash() == hashlib.sha1(b"").digest()
    got = b""
    for want_n in (1, 31, 32, 33, 65551, 65552, 100000):
        data, err = e.read_go(want_n)
        assert err is None
        got += data
        assert got == ct[:len(got)]
        assert e.hash() == hashlib.sha1(got).digest(), (want_n, len(got))
        with pytest.raises(crypt.CryptError):
            e.md5()  # the tee is SHA-1's: no 16-byte digest
    with pytest.raises(crypt.CryptError):
        e.set_hash("sha1")  # before the first read only
    while True:
        data, err = e.read_go(1 << 20)
        got += data
        if err is not None:
            assert err is crypt.EOF
            break
    assert got == ct and e.hash() == hashlib.sha1(ct).digest()
    # an MD5 tee beside it is what it was
    got_m = b""
    for want_n in (1, 31, 32, 33, 65551, 65552, 100000):
        data, err = m.read_go(want_n)
        got_m += data
        assert m.md5() == hashlib.md5(got_m).digest() == m.hash()
    # off: no digest
    off = c.encrypt_data(Buffer(plain), nonce)
    off.set_hash("sha1")
    off.set_hash(None)
    with pytest.raises(crypt.CryptError):
        off.hash()


def _overlay_flow(hash_type):
    from rclone_amd import crypt
    from rclone_amd.cryptfs import CryptFs, MemoryRemote
    hl = getattr(hashlib, hash_type)

    class Flipping(MemoryRemote):
        """Stores one byte wrong (a transfer that corrupts the object)."""

        def put(self, remote, reader, size=-1):
            super().put(remote, reader, size)
            b = bytearray(self.objects[remote])
            b[len(b) // 2] ^= 0x10
            self.objects[remote] = bytes(b)

    c = crypt.Cipher("potato", "")
    mem = MemoryRemote(hash_type=hash_type) if hash_type != "md5" else MemoryRemote()
    assert mem.hashes == (hash_type,)
    fs = CryptFs(mem, c)
    assert fs.hash_type() == hash_type
    sizes = [0, 1, 15, 16, 100, 4095, 4096, 65535, 65536, 65537, 2 * 65536, 3 * 65536 + 7, 70000, 200000, 23, 24, 55, 56,
             1000, 5 * 65536 + 3]
    assert len(sizes) == 20
    plains = {f"obj{i:02d}": splitmix64_bytes(900 + i, n) for i, n in enumerate(sizes)}
    for name, p in plains.items():
        nonce = fs.put(name, Buffer(p), len(p))  # the put check is on: tee hash vs the remote's
        ct = orc.encrypt_file(p, nonce, c.data_key)
        assert mem.objects[name + ".bin"] == ct
        assert mem.hash(name + ".bin") == hl(ct).hexdigest()
        assert fs.compute_hash(name, Buffer(p)) == hl(ct).hexdigest()
    # a remote that stores a byte wrong: put raises, names the hash type and removes the object
    bad_mem = Flipping(hash_type=hash_type)
    bad_fs = CryptFs(bad_mem, c)
    with pytest.raises(crypt.CryptError, match=f"corrupted on transfer: {hash_type} encrypted hashes differ"):
        bad_fs.put("x", Buffer(plains["obj13"]), len(plains["obj13"]))
    assert "x.bin" not in bad_mem.objects
    # cryptcheck in both shapes: exactly the one altered source differs
    clean = {k: (lambda v=v: Buffer(v)) for k, v in plains.items()}
    altered = dict(plains)
    altered["obj11"] = altered["obj11"][:-1] + bytes([altered["obj11"][-1] ^ 1])
    bad = {k: (lambda v=v: Buffer(v)) for k, v in altered.items()}
    for kw in ({"batch": 7}, {"checkers": 4}):
        assert fs.cryptcheck(clean, **kw) == {"differ": [], "no_hash": [], "errors": {}, "ok": 20}
        res = fs.cryptcheck(bad, **kw)
        assert res == {"differ": ["obj11"], "no_hash": [], "errors": {}, "ok": 19}


def test_overlay_over_a_sha1_remote():
    _overlay_flow("sha1")


def test_overlay_over_the_md5_remote_is_unchanged():
    _overlay_flow("md5")
