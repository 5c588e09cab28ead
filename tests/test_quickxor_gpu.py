"""QuickXorHash of crypt ciphertext for wrapped remotes whose Hashes().GetOne() is "quickxor"
(OneDrive Personal, Business, SharePoint): Fs.put's ciphertext hash (crypt.go:516-533) and
cryptcheck's computeHashWithNonce / ComputeHash (crypt.go:784-852), through every layer MD5 and
SHA-1 have -- the kernel (xs_quickxor: many workgroups per object), the batched seal + hash of the
engine and the pool (nothing routed to the host), the per-object streaming paths on host cores, the
encrypter's tee, and the overlay.

Checker: the restatement of the hash's bit rule below (numpy for random data, analytic for sparse
inputs) over the oracle's crypt files (orc.encrypt_file).  It is written from the rule, not from
the C++; tests/test_quickxor_cpu.py holds it against the reference's 70 test vectors.
"""
import ctypes
import threading

import numpy as np
import pytest

from oracle import pyoracle as orc
from rclone_amd.testdata import splitmix64_bytes
from tests.go_readers import Buffer, CloseDetector, ErrorReader, MultiReader, Potato

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

XS_HASH_QUICKXOR = 0x40000000
HASH_DESC = np.dtype([("off", "<u8"), ("len", "<u8"), ("prefix", "u1", (32,)), ("prefix_len", "<u4"),
                      ("res", "<u4", (3,))])
RING = (1 << 160) - 1


def quickxor(data) -> bytes:
    """The rule, restated: stream byte i is XORed into a 160-bit ring at bit (11 i) mod 160, bits
    past 159 wrapping to bit 0; the ring is 20 little-endian bytes and the 64-bit little-endian
    length is XORed into bytes 12..19.  Bytes i and i + 160 meet the same bit, so the column-wise
    XOR of the stream in rows of 160 bytes is folded, 160 rotations."""
    a = data if isinstance(data, np.ndarray) else np.frombuffer(bytes(data), dtype=np.uint8)
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
    return (ring ^ (n << 96)).to_bytes(20, "little")


def quickxor_sparse(length, set_bytes) -> bytes:
    """The digest of `length` zero bytes with stream byte p set to v for (p, v) in set_bytes."""
    ring = 0
    for p, v in set_bytes:
        assert 0 <= p < length
        x = v << (11 * p % 160)
        ring ^= (x & RING) | (x >> 160)
    return (ring ^ (length << 96)).to_bytes(20, "little")


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _slice():
    from rclone_amd import _lib
    T = int(_lib.lib().xs_quickxor_slice())
    assert T > 0 and T % 160 == 0
    return T


def _run(desc, src):
    from rclone_amd import device
    dig, ok = device.hash_batch("quickxor", desc, src)
    torch.cuda.synchronize()
    dig, ok = dig.cpu().numpy(), ok.cpu().numpy()
    assert dig.shape == (len(desc), 20)
    return [dig[i].tobytes() for i in range(len(desc))], list(ok)


def _check_lengths(lengths, seed):
    """Every length under prefix lengths 0, 16 and 32, each at its own non-zero 16-byte aligned
    offset, in one batch (digest stride 20: every neighbour is checked too)."""
    offs, pos = {}, 48
    for n in lengths:
        offs[n] = pos
        pos += ((n + 15) & ~15) + 16 * (n % 3)
    data = np.frombuffer(splitmix64_bytes(seed, pos + 64), dtype=np.uint8)
    src = torch.from_numpy(data.copy()).cuda()
    rng = np.random.default_rng(seed)
    cases = [(n, plen) for n in lengths for plen in (0, 16, 32)]
    desc = np.zeros(len(cases), dtype=HASH_DESC)
    want = []
    for i, (n, plen) in enumerate(cases):
        pre = rng.integers(0, 256, 32, dtype=np.uint8)
        desc["off"][i], desc["len"][i], desc["prefix_len"][i] = offs[n], n, plen
        desc["prefix"][i] = pre
        want.append(quickxor(np.concatenate([pre[:plen], data[offs[n]:offs[n] + n]])))
    got, ok = _run(desc, src)
    assert ok == [1] * len(cases)
    for i, c in enumerate(cases):
        assert got[i] == want[i], c


def test_kernel_small_lengths():
    # every len mod 16 tail, the 160- and 320-byte rows, the empty stream
    assert HASH_DESC.itemsize == 64
    _check_lengths(list(range(0, 401)), 3)


def test_kernel_lengths_around_the_slice():
    T = _slice()
    lengths = [1759, 1760, 1761, 65583, 65584, 65585, T - 1, T, T + 1, 2 * T - 1, 2 * T + 1, T - 32, T - 33, 2 * T - 16,
               (8 << 20) + 13]
    _check_lengths(sorted(set(lengths)), 4)


def test_kernel_one_hot_positions():
    # a zero stream of three slices with a single 0xFF byte: the digest is 0xFF rotated to
    # 11 p mod 160, XORed with the length.  Random data can mask a lane or slice position error.
    T = _slice()
    L = 3 * T
    ps = list(range(0, 176))
    for b in (T, 2 * T, 3 * T):
        ps += [p for p in range(b - 2, b + 3) if p < L]
    cases = [(p, plen) for p in ps for plen in (0, 32)]
    src = torch.zeros(len(cases) * L, dtype=torch.uint8, device="cuda")
    idx = torch.tensor([k * L + p for k, (p, _) in enumerate(cases)], device="cuda")
    src[idx] = 0xFF
    desc = np.zeros(len(cases), dtype=HASH_DESC)
    want = []
    for k, (p, plen) in enumerate(cases):
        desc["off"][k], desc["len"][k], desc["prefix_len"][k] = k * L, L, plen  # the prefix bytes are zero
        want.append(quickxor_sparse(plen + L, [(plen + p, 0xFF)]))
    got, ok = _run(desc, src)
    assert ok == [1] * len(cases)
    for k, c in enumerate(cases):
        assert got[k] == want[k], c


def test_kernel_skewed_batch_and_long_object_alone():
    # one 64 MiB object with 2 000 objects of 1..4 096 bytes: the long one's workgroups stride
    # over its slices; then the long object alone (n = 1), every slice its own workgroup
    rng = np.random.default_rng(11)
    big = 64 << 20
    small = [int(x) for x in rng.integers(1, 4097, 2000)]
    lens = small[:1000] + [big] + small[1000:]
    offs, pos = [], 0
    for n in lens:
        offs.append(pos)
        pos += (n + 15) & ~15
    data = rng.integers(0, 256, pos, dtype=np.uint8)
    src = torch.from_numpy(data).cuda()
    desc = np.zeros(len(lens), dtype=HASH_DESC)
    desc["off"], desc["len"] = offs, lens
    want = [quickxor(data[o:o + n]) for o, n in zip(offs, lens)]
    got, ok = _run(desc, src)
    assert ok == [1] * len(lens)
    assert got == want
    got1, ok1 = _run(desc[1000:1001], src)
    assert ok1 == [1] and got1 == [want[1000]]


def test_kernel_64_bit_lengths():
    free, _ = torch.cuda.mem_get_info()
    if free < (6 << 30):
        pytest.skip(f"needs 6 GiB of free device memory for a 4 GiB + 17 object, {free >> 20} MiB are free")
    n = (4 << 30) + 17
    off = 32
    src = torch.zeros(off + n + 15, dtype=torch.uint8, device="cuda")
    # the object ends 17 bytes past 2^32: three of the set bytes lie past offset 2^32, one in the tail
    sets = [(0, 0x01), (5, 0x80), ((1 << 31) + 3, 0x5A), ((1 << 32) - 7, 0x7E), ((1 << 32) + 1, 0xC3), ((1 << 32) + 9, 0xFF),
            (n - 1, 0x81)]
    for p, v in sets:
        src[off + p] = v
    desc = np.zeros(1, dtype=HASH_DESC)
    desc["off"], desc["len"] = off, n
    got, ok = _run(desc, src)
    assert ok == [1] and got == [quickxor_sparse(n, sets)]
    del src


def test_kernel_invalid_descriptors():
    T = _slice()
    data = np.frombuffer(splitmix64_bytes(21, 3 * T + 64), dtype=np.uint8)
    src = torch.from_numpy(data.copy()).cuda()
    # (off, len, prefix_len, valid): misaligned offset, past the end, prefix length 8, among valid ones
    rows = [(0, 100, 0, True), (8, 10, 0, False), (16, 2 * T + 5, 32, True), (len(data) - 16, 32, 0, False),
            (32, 0, 16, True), (0, 10, 8, False), (len(data) + 16, 0, 0, False), (48, T, 0, True), (0, len(data) + 1, 0, False),
            (len(data), 0, 0, True)]
    desc = np.zeros(len(rows), dtype=HASH_DESC)
    pre = np.arange(32, dtype=np.uint8)
    want = []
    for i, (o, n, plen, valid) in enumerate(rows):
        desc["off"][i], desc["len"][i], desc["prefix_len"][i] = o, n, plen
        desc["prefix"][i] = pre
        want.append(quickxor(np.concatenate([pre[:plen], data[o:o + n]])) if valid else bytes(20))
    got, ok = _run(desc, src)
    assert ok == [int(r[3]) for r in rows]
    assert got == want


def _carry_nonce(i):
    return b"\xfd" + b"\xff" * 7 + splitmix64_bytes(i, 16)  # + block index carries across byte 8


SIZES = [0, 1, 15, 16, 65535, 65536, 65537, 2 * 65536, 300000, 5 * 65536 + 3, 1 << 20]


def test_hash_batch_with_nonce_quickxor_vs_oracle():
    from rclone_amd import crypt
    c = crypt.Cipher("", "")
    key = bytes(32)
    items, expect = [], []
    for i, n in enumerate(SIZES):
        plain = splitmix64_bytes(100 + i, n)
        nonce = _carry_nonce(i) if i % 4 == 0 else splitmix64_bytes(200 + i, 24)
        items.append((nonce, Buffer(plain)))
        expect.append(quickxor(orc.encrypt_file(plain, nonce, key)))
    assert c.hash_batch_with_nonce(items, "quickxor") == expect


def _stage(sizes, plains):
    offs, pos = [], 0
    for n in sizes:
        offs.append(pos)
        pos += (n + 15) & ~15
    stage = bytearray(pos + 16)
    for o, p in zip(offs, plains):
        stage[o:o + len(p)] = p
    return stage, offs


def test_put_batch_hash_quickxor_bodies_and_digests_vs_oracle():
    from rclone_amd import _lib
    L = _lib.lib()
    key = splitmix64_bytes(77, 32)
    sizes = SIZES
    plains = [splitmix64_bytes(300 + i, n) for i, n in enumerate(sizes)]
    nonces = b"".join(splitmix64_bytes(400 + i, 24) if i % 5 else b"\xff" * 8 + splitmix64_bytes(i, 16)
                      for i in range(len(sizes)))
    stage, offs = _stage(sizes, plains)
    n = len(sizes)
    u64s = ctypes.c_uint64 * n
    lens_c, offs_c = u64s(*sizes), u64s(*offs)
    total = L.xs_put_body_bytes(n, lens_c)
    body = (ctypes.c_uint8 * (total + 16))()
    dig_put = (ctypes.c_uint8 * (20 * n))()
    dig_seal = (ctypes.c_uint8 * (20 * n))()
    dig_pool = (ctypes.c_uint8 * (20 * n))()
    src = (ctypes.c_uint8 * len(stage)).from_buffer(stage)
    e = L.xs_engine_create(0, 64, 1)
    assert e
    try:
        assert L.xs_engine_put_batch_hash(e, XS_HASH_QUICKXOR, key, n, nonces, offs_c, lens_c, src, body, dig_put) == 0, \
            _lib.last_error()
        assert L.xs_engine_seal_hash(e, XS_HASH_QUICKXOR, key, n, nonces, offs_c, lens_c, src, dig_seal) == 0, \
            _lib.last_error()
    finally:
        L.xs_engine_destroy(e)
    p = L.xs_pool_create((ctypes.c_int * 2)(0, 0), 2, 64, 1)
    assert p
    try:
        assert L.xs_pool_seal_hash(p, XS_HASH_QUICKXOR, key, n, nonces, offs_c, lens_c, src, dig_pool) == 0, \
            _lib.last_error()
    finally:
        L.xs_pool_destroy(p)
    raw, dig = bytes(body), bytes(dig_put)
    bpos = 0
    for i, pl in enumerate(plains):
        want = orc.encrypt_file(pl, nonces[24 * i:24 * i + 24], key)
        blen = len(want) - 32
        assert raw[bpos:bpos + blen] == want[32:], (i, sizes[i])
        assert dig[20 * i:20 * i + 20] == quickxor(want), (i, sizes[i])
        bpos += (blen + 15) & ~15
    assert bytes(dig_seal) == dig
    assert bytes(dig_pool) == dig


def test_long_object_stays_on_the_gpu():
    # one 40 MiB object among 200 small ones (the engine launches the two parts apart): exact
    # digests, and nothing is routed to host cores although host threads are allowed
    from rclone_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(5)
    sizes = [int(x) for x in rng.integers(1, 131072, 200)]
    sizes[77] = 40 << 20
    sizes[17] = 0
    offs, pos = [], 0
    for n in sizes:
        offs.append(pos)
        pos += (n + 15) & ~15
    stage = rng.integers(0, 256, pos + 16, dtype=np.uint8)
    nonces = rng.integers(0, 256, 24 * len(sizes), dtype=np.uint8).tobytes()
    key = splitmix64_bytes(12, 32)
    want = b"".join(quickxor(orc.encrypt_file(stage[o:o + n].tobytes(), nonces[24 * i:24 * i + 24], key))
                    for i, (o, n) in enumerate(zip(offs, sizes)))
    n = len(sizes)
    u64s = ctypes.c_uint64 * n
    lens_c, offs_c = u64s(*sizes), u64s(*offs)
    src = ctypes.c_void_p(stage.ctypes.data)
    st0, st1 = ((ctypes.c_uint64 * 3)() for _ in range(2))
    out = (ctypes.c_uint8 * (20 * n))()
    e = L.xs_engine_create(0, 256, 1)
    assert e
    try:
        L.xs_engine_set_host_md5(e, 2)
        L.xs_engine_md5_stats(e, st0)
        assert L.xs_engine_seal_hash(e, XS_HASH_QUICKXOR, key, n, nonces, offs_c, lens_c, src, out) == 0, _lib.last_error()
        L.xs_engine_md5_stats(e, st1)
    finally:
        L.xs_engine_destroy(e)
    assert bytes(out) == want
    assert st1[0] == st0[0] and st1[1] == st0[1] and st1[2] - st0[2] == n, (list(st0), list(st1))


def test_compute_hash_with_nonce_quickxor_per_object():
    from rclone_amd import crypt
    c = crypt.Cipher("potato", "")
    c.batch_blocks = 4
    key = c.data_key
    cases = []
    for i, n in enumerate((0, 1, 65536, 3 * 65536 + 7, 9 * 65536 + 5)):  # the last crosses seal batches
        plain = splitmix64_bytes(500 + i, n)
        nonce = splitmix64_bytes(600 + i, 24) if i != 3 else _carry_nonce(i)
        cases.append((plain, nonce, quickxor(orc.encrypt_file(plain, nonce, key)).hex()))
    for plain, nonce, want in cases:
        cd = CloseDetector(Buffer(plain))
        assert c.compute_hash_with_nonce(nonce, cd, "quickxor") == want, len(plain)
        assert cd.closed == 1
    got, errors = {}, []

    def checker(t):
        try:
            for k, (plain, nonce, _) in enumerate(cases):
                got[(t, k)] = c.compute_hash_with_nonce(nonce, Buffer(plain), "quickxor")
        except BaseException as exc:  # noqa: BLE001 -- reported by the assertion below
            errors.append(exc)

    th = [threading.Thread(target=checker, args=(t,)) for t in range(8)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
    assert got == {(t, k): cases[k][2] for t in range(8) for k in range(len(cases))}
    plain, nonce, want = cases[3]
    ct = orc.encrypt_file(plain, nonce, key)
    assert c.compute_hash(Buffer(ct), Buffer(plain), "quickxor") == want


def test_hash_errors_pass_through_quickxor():
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

    got = c.hash_batch_with_nonce(items(), "quickxor")
    want = quickxor(orc.encrypt_file(good, n0, key))
    assert got[0] == want and got[5] == want
    assert got[1] is potato and got[2] is potato and got[4] is potato
    assert isinstance(got[3], crypt.ErrUnexpectedEOF)
    cd = CloseDetector(Buffer(good))
    assert c.hash_batch_with_nonce([(n0, cd)], "quickxor")[0] == want and cd.closed == 1
    for k, (_, src) in enumerate(items()):
        if k in (0, 5):
            assert c.compute_hash_with_nonce(n0, src, "quickxor") == want.hex()
        elif k == 3:
            with pytest.raises(crypt.ErrUnexpectedEOF):
                c.compute_hash_with_nonce(n0, src, "quickxor")
        else:
            with pytest.raises(Potato):
                c.compute_hash_with_nonce(n0, src, "quickxor")


def test_encrypter_tee_quickxor_after_every_read():
    from rclone_amd import crypt
    c = crypt.Cipher("potato", "")
    plain = splitmix64_bytes(77, 3 * 65536 + 99)
    nonce = splitmix64_bytes(78, 24)
    ct = orc.encrypt_file(plain, nonce, c.data_key)
    e = c.encrypt_data(Buffer(plain), nonce)
    e.set_hash("sha1")
    e.set_hash("quickxor")  # one type per encrypter: the second call replaces the first
    assert e.hash() == quickxor(b"") == bytes(20)
    got = b""
    for want_n in (1, 31, 32, 33, 159, 160, 161, 65551, 65552, 100000):
        data, err = e.read_go(want_n)
        assert err is None
        got += data
        assert got == ct[:len(got)]
        assert e.hash() == quickxor(got), (want_n, len(got))
        assert e.hash() == quickxor(got)  # reading the digest does not disturb the state
        with pytest.raises(crypt.CryptError):
            e.md5()  # a 20-byte digest: no MD5
    with pytest.raises(crypt.CryptError):
        e.set_hash("quickxor")  # before the first read only
    while True:
        data, err = e.read_go(1 << 20)
        got += data
        if err is not None:
            assert err is crypt.EOF
            break
    assert got == ct and e.hash() == quickxor(ct)
    off = c.encrypt_data(Buffer(plain), nonce)
    off.set_hash("quickxor")
    off.set_hash(None)
    with pytest.raises(crypt.CryptError):
        off.hash()


def test_overlay_over_a_quickxor_remote():
    from rclone_amd import crypt
    from rclone_amd.cryptfs import CryptFs, MemoryRemote

    class Flipping(MemoryRemote):
        """Stores one byte wrong (a transfer that corrupts the object)."""

        def put(self, remote, reader, size=-1):
            super().put(remote, reader, size)
            b = bytearray(self.objects[remote])
            b[len(b) // 2] ^= 0x10
            self.objects[remote] = bytes(b)

    c = crypt.Cipher("potato", "")
    mem = MemoryRemote(hash_type="quickxor")
    assert mem.hashes == ("quickxor",)
    sizes = [0, 1, 15, 16, 100, 4095, 4096, 65535, 65536, 65537, 2 * 65536, 3 * 65536 + 7, 70000, 200000, 23, 24, 55, 56,
             1000, 5 * 65536 + 3]
    plains = {f"obj{i:02d}": splitmix64_bytes(900 + i, n) for i, n in enumerate(sizes)}
    for tee_by_encrypter in (True, False):  # QuickXorHash is taken by the encrypter either way
        fs = CryptFs(mem, c, encrypter_md5=tee_by_encrypter)
        assert fs.hash_type() == "quickxor"
        for name, p in plains.items():
            nonce = fs.put(name, Buffer(p), len(p))  # the put check is on: tee hash vs the remote's
            ct = orc.encrypt_file(p, nonce, c.data_key)
            assert mem.objects[name + ".bin"] == ct
            assert mem.hash(name + ".bin") == quickxor(ct).hex()
            assert fs.compute_hash(name, Buffer(p)) == quickxor(ct).hex()
            d = fs.open(name)
            assert d.read() == p
            d.close()
    bad_mem = Flipping(hash_type="quickxor")
    bad_fs = CryptFs(bad_mem, c)
    with pytest.raises(crypt.CryptError, match="corrupted on transfer: quickxor encrypted hashes differ"):
        bad_fs.put("x", Buffer(plains["obj13"]), len(plains["obj13"]))
    assert "x.bin" not in bad_mem.objects
    clean = {k: (lambda v=v: Buffer(v)) for k, v in plains.items()}
    altered = dict(plains)
    altered["obj11"] = altered["obj11"][:-1] + bytes([altered["obj11"][-1] ^ 1])
    bad = {k: (lambda v=v: Buffer(v)) for k, v in altered.items()}
    for kw in ({"batch": 7}, {"checkers": 4}):
        assert fs.cryptcheck(clean, **kw) == {"differ": [], "no_hash": [], "errors": {}, "ok": 20}
        assert fs.cryptcheck(bad, **kw) == {"differ": ["obj11"], "no_hash": [], "errors": {}, "ok": 19}
    # a remote offering SHA-1 as well: GetOne() is the lowest registered type, SHA-1
    import hashlib
    both = MemoryRemote(hash_type="sha1")
    both.hashes = ("sha1", "quickxor")
    fs2 = CryptFs(both, c)
    assert fs2.hash_type() == "sha1"
    p = plains["obj12"]
    nonce = fs2.put("y", Buffer(p), len(p))
    assert both.hash("y.bin") == hashlib.sha1(orc.encrypt_file(p, nonce, c.data_key)).hexdigest()
    assert fs2.cryptcheck({"y": lambda: Buffer(p)}) == {"differ": [], "no_hash": [], "errors": {}, "ok": 1}
