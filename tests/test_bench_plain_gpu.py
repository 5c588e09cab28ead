"""A plain bench.py run (no --full) and --dump-outputs: the line keeps its headline keys and runs
none of the extra legs, --steps is the number of timed steps, and the dumped arrays are the
last step's outputs -- checked byte for byte against the CPU oracle's seal of the seeded inputs."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NB = 300  # more than DUMP_BLOCKS (so the whole blocks are a sample) and more than one block per CU


def _bench_mod():
    spec = importlib.util.spec_from_file_location("bench_plain", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_sample_is_fixed_and_bounded():
    bench = _bench_mod()
    for nb in (1, bench.DUMP_BLOCKS, NB, 100_000, bench.DUMP_TAG_ROWS + 1, 1_000_000):
        blocks, rows = bench.dump_sample(nb)
        again = bench.dump_sample(nb)
        assert np.array_equal(blocks, again[0]) and np.array_equal(rows, again[1])
        assert len(blocks) == len(set(blocks.tolist())) <= bench.DUMP_BLOCKS and len(rows) <= bench.DUMP_TAG_ROWS
        assert blocks[0] == 0 and blocks[-1] == nb - 1 and 0 <= rows.min() and rows.max() < nb
        assert np.all(np.diff(blocks) > 0) and np.all(np.diff(rows) > 0)
        # float32, one byte per element: wire + opened blocks, 16 tag bytes + 1 verdict per row
        total = 4 * (len(blocks) * (bench.BLOCK_SIZE + bench.BLOCK_DATA) + len(rows) * 17)
        assert total <= 64_000_000, (nb, total)
    assert len(bench.dump_sample(100_000)[1]) == 100_000  # the headline set: every block's tag


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(tmp_path):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from oracle import pyoracle as orc
    from rclone_amd import shard
    from rclone_amd.testdata import splitmix64_block
    bench = _bench_mod()
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--warmup-seconds", "0", "--blocks", str(NB), "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    res = json.loads(lines[0])
    assert res["metric"] == bench.METRIC and res["unit"] == "GiB/s" and res["higher_is_better"] is True
    assert res["dtype"] == "u32" and res["value"] > 0 and res["ms_per_step"] > 0
    # --steps timed steps, each one seal + one open of every block
    assert res["steps"] == 3 and res["counters"]["blocks"] == 3 * 2 * NB and res["counters"]["tag_failures"] == 0
    # value and ms_per_step are the same measurement (ms_per_step is rounded to 1 us, value to 0.001)
    gib, ms = 2 * NB * bench.BLOCK_DATA / 2**30, res["ms_per_step"]
    assert gib / ((ms + 0.00051) * 1e-3) - 0.001 <= res["value"] <= gib / ((ms - 0.00051) * 1e-3) + 0.001
    # none of the --full legs ran
    assert res["objectset"] is None and res["cpu_baseline"] is None and "pool_check" not in res
    assert res["counters"]["tag_digest"] is None and res["counters"]["tag_digest_ok"] is None

    blocks, rows = bench.dump_sample(NB)
    arrays = {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}
    assert sorted(arrays) == ["opened_blocks", "tag_ok", "wire_blocks", "wire_tags"]
    assert all(a.dtype == np.float32 for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64_000_000
    assert arrays["wire_blocks"].shape == (len(blocks), bench.BLOCK_SIZE)
    assert arrays["opened_blocks"].shape == (len(blocks), bench.BLOCK_DATA)
    assert arrays["wire_tags"].shape == (NB, 16) and arrays["tag_ok"].shape == (NB,)
    assert np.all(arrays["tag_ok"] == 1)
    nonces = shard.nonce_plus(bench.HEADLINE_NONCE0, blocks)
    for j, g in enumerate(blocks.tolist()):
        plain = splitmix64_block(bench.HEADLINE_SEED, g)
        assert arrays["opened_blocks"][j].astype(np.uint8).tobytes() == plain, g
        wire = arrays["wire_blocks"][j].astype(np.uint8).tobytes()
        assert wire == orc.seal(plain, bytes(nonces[j]), bench.HEADLINE_KEY), g
        assert arrays["wire_tags"][g].astype(np.uint8).tobytes() == wire[:16], g
