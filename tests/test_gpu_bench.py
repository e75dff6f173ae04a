"""GPU: a plain bench.py run (no --full) times exactly --steps steps, prints the headline line only, and --dump-outputs writes what
the timed path computed in its last step - the same arrays on every run with the same arguments, equal to the oracle's."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ARGS = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--batches-per-step", "4", "--batch", "16"]
NAMES = ("counts", "match_counts", "sample", "keypoints", "descriptors", "matches")


def _bench(out_dir):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + ARGS + ["--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), {n: np.load(os.path.join(str(out_dir), n + ".npy")) for n in NAMES}


@pytest.mark.gpu
def test_plain_run_and_dumped_outputs(tmp_path, oracle):
    import bench
    j, a = _bench(tmp_path / "a")
    assert j["steps"] == 3 and j["warmup"] == 1 and j["ms_per_step"] > 0 and j["value"] > 0
    assert j["unit"] == "frames/s" and j["higher_is_better"] is True and j["dtype"] == "u8" and j["metric"].startswith("frames/sec")
    assert abs(j["value"] - 16 * 4 / (j["ms_per_step"] * 1e-3)) < 1e-6 * j["value"]
    for k in ("roofline", "kernels", "one_stream", "localba", "cpu_baseline", "pcie_inclusive", "oracle_check"):
        assert k not in j, k                                               # the secondary figures run under --full only
    assert sorted(os.listdir(tmp_path / "a")) == sorted(n + ".npy" for n in NAMES)
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert a["counts"].shape == (2, 16) and (a["counts"] > 0).all() and (a["match_counts"] > 0).all()
    assert a["sample"].shape == (16 * 2, 3) and set(a["sample"][:, 0]) == {2.0, 3.0}       # the last step's batches 2 and 3
    assert len(a["keypoints"]) == len(a["descriptors"]) == len(a["matches"]) == a["sample"][:, 2].sum()

    # the same arguments: the same inputs and the same arrays
    _, b = _bench(tmp_path / "b")
    for n in NAMES:
        assert np.array_equal(a[n], b[n]), n

    # two sampled frames against the oracle: the frames the bench built (base batch m % 2 cropped at (2v, 3v), v = m // 2)
    base = [bench.make_frames(16, seed=s, pad_w=3, pad_h=2) for s in range(2)]
    E = oracle.OracleExtractor(bench.NFEAT)
    off = 0
    for m, f, n in a["sample"].astype(int)[:2]:
        v = m // 2
        img = np.ascontiguousarray(base[m % 2][f, 2 * v:2 * v + bench.H_IMG, 3 * v:3 * v + bench.W_IMG])
        ok, od = E.extract(img)
        assert n == len(ok) == a["counts"][m - 2, f]
        want = np.stack([ok[k].astype(np.float64) for k in ("x", "y", "size", "angle", "response", "octave", "class_id")], axis=1)
        assert np.array_equal(a["keypoints"][off:off + n], want)
        assert np.array_equal(a["descriptors"][off:off + n], od.astype(np.float32))
        off += n
