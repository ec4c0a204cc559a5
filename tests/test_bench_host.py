"""CPU: bench.py's host-side pieces -- the C1 input generator (rand 0.10
StdRng, pinned to the oracle's restatement, itself pinned to the reference
snapshots) and the --gpus / WORLD_SIZE contract."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stdrng_numpy_matches_oracle(oracle_mod):
    sys.path.insert(0, ROOT)
    from bench import stdrng_numpy
    for seed, n in [(23, 4096 + 13), (0x256, 1 << 16), (1000, 777)]:
        assert np.array_equal(stdrng_numpy(seed, n), oracle_mod.stdrng_bytes(seed, n)), seed


def test_ref_slide_bytes():
    sys.path.insert(0, ROOT)
    from bench import ref_slide_bytes
    mn = 512 << 10
    # chunks: min exactly (63 prefill bytes, 0 slides), min + 100, and a short tail
    cuts = [np.array([mn, 2 * mn + 100, 2 * mn + 150], np.uint64)]
    assert ref_slide_bytes(cuts, mn) == 63 + (63 + 100)


def test_dump_outputs(tmp_path, monkeypatch):
    """--dump-outputs: float64 counts and concatenated cuts, exact; above the
    byte cap the same seeded sample of the cuts on every call."""
    sys.path.insert(0, ROOT)
    import bench
    cuts = [np.array([5, (1 << 40) + 1], np.uint64), np.zeros(0, np.uint64),
            np.array([7], np.uint64)]
    bench.dump_outputs(str(tmp_path / "a"), cuts)
    n = np.load(tmp_path / "a" / "cut_counts.npy")
    c = np.load(tmp_path / "a" / "cuts.npy")
    assert n.dtype == np.float64 and c.dtype == np.float64
    assert n.tolist() == [2, 0, 1] and c.tolist() == [5, (1 << 40) + 1, 7]
    bench.dump_outputs(str(tmp_path / "r"), cuts, rank=1, world=2)
    assert sorted(os.listdir(tmp_path / "r")) == ["cut_counts_rank1.npy", "cuts_rank1.npy"]
    monkeypatch.setattr(bench, "DUMP_CAP_BYTES", 4096 + 3 * 8 + 50 * 8)
    big = [np.arange(1000, dtype=np.uint64)] * 3
    bench.dump_outputs(str(tmp_path / "b"), big)
    bench.dump_outputs(str(tmp_path / "c"), big)
    s = np.load(tmp_path / "b" / "cuts.npy")
    assert s.size == 50 and np.array_equal(s, np.load(tmp_path / "c" / "cuts.npy"))
    assert np.all(np.isin(s, np.arange(1000)))


def test_plain_run_switches_off_the_full_legs(monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    a = bench.parse()
    assert a.steps == 3 and not a.full and a.dump_outputs is None
    assert a.no_parity and a.no_cpu_baseline and a.no_h2h
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--no-h2h", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d"
    assert not a.no_parity and not a.no_cpu_baseline and a.no_h2h


def test_gpus_must_match_world_size():
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4"],
                       env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "WORLD_SIZE" in r.stderr
