"""`python bench.py --gpus N`, typed the way the driver types its 1-GPU run: bench.py starts its N ranks itself (round-4 verdict:
that spelling used to exit before anything ran).  Here, without a GPU, every rank must come up, say which rank of how many it is
and why it cannot run, and the launcher must return a non-zero code."""
import os
import subprocess
import sys

import pytest

from oracle_lib import ROOT


@pytest.mark.parametrize("n", [2, 3])
def test_bare_gpus_n_spawns_n_ranks(n):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--steps", "1", "--warmup", "0", "--no-cpu-baseline", "--no-extras"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)
    err = p.stderr.decode()
    import torch
    if torch.cuda.is_available() and torch.cuda.device_count() >= n:
        assert p.returncode == 0, err[-2000:]
        return
    assert p.returncode != 0
    for r in range(n):
        assert "bench.py rank %d of %d:" % (r, n) in err, err[-2000:]
    if torch.cuda.is_available():
        assert "%d GPUs needed, %d visible" % (n, torch.cuda.device_count()) in err
    else:
        assert "needs a GPU" in err
    assert not p.stdout.decode().strip().startswith("{"), "no JSON line from a run that did not happen"


@pytest.mark.gpu
def test_bare_gpus_two_on_this_box():
    """On the GPU box: with one device the two ranks come up and say '2 GPUs needed, 1 visible'; with two or more the run succeeds
    (test_bench_runs_on_two_ranks_over_rccl checks its line)."""
    test_bare_gpus_n_spawns_n_ranks(2)


def test_dump_outputs_writes_the_tile_and_a_seeded_sample_of_a_large_one(tmp_path, monkeypatch):
    """--dump-outputs: the image as the caller holds it (float32) and the ray total (float64); an image above the size limit as the
    same seeded sample of pixels in every run, with their indices."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    tile = torch.arange(6 * 5 * 4, dtype=torch.float32).reshape(6, 5, 4) / 7
    bench.dump_outputs(str(tmp_path / "full"), tile, 1234)
    img = np.load(tmp_path / "full" / "image.npy")
    assert img.dtype == np.float32 and np.array_equal(img, tile.numpy())
    rays = np.load(tmp_path / "full" / "rays.npy")
    assert rays.dtype == np.float64 and rays.tolist() == [1234.0]
    assert not (tmp_path / "full" / "image_pixel_index.npy").exists()
    monkeypatch.setattr(bench, "DUMP_MAX_PIXELS", 8)
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), tile, 1234)
    idx = np.load(tmp_path / "s1" / "image_pixel_index.npy")
    assert idx.dtype == np.float64 and len(idx) == 8 and np.all(np.diff(idx) > 0)
    assert np.array_equal(np.load(tmp_path / "s1" / "image.npy"), tile.numpy().reshape(30, 4)[idx.astype(np.int64)])
    for f in ("image.npy", "image_pixel_index.npy", "rays.npy"):
        assert np.array_equal(np.load(tmp_path / "s1" / f), np.load(tmp_path / "s2" / f)), f
