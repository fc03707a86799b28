"""bench.py's plain run on the GPU: one JSON line with the headline keys and nothing of the --full sections, and
--dump-outputs writing what the last timed step returned - the same arrays a caller of the pipeline gets on the same seeded
inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_dumps_the_outputs_of_its_last_timed_step(tmp_path):
    assert torch.cuda.is_available()
    out_dir = tmp_path / "outputs"
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["unit"] == "ray-samples/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["steps"] == 3 and line["warmup"] == 1 and line["metric"].startswith("ray-samples/sec (coarse+fine)")
    assert abs(line["value"] - 16384 * 256 / (line["ms_per_step"] * 1e-3)) <= 1e-6 * line["value"]
    for key in ("train", "cpu_baseline", "other_precisions_1gpu", "operating_points_render", "netwidth_points", "psnr_db"):
        assert key not in line, key
    assert line["roofline"]["traffic"] is None and "traffic_detail" not in line["roofline"]

    names = ["rgb", "rgb_fine", "ray_samples_fine", "densities_fine"]
    shapes = {"rgb": (16384, 3), "rgb_fine": (16384, 3), "ray_samples_fine": (16384, 192, 3), "densities_fine": (16384, 192)}
    assert sorted(os.listdir(out_dir)) == sorted(n + ".npy" for n in names)
    assert sum(os.path.getsize(out_dir / (n + ".npy")) for n in names) <= 64_000_000
    got = {n: np.load(out_dir / (n + ".npy")) for n in names}
    assert all(got[n].dtype == np.float32 and got[n].shape == shapes[n] for n in names)
    assert {n: tuple(v["shape"]) for n, v in line["dumped_outputs"].items()} == shapes

    # the same pipeline on the same seeded frame in this process, through the same five-call path (under a launch profile)
    sys.path.insert(0, ROOT)
    import bench
    from smpl_nerf_amd import _lib
    dev = torch.device("cuda:0")
    pipe, _, _ = bench.build_pipeline(dev)
    data = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in bench.frame_inputs("nerf", 128, 0)]
    with torch.no_grad(), _lib.profile():
        ref = pipe(data)
    torch.cuda.synchronize()
    for n, t in zip(names, ref):
        assert np.array_equal(got[n], t.cpu().numpy()), n
    assert float(got["rgb_fine"].std()) > 0.01
