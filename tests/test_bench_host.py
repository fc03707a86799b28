"""Host-side logic of bench.py that needs no GPU: launcher command, profiler detection, PMC CSV reduction, roofline
arithmetic of the JSON line, CPU-baseline leg on a tiny sample."""
import csv
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_profiler_detection_and_child_environment(monkeypatch):
    for k in list(os.environ):
        if bench._profiler_env_key(k):
            monkeypatch.delenv(k)
    monkeypatch.setenv("LD_PRELOAD", "")
    assert not bench.under_profiler()
    monkeypatch.setenv("ROCPROFILER_REGISTER_FORCE_LOAD", "1")
    assert bench.under_profiler()          # a --pmc child would nest inside a traced run: bench.py must skip it
    monkeypatch.delenv("ROCPROFILER_REGISTER_FORCE_LOAD")
    monkeypatch.setenv("LD_PRELOAD", "/opt/rocm/lib/librocprofiler-sdk-tool.so")
    assert bench.under_profiler()
    out, err = bench.pmc_traffic(["--steps", "1"], "mlp_fwd_kernel")
    assert out is None and ("profiler" in err or "rocprofv3 not found" in err)


def test_self_launch_command(monkeypatch):
    seen = {}

    def fake_call(cmd, env=None):
        seen["cmd"], seen["env"] = cmd, env
        return 0

    monkeypatch.setattr(subprocess, "call", fake_call)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "7"])
    assert bench.self_launch(4) == 0
    cmd = seen["cmd"]
    assert cmd[1:4] == ["-m", "torch.distributed.run", "--nnodes=1"] and "--nproc-per-node=4" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and cmd[-4:] == ["--gpus", "4", "--steps", "7"]
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_flop_count_and_modes():
    assert bench.FLOP_PER_EVAL == 1215744                      # 607 872 MAC per ray-sample
    assert set(bench.MODES) == {"fp32", "bf16x6", "f16x3", "bf16x3"} and bench.MODES["fp32"][2] == "f32"
    assert bench.PEAK_F32_MFMA_TFLOPS == 157.3 and bench.PEAK_16BIT_MFMA_TFLOPS == 2500.0


def test_committed_bench_line_is_self_consistent():
    """The r02 driver-style line under profiles/: value = units / time, frac = achieved / peak with achieved from the
    algorithmic FLOP count and the average launch duration, and the kernel-stats CSV of the profiled run agrees."""
    line = json.loads(open(os.path.join(ROOT, "profiles", "r02_bench_under_rocprof.json.log")).read().strip().splitlines()[-1])
    r = line["roofline"]
    assert line["dtype"] == "f32" and line["unit"] == "ray-samples/s" and line["vs_baseline"] is None
    assert abs(line["value"] - line["n_gpus"] * 16384 * 256 / (line["ms_per_step"] * 1e-3)) <= 1e-6 * line["value"]
    ach = r["flop_per_unit"] * r["units_per_launch"] / (r["avg_launch_ms"] * 1e-3) / 1e12
    assert r["flop_per_unit"] == 1215744 and abs(ach - r["achieved"]) <= 1e-9 * ach
    assert abs(r["frac"] - r["achieved"] / r["peak"]) <= 1e-12 and r["peak"] == 157.3
    rows = list(csv.DictReader(open(os.path.join(ROOT, "profiles", "r02_bench_kernel_stats.csv"))))
    k = [x for x in rows if x["Name"].startswith("void snerf::mlp_fwd_kernel<256, 8, false, false>")][0]
    assert int(k["Calls"]) == 2 * (line["steps"] + line["warmup"])        # frame launches only
    assert abs(float(k["AverageNs"]) * 1e-6 - r["avg_launch_ms"]) <= 0.02 * r["avg_launch_ms"]
    for prec, alt in line["other_precisions_1gpu"].items():
        ra = alt["roofline"]
        assert abs(ra["frac"] - ra["achieved"] / 2500.0) <= 1e-12
        assert abs(ra["mfma_issue_frac"] - ra["products_per_fp32_mac"] * ra["frac"]) <= 1e-12


def test_cpu_baseline_leg_runs_and_matches_the_numpy_oracle():
    from oracle import nerf_oracle as O
    from smpl_nerf_amd import synthetic as syn
    params = list(syn.make_scene_nets(101))
    data = bench.frame_inputs("nerf", 128, 0)
    info, out = bench.cpu_baseline("nerf", params, data, 32)
    assert info["kind"] == "port" and info["unit"] == "ray-samples/s" and info["value"] > 0 and info["cores"] >= 1
    assert info["calibration_vs_reference_in_build_container"]["outputs_bit_identical"] is True
    import torch
    ref = O.nerf_pipeline_forward(params[0], params[1], O.Args(u=torch.linspace(0., 1., steps=128).numpy()),
                                  O.PositionalEncoder(10, 0), O.PositionalEncoder(4, 0), [a[:32] for a in data])
    assert float(np.max(np.abs(out[1] - ref[1]))) <= 1e-4 and float(np.max(np.abs(out[0] - ref[0]))) <= 1e-5


def test_cpu_baseline_coarse_only_and_training_legs():
    """BASELINE configs[0] (coarse-only, 64 samples per ray) and the training step both have a CPU figure beside them."""
    from smpl_nerf_amd import synthetic as syn
    params = list(syn.make_scene_nets(101))
    data = bench.frame_inputs("nerf", 128, 0)
    info, out = bench.cpu_baseline("nerf", params, data, 16, run_fine=0)
    assert info["value"] > 0 and "1024 ray-samples per pass" in info["sample"]          # 16 rays x 64 samples
    assert np.array_equal(out[0], out[1]) and out[3].shape == (16, 64)                  # models/nerf_pipeline.py:43-44
    tr = bench.cpu_train_baseline("nerf", params, data, 8, info["cores"], bench.TRAIN_LR)
    assert tr["kind"] == "port" and tr["value"] > 0 and np.isfinite(tr["loss_first"]) and np.isfinite(tr["loss_last"])
    cal = tr["calibration_vs_reference_in_build_container"]
    assert cal["losses_bit_identical"] is True and 0.9 <= cal["port_over_reference_speed"] <= 1.1


def test_no_hard_coded_measurements_in_the_bench_line():
    """A number the run did not measure must not be in the JSON line."""
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert "0.894" not in src and "aggregate_rms_error_vs_float64" not in src
    assert bench.WARP_FLOP_PER_EVAL == 52736                   # the warp net's algorithmic FLOPs


def test_committed_r03_bench_lines_are_self_consistent():
    """Round 3: the driver-style line under profiles/ - value = units / time, frac = algorithmic FLOPs / HIP-event launch time
    / peak, the kernel-stats CSV of the profiled run agrees; the training fraction reproduces from the training CSV; the
    smpl_nerf line quotes the warp kernel on ALGORITHMIC FLOPs."""
    P = lambda n: os.path.join(ROOT, "profiles", n)
    line = json.loads(open(P("r03_bench_under_rocprof.json.log")).read().strip().splitlines()[-1])
    r = line["roofline"]
    assert abs(line["value"] - 16384 * 256 / (line["ms_per_step"] * 1e-3)) <= 1e-6 * line["value"]
    assert abs(r["frac"] - 1215744 * r["units_per_launch"] / (r["avg_launch_ms"] * 1e-3) / 1e12 / 157.3) <= 1e-9
    rows = list(csv.DictReader(open(P("r03_bench_kernel_stats.csv"))))
    k = [x for x in rows if x["Name"].startswith("void snerf::mlp_fwd_kernel<256, 8, false, false>")][0]
    assert int(k["Calls"]) == 2 * (line["steps"] + line["warmup"])
    assert abs(float(k["AverageNs"]) * 1e-6 - r["avg_launch_ms"]) <= 0.02 * r["avg_launch_ms"]
    # training: 3 x FLOPs x samples over the fp32 kernels' average launch times (two launches of each per step)
    t = json.loads(open(P("r03_bench_default.json.log")).read().strip().splitlines()[-1])["train"]
    rows = {x["Name"].split("(")[0]: float(x["AverageNs"]) * 1e-6 for x in csv.DictReader(open(P("r03_train_kernel_stats.csv")))}
    ms = 2 * sum(v for n, v in rows.items() if n in ("void snerf::mlp_fwd_kernel<256, 8, false, true>",
                                                      "void snerf::mlp_bwd_kernel<256, 8, false, 4, 2>", "snerf::mlp_wgrad_kernel",
                                                      "void snerf::mlp_wgrad_direct_kernel<4>", "snerf::mlp_wgrad_reduce_kernel"))
    frac = 3 * 1215744 * 4096 * 256 / (ms * 1e-3) / 1e12 / 157.3
    assert abs(frac - t["mlp_roofline_frac"]) <= 0.02 and t["mlp_roofline_frac"] >= 0.79, (frac, t["mlp_roofline_frac"])
    assert t["cpu_baseline"]["kind"] == "port" and t["cpu_baseline"]["calibration_vs_reference_in_build_container"]["losses_bit_identical"]
    assert {p["rays_per_step_per_gpu"] for p in t["operating_points"]} == {64, 800, 2048}
    s = json.loads(open(P("r03_bench_smpl_nerf.json.log")).read().strip().splitlines()[-1])
    w = s["warp_roofline"]
    assert w["flop_per_unit"] == 52736 and abs(w["frac"] - w["achieved"] / 157.3) <= 1e-12 and 0.8 <= w["frac"] <= 0.95 and w["pose_columns_folded_per_ray"]   # 0.65 before the per-ray pose fold
    assert "train" in s and s["train"]["cpu_baseline"]["value"] > 0 and s["cpu_baseline"]["value"] > 0
    c = json.loads(open(P("r03_bench_coarse_only.json.log")).read().strip().splitlines()[-1])
    assert c["config"]["ray_samples_per_ray"] == 64 and c["cpu_baseline"]["value"] > 0 and "configs[0]" in c["config"]["workload"]
    e = json.loads(open(P("r03_bench_8ranks_1gpu_gloo.json.log")).read().strip().splitlines()[-1])
    assert e["n_gpus"] == 8 and "gloo" in e["config"]["parallelism"]


def test_committed_r04_bench_lines_are_self_consistent():
    """Round 4: the driver-style line and the kernel trace agree; the training line is the one-call step within the memory
    bound VERDICT r03 #4 set (<= 2.6 MB per ray at 4096 rays) with host enqueue below 0.3 ms at the reference's batch sizes;
    the grouped dry runs carry per-rank and collective records; raygen is < 1 % of a 2048-ray step."""
    P = lambda n: os.path.join(ROOT, "profiles", n)
    J = lambda n: json.loads(open(P(n)).read().strip().splitlines()[-1])
    line = J("r04_bench_under_rocprof.json.log")
    r = line["roofline"]
    assert abs(line["value"] - 16384 * 256 / (line["ms_per_step"] * 1e-3)) <= 1e-6 * line["value"]
    assert abs(r["frac"] - 1215744 * r["units_per_launch"] / (r["avg_launch_ms"] * 1e-3) / 1e12 / 157.3) <= 1e-9 and r["frac"] >= 0.85
    rows = list(csv.DictReader(open(P("r04_bench_kernel_stats.csv"))))
    k = [x for x in rows if x["Name"].startswith("void snerf::mlp_fwd_kernel<256, 8, false, false>")][0]
    assert int(k["Calls"]) == 2 * (line["steps"] + line["warmup"])
    assert abs(float(k["AverageNs"]) * 1e-6 - r["avg_launch_ms"]) <= 0.02 * r["avg_launch_ms"]
    d = J("r04_bench_default.json.log")
    assert 0.9 <= d["roofline"]["traffic"] / d["roofline"]["algorithmic_hbm_bytes_per_launch"] <= 1.1
    t = d["train"]
    assert t["step_entry"].startswith("snerf_nerf_train_step_f32") and t["c_abi_calls_per_step"] == 1.0
    assert t["peak_allocated_bytes"] <= 2.6e6 * t["rays_per_step_per_gpu"] and t["mlp_roofline_frac"] >= 0.78
    pts = {p["rays_per_step_per_gpu"]: p for p in t["operating_points"]}
    assert pts[64]["ms_per_step"] <= 1.9 and pts[2048]["ms_per_step"] <= 15.9
    assert all(p["host_enqueue_ms_per_step"] < 0.3 for p in pts.values())
    assert any("eval_without_no_grad" in p.get("mode", "") for p in d["operating_points_render"])
    # the 64-ray trace: the step's kernels are the library's own - no pack kernel, no torch optimiser kernel per step
    names = {x["Name"].split("(")[0]: int(x["Calls"]) for x in csv.DictReader(open(P("r04_train64_kernel_stats.csv")))}
    assert names["snerf::adam_kernel"] == 102 and not any("multi_tensor_apply" in n for n in names)   # 2 warm-up + 50 timed + 50 plain-host steps
    assert names.get("snerf::mlp_pack_t_kernel", 0) <= 4 and names.get("snerf::mlp_pack_kernel", 0) <= 8     # initial packs only
    g = J("r04_bench_train_from_raygen.json.log")["train"]
    assert g["raygen_ms_per_step"] < 0.01 * g["ms_per_step"] and "1200 of the data set's frames" in g["batches"]
    e = J("r04_bench_8ranks_1gpu_gloo.json.log")
    assert [p["rank"] for p in e["per_rank"]] == list(range(8)) and e["collective"]["world_size_seen_by_backend"] == 8
    c = e["train"]["collective"]
    assert c["bytes"] == 4 * 1220872 and c["allreduce_ms_per_step"] > 0 and c["allreduce_calls"] == 3 and c["broadcast_ms"] > 0
    s = J("r04_bench_2ranks_strong_1gpu_gloo.json.log")
    assert s["scaling"] == "strong" and s["collective"]["strong_frame_max_abs_diff_vs_single_rank_render"] == 0.0
    w = J("r04_bench_world1_rccl.json.log")
    assert w["train"]["collective"]["backend"] == "nccl (RCCL)" and w["train"]["collective"]["allreduce_calls"] == 10
    co = J("r04_bench_8ranks_coarse_only_1gpu_gloo.json.log")
    assert co["config"]["ray_samples_per_ray"] == 64 and co["n_gpus"] == 8 and len(co["per_rank"]) == 8
    for wl in ("append_vertices", "append_smpl_params"):
        a = J(f"r04_bench_{wl}_input_grads.json.log")["train"]
        assert a["input_gradients"] and any(k.startswith("dy_contract") for k in a["kernels_ms_per_step"])


def test_quality_keys_of_the_bench_line():
    """The quality half of BASELINE's metric in the JSON line: PSNR by util/scores.py:47-48 of the HIP render and of the CPU
    reference path's render against the same ground truth, their difference, the PSNR between the two renders (the sampler
    key needs the GPU and is covered by the -m gpu bench test)."""
    import torch
    rng = np.random.default_rng(0)
    gt = rng.random((64, 3)).astype(np.float32)
    cpu = (gt + 0.05 * rng.standard_normal((64, 3))).astype(np.float32)
    hip = cpu + np.float32(1e-5)
    out = [torch.zeros(64, 3), torch.from_numpy(hip)]
    q = bench.quality_keys(out, [np.zeros((64, 3), np.float32), cpu], gt, 64, None, None, None)
    mse = np.mean((hip.astype(np.float64) - gt) ** 2)
    assert abs(q["psnr_db"] - (-10.0 * np.log(mse) / np.log(10.0))) < 1e-9
    assert abs(q["psnr_delta_db_vs_oracle"] - (q["psnr_db"] - q["psnr_db_cpu_reference_path"])) < 1e-12
    assert abs(q["psnr_delta_db_vs_oracle"]) < 0.01 and q["psnr_db_hip_vs_cpu_reference_render"] > 90
    assert "sampler_index_equal_frac" not in q
    same = bench.quality_keys([out[0], torch.from_numpy(cpu)], [cpu, cpu], gt, 64, None, None, None)
    assert same["psnr_db_hip_vs_cpu_reference_render"] is None and same["psnr_delta_db_vs_oracle"] == 0.0
    json.dumps(same)


def test_plain_run_options():
    """A plain run measures the headline only: --full (everything else) is off by default, --steps sets the timed steps."""
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    a = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert a.full is True and a.dump_outputs == "out"
    for bad in (["--steps", "0"], ["--warmup", "-1"]):
        with pytest.raises(SystemExit):
            bench.parse_args(bad)


def test_dump_outputs_names_dtypes_and_size_bound(tmp_path):
    """--dump-outputs: float32 .npy files named after the pipeline's return tuple; above the byte bound every array keeps the
    same seeded sample of rows, identical from run to run."""
    assert bench.output_names(4) == ["rgb", "rgb_fine", "ray_samples_fine", "densities_fine"]
    assert bench.output_names(4, run_fine=0)[2:] == ["ray_samples", "densities"] and len(bench.output_names(6)) == 6
    rng = np.random.default_rng(3)
    named = {"rgb": rng.random((1000, 3)), "samples": rng.random((1000, 40, 3)).astype(np.float32),
             "idx": np.arange(1000, dtype=np.int64)}
    w = bench.dump_outputs(str(tmp_path / "all"), named)
    assert w["samples"] == {"shape": [1000, 40, 3], "rows_of": 1000}
    got = {k: np.load(tmp_path / "all" / (k + ".npy")) for k in named}
    assert got["rgb"].dtype == np.float64 and got["samples"].dtype == np.float32 and got["idx"].dtype == np.float32
    assert np.array_equal(got["samples"], named["samples"]) and np.array_equal(got["idx"], np.arange(1000))
    limit = 200_000
    for d in ("a", "b"):
        w = bench.dump_outputs(str(tmp_path / d), named, limit=limit)
        assert sum(os.path.getsize(tmp_path / d / (k + ".npy")) for k in named) <= limit
    a = {k: np.load(tmp_path / "a" / (k + ".npy")) for k in named}
    b = {k: np.load(tmp_path / "b" / (k + ".npy")) for k in named}
    rows = a["idx"].astype(np.int64)
    assert 0 < len(rows) < 1000 and np.all(np.diff(rows) > 0) and w["idx"]["rows_of"] == 1000
    assert all(np.array_equal(a[k], b[k]) for k in named)
    assert np.array_equal(a["samples"], named["samples"][rows]) and np.array_equal(a["rgb"], named["rgb"][rows])
