"""Maker of tests/golden/g23_mlp_fwd_bits.npz: the bits of the fp32 throughput forward kernels (csrc/mlp.hip:
mlp_fwd_kernel<256, 8, false, false> on the regular and on the composed stream, mlp_fwd_fold_kernel<256, 8>), recorded once with the
library of the commit BEFORE the A-operand prefetch of kblock() was re-placed.  A change of the instruction schedule that keeps
the MFMA order per accumulator must reproduce them bit for bit (tests/test_gpu_mfma_stream_bits.py).

    python tests/golden/make_golden_mlp_fwd_bits.py            (on the GPU, from the repository root)

Per case the fixture holds the SHA-256 of the output's bytes and 64 seeded rows (index + values) for a readable failure message.
The outputs are computed in a child process with SNERF_LAT=0, so that the throughput kernel - not the latency-class kernels
or the hybrid of both - computes every row."""
import hashlib
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "g23_mlp_fwd_bits.npz")
F32 = np.float32
ROWS = 64


def sizes(n_cu):
    """One 128-sample tile per workgroup (no wrap of the weight stream); every workgroup wraps the stream, one takes a third tile
    and the last tile is ragged."""
    return [n_cu * 128, (2 * n_cu + 1) * 128 - 37]


def samples_per_ray(n):
    """Smallest ray length of at least 8 samples that divides n (the per-ray fold needs 8 and whole rays)."""
    return next(s for s in range(8, 4096) if n % s == 0)


def compute(path):
    """Child process: {case: raw [n, 4]} of every case as an .npz at `path`."""
    import torch
    sys.path.insert(0, ROOT)
    from smpl_nerf_amd import _lib, synthetic as syn
    from smpl_nerf_amd.nets import RenderRayNet
    from smpl_nerf_amd.ops import PositionalEncoder
    assert os.environ.get("SNERF_LAT") == "0"
    dev = torch.device("cuda:0")
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    pe, de = PositionalEncoder(10, 0), PositionalEncoder(4, 0)

    def net_of(params, add_dim=0):
        m = RenderRayNet(8, 256, 60, 24, add_dim, skips=[4])
        m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
        return m.to(dev)

    plain = net_of(syn.make_scene_nets(101)[0])
    posed = net_of(syn.make_scene_net_params(301, add_first=True, additional_input_dim=69), 69)
    out = {"n_cu": np.int64(n_cu)}
    lib = _lib.load()
    for n in sizes(n_cu):
        spr = samples_per_ray(n)
        rng = np.random.default_rng(n)
        x = torch.from_numpy(rng.uniform(-2, 2, (n, 3)).astype(F32)).to(dev)
        d = torch.from_numpy(rng.normal(size=(n // spr, 3)).astype(F32)).to(dev)
        add = torch.from_numpy(rng.uniform(-1, 1, (n // spr, 69)).astype(F32)).to(dev)
        with torch.no_grad():
            out[f"regular_{n}"] = plain.train().forward_fused(x, d, spr, pe, de).cpu().numpy()
            out[f"composed_{n}"] = plain.eval().forward_fused(x, d, spr, pe, de).cpu().numpy()
            desc = posed.desc_for_encoders(pe, de, True)
            assert int(lib.snerf_mlp_fold_workspace_bytes(desc, n, spr)) > 0, "the per-ray fold must apply"
            out[f"fold_{n}"] = posed.eval().forward_fused(x, d, spr, pe, de, additional=add, add_first=True).cpu().numpy()
    np.savez(path, **out)


def run_child(path):
    subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path], check=True, env=dict(os.environ, SNERF_LAT="0"))
    return dict(np.load(path))


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=F32).tobytes()).hexdigest()


def row_ids(name, n):
    return np.sort(np.random.default_rng(sum(name.encode())).choice(n, ROWS, replace=False))


def digest(outputs):
    fx = {"n_cu": outputs["n_cu"]}
    for name, a in outputs.items():
        if name == "n_cu":
            continue
        assert a.dtype == F32 and a.ndim == 2 and a.shape[1] == 4 and np.isfinite(a).all(), name
        ids = row_ids(name, a.shape[0])
        fx[name + ".sha256"] = np.array(sha(a))
        fx[name + ".rows"] = ids
        fx[name + ".values"] = a[ids]
    return fx


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        compute(sys.argv[2])
    else:
        import tempfile
        with tempfile.TemporaryDirectory() as tmp:
            fx = digest(run_child(os.path.join(tmp, "out.npz")))
        np.savez(FIXTURE, **fx)
        print("wrote", FIXTURE, sorted(k for k in fx if k.endswith(".sha256")))
