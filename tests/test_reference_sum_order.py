"""snerf_reference_sum_*_f32 (include/smplnerf.h, csrc/refsum.h): torch.sum(x + add, -1) in the order of torch's CPU kernel -
the reference's normalising sum (utils.py:200-201) - bit for bit.  CPU only: the host entry, the fixture host's recorded sums,
the strict-mode probe and the argument checks of the new entries and of the SNERF_REFERENCE_SUM flag."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
from smpl_nerf_amd import _lib, ops

F32 = np.float32
BADARG = -1           # SNERF_E_BADARG
LENGTHS = list(range(0, 1101)) + [2047, 4096, 8191, 8192, 8193, 16384, 32767]


def _rows(rng, B, n, stride, kind_offset=0):
    """[B, stride] fp32 rows: random over 1e-3 .. 1e3, and (B > 1) all-zero, constant, single-spike and alternating rows."""
    x = (10.0 ** rng.uniform(-3, 3, size=(B, stride))).astype(F32)
    for b in range(B):
        kind = (b + kind_offset) % 6 if B > 1 else 0
        if kind == 1:
            x[b] = 0
        elif kind == 2:
            x[b] = F32(0.37)
        elif kind == 3:
            x[b] = 0
            x[b, rng.integers(0, max(n, 1))] = F32(812.5)
        elif kind == 4:
            x[b] = 0
            x[b, 1::2] = F32(977.3)
    return x


def _host_sum(x, B, n, add, stride):
    out = np.full(B, np.nan, F32)
    rc = _lib.load().snerf_reference_sum_host_f32(x.ctypes.data, stride, B, n, add, out.ctypes.data)
    assert rc == 0, _lib.load().snerf_last_error_string()
    return out


def _torch_sum(x, n, add):
    return torch.sum(torch.from_numpy(x)[:, :n] + add, -1).numpy()


def _bits(a):
    return np.asarray(a, F32).view(np.uint32)


def test_host_entry_equals_torch_sum_bit_for_bit():
    rng = np.random.default_rng(20261016)
    fp64_differs = 0
    for i, n in enumerate(LENGTHS):
        for B in (1, 3, 8, 37):
            stride = n + 1 + (i % 5)                     # rows strided: row_stride > n
            x = _rows(rng, B, n, stride, kind_offset=i)
            for add in (0.0, 1e-5):
                got, want = _host_sum(x, B, n, add, stride), _torch_sum(x, n, add)
                assert np.array_equal(_bits(got), _bits(want)), (n, B, add, got, want)
                xa = (x[:, :n] + F32(add)).astype(F32)
                fp64_differs += int(np.sum(xa.astype(np.float64).sum(-1).astype(F32) != want))
    # the set tells the two orders apart: the fp64 sum rounded once (the default mode's) differs from torch's in many rows
    assert fp64_differs > 100


_CHILD = r'''
import sys
sys.path.insert(0, {root!r})
import numpy as np, torch
from smpl_nerf_amd import _lib
cap = torch.backends.cpu.get_cpu_capability()
if cap != {want!r}:
    print("CAPABILITY " + cap)
    sys.exit(77)
lib = _lib.load()
rng = np.random.default_rng(7)
for n in list(range(0, 300)) + [511, 512, 513, 1022, 4096, 8193, 32767]:
    for B in (1, 37):
        x = (10.0 ** rng.uniform(-3, 3, size=(B, n + 3))).astype(np.float32)
        for add in (0.0, 1e-5):
            out = np.zeros(B, np.float32)
            assert lib.snerf_reference_sum_host_f32(x.ctypes.data, n + 3, B, n, add, out.ctypes.data) == 0
            want = torch.sum(torch.from_numpy(x)[:, :n] + add, -1).numpy()
            assert np.array_equal(out.view(np.uint32), want.view(np.uint32)), (n, B, add)
print("OK " + cap)
'''


@pytest.mark.parametrize("cap", ["default", "avx2", "avx512"])
def test_host_entry_equals_torch_sum_under_every_cpu_capability(cap):
    want = cap.upper()
    env = dict(os.environ, ATEN_CPU_CAPABILITY=cap)
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT, want=want)], env=env, capture_output=True, text=True,
                       timeout=600)
    if r.returncode == 77:
        pytest.skip(f"this CPU does not run torch's {cap} kernels ({r.stdout.strip()})")
    assert r.returncode == 0 and f"OK {want}" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_host_entry_reproduces_the_fixture_hosts_normalising_sums():
    """All 240 sums torch.sum(w[:, 1:-1] + 1e-5, -1) recorded on the fixture host (g4), read in place: x = w + 1, row_stride =
    Nc, n = Nc - 2."""
    g = load_golden("g4_sampler.npz")
    total = 0
    for wk, tk in (("w", "tot"), ("w_16_8", "tot_16_8"), ("w_32_64", "tot_32_64"), ("w_64_64", "tot_64_64"),
                   ("w_48_200", "tot_48_200")):
        w = np.ascontiguousarray(g[wk], F32)
        B, Nc = w.shape
        out = np.full(B, np.nan, F32)
        assert _lib.load().snerf_reference_sum_host_f32(w.ctypes.data + 4, Nc, B, Nc - 2, 1e-5, out.ctypes.data) == 0
        assert np.array_equal(_bits(out), _bits(g[tk].reshape(-1))), wk
        total += B
    assert total == 240


def test_device_reference_sum_ok_needs_x86_and_an_8_lane_capability(monkeypatch):
    import platform
    monkeypatch.setattr(ops, "_REFSUM_OK", None)
    assert ops.device_reference_sum_ok()
    monkeypatch.setattr(ops, "_REFSUM_OK", None)
    monkeypatch.setattr(platform, "machine", lambda: "aarch64")
    assert not ops.device_reference_sum_ok()
    monkeypatch.undo()
    monkeypatch.setattr(ops, "_REFSUM_OK", None)
    monkeypatch.setattr(torch.backends.cpu, "get_cpu_capability", lambda: "SVE256")
    assert not ops.device_reference_sum_ok()
    monkeypatch.undo()


def test_new_entries_check_their_arguments_on_the_host():
    lib = _lib.load()
    x = np.ones((2, 8), F32)
    out = np.zeros(2, F32)
    for fn, tail in ((lib.snerf_reference_sum_f32, (None,)), (lib.snerf_reference_sum_host_f32, ())):
        assert fn(None, 8, 2, 8, 0.0, out.ctypes.data, *tail) == BADARG
        assert fn(x.ctypes.data, 8, 2, 8, 0.0, None, *tail) == BADARG
        assert fn(x.ctypes.data, 8, 2, -1, 0.0, out.ctypes.data, *tail) == BADARG
        assert fn(x.ctypes.data, 8, 2, 32768, 0.0, out.ctypes.data, *tail) == BADARG
        assert fn(x.ctypes.data, 8, -1, 8, 0.0, out.ctypes.data, *tail) == BADARG
        assert fn(None, 8, 0, 8, 0.0, None, *tail) == 0                                   # B = 0: a no-op
    # the render entries strip SNERF_REFERENCE_SUM before their precision check
    R = _lib.REFERENCE_SUM
    args = lambda prec: (None, None, None, None, prec, None, None, None, None, None, None, None, 0, 64, 128, 0, None, None, None,
                         None, None, None)
    assert lib.snerf_render_rays_f32(*args(3 | R)) == 0
    assert lib.snerf_render_rays_f32(*args(1 | R)) == BADARG
    assert b"precision" in lib.snerf_last_error_string()
    # and the training entries: a bad precision is named before the (null) batch, a good one passes on to the batch check
    targs = lambda prec: (None, None, None, None, None, None, prec, None, 0, None, None, None, None, None, None, None, None)
    assert lib.snerf_nerf_train_grads_f32(*targs(1 | R)) == BADARG
    assert b"precision" in lib.snerf_last_error_string()
    assert lib.snerf_nerf_train_grads_f32(*targs(_lib.SPLIT_F16X3 | R)) == BADARG
    assert b"batch is null" in lib.snerf_last_error_string()


def test_reference_sum_flag_matches_the_header():
    text = open(os.path.join(ROOT, "include", "smplnerf.h")).read()
    m = re.search(r"#define\s+SNERF_REFERENCE_SUM\s+(0x[0-9a-fA-F]+|\d+)", text)
    assert m and int(m.group(1), 0) == _lib.REFERENCE_SUM
    assert _lib.REFERENCE_SUM & 0xff == 0          # clear of every precision code (0, 2, 3, 16)
