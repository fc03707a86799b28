"""The fp32 throughput forward kernels against bits recorded with the library of the commit before kblock()'s A-operand prefetch
was re-placed (tests/golden/g23_mlp_fwd_bits.npz, maker: tests/golden/make_golden_mlp_fwd_bits.py).  Moving LDS reads between
MFMAs changes no accumulator's MFMA order, so every output must be what it was, bit for bit: the regular stream (net in train()
mode, no grad), the composed inference stream (eval()) and the default net with 69 per-ray additional inputs through the fold kernel,
each at n_cu * 128 samples (one tile per workgroup, the weight stream does not wrap) and at (2 * n_cu + 1) * 128 - 37 (every
workgroup wraps the stream, one takes a third tile, the last tile is ragged).  The outputs come from ONE child process with
SNERF_LAT=0: the throughput kernel computes every row, not the latency-class kernels or the hybrid of both."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("make_golden_mlp_fwd_bits", os.path.join(GOLDEN, "make_golden_mlp_fwd_bits.py"))
maker = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(maker)

KINDS = ("regular", "composed", "fold")


@pytest.fixture(scope="module")
def golden():
    return load_golden("g23_mlp_fwd_bits.npz")


@pytest.fixture(scope="module")
def outputs(tmp_path_factory):
    return maker.run_child(str(tmp_path_factory.mktemp("bits") / "out.npz"))


def test_fixture_was_recorded_for_this_device(golden, outputs):
    assert int(outputs["n_cu"]) == int(golden["n_cu"]), "the sample counts of the fixture follow the CU count it was recorded on"
    names = {f"{k}_{n}" for k in KINDS for n in maker.sizes(int(golden["n_cu"]))}
    assert names == {k for k in outputs if k != "n_cu"} == {k[:-len(".sha256")] for k in golden if k.endswith(".sha256")}


@pytest.mark.parametrize("which", [0, 1], ids=["one_tile_per_workgroup", "wrapped_ragged"])
@pytest.mark.parametrize("kind", KINDS)
def test_throughput_forward_reproduces_the_recorded_bits(golden, outputs, kind, which):
    n = maker.sizes(int(golden["n_cu"]))[which]
    name = f"{kind}_{n}"
    a = outputs[name]
    assert a.shape == (n, 4) and a.dtype == np.float32 and np.isfinite(a).all()
    ids, want = golden[name + ".rows"], golden[name + ".values"]
    np.testing.assert_array_equal(ids, maker.row_ids(name, n))
    got = a[ids]
    same = got.view(np.uint32) == want.view(np.uint32)
    assert same.all(), (name, "rows that differ:", ids[~same.all(axis=1)][:8], "max|delta|", float(np.abs(got - want).max()))
    assert maker.sha(a) == str(golden[name + ".sha256"]), (name, "the 64 recorded rows agree, other rows do not")
