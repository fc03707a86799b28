"""CPU-side checks of the canonical-density loss (GaussianMixture.pdf): the torch restatement the GPU tests measure against reproduces
what the reference computed (tests/golden/g18_gmm_loss.npz), the C entry point exists and validates its arguments before touching a
device, the mirror class has the reference's surface and the drop-in rebinds utils.GaussianMixture.  No GPU needed, nothing launched."""
import importlib
import json
import sys

import numpy as np
import pytest
import torch

import gmm_ref as GR
from conftest import load_golden
from smpl_nerf_amd import _lib, build


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.load()


@pytest.fixture(scope="module")
def g18():
    g = load_golden("g18_gmm_loss.npz")
    assert json.loads(str(g["config"])) == json.loads(json.dumps(GR.G18)), "the fixture was generated with other seeds than gmm_ref.G18"
    return g


@pytest.mark.parametrize("std", GR.STDS)
@pytest.mark.parametrize("B,S,V", GR.G18_OP_SHAPES)
def test_restatement_reproduces_the_reference(g18, B, S, V, std):
    """fp32 on the CPU: the chunked restatement is the reference's own arithmetic on fewer rows at a time.  Bound against the
    recorded arrays: 4 ulp of the largest value (2^-22; another CPU's exp and reduction blocking are all that may differ -
    measured where the fixture was made: equal bit for bit, all twenty arrays).  And the recorded arrays themselves sit within
    1e-6 = 16 ulp of the float64 restatement (measured: pdf 4.5e-9 .. 1.0e-7, gradient 8.3e-8 .. 2.7e-7), which is what makes
    float64 the yardstick of the GPU tests."""
    samples, means, d = GR.op_inputs(B, S, V, std, GR.G18["op_seed"])
    y32, y64 = GR.restated(samples, means, d, std, torch.float32), GR.restated(samples, means, d, std, torch.float64)
    key = f"op/{B}_{S}_{V}_{std}"
    for name in ("pdf", "d_samples"):
        ref = g18[f"{key}/{name}"]
        assert ref.shape == y32[name].shape and np.isfinite(ref).all()
        scale = np.abs(ref).max()
        diff = np.abs(y32[name].astype(np.float64) - ref).max()
        e_ref, e32 = GR.relative_error(ref, y64[name]), GR.relative_error(y32[name], y64[name])
        print(f"{key} {name}: |fp32 restatement - reference| {diff / scale if scale else 0:.3e} of max; E reference {e_ref:.3e}, E fp32 {e32:.3e}")
        assert diff <= 2.0 ** -22 * scale
        assert e_ref <= 1e-6 and e32 <= 1e-6
    assert np.abs(g18[f"{key}/pdf"]).max() > 0
    if B * S > 1:
        assert np.abs(g18[f"{key}/d_samples"]).max() > 0
        assert g18[f"{key}/pdf"].reshape(-1)[-1] == 0            # the planted far sample underflows in the reference too


def test_pipeline_case_of_the_fixture(g18):
    """The pipeline case of the fixture is what gmm_ref describes: 1000 fp32 means, pdf [64, 192], factor / var of the parser's
    gmm_std, and a mixture term that matters (the generator's own condition)."""
    assert g18["means"].shape == (GR.G18["V"], 3) and g18["means"].dtype == np.float32
    assert g18["pdf"].shape == (64, 192) and g18["pdf"].max() > 0.1
    f, v = GR.factor_var(GR.G18["gmm_std"])
    assert tuple(g18["factor_var"]) == (f, v)
    assert g18["term"][0] >= 0.1 * g18["loss"][0]                # the generator's own condition: the term matters


def test_symbol_is_exported_and_prototyped(lib):
    name = "snerf_gmm_pdf_f32"
    assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == 8
    assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert "snerf_gmm_pdf_f32(" in open(_lib.HERE + "/../include/smplnerf.h").read()
    assert lib.snerf_version() == 109


def test_argument_validation_happens_on_the_host(lib):
    N = None
    one = 8        # any non-null "pointer": validation never dereferences

    def call(n=128, V=10, std=0.07, samples=one, means=one, pdf=one, dpdf=N):
        return lib.snerf_gmm_pdf_f32(samples, means, n, V, std, pdf, dpdf, N)

    def err():
        return lib.snerf_last_error_string()

    # n = 0: a no-op that returns 0, also with no GPU and null pointers
    assert call(n=0, samples=N, means=N, pdf=N) == 0
    assert call(n=-1) == -1 and b"n " in err()
    assert call(V=0) == -1 and b"V " in err()
    assert call(V=-3) == -1
    for bad in (0.0, -0.07, float("nan")):
        assert call(std=bad) == -1 and b"std" in err()
        assert call(n=0, std=bad) == -1                          # a bad scalar is an error whatever n is
    assert call(n=0, V=0) == -1
    assert call(V=1 << 30) == -1 and b"V " in err()              # V * 3 does not fit 32 bits
    assert call(n=0, V=1 << 30) == -1
    assert call(n=64 << 31) == -1 and b"n " in err()             # 2^31 blocks of 64 samples
    assert call(samples=N) == -1 and b"samples" in err()
    assert call(means=N) == -1 and b"means" in err()
    assert call(pdf=N) == -1 and b"pdf" in err()


def test_mirror_class(g18):
    from smpl_nerf_amd import ops
    means64 = np.random.default_rng(0).normal(size=(5, 3))       # float64, as numpy hands it out
    mix = ops.GaussianMixture(means64, GR.G18["gmm_std"], torch.device("cpu"))
    assert (mix.factor, mix.var) == tuple(g18["factor_var"])     # utils.py:84-86, the recorded numbers
    assert mix.means.dtype == torch.float32 and torch.equal(mix.means, torch.from_numpy(means64.astype(np.float32)))
    for std in GR.STDS:
        m = ops.GaussianMixture(means64.astype(np.float32), std, "cpu")
        assert (m.factor, m.var) == tuple(g18[f"op/2_7_63_{std}/factor_var"])
    with pytest.raises(ValueError, match="Dimension of samples"):
        mix.pdf(torch.zeros(2, 4, 2))
    with pytest.raises(ValueError):                              # a mixture that is not 3-dimensional is refused, not mis-read
        ops.GaussianMixture(np.zeros((5, 2)), 0.07, "cpu").pdf(torch.zeros(2, 4, 2))
    with pytest.raises(RuntimeError, match="GPU"):
        mix.pdf(torch.zeros(2, 4, 3))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.gaussian_mixture_pdf(torch.zeros(4, 3), torch.zeros(5, 3), 0.07)


def test_trainer_reads_the_switches_from_the_pipeline_args():
    """use_gmm_loss / restrict_gmm_loss: a missing one counts as 0 (the reference's parser defines no restrict_gmm_loss)."""
    from types import SimpleNamespace
    from smpl_nerf_amd.trainer import DataParallelTrainer, SmplNerfTrainer
    net = torch.nn.Linear(3, 3)
    pipe = SimpleNamespace(args=SimpleNamespace())
    tr = SmplNerfTrainer(pipe, [net], np.zeros((4, 3), np.float32), gmm_std=0.07, fused=False)
    assert isinstance(tr, DataParallelTrainer) and tuple(tr.canonical_mixture.means.shape) == (4, 3)
    assert not tr.gmm_term_on() and tr._default_batch_loss()
    pipe.args.use_gmm_loss = 1
    assert tr.gmm_term_on() and not tr._default_batch_loss() and tr._one_call_state() is None
    pipe.args.restrict_gmm_loss = 1
    assert not tr.gmm_term_on()
    # the hook of the base class is today's loss of the two colours
    base = DataParallelTrainer(pipe, [torch.nn.Linear(3, 3)], fused=False)
    rgb, fine, gt = torch.rand(4, 3), torch.rand(4, 3), torch.rand(4, 3)
    assert torch.equal(base.batch_loss((rgb, fine, None, None, None, None), [None, gt]), base.loss(rgb, fine, gt))
    assert torch.equal(tr.batch_loss((rgb, fine, None, None, None, None), [None, gt]), base.loss(rgb, fine, gt))


def test_dropin_rebinds_the_gaussian_mixture(tmp_path):
    """A stand-in checkout with the reference's layout: utils.GaussianMixture and two solvers that copy the class."""
    root = tmp_path / "checkout"
    solver = "from utils import GaussianMixture\n\n\nclass %s:\n    pass\n"
    for rel, src in {"utils.py": ("def raw2outputs(*a, **k):\n    raise NotImplementedError\n\n\n"
                                  "class GaussianMixture():\n    pass\n"),
                     "solver/smpl_nerf_solver.py": solver % "SmplNerfSolver",
                     "solver/warp_solver.py": solver % "WarpSolver"}.items():
        (root / rel).parent.mkdir(parents=True, exist_ok=True)
        (root / rel).write_text(src)
    top = ("utils", "models", "solver", "torchsearchsorted")
    from smpl_nerf_amd import dropin, ops
    assert dropin.REPLACEMENTS["utils"]["GaussianMixture"] is ops.GaussianMixture
    before = set(sys.modules)
    saved = {k: sys.modules.get(k) for k in list(sys.modules) if k.split(".")[0] in top}
    saved_path, saved_meta = list(sys.path), list(sys.meta_path)
    try:
        for k in list(saved):
            sys.modules.pop(k, None)
        dropin._installed = False
        dropin._originals.clear()
        dropin.install(str(root))
        for mod in ("solver.smpl_nerf_solver", "solver.warp_solver"):          # `from utils import GaussianMixture`
            assert importlib.import_module(mod).GaussianMixture is ops.GaussianMixture
        assert importlib.import_module("utils").GaussianMixture is ops.GaussianMixture
    finally:
        sys.meta_path[:] = saved_meta
        sys.path[:] = saved_path
        for k in [k for k in sys.modules if k.split(".")[0] in top]:
            sys.modules.pop(k, None)
        sys.modules.update({k: v for k, v in saved.items() if v is not None})
        dropin._installed = False
        for k in set(sys.modules) - before:
            if k.split(".")[0] in top:
                sys.modules.pop(k, None)
