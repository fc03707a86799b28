"""smpl_nerf_amd.dropin against a stand-in checkout written per test: the reference's module layout (namespace packages
models/ and solver/ beside utils.py) with the import forms the drop-in has to follow - `from torchsearchsorted import
searchsorted` in utils.py (utils.py:14), `from utils import ...` and `from models.x import Y` copies in models/*.py and
solver/*.py.  Wiring only - no compute: after install() those modules hold the HIP-backed classes and operators."""
import importlib
import importlib.util
import os
import sys

import pytest

# stand-in modules: path -> source (the reference's names and import forms, no behaviour)
STAND_IN = {
    "utils.py": (
        "from torchsearchsorted import searchsorted\n\n\n"
        "class PositionalEncoder():\n"
        "    def __init__(self, number_frequencies, include_identity):\n"
        "        self.number_frequencies = number_frequencies\n"
        "        self.include_identity = include_identity\n\n\n"
        "def raw2outputs(*args, **kw):\n    raise NotImplementedError\n\n\n"
        "def sample_pdf(*args, **kw):\n    raise NotImplementedError\n\n\n"
        "def fine_sampling(*args, **kw):\n    raise NotImplementedError\n"),
    "models/render_ray_net.py": "class RenderRayNet:\n    pass\n",
    "models/warp_field_net.py": "class WarpFieldNet:\n    pass\n",
    "models/nerf_pipeline.py": ("from utils import raw2outputs, fine_sampling, PositionalEncoder\n\n\n"
                                "class NerfPipeline:\n    pass\n"),
    "models/smpl_nerf_pipeline.py": ("from models.nerf_pipeline import NerfPipeline\n\n\n"
                                     "class SmplNerfPipeline(NerfPipeline):\n    pass\n"),
    "models/append_smpl_params_pipeline.py": ("from models.nerf_pipeline import NerfPipeline\n"
                                              "from utils import fine_sampling, raw2outputs\n\n\n"
                                              "class AppendSmplParamsPipeline(NerfPipeline):\n    pass\n"),
    "solver/nerf_solver.py": ("from models.nerf_pipeline import NerfPipeline\nfrom utils import PositionalEncoder\n\n\n"
                              "class NerfSolver:\n    pass\n"),
    "solver/smpl_nerf_solver.py": ("from models.smpl_nerf_pipeline import SmplNerfPipeline\n"
                                   "from solver.nerf_solver import NerfSolver\n\n\n"
                                   "class SmplNerfSolver(NerfSolver):\n    pass\n"),
}
TOP = ("utils", "models", "solver", "torchsearchsorted")


def stand_in_checkout(root):
    for rel, src in STAND_IN.items():
        path = root / rel
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(src)
    return str(root)


def test_install_rebinds_the_reference_modules(tmp_path):
    ref = stand_in_checkout(tmp_path / "checkout")
    before = set(sys.modules)
    saved = {k: sys.modules.get(k) for k in list(sys.modules) if k.split(".")[0] in TOP}
    saved_path, saved_meta = list(sys.path), list(sys.meta_path)
    from smpl_nerf_amd import dropin, nets, ops, pipelines
    try:
        for k in list(saved):
            sys.modules.pop(k, None)
        dropin._installed = False
        dropin._originals.clear()
        dropin.install(ref)
        import torchsearchsorted
        assert torchsearchsorted.searchsorted is ops.searchsorted
        U = importlib.import_module("utils")                       # the checkout's utils.py (imports torchsearchsorted)
        assert U.searchsorted is ops.searchsorted and U.raw2outputs is ops.raw2outputs
        assert U.fine_sampling is ops.fine_sampling and U.sample_pdf is ops.sample_pdf
        NS = importlib.import_module("solver.nerf_solver")         # `from models.nerf_pipeline import NerfPipeline`
        assert NS.NerfPipeline is pipelines.NerfPipeline
        SS = importlib.import_module("solver.smpl_nerf_solver")
        assert SS.SmplNerfPipeline is pipelines.SmplNerfPipeline
        M = importlib.import_module("models.render_ray_net")
        assert M.RenderRayNet is nets.RenderRayNet
        NP = importlib.import_module("models.nerf_pipeline")
        assert NP.NerfPipeline is pipelines.NerfPipeline and NP.raw2outputs is ops.raw2outputs
        assert importlib.import_module("models.warp_field_net").WarpFieldNet is nets.WarpFieldNet
        AP = importlib.import_module("models.append_smpl_params_pipeline")
        assert AP.AppendSmplParamsPipeline is pipelines.AppendSmplParamsPipeline and AP.fine_sampling is ops.fine_sampling
        # the checkout's own encoder class is kept and is what our pipelines accept
        enc = U.PositionalEncoder(10, False)
        assert U.PositionalEncoder is not None and not isinstance(enc, ops.PositionalEncoder)
        pipe = NS.NerfPipeline(nets.RenderRayNet(), nets.RenderRayNet(), object(), enc, U.PositionalEncoder(4, False))
        d = pipe.model_coarse.desc_for_encoders(pipe.position_encoder, pipe.direction_encoder)
        assert (d.pos_freqs, d.dir_freqs, d.pos_identity) == (10, 4, 0)
        assert dropin.install(ref) == 0                            # idempotent
    finally:
        sys.meta_path[:] = saved_meta
        sys.path[:] = saved_path
        for k in [k for k in sys.modules if k.split(".")[0] in TOP]:
            sys.modules.pop(k, None)
        sys.modules.update({k: v for k, v in saved.items() if v is not None})
        dropin._installed = False
        for k in set(sys.modules) - before:               # whatever the checkout pulled in
            if k.split(".")[0] in TOP:
                sys.modules.pop(k, None)


def test_install_normalises_the_root(tmp_path):
    """a symlinked root matches the (absolute, resolved) module paths; a sibling directory whose name merely
    starts with the root's does not; a missing directory is an error."""
    from smpl_nerf_amd import dropin
    ref = stand_in_checkout(tmp_path / "checkout")
    link = tmp_path / "ref_link"
    os.symlink(ref, link)
    root = dropin._norm_root(str(link))
    assert root == os.path.join(os.path.realpath(ref), "")
    assert dropin._under(os.path.join(ref, "utils.py"), root)
    assert not dropin._under(os.path.realpath(ref) + "2/utils.py", root)
    with pytest.raises(FileNotFoundError):
        dropin.install(str(tmp_path / "nope"))


def test_install_wraps_the_render_entry_point_in_no_grad(tmp_path):
    """inference.inference (inference.py:222-265) calls pipeline(data) with autograd recording on (:247-253); the drop-in
    runs it under torch.no_grad() so that the pipelines take their inference kernels.  A stand-in module of that name under a
    scratch root (the reference's own inference.py needs imageio / torchvision at import)."""
    import torch
    from smpl_nerf_amd import dropin
    root = tmp_path / "checkout"
    root.mkdir()
    (root / "inference.py").write_text("import torch\n\ndef inference(x=1):\n    'render'\n    return torch.is_grad_enabled(), x\n")
    saved_path, saved_meta, saved_mod = list(sys.path), list(sys.meta_path), sys.modules.pop("inference", None)
    try:
        dropin._installed = False
        sys.path.insert(0, str(root))
        import inference as inf                                    # imported BEFORE install: swept
        assert inf.inference() == (True, 1)
        assert dropin.install(str(root)) >= 1
        assert inf.inference(5) == (False, 5) and inf.inference.__doc__ == "render"
        assert torch.is_grad_enabled()
        assert dropin.install(str(root)) == 0                      # idempotent: not wrapped twice
        sys.modules.pop("inference")
        inf2 = importlib.import_module("inference")                # imported AFTER install: patched on import
        assert inf2.inference() == (False, 1)
    finally:
        sys.meta_path[:] = saved_meta
        sys.path[:] = saved_path
        sys.modules.pop("inference", None)
        if saved_mod is not None:
            sys.modules["inference"] = saved_mod
        dropin._installed = False
