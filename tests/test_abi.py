"""CPU-side checks of the C-ABI library: it builds, loads, exports every symbol the public header
declares, and validates arguments before touching a device.  No GPU needed, no compute launched."""
import ctypes
import os
import re

import pytest

from conftest import ROOT
from smpl_nerf_amd import _lib, build


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.load()


def header_symbols():
    text = open(os.path.join(ROOT, "include", "smplnerf.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(snerf_[a-z0-9_]+)\s*\(", text)))


def test_header_and_binding_agree(lib):
    syms = header_symbols()
    assert len(syms) >= 12
    assert sorted(_lib.SIGNATURES) == syms          # the ctypes table lists exactly the header's functions
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/smplnerf.h but not exported"


def test_version_and_error_string(lib):
    assert lib.snerf_version() == 109
    assert isinstance(lib.snerf_last_error_string(), bytes)
    assert lib.snerf_device_count() >= 0


def test_only_the_header_symbols_are_exported(lib):
    """-fvisibility=hidden + SNERF_API: `nm -D --defined-only` of the library lists the header's entry points and nothing else
    (no C++ symbols of namespace snerf, no template instantiations a host's own code could collide with)."""
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = sorted(ln.split()[-1] for ln in out.splitlines() if ln.strip())
    assert names == header_symbols(), sorted(set(names) ^ set(header_symbols()))
    assert lib.snerf_shutdown() == 0 and lib.snerf_shutdown() == 0          # idempotent, nothing to destroy on a CPU box


def test_argument_validation_happens_on_the_host(lib):
    # mismatched row counts (searchsorted.py:23-28) -> BADARG, nothing launched
    rc = lib.snerf_searchsorted_f32(None, 3, 4, None, 2, 4, None, 0, None)
    assert rc == -1 and b"rows" in lib.snerf_last_error_string()
    assert lib.snerf_searchsorted_f32(None, 0, 4, None, 0, 4, None, 0, None) == 0      # empty is a no-op
    assert lib.snerf_posenc_f32(None, 5, 0, 10, 0, None, None) == -1
    assert lib.snerf_composite_fwd_f32(None, None, None, 0, None, 4, 0, 0, None, None, None, None) == -1
    assert lib.snerf_sample_pdf_f32(None, None, None, None, None, 4, 2, 128, None, None, None, None, None) == -1
    assert lib.snerf_sample_pdf_f32(None, None, None, None, None, 0, 64, 128, None, None, None, None, None) == 0


def test_mlp_descriptor_arithmetic(lib):
    d = _lib.MlpDesc(8, 256, 10, 0, 4, 0, 0, 1 << 4, 1)
    assert lib.snerf_mlp_param_floats(d) == 610436        # skips=[4]
    d0 = _lib.MlpDesc(8, 256, 10, 0, 4, 0, 0, 0, 1)
    assert lib.snerf_mlp_param_floats(d0) == 595076       # skips=[]
    # 77 slabs of 33 KiB (32 A tiles + bias) + 3 pad slabs (mlp_plan.h)
    assert lib.snerf_mlp_packed_floats(d) == (77 + 3) * 8448
    # any width up to 256 (other widths than 128 / 256 run zero-padded): the parameter count is RenderRayNet's own
    w200 = _lib.MlpDesc(8, 200, 10, 0, 4, 0, 0, 0, 1)
    assert lib.snerf_mlp_param_floats(w200) == (200 * 61 + 7 * 200 * 201 + 200 * 201 + 201 + 100 * 225 + 100 * 101 + 3 * 101)
    assert lib.snerf_mlp_packed_floats(w200) == lib.snerf_mlp_packed_floats(d0)       # the stream of the 256-wide kernel
    # above 256 (r05): kernels of 320 / 384 / 448 / 512 features (other widths zero-padded); a slab is one k-block of all output tiles
    w320 = _lib.MlpDesc(8, 320, 10, 0, 4, 0, 0, 0, 1)
    assert lib.snerf_mlp_param_floats(w320) == (320 * 61 + 7 * 320 * 321 + 320 * 321 + 321 + 160 * 345 + 160 * 161 + 3 * 161)
    w300 = _lib.MlpDesc(8, 300, 10, 0, 4, 0, 0, 0, 1)
    slabs320 = 4 + 7 * 20 + 20 + 1 + (20 + 2 + 2) // 3 + (10 + 2) // 3 + 1    # k-blocks per layer / (32 tiles per slab // output tiles)
    assert lib.snerf_mlp_packed_floats(w320) == lib.snerf_mlp_packed_floats(w300) == (slabs320 + 3) * 8448
    w512 = _lib.MlpDesc(8, 512, 10, 0, 4, 0, 0, 0, 1)
    slabs512 = 4 + 7 * 32 + 32 + 1 + (32 + 2) // 2 + 16 // 2 + 1
    assert lib.snerf_mlp_packed_floats(w512) == (slabs512 + 3) * 8448
    bad = _lib.MlpDesc(8, 640, 10, 0, 4, 0, 0, 0, 1)
    assert lib.snerf_mlp_param_floats(bad) < 0
    assert lib.snerf_mlp_pack_f32(bad, None, None, None) == -1 and b"width must be in [2, 512]" in lib.snerf_last_error_string()
    from smpl_nerf_amd.nets import RenderRayNet, WarpFieldNet
    RenderRayNet(8, 320, 60, 24)                                 # config_parser.py:20 accepts it, and so do the kernels since r05
    # r06: any width constructs - above the fused kernels' limits (the snerf_mlp_* entries above stay at 512: SNERF_E_BADARG) the net
    # runs one nn.Linear at a time through snerf_linear_* (smpl_nerf_amd/layered.py)
    assert RenderRayNet(8, 640, 60, 24)._layered and not RenderRayNet(8, 512, 60, 24)._layered
    assert WarpFieldNet(8, 512, 60, 40)._layered and not WarpFieldNet(8, 256, 60, 40)._layered
    assert RenderRayNet(20, 64, 60, 24)._layered                 # ... and any --netdepth (config_parser.py:19)
    with pytest.raises(ValueError):
        RenderRayNet(8, 1, 60, 24)
    assert lib.snerf_linear_bwd_weight_scratch_floats(1000, 768, 828) == 4 * (768 * 828 + 768)
    assert lib.snerf_mlp_packed_bf16_bytes(w200, 3) < 0     # the split-precision entry points: width 256 only
    assert lib.snerf_mlp_pack_f32(d, None, None, None) == -1


def test_missing_library_is_a_hard_error(monkeypatch):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", "/nonexistent/libsmplnerf_hip.so")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.load()


def test_cpu_tensors_are_rejected():
    import torch
    from smpl_nerf_amd import ops
    a = torch.sort(torch.rand(4, 8), dim=1)[0]
    v = torch.rand(4, 3)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.searchsorted(a, v)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.PositionalEncoder(4, 0).encode(torch.rand(5, 3))
    with pytest.raises(AssertionError):
        ops.searchsorted(torch.rand(3, 4), torch.rand(2, 4))       # reference's shape assert


def test_directions_argument_views():
    import torch
    from smpl_nerf_amd import ops
    d = torch.rand(5, 3)
    t, per = ops._directions_arg(d[:, None, :].expand(5, 7, 3), 5, 7)
    assert per == 0 and t.shape == (5, 3) and torch.equal(t, d)
    t, per = ops._directions_arg(torch.rand(5, 7, 3), 5, 7)
    assert per == 1 and t.shape == (5, 7, 3)
    t, per = ops._directions_arg(d, 5, 7)
    assert per == 0


def test_render_ray_net_state_dict_contract():
    """Checkpoints written by the reference (utils.py:282-283) must load: same keys, same shapes."""
    from smpl_nerf_amd.nets import RenderRayNet
    from smpl_nerf_amd import synthetic as syn
    net = RenderRayNet(8, 256, 60, 24, skips=[4])
    sd = net.state_dict()
    expect = []
    for name, fo, fi in syn.render_ray_net_shapes(skips=(4,)):
        expect += [(name + ".weight", (fo, fi)), (name + ".bias", (fo,))]
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == expect
    assert sum(v.numel() for v in sd.values()) == 610436
    d = net.desc_for_encoded()
    assert (d.pos_freqs, d.pos_identity, d.dir_freqs, d.dir_identity, d.add_dim, d.skip_mask) == (10, 0, 4, 0, 0, 16)
    odd = RenderRayNet(4, 128, 5, 24, additional_input_dim=2, skips=[1])
    d = odd.desc_for_encoded()
    assert (d.pos_freqs, d.add_dim) == (0, 7)


def test_torchsearchsorted_shim_imports_and_has_no_cpu_path():
    """shims/torchsearchsorted is the package reference code imports (utils.py:14); on CPU tensors it must raise -
    the product has no CPU fallback."""
    import importlib
    import sys
    import numpy as np
    import pytest
    import torch
    shims = os.path.join(ROOT, "shims")
    sys.path.insert(0, shims)
    try:
        sys.modules.pop("torchsearchsorted", None)
        mod = importlib.import_module("torchsearchsorted")
        assert mod.__file__.startswith(shims)
        a = torch.from_numpy(np.sort(np.random.default_rng(0).random((3, 9)).astype(np.float32), 1))
        v = torch.rand(3, 5)
        with pytest.raises(RuntimeError):
            mod.searchsorted(a, v, side="right")
        with pytest.raises(AssertionError):          # the reference's own shape asserts come first
            mod.searchsorted(a[0], v)
    finally:
        sys.path.remove(shims)
        sys.modules.pop("torchsearchsorted", None)


def test_split_bf16_and_render_entry_points_validate_on_the_host(lib):
    """Host-side argument checks of the entry points added for the bf16 matrix-core path, the training variants and the
    one-call renderer: descriptor arithmetic, nsplit / precision ranges, null pointers - nothing is launched."""
    d = _lib.MlpDesc(8, 256, 10, 0, 4, 0, 0, 1 << 4, 1)
    # slab = one 32-wide k-block x 16 tiles x nsplit parts (+1 KiB bias): 79 slabs + 3 pad slabs for this net
    b3, b2 = lib.snerf_mlp_packed_bf16_bytes(d, 3), lib.snerf_mlp_packed_bf16_bytes(d, 2)
    assert b3 % (3 * 16384 + 1024) == 0 and b2 % (2 * 16384 + 1024) == 0
    assert b3 // (3 * 16384 + 1024) == b2 // (2 * 16384 + 1024) > 3
    assert lib.snerf_mlp_packed_bf16_bytes(d, 4) == -1 and b"nsplit" in lib.snerf_last_error_string()
    # nsplit = SNERF_SPLIT_F16X3 (16): two fp16 parts - the layout of nsplit = 2, accepted by every split entry point
    assert _lib.SPLIT_F16X3 == 16
    assert lib.snerf_mlp_packed_bf16_bytes(d, _lib.SPLIT_F16X3) == b2
    assert lib.snerf_mlp_packed_t_bf16_bytes(d, _lib.SPLIT_F16X3, 1) == lib.snerf_mlp_packed_t_bf16_bytes(d, 2, 1)
    assert lib.snerf_mlp_fwd_bf16_f32(d, None, _lib.SPLIT_F16X3, None, None, 0, None, 0, 64, None, None) == 0
    assert lib.snerf_mlp_bwd_bf16_f32(d, None, _lib.SPLIT_F16X3, None, None, 0, None, None, None, None) == 0
    narrow = _lib.MlpDesc(4, 128, 10, 0, 4, 0, 0, 2, 1)
    assert lib.snerf_mlp_packed_bf16_bytes(narrow, 3) == -1 and b"256" in lib.snerf_last_error_string()
    assert lib.snerf_mlp_packed_t_bf16_bytes(d, 3, 0) > 0
    assert lib.snerf_mlp_packed_t_bf16_bytes(d, 3, 1) > lib.snerf_mlp_packed_t_bf16_bytes(d, 3, 0)   # + encoder columns
    assert lib.snerf_mlp_packed_t_bf16_bytes(d, 1, 0) == -1
    assert lib.snerf_mlp_pack_bf16(d, None, None, 3, None) == -1
    assert lib.snerf_mlp_pack_t_bf16(d, None, None, 3, 0, None) == -1
    assert lib.snerf_mlp_fwd_bf16_f32(d, None, 3, None, None, 0, None, 0, 64, None, None) == 0        # n = 0: no-op
    assert lib.snerf_mlp_fwd_bf16_f32(d, None, 3, None, None, 0, None, 128, 64, None, None) == -1     # null pointers
    assert lib.snerf_mlp_fwd_train_bf16_f32(d, None, 5, None, None, 0, None, 128, 64, None, None, None) == -1
    assert lib.snerf_mlp_bwd_bf16_f32(d, None, 3, None, None, 0, None, None, None, None) == 0
    assert lib.snerf_mlp_bwd_bf16_f32(d, None, 3, None, None, 128, None, None, None, None) == -1
    assert lib.snerf_mlp_bwd_inputs_bf16_f32(d, None, 3, None, None, None, None, 0, 1, 128, None, None, None, None, None,
                                             None) == -1
    # one-call renderer
    ws = lib.snerf_render_rays_workspace_bytes(16384, 64, 128)
    assert ws >= 16384 * (64 * 16 + 64 * 8 + 128 * 4 + 192 * 4 + 192 * 16) and ws % 16 == 0
    assert lib.snerf_render_rays_workspace_bytes(16384, 0, 128) == -1
    args = [d, None, d, None, 3] + [None] * 7 + [0, 64, 128, 0, None, None, None, None, None, None]
    assert lib.snerf_render_rays_f32(*args) == 0                                                         # B = 0: no-op
    args[12] = 4
    assert lib.snerf_render_rays_f32(*args) == -1 and b"null" in lib.snerf_last_error_string()
    args[4] = 1
    assert lib.snerf_render_rays_f32(*args) == -1 and b"precision" in lib.snerf_last_error_string()


def test_pipeline_set_precision_reaches_every_net():
    import torch
    from smpl_nerf_amd.nets import RenderRayNet, WarpFieldNet
    from smpl_nerf_amd.ops import PositionalEncoder
    from smpl_nerf_amd.pipelines import PipelineArgs, SmplNerfPipeline
    enc = PositionalEncoder(10, 0)
    pipe = SmplNerfPipeline(RenderRayNet(), RenderRayNet(), WarpFieldNet(8, 256, 60, 40), PipelineArgs(), enc,
                            PositionalEncoder(4, 0), enc)
    assert pipe.set_precision("bf16x6") is pipe
    assert {pipe.model_coarse.precision, pipe.model_fine.precision, pipe.model_warp_field.precision} == {"bf16x6"}
    with pytest.raises(ValueError):
        pipe.set_precision("fp16")


def test_training_buffer_sizes_of_widths_above_256(lib):
    """Host-side layout of the 320 .. 512 kernels (csrc/mlp_plan.h: make_train_layout): tile-rows of 16 features per layer input,
    one tile-row per ReLU sign mask (four words per lane) instead of half a row, d Y rows per layer output; the transposed stream
    of the dgrad; a width is laid out as the next kernel width above it (config_parser.py:20 --netwidth)."""
    import ctypes

    def sizes(width, n, depth=8, skip_mask=1 << 4):
        d = _lib.MlpDesc(depth, width, 10, 0, 4, 0, 0, skip_mask, 1)
        v = [ctypes.c_int64() for _ in range(4)]
        cnt = ctypes.c_int32()
        assert lib.snerf_mlp_train_sizes(d, n, *[ctypes.byref(x) for x in v], ctypes.byref(cnt)) == 0
        return [x.value for x in v] + [cnt.value]

    n = 1000
    for width, T in ((512, 32), (500, 32), (448, 28), (384, 24), (330, 24), (320, 20), (257, 20)):
        act, dy, pt, gp, cnt = sizes(width, n)
        nh = 7
        rows = 4 + 2 + (nh + 1) * T + T + T // 2 + T // 2 + (nh + 2)      # encoders, x[1..nh+1], o, h1, h2, one row per mask
        assert act >= rows * n * 16 and act - rows * n * 16 <= 64, (width, act, rows)
        dy_rows = (nh + 2) * T + 1 + T // 2 + T // 2 + 1                  # trunk layers + additional, sigma, directional x 2, rgb
        assert dy >= dy_rows * n * 16 and dy - dy_rows * n * 16 <= 64, (width, dy, dy_rows)
        assert cnt == 8 and gp % cnt == 0                                  # wgrad_chunks(1000) partials of one slot-ordered gradient
        assert pt % 8448 == 0                                              # whole slabs
    # the same description below 256 keeps two masks per tile-row
    act256 = sizes(256, n)[0]
    assert act256 >= (4 + 2 + 8 * 16 + 16 + 8 + 8 + 5) * n * 16 and act256 - (4 + 2 + 8 * 16 + 16 + 8 + 8 + 5) * n * 16 <= 64
    # a 512-wide first layer needs two k-blocks of input: 3 identity columns alone are refused by name
    tiny = _lib.MlpDesc(2, 512, 0, 1, 0, 1, 0, 0, 1)
    assert lib.snerf_mlp_param_floats(tiny) < 0
    assert lib.snerf_mlp_pack_f32(tiny, None, None, None) == -1 and b"two k-blocks" in lib.snerf_last_error_string()


# ---- the per-net entries: what each refuses on the host, and with which code -------------------------------------------------
# Every row is one call that differs from the entry's BASE call (n = 16 samples in rays of 4, every pointer the fake address 64)
# in the arguments named; BASE itself is never called.  A row is refused on the host (code < 0) or is an empty call (n == 0), so
# nothing is ever launched on the fake pointers.  (-1 = SNERF_E_BADARG, -2 = SNERF_E_ALIGN; the text is a part of
# snerf_last_error_string() that names the argument.)  A tuple of names stands for one row per name; EMPTY: n = 0 with every
# pointer null ("EMPTY d_x": every pointer but d_x).
_NET = _lib.MlpDesc(8, 256, 10, 0, 4, 0, 6, 1 << 4, 1, 0)        # reads dirs and per-ray additional inputs; a width every entry has
_NET_W1 = _lib.MlpDesc(8, 1, 10, 0, 4, 0, 6, 1 << 4, 1, 0)
_WARP = _lib.WarpDesc(256, 10, 0, 40)
_WARP_W0 = _lib.WarpDesc(0, 10, 0, 40)                            # (a WarpFieldNet of width 1 is valid)
EMPTY = "EMPTY"
_FWD = "desc packed x dirs dps add n spr raw"
_BWD_IN = "x dirs dps spr n dy gpart flat_grad d_x d_dirs stream"
_WFWD = "desc packed x pose_enc o n spr warp warped sdirs"
NET_ENTRIES = {
    "snerf_mlp_fwd_f32": _FWD + " stream",
    "snerf_mlp_fwd_ws_f32": _FWD + " workspace workspace_bytes stream",
    "snerf_mlp_fwd_train_f32": _FWD + " act stream",
    "snerf_mlp_fwd_encoded_f32": "desc packed x n row_floats raw stream",
    "snerf_mlp_fwd_encoded_train_f32": "desc packed x n row_floats raw act stream",
    "snerf_mlp_fwd_bf16_f32": "desc packed nsplit x dirs dps add n spr raw stream",
    "snerf_mlp_fwd_train_bf16_f32": "desc packed nsplit x dirs dps add n spr raw act stream",
    "snerf_mlp_bwd_f32": "desc packed_t act d_raw n dy gpart flat_grad stream",
    "snerf_mlp_bwd_inputs_f32": "desc packed_t act d_raw " + _BWD_IN,
    "snerf_mlp_bwd_bf16_f32": "desc packed_t nsplit act d_raw n dy gpart flat_grad stream",
    "snerf_mlp_bwd_inputs_bf16_f32": "desc packed_t nsplit act d_raw " + _BWD_IN,
    "snerf_warp_fwd_f32": _WFWD + " stream",
    "snerf_warp_fwd_ws_f32": _WFWD + " workspace workspace_bytes stream",
    "snerf_warp_fwd_train_f32": _WFWD + " act stream",
    "snerf_warp_fwd_bf16_f32": _WFWD + " stream",
    "snerf_warp_bwd_f32": "desc packed_t act d_warp n dy gpart flat_grad stream",
    # pack and size entries that take a descriptor
    "snerf_mlp_param_floats": "desc", "snerf_mlp_packed_floats": "desc",
    "snerf_mlp_pack_f32": "desc params packed stream",
    "snerf_mlp_pack_t_f32": "desc params packed input_grad stream",
    "snerf_mlp_fold_workspace_bytes": "desc n spr",
    "snerf_mlp_train_sizes": "desc n o0 o1 o2 o3 o4",
    "snerf_mlp_dy_layout": "desc o0 o1 o2 o3",
    "snerf_mlp_stream_slots": "desc o0 o1 input_grad stream",
    "snerf_mlp_packed_bf16_bytes": "desc nsplit",
    "snerf_mlp_pack_bf16": "desc params packed nsplit stream",
    "snerf_mlp_packed_t_bf16_bytes": "desc nsplit input_grad",
    "snerf_mlp_pack_t_bf16": "desc params packed nsplit input_grad stream",
    "snerf_warp_param_floats": "desc", "snerf_warp_packed_floats": "desc",
    "snerf_warp_pack_f32": "desc params packed stream",
    "snerf_warp_pack_t_f32": "desc params packed stream",
    "snerf_warp_fold_workspace_bytes": "desc n spr",
    "snerf_warp_train_sizes": "desc n o0 o1 o2 o3",
    "snerf_warp_packed_bf16_bytes": "desc",
    "snerf_warp_pack_bf16": "desc params packed stream",
}
_SCALARS = {"n": 16, "spr": 4, "dps": 0, "nsplit": 3, "row_floats": 200, "workspace_bytes": 0, "input_grad": 1, "stream": None,
            "workspace": None, "o0": None, "o1": None, "o2": None, "o3": None, "o4": None}


def _base(entry):
    """The call every row of `entry` departs from.  Never made: with real buffers it would be a valid call."""
    base = {a: _SCALARS.get(a, 64) for a in NET_ENTRIES[entry].split()}
    base["desc"] = _WARP if "warp" in entry else _NET
    return base


_DESC = [({"desc": None}, -1, b"desc is null"), ({"desc": _NET_W1}, -1, b"width must be in [2, 512]")]
_WDESC = [({"desc": None}, -1, b"desc is null"), ({"desc": _WARP_W0}, -1, b"width must be in [1, 256]")]
_N_SPR = [({"n": -1}, -1, b"bad n/samples_per_ray"), ({"spr": 0}, -1, b"bad n/samples_per_ray"), (EMPTY, 0, b"")]
_MLP_PTRS = [(("packed", "x", "raw"), -1, b"null pointer"), ({"dirs": None}, -1, b"dirs is null"), ({"add": None}, -1, b"add is null")]
_DPS_BITS = [({"dps": 4, "n": 0}, -1, b"dirs_per_sample is a bit set"), ({"dps": -1, "n": 0}, -1, b"dirs_per_sample is a bit set")]
_NSPLIT = [({"nsplit": 4, "n": 0}, -1, b"nsplit"), ({"nsplit": 0, "n": 0}, -1, b"nsplit"),
           ({"desc": _lib.MlpDesc(8, 128, 10, 0, 4, 0, 6, 1 << 4, 1, 0)}, -1, b"width 256 only")]
_NSPLIT_PACK = [({"nsplit": 4}, -1, b"nsplit"), _NSPLIT[2]]
_BWD = [({"n": -1}, -1, b"negative n"),
        (("packed_t", "act", "dy", "gpart", "flat_grad"), -1, b"null pointer"),
        ({"packed_t": 68}, -2, b"aligned"), ({"act": 68}, -2, b"aligned"), ({"dy": 68}, -2, b"aligned"), ({"gpart": 68}, -2, b"aligned")]
_MLP_BWD = _BWD + [({"d_raw": None}, -1, b"null pointer"), ({"d_raw": 68}, -2, b"aligned")]
_BWD_INPUTS = [(EMPTY, -1, b"d_x is null"), (EMPTY + " d_x", 0, b""), ({"d_x": None, "n": 0}, -1, b"d_x is null"), ({"d_x": None}, -1, b"d_x is null"),
               (("x", "dirs", "d_dirs"), -1, b"input gradients need"), ({"spr": 0}, -1, b"input gradients need")]
_WARP_PTRS = [(("packed", "warp"), -1, b"null pointer"), ({"pose_enc": None}, -1, b"pose_enc is null"),
              ({"warped": None}, -1, b"sdirs needs warped and o"), ({"o": None}, -1, b"sdirs needs warped and o"),
              ({"packed": 68}, -2, b"packed must be 16-byte aligned")]
_WARP_X = [({"x": None}, -1, b"x is null"), ({"x": None, "sdirs": None}, -1, b"x is null")]
_PACK = [(("params", "packed"), -1, b"null pointer"), ({"packed": 68}, -2, b"aligned")]
NET_ROWS = {
    "snerf_mlp_fwd_f32": _DESC + _N_SPR + _MLP_PTRS + _DPS_BITS + [({"packed": 68}, -2, b"packed/raw"), ({"raw": 68}, -2, b"packed/raw")],
    "snerf_mlp_fwd_ws_f32": _DESC + _N_SPR + _MLP_PTRS + _DPS_BITS + [
        ({"packed": 68}, -2, b"packed/raw"), ({"raw": 68}, -2, b"packed/raw"),
        ({"workspace": 64, "workspace_bytes": -1}, -1, b"negative workspace_bytes"),
        ({"workspace": 64, "workspace_bytes": -1, "n": 0}, 0, b"")],          # (an empty call returns before it looks at the workspace)
    "snerf_mlp_fwd_train_f32": _DESC + _N_SPR + _MLP_PTRS + [
        ({"act": None}, -1, b"null pointer"), ({"dps": 4, "n": 0}, 0, b""),    # (dirs_per_sample is a boolean here)
        ({"packed": 68}, -2, b"packed/raw/act"), ({"raw": 68}, -2, b"packed/raw/act"), ({"act": 68}, -2, b"packed/raw/act")],
    "snerf_mlp_fwd_encoded_f32": _DESC + [
        ({"n": -1}, -1, b"bad n"), (EMPTY, 0, b""), (("packed", "x", "raw"), -1, b"null pointer"),
        ({"packed": 68}, -2, b"packed/raw"), ({"raw": 68}, -2, b"packed/raw"),
        ({"row_floats": 65}, -1, b"too short"), ({"row_floats": 1 << 31}, -1, b"row of"), ({"row_floats": 0, "n": 0}, 0, b"")],
    "snerf_mlp_fwd_encoded_train_f32": _DESC + [
        ({"n": -1}, -1, b"bad n"), (EMPTY, 0, b""), (("packed", "x", "raw", "act"), -1, b"null pointer"),
        ({"packed": 68}, -2, b"packed/raw/act"), ({"raw": 68}, -2, b"packed/raw/act"), ({"act": 68}, -2, b"packed/raw/act"),
        ({"row_floats": 65}, -1, b"too short"), ({"row_floats": 1 << 31}, -1, b"row of"), ({"row_floats": 0, "n": 0}, 0, b"")],
    "snerf_mlp_fwd_bf16_f32": _DESC + _N_SPR + _MLP_PTRS + _NSPLIT + [
        ({"dps": 4, "n": 0}, 0, b""), ({"packed": 68}, -2, b"packed/raw"), ({"raw": 68}, -2, b"packed/raw")],
    "snerf_mlp_fwd_train_bf16_f32": _DESC + _N_SPR + _MLP_PTRS + _NSPLIT + [
        ({"act": None}, -1, b"null pointer"), ({"dps": 4, "n": 0}, 0, b""),
        ({"packed": 68}, -2, b"packed/raw/act"), ({"raw": 68}, -2, b"packed/raw/act"), ({"act": 68}, -2, b"packed/raw/act")],
    "snerf_mlp_bwd_f32": _DESC + _MLP_BWD + [(EMPTY, 0, b"")],
    "snerf_mlp_bwd_inputs_f32": _DESC + _MLP_BWD + _BWD_INPUTS,
    "snerf_mlp_bwd_bf16_f32": _DESC + _MLP_BWD + _NSPLIT + [(EMPTY, 0, b"")],
    "snerf_mlp_bwd_inputs_bf16_f32": _DESC + _MLP_BWD + _BWD_INPUTS + _NSPLIT,
    "snerf_warp_fwd_f32": _WDESC + _N_SPR + _WARP_PTRS + _WARP_X,
    "snerf_warp_fwd_ws_f32": _WDESC + _N_SPR + _WARP_PTRS + _WARP_X + [
        ({"workspace": 64, "workspace_bytes": -1}, -1, b"negative workspace_bytes"),
        ({"workspace": 64, "workspace_bytes": -1, "n": 0}, -1, b"negative workspace_bytes")],
    "snerf_warp_fwd_train_f32": _WDESC + _N_SPR[:2] + _WARP_PTRS + _WARP_X + [
        (EMPTY, -1, b"act is null"), (EMPTY + " act", 0, b""), ({"act": None, "n": 0}, -1, b"act is null"), ({"act": None}, -1, b"act is null")],
    # the split-bf16 warp requires x in every call
    "snerf_warp_fwd_bf16_f32": _WDESC + _N_SPR + _WARP_PTRS + [
        ({"x": None}, -1, b"null pointer"), ({"x": None, "warped": None, "sdirs": None}, -1, b"null pointer"),
        ({"desc": _lib.WarpDesc(128, 10, 0, 40)}, -1, b"width 256 only")],
    "snerf_warp_bwd_f32": _WDESC + _BWD + [({"d_warp": None}, -1, b"null pointer"), (EMPTY, 0, b"")],
    # (snerf_*_param_floats / _packed_floats name the net, not the reason, in one of the two builds this table is run against)
    "snerf_mlp_param_floats": [({"desc": None}, -1, b"mlp"), ({"desc": _NET_W1}, -1, b"mlp")],
    "snerf_mlp_packed_floats": [({"desc": None}, -1, b"mlp"), ({"desc": _NET_W1}, -1, b"mlp")],
    "snerf_mlp_pack_f32": _DESC + _PACK,
    "snerf_mlp_pack_t_f32": _DESC + _PACK,
    "snerf_mlp_fold_workspace_bytes": _DESC + [({"n": -1}, -1, b"bad n/samples_per_ray"), ({"spr": 0}, -1, b"bad n/samples_per_ray")],
    "snerf_mlp_train_sizes": _DESC + [({"n": -1}, -1, b"negative n")],
    "snerf_mlp_dy_layout": _DESC,
    "snerf_mlp_stream_slots": _DESC,
    "snerf_mlp_packed_bf16_bytes": _DESC + _NSPLIT_PACK,
    "snerf_mlp_pack_bf16": _DESC + _PACK + _NSPLIT_PACK,
    "snerf_mlp_packed_t_bf16_bytes": _DESC + _NSPLIT_PACK,
    "snerf_mlp_pack_t_bf16": _DESC + _PACK + _NSPLIT_PACK,
    "snerf_warp_param_floats": [({"desc": None}, -1, b"warp"), ({"desc": _WARP_W0}, -1, b"warp")],
    "snerf_warp_packed_floats": [({"desc": None}, -1, b"warp"), ({"desc": _WARP_W0}, -1, b"warp")],
    "snerf_warp_pack_f32": _WDESC + _PACK,
    "snerf_warp_pack_t_f32": _WDESC + _PACK,
    "snerf_warp_fold_workspace_bytes": _WDESC + [({"n": -1}, -1, b"bad n/samples_per_ray"), ({"spr": 0}, -1, b"bad n/samples_per_ray")],
    "snerf_warp_train_sizes": _WDESC + [({"n": -1}, -1, b"negative n")],
    "snerf_warp_packed_bf16_bytes": _WDESC + [({"desc": _lib.WarpDesc(128, 10, 0, 40)}, -1, b"width 256 only")],
    "snerf_warp_pack_bf16": _WDESC + _PACK + [({"desc": _lib.WarpDesc(128, 10, 0, 40)}, -1, b"width 256 only")],
}


def _net_rows(table):
    out = []
    for entry, rows in table.items():
        base = _base(entry)
        for change, code, text in rows:
            if isinstance(change, str) and change.startswith(EMPTY):
                changes = [dict({a: None for a, v in base.items() if v == 64 and a not in change.split()[1:]}, n=0)]
            elif isinstance(change, tuple):
                changes = [{a: None} for a in change]
            else:
                changes = [change]
            for ch in changes:
                assert ch and set(ch) <= set(base) and any(base[a] is not ch[a] for a in ch), (entry, ch)   # departs from BASE
                assert code < 0 or ch.get("n") == 0, (entry, ch)                                            # refused, or empty
                label = ",".join(f"{a}={'bad' if a == 'desc' and v is not None else v}" for a, v in ch.items())
                out.append(pytest.param(entry, ch, code, text, id=f"{entry[6:]}-{label}-{len(out)}"))
    return out


def _call(lib, entry, change):
    args = dict(_base(entry), **change)
    rc = getattr(lib, entry)(*[args[a] for a in NET_ENTRIES[entry].split()])
    return rc, lib.snerf_last_error_string()


def test_net_entry_table_covers_every_entry():
    assert set(NET_ROWS) == set(NET_ENTRIES)
    for entry, names in NET_ENTRIES.items():
        assert len(names.split()) == len(_lib.SIGNATURES[entry][1]), entry


@pytest.mark.parametrize("entry,change,code,text", _net_rows(NET_ROWS))
def test_net_entries_refuse_on_the_host(lib, entry, change, code, text):
    rc, err = _call(lib, entry, change)
    assert rc == code, (rc, err)
    assert text in err, err


# Calls wrong in two ways at once, where the copies of the forward checks disagreed before they became one: the encoded inference
# looked at the row length first, the encoded training forward at the alignment.  One order now: alignment first.
NET_ROWS_TWO_FAULTS = {
    "snerf_mlp_fwd_encoded_f32": [({"packed": 68, "row_floats": 65}, -2, b"aligned"), ({"raw": 68, "row_floats": 65}, -2, b"aligned")],
    "snerf_mlp_fwd_encoded_train_f32": [({"packed": 68, "row_floats": 65}, -2, b"aligned"), ({"act": 68, "row_floats": 65}, -2, b"aligned")],
}


@pytest.mark.parametrize("entry,change,code,text", _net_rows(NET_ROWS_TWO_FAULTS))
def test_net_entries_checked_in_one_order_when_wrong_twice(lib, entry, change, code, text):
    rc, err = _call(lib, entry, change)
    assert rc == code, (rc, err)
    assert text in err, err
