"""CPU-side checks of the composed fp32 inference stream's entries (include/smplnerf.h: snerf_mlp_packed_infer_floats,
snerf_mlp_pack_infer_f32, snerf_mlp_fwd_infer_f32, precision SNERF_FP32_INFER of the render entries): sizes and refusals.  Nothing is
launched."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT
from smpl_nerf_amd import _lib, build

SLAB = 8448
NET = _lib.MlpDesc(8, 256, 10, 0, 4, 0, 0, 1 << 4, 1, 0)


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.load()


def test_size_query(lib):
    n = lib.snerf_mlp_packed_infer_floats(NET)
    # 60 trunk slabs + sigma' + 5 of dir-net' + the rgb head, 3 pad slabs, then the scratch of the pack: the float64 intermediate
    # [W_d1 W_a | W_d1 b_a + b_d] (128 x 257 doubles) and the composed parameters (257 + 128 x 281 floats)
    stream, scratch = (67 + 3) * SLAB, 2 * 128 * 257 + 257 + 128 * 281
    assert n >= stream and n == stream + (scratch + 3) // 4 * 4
    assert lib.snerf_mlp_packed_floats(NET) == (77 + 3) * SLAB                  # the regular stream is what it was
    # other shapes: the trunk of the regular stream, + 1 + ceil((T + dir k-blocks) / (32 / TD)) + 1 slabs
    w200 = _lib.MlpDesc(8, 200, 10, 0, 4, 0, 0, 0, 1, 0)
    assert lib.snerf_mlp_packed_infer_floats(w200) >= (2 + 7 * 8 + 1 + 5 + 1 + 3) * SLAB
    w64 = _lib.MlpDesc(3, 64, 10, 0, 4, 0, 0, 0, 0, 0)                          # no directions: T = 4, TD = 2
    assert lib.snerf_mlp_packed_infer_floats(w64) == (1 + 2 * 1 + 1 + 1 + 1 + 3) * SLAB + (2 * 32 * 65 + 65 + 32 * 65 + 3) // 4 * 4
    # no inference stream above width 256: 0, not an error - the caller uses the regular stream
    for width in (320, 512):
        assert lib.snerf_mlp_packed_infer_floats(_lib.MlpDesc(8, width, 10, 0, 4, 0, 0, 1 << 4, 1, 0)) == 0
    # a descriptor no plan exists for is an error here as everywhere
    assert lib.snerf_mlp_packed_infer_floats(None) == -1 and b"desc is null" in lib.snerf_last_error_string()
    assert lib.snerf_mlp_packed_infer_floats(_lib.MlpDesc(8, 1, 10, 0, 4, 0, 0, 0, 1, 0)) == -1


def test_knob_switches_the_stream_off():
    """SNERF_MLP_COMPOSE=0 (read once per process: a child): the size query returns 0 and the entries refuse."""
    code = ("import sys; sys.path.insert(0, sys.argv[1])\n"
            "from smpl_nerf_amd import _lib\n"
            "lib = _lib.load(); d = _lib.MlpDesc(8, 256, 10, 0, 4, 0, 0, 16, 1, 0)\n"
            "assert lib.snerf_mlp_packed_infer_floats(d) == 0\n"
            "assert lib.snerf_mlp_packed_floats(d) == 80 * 8448\n"
            "assert lib.snerf_mlp_pack_infer_f32(d, 64, 64, None) == -1 and b'SNERF_MLP_COMPOSE' in lib.snerf_last_error_string()\n"
            "assert lib.snerf_mlp_fwd_infer_f32(d, 64, 64, 64, 0, None, 16, 4, 64, None, 0, None) == -1\n"
            "assert b'SNERF_MLP_COMPOSE' in lib.snerf_last_error_string()\n")
    subprocess.run([sys.executable, "-c", code, ROOT], check=True, env=dict(os.environ, SNERF_MLP_COMPOSE="0"), timeout=120)


def test_pack_refusals(lib):
    assert lib.snerf_mlp_pack_infer_f32(None, 64, 64, None) == -1 and b"desc is null" in lib.snerf_last_error_string()
    assert lib.snerf_mlp_pack_infer_f32(NET, None, 64, None) == -1 and b"null pointer" in lib.snerf_last_error_string()
    assert lib.snerf_mlp_pack_infer_f32(NET, 64, None, None) == -1 and b"null pointer" in lib.snerf_last_error_string()
    assert lib.snerf_mlp_pack_infer_f32(NET, 64, 68, None) == -2 and b"aligned" in lib.snerf_last_error_string()
    wide = _lib.MlpDesc(8, 320, 10, 0, 4, 0, 0, 1 << 4, 1, 0)
    assert lib.snerf_mlp_pack_infer_f32(wide, 64, 64, None) == -1 and b"above width 256" in lib.snerf_last_error_string()


def test_forward_refusals(lib):
    def call(desc=NET, packed=64, x=64, dirs=64, dps=0, add=None, n=16, spr=4, raw=64, ws=None, ws_bytes=0):
        return lib.snerf_mlp_fwd_infer_f32(desc, packed, x, dirs, dps, add, n, spr, raw, ws, ws_bytes, None), lib.snerf_last_error_string()
    assert call(desc=None) == (-1, b"mlp_fwd_infer: desc is null")
    for arg in ("packed", "x", "raw"):
        rc, err = call(**{arg: None})
        assert rc == -1 and b"null pointer" in err, arg
    rc, err = call(dirs=None)
    assert rc == -1 and b"dirs is null" in err
    rc, err = call(desc=_lib.MlpDesc(8, 256, 10, 0, 4, 0, 69, 1 << 4, 1, 1))
    assert rc == -1 and b"add is null" in err
    for arg in ("packed", "raw"):
        rc, err = call(**{arg: 68})
        assert rc == -2 and b"packed/raw" in err, arg
    assert call(n=-1)[0] == -1 and call(spr=0)[0] == -1
    rc, err = call(dps=4, n=0)                      # no new dirs_per_sample bit
    assert rc == -1 and b"dirs_per_sample is a bit set" in err
    rc, err = call(ws=64, ws_bytes=-1)
    assert rc == -1 and b"negative workspace_bytes" in err
    assert call(n=0, packed=None, x=None, raw=None, dirs=None)[0] == 0          # an empty call is a no-op
    rc, err = call(desc=_lib.MlpDesc(8, 320, 10, 0, 4, 0, 0, 1 << 4, 1, 0))
    assert rc == -1 and b"above width 256" in err


def test_render_entries_take_the_new_precision_code(lib):
    assert _lib.FP32_INFER == 32
    text = open(os.path.join(ROOT, "include", "smplnerf.h")).read()
    assert "#define SNERF_FP32_INFER 32" in text and "#define SNERF_VERSION 109 " in text
    d = NET
    args = [d, None, d, None, _lib.FP32_INFER] + [None] * 7 + [0, 64, 128, 0] + [None] * 6
    assert lib.snerf_render_rays_f32(*args) == 0                                          # B = 0: accepted, a no-op
    assert lib.snerf_render_rays_f32(*(args[:4] + [_lib.FP32_INFER | _lib.REFERENCE_SUM] + args[5:])) == 0
    args[4] = 1
    assert lib.snerf_render_rays_f32(*args) == -1 and b"precision" in lib.snerf_last_error_string()
    args[4] = 33
    assert lib.snerf_render_rays_f32(*args) == -1 and b"precision" in lib.snerf_last_error_string()
    add = [d, None, d, None, _lib.FP32_INFER] + [None] * 8 + [0, 64, 128, 0] + [None] * 6
    da = _lib.MlpDesc(8, 256, 10, 0, 4, 0, 69, 1 << 4, 1, 1)
    add[0] = add[2] = da
    assert lib.snerf_render_rays_add_f32(*add) == 0
    w = _lib.WarpDesc(256, 10, 0, 40)
    smpl = [d, None, d, None, w, None, _lib.FP32_INFER] + [None] * 8 + [0, 64, 128, 0] + [None] * 8
    assert lib.snerf_render_rays_smpl_f32(*smpl) == 0
    # the training entries know no inference stream
    batch = _lib.NerfBatch()
    assert lib.snerf_nerf_train_grads_f32(d, None, None, d, None, None, _lib.FP32_INFER, batch, 0, None, None, None, None, None, None, None, None) < 0
