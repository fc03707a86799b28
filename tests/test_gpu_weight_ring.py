"""The LDS-DMA weight ring (csrc/mlp_device.h: SlabPipeDma) with its slabs in flight across the slab barrier, on the GPU: the
race screen at frame size.  A slab read before it has landed, or overwritten before its last read, shows as rows that differ
between two runs, between the 8-wave DMA kernel and the kernels of small calls (register-staged ring: an independent pipe with
bit-identical arithmetic), or from a float64 evaluation.  tests/test_weight_ring_isa.py holds the compiled waits themselves."""
import numpy as np
import pytest
import torch

import torch_ref as R
from smpl_nerf_amd import synthetic as syn

pytestmark = pytest.mark.gpu
F32 = np.float32
RAYS, SPR = 16384, 192            # one 128 x 128 frame, 64 coarse + 128 fine samples per ray


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _net(dev, params, **kw):
    from smpl_nerf_amd.nets import RenderRayNet
    net = RenderRayNet(kw.get("n_layers", 8), kw.get("width", 256), 60, 24, skips=list(kw.get("skips", (4,))))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    return net.to(dev)


def _encoders():
    from smpl_nerf_amd.ops import PositionalEncoder
    return PositionalEncoder(10, 0), PositionalEncoder(4, 0)


def test_frame_sized_render_is_repeatable_and_equals_small_calls(dev):
    """16 384 x 192 samples through the coarse and the fine net in turn, twice: every workgroup of the persistent 8-wave kernel
    walks ~96 tiles of 128 samples and wraps the 77-slab stream as often, and a launch starts on LDS the other net's weights
    were in.  Both rounds bit-equal; the first, a middle and the last tile of several workgroups bit-equal to the same rows
    evaluated by small calls (one per block: the latency-class kernels on the register-staged ring)."""
    pc, pf = syn.make_scene_nets(101)
    coarse, fine = _net(dev, pc), _net(dev, pf)
    pe, de = _encoders()
    rng = np.random.default_rng(20)
    n = RAYS * SPR
    pts = torch.from_numpy(rng.uniform(-1.5, 1.5, (n, 3)).astype(F32)).to(dev)
    dirs = torch.from_numpy(rng.normal(size=(RAYS, 3)).astype(F32)).to(dev)
    with torch.no_grad():
        outs = []
        for _ in range(2):
            outs.append((coarse.forward_fused(pts, dirs, SPR, pe, de).clone(), fine.forward_fused(pts, dirs, SPR, pe, de).clone()))
        torch.cuda.synchronize()
        for k, name in enumerate(("coarse", "fine")):
            a, b = outs[0][k], outs[1][k]
            assert bool(torch.isfinite(a).all()), name
            assert torch.equal(a, b), (name, int((a != b).any(dim=1).sum()), "rows differ between two runs")
        assert not torch.equal(outs[0][0], outs[0][1])       # (two different nets)
        # tiles of workgroup b: b, b + G, b + 2 G, ... (G workgroups = the CUs)
        G = torch.cuda.get_device_properties(dev).multi_processor_count
        n_tiles = n // 128
        per_wg = n_tiles // G
        assert per_wg >= 8
        for b in (0, 1, G // 2 + 3, G - 1):
            for j in (0, per_wg // 2, per_wg - 1):
                t = b + j * G
                rows = slice(t * 128, (t + 1) * 128)
                d_rows = dirs[torch.arange(t * 128, (t + 1) * 128, device=dev) // SPR]       # per-sample directions: the same values
                for k, net in enumerate((coarse, fine)):
                    small = net.forward_fused(pts[rows], d_rows, 1, pe, de)
                    got = outs[0][k][rows]
                    assert torch.equal(got, small), (k, b, j, int((got != small).any(dim=1).sum()), "rows differ from the small call")


def test_width_512_net_on_the_dma_ring_against_float64(dev):
    """Width 512: the DMA pipe at one wave per SIMD (no partner wave covers a wave that waits for its weights), eight pieces per
    wave and slab.  ~36 000 samples (two to three 64-sample tiles per workgroup: the stream wraps) against a float64 evaluation, at the
    tolerance of the width tests (tests/test_gpu_round3.py: 5 x 2e-5 max(1, max|ref|) for the fused form)."""
    kw = dict(n_layers=8, width=512, skips=(4,))
    params = syn.make_render_ray_net_params(7 + 512, 30.0, 10.0, **kw)
    net = _net(dev, params, **kw)
    pe, de = _encoders()
    rng = np.random.default_rng(512)
    n = 256 * 64 * 2 + 64 * 50 + 13
    pts, dirs = rng.uniform(-2, 2, (n, 3)).astype(F32), rng.normal(size=(n, 3)).astype(F32)
    p64, d64 = torch.from_numpy(pts).double(), torch.from_numpy(dirs).double()
    dn = d64 / torch.norm(d64, dim=-1, keepdim=True)
    x_enc = torch.cat([R.posenc(p64, 10, 0), R.posenc(dn, 4, 0)], -1)
    P = {k: torch.from_numpy(v).double() for k, v in params.items()}
    ref = R.render_ray_net(P, x_enc, n_layers=8, skips=(4,)).numpy()
    tol = 2e-5 * max(1.0, float(np.abs(ref).max()))
    with torch.no_grad():
        a = net.forward_fused(torch.from_numpy(pts).to(dev), torch.from_numpy(dirs).to(dev), 1, pe, de)
        b = net.forward_fused(torch.from_numpy(pts).to(dev), torch.from_numpy(dirs).to(dev), 1, pe, de)
    assert torch.equal(a, b)
    err = np.abs(a.cpu().numpy().astype(np.float64) - ref)
    print(f"width 512: max|err| {err.max():.3e} (tolerance {5 * tol:.3e}, max|ref| {np.abs(ref).max():.3e})")
    np.testing.assert_allclose(a.cpu().numpy().astype(np.float64), ref, rtol=0, atol=5 * tol)
