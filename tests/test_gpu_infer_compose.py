"""The composed fp32 inference stream (csrc/mlp_plan.h: make_plan_infer; snerf_mlp_pack_infer_f32 / snerf_mlp_fwd_infer_f32 and the
render entries' precision SNERF_FP32_INFER) on the GPU.  additional_linear_layer, sigma_out_layer, directional_input and
directional_net[0] follow each other without an activation; for inference they are packed as two affine maps of the last trunk
activation (sigma', dir-net'), composed in float64 and rounded once.  A net in eval() mode runs its no-grad fp32 calls on that
stream; in train() mode (and with SNERF_MLP_COMPOSE=0) on the regular one, whose bits are the training forward's.

Every error figure is printed before its assert (pytest -s; profiles/compose_errors.txt holds a run): the composed kernel's
error against float64 beside the regular kernel's on the same inputs."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import torch_ref as R
from conftest import ROOT
from smpl_nerf_amd import synthetic as syn

pytestmark = pytest.mark.gpu
F32 = np.float32

# name -> (RenderRayNet arguments, position encoder (L, identity), direction encoder, add_first, samples per ray)
DEFAULT = dict(n_layers=8, width=256, skips=(4,))
NETS = {
    "default": (DEFAULT, (10, 0), (4, 0), False, 1),
    "n4-skip1-identity": (dict(n_layers=4, width=256, skips=(1,)), (6, 1), (4, 1), False, 1),
    "n2-noskip": (dict(n_layers=2, width=256, skips=()), (10, 0), (4, 0), False, 1),
    "n10-skips257": (dict(n_layers=10, width=256, skips=(2, 5, 7)), (10, 0), (4, 0), False, 1),
    "n1": (dict(n_layers=1, width=256, skips=()), (10, 0), (4, 0), False, 1),
    "nodir": (dict(n_layers=8, width=256, skips=(4,), use_directional_input=0), (10, 0), (4, 0), False, 1),
    "w64": (dict(n_layers=8, width=64, skips=(4,)), (10, 0), (4, 0), False, 1),
    "w200": (dict(n_layers=8, width=200, skips=(4,)), (10, 0), (4, 0), False, 1),
    "add69-first-fold": (dict(n_layers=8, width=256, skips=(4,), additional_input_dim=69), (10, 0), (4, 0), True, 24),
    "add69-last-fold": (dict(n_layers=8, width=256, skips=(4,), additional_input_dim=69), (10, 0), (4, 0), False, 24),
    "add69-first-nofold": (dict(n_layers=8, width=256, skips=(4,), additional_input_dim=69), (10, 0), (4, 0), True, 4),
    "add69-last-nofold": (dict(n_layers=8, width=256, skips=(4,), additional_input_dim=69), (10, 0), (4, 0), False, 4),
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _encoders(pos, dirs):
    from smpl_nerf_amd.ops import PositionalEncoder
    return PositionalEncoder(pos[0], bool(pos[1])), PositionalEncoder(dirs[0], bool(dirs[1]))


def _dims(pos, dirs):
    return 3 * (pos[1] + 2 * pos[0]), 3 * (dirs[1] + 2 * dirs[0])


def _build(dev, name, seed=None):
    from smpl_nerf_amd.nets import RenderRayNet
    kw, pos, dirs, add_first, spr = NETS[name]
    pdim, ddim = _dims(pos, dirs)
    shape = dict(kw, positions_dim=pdim, directions_dim=ddim)
    params = syn.make_render_ray_net_params(1000 + sorted(NETS).index(name) if seed is None else seed, 30.0, 10.0, **shape)
    net = RenderRayNet(kw["n_layers"], kw["width"], pdim, ddim, kw.get("additional_input_dim", 0), skips=list(kw["skips"]),
                       use_directional_input=kw.get("use_directional_input", 1))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    return net.to(dev), params, shape


def _inputs(dev, name, rays, seed):
    kw, pos, dirs, add_first, spr = NETS[name]
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(rng.uniform(-2, 2, (rays * spr, 3)).astype(F32)).to(dev)
    d = torch.from_numpy(rng.normal(size=(rays, 3)).astype(F32)).to(dev)
    na = kw.get("additional_input_dim", 0)
    add = torch.from_numpy(rng.normal(size=(rays, na)).astype(F32)).to(dev) if na else None
    return x, d, add


def _fused(net, name, x, d, add):
    kw, pos, dirs, add_first, spr = NETS[name]
    pe, de = _encoders(pos, dirs)
    with torch.no_grad():
        return net.forward_fused(x, d, spr, pe, de, additional=add, add_first=add_first)


def _ref64(dev, name, params, shape, x, d, add):
    """float64 evaluation of the UNCOMPOSED network (tests/torch_ref.py), on the device."""
    kw, pos, dirs, add_first, spr = NETS[name]
    P = {k: torch.from_numpy(v).double().to(dev) for k, v in params.items()}
    x64, d64 = x.double(), d.double().repeat_interleave(spr, dim=0)
    dn = d64 / torch.norm(d64, dim=-1, keepdim=True)
    cols = [R.posenc(x64, pos[0], pos[1])]
    if add is not None:
        a = add.double().repeat_interleave(spr, dim=0)
        cols = [a] + cols if add_first else cols + [a]
    rows = torch.cat(cols + [R.posenc(dn, dirs[0], dirs[1])], -1)
    return R.render_ray_net(P, rows, n_layers=kw["n_layers"], positions_dim=shape["positions_dim"], directions_dim=shape["directions_dim"],
                            additional_input_dim=kw.get("additional_input_dim", 0), skips=kw["skips"],
                            use_directional_input=kw.get("use_directional_input", 1))


def _check_against_float64(dev, name, rays, tag):
    net, params, shape = _build(dev, name)
    x, d, add = _inputs(dev, name, rays, 7 * rays + len(name))
    ref = _ref64(dev, name, params, shape, x, d, add)
    composed = _fused(net.eval(), name, x, d, add)
    assert net.packed_weights_infer(net.desc_for_encoders(*_encoders(*NETS[name][1:3]), NETS[name][3])) is not None
    regular = _fused(net.train(), name, x, d, add)
    tol = 5 * 2e-5 * max(1.0, float(ref.abs().max()))
    e_c, e_r = float((composed.double() - ref).abs().max()), float((regular.double() - ref).abs().max())
    print(f"compose {name:22s} {tag:>14s} n={x.shape[0]:6d}: max|err| composed {e_c:.3e}  regular {e_r:.3e}  "
          f"(tolerance {tol:.3e}, max|ref| {float(ref.abs().max()):.3e})")
    assert bool(torch.isfinite(composed).all()) and e_c <= tol
    return composed, regular


@pytest.mark.parametrize("name", sorted(NETS))
@pytest.mark.parametrize("rays", [1, 131])
def test_composed_output_against_float64(dev, name, rays):
    """1 and 131 samples (nets with per-ray additional inputs: 1 and 6 rays of 24 samples - the per-ray fold - or 1 and 33 rays of 4
    - no fold) against a float64 evaluation of the uncomposed network, at the tolerance of the fused form
    (tests/test_gpu_weight_ring.py: 5 x 2e-5 max(1, max|ref|))."""
    spr = NETS[name][4]
    n_rays = rays if spr == 1 else (1 if rays == 1 else {24: 6, 4: 33}[spr])
    composed, regular = _check_against_float64(dev, name, n_rays, f"{n_rays} x {spr}")
    # (the two streams hold different roundings of the same maps: equal bits would mean the composed stream was not used)
    if rays > 1:
        assert not torch.equal(composed, regular)


def _big_n(dev):
    return 3 * torch.cuda.get_device_properties(dev).multi_processor_count * 128 + 77


@pytest.fixture(scope="module")
def big(dev):
    """One throughput-sized call of the default net: 3 x CUs x 128 + 77 samples (rays of 8 samples + a ragged tail evaluated as a
    second call is avoided: one sample per ray, so any n is whole rays) - the 67-slab stream wraps in every workgroup."""
    net, params, shape = _build(dev, "default")
    n = _big_n(dev)
    x, d, _ = _inputs(dev, "default", n, 99)
    out = _fused(net.eval(), "default", x, d, None)
    return net, params, shape, x, d, out


def test_throughput_sized_call_against_float64(dev, big):
    net, params, shape, x, d, out = big
    ref = _ref64(dev, "default", params, shape, x, d, None)
    regular = _fused(net.train(), "default", x, d, None)
    net.eval()
    tol = 5 * 2e-5 * max(1.0, float(ref.abs().max()))
    e_c, e_r = float((out.double() - ref).abs().max()), float((regular.double() - ref).abs().max())
    print(f"compose {'default':22s} {'3 CUs 128 + 77':>14s} n={x.shape[0]:6d}: max|err| composed {e_c:.3e}  regular {e_r:.3e}  "
          f"(tolerance {tol:.3e}, max|ref| {float(ref.abs().max()):.3e})")
    assert e_c <= tol
    again = _fused(net, "default", x, d, None)
    assert torch.equal(out, again)


@pytest.mark.parametrize("rays", [1, 3, 31, 513])
def test_small_calls_equal_rows_of_the_frame_sized_call(dev, big, rays):
    """rays x 8 samples (the latency-class kernels, the 64-sample tiles, and a throughput launch with a latency remainder) equal the
    same rows of the throughput-sized call bit for bit."""
    net, params, shape, x, d, out = big
    from smpl_nerf_amd.ops import PositionalEncoder
    n = rays * 8
    d_rows = d[:n]                  # (the big call has one direction per sample: per-sample directions here, the same values)
    with torch.no_grad():
        small = net.eval().forward_fused(x[:n], d_rows, 8, PositionalEncoder(10, 0), PositionalEncoder(4, 0))
    assert torch.equal(small, out[:n]), int((small != out[:n]).any(dim=1).sum())


# ------------------------------------------------------------------------------------------------ the pack
def _desc_and_flat(net, name):
    from smpl_nerf_amd.nets import flat_parameter_vector
    desc = net.desc_for_encoders(*_encoders(*NETS[name][1:3]), NETS[name][3])
    return desc, flat_parameter_vector(net._ordered_params())


def _pack_infer(lib, desc, flat):
    from smpl_nerf_amd._lib import check, current_stream, ptr
    n = int(lib.snerf_mlp_packed_infer_floats(desc))
    assert n > 0
    out = torch.full((n,), float("nan"), device=flat.device)
    check(lib.snerf_mlp_pack_infer_f32(desc, ptr(flat), ptr(out), current_stream()), "snerf_mlp_pack_infer_f32")
    return out


def _slot_cols(L, ident, nkb):
    """column of a 3-channel encoding that feeds slot (kb, g, r) (csrc/mlp_plan.h: pe_slot_col), -1 = padding"""
    out = -np.ones((nkb, 4, 4), np.int64)
    nid = 3 if ident else 0
    for kb in range(nkb):
        for g in range(4):
            for r in range(4):
                p = 4 * (2 * kb + (r >> 1)) + g
                if p < nid:
                    out[kb, g, r] = -1 if r & 1 else p
                    continue
                pp = p - nid
                if pp < 3 * L:
                    k, c = divmod(pp, 3)
                    out[kb, g, r] = nid + 6 * k + (3 if r & 1 else 0) + c
    return out


def _unpack_layer(stream, first_slab, t_out, n_out, col_of_slot):
    """[n_out, len(col_of_slot) slots] weight values and the bias of a layer of the stream (csrc/mlp_plan.h: fwd_slab_src)."""
    S = 8448
    kps = 32 // t_out
    nkb = col_of_slot.shape[0]
    W = {}
    for kb in range(nkb):
        slab = stream[(first_slab + kb // kps) * S:(first_slab + kb // kps + 1) * S]
        blk = slab[(kb % kps) * t_out * 256:(kb % kps + 1) * t_out * 256].reshape(t_out, 64, 4)     # [to][lane][r]
        for g in range(4):
            for r in range(4):
                col = col_of_slot[kb, g, r]
                vals = blk[:, 16 * g:16 * g + 16, r].reshape(-1)[:n_out]                            # rows 16 to + i
                if col >= 0:
                    W[int(col)] = vals
                else:
                    assert not vals.any()                                                           # padding slots hold zeros
    bias = stream[first_slab * S + 32 * 256:first_slab * S + 32 * 256 + n_out]
    return W, bias


@pytest.mark.parametrize("name", ["default", "w200", "nodir", "n1"])
def test_pack(dev, name):
    """Two packs are bit-equal; the trunk and rgb slabs are the regular stream's; every composed entry c is within
    2^-24 |c64| + 2^-40 sum|factors| of the numpy float64 product (the second term: the order-of-summation bound of a 256- or
    128 x 256-term float64 sum, sum|factors| = the same product of the absolute values)."""
    from smpl_nerf_amd import _lib
    lib = _lib.load()
    net, params, shape = _build(dev, name)
    kw, pos, dirs, add_first, spr = NETS[name]
    desc, flat = _desc_and_flat(net, name)
    a, b = _pack_infer(lib, desc, flat), _pack_infer(lib, desc, flat)
    torch.cuda.synchronize()
    S = 8448
    W, WD, nh = kw["width"], kw["width"] // 2, kw["n_layers"] - 1
    WK = 64 if W <= 64 else 128 if W <= 128 else 256
    T, TD = WK // 16, WK // 32
    use_dir = kw.get("use_directional_input", 1)
    pos_nkb = (2 * ((3 * pos[1] + 3 * pos[0] + 3) // 4) + 3) // 4
    dir_nkb = (2 * ((3 * dirs[1] + 3 * dirs[0] + 3) // 4) + 3) // 4 if use_dir else 0
    kps = 32 // T
    trunk = -(-pos_nkb // kps) + sum(-(-(T + (pos_nkb if i in kw["skips"] else 0)) // kps) for i in range(nh))
    n_sig, n_dn, n_dnet = 1, -(-(T + dir_nkb) // (32 // TD)), -(-TD // (32 // TD))
    total_infer, total_reg = trunk + n_sig + n_dn + 1, trunk + -(-T // kps) + n_sig + n_dn + n_dnet + 1
    stream = (total_infer + 3) * S
    assert a.numel() >= stream and torch.equal(a[:stream], b[:stream]) and bool(torch.isfinite(a[:stream]).all())
    assert not bool(a[total_infer * S:stream].any())                       # the pad slabs
    reg = net.train().packed_weights(desc)
    assert reg.numel() == (total_reg + 3) * S
    assert torch.equal(a[:trunk * S], reg[:trunk * S])                     # trunk
    assert torch.equal(a[(total_infer - 1) * S:total_infer * S], reg[(total_reg - 1) * S:total_reg * S])      # rgb head
    # composed entries against numpy float64
    P = {k: v.astype(np.float64) for k, v in params.items()}
    Wa, ba = P["additional_linear_layer.weight"], P["additional_linear_layer.bias"]
    ws, bs = P["sigma_out_layer.weight"], P["sigma_out_layer.bias"]
    Wd, bd = P["directional_input.weight"], P["directional_input.bias"]
    Wn, bn = P["directional_net.0.weight"], P["directional_net.0.bias"]
    Wd1, Wd2 = Wd[:, :W], Wd[:, W:]
    A = np.abs
    want = {"sigma'.weight": (ws @ Wa, A(ws) @ A(Wa)), "sigma'.bias": (ws @ ba + bs, A(ws) @ A(ba) + A(bs)),
            "dir-net'.weight": (np.concatenate([Wn @ Wd1 @ Wa, Wn @ Wd2], 1), np.concatenate([A(Wn) @ A(Wd1) @ A(Wa), A(Wn) @ A(Wd2)], 1)),
            "dir-net'.bias": (Wn @ (Wd1 @ ba + bd) + bn, A(Wn) @ (A(Wd1) @ A(ba) + A(bd)) + A(bn))}
    host = a[:stream].cpu().numpy()
    hidden = np.arange(T * 16).reshape(T, 4, 4)
    hidden = np.where(hidden < W, hidden, -1)
    got_w, got_b = _unpack_layer(host, trunk, 1, 1, hidden)
    got = {"sigma'.weight": np.stack([got_w[c] for c in range(W)], 1), "sigma'.bias": got_b}
    dcols = _slot_cols(dirs[0], dirs[1], dir_nkb)
    got_w, got_b = _unpack_layer(host, trunk + 1, TD, WD, np.concatenate([hidden, np.where(dcols >= 0, dcols + W, -1)], 0))
    got.update({"dir-net'.weight": np.stack([got_w[c] for c in range(Wd.shape[1])], 1), "dir-net'.bias": got_b})
    for key, (c64, mag) in want.items():
        g = got[key].astype(np.float64).reshape(c64.shape)
        bound = 2.0 ** -24 * np.abs(c64) + 2.0 ** -40 * mag
        worst = float((np.abs(g - c64) / bound).max())
        print(f"pack {name:8s} {key:16s}: max |c - c64| / bound = {worst:.3f}")
        assert worst <= 1.0, key


# ------------------------------------------------------------------------------------------------ freshness
def test_fresh_after_in_place_change_and_after_a_trainer_step(dev):
    """After an in-place parameter change announced with mark_weights_changed(), and after DataParallelTrainer.step (whose optimiser
    refreshes the regular stream in place), no-grad output equals that of a freshly built net with the same parameters."""
    from smpl_nerf_amd.ops import PositionalEncoder
    from smpl_nerf_amd.nets import RenderRayNet
    from smpl_nerf_amd.pipelines import NerfPipeline, PipelineArgs
    from smpl_nerf_amd.trainer import DataParallelTrainer
    pe, de = PositionalEncoder(10, 0), PositionalEncoder(4, 0)
    net, params, shape = _build(dev, "default")
    x, d, _ = _inputs(dev, "default", 300, 5)

    def fresh_like(m):
        f = RenderRayNet(8, 256, 60, 24, skips=[4])
        f.load_state_dict({k: v.detach().cpu().clone() for k, v in m.state_dict().items()})
        return f.to(dev).eval()

    def infer(m):
        with torch.no_grad():
            return m.forward_fused(x, d, 1, pe, de)

    net.eval()
    before = infer(net)
    with torch.no_grad():
        net.additional_linear_layer.weight.data.mul_(1.25)      # (`.data`: autograd's version counter does not see it)
        net.directional_net[0].bias.data.add_(0.5)
    net.mark_weights_changed()
    after = infer(net)
    assert not torch.equal(before, after) and torch.equal(after, infer(fresh_like(net)))
    # a training step through the one-call entry: Adam refreshes the regular streams in place
    pc, pf = syn.make_scene_nets(101)
    nets = []
    for p in (pc, pf):
        m = RenderRayNet(8, 256, 60, 24, skips=[4])
        m.load_state_dict({k: torch.from_numpy(v) for k, v in p.items()})
        nets.append(m.to(dev).train())
    pipe = NerfPipeline(nets[0], nets[1], PipelineArgs(sigma_noise_std=0.0), pe, de)
    tr = DataParallelTrainer(pipe, nets, lr=1e-2)
    data = syn.frame_batch(128, 128, seed=7)
    batch = [torch.from_numpy(a[np.arange(0, 16384, 128)]).to(dev) for a in data]
    for m in nets:
        m.eval()
    first = [infer(m) for m in nets]
    for _ in range(2):
        for m in nets:
            m.train()
        tr.step(batch)
        for m in nets:
            m.eval()
        now = [infer(m) for m in nets]
        for m, a, b in zip(nets, first, now):
            assert not torch.equal(a, b) and torch.equal(b, infer(fresh_like(m)))
        first = now


# ------------------------------------------------------------------------------------------------ the regular stream stays
_CHILD = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_infer_compose as T
dev = torch.device("cuda:0")
net, params, shape = T._build(dev, "default")
x, d, _ = T._inputs(dev, "default", 300, 5)
out = T._fused(net.eval(), "default", x, d, None)
from smpl_nerf_amd import _lib
assert _lib.load().snerf_mlp_packed_infer_floats(net.desc_for_encoders(*T._encoders((10, 0), (4, 0)), False)) == 0
np.save(sys.argv[2], out.cpu().numpy())
"""


def test_like_training_and_the_knob_keep_the_training_forwards_bits(dev, tmp_path):
    """_launch_forward(like_training=True) on a net in eval mode, and every no-grad call with SNERF_MLP_COMPOSE=0 (a child process:
    the knob is read once), return the training forward's `raw` bit for bit."""
    from smpl_nerf_amd import nets as N
    net, params, shape = _build(dev, "default")
    x, d, _ = _inputs(dev, "default", 300, 5)
    pe, de = _encoders((10, 0), (4, 0))
    desc = net.desc_for_encoders(pe, de, False)
    raw_train = net.train().forward_fused(x, d, 1, pe, de).detach()            # autograd on: the training forward
    net.eval()
    raw_like = torch.empty_like(raw_train)
    with torch.no_grad():
        N._launch_forward(net, desc, 0, x, d, 0, 1, None, raw_like, like_training=True)
        raw_plain = torch.empty_like(raw_train)
        N._launch_forward(net, desc, 0, x, d, 0, 1, None, raw_plain)
        composed = net.forward_fused(x, d, 1, pe, de)
    assert torch.equal(raw_like, raw_train)
    assert torch.equal(raw_plain, composed) and not torch.equal(composed, raw_train)
    out = str(tmp_path / "raw.npy")
    env = dict(os.environ, SNERF_MLP_COMPOSE="0")
    subprocess.run([sys.executable, "-c", _CHILD, ROOT, out], check=True, env=env, timeout=300)
    assert np.array_equal(np.load(out), raw_train.cpu().numpy())


def test_forward_rays_stays_on_the_regular_stream(dev):
    """AppendVerticesNet.forward_rays (6 rays of 8 samples, the default net) does not run on the composed inference stream, though
    the library has one for its descriptor: its no-grad output in eval() equals that in train() bit for bit - where forward_fused of
    a RenderRayNet differs between the two (the test above).  Moving it to that stream is a change of its bits, to be made on
    purpose."""
    from smpl_nerf_amd import _lib
    from smpl_nerf_amd.nets import AppendVerticesNet
    torch.manual_seed(11)
    net = AppendVerticesNet().to(dev)
    assert _lib.load().snerf_mlp_packed_infer_floats(net.desc_for_rows()) > 0
    rng = np.random.default_rng(12)
    rows = torch.from_numpy(rng.uniform(-1, 1, (6, 60)).astype(F32)).to(dev)
    d = torch.from_numpy(rng.normal(size=(6, 3)).astype(F32)).to(dev)
    with torch.no_grad():
        in_eval = net.eval().forward_rays(rows, d, 8, 48)
        in_train = net.train().forward_rays(rows, d, 8, 48)
    assert bool(torch.isfinite(in_eval).all()) and bool((in_eval != 0).any())
    assert torch.equal(in_eval, in_train)


# ------------------------------------------------------------------------------------------------ the render entries
def _render_rays_spied(pipe, batch, entry, precision_arg):
    """pipe.render_rays(batch) under no_grad, and the precision codes it passed to `entry` of the library."""
    from smpl_nerf_amd import _lib
    lib = _lib.load()
    real = getattr(lib, entry)
    seen = []

    def spy(*a):
        seen.append(a[precision_arg])
        return real(*a)
    try:
        setattr(lib, entry, spy)
        with torch.no_grad():
            out = pipe.render_rays(batch)
    finally:
        setattr(lib, entry, real)
    return out, seen


def _eval_net(dev, params, add_dim=0):
    from smpl_nerf_amd.nets import RenderRayNet
    m = RenderRayNet(8, 256, 60, 24, add_dim, skips=[4])
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    return m.to(dev).eval()


def _posed_batch(dev, stride):
    data = syn.frame_batch(128, 128, phi=5.0, theta=15.0, seed=9)
    sub = np.arange(0, 16384, stride)
    pose = torch.from_numpy(syn.human_poses()[np.arange(len(sub)) % 10].astype(F32)).to(dev)
    return [torch.from_numpy(a[sub]).to(dev) for a in data[:4]] + [pose, torch.from_numpy(data[4][sub]).to(dev)]


def _check_one_call_against_forward_calls(pipe, batch, entry, precision_arg):
    from smpl_nerf_amd import _lib
    out, seen = _render_rays_spied(pipe, batch, entry, precision_arg)
    assert seen == [_lib.FP32_INFER]
    nets = [pipe.model_coarse, pipe.model_fine]
    with torch.no_grad():
        ref = pipe._forward_calls(batch)
        for m in nets:
            m.train()
        regular = pipe._forward_calls(batch)
        for m in nets:
            m.eval()
    assert len(ref) == len(out)
    for a, b in zip(ref, out):
        assert a.shape == b.shape and torch.equal(a, b)
    assert not torch.equal(regular[0], out[0]) and float((regular[0] - out[0]).abs().max()) < 1e-4


@pytest.mark.parametrize("run_fine", [1, 0])
def test_render_rays_add_with_the_inference_streams_equals_the_per_kernel_forward(dev, run_fine):
    """AppendSmplParamsPipeline.render_rays of nets in eval mode: snerf_render_rays_add_f32 with SNERF_FP32_INFER - the per-ray fold
    table in the call's workspace together with the composed streams - against the separate calls of the no-grad forward."""
    from smpl_nerf_amd.ops import PositionalEncoder
    from smpl_nerf_amd.pipelines import AppendSmplParamsPipeline, PipelineArgs
    nets = [_eval_net(dev, syn.make_scene_net_params(seed, add_first=True, additional_input_dim=69), 69) for seed in (301, 303)]
    pipe = AppendSmplParamsPipeline(nets[0], nets[1], PipelineArgs(sigma_noise_std=0.0, human_pose_encoding=0, run_fine=run_fine),
                                    PositionalEncoder(10, 0), PositionalEncoder(4, 0), PositionalEncoder(10, 0))
    _check_one_call_against_forward_calls(pipe, _posed_batch(dev, 61), "snerf_render_rays_add_f32", 4)


def test_render_rays_smpl_with_the_inference_streams_equals_the_per_kernel_forward(dev):
    """SmplNerfPipeline.render_rays of nets in eval mode: snerf_render_rays_smpl_f32 with SNERF_FP32_INFER (the warp net on its fp32
    kernel and stream, the render nets on the composed streams, per-sample directions) against the separate calls."""
    from smpl_nerf_amd.nets import WarpFieldNet
    from smpl_nerf_amd.ops import PositionalEncoder
    from smpl_nerf_amd.pipelines import PipelineArgs, SmplNerfPipeline
    pc, pf = syn.make_scene_nets(101)
    mw = WarpFieldNet(8, 256, 60, 40)
    mw.load_state_dict({k: torch.from_numpy(v) for k, v in syn.make_warp_field_params(103, out_scale=0.3).items()})
    pipe = SmplNerfPipeline(_eval_net(dev, pc), _eval_net(dev, pf), mw.to(dev).eval(),
                            PipelineArgs(sigma_noise_std=0.0, human_pose_encoding=1, run_fine=1),
                            PositionalEncoder(10, 0), PositionalEncoder(4, 0), PositionalEncoder(10, 0))
    _check_one_call_against_forward_calls(pipe, _posed_batch(dev, 53), "snerf_render_rays_smpl_f32", 6)


@pytest.mark.parametrize("run_fine", [1, 0])
def test_render_rays_with_the_inference_streams_equals_the_per_kernel_forward(dev, run_fine):
    """NerfPipeline.render_rays of nets in eval mode (precision SNERF_FP32_INFER) returns what the five separate calls of the no-grad
    forward() return, bit for bit."""
    from smpl_nerf_amd.ops import PositionalEncoder
    from smpl_nerf_amd.pipelines import NerfPipeline, PipelineArgs
    pc, pf = syn.make_scene_nets(101)
    pipe = NerfPipeline(_eval_net(dev, pc), _eval_net(dev, pf), PipelineArgs(sigma_noise_std=0.0, run_fine=run_fine),
                        PositionalEncoder(10, 0), PositionalEncoder(4, 0))
    data = syn.frame_batch(128, 128, phi=20.0, theta=10.0, seed=3, near=1.0, far=4.0)
    batch = [torch.from_numpy(a[np.arange(0, 16384, 37)]).to(dev) for a in data]
    _check_one_call_against_forward_calls(pipe, batch, "snerf_render_rays_f32", 4)
