"""snerf_adam_step_f32 (csrc/train_step.hip: adam_scalars_kernel, adam_kernel, the slot-table scatter into the weight streams and the
re-pack of split-precision streams) held to tests/adam_ref.py bit for bit, through ctypes, at its edges.

What each family of cases pins (tests/adam_ref.py: CASES; tests/test_adam_host.py and profiles/adam_exact_cases.txt show on the CPU which
wrong variant of the statements each case tells from the right one):
  * defaults, defaults_wd, betas_near_1, beta1_0, beta2_0, lr0 - the five statements themselves: the three fused multiply-adds (one
    rounding each), sqrt(v) / sqrt(bc2) + eps in that order, weight decay on the gradient in front of the moments, the constants as
    fp32 conversions of float64 values;
  * tiny_and_huge, eps0 - nothing flushed and nothing clamped: subnormal and zero exp_avg_sq through the root, 0 / 0 = NaN at exactly
    the places where it arises, +-inf where a root underflowed;
  * boundaries, many_ranges, skipped - the index arithmetic: a one-element range, boundaries that are no multiple of 256, an empty
    range, parameters that belong to no range, 32 ranges with their own step counts (an element reading its neighbour's scalars
    shows), 1 / 64 / 65 / 130 step counters per range, t = 100001 where beta^t underflows, a range left out of two calls;
  * every case: the two scalars of every range in the scratch buffer, as fp32 bits, against 120-digit arithmetic.
Every array is cut out of a larger buffer filled with a marker; the bands around it, every element outside the call's ranges, the
scratch floats behind the call's ranges and the counters of ranges left out must keep their bits.

test_streams_follow_the_update holds the scatter: after every call each weight stream equals, byte for byte and padding included, a
fresh pack of the new parameters into a buffer that started with the same contents - nets with both streams, one stream, no range,
part of a range, two ranges, the maximum of eight nets, and the split-precision formats, which the entry re-packs.

Still held by tolerance only: the parameters against torch.optim.Adam itself (tests/test_adam_host.py on the CPU and
test_hip_adam_follows_torch_adam in tests/test_gpu_round4.py; torch's CPU sqrt is not correctly rounded).  Not held here:
mse_grad_kernel, snerf_warp_repack_f32 and the data-parallel average in front of the update (the one-call-step tests)."""
import ctypes

import numpy as np
import pytest
import torch

import adam_ref as A

pytestmark = pytest.mark.gpu
IDS = lambda c: c.name
F32 = np.float32
BADARG = -1                     # SNERF_E_BADARG
GUARD = 64                      # elements in front of and behind every array
MARK = {np.dtype(np.float32): np.array([0x7fc5a5a5], np.uint32).view(F32)[0], np.dtype(np.int64): np.int64(-0x5a5a5a5a5a5a5a5a),
        np.dtype(np.uint8): np.uint8(0xa5)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from smpl_nerf_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _raw(a):
    """an array as unsigned integers of its width (NaN payloads and signed zeros count)"""
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


class Guarded:
    """a device array cut out of a larger buffer filled with a marker"""

    def __init__(self, dev, host):
        host = np.ascontiguousarray(host)
        self.n, self.dtype = host.size, host.dtype
        full = np.full(self.n + 2 * GUARD, MARK[host.dtype], host.dtype)
        full[GUARD:GUARD + self.n] = host.ravel()
        self.t = torch.from_numpy(full).to(dev)
        self.ptr = self.t.data_ptr() + GUARD * host.dtype.itemsize

    @classmethod
    def marked(cls, dev, n, dtype):
        return cls(dev, np.full(n, MARK[np.dtype(dtype)], dtype))

    def upload(self, host):
        self.t[GUARD:GUARD + self.n].copy_(torch.from_numpy(np.ascontiguousarray(host, self.dtype).ravel()))

    def read(self):
        return self.t.cpu().numpy()[GUARD:GUARD + self.n]

    def everything(self):
        return _raw(self.t.cpu().numpy())

    def guards_intact(self):
        full = _raw(self.t.cpu().numpy())
        mark = _raw(np.array([MARK[self.dtype]], self.dtype))[0]
        return bool((full[:GUARD] == mark).all() and (full[GUARD + self.n:] == mark).all())


# ------------------------------------------------------------------------------------------------ a case on the device
class Device:
    """the buffers of a case: params, grads, both moments, the step counters (each range's own, three marked int64 between two
    ranges) and the 64 scratch floats, all guarded"""

    def __init__(self, dev, case):
        self.case = case
        self.p = Guarded(dev, A.initial_params(case))
        self.g = Guarded.marked(dev, case.n, F32)
        self.m = Guarded(dev, np.zeros(case.n, F32))
        self.v = Guarded(dev, np.zeros(case.n, F32))
        self.scratch = Guarded.marked(dev, 2 * A.MAX_RANGES, F32)
        self.at, steps = [], []
        for r in case.ranges:
            steps += [MARK[np.dtype(np.int64)]] * 3
            self.at.append(len(steps))
            steps += [r.preset] * r.n_steps
        self.steps = Guarded(dev, np.array(steps, np.int64))
        self.want_scratch = np.full(2 * A.MAX_RANGES, MARK[np.dtype(F32)], F32)      # (a call writes two floats per range of ITS ranges)
        self.buffers = {"params": self.p, "grads": self.g, "exp_avg": self.m, "exp_avg_sq": self.v, "steps": self.steps,
                        "scratch": self.scratch}

    def state(self):
        from smpl_nerf_amd import _lib
        h = self.case.hyper
        return _lib.AdamState(self.p.ptr, self.g.ptr, self.m.ptr, self.v.ptr, self.case.n, self.scratch.ptr, h.lr, h.beta1, h.beta2,
                              h.eps, h.wd)

    def c_ranges(self, act):
        from smpl_nerf_amd import _lib
        arr = (_lib.AdamRange * max(len(act), 1))()
        for j, i in enumerate(act):
            r = self.case.ranges[i]
            arr[j] = _lib.AdamRange(r.begin, r.end, self.steps.ptr + 8 * self.at[i], r.n_steps)
        return arr

    def load_gradients(self, k):
        """the gradients of call k; NaN at every element the call must not read"""
        g = A.gradients(self.case, k)
        on = np.zeros(self.case.n, bool)
        for i in A.active_ranges(self.case, k):
            on[self.case.ranges[i].begin:self.case.ranges[i].end] = True
        self.g.upload(np.where(on, g, F32(np.nan)))

    def call(self, k, nets=None, n_nets=0):
        from smpl_nerf_amd import _lib
        act = A.active_ranges(self.case, k)
        st = self.state()
        _lib.check(_lib.load().snerf_adam_step_f32(ctypes.byref(st), self.c_ranges(act), len(act), nets, n_nets, _stream()),
                   f"snerf_adam_step_f32 ({self.case.name}, call {k})")

    def hold(self, k, ref):
        """the state after call k against row k + 1 of the restatement: no tolerance"""
        case, act = self.case, A.active_ranges(self.case, k)
        torch.cuda.synchronize()
        for name, buf, want in (("exp_avg_sq", self.v, ref.exp_avg_sq), ("exp_avg", self.m, ref.exp_avg), ("params", self.p, ref.params)):
            A.assert_same_bits(case, f"{name} after call {k}", buf.read(), want[k + 1])
        steps = self.steps.read()
        for i, r in enumerate(case.ranges):
            got = steps[self.at[i]:self.at[i] + r.n_steps]
            assert (got == ref.steps[k + 1][i]).all(), f"{case.name}: counters of range {i} after call {k}: {got[:4]} .., want {ref.steps[k + 1][i]}"
            assert (steps[self.at[i] - 3:self.at[i]] == MARK[np.dtype(np.int64)]).all(), f"{case.name}: the int64 in front of range {i}'s counters"
        scal = self.scratch.read()
        want = self.want_scratch
        for j, i in enumerate(act):
            want[2 * j], want[2 * j + 1] = ref.scal[k][i]
        bad = np.flatnonzero(_raw(scal) != _raw(want))
        assert not bad.size, (f"{case.name}: scratch after call {k}: float {bad[0]} (range {act[bad[0] // 2] if bad[0] // 2 < len(act) else None} "
                              f"of the call, {'neg_step' if bad[0] % 2 == 0 else 'bc2_sqrt'}): got {scal[bad[0]]!r}, want {want[bad[0]]!r}")
        for name, buf in self.buffers.items():
            assert buf.guards_intact(), f"{case.name}: the bands around {name} after call {k}"

    def everything(self):
        torch.cuda.synchronize()
        return {name: buf.everything() for name, buf in self.buffers.items()}


def _line(case, ref):
    v, tiny = ref.exp_avg_sq[1:], float(np.finfo(F32).tiny)
    calls = sum(len(A.active_ranges(case, k)) for k in range(case.iters))
    return (f"adam-exact {case.name:<14} n {case.n:<5} ranges {len(case.ranges):<2} calls {case.iters} (range updates {calls:<3}) t up to "
            f"{int(ref.steps.max()):<6} exp_avg_sq zero {int((v == 0).sum()):<5} subnormal {int(((v != 0) & (v < tiny)).sum()):<5} max {float(v.max()):.3g}  "
            f"params NaN {int(np.isnan(ref.params[-1]).sum())} inf {int(np.isinf(ref.params[-1]).sum())}")


@pytest.mark.parametrize("case", A.CASES, ids=IDS)
def test_every_case_is_the_restatement_bit_for_bit(dev, case):
    ref = A.run(case)
    print("\n" + _line(case, ref))
    d = Device(dev, case)
    for k in range(case.iters):
        d.load_gradients(k)
        d.call(k)
        d.hold(k, ref)


def test_two_runs_give_the_same_bits(dev):
    for case in (A.CASE["tiny_and_huge"], A.CASE["many_ranges"]):
        runs = []
        for _ in range(2):
            d = Device(dev, case)
            for k in range(case.iters):
                d.load_gradients(k)
                d.call(k)
            runs.append(d.everything())
        for name in runs[0]:
            assert np.array_equal(runs[0][name], runs[1][name]), (case.name, name)


GRAPH_CASE = A.make_case("graph", 1500, [(2, 700, 3, 0), (700, 1490, 2, 0)], A.DEFAULT._replace(wd=0.01), iters=3)


def test_replay_from_a_captured_graph(dev):
    """One linear capture of the entry on one stream (no branches); the step counters and the bias corrections live on the device,
    so three replays, with the gradients changed in place between them, are three eager calls."""
    case = GRAPH_CASE
    ref = A.run(case)
    eager = Device(dev, case)
    for k in range(case.iters):                        # (also loads the kernels before anything is captured)
        eager.load_gradients(k)
        eager.call(k)
        eager.hold(k, ref)
    d = Device(dev, case)
    d.load_gradients(0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        d.call(0)
    before = d.everything()
    assert (d.steps.read()[d.at[0]:d.at[0] + 3] == 0).all() and np.array_equal(before["params"], Device(dev, case).everything()["params"])
    for k in range(case.iters):
        d.load_gradients(k)
        graph.replay()
        d.hold(k, ref)
    want, got = eager.everything(), d.everything()
    for name in want:
        assert np.array_equal(want[name], got[name]), name
    steps = d.steps.read()
    assert all((steps[d.at[i]:d.at[i] + r.n_steps] == 3).all() for i, r in enumerate(case.ranges))


# ------------------------------------------------------------------------------------------------ the weight streams
def _desc(kind):
    from smpl_nerf_amd import _lib
    if kind == "w64":         # 2 layers of width 64
        return _lib.MlpDesc(2, 64, 4, 1, 2, 1, 0, 0, 1, 0)
    if kind == "w100":        # 4 layers of width 100, a skip connection into positional_net[1]
        return _lib.MlpDesc(4, 100, 5, 1, 2, 0, 0, 2, 1, 0)
    assert kind == "w256"     # the split-precision kernels exist for width 256
    return _lib.MlpDesc(2, 256, 4, 1, 2, 1, 0, 0, 1, 0)


class Net:
    """a net inside the flat buffer with the streams the update keeps current"""

    def __init__(self, dev, kind, streams, precision, offset):
        from smpl_nerf_amd import _lib
        lib = _lib.load()
        self.desc, self.precision, self.offset, self.streams = _desc(kind), precision, offset, streams
        self.n = int(lib.snerf_mlp_param_floats(self.desc))
        assert self.n > 0
        if precision == 0:
            nt = ctypes.c_int64()
            _lib.check(lib.snerf_mlp_train_sizes(self.desc, 0, None, None, ctypes.byref(nt), None, None), "sizes")
            self.sizes = {"fwd": (int(lib.snerf_mlp_packed_floats(self.desc)), F32), "t": (nt.value, F32)}
        else:
            self.sizes = {"fwd": (int(lib.snerf_mlp_packed_bf16_bytes(self.desc, precision)), np.uint8),
                          "t": (int(lib.snerf_mlp_packed_t_bf16_bytes(self.desc, precision, 0)), np.uint8)}
        assert all(s[0] > 0 for s in self.sizes.values())
        self.live = {w: Guarded.marked(dev, *self.sizes[w]) for w in self.which()}
        self.slots = {}
        if precision == 0:
            self.slots = {w: torch.empty(self.n, dtype=torch.int32, device=dev) for w in self.which()}
            _lib.check(lib.snerf_mlp_stream_slots(self.desc, _lib.ptr(self.slots.get("fwd")), _lib.ptr(self.slots.get("t")), 0, _stream()), "slots")

    def which(self):
        return {"both": ("fwd", "t"), "fwd": ("fwd",), "t": ("t",)}[self.streams]

    def pack(self, params_ptr, into):
        """the library's own pack of the parameters at params_ptr into the guarded buffers `into`"""
        from smpl_nerf_amd import _lib
        lib, src = _lib.load(), params_ptr + 4 * self.offset
        for w, buf in into.items():
            if self.precision == 0:
                rc = lib.snerf_mlp_pack_f32(self.desc, src, buf.ptr, _stream()) if w == "fwd" else lib.snerf_mlp_pack_t_f32(self.desc, src, buf.ptr, 0, _stream())
            elif w == "fwd":
                rc = lib.snerf_mlp_pack_bf16(self.desc, src, buf.ptr, self.precision, _stream())
            else:
                rc = lib.snerf_mlp_pack_t_bf16(self.desc, src, buf.ptr, self.precision, 0, _stream())
            _lib.check(rc, f"pack {w}")

    def c_net(self):
        from smpl_nerf_amd import _lib
        ptr = lambda d, w: d[w].ptr if w in d else None
        return _lib.AdamNet(ctypes.pointer(self.desc), self.offset, self.precision, ptr(self.live, "fwd"), ptr(self.live, "t"),
                            _lib.ptr(self.slots.get("fwd")), _lib.ptr(self.slots.get("t")))


# (kind, streams, how the ranges cover it): full - inside one range that goes on into the parameters around it; part - a range ends
# inside it; none - no range; two - two ranges with different step counts meet inside it at an odd index
FIVE = [("w64", "both", "full"), ("w100", "fwd", "part"), ("w64", "t", "full"), ("w100", "both", "none"), ("w64", "both", "two")]
EIGHT = FIVE + [("w64", "fwd", "two"), ("w64", "both", "full"), ("w100", "t", "two")]
LAYOUTS = {"fp32-five-nets": (FIVE, 0), "fp32-eight-nets": (EIGHT, 0),
           "bf16x3": ([("w256", "both", "two"), ("w256", "fwd", "part")], 2), "bf16x6": ([("w256", "both", "two"), ("w256", "t", "part")], 3),
           "f16x3": ([("w256", "both", "two"), ("w256", "both", "none")], 16)}


def _lay_out(dev, layout, precision):
    """nets at odd offsets with parameters of no net between them, and the ranges that cover them as the layout says"""
    nets, ranges, at = [], [], 5
    for j, (kind, streams, cover) in enumerate(layout):
        net = Net(dev, kind, streams, precision, at)
        nets.append(net)
        a, b = at, at + net.n
        if cover == "full":
            ranges.append((a - 2, b + 1, 1 + j, 10 * j))
        elif cover == "part":
            ranges.append((a - 1, a + (6 * net.n) // 10 + 1, 2, 3))
        elif cover == "two":
            mid = a + net.n // 2 + 1 - (a + net.n // 2) % 2       # odd
            ranges += [(a, mid, 1, 3 + j), (mid, b, 65, 40 + j)]
        at = b + 3 + 2 * j
    return nets, A.make_case(f"streams-p{precision}-{len(layout)}", at + 4, ranges, A.DEFAULT._replace(wd=0.01), iters=3)


@pytest.mark.parametrize("name", LAYOUTS)
def test_streams_follow_the_update(dev, name):
    from smpl_nerf_amd import _lib
    layout, precision = LAYOUTS[name]
    assert len(layout) <= A.MAX_NETS
    nets, case = _lay_out(dev, layout, precision)
    ref = A.run(case)
    print(f"\nadam-streams {name:<16} n {case.n} nets {len(nets)} ranges {len(case.ranges)} " +
          " ".join(f"{k}/{s}/{c}@{n.offset}+{n.n}" for (k, s, c), n in zip(layout, nets)))
    d = Device(dev, case)
    for net in nets:
        net.pack(d.p.ptr, net.live)
    c_nets = (_lib.AdamNet * len(nets))(*[net.c_net() for net in nets])
    torch.cuda.synchronize()
    start = {(j, w): buf.everything() for j, net in enumerate(nets) for w, buf in net.live.items()}
    for k in range(case.iters):
        d.load_gradients(k)
        d.call(k, c_nets, len(nets))
        d.hold(k, ref)
        for j, (net, (kind, streams, cover)) in enumerate(zip(nets, layout)):
            fresh = {w: Guarded.marked(dev, *net.sizes[w]) for w in net.which()}
            net.pack(d.p.ptr, fresh)
            torch.cuda.synchronize()
            for w in net.which():
                got, want = net.live[w].everything(), fresh[w].everything()
                bad = np.flatnonzero(got != want)
                assert not bad.size, (f"{name}: net {j} ({kind}, {cover}), stream {w} after call {k}: {bad.size} of {want.size} elements differ from a "
                                      f"fresh pack, first at {bad[0] - GUARD}: got 0x{int(got[bad[0]]):x}, want 0x{int(want[bad[0]]):x}")
                assert net.live[w].guards_intact()
                if cover == "none":
                    assert np.array_equal(got, start[(j, w)]), f"{name}: net {j} has no range, yet stream {w} changed"
                else:
                    assert not np.array_equal(got, start[(j, w)]), f"{name}: net {j}: stream {w} did not follow"


# ------------------------------------------------------------------------------------------------ refusals
REFUSAL_N = 15000
REFUSAL_CASE = A.make_case("refusals", REFUSAL_N, [(0, 300, 2, 0), (300, REFUSAL_N - 10, 1, 4)], iters=1)
NAN = float("nan")


def _set(**kw):
    def change(c):
        for k, v in kw.items():
            setattr(c["st"], k, v)
    return change


def _range1(**kw):
    def change(c):
        for k, v in kw.items():
            setattr(c["ranges"][1], k, v)
    return change


def _net0(**kw):
    def change(c):
        for k, v in kw.items():
            setattr(c["nets"][0], k, v)
    return change


def _args(**kw):
    return lambda c: c.update(kw)


STATE, COUNTS, ARRAYS = b"null pointer in the optimiser state", b"at most 32 ranges, 8 nets", b"null range / net array"
RANGE1, HYPER = b"range 1: outside the parameter buffer, or no step counters", b"invalid hyper-parameters"
REFUSALS = [("null-state", _args(st=None), STATE)] + [(f"null-{f}", _set(**{f: None}), STATE) for f in ("params", "grads", "exp_avg", "exp_avg_sq", "scratch")] + [
    ("negative-n_params", _set(n_params=-1), COUNTS), ("33-ranges", _args(n_ranges=33), COUNTS), ("negative-n_ranges", _args(n_ranges=-1), COUNTS),
    ("9-nets", _args(n_nets=9), COUNTS), ("negative-n_nets", _args(n_nets=-1), COUNTS),
    ("null-ranges", _args(ranges=None), ARRAYS), ("null-nets", _args(nets=None), ARRAYS),
    ("begin-negative", _range1(begin=-1), RANGE1), ("end-past-n_params", _range1(end=REFUSAL_N + 1), RANGE1), ("begin-past-end", _range1(begin=REFUSAL_N - 9), RANGE1),
    ("null-step", _range1(step=None), RANGE1), ("n_steps-0", _range1(n_steps=0), RANGE1),
    ("lr-negative", _set(lr=-1e-3), HYPER), ("lr-nan", _set(lr=NAN), HYPER), ("eps-negative", _set(eps=-1e-8), HYPER), ("eps-nan", _set(eps=NAN), HYPER),
    ("wd-negative", _set(weight_decay=-0.01), HYPER), ("wd-nan", _set(weight_decay=NAN), HYPER),
    ("beta1-1", _set(beta1=1.0), HYPER), ("beta1-negative", _set(beta1=-0.1), HYPER), ("beta2-1", _set(beta2=1.0), HYPER),
    ("beta2-negative", _set(beta2=-0.1), HYPER), ("beta2-nan", _set(beta2=NAN), HYPER),
    ("precision-1", _net0(precision=1), b"net 0: bad precision code"),
    ("net-past-the-buffer", _net0(param_offset=REFUSAL_N - 100), b"net 0 does not lie inside the flat parameter buffer"),
    ("net-before-the-buffer", _net0(param_offset=-1), b"net 0 does not lie inside the flat parameter buffer"),
    ("null-desc", _net0(desc=None), b"adam_step: net 0: desc is null"),
    ("packed-without-slots", _net0(slot_fwd=None), b"net 0: an fp32 stream needs its slot table"),
    ("packed_t-without-slots", _net0(slot_t=None), b"net 0: an fp32 stream needs its slot table")]


@pytest.fixture(scope="module")
def refusal_setup(dev):
    d = Device(dev, REFUSAL_CASE)
    d.load_gradients(0)
    net = Net(dev, "w64", "both", 0, 40)
    assert net.offset + net.n < REFUSAL_CASE.n - 100
    net.pack(d.p.ptr, net.live)
    torch.cuda.synchronize()
    return d, net


def _refusal_call(d, net, change):
    from smpl_nerf_amd import _lib
    lib = _lib.load()
    ranges = (_lib.AdamRange * 33)()                   # (33 valid entries: the entry must refuse by the count alone)
    for j in range(33):
        ranges[j] = d.c_ranges([0, 1])[j % 2]
    nets = (_lib.AdamNet * 9)(*[net.c_net() for _ in range(9)])
    c = {"st": d.state(), "ranges": ranges, "n_ranges": 2, "nets": nets, "n_nets": 1}
    change(c)
    before = d.everything()
    before.update({w: buf.everything() for w, buf in net.live.items()})
    with _lib.profile() as prof:
        rc = lib.snerf_adam_step_f32(None if c["st"] is None else ctypes.byref(c["st"]), c["ranges"], c["n_ranges"], c["nets"], c["n_nets"], _stream())
    after = d.everything()
    after.update({w: buf.everything() for w, buf in net.live.items()})
    return rc, lib.snerf_last_error_string(), prof.records, before, after


@pytest.mark.parametrize("what,change,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_return_before_any_launch(refusal_setup, what, change, message):
    """SNERF_E_BADARG with the entry's message, and nothing ran: the first launch of the entry writes the call's scalars into the scratch
    buffer and the step counters, the second the three arrays, the scatter the streams - all of them, bands included, keep their bits
    (the profile of the Python layer, which sees the launches made through it, stays empty as well)."""
    d, net = refusal_setup
    rc, msg, records, before, after = _refusal_call(d, net, change)
    assert rc == BADARG and message in msg, (what, rc, msg)
    assert records == []
    for name in before:
        assert np.array_equal(before[name], after[name]), f"{what}: {name} changed"


def test_no_ranges_is_ok_and_writes_nothing(refusal_setup):
    d, net = refusal_setup
    rc, _, records, before, after = _refusal_call(d, net, lambda c: c.update(n_ranges=0))
    assert rc == 0 and records == []
    for name in before:
        assert np.array_equal(before[name], after[name]), name
    rc, _, _, before, after = _refusal_call(d, net, lambda c: c.update(n_ranges=0, ranges=None, n_nets=0, nets=None))
    assert rc == 0 and all(np.array_equal(before[name], after[name]) for name in before)


def test_the_refusal_setup_is_accepted_as_it_stands(refusal_setup):
    """(last: the one call of this group that runs) the unchanged arguments pass every check, so each refusal above is the work of
    its one change"""
    d, net = refusal_setup
    rc, msg, _, before, after = _refusal_call(d, net, lambda c: None)
    assert rc == 0, msg
    d.hold(0, A.run(REFUSAL_CASE))
    assert not np.array_equal(before["fwd"], after["fwd"]) and not np.array_equal(before["t"], after["t"])
