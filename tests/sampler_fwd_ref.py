"""What tests/test_gpu_sample_pdf_fwd.py holds sample_pdf_kernel (csrc/sampler.hip) to: the cases, their expected outputs and the
premises under which the kernel owes the oracle every bit.  CPU only; tests/test_sampler_fwd_host.py checks all of it without a GPU.

A case is (Nc, Nf, family of z, family of weights, family of u, B) with seeded inputs.  The expected outputs are
oracle.nerf_oracle's: sample_pdf_detail for the indices and the samples, fine_sampling for the merged depths and the points.
There is no tolerance anywhere: the kernel's contract is equality, and what licenses it is checked here -
  * the fp32 terms of the normalising sum and of every cdf prefix add up exactly in float64 (math.fsum agrees with numpy's sum in
    both directions and with every prefix of the cumsum), so a wavefront's tree and a sequential loop cannot round differently;
  * a literal torch restatement of the reference (utils.py:194-228 and :258-263) with its own torch.sum handed to the oracle as
    `tot` gives the oracle's indices, samples, merged depths and points bit for bit on every case without NaN or infinity.
The shapes sit on the edges of the launcher's own formulas (restated here as lds_bytes, n_in, vector_store, instance), the families
on the kernel's branches (fast merge or rank sort per ray, both sides of `denom < 1e-5`, u on a cdf entry and on either side of it,
samples on a coarse depth).  profiles/sample_pdf_fwd_cases.txt lists every case with these counts (rewrite its table with
`python tests/sampler_fwd_ref.py`; the host test compares)."""
import math
import os
import sys
from collections import namedtuple
from functools import lru_cache

import numpy as np
import torch

try:
    from oracle import nerf_oracle as O
except ImportError:                                   # run as a script from another directory
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import nerf_oracle as O

F32, F64 = np.float32, np.float64
WAVE, WAVES = 64, 4                                   # lanes of a wave (one ray); waves of a workgroup
B_DEFAULT = 9                                         # two workgroups of four rays and one ray into a third: `ray >= B` runs
EPS = F32(1e-5)

Case = namedtuple("Case", "name Nc Nf zfam wfam ufam B")
Inputs = namedtuple("Inputs", "z w u o d")             # z, w [B, Nc]; u [Nf]; o, d [B, 3]
Expected = namedtuple("Expected", "cdf inds samples z_fine pts")


# ------------------------------------------------------------------------------------------------ the launcher's formulas
def round4(n):
    """sp_round4"""
    return (n + 3) & ~3


def n_in(Nc, Nf):
    """floats of LDS a wave keeps below its output area: z [Nc], bins and cdf [Nc - 1] each, samples [Nf]"""
    return round4(Nc + 2 * (Nc - 1) + Nf)


def per_wave(Nc, Nf):
    return n_in(Nc, Nf) + round4(Nc + Nf)


def lds_bytes(Nc, Nf):
    return WAVES * per_wave(Nc, Nf) * 4


def vector_store(Nc, Nf):
    """the kernel's `vec` but for the pointers' alignment"""
    return (Nc + Nf) % 4 == 0 and n_in(Nc, Nf) >= 3 * WAVE


def instance(Nc, Nf):
    return "64+128" if (Nc, Nf) == (64, 128) else "runtime"


def raised(Nc, Nf):
    return lds_bytes(Nc, Nf) > 64 * 1024


# ------------------------------------------------------------------------------------------------ the cases
SHAPES = [(3, 1), (4, 2), (5, 5), (9, 7), (10, 8), (17, 3),         # Nb = 2, 3, 4, 8, 9, 16 in the runtime count_below; dword stores
          (65, 63), (66, 129), (67, 64), (130, 65),                 # M = 63, 64, 65, 128: the scan's carry; Nb = 64, 65
          (47, 49), (48, 48),                                       # n_in = 188 (dword) against 192 (vector); Nt = 96
          (64, 128),                                                # the compile-time instance
          (512, 1024), (513, 1024),                                 # 65 536 B (limit not raised) against 65 664 B (raised)
          (1024, 1024), (1024, 1)]                                  # 96 KiB; 65 600 B with a single sample
CROSS = [(9, 7), (66, 129), (64, 128), (513, 1024)]                 # every family runs at these
TIE_SHAPES = [(6, 5), (10, 9), (66, 65), (18, 33)]                  # plateau with M = 4, 8, 64, 16 and u = linspace: u on cdf entries
Z_FAMILIES = ("jitter", "runs", "equal", "descending", "shuffled", "special")
W_FAMILIES = ("rand4", "zero", "plateau", "spike_first", "spike_mid", "spike_last", "alternating", "ends", "tiny")
U_FAMILIES = ("linspace", "sorted01", "unsorted", "cdf_neighbours")
DENOM_FAMILIES = ("zero", "spike_first", "spike_mid", "spike_last", "alternating")
BASE = ("jitter", "rand4", "linspace")


def _name(Nc, Nf, zf, wf, uf):
    return f"{Nc}x{Nf}-{zf}-{wf}-{uf}"


def _cases():
    out = {}

    def add(Nc, Nf, zf=BASE[0], wf=BASE[1], uf=BASE[2], B=B_DEFAULT):
        c = Case(_name(Nc, Nf, zf, wf, uf), Nc, Nf, zf, wf, uf, B)
        out.setdefault(c.name, c)
    for Nc, Nf in SHAPES:
        add(Nc, Nf)
    for Nc, Nf in CROSS:
        for zf in Z_FAMILIES:
            add(Nc, Nf, zf=zf)
        for wf in W_FAMILIES:
            add(Nc, Nf, wf=wf)
        for uf in U_FAMILIES:
            add(Nc, Nf, uf=uf)
        add(Nc, Nf, zf="grid", wf="plateau", uf="cdf_neighbours")   # u on and beside entries of an exactly representable cdf
    for Nc, Nf in TIE_SHAPES:
        add(Nc, Nf, zf="grid", wf="plateau")
    add(1024, 1024, uf="unsorted")                                  # the rank sort at the largest call: 2048 elements per ray
    add(1024, 1024, zf="shuffled")
    return out


CASE = _cases()
CASES = list(CASE.values())


def _rng(c, what):
    """z, weights, o and d depend on (Nc, B) alone, so that cases of one Nc share them; u on Nf as well"""
    return np.random.default_rng([c.Nc, c.B, what] + ([c.Nf] if what == 4 else []))


def _jitter(rng, B, Nc):
    """stratified depths in [2, 6), strictly ascending"""
    t = (np.arange(Nc) + rng.uniform(0.05, 0.95, (B, Nc))) / Nc
    return (2.0 + 4.0 * t).astype(F32)


def make_z(c):
    rng, B, Nc = _rng(c, 1), c.B, c.Nc
    z = _jitter(rng, B, Nc)
    if c.zfam == "grid":                                            # 2 + i / 8: every midpoint, and every midpoint of midpoints, is exact
        z = np.broadcast_to((2.0 + np.arange(Nc) / 8.0).astype(F32), (B, Nc)).copy()
    elif c.zfam == "runs":                                          # ascending with runs of equal depths
        z = (2.0 + np.sort(rng.integers(0, max(2, Nc // 3), (B, Nc)), -1) / 8.0).astype(F32)
    elif c.zfam == "equal":
        z = np.broadcast_to((2.0 + np.arange(B)[:, None] / 4.0).astype(F32), (B, Nc)).copy()
    elif c.zfam == "descending":
        z = z[:, ::-1].copy()
    elif c.zfam == "shuffled":                                      # odd rays shuffled, even rays ascending: both merges in one workgroup
        for r in range(1, B, 2):
            z[r] = z[r][rng.permutation(Nc)]
    elif c.zfam == "special":
        z[0, Nc // 2] = np.nan                                      # ray 0: a NaN in the middle
        z[1, -1] = np.inf                                           # ray 1: the last depth infinite
    return z


def make_w(c):
    rng, B, Nc = _rng(c, 2), c.B, c.Nc
    w = np.zeros((B, Nc), F32)
    M = Nc - 2
    if c.wfam == "rand4":
        w = (rng.random((B, Nc)) ** 4).astype(F32)
    elif c.wfam == "plateau":
        w[:] = F32(0.25)
    elif c.wfam.startswith("spike"):
        w[:, 1 + {"spike_first": 0, "spike_mid": M // 2, "spike_last": M - 1}[c.wfam]] = 1
    elif c.wfam == "alternating":
        w[:, 1::2] = F32(0.5)
    elif c.wfam == "ends":                                          # all the mass where the pdf does not look
        w[:, 0] = w[:, -1] = 1
    elif c.wfam == "tiny":                                          # at and below the added 1e-5
        w = np.where(rng.random((B, Nc)) < 0.5, F32(1e-30), F32(1e-5)).astype(F32)
    assert (w >= 0).all() and (w <= 1).all()
    return w


def make_od(c):
    rng = _rng(c, 3)
    o = rng.uniform(-1, 1, (c.B, 3)).astype(F32)
    d = rng.normal(size=(c.B, 3)).astype(F32)
    if c.zfam == "special":
        d[2, 1] = 0                                                 # ray 2: a zero direction component
    return o, d


def default_tot(w):
    """the fp32 of the float64 sum of the interior weights + 1e-5: the oracle's default and the kernel's own sum [B]"""
    return np.sum((w[:, 1:-1] + EPS).astype(F32).astype(F64), -1).astype(F32)


def make_u(c, w):
    rng, Nf = _rng(c, 4), c.Nf
    if c.ufam == "linspace" or Nf == 1:
        return O.linspace01(Nf)
    if c.ufam == "sorted01":
        u = np.sort(rng.random(Nf)).astype(F32)
        u[0], u[-1] = 0, 1
        return u
    if c.ufam == "unsorted":
        u = rng.random(Nf).astype(F32)
        if Nf >= 4:
            u[1], u[Nf // 2] = 1, 0
        assert (np.diff(u) < 0).any()
        return u
    # entries of ray 0's cdf - the first, the last and others evenly between - each with its two fp32 neighbours; the rest 0.5
    cdf = O.cdf_from_weights(w[:1, 1:-1])[0]
    m = Nf // 3
    pick = np.unique(np.round(np.linspace(0, len(cdf) - 1, m)).astype(int)) if m else np.zeros(0, int)
    e = cdf[pick]
    u = np.concatenate([np.nextafter(e, F32(-np.inf)), e, np.nextafter(e, F32(np.inf)), np.full(Nf - 3 * len(e), 0.5, F32)])
    return np.sort(u).astype(F32)


@lru_cache(maxsize=None)
def inputs(name):
    """the case's inputs, made once and shared; nobody writes to them"""
    c = CASE[name]
    z, w = make_z(c), make_w(c)
    o, d = make_od(c)
    out = Inputs(z, w, make_u(c, w), o, d)
    assert out.z.shape == out.w.shape == (c.B, c.Nc) and out.u.shape == (c.Nf,) and out.o.shape == out.d.shape == (c.B, 3)
    assert all(a.dtype == F32 for a in out)
    return out


def bins_of(z):
    """utils.py:258"""
    return (F32(0.5) * (z[:, 1:] + z[:, :-1])).astype(F32)


def strict_tot(w):
    """a `tot` one unit in the last place off the default on two rays of three: up on rays 0, 3, ..., down on rays 1, 4, ..."""
    tot = default_tot(w)
    tot[0::3] = np.nextafter(tot[0::3], F32(np.inf))
    tot[1::3] = np.nextafter(tot[1::3], F32(0))
    return tot


def oracle(x, tot=None):
    """Expected(cdf, inds, samples, z_fine, pts) of inputs x from oracle.nerf_oracle, `tot` [B] or the oracle's default"""
    t = None if tot is None else np.asarray(tot, F32)[:, None]
    with np.errstate(invalid="ignore"):
        det = O.sample_pdf_detail(bins_of(x.z), x.w[:, 1:-1], len(x.u), u=x.u, tot=t)
        z_fine, pts = O.fine_sampling(x.o, x.d, x.z, x.w, len(x.u), u=x.u, tot=t)
    out = Expected(det["cdf"], det["inds"], det["samples"], z_fine, pts)
    for a in out:
        a.setflags(write=False)
    return out


@lru_cache(maxsize=None)
def expected(name, strict=False):
    x = inputs(name)
    return oracle(x, strict_tot(x.w) if strict else None)


def has_specials(x):
    return not np.isfinite(x.z).all()


# ------------------------------------------------------------------------------------------------ the reference, literally
def torch_reference(x):
    """utils.py:194-228 and :258-263 on the CPU with torch's own kernels (torch.searchsorted for the torchsearchsorted extension),
    the case's u in place of torch.linspace.  Returns (tot [B], inds, samples, z_fine, pts) as numpy; tot is torch.sum's."""
    z, w, u1, o, d = (torch.from_numpy(np.array(a)) for a in x)
    nf = len(u1)
    bins = .5 * (z[..., 1:] + z[..., :-1])                                                    # :258
    weights = w[..., 1:-1] + 1e-5                                                             # :200
    tot = torch.sum(weights, -1, keepdim=True)
    pdf = weights / tot                                                                       # :201
    cdf = torch.cumsum(pdf, -1)                                                               # :202
    cdf = torch.cat([torch.zeros_like(cdf[..., :1]), cdf], -1)                                # :203
    u = u1.expand(list(cdf.shape[:-1]) + [nf]).contiguous()                                   # :206-210
    inds = torch.searchsorted(cdf.contiguous(), u, right=True)                                # :212
    below = torch.max(torch.zeros_like(inds - 1), inds - 1)                                   # :213
    above = torch.min((cdf.shape[-1] - 1) * torch.ones_like(inds), inds)                      # :214
    g = torch.stack([below, above], -1)                                                       # :215
    shape = [g.shape[0], g.shape[1], cdf.shape[-1]]
    cdf_g = torch.gather(cdf.unsqueeze(1).expand(shape), 2, g)                                # :219-221
    bins_g = torch.gather(bins.unsqueeze(1).expand(shape), 2, g)
    denom = cdf_g[..., 1] - cdf_g[..., 0]                                                     # :223
    denom = torch.where(denom < 1e-5, torch.ones_like(denom), denom)                          # :224
    t = (u - cdf_g[..., 0]) / denom                                                           # :225
    samples = bins_g[..., 0] + t * (bins_g[..., 1] - bins_g[..., 0])                          # :226
    z_fine, _ = torch.sort(torch.cat([z, samples], -1), -1)                                   # :261
    pts = o[..., None, :] + d[..., None, :] * z_fine[..., :, None]                            # :262-263
    return tot[:, 0].numpy(), inds.numpy(), samples.numpy(), z_fine.numpy(), pts.numpy()


# ------------------------------------------------------------------------------------------------ the premises
@lru_cache(maxsize=None)
def sums_are_order_free(wfam, Nc, B):
    """For every ray of the weights of family `wfam` at [B, Nc]: math.fsum of the fp32 terms w + 1e-5 equals numpy's float64 sum forwards and reversed,
    and every float64 prefix of the cumsum of the fp32 pdf equals math.fsum of that prefix - with the default `tot` and with
    strict_tot.  Returns the number of prefixes checked."""
    w = make_w(Case("", Nc, 0, "", wfam, "", B))
    name = f"{wfam} [{B}, {Nc}]"
    terms = (w[:, 1:-1] + EPS).astype(F32).astype(F64)
    checked = 0
    for r in range(len(w)):
        exact = math.fsum(terms[r])
        assert exact == float(np.sum(terms[r])) == float(np.sum(terms[r][::-1])), (name, r)
    for tot in (default_tot(w), strict_tot(w)):
        pdf = ((w[:, 1:-1] + EPS).astype(F32) / tot[:, None]).astype(F32).astype(F64)
        cum = np.cumsum(pdf, -1)
        for r in range(len(w)):
            row = pdf[r].tolist()
            for k in range(len(row)):
                assert math.fsum(row[:k + 1]) == cum[r, k], (name, r, k)
            checked += len(row)
    return checked


def ray_paths(x, e):
    """per ray: does the wave take the fast merge?  sorted_in && sorted_s as the kernel forms them (a NaN compares false)"""
    with np.errstate(invalid="ignore"):
        sorted_in = (x.z[:, :-1] <= x.z[:, 1:]).all(-1)
        sorted_s = (e.samples[:, :-1] <= e.samples[:, 1:]).all(-1)
    return sorted_in & sorted_s


def counts(name):
    """what the case reaches, with the oracle's default `tot`"""
    c, x, e = CASE[name], inputs(name), expected(name)
    Nb = c.Nc - 1
    below, above = np.maximum(0, e.inds - 1), np.minimum(Nb - 1, e.inds)
    denom = (np.take_along_axis(e.cdf, above, -1) - np.take_along_axis(e.cdf, below, -1)).astype(F32)
    fast = ray_paths(x, e)
    groups = [fast[g:g + WAVES] for g in range(0, c.B, WAVES)]
    with np.errstate(invalid="ignore"):
        on_coarse = int((e.samples[:, :, None] == x.z[:, None, :]).any(-1).sum())
        on_bin = int((e.samples[:, :, None] == bins_of(x.z)[:, None, :]).any(-1).sum())
    u = np.broadcast_to(x.u, e.inds.shape)
    return dict(cdf_ties=int((u[:, :, None] == e.cdf[:, None, :]).any(-1).sum()), cdf_ties_ray0=int(np.isin(x.u, e.cdf[0]).sum()),
                on_coarse=on_coarse, on_bin=on_bin, denom_small=int((denom < EPS).sum()), denom_large=int((denom >= EPS).sum()),
                ind_zero=int((e.inds == 0).sum()), ind_nb=int((e.inds == Nb).sum()), fallback_rays=int((~fast).sum()),
                mixed_groups=sum(1 for g in groups if g.any() and not g.all()), nan_out=int(np.isnan(e.z_fine).sum()))


def describe(name):
    """one line for profiles/sample_pdf_fwd_cases.txt and for the GPU test's printout"""
    c, k = CASE[name], counts(name)
    lds = lds_bytes(c.Nc, c.Nf)
    return (f"{name:<44} B {c.B} lds {lds:>6}{'^' if raised(c.Nc, c.Nf) else ' '} n_in {n_in(c.Nc, c.Nf):>4} "
            f"{'vector' if vector_store(c.Nc, c.Nf) else 'dword '} {instance(c.Nc, c.Nf):<7} ties cdf {k['cdf_ties']:>4} coarse {k['on_coarse']:>5} "
            f"bin {k['on_bin']:>5} denom<1e-5 {k['denom_small']:>4} >= {k['denom_large']:>4} ind=0 {k['ind_zero']:>3} ind=Nb {k['ind_nb']:>4} "
            f"fallback rays {k['fallback_rays']}/{c.B} mixed groups {k['mixed_groups']} NaN out {k['nan_out']}")


# ------------------------------------------------------------------------------------------------ the record
PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "sample_pdf_fwd_cases.txt")
RUN_MARK = "# ---- a run of tests/test_gpu_sample_pdf_fwd.py on an MI355X"


def profile_text():
    out = ["# tests/sampler_fwd_ref.py: the cases of tests/test_gpu_sample_pdf_fwd.py (rewrite this table with `python tests/sampler_fwd_ref.py`;",
           "# tests/test_sampler_fwd_host.py compares).  lds: bytes of LDS per workgroup, ^ where the launch raises the 64 KiB limit; n_in: floats",
           "# below a wave's output area (vector stores from 192 where Nc + Nf is a multiple of 4); ties: (ray, u) pairs on a cdf entry, samples",
           "# equal to a coarse depth / to a bin; denom: gathered pairs on either side of 1e-5; fallback rays: waves that take the rank sort;",
           "# mixed groups: workgroups with both merges.  All with the oracle's default normalising sum.", ""]
    out += [describe(c.name) for c in CASES]
    return "\n".join(out) + "\n"


def stable_part(text):
    return text.split(RUN_MARK)[0].rstrip("\n") + "\n"


if __name__ == "__main__":
    rest = ""
    if os.path.exists(PROFILE):
        with open(PROFILE) as f:
            old = f.read()
        if RUN_MARK in old:
            rest = "\n" + RUN_MARK + old.split(RUN_MARK, 1)[1]
    with open(PROFILE, "w") as f:
        f.write(profile_text() + rest)
    print("wrote", PROFILE)
