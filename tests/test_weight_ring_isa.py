"""The weight ring of the LDS-DMA slab pipe (csrc/mlp_device.h: SlabPipeDma) must stay in flight across the slab barrier: what
hipcc makes of it is checked on the gfx950 assembly of csrc/mlp.hip (CPU only: hipcc cross-compiles; skipped without hipcc).

What went wrong before, and what these tests pin: with the DMA issued through the builtin, every `__syncthreads()` of the slab
loop was compiled to `s_waitcnt vmcnt(0)` + `s_barrier` - the counted `vmcnt(PPW)` in front of it was dead and a slab had half a
period to land, not two.  With a raw barrier and the builtin, every LDS-read wait degraded to `lgkmcnt(0)`.  Now the DMA, the
counted wait and the barrier are inline asm (the comment of SlabPipeDma has the safety argument in counts)."""
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from smpl_nerf_amd import build as B

HEADLINE = "_ZN5snerf14mlp_fwd_kernelILi256ELi8ELb0ELb0EEEvNS_7FwdArgsE"     # snerf::mlp_fwd_kernel<256, 8, false, false>
PPW = 4     # 1 KiB pieces of a slab's A region per wave of the 8-wave kernel (32 / 8); wave 0 moves the aux block as well


@pytest.fixture(scope="module")
def asms(tmp_path_factory):
    """gfx950 assembly of the two sources whose kernels take the DMA pipe, compiled side by side with build.py's flags."""
    try:
        cc = B.hipcc()
    except RuntimeError:
        pytest.skip("no hipcc")
    tmp = tmp_path_factory.mktemp("isa")

    def compile_one(src):
        out = tmp / src.replace(".hip", ".s")
        cmd = [cc] + B.FLAGS + B.EXTRA_FLAGS.get(src, []) + ["--cuda-device-only", "-S", os.path.join(B.CSRC, src), "-o", str(out)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return out.read_text()

    sources = ("mlp.hip", "mlp_train.hip")
    with ThreadPoolExecutor(max_workers=2) as ex:
        return dict(zip(sources, ex.map(compile_one, sources)))


@pytest.fixture(scope="module")
def asm(asms):
    return asms["mlp.hip"]


def kernel_names(text):
    return re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)\s*$", text, re.M)


def instructions(text, name):
    """Instructions of one kernel in program-text order (labels, directives, comments and the asm markers dropped)."""
    m = re.search(r"^%s:.*?^\.Lfunc_end\d+:" % re.escape(name), text, re.M | re.S)
    assert m, name
    out = []
    for line in m.group(0).splitlines()[1:]:
        line = line.split(";")[0].strip()
        if line and not line.startswith(".") and not line.endswith(":"):
            out.append(line)
    return out


def descriptor(text, name):
    m = re.search(r"^\s*\.amdhsa_kernel\s+%s\s*$(.*?)^\s*\.end_amdhsa_kernel" % re.escape(name), text, re.M | re.S)
    assert m, name
    return dict(re.findall(r"^\s*\.(amdhsa_\w+)\s+(\S+)\s*$", m.group(1), re.M))


def metadata(text, name):
    """The kernel's entry of the amdhsa.kernels note as {key: value} of its scalar fields."""
    note = text[text.index("amdhsa.kernels:"):]
    for entry in re.split(r"^  - (?=\.)", note, flags=re.M)[1:]:
        fields = dict(re.findall(r"^\s*\.(\w+):\s+(\S+)\s*$", entry, re.M))
        if fields.get("name") == name:
            return fields
    raise AssertionError(name)


def waits_before(ins, i):
    """The run of s_waitcnt instructions directly in front of instruction i, joined."""
    j = i
    while j > 0 and ins[j - 1].startswith("s_waitcnt"):
        j -= 1
    return " ".join(ins[j:i])


def test_no_slab_barrier_of_the_headline_kernel_drains_the_ring(asm):
    ins = instructions(asm, HEADLINE)
    barriers = [i for i, x in enumerate(ins) if x == "s_barrier"]
    assert len(barriers) > 10      # (one per slab position of the unrolled layers + the prologue's)
    # the prologue's barrier is the first of the kernel: slabs 0 .. 2 are waited for in full there
    assert "vmcnt(0)" in waits_before(ins, barriers[0])
    for i in barriers[1:]:
        w = waits_before(ins, i)
        assert "vmcnt(0)" not in w, (i, w)
        assert "lgkmcnt(0)" in w, (i, w)      # WAR: this wave's LDS reads of the slab that is given back have returned
    # the counted waits: one per slab barrier for wave 0 (its PPW pieces + the aux block stay in flight) and one for the others
    counted = {n: sum(1 for x in ins if x == f"s_waitcnt vmcnt({n})") for n in (PPW, PPW + 1)}
    assert counted[PPW] == counted[PPW + 1] == len(barriers) - 1, (counted, len(barriers))


def test_full_drains_of_the_headline_kernel_are_the_named_ones(asm):
    ins = instructions(asm, HEADLINE)
    drains = [i for i, x in enumerate(ins) if x.startswith("s_waitcnt") and "vmcnt(0)" in x]
    # 1  prologue: slabs 0 .. 2 before the first barrier
    # 1  drain() in front of s_endpgm
    # 1  tile start: the positions and the direction of the tile, prefetched two layers earlier (once per 77 slabs)
    # 4  the per-sample additional-input operand (add_operand: a plain load per k-block) of layer 0 and of the skip layer, once for
    #    each column order (add_first or not): loops that run only for nets with additional inputs called without the per-ray
    #    fold - an over-wait there, never an under-wait
    assert len(drains) == 7, [(i, ins[i], ins[i + 1]) for i in drains]
    assert sum(1 for i in drains if ins[i + 1] == "s_barrier") == 1
    assert sum(1 for i in drains if ins[i + 1] == "s_endpgm") == 1
    # the A-operand prefetch of kblock() stays pipelined: a wait for an LDS read leaves the pair behind it in flight
    # (`lgkmcnt(2)`).  Each pair of tiles has one such wait; full `lgkmcnt(0)` waits are the slab barriers' and a few layer heads.
    lgkm = [x for x in ins if x.startswith("s_waitcnt") and "lgkmcnt" in x]
    full = [x for x in lgkm if "lgkmcnt(0)" in x]
    assert 4 * len(full) < len(lgkm), (len(full), len(lgkm))


def test_headline_kernel_has_no_scratch_and_no_register_spill(asm):
    ins = instructions(asm, HEADLINE)
    d, m = descriptor(asm, HEADLINE), metadata(asm, HEADLINE)
    assert d["amdhsa_private_segment_fixed_size"] == "0" and d["amdhsa_enable_private_segment"] == "0"
    assert m["private_segment_fixed_size"] == "0" and m["vgpr_spill_count"] == "0"
    assert not [x for x in ins if x.startswith(("scratch_", "buffer_"))]
    assert int(m["vgpr_count"]) <= 256          # two waves per SIMD
    # (scalar registers parked in lanes of a vector register - .sgpr_spill_count, v_writelane / v_readlane - are not memory
    # traffic; the kernel has had about a dozen of them since its persistent loop)
    print("sgpr_spill_count", m["sgpr_spill_count"], "vgpr_count", m["vgpr_count"])


@pytest.mark.parametrize("src,family,at_least", [("mlp.hip", "mlp_fwd_", 5), ("mlp_train.hip", "mlp_bwd_kernel", 4)])
def test_every_dma_kernel_keeps_its_ring_in_flight(asms, src, family, at_least):
    """The widths above 256 (one wave per SIMD: forward and training forward in mlp.hip, the backward kernels in mlp_train.hip) and
    the per-ray fold kernel take the same pipe: in any kernel that issues LDS-DMA no barrier behind the prologue's may follow a
    full drain, and the hand-counted pieces must not have cost it scratch or a vector-register spill the kernel did not have
    (mlp.hip: 256 x 8 waves plain and fold, 320 .. 512; mlp_train.hip: mlp_bwd_kernel<320 .. 512> - the weight-gradient kernels
    there stage their operands with a DMA of their own, not through this pipe)."""
    text = asms[src]
    seen = 0
    for name in kernel_names(text):
        ins = instructions(text, name)
        if family not in name or not any(x.startswith("global_load_lds") for x in ins):
            continue
        seen += 1
        barriers = [i for i, x in enumerate(ins) if x == "s_barrier"]
        assert "vmcnt(0)" in waits_before(ins, barriers[0]), name
        bad = [i for i in barriers[1:] if "vmcnt(0)" in waits_before(ins, i)]
        assert not bad, (name, bad)
        m = metadata(text, name)
        assert m["private_segment_fixed_size"] == "0" and m["vgpr_spill_count"] == "0", (name, m)
    assert seen >= at_least, seen
