"""Hazard wait states between the MFMAs of the 8-wave width-256 inference kernels, counted on the gfx950 assembly of csrc/mlp.hip
(CPU only: hipcc cross-compiles; skipped without hipcc).

What went wrong before, and what this pins: hipcc lets a tile pair's last MFMA write its accumulator into the A-operand registers
that just died and gives the old accumulator quad to the next `ds_read_b128`.  With the A-operand prefetch pinned to the top of
the next pair (kblock()), that read stood right behind the MFMA that still reads the quad as SrcC, and the hazard recognizer put
`s_nop 6` / `s_nop 7` between them: 7 - 8 wait states of 4 clocks in 1 MFMA gap of 20, which no MFMA covers (167 such gaps in the
headline kernel).  kblock_deep() (csrc/mlp_device.h) reads two pairs ahead, behind the pair's 2nd MFMA; what is left is 6 wait
states at the most per gap in the slab loops - 6 x 4 + the MFMA's own 8 clocks are the 32 that the MFMA in front of it occupies
the pipe - and the waits for the reads stay counted (`lgkmcnt(2)`)."""
import os
import re
import subprocess

import pytest

from smpl_nerf_amd import build as B
from test_weight_ring_isa import HEADLINE, descriptor, instructions, metadata

FOLD = "_ZN5snerf19mlp_fwd_fold_kernelILi256ELi8EEEvNS_7FwdArgsE"                            # snerf::mlp_fwd_fold_kernel<256, 8>
FITS = 6      # wait states of an `s_nop` run that fit beside a 16x16x4 fp32 MFMA: 6 x 4 + 8 clocks = its 32


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    """gfx950 assembly of csrc/mlp.hip with build.py's flags."""
    try:
        cc = B.hipcc()
    except RuntimeError:
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("isa") / "mlp.s"
    cmd = [cc] + B.FLAGS + B.EXTRA_FLAGS.get("mlp.hip", []) + ["--cuda-device-only", "-S", os.path.join(B.CSRC, "mlp.hip"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out.read_text()


def mfma_gaps(ins):
    """`s_nop` wait states (operand + 1) between consecutive v_mfma instructions, in program-text order."""
    gaps, cur, seen = [], 0, False
    for x in ins:
        if x.startswith("v_mfma"):
            if seen:
                gaps.append(cur)
            seen, cur = True, 0
        elif x.startswith("s_nop"):
            cur += int(x.split()[1], 0) + 1
    return gaps


@pytest.mark.parametrize("name", [HEADLINE, FOLD], ids=["mlp_fwd_kernel<256,8>", "mlp_fwd_fold_kernel<256,8>"])
def test_hazard_wait_states_fit_beside_the_mfmas(asm, name):
    ins = instructions(asm, name)
    gaps = mfma_gaps(ins)
    n_mfma = len(gaps) + 1
    assert n_mfma > 3000, n_mfma
    long_gaps = [g for g in gaps if g > FITS]
    print(name, "MFMAs", n_mfma, "s_nop wait states", sum(gaps), "gaps >", FITS, ":", sorted(long_gaps))
    # at most one gap in 64 static MFMAs may carry more (52 for the headline kernel's 3328).  The 12 (headline) / 17 (fold) that
    # remain are not between the tile pairs of the slab loops:
    #   * encoder gaps: the positional-encoding operand of a k-block of layer 0, of the skip layer and of the directional layer is
    #     evaluated between two k-blocks (sincosf: 360 - 380 instructions with `s_nop`s of their own) - 25 - 26 wait states; in the
    #     fold kernel the per-ray table rows are added there as well (up to 52);
    #   * tile start and layer boundaries: relu_into(), the result store, the next tile's bookkeeping, the bias reads of init() -
    #     28 - 34 wait states over some 380 instructions, once per tile;
    #   * the one-tile sigma / rgb heads (kblock<1>: 4 dependent MFMAs per k-block, its two reads at the top): 9 wait states in
    #     front of a read that takes over the registers of the chain's previous MFMA, three or four times per head;
    #   * the DMA issue: where stage() sits between two pairs the `s_nop 0` of its M0 writes comes on top of a short hazard pad -
    #     10 - 11 wait states, in the unrolled heads only;
    #   * the address select of a rolled k-block loop (v_cndmask on the next block's pointer): 7 - 8 wait states, once per loop.
    assert len(long_gaps) * 64 <= n_mfma, (len(long_gaps), n_mfma, sorted(long_gaps))


@pytest.mark.parametrize("name", [HEADLINE, FOLD], ids=["mlp_fwd_kernel<256,8>", "mlp_fwd_fold_kernel<256,8>"])
def test_the_prefetch_costs_no_scratch_and_stays_pipelined(asm, name):
    ins = instructions(asm, name)
    d, m = descriptor(asm, name), metadata(asm, name)
    assert d["amdhsa_private_segment_fixed_size"] == "0" and m["private_segment_fixed_size"] == "0"
    assert m["vgpr_spill_count"] == "0"
    assert int(m["vgpr_count"]) <= 256          # two waves per SIMD
    # the A-operand prefetch stays in flight behind the MFMAs that hide it: a wait for one pair's reads leaves the next pair's
    # outstanding, so most LDS waits are counted, not full
    lgkm = [x for x in ins if x.startswith("s_waitcnt") and "lgkmcnt" in x]
    nonzero = [x for x in lgkm if not re.search(r"lgkmcnt\(0\)", x)]
    assert len(lgkm) > 100 and 2 * len(nonzero) >= len(lgkm), (len(nonzero), len(lgkm))
