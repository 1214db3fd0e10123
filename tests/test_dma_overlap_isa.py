"""No GPU: compile csrc/gemm.hip and csrc/attention.hip with the Makefile's own flags, keep the
assembly, and let tools/isa_dma_waits.py look at every loop that stages tiles by LDS-DMA.  A
compiler-inserted `s_waitcnt vmcnt(0)` inside such a loop drains the DMA ring in the middle of
the loop body (hipcc adds one in front of a transposed LDS read it issues itself): results stay
right, fill and MFMA stop overlapping, and only the assembly shows it.  Also held here: no
spills in those kernels and the register budgets their occupancy rests on (dQ: 168 VGPRs for 3
waves per SIMD; everything else 256)."""
import importlib.util
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "multi-modal-uncertainty_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")


def _tool():
    spec = importlib.util.spec_from_file_location("isa_dma_waits", os.path.join(REPO, "tools", "isa_dma_waits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="session")
def asm_dir(tmp_path_factory):
    """both files compiled once (about a minute): <dir>/<name>-hip-amdgcn-amd-amdhsa-gfx950.s"""
    d = str(tmp_path_factory.mktemp("isa"))
    objs = [os.path.join(d, n + ".o") for n in ("gemm", "attention")]
    subprocess.run(["make", "-s", "-j2", "HIPCC=" + HIPCC, "OBJDIR=" + d, "EXTRA=-save-temps=obj"] + objs, cwd=CSRC,
                   check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    return d


VGPR_CAP = {"mmu::attn_dq_dma_kernel": 168}
# the forward keeps the builtin read (and with it the compiler's wait): its 2-deep ring with a full
# wait per tile measured no gain from the asm reads (profiles/dma_overlap_ab.txt)
NOT_CONVERTED = "attn_fwd_v2_kernel"


@pytest.mark.parametrize("name,kernels", [
    ("gemm", ["gemm_big_kernel<false, false, 0, true>", "gemm_big_kernel<true, false, 8, false>",
              "gemm_big_kernel<false, true, 0, true>", "gemm_convw_kernel", "gemm_conva_kernel<0>",
              "gemm_wide_kernel<0, false>"]),
    ("attention", ["attn_dq_dma_kernel", "attn_dkdv_dma_kernel<true>", "attn_dkdv_dma_kernel<false>"])])
def test_no_compiler_drain_in_dma_loops(asm_dir, name, kernels):
    tool = _tool()
    path = os.path.join(asm_dir, name + "-hip-amdgcn-amd-amdhsa-gfx950.s")
    rows = [r for r in tool.scan(path) if NOT_CONVERTED not in r["kernel"]]
    found = {r["kernel"] for r in rows}
    for kn in kernels:  # the scan saw the kernels it is meant to guard, with their DMA loops
        assert "mmu::" + kn in found, f"{kn}: no LDS-DMA loop found in {name}.s"
    bad = [f"{r['kernel']}: {r['sites']} compiler vmcnt(0) in LDS-DMA loops" for r in rows if r["sites"]]
    # spills: the attention kernels and the 256x256 body (the 256x384 wide kernel's f32-residual
    # epilogues spill a few registers outside the K loop, as before)
    bad += [f"{r['kernel']}: {r['spills']} VGPRs spilled" for r in rows
            if r["spills"] and "gemm_wide_kernel" not in r["kernel"]]
    bad += [f"{r['kernel']}: {r['vgprs']} VGPRs > {VGPR_CAP.get(r['kernel'], 256)}" for r in rows
            if r["vgprs"] > VGPR_CAP.get(r["kernel"], 256)]
    assert not bad, "\n".join(bad)
    if name == "gemm":
        assert tool.main([path, "--quiet"]) == 0


def test_tool_flags_a_compiler_drain(tmp_path):
    """a hand-made loop: one hand-placed counted wait, one compiler vmcnt(0) before a transposed read"""
    tool = _tool()
    s = tmp_path / "k.s"
    s.write_text("\n".join([
        "_Z1kv:", ".LBB0_1:", "\tbuffer_load_dwordx4 v1, s[0:3], 0 offen lds", "\t;;#ASMSTART",
        "\ts_waitcnt vmcnt(1)", "\t;;#ASMEND", "\ts_waitcnt vmcnt(0)", "\tds_read_b64_tr_b16 v[2:3], v4",
        "\ts_cbranch_scc1 .LBB0_1", ".Lfunc_end0:", "    .name:           _Z1kv", "    .vgpr_count:     5",
        "    .vgpr_spill_count: 0", ""]))
    (row,) = tool.scan(str(s))
    assert (row["sites"], row["tr_sites"], row["vgprs"], row["spills"]) == (1, 1, 5, 0)
    assert tool.main([str(s)]) == 1
    s.write_text(s.read_text().replace("\ts_waitcnt vmcnt(0)\n", "\t;;#ASMSTART\n\ts_waitcnt vmcnt(0)\n\t;;#ASMEND\n"))
    assert tool.main([str(s)]) == 0
