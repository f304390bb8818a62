"""Regression guard on the compiled bulk attempt loop of the four default-mode Michaelis-Menten solve kernels: registers,
spills and scratch from the kernels' metadata, and the number of vector instructions that one attempt with no output due
executes (tools/bulk_loop_report.py: `attempt path`; the loop is issue-bound, so that count is time).  CPU only: compiles
csrc/mm_kernels.hip for gfx950 with -S as the tool does, reads metadata and counts `v_`-prefixed lines."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"

# (kernel, instantiation <WRITE_PRED, EXACT, FAST>): scratch bytes and vector spills allowed (the parent's), vector instructions on
# the attempt path of the tree as committed in profiles/ab_bulk_attempt_listing.txt
KERNELS = {
    ("15mm_solve_kernel", "ILb0ELb0ELb1"): {"scratch": 0, "vgpr_spills": 0, "path_valu": 140},          # parent: 155
    ("15mm_solve_kernel", "ILb0ELb0ELb0"): {"scratch": 0, "vgpr_spills": 0, "path_valu": 140},          # parent: 155
    ("21mm_solve_share_kernel", "ILb0ELb0ELb1"): {"scratch": 20, "vgpr_spills": 6, "path_valu": 143},   # parent: 155
    ("21mm_solve_share_kernel", "ILb0ELb0ELb0"): {"scratch": 20, "vgpr_spills": 6, "path_valu": 143},   # parent: 155
}
# spill moves (v_readlane / v_writelane of spilled scalars) inside the bulk loop: the parent's
LOOP_SPILL_MOVES = {("15mm_solve_kernel", "ILb0ELb0ELb1"): 5, ("15mm_solve_kernel", "ILb0ELb0ELb0"): 5,
                    ("21mm_solve_share_kernel", "ILb0ELb0ELb1"): 22, ("21mm_solve_share_kernel", "ILb0ELb0ELb0"): 21}


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    spec = importlib.util.spec_from_file_location("bulk_loop_report", os.path.join(ROOT, "tools", "bulk_loop_report.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    lines = tool.compile_listing(out=str(tmp_path_factory.mktemp("listing") / "mm_bulk.s"))
    return tool, lines


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_default_mode_solve_kernel_keeps_its_registers_and_its_attempt_path(listing, kernel):
    tool, lines = listing
    want = KERNELS[kernel]
    r = tool.report(lines, *kernel)
    assert r is not None, kernel
    regs, path = r["regs"], r["path"]
    print(kernel, regs, "loop", r["total"], "path", path)
    assert regs["vgpr_count"] == 128                                  # four waves per SIMD
    assert regs["vgpr_spill_count"] <= want["vgpr_spills"]
    assert regs["private_segment_fixed_size"] <= want["scratch"]
    assert regs["group_segment_fixed_size"] == 0                      # LDS is dynamic only (solve_lds_bytes)
    assert r["total"]["spill"] <= LOOP_SPILL_MOVES[kernel]
    assert path["spill"] == 0
    assert 100 <= path["valu"] <= want["path_valu"]                   # the walk found the attempt (>= its 94 FP64 stage operations)
