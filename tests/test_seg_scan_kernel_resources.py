"""CPU (hipcc cross-compile): what the compiler made of the kernels that run
the block scan of csrc/seg_scan.hpp -- cpoisson.hip's two passes, cox.hip's
stratified passes (cox_strat.hpp) and the copy of cox_scan_out_kernel
(cox_scan.hpp) in each of the five Cox files.  None uses scratch or spills a
register, and none needs more vector registers or runs at a lower occupancy
than it did in the build before the three copies of the scan were folded onto
one skeleton: a monoid inlined through a policy is the same code.  The figures
are those of that build, with the Makefile's flags.  (After the fold the two
CO_SUM kernels, which no longer carry an unused m through shuffles and LDS,
need 43 and 64 registers and cp_out_kernel<1> runs at 8 waves per SIMD.)"""
import os

import pytest

from conftest import ROOT
from test_cholesky_kernel_resources import HIPCC, _resource_table

SCAN_OUT = {"cox_scan_out_kernel": (60, 8)}
# file: {a piece of the mangled name that only this kernel has:
#        (VGPRs, occupancy [waves/SIMD]) of its predecessor}
EXPECTED = {
    "cpoisson.hip": {
        "cp_agg_kernelILi0E": (70, 7),
        "cp_agg_kernelILi1E": (44, 8),
        "cp_out_kernelILi0E": (120, 4),
        "cp_out_kernelILi1E": (65, 7),
    },
    "cox.hip": {
        "coxs_agg_kernelILi0E": (24, 8),
        "coxs_agg_kernelILi1E": (68, 7),
        "coxs_agg_kernelILi2E": (32, 8),
        "coxs_agg_kernelILi3E": (64, 8),
        "coxs_agg_kernelILi4E": (32, 8),
        "coxs_out_kernelILi0E": (84, 5),
        "coxs_out_kernelILi1E": (74, 6),
        "coxs_out_kernelILi2E": (75, 6),
        **SCAN_OUT,
    },
    "cox_efron.hip": SCAN_OUT,
    "cox_interval.hip": SCAN_OUT,
    "cox_weighted.hip": SCAN_OUT,
    "cox_finegray.hip": SCAN_OUT,
}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.parametrize("src", sorted(EXPECTED))
def test_scan_kernels_keep_their_registers(src, tmp_path):
    table = _resource_table(
        os.path.join(ROOT, "bayes-bridge_amd", "csrc", src), tmp_path)
    for piece, (vgprs, occupancy) in EXPECTED[src].items():
        names = [name for name in table if piece in name]
        assert len(names) == 1, (piece, sorted(table))
        res = table[names[0]]
        print(src, piece, res)
        assert res["ScratchSize [bytes/lane]"] == 0, (piece, res)
        assert res["VGPRs Spill"] == 0, (piece, res)
        assert res["SGPRs Spill"] == 0, (piece, res)
        assert res["VGPRs"] <= vgprs, (piece, res)
        assert res["Occupancy [waves/SIMD]"] >= occupancy, (piece, res)
