"""CPU (hipcc cross-compile): what the compiler made of the quantile family's
kernels (quantile.hip on latent_rows.hpp).  The file instantiates exactly the
kernels listed here, none uses scratch or spills a vector register, and the
row kernel runs at no lower an occupancy than its sibling
latent_row_kernel<StudentTRows> (160 VGPRs, 3 waves/SIMD): the inverse-Gaussian
draw is shorter than gamma_draw, so being worse would be a finding.  The
figures are those of the build that added the family, with the Makefile's
flags."""
import os

import pytest

from conftest import ROOT
from test_cholesky_kernel_resources import HIPCC, _resource_table
from test_latent_kernel_resources import EXPECTED as SIBLINGS

# {a piece of the mangled name that only this kernel has:
#  (VGPRs, occupancy [waves/SIMD]) found}
EXPECTED = {
    "latent_row_kernelINS_12_GLOBAL__N_112QuantileRowsE": (88, 5),
    "latent_draw_kernelINS_12_GLOBAL__N_120InverseGaussianDrawsE": (75, 6),
    "quantile_sum_kernel": (24, 8),
    "quantile_tau_kernel": (102, 4),
}
ROW = "latent_row_kernelINS_12_GLOBAL__N_112QuantileRowsE"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_quantile_kernels_keep_their_registers(tmp_path):
    table = _resource_table(
        os.path.join(ROOT, "bayes-bridge_amd", "csrc", "quantile.hip"),
        tmp_path)
    assert len(table) == len(EXPECTED), sorted(table)
    for piece, (vgprs, occupancy) in EXPECTED.items():
        names = [name for name in table if piece in name]
        assert len(names) == 1, (piece, sorted(table))
        res = table[names[0]]
        assert res["ScratchSize [bytes/lane]"] == 0, (piece, res)
        assert res["VGPRs Spill"] == 0, (piece, res)
        assert res["VGPRs"] <= vgprs, (piece, res)
        assert res["Occupancy [waves/SIMD]"] >= occupancy, (piece, res)
    # against the sibling: Student-t's row kernel
    sibling = SIBLINGS["student_t.hip"][
        "latent_row_kernelINS_12_GLOBAL__N_112StudentTRowsE"]
    assert sibling == (160, 3)
    assert EXPECTED[ROW][0] <= sibling[0] and EXPECTED[ROW][1] >= sibling[1]
