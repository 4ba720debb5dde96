"""CPU (hipcc cross-compile): what the compiler made of the latent families'
kernels (probit.hip, student_t.hip, censored.hip on latent_rows.hpp).  Each
file instantiates exactly the kernels listed here, none uses scratch or spills
a vector register, and none needs more vector registers or runs at a lower
occupancy than the kernel it replaced in the build before the fold: a row
expression inlined through a policy is the same code.  The figures are those of
that build, with the Makefile's flags."""
import os

import pytest

from conftest import ROOT
from test_cholesky_kernel_resources import HIPCC, _resource_table

# file: {a piece of the mangled name that only this kernel has:
#        (VGPRs, occupancy [waves/SIMD]) of its predecessor}
# (latent_row_kernel<Policy> after chain_probit_kernel, student_t_mix_kernel and
# chain_censored_kernel; latent_draw_kernel<Policy> after
# dev_truncated_normal_kernel and dev_censored_normal_kernel; ProbitRowsIdE: on
# the chain's double outcome, IhE: on the sampler's bytes)
EXPECTED = {
    "probit.hip": {
        "latent_row_kernelINS_12_GLOBAL__N_110ProbitRowsIdE": (146, 3),
        "latent_draw_kernelINS_12_GLOBAL__N_110ProbitRowsIhE": (94, 5),
    },
    "student_t.hip": {
        "latent_row_kernelINS_12_GLOBAL__N_112StudentTRowsE": (160, 3),
        "student_t_wrss_kernel": (16, 8),
        "student_t_tau_kernel": (102, 4),
    },
    "censored.hip": {
        "latent_row_kernelINS_12_GLOBAL__N_112CensoredRowsE": (154, 3),
        "latent_draw_kernelINS_12_GLOBAL__N_112CensoredRowsE": (99, 4),
    },
}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.parametrize("src", sorted(EXPECTED))
def test_latent_kernels_keep_their_registers(src, tmp_path):
    table = _resource_table(
        os.path.join(ROOT, "bayes-bridge_amd", "csrc", src), tmp_path)
    expected = EXPECTED[src]
    assert len(table) == len(expected), sorted(table)
    for piece, (vgprs, occupancy) in expected.items():
        names = [name for name in table if piece in name]
        assert len(names) == 1, (piece, sorted(table))
        res = table[names[0]]
        assert res["ScratchSize [bytes/lane]"] == 0, (piece, res)
        assert res["VGPRs Spill"] == 0, (piece, res)
        assert res["VGPRs"] <= vgprs, (piece, res)
        assert res["Occupancy [waves/SIMD]"] >= occupancy, (piece, res)
