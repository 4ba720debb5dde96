"""CPU (hipcc cross-compile): no kernel of the woodbury sampler
(woodbury.hip: the Gram over the columns on the f64 matrix cores and the
draw's vector kernels) and neither kernel of the wide dense product
(dense.hip) uses scratch or spills registers, and their LDS stays inside the
64 KiB a workgroup may declare statically."""
import os

import pytest

from conftest import ROOT
from test_cholesky_kernel_resources import HIPCC, _resource_table

KERNELS = ("wb_gram_tiles_kernel", "wb_gram_reduce_kernel", "wb_prep_kernel",
           "wb_reset_kernel", "wb_rows_kernel", "wb_phif_kernel",
           "wb_resid_kernel", "wb_lincomb_kernel", "wb_inner_kernel",
           "wb_beta_r_kernel", "wb_scatter_kernel")
LDS_LIMIT = 64 * 1024


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_woodbury_kernels_do_not_spill(tmp_path):
    table = _resource_table(
        os.path.join(ROOT, "bayes-bridge_amd", "csrc", "woodbury.hip"),
        tmp_path)
    for k in KERNELS:
        assert any(k in name for name in table), (k, sorted(table))
    assert sum("wb_gram_tiles_kernel" in k for k in table) == 2
    for name, res in table.items():
        assert res["VGPRs Spill"] == 0, (name, res)
        assert res["SGPRs Spill"] == 0, (name, res)
        assert res["ScratchSize [bytes/lane]"] == 0, (name, res)
        assert res["LDS Size [bytes/block]"] <= LDS_LIMIT, (name, res)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_wide_dense_kernels_do_not_spill(tmp_path):
    table = _resource_table(
        os.path.join(ROOT, "bayes-bridge_amd", "csrc", "dense.hip"), tmp_path)
    wide = {k: v for k, v in table.items() if "dense_dot_wide" in k}
    assert len(wide) == 3, sorted(wide)       # f32, f64, the reduction
    for name, res in wide.items():
        assert res["VGPRs Spill"] == 0, (name, res)
        assert res["SGPRs Spill"] == 0, (name, res)
        assert res["ScratchSize [bytes/lane]"] == 0, (name, res)
        assert res["LDS Size [bytes/block]"] <= LDS_LIMIT, (name, res)
