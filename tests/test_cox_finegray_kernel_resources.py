"""CPU (hipcc cross-compile): no kernel of the Fine-Gray handle
(cox_finegray.hip: its instantiations of cox_family.hpp's three kernels,
its copies of the scan kernels of cox_scan.hpp and of the trajectory kernels
of hamiltonian.hpp) uses scratch or spills registers."""
import os

import pytest

from conftest import ROOT
from test_cholesky_kernel_resources import HIPCC, _resource_table

OWN = {"cox_risk_sum_kernel": 2,        # h and h / G; h u and (h u) / G
       "cox_event_sum_kernel": 2,       # 1/H and g/H; z and g z
       "cox_row_weight_kernel": 2}      # gradient, Hessian
SHARED = ("cox_max_kernel", "cox_scan_out_kernel", "cox_loglik_kernel",
          "cox_reset_kernel", "cox_step1_kernel", "cox_post_a_kernel",
          "cox_post_b_kernel", "cox_nuts_leaf_kernel",
          "cox_nuts_merge_a_kernel", "cox_nuts_merge_b_kernel")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_cox_finegray_kernels_do_not_spill(tmp_path):
    table = _resource_table(
        os.path.join(ROOT, "bayes-bridge_amd", "csrc", "cox_finegray.hip"),
        tmp_path)
    for k, count in OWN.items():
        assert sum(k in name for name in table) == count, (k, sorted(table))
    for k in SHARED:
        assert any(k in name for name in table), (k, sorted(table))
    for name, res in table.items():
        assert res["VGPRs Spill"] == 0, (name, res)
        assert res["SGPRs Spill"] == 0, (name, res)
        assert res["ScratchSize [bytes/lane]"] == 0, (name, res)
