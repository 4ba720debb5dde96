"""CPU: a NULL handle is refused by every shared entry point of the
Hamiltonian likelihood handles (bbx_cox_*, bbx_logit_*, bbx_poisson_*,
bbx_cpoisson_*) with BBX_ERR_INVALID and the message "NULL <family> handle";
destroy(NULL) is free(NULL).  The check comes before any HIP call, so no GPU
is needed."""
import pytest

import ham_cabi as hc


@pytest.mark.parametrize('kind', sorted(hc.KINDS))
def test_null_handle_is_refused_by_every_shared_entry_point(kind):
    from bayesbridge_amd import _lib
    family = hc.KINDS[kind]
    calls = hc.Calls(_lib.load(), family)
    for name in hc.SHARED:
        assert calls.call(name, None) == (
            hc.ERR_INVALID, 'NULL %s handle' % family), name
    assert calls.destroy(None) == hc.OK
