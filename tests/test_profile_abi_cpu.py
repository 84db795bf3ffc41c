"""The stage-timer entry points of CMA-ES and TMCMC check their handle like
those of the other solvers: a null handle comes back as an error through
kg_last_error instead of being dereferenced (CPU, no GPU needed)."""
import pytest

from korali_amd import native


@pytest.mark.parametrize("call,args", [
    ("kg_cmaes_profile", (1,)), ("kg_cmaes_profile_read", (b"eigen", None, None)),
    ("kg_cmaes_profile_mark", (b"exchange", 0)),
    ("kg_tmcmc_profile", (1,)), ("kg_tmcmc_profile_read", (b"draw", None, None)),
])
def test_null_handle_is_an_error(call, args):
    L = native.lib()
    assert getattr(L, call)(None, *args) != 0
    assert L.kg_last_error().decode() == call + ": null handle"
