"""The kg_nested_* entry points check their arguments, and create its
configuration, before they touch a device: errors come back through
kg_last_error.  kg_nested_permutation is host code.  (CPU, no GPU needed.)"""
import ctypes as C

import numpy as np
import pytest

from korali_amd import native


@pytest.mark.parametrize("call,args", [
    ("kg_nested_first_generation", ()), ("kg_nested_generation", (2, None)), ("kg_nested_prepare", (2,)),
    ("kg_nested_get_candidates", (None, 0)), ("kg_nested_set_evaluations", (None,)), ("kg_nested_eval_builtin", ()),
    ("kg_nested_process", (2, None, None)), ("kg_nested_finalize", ()), ("kg_nested_synchronize", ()),
    ("kg_nested_field_size", (b"LStar", None)), ("kg_nested_get_field", (b"LStar", None, 0)),
    ("kg_nested_set_field", (b"LStar", None, 0)), ("kg_nested_get_rng", (1, None)), ("kg_nested_set_rng", (1, None)),
    ("kg_nested_diagnostics", (None, None, None)), ("kg_nested_profile", (1,)),
    ("kg_nested_profile_read", (b"draw", None, None)),
])
def test_null_handle_is_an_error(call, args):
    L = native.lib()
    assert getattr(L, call)(None, *args) != 0
    assert L.kg_last_error().decode() == call + ": null handle"


def test_destroy_accepts_null_and_create_rejects_null():
    L = native.lib()
    assert L.kg_nested_destroy(None) == 0
    h = C.c_void_p()
    assert L.kg_nested_create(None, C.byref(h)) != 0
    with pytest.raises(native.KoraliDeviceError, match="null argument"):
        native.check(1)
    cfg = native._NestedCfg()
    assert L.kg_nested_create(C.byref(cfg), None) != 0
    with pytest.raises(native.KoraliDeviceError, match="null argument"):
        native.check(1)


@pytest.mark.parametrize("kw,msg", [
    (dict(min_log_evidence_delta=-0.5), r"Min Log Evidence Delta must be larger equal 0.0 \(is -0.500000\)."),
    (dict(method="Multi Ellipse"), "'Multi Ellipse' is not available"),
    (dict(method=7), "Only accepted Resampling Method are 'Box', 'Ellipse' and 'Multi Ellipse'"),
    (dict(proposal_update_frequency=0), "Proposal Update Frequency must be larger 0"),
    (dict(N=2), r"Resampling Method 'Ellipse' and 'Multi Ellipse' only suitable for problems of dim larger 2 "
                r"\(use Resampling Method 'Box'\)."),
    (dict(N=0, method="Box"), "'Variable Count' must be >= 1"),
    (dict(N=65), "more than 64 variables"),
    (dict(L=1), "'Number Live Points' must be at least 2"),
    (dict(batch_size=0), "'Batch Size' must be at least 1"),
    (dict(prior_kinds=["Normal", "Uniform", "Uniform"], upper_bound=1.0),
     "Prior of variable 0 is not 'Univariate/Uniform' AND lower bound not set"),
    (dict(prior_kinds=["Uniform", "Uniform", "LogNormal"], lower_bound=0.5),
     "Prior of variable 2 is not 'Univariate/Uniform' AND upper bound not set"),
    (dict(prior_kinds=[0, 9, 0]), "prior_kind entries"),
])
def test_create_checks_the_configuration_before_the_device(kw, msg):
    kw = dict(kw)
    N, L = kw.pop("N", 3), kw.pop("L", 16)
    if "prior_kinds" in kw and len(kw["prior_kinds"]) != N:
        kw["prior_kinds"] = kw["prior_kinds"][:N]
    with pytest.raises(native.KoraliDeviceError, match=msg):
        native.NestedDevice(N, L, -1.0, 1.0, **kw)


@pytest.mark.parametrize("n", [0, 1, 2, 17, 1000])
def test_permutation_is_a_permutation_and_deterministic_per_seed(n):
    p = native.nested_permutation(12345, n)
    assert sorted(p.tolist()) == list(range(n))
    assert np.array_equal(p, native.nested_permutation(12345, n))
    if n >= 17:
        assert not np.array_equal(p, native.nested_permutation(12346, n))
        assert not np.array_equal(p, np.arange(n))


def test_method_and_termination_names():
    assert native.NESTED_METHODS == {"box": 0, "ellipse": 1, "multi ellipse": 2}
    assert native.NESTED_TERMINATION == {1: "Min Log Evidence Delta", 2: "Max Effective Sample Size",
                                         4: "Max Log Likelihood"}
