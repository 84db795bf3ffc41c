"""The kg_mcmc_* entry points check their arguments, and create its
configuration, before they touch a device: errors come back through
kg_last_error.  (CPU, no GPU needed.)"""
import ctypes as C

import pytest

from korali_amd import native


@pytest.mark.parametrize("call,args", [
    ("kg_mcmc_run", (1, 1, 0, None, None)), ("kg_mcmc_propose", (0,)), ("kg_mcmc_get_candidate", (None,)),
    ("kg_mcmc_decide", (0, 0.0, None)), ("kg_mcmc_end_generation", (1,)), ("kg_mcmc_database", (None, None, None)),
    ("kg_mcmc_synchronize", ()), ("kg_mcmc_field_size", (b"Chain Leader", None)),
    ("kg_mcmc_get_field", (b"Chain Leader", None, 0)), ("kg_mcmc_set_field", (b"Chain Leader", None, 0)),
    ("kg_mcmc_get_rng", (1, None)), ("kg_mcmc_set_rng", (1, None)), ("kg_mcmc_diagnostics", (None, None, None)),
    ("kg_mcmc_profile", (1,)), ("kg_mcmc_profile_read", (b"chain", None, None)),
])
def test_null_handle_is_an_error(call, args):
    L = native.lib()
    assert getattr(L, call)(None, *args) != 0
    assert L.kg_last_error().decode() == call + ": null handle"


def test_destroy_accepts_null_and_create_rejects_null():
    L = native.lib()
    assert L.kg_mcmc_destroy(None) == 0
    h = C.c_void_p()
    assert L.kg_mcmc_create(None, C.byref(h)) != 0
    with pytest.raises(native.KoraliDeviceError, match="null argument"):
        native.check(1)
    cfg = native._McmcCfg()
    assert L.kg_mcmc_create(C.byref(cfg), None) != 0
    with pytest.raises(native.KoraliDeviceError, match="null argument"):
        native.check(1)


@pytest.mark.parametrize("kw,msg", [
    # MCMC.cpp.base:23-27, verbatim (a negative size_t prints as the reference's %zu does)
    (dict(chain_covariance_scaling=0.0), r"^Chain Covariance Scaling must be larger 0.0 \(is 0.000000\).\n$"),
    (dict(chain_covariance_scaling=-1.5), r"^Chain Covariance Scaling must be larger 0.0 \(is -1.500000\).\n$"),
    (dict(leap=0), r"^Leap must be larger 0 \(is 0\).\n$"),
    (dict(burn_in=-1), r"^Burn In must be larger equal 0 \(is 18446744073709551615\).\n$"),
    (dict(rejection_levels=0), r"^Rejection Levels must be larger 0 \(is 0\).\n$"),
    (dict(non_adaption_period=-2), r"^Non Adaption Period must be larger equal 0 \(is 18446744073709551614\).\n$"),
    # the device's limits
    (dict(N=0), "'Variable Count' must be >= 1"),
    (dict(N=65), "more than 64 variables"),
    (dict(rejection_levels=9), "more than 8 'Rejection Levels'"),
    (dict(max_samples=0), "'Max Samples' must be at least 1"),
    (dict(N=64, max_samples=2**21 + 1), r"exceeds the database's capacity on the device \(2\^27 values\)"),
    (dict(probability=7), "unknown builtin probability kernel"),
    (dict(prior_kinds=[0, 9, 0], prior_min=0.0, prior_max=1.0), "prior_kind entries"),
])
def test_create_checks_the_configuration_before_the_device(kw, msg):
    kw = dict(kw)
    N = kw.pop("N", 3)
    with pytest.raises(native.KoraliDeviceError, match=msg):
        native.McmcDevice(N, 0.0, 1.0, **kw)


def test_create_needs_the_initial_values_and_prior_parameters():
    L = native.lib()
    cfg = native._McmcCfg()
    cfg.variable_count, cfg.leap, cfg.rejection_levels, cfg.chain_covariance_scaling, cfg.max_samples = 2, 1, 1, 1.0, 10
    h = C.c_void_p()
    assert L.kg_mcmc_create(C.byref(cfg), C.byref(h)) != 0
    assert "'Initial Mean' and 'Initial Standard Deviation'" in L.kg_last_error().decode()
    v = (C.c_double * 2)(0.0, 1.0)
    cfg.initial_mean = cfg.initial_sdev = v
    cfg.prior_kind = (C.c_int * 2)(0, 0)
    assert L.kg_mcmc_create(C.byref(cfg), C.byref(h)) != 0
    assert "parameters of every variable's prior" in L.kg_last_error().decode()


def test_kernel_and_stop_names():
    assert native.MCMC_KERNELS == {"gaussian": 1}
    assert native.MCMC_STOP == {1: "Max Samples", 2: "Max Model Evaluations"}
