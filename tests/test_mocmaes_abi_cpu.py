"""The kg_mocmaes_* entry points check their arguments, and create its
configuration, before they touch a device: errors come back through
kg_last_error (CPU, no GPU needed)."""
import ctypes as C

import pytest

from korali_amd import native


@pytest.mark.parametrize("call,args", [
    ("kg_mocmaes_initialize", ()), ("kg_mocmaes_prepare", (2,)), ("kg_mocmaes_eval_builtin", (0,)),
    ("kg_mocmaes_get_candidates", (None, 0)), ("kg_mocmaes_set_values", (None,)), ("kg_mocmaes_update", (1,)),
    ("kg_mocmaes_generation", (1, 0)), ("kg_mocmaes_synchronize", ()),
    ("kg_mocmaes_field_size", (b"Current Values", None)), ("kg_mocmaes_get_field", (b"Current Values", None, 0)),
    ("kg_mocmaes_set_field", (b"Current Values", None, 0)), ("kg_mocmaes_get_rng", (1, None)),
    ("kg_mocmaes_set_rng", (1, None)), ("kg_mocmaes_diagnostics", (None, None, None, None)),
    ("kg_mocmaes_profile", (1,)), ("kg_mocmaes_profile_read", (b"update", None, None)),
])
def test_null_handle_is_an_error(call, args):
    L = native.lib()
    assert getattr(L, call)(None, *args) != 0
    assert L.kg_last_error().decode() == call + ": null handle"


def test_destroy_accepts_null_and_create_rejects_null():
    L = native.lib()
    assert L.kg_mocmaes_destroy(None) == 0
    h = C.c_void_p()
    assert L.kg_mocmaes_create(None, C.byref(h)) != 0
    with pytest.raises(native.KoraliDeviceError, match="null argument"):
        native.check(1)
    cfg = native._MocmaesCfg()
    assert L.kg_mocmaes_create(C.byref(cfg), None) != 0
    with pytest.raises(native.KoraliDeviceError, match="null argument"):
        native.check(1)


@pytest.mark.parametrize("kw,msg", [
    (dict(num_objectives=1), "requires multiple objectives"),
    (dict(num_objectives=9), "above 8"),
    (dict(P=8, mu=9), "must be smaller or equal with population size"),
    (dict(N=129, P=200), "more than 128 variables"),
    (dict(N=5, P=4), "_currentSigma"),
    (dict(success_learning_rate=0.0), "Success Learning Rate"),
    (dict(success_learning_rate=1.5), "Success Learning Rate"),
    (dict(target_success_rate=0.0), "Target Success Rate"),
    (dict(target_success_rate=1.01), "Target Success Rate"),
    (dict(upper=float("inf")), "cannot be inferred"),
    (dict(lower=float("-inf"), initial_value=0.0), "cannot be inferred"),  # the deviation still needs the bounds
    (dict(lower=None), "Lower Bound"),
    (dict(parent_order=5), "parent order"),
])
def test_create_checks_the_configuration_before_the_device(kw, msg):
    kw = dict(kw)
    N, P = kw.pop("N", 2), kw.pop("P", 8)
    lower, upper = kw.pop("lower", -1.0), kw.pop("upper", 1.0)
    with pytest.raises(native.KoraliDeviceError, match=msg):
        native.MocmaesDevice(N, P, lower, upper, **kw)


def test_parent_order_names():
    assert native.MOCMAES_PARENT_ORDERS == {"descending": 0, "recorded": 1}
