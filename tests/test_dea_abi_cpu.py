"""The kg_dea_* entry points check their arguments before they touch a
device: a null handle or configuration comes back as an error through
kg_last_error (CPU, no GPU needed)."""
import ctypes as C

import pytest

from korali_amd import native


@pytest.mark.parametrize("call,args", [
    ("kg_dea_initialize", ()), ("kg_dea_prepare", (2,)), ("kg_dea_eval_builtin", (0,)),
    ("kg_dea_get_candidates", (None, 0)), ("kg_dea_set_fitness", (None,)), ("kg_dea_update", (1,)),
    ("kg_dea_generation", (1, 0)), ("kg_dea_synchronize", ()), ("kg_dea_field_size", (b"Value Vector", None)),
    ("kg_dea_get_field", (b"Value Vector", None, 0)), ("kg_dea_set_field", (b"Value Vector", None, 0)),
    ("kg_dea_get_rng", (1, None)), ("kg_dea_set_rng", (1, None)), ("kg_dea_windows", (None, None)),
    ("kg_dea_profile", (1,)), ("kg_dea_profile_read", (b"propose", None, None)),
])
def test_null_handle_is_an_error(call, args):
    L = native.lib()
    assert getattr(L, call)(None, *args) != 0
    assert L.kg_last_error().decode() == call + ": null handle"


def test_destroy_accepts_null_and_create_rejects_null():
    L = native.lib()
    assert L.kg_dea_destroy(None) == 0
    h = C.c_void_p()
    assert L.kg_dea_create(None, C.byref(h)) != 0
    with pytest.raises(native.KoraliDeviceError, match="null argument"):
        native.check(1)


@pytest.mark.parametrize("kw,msg", [
    (dict(P=3), "at least 4"), (dict(P=2, parent_rule="Best"), "at least 4 with Parent Selection Rule 'Random' and 3"),
    (dict(lower=[0.0, 2.0]), "Lower Bound exceeds Upper Bound"), (dict(upper=[1.0, float("inf")]), "finite"),
    (dict(accept_rule=7), "Accept Rule"),
])
def test_create_checks_the_configuration_before_the_device(kw, msg):
    """What the reference cannot run either (its rejection loops never end
    with too few samples; DEA.cpp.base:19-21 for the bounds)."""
    kw = dict(kw)
    P, lower, upper = kw.pop("P", 8), kw.pop("lower", [0.0, 0.0]), kw.pop("upper", [1.0, 1.0])
    with pytest.raises(native.KoraliDeviceError, match=msg):
        native.DeaDevice(2, P, lower, upper, **kw)
