"""ctypes binding of the DeepSupervisor learner's C-ABI (include/korali_amd.h,
kg_supervisor_*).

The device path of Korali's `Learner / DeepSupervisor` solver on a
`Supervised Learning` problem (solver/learner/deepSupervisor/
deepSupervisor.cpp.base): feed-forward networks of Linear and Activation
layers in float32.  Every call goes to the HIP kernels of
korali_amd/libkorali_amd.so; there is no CPU fallback.
"""
import ctypes as C

import numpy as np

from .native import KoraliDeviceError, check, lib

FUNCTIONS = {"Elementwise/Tanh": 0, "Elementwise/ReLU": 1, "Elementwise/Logistic": 2, "Elementwise/SoftReLU": 3,
             "Elementwise/SoftSign": 4, "Elementwise/Linear": 5, "Elementwise/Log": 6, "Softmax": 7}
MASKS = {"Identity": 0, "Absolute": 1, "Softplus": 2, "Tanh": 3, "Sigmoid": 4}
OPTIMIZERS = {"Adam": 0, "AdaBelief": 1, "MADGRAD": 2, "RMSProp": 3, "Adagrad": 4}
LOSSES = {"Mean Squared Error": 0, "Direct Gradient": 1}
STATE_FIELDS = {"Adam": ("first_moment", "second_moment"), "AdaBelief": ("first_moment", "second_central_moment"),
                "MADGRAD": ("s", "v", "z"), "RMSProp": ("r", "v"), "Adagrad": ("s",)}


class _Layer(C.Structure):
    _fields_ = [("type", C.c_int), ("output_channels", C.c_size_t), ("function", C.c_int), ("alpha", C.c_float),
                ("beta", C.c_float)]


class _Cfg(C.Structure):
    _fields_ = [("input_size", C.c_size_t), ("solution_size", C.c_size_t), ("training_batch_size", C.c_size_t),
                ("inference_batch_size", C.c_size_t), ("layer_count", C.c_size_t), ("layers", C.POINTER(_Layer)),
                ("output_scale", C.POINTER(C.c_float)), ("output_shift", C.POINTER(C.c_float)),
                ("output_mask", C.POINTER(C.c_int)), ("optimizer", C.c_int), ("loss", C.c_int),
                ("learning_rate", C.c_float), ("l2_enabled", C.c_int), ("l2_importance", C.c_float), ("device", C.c_int)]


_BOUND = False


def _lib():
    global _BOUND
    L = lib()
    if not _BOUND:
        vp, sz, cp = C.c_void_p, C.c_size_t, C.c_char_p
        fp = C.POINTER(C.c_float)
        L.kg_supervisor_create.argtypes = [C.POINTER(_Cfg), C.POINTER(vp)]
        for f in ("kg_supervisor_destroy", "kg_supervisor_synchronize"):
            getattr(L, f).argtypes = [vp]
        L.kg_supervisor_hyperparameter_count.argtypes = [vp, C.POINTER(sz)]
        L.kg_supervisor_set_training_data.argtypes = [vp, fp, fp]
        L.kg_supervisor_train.argtypes = [vp, sz, fp]
        L.kg_supervisor_forward.argtypes = [vp, fp, sz, fp]
        L.kg_supervisor_backward_direct.argtypes = [vp, fp]
        L.kg_supervisor_field_size.argtypes = [vp, cp, C.POINTER(sz), C.POINTER(sz)]
        L.kg_supervisor_get_field.argtypes = [vp, cp, vp, sz]
        L.kg_supervisor_set_field.argtypes = [vp, cp, vp, sz]
        L.kg_supervisor_get_scalar.argtypes = [vp, cp, C.POINTER(C.c_double)]
        L.kg_supervisor_set_scalar.argtypes = [vp, cp, C.c_double]
        L.kg_supervisor_profile.argtypes = [vp, C.c_int]
        L.kg_supervisor_profile_read.argtypes = [vp, cp, C.POINTER(C.c_double), C.POINTER(sz)]
        _BOUND = True
    return L


def _fptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


class SupervisorDevice:
    """One DeepSupervisor learner on one GPU.

    `layers` lists the network after the input, in the reference's JSON form:
    {"Type": "Layer/Linear", "Output Channels": n} and {"Type":
    "Layer/Activation", "Function": name, "Alpha": a, "Beta": b}; the last
    Linear (solution_size channels) and an output activation are part of the
    list.  Layer numbers in field names count the input as layer 0."""

    def __init__(self, input_size, solution_size, layers, training_batch_size, inference_batch_size=None,
                 output_scale=None, output_shift=None, output_mask=None, optimizer="Adam",
                 loss="Mean Squared Error", learning_rate=1e-3, l2_enabled=False, l2_importance=0.0, device=0,
                 hyperparameters=None):
        L = _lib()
        if optimizer not in OPTIMIZERS:
            raise KoraliDeviceError(f"Optimizer '{optimizer}' is not one of {sorted(OPTIMIZERS)}")
        if loss not in LOSSES:
            raise KoraliDeviceError(f"Loss Function '{loss}' is not one of {sorted(LOSSES)}")
        arr = (_Layer * len(layers))()
        for i, ly in enumerate(layers):
            if ly["Type"] == "Layer/Linear":
                arr[i] = _Layer(0, int(ly["Output Channels"]), 0, 0.0, 0.0)
            elif ly["Type"] == "Layer/Activation":
                if ly["Function"] not in FUNCTIONS:
                    raise KoraliDeviceError(f"Activation function '{ly['Function']}' is not provided")
                arr[i] = _Layer(1, 0, FUNCTIONS[ly["Function"]], float(ly.get("Alpha", 1.0)), float(ly.get("Beta", 0.0)))
            else:
                raise KoraliDeviceError(f"Layer type '{ly['Type']}' is not provided")
        self.I, self.O = int(input_size), int(solution_size)
        self.N = int(training_batch_size)
        self.NI = self.N if inference_batch_size is None else int(inference_batch_size)
        self.optimizer = optimizer
        self._keep = [arr]

        def vec(a, dt, what):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dt)
            if a.shape != (self.O,):
                raise KoraliDeviceError(f"{what}: expected {self.O} values, provided {a.size}")
            self._keep.append(a)
            return a

        sc, sh = vec(output_scale, np.float32, "output_scale"), vec(output_shift, np.float32, "output_shift")
        mk = None if output_mask is None else vec([MASKS[m] for m in output_mask], np.int32, "output_mask")
        cfg = _Cfg(self.I, self.O, self.N, self.NI, len(layers), arr,
                   None if sc is None else _fptr(sc), None if sh is None else _fptr(sh),
                   None if mk is None else mk.ctypes.data_as(C.POINTER(C.c_int)), OPTIMIZERS[optimizer], LOSSES[loss],
                   float(learning_rate), int(bool(l2_enabled)), float(l2_importance), device)
        h = C.c_void_p()
        check(L.kg_supervisor_create(C.byref(cfg), C.byref(h)))
        self._h = h
        n = C.c_size_t()
        check(L.kg_supervisor_hyperparameter_count(h, C.byref(n)))
        self.hyperparameter_count = n.value
        if hyperparameters is not None:
            self.set("hyperparameters", hyperparameters)

    def close(self):
        if getattr(self, "_h", None):
            _lib().kg_supervisor_destroy(self._h)
            self._h = None

    __del__ = close

    # ---- fields and scalars
    def field_size(self, name):
        e, c = C.c_size_t(), C.c_size_t()
        check(_lib().kg_supervisor_field_size(self._h, name.encode(), C.byref(e), C.byref(c)))
        return e.value, c.value

    def get(self, name):
        _, n = self.field_size(name)
        a = np.empty(n, np.float32)
        check(_lib().kg_supervisor_get_field(self._h, name.encode(), a.ctypes.data_as(C.c_void_p), a.nbytes))
        return a

    def set(self, name, values):
        a = np.ascontiguousarray(values, dtype=np.float32).ravel()
        check(_lib().kg_supervisor_set_field(self._h, name.encode(), a.ctypes.data_as(C.c_void_p), a.nbytes))

    def scalar(self, name):
        v = C.c_double()
        check(_lib().kg_supervisor_get_scalar(self._h, name.encode(), C.byref(v)))
        return v.value

    def set_scalar(self, name, value):
        check(_lib().kg_supervisor_set_scalar(self._h, name.encode(), float(value)))

    @property
    def hyperparameters(self):
        return self.get("hyperparameters")

    # ---- learner operations
    def set_training_data(self, inputs, solutions):
        X = np.ascontiguousarray(inputs, np.float32).reshape(self.N, self.I)
        S = np.ascontiguousarray(solutions, np.float32).reshape(self.N, self.O)
        check(_lib().kg_supervisor_set_training_data(self._h, _fptr(X), _fptr(S)))

    def train(self, steps=1):
        """`steps` optimisation steps; returns the last step's loss (Mean Squared Error)."""
        loss = C.c_float(0.0)
        check(_lib().kg_supervisor_train(self._h, steps, C.byref(loss)))
        return loss.value

    def forward(self, inputs):
        X = np.ascontiguousarray(inputs, np.float32).reshape(-1, self.I)
        out = np.empty((X.shape[0], self.O), np.float32)
        check(_lib().kg_supervisor_forward(self._h, _fptr(X), X.shape[0], _fptr(out)))
        return out

    def backward_direct(self, gradients):
        G = np.ascontiguousarray(gradients, np.float32).reshape(self.N, self.O)
        check(_lib().kg_supervisor_backward_direct(self._h, _fptr(G)))

    def synchronize(self):
        check(_lib().kg_supervisor_synchronize(self._h))

    def profile(self, enable=True):
        check(_lib().kg_supervisor_profile(self._h, int(bool(enable))))

    def profile_read(self, stage):
        ms, n = C.c_double(), C.c_size_t()
        check(_lib().kg_supervisor_profile_read(self._h, stage.encode(), C.byref(ms), C.byref(n)))
        return ms.value, n.value


__all__ = ["SupervisorDevice", "KoraliDeviceError", "FUNCTIONS", "MASKS", "OPTIMIZERS", "LOSSES", "STATE_FIELDS"]
