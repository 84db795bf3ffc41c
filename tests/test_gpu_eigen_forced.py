"""Hard covariances teacher-forced through every device eigensolver kernel.

Every other GPU test of the eigendecomposition is a seeded CMA-ES run from
C = I: the kernels see the identity and a few well-conditioned matrices next
to it.  Here one handle per configuration is walked through the families of
eigen_cases.py (graded, clustered, block diagonal, zero columns, 1e-280 and
1e140 scales, indefinite and singular matrices) with
dev["Covariance Matrix"] = M; dev.sample(), against the CPU oracle with the
same assignment and prepare().  Every comparison is equality of bits.

The configurations select the kernels: the five tridiagonalisations (four on
the device, one on the host core), the unpack forms, the host and the device
chase, the streamed and the plain rotation replay.  Every switch is read when
a handle is created; the team, chop-pass and progress-word switches also run
in a child process (this file, started as a script), as when they were
process-wide.  test_eigen_cases_cpu.py pins the families and the oracle's
handling of them on the CPU.
"""
import os
import subprocess
import sys

if __name__ == "__main__":  # the child of test_process_wide_switches: no conftest has set the path
    _ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_ROOT, os.path.join(_ROOT, "oracle"), os.path.join(_ROOT, "tests")]

import numpy as np
import pytest

import eigen_cases as E
import refcpu as R

pytestmark = pytest.mark.gpu

LAM = 8
SEED = 1337
EIGEN = ("Covariance Eigenvector Matrix", "Axis Lengths", "Minimum Covariance Eigenvalue",
         "Maximum Covariance Eigenvalue", "Eigen Failures", "Sample Population")
STATE = ("Current Mean", "Previous Mean", "Evolution Path", "Conjugate Evolution Path",
         "Conjugate Evolution Path L2 Norm", "Covariance Matrix", "Covariance Eigenvector Matrix", "Axis Lengths",
         "Sigma", "Best Ever Value", "Best Ever Variables", "Current Best Value", "Minimum Covariance Eigenvalue",
         "Maximum Covariance Eigenvalue", "Eigen Failures", "Sample Population", "Value Vector")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).reshape(-1).view(np.uint64)


def assert_same_bits(got, want, where):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, where
    if not np.array_equal(g, w):
        bad = np.flatnonzero(g != w)
        i = int(bad[0])
        raise AssertionError("%s: %d of %d elements differ, first at %d: device %r, oracle %r"
                             % (where, bad.size, g.size, i, float(np.asarray(got).reshape(-1)[i]),
                                float(np.asarray(want).reshape(-1)[i])))


def pair(N, lam=LAM, chase="host", diagonal=False):
    from korali_amd.native import CmaesDevice
    o = R.CMAES(N, lam, 0)
    o["Initial Value"] = np.zeros(N)
    o["Initial Standard Deviation"] = np.ones(N)
    if diagonal:
        o.option("Diagonal Covariance", 1)
    R.lib().kr_rng_seed(o.rng(0).ptr, SEED)
    R.lib().kr_rng_seed(o.rng(1).ptr, SEED + 1)
    dev = CmaesDevice(N, lam, initial_value=np.zeros(N), initial_std=np.ones(N), normal_seed=SEED,
                      uniform_seed=SEED + 1, cov_mode="exact", eigen_chase=chase, diagonal=diagonal)
    return o, dev


def forced_step(o, dev, M, fails, where):
    """C = M on both sides, one decomposition and draw, everything compared;
    synchronize() raises on a device error flag"""
    B0, D0 = dev["Covariance Eigenvector Matrix"], dev["Axis Lengths"]
    f0 = dev["Eigen Failures"][0]
    o["Covariance Matrix"] = M
    dev["Covariance Matrix"] = M
    o.prepare()
    dev.sample()
    dev.synchronize()
    for key in EIGEN:
        assert_same_bits(dev[key], o[key], "%s, %s" % (where, key))
    if fails:
        assert_same_bits(dev["Covariance Eigenvector Matrix"], B0, where + ", B kept after the failure")
        assert_same_bits(dev["Axis Lengths"], D0, where + ", D kept after the failure")
    assert dev["Eigen Failures"][0] == f0 + (1.0 if fails else 0.0), where


def walk(N, chase="host", device_tridiag=None):
    """One handle through E.WALK.  device_tridiag: True / False asserts, through
    the profile counters, that every tridiagonalisation ran on the device / on
    the host core."""
    o, dev = pair(N, chase=chase)
    try:
        o.initialize()
        dev.initialize()
        if device_tridiag is not None:
            dev.profile()
        for kind in E.WALK:
            forced_step(o, dev, E.family(kind, N), kind in E.FAILING, "N=%d %s chase, %s" % (N, chase, kind))
        assert dev.get_rng(0) == o.rng(0).get_bytes(), "N=%d %s chase, Normal generator state" % (N, chase)
        assert dev["Eigen Failures"][0] == float(len(E.FAILING))
        if device_tridiag is not None:
            on_device, on_host = dev.profile_read("eigen_tridiag")[1], dev.profile_read("eigen_tridiag_host")[1]
            want = (len(E.WALK), 0) if device_tridiag else (0, len(E.WALK))
            assert (on_device, on_host) == want, "N=%d: tridiagonalisations on the device %d, on the host %d" % (
                N, on_device, on_host)
    finally:
        dev.close()


# every switch that selects an eigensolver kernel: a test sets exactly its own
SWITCHES = ("KORALI_AMD_TRIDIAG", "KORALI_AMD_SQ_DPP", "KORALI_AMD_EIGEN_MW_MIN", "KORALI_AMD_UNPACK",
            "KORALI_AMD_UNPACK_ALLH", "KORALI_AMD_EIGEN_CHASE", "KORALI_AMD_HOST_TRIDIAG_MAX", "KORALI_AMD_TMW_ROWS",
            "KORALI_AMD_APPLY_TEAM", "KORALI_AMD_CHASE_FUSED", "KORALI_AMD_CHASE_PUBLISH_EVERY")


def setenv(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


# ------------------------------------------------- per-handle configurations

@pytest.mark.parametrize("N", [3, 4, 5, 16, 17, 63, 64, 65, 127, 128, 129, 200])
def test_default_host_tridiag_host_chase_streamed_apply(monkeypatch, N):
    setenv(monkeypatch, {})
    walk(N, device_tridiag=False)


@pytest.mark.parametrize("N", [1, 2])
def test_default_below_three_takes_the_device_path(monkeypatch, N):
    """the host tridiagonalisation needs N >= 3: k_tridiag, k_unpack"""
    setenv(monkeypatch, {})
    walk(N, device_tridiag=True)


@pytest.mark.parametrize("N", [3, 5, 17, 64, 65, 127, 128])
@pytest.mark.parametrize("dpp", ["0", "1"])
def test_tridiag_sq(monkeypatch, dpp, N):
    setenv(monkeypatch, {"KORALI_AMD_TRIDIAG": "sq", "KORALI_AMD_SQ_DPP": dpp})
    walk(N, device_tridiag=True)


@pytest.mark.parametrize("N", [3, 17, 64, 95])
def test_tridiag_lds(monkeypatch, N):
    setenv(monkeypatch, {"KORALI_AMD_TRIDIAG": "lds"})
    walk(N, device_tridiag=True)


@pytest.mark.parametrize("N", [17, 65, 129, 200])
@pytest.mark.parametrize("dpp", ["0", "1"])
def test_tridiag_mw2(monkeypatch, dpp, N):
    setenv(monkeypatch, {"KORALI_AMD_TRIDIAG": "mw2", "KORALI_AMD_SQ_DPP": dpp})
    walk(N, device_tridiag=True)


@pytest.mark.parametrize("N", [5, 17, 129])
def test_tridiag_mw(monkeypatch, N):
    setenv(monkeypatch, {"KORALI_AMD_TRIDIAG": "mw"})
    walk(N, device_tridiag=True)


@pytest.mark.parametrize("N", [5, 17, 129])
@pytest.mark.parametrize("allh", [None, "0"])
def test_multi_workgroup_unpack(monkeypatch, allh, N):
    """KORALI_AMD_EIGEN_MW_MIN=0 takes the one-workgroup k_unpack away at every
    N: k_unpack_wv up to 128, above it k_unpack_mw with every reflector row in
    LDS, or streamed (KORALI_AMD_UNPACK_ALLH=0).  With the host chase the
    tridiagonalisation stays on the host core."""
    env = {"KORALI_AMD_EIGEN_MW_MIN": "0"}
    if allh is not None:
        env["KORALI_AMD_UNPACK_ALLH"] = allh
    setenv(monkeypatch, env)
    walk(N, device_tridiag=False)


@pytest.mark.parametrize("N", [17, 128])
def test_unpack_mw_where_unpack_wv_is_the_default(monkeypatch, N):
    setenv(monkeypatch, {"KORALI_AMD_UNPACK": "mw", "KORALI_AMD_EIGEN_MW_MIN": "0"})
    walk(N, device_tridiag=False)


@pytest.mark.parametrize("tridiag,N", [(None, N) for N in (1, 2, 3, 17, 65, 128, 129)] +
                         [("sq", N) for N in (3, 17, 65, 128)])
def test_device_chase(monkeypatch, tridiag, N):
    """k_chase and the plain k_apply behind the device's default
    tridiagonalisation for N (k_tridiag below 3, k_tridiag_sq<dpp> up to 128,
    k_tridiag_mw2 above) and behind a forced sq.  sq fits 3 <= N <= 128, where
    it is also the default, so the forced rows take its other form
    (KORALI_AMD_SQ_DPP=0)."""
    setenv(monkeypatch, {} if tridiag is None else {"KORALI_AMD_TRIDIAG": tridiag, "KORALI_AMD_SQ_DPP": "0"})
    walk(N, chase="device", device_tridiag=True)


def test_unknown_tridiag_kind_is_an_error(monkeypatch):
    """A value outside host | sq | mw2 | lds | mw (a removed kernel's name, a
    typo) fails the handle's creation and is quoted in the message."""
    from korali_amd.native import KoraliDeviceError
    setenv(monkeypatch, {"KORALI_AMD_TRIDIAG": "1wg2"})
    with pytest.raises(KoraliDeviceError, match="1wg2"):
        pair(3)


# ------------------------------------------------------ process-wide switches

TEAM_ENVS = [
    {"KORALI_AMD_APPLY_TEAM": "16", "KORALI_AMD_CHASE_FUSED": "0", "KORALI_AMD_CHASE_PUBLISH_EVERY": "3"},
    {"KORALI_AMD_APPLY_TEAM": "16"},
]


@pytest.mark.parametrize("N", [17, 65])
@pytest.mark.parametrize("env", TEAM_ENVS, ids=["team16-unfused-every3", "team16"])
def test_team_and_chase_switches_per_handle(monkeypatch, env, N):
    """The same two environments in this process, after handles created
    without them: the handle reads the switches at its creation."""
    setenv(monkeypatch, env)
    walk(N)


CHILD_WALKS = ((3, "host"), (17, "host"), (65, "host"), (129, "host"), (17, "device"))


def child_main():
    for N, chase in CHILD_WALKS:
        try:
            walk(N, chase=chase)
        except AssertionError as e:
            print("MISMATCH %s" % e, flush=True)
            return 1
        print("walk N=%d %s chase: equal" % (N, chase), flush=True)
    return 0


@pytest.mark.parametrize("env", [
    {"KORALI_AMD_APPLY_TEAM": "16", "KORALI_AMD_CHASE_FUSED": "0", "KORALI_AMD_CHASE_PUBLISH_EVERY": "3"},
    {"KORALI_AMD_APPLY_TEAM": "16"},
], ids=["team16-unfused-every3", "team16"])
def test_process_wide_switches(env):
    """The 16-lane team form of k_apply and the host chase's separate chop pass
    and sparser progress word are read once into statics: a fresh process."""
    child = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    child.update(env)
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__)]
    p = subprocess.run(cmd, env=child, timeout=120, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-4000:]
    assert p.stdout.count("equal") == len(CHILD_WALKS), p.stdout[-4000:]


# ---------------------------------------------------------- the fused hand-off

@pytest.mark.parametrize("N,lam", [(17, 300), (128, 272)])
def test_graded_matrix_through_the_fused_hand_off(monkeypatch, N, lam):
    """From the second update on, C reaches the host through the publish inside
    kg_cmaes_update.  graded set between evaluate and update(3): the matrix
    that update produces and publishes inherits the grading."""
    setenv(monkeypatch, {})
    obj = "rosenbrock"
    o, dev = pair(N, lam=lam)
    try:
        for g in (1, 2):
            o.generation(g, obj)
            dev.generation(g, obj)
        M = E.family("graded", N)
        for g in (3, 4):
            o.prepare()
            o.evaluate(obj)
            dev.sample()
            dev.evaluate(obj)
            if g == 3:
                o["Covariance Matrix"] = M
                dev["Covariance Matrix"] = M
            o.update(g)
            dev.update(g)
            dev.synchronize()
            for key in STATE:
                assert_same_bits(dev[key], o[key], "generation %d, %s" % (g, key))
            assert np.array_equal(dev.sorting_index(), o.sorting_index()), g
        # generation 5 decomposes what update(4) published
        o.generation(5, obj)
        dev.generation(5, obj)
        dev.synchronize()
        for key in STATE:
            assert_same_bits(dev[key], o[key], "generation 5, %s" % key)
        assert dev.get_rng(0) == o.rng(0).get_bytes()
    finally:
        dev.close()


# ----------------------------------------------------------- the diagonal mode

@pytest.mark.parametrize("N", [1, 5, 300])
def test_diagonal_mode(monkeypatch, N):
    """k_eigen_diag reads the diagonal alone: off-diagonal garbage (a NaN and
    an infinity among it) is ignored; a zero or a negative entry is an eigen
    failure that keeps B and D."""
    setenv(monkeypatch, {})
    rng = np.random.default_rng([7, N])
    G = 1e3 * rng.standard_normal((N, N))
    if N > 1:
        G[0, N - 1], G[N - 1, 0] = np.nan, -np.inf
    good = G.copy()
    good[np.diag_indices(N)] = rng.uniform(0.5, 2.0, N)
    zero = good.copy()
    zero[N // 2, N // 2] = 0.0
    negative = good.copy()
    negative[N - 1, N - 1] = -1e-300
    again = G.T.copy()
    again[np.diag_indices(N)] = rng.uniform(1e-3, 1e3, N)
    o, dev = pair(N, diagonal=True)
    try:
        o.initialize()
        dev.initialize()
        for name, M, fails in (("positive", good, False), ("zero entry", zero, True),
                               ("negative entry", negative, True), ("positive again", again, False)):
            forced_step(o, dev, M, fails, "diagonal mode N=%d, %s" % (N, name))
        assert dev["Eigen Failures"][0] == 2.0
        assert dev.get_rng(0) == o.rng(0).get_bytes()
    finally:
        dev.close()


if __name__ == "__main__":
    sys.exit(child_main())
