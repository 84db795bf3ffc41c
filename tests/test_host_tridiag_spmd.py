"""The multi-threaded host tridiagonalisation's protocol
(korali_amd/csrc/kg_host_tridiag.cpp: every thread runs the whole step loop
on private vectors; per step only its blocks' sums and the next column cross,
through per-thread parity slots and one flag each) against the oracle's
kr_symmtd_decomp, bit for bit, at the smallest orders where the protocol can
go wrong.  CPU only."""
import numpy as np
import pytest

from test_host_tridiag import _check, _oracle, _spd, _vp


def _device_lib():
    from korali_amd.native import lib
    return lib()


def _assert_equals_oracle(C, H, tau, d, sd):
    N = C.shape[0]
    A, t_ref = _oracle(C)
    assert np.array_equal(d.view(np.uint64), np.diag(A).copy().view(np.uint64))
    assert np.array_equal(sd[:N - 1].view(np.uint64), np.diag(A, -1).copy().view(np.uint64))
    for i in range(N - 2):
        assert np.array_equal(H[i, :N - 1 - i].view(np.uint64), A[i + 1:, i].copy().view(np.uint64)), i
        assert tau[i].tobytes() == t_ref[i].tobytes(), i


def _check_seq(mats):
    """The matrices one after the other on one handle (one pool)."""
    N, K = mats[0].shape[0], len(mats)
    C = np.ascontiguousarray(np.stack(mats))
    H = np.zeros((K, N, N))
    tau, d, sd = np.zeros((K, N)), np.zeros((K, N)), np.zeros((K, N))
    assert _device_lib().kg_debug_host_tridiag_seq(N, K, _vp(C), _vp(H), _vp(tau), _vp(d), _vp(sd)) == 0
    for k in range(K):
        _assert_equals_oracle(mats[k], H[k], tau[k], d[k], sd[k])


def _zero_columns(N, seed, cols):
    C = _spd(N, seed)
    for z in cols:
        C[:, z] = C[z, :] = 0.0
        C[z, z] = 2.0
    return C


def test_one_block_caps_to_one_thread(monkeypatch):
    monkeypatch.setenv("KORALI_AMD_HOST_TRIDIAG_THREADS", "2")
    _check(_spd(8, 8))
    _check_seq([_spd(8, 1), _spd(8, 2)])


@pytest.mark.parametrize("N", [9, 16])
def test_two_blocks_two_threads(monkeypatch, N):
    """threads <= ceil(N / 8); thread 0's only block empties at step 7 and it
    goes on publishing"""
    monkeypatch.setenv("KORALI_AMD_HOST_TRIDIAG_THREADS", "4")  # (capped to 2)
    _check(_spd(N, N))
    monkeypatch.setenv("KORALI_AMD_HOST_TRIDIAG_THREADS", "2")
    _check(_spd(N, N + 1))
    _check_seq([_spd(N, 3), _spd(N, 4)])


CASES = [(N, P) for N in (17, 24, 25) for P in (2, 3, 4)] + [(33, 5)] + [(N, P) for N in (127, 128, 129) for P in (4, 8)]


@pytest.mark.parametrize("N,threads", CASES)
def test_spmd_matches_oracle_bit_exact(monkeypatch, N, threads):
    monkeypatch.setenv("KORALI_AMD_HOST_TRIDIAG_THREADS", str(threads))
    C = _spd(N, 100 * N + threads)
    C[np.triu_indices(N, 1)] = np.nan  # only the lower triangle is read
    _check(C)


@pytest.mark.parametrize("N,threads", CASES)
def test_spmd_zero_columns(monkeypatch, N, threads):
    """tau = 0 steps between ordinary ones: every thread takes that branch
    alike and the pending update is dropped afterwards"""
    monkeypatch.setenv("KORALI_AMD_HOST_TRIDIAG_THREADS", str(threads))
    z = N // 2
    _check(_zero_columns(N, N + threads, [z]))
    _check(_zero_columns(N, N + threads + 1, [z, z + 1]))


@pytest.mark.parametrize("N,threads", CASES)
def test_spmd_scales(monkeypatch, N, threads):
    monkeypatch.setenv("KORALI_AMD_HOST_TRIDIAG_THREADS", str(threads))
    _check(_spd(N, 7 * N + threads, scale=1e-150))
    _check(_spd(N, 9 * N + threads, scale=1e150))


@pytest.mark.parametrize("N,threads", CASES)
def test_spmd_two_decompositions_on_one_handle(monkeypatch, N, threads):
    """the parity slots and the flags start clean: a second, different matrix
    (and a third with tau = 0 steps) on the same pool"""
    monkeypatch.setenv("KORALI_AMD_HOST_TRIDIAG_THREADS", str(threads))
    _check_seq([_spd(N, 11 * N + threads), _spd(N, 13 * N + threads, scale=3.0),
                _zero_columns(N, 17 * N + threads, [N // 2, N // 2 + 1])])
