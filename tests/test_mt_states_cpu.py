"""tests/mt_states.py against the oracle's GSL mt19937 (oracle/refcpu.py Rng):
the states test_gpu_mt_stream.py imports hold the words they were built to
hold, and nothing else that the device treats specially.  CPU only."""
import numpy as np
import pytest

import mt_states as S
import refcpu as R


def test_untemper_inverts_temper():
    rs = np.random.RandomState(5)
    for x in [0, 1, 0x80000000, 0xFFFFFFFF] + [int(v) for v in rs.randint(0, 2 ** 32, size=2000, dtype=np.uint64)]:
        assert S.untemper(S.temper(x)) == x
        assert S.temper(S.untemper(x)) == x
    assert S.temper(0) == 0 and S.untemper(0) == 0  # a zero word is zero before tempering too
    xs = rs.randint(0, 2 ** 32, size=64, dtype=np.uint64).astype(np.uint32)
    assert [S.temper(x) for x in xs] == [int(v) for v in S.temper_np(xs)]


@pytest.mark.parametrize("mti", [0, 5, 623, 624])
def test_forward_matches_oracle(mti):
    st = S.with_words_at({}, mti, 3)
    r = S.rng_of(st)
    w = np.array([r.get() for _ in range(3000)], dtype=np.uint32)
    assert np.array_equal(S.temper_np(S.forward(st, 3000)), w)


@pytest.mark.parametrize("name", sorted(S.all_states()))
def test_state_holds_requested_words_and_no_other_zero(name):
    want, st, n = S.all_states()[name]
    mt, mti = S.state_words(st)
    assert mti == S.MTI and len(st) == R.RNG_BYTES
    r = S.rng_of(st)
    w = np.array([r.get() for _ in range(n)], dtype=np.uint32)
    for p, v in want.items():
        if p >= 0:
            assert w[p] == v, (p, v)
        else:  # a word of mt[] below mti: in the state, never drawn
            assert S.temper(mt[mti + p]) == v
    assert sorted(np.flatnonzero(w == 0)) == sorted(p for p, v in want.items() if v == 0 and p >= 0)
    assert np.array_equal(S.temper_np(S.forward(st, n)), w)


@pytest.mark.parametrize("name", sorted(S.plain_states()))
def test_plain_state_has_no_zero_word(name):
    st, n = S.plain_states()[name]
    w = S.temper_np(S.forward(st, n))
    assert len(w) == n and not np.any(w == 0)
    r = S.rng_of(st)
    assert [r.get() for _ in range(700)] == [int(v) for v in w[:700]]


@pytest.mark.parametrize("name", sorted(S.all_states()))
def test_polar_attempts_follows_gaussian(name):
    """after k normals the restated loop has drawn as many words as
    gsl_ran_gaussian did, and left the same state"""
    _, st, _ = S.all_states()[name]
    M = 300
    attempts, words = S.polar_attempts(S.rng_of(st), M)
    assert len(attempts) == M and all(b > a for a, b in zip(attempts, attempts[1:]))
    ref, walk = S.rng_of(st), S.rng_of(st)
    drawn = 0
    for k in range(M):
        ref.gaussian()
        for _ in range(words[k] - drawn):
            walk.get()
        drawn = words[k]
        assert walk.get_bytes() == ref.get_bytes(), k
    acc, wds = S.polar_attempts_np(st, M)
    assert list(acc) == attempts and list(wds) == words


def test_polar_attempts_np_on_a_seeded_state():
    st = S.seeded(790510)
    attempts, words = S.polar_attempts(S.rng_of(st), 5000)
    acc, wds = S.polar_attempts_np(st, 5000)
    assert list(acc) == attempts and list(wds) == words
    z, after = S.gaussians(st, 5000)
    r = S.rng_of(st)
    assert [r.gaussian() for _ in range(5000)] == list(z) and r.get_bytes() == after


def test_case_a_zero_follows_an_accepted_attempt():
    """the states whose test consumes up to the word before a zero word"""
    for name in ("both_of_attempt", "word_623", "words_623_624"):
        want, st = S.case_a()[name]
        p = min(want)
        _, words = S.polar_attempts(S.rng_of(st), 300)
        assert p in words, name
        # gsl_ran_gaussian stops there: the zero word is the next one drawn
        r = S.rng_of(st)
        for _ in range(words.index(p) + 1):
            r.gaussian()
        assert r.get() == 0


def test_case_b_attempt_is_rejected_for_r2_zero():
    for name, (want, st) in S.case_b().items():
        p = min(want)
        assert p % 2 == 0 and want == {p: S.HALF, p + 1: S.HALF}  # words (2a, 2a + 1) of attempt a = p / 2
        attempts, _ = S.polar_attempts(S.rng_of(st), 600)
        assert p // 2 not in attempts and attempts[-1] > p // 2, name


def test_case_d_zero_counts():
    d = S.case_d()
    assert [len(d[k][0]) for k in ("exactly_64", "imported_65", "device_65th")] == [64, 65, 65]
    assert sum(S.MTI + p < 624 for p in d["device_65th"][0]) == 64
