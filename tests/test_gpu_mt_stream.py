"""The device mt19937 stream (korali_amd/csrc/kg_rng.hip MtStream) with no
solver around it, through the kg_debug_mt_* entries, against one sequential
GSL generator (oracle/refcpu.py Rng) started from the same 5000-byte state.
The states come from tests/mt_states.py: the recurrence run backwards puts a
zero word (which gsl_rng_uniform_pos skips and gsl_rng_uniform does not) or a
0x80000000 pair (r2 == 0) wherever a case needs one.  Every comparison is on
the bits; buffers are handed in full of a sentinel, and what a call does not
write must still hold it.  Cases (a) to (l) as in the stream's test plan;
each runs with the serial producer (the default) and with the chunked one
(KORALI_AMD_MT_PARALLEL_MIN=0, KORALI_AMD_MT_CHUNK_LOG2=15) unless it says
otherwise."""
import bisect
import ctypes as C
import functools

import numpy as np
import pytest

import mt_states as S

pytestmark = pytest.mark.gpu

SENT = -7.25e77                     # no normal, no uniform
BE_SENT = 0xDEADBEEFDEADBEEF
ERR_UNDERRUN, ERR_ZERO_LIST = 1 << 1, 1 << 3  # csrc/kg_common.hpp KG_ERR_*
ENV = ("KORALI_AMD_MT_PARALLEL_MIN", "KORALI_AMD_MT_CHUNK_LOG2", "KORALI_AMD_MT_CHUNK_PARTS")
WAVE_ATTEMPTS, BLOCK_ATTEMPTS = 64 * 8, 256 * 8  # attempts a wave / a workgroup of the polar passes holds


@pytest.fixture(params=["serial", "chunked"])
def mode(request, monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    if request.param == "chunked":
        monkeypatch.setenv("KORALI_AMD_MT_PARALLEL_MIN", "0")
        monkeypatch.setenv("KORALI_AMD_MT_CHUNK_LOG2", "15")
    return request.param


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def capacity(M):
    """ring words for draws of M normals, sized as the solvers size theirs"""
    return 4 * M + 16384


class Stream:
    """one kg_debug_mt handle; every call asserts a zero return"""

    def __init__(self, state, capacity_words):
        from korali_amd.native import lib
        self.L = lib()
        self.h = C.c_void_p()
        rc = self.L.kg_debug_mt_open(0, capacity_words, state, C.byref(self.h))
        assert rc == 0, self.L.kg_last_error()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.L.kg_debug_mt_close(self.h)
        self.h = None

    def reimport(self, state):
        assert self.L.kg_debug_mt_import(self.h, state) == 0, self.L.kg_last_error()

    def count_blocks(self, M):
        nb = C.c_size_t()
        assert self.L.kg_debug_mt_count_blocks(self.h, M, C.byref(nb)) == 0
        return nb.value

    def polar(self, M, block_len=0, k_lo=0, k_hi=None, pad=64):
        """(the window's normals, block_end, count blocks); `pad` sentinels
        after the window and every unwritten block_end entry are checked"""
        n = max(0, min(M, M if k_hi is None else k_hi) - k_lo)
        z = np.full(n + pad, SENT)
        be = np.full(M // block_len, BE_SENT, dtype=np.uint64) if block_len else None
        nb = C.c_size_t()
        rc = self.L.kg_debug_mt_polar_normals(self.h, M, block_len, k_lo, 2 ** 64 - 1 if k_hi is None else k_hi,
                                              _vp(z), len(z), _vp(be), C.byref(nb))
        assert rc == 0, self.L.kg_last_error()
        assert np.array_equal(bits(z[n:]), bits(np.full(pad, SENT))), "wrote past the window"
        return z[:n], be, nb.value

    def consume(self, used, block_len=0, use_block_end=False):
        rc = self.L.kg_debug_mt_consume_normals(self.h, used, block_len, 1 if use_block_end else 0)
        assert rc == 0, self.L.kg_last_error()

    def consume_dev(self, used_blocks, block_len):
        assert self.L.kg_debug_mt_consume_normals_dev(self.h, used_blocks, block_len) == 0, self.L.kg_last_error()

    def uniforms(self, M, peek=False):
        u = np.full(M + 8, SENT)
        f = self.L.kg_debug_mt_peek_uniforms if peek else self.L.kg_debug_mt_uniforms
        assert f(self.h, M, _vp(u)) == 0, self.L.kg_last_error()
        assert np.all(u[M:] == SENT)
        return u[:M]

    def consume_words(self, words):
        assert self.L.kg_debug_mt_consume_words_dev(self.h, words) == 0, self.L.kg_last_error()

    def prefetch(self, M):
        assert self.L.kg_debug_mt_prefetch(self.h, M) == 0, self.L.kg_last_error()

    def polar_ahead(self, M, block_len=0):
        z = np.full(M + 64, SENT)
        launched = C.c_int(-1)
        rc = self.L.kg_debug_mt_polar_normals_ahead(self.h, M, block_len, _vp(z), len(z), C.byref(launched))
        assert rc == 0, self.L.kg_last_error()
        return launched.value

    def join(self, M=None):
        if M is None:
            assert self.L.kg_debug_mt_join(self.h, None, 0) == 0, self.L.kg_last_error()
            return None
        z = np.zeros(M + 64)
        assert self.L.kg_debug_mt_join(self.h, _vp(z), len(z)) == 0, self.L.kg_last_error()
        assert np.all(z[M:] == SENT), "wrote past the draw"
        return z[:M]

    def export(self):
        buf = C.create_string_buffer(5000)
        assert self.L.kg_debug_mt_export_gsl(self.h, buf) == 0, self.L.kg_last_error()
        return buf.raw

    def state(self):
        out = np.zeros(7, dtype=np.uint64)
        ring = C.c_ulonglong()
        assert self.L.kg_debug_mt_state(self.h, _vp(out), C.byref(ring)) == 0, self.L.kg_last_error()
        d = dict(zip(("lo", "pos", "hi", "nzero", "errors", "last_attempt", "total_normals"), (int(v) for v in out)))
        d["ring"] = ring.value
        return d


@functools.lru_cache(maxsize=None)
def reference(state, M):
    """the oracle's M normals from `state`, the attempt index of each and the
    words drawn through each (computed once per state, left unchanged)"""
    z, after = S.gaussians(state, M)
    attempts, words = S.polar_attempts_np(state, M)
    z.setflags(write=False)
    return z, after, attempts, words


@functools.lru_cache(maxsize=None)
def after_normals(state, n):
    return state if n == 0 else S.gaussians(state, n)[1]


def after_words(state, n):
    r = S.rng_of(state)
    u = np.array([r.get() / 4294967296.0 for _ in range(n)])
    return u, r.get_bytes()


def pending_zeros(want, st):
    """zero words the device has recorded: those in [pos, hi)"""
    return sum(1 for p, v in want.items() if v == 0 and st["pos"] <= S.MTI + p < st["hi"])


# ---------------------------------------------------------------- (a) zeros
@pytest.mark.parametrize("name", sorted(S.case_a()))
def test_a_zero_words_in_the_imported_block(mode, name):
    want, st0 = S.case_a()[name]
    M = 300
    zref, _, attempts, words = reference(st0, M)
    first_zero = min(want)
    useds = [1, M]
    if first_zero in words:  # a normal whose last word immediately precedes the zero word
        useds.append(int(np.flatnonzero(words == first_zero)[0]) + 1)
    assert (len(useds) == 3) == (name in ("both_of_attempt", "word_623", "words_623_624"))
    with Stream(st0, capacity(M)) as s:
        for i, used in enumerate(useds):
            if i:
                s.reimport(st0)
            z, be, _ = s.polar(M, block_len=1)
            assert np.array_equal(bits(z), bits(zref))
            assert np.array_equal(be, attempts.astype(np.uint64))
            st = s.state()
            assert st["errors"] == 0 and st["nzero"] == pending_zeros(want, st)
            assert st["last_attempt"] == attempts[-1] and st["total_normals"] >= M
            s.consume(used, 1, True)
            exported = s.export()
            assert exported == after_normals(st0, used)
            if i == 2:  # the zero word stays unconsumed: gsl_rng_uniform returns it
                mt, mti = S.state_words(exported)
                assert mti == S.MTI + first_zero and mt[mti] == 0
                u = s.uniforms(2)
                uref, after = after_words(exported, 2)
                assert u[0] == 0.0 and np.array_equal(bits(u), bits(uref))
                assert s.export() == after
                assert s.state()["errors"] == 0


def test_a_zero_word_below_mti_is_not_recorded(mode):
    want, st0 = S.case_a_below_mti()
    M = 300
    zref, after, attempts, _ = reference(st0, M)
    with Stream(st0, capacity(M)) as s:
        assert s.state()["nzero"] == 0
        z, be, _ = s.polar(M, block_len=1)
        assert s.state()["nzero"] == 0 and s.state()["errors"] == 0
        assert np.array_equal(bits(z), bits(zref)) and np.array_equal(be, attempts.astype(np.uint64))
        s.consume(M)
        assert s.export() == after


# ------------------------------------------------------------- (b) r2 == 0
@pytest.mark.parametrize("name", sorted(S.case_b()))
def test_b_attempt_with_r2_zero_is_rejected(mode, name):
    want, st0 = S.case_b()[name]
    M = 600
    zref, after, attempts, _ = reference(st0, M)
    assert min(want) // 2 not in attempts
    with Stream(st0, capacity(M)) as s:
        z, be, _ = s.polar(M, block_len=1)
        assert np.array_equal(bits(z), bits(zref)) and np.array_equal(be, attempts.astype(np.uint64))
        s.consume(M)
        assert s.export() == after and s.state()["errors"] == 0


# ------------------------------------------- (c) zeros at each recording site
@pytest.mark.parametrize("name", sorted(S.case_c()))
def test_c_zero_words_the_device_records(mode, name):
    want, st0 = S.case_c()[name]
    M = 30000
    zref, after, attempts, words = reference(st0, M)
    assert words[-1] > max(want)  # the draw reaches past every zero word
    with Stream(st0, capacity(M)) as s:
        z, _, _ = s.polar(M)
        assert np.array_equal(bits(z), bits(zref))
        st = s.state()
        assert st["hi"] >= S.MTI + words[-1] and st["errors"] == 0
        assert st["nzero"] == pending_zeros(want, st) > 0
        assert st["last_attempt"] == attempts[-1]
        s.consume(M)
        assert s.export() == after
        st = s.state()
        assert st["errors"] == 0 and st["nzero"] == pending_zeros(want, st)


# ------------------------------------------------- (d) zero-list capacity
def test_d_exactly_64_pending_zeros(mode):
    want, st0 = S.case_d()["exactly_64"]
    M = 300
    zref, after, attempts, _ = reference(st0, M)
    with Stream(st0, capacity(M)) as s:
        assert s.state()["nzero"] == 64 and s.state()["errors"] == 0
        z, be, _ = s.polar(M, block_len=1)
        assert np.array_equal(bits(z), bits(zref)) and np.array_equal(be, attempts.astype(np.uint64))
        assert s.state()["errors"] == 0
        s.consume(M)
        assert s.export() == after
        assert s.state()["errors"] == 0 and s.state()["nzero"] == 0


def test_d_65_imported_zeros_set_the_flag(mode):
    """(import_gsl stopped recording at 64 without a word: the flag is new)"""
    want, st0 = S.case_d()["imported_65"]
    with Stream(st0, capacity(300)) as s:
        s.polar(300)  # returns normally; its normals are not the reference's
        assert s.state()["errors"] & ERR_ZERO_LIST


def test_d_65th_zero_made_on_the_device_sets_the_flag(mode):
    want, st0 = S.case_d()["device_65th"]
    with Stream(st0, capacity(300)) as s:
        st = s.state()
        if st["hi"] <= 700:  # (the chunked import has produced it already)
            assert st["nzero"] == 64 and st["errors"] == 0
        s.polar(300)
        assert s.state()["errors"] & ERR_ZERO_LIST


# ------------------------------------------- (e) scan past 1024 count blocks
@pytest.mark.parametrize("producer", ["serial", "chunked_default"])
def test_e_scan_beyond_1024_count_blocks(producer, monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    if producer == "serial":
        monkeypatch.setenv("KORALI_AMD_MT_PARALLEL_MIN", str(1 << 40))
    st0 = S.plain_states()["e"][0]
    with Stream(st0, 8 << 20) as s:
        lo, hi = 1, 1 << 22  # the smallest M whose draw launches more than 1024 count blocks, from the entry
        assert s.count_blocks(hi) > 1024
        while lo < hi:
            mid = (lo + hi) // 2
            lo, hi = (lo, mid) if s.count_blocks(mid) > 1024 else (mid + 1, hi)
        M = lo
        assert s.count_blocks(M) == 1025 and s.count_blocks(M - 1) == 1024
        # one reference for this draw and the longer one below
        big = M + 16384
        zref, _, attempts, words = reference(st0, big)
        assert words[-1] <= S.plain_states()["e"][1]
        after = after_normals(st0, M)
        z, _, nb = s.polar(M)
        assert nb > 1024
        assert np.array_equal(bits(z), bits(zref[:M]))
        st = s.state()
        assert st["last_attempt"] == attempts[M - 1] and st["errors"] == 0
        s.consume(M)
        assert s.export() == after
        # The first normal of count block 1024, from the oracle's accepts.  The draw's 12-sigma margin of
        # attempts puts it past the smallest M (block 1024 holds spare attempts only there), so the window
        # run draws M2 > k normals: block 1024's normals are written, at the offset the second scan pass gave.
        k = bisect.bisect_left(attempts, 1024 * BLOCK_ATTEMPTS)
        assert M <= k and k + 4096 <= big
        M2 = k + 4096
        for k_lo, k_hi in ((k - 2048, k + 2048), (0, None)):
            s.reimport(st0)
            z, _, nb = s.polar(M2, k_lo=k_lo, k_hi=k_hi)
            assert nb > 1024 and np.array_equal(bits(z), bits(zref[k_lo:M2 if k_hi is None else k_hi]))
            st = s.state()
            assert st["last_attempt"] == attempts[M2 - 1] and st["errors"] == 0
            s.consume(M2)
            assert s.export() == after_normals(st0, M2)


# --------------------------------------------------------------- (f) windows
def test_f_windows(mode):
    st0 = S.plain_states()["f"][0]
    M = 5000
    zref, after, attempts, _ = reference(st0, M)
    kw = bisect.bisect_left(attempts, 3 * WAVE_ATTEMPTS)  # wave 3 of block 0: its first normal
    kb = bisect.bisect_left(attempts, BLOCK_ATTEMPTS)     # block 1: its first normal
    assert 100 < kw < kb < M - 100
    windows = [(0, 1), (M - 1, M), (1234, 1234), (0, 10 ** 9), (M, M + 5)]
    for base in (kw, kb):
        for e in (base - 1, base, base + 1):
            windows += [(e - 37, e), (e, e + 37)]
    with Stream(st0, capacity(M)) as s:
        z, _, _ = s.polar(M)
        assert np.array_equal(bits(z), bits(zref))
        full = s.state()
        assert full["last_attempt"] == attempts[-1]
        for k_lo, k_hi in windows:
            s.reimport(st0)
            z, _, _ = s.polar(M, k_lo=k_lo, k_hi=k_hi)
            assert np.array_equal(bits(z), bits(zref[k_lo:min(k_hi, M)])), (k_lo, k_hi)
            st = s.state()
            assert (st["last_attempt"], st["total_normals"]) == (full["last_attempt"], full["total_normals"])
            s.consume(M)
            assert s.export() == after, (k_lo, k_hi)
            assert s.state()["errors"] == 0


# ---------------------------------------------------------------- (g) blocks
@pytest.mark.parametrize("block_len", [1, 7, 64, 4096])
def test_g_blocks(mode, block_len):
    st0 = S.plain_states()["g"][0]
    M = 4096
    zref, after, attempts, _ = reference(st0, M)
    nblk = M // block_len
    want_be = np.array([attempts[(b + 1) * block_len - 1] for b in range(nblk)], dtype=np.uint64)
    assert nblk == {1: 4096, 7: 585, 64: 64, 4096: 1}[block_len]
    with Stream(st0, capacity(M)) as s:
        for used_blocks in sorted({0, 1, nblk // 2, nblk}):
            s.reimport(st0)
            z, be, _ = s.polar(M, block_len=block_len)
            assert np.array_equal(bits(z), bits(zref))
            assert len(be) == nblk and np.array_equal(be, want_be)  # (no entry for a partial block)
            s.consume_dev(used_blocks, block_len)
            assert s.export() == after_normals(st0, used_blocks * block_len), used_blocks
            assert s.state()["errors"] == 0
        if M % block_len == 0:  # block_end's last entry and the pass's own record of normal M - 1
            s.reimport(st0)
            s.polar(M, block_len=block_len)
            s.consume(M, block_len, True)
            assert s.export() == after
            s.reimport(st0)
            s.polar(M, block_len=block_len)
            s.consume(M)
            assert s.export() == after


# -------------------------------------------------------------- (h) uniforms
COUNTS = (1, 255, 256, 257, 623, 624, 625)


@pytest.mark.parametrize("mti", [0, 1, 623, 624])
def test_h_uniforms(mode, mti):
    st0 = S.plain_states()["h_%d" % mti][0]
    assert S.state_words(st0)[1] == mti
    uref, _ = after_words(st0, max(COUNTS))
    with Stream(st0, 16384) as s:
        assert s.export() == st0  # mti of 0 and 624 come back as imported
        for n in COUNTS:
            s.reimport(st0)
            u = s.uniforms(n)
            assert np.array_equal(bits(u), bits(uref[:n])), n
            exported = s.export()
            assert exported == after_words(st0, n)[1], n
            if (mti + n) % 624 == 0:  # consumed exactly to a block's end: GSL leaves mti == 624
                assert S.state_words(exported)[1] == 624
            for w in (0, 1, n):
                s.reimport(st0)
                u = s.uniforms(n, peek=True)
                assert np.array_equal(bits(u), bits(uref[:n])), n
                s.consume_words(w)
                assert s.export() == after_words(st0, w)[1], (n, w)
        assert s.state()["errors"] == 0


def test_h_interleaved_uniforms_and_normals(mode):
    st0 = S.plain_states()["h_mixed"][0]
    r = S.rng_of(st0)
    with Stream(st0, capacity(50)) as s:
        u = s.uniforms(100, peek=True)
        s.consume_words(37)
        peeked = np.array([r.get() / 4294967296.0 for _ in range(37)])
        assert np.array_equal(bits(u[:37]), bits(peeked))
        z, _, _ = s.polar(50)
        s.consume(50)
        assert np.array_equal(bits(z), bits(np.array([r.gaussian() for _ in range(50)])))
        u = s.uniforms(3)
        assert np.array_equal(bits(u), bits(np.array([r.flat(0.0, 1.0) for _ in range(3)])))
        assert s.export() == r.get_bytes() and s.state()["errors"] == 0


# ------------------------------------------------------------ (i) small ring
def test_i_small_ring_wraps(mode):
    st0 = S.plain_states()["i"][0]
    M = 300
    cap = 1329  # words_for_normals(300) + 128: what one draw asks the producer for
    draws = 40 if mode == "serial" else 130
    _, _, _, words = reference(st0, M * draws)
    with Stream(st0, cap) as s:
        R_ = s.state()["ring"]
        if mode == "serial":
            assert R_ == 8192
        # the oracle's block start after each draw; some draw ends in a block that straddles the ring's end
        pos = [S.MTI + int(words[M * (d + 1) - 1]) for d in range(draws)]
        los = [624 * ((p - 1) // 624) for p in pos]
        assert any(lo % R_ > R_ - 624 for lo in los)
        cur, wrapped = st0, 0
        for d in range(draws):
            zref, cur = S.gaussians(cur, M)
            z, _, _ = s.polar(M)
            assert np.array_equal(bits(z), bits(zref)), d
            s.consume(M)
            st = s.state()
            assert (st["lo"], st["pos"]) == (los[d], pos[d]) and st["errors"] == 0
            wrapped += st["lo"] % R_ > R_ - 624
            assert s.export() == cur, d
        assert wrapped >= 1


# ----------------------------------------------------------- (j) side stream
@pytest.mark.parametrize("which", ["plain", "zero_words"])
def test_j_side_stream(mode, which):
    st0 = S.plain_states()["j"][0] if which == "plain" else S.case_a()["both_of_attempt"][1]
    M = 300
    zref, after, _, _ = reference(st0, M)
    with Stream(st0, capacity(M)) as s:
        assert s.polar_ahead(M) == 0  # no side stream yet: nothing launched
        s.prefetch(M)
        z, _, _ = s.polar(M)
        assert np.array_equal(bits(z), bits(zref))
        s.consume(M)
        assert s.export() == after
        s.reimport(st0)
        s.prefetch(M)
        assert s.polar_ahead(M) == 1
        z = s.join(M)
        assert np.array_equal(bits(z), bits(zref))
        s.consume(M)
        assert s.export() == after and s.state()["errors"] == 0


# ------------------------------------------------------------- (k) re-import
def test_k_reimport_on_a_used_handle(mode):
    M = 30000
    _, st1 = S.case_c()["chunk_edge"]
    want2, st2 = S.case_c()["rolling_tail"]
    zref, after, attempts, _ = reference(st2, M)
    with Stream(st2, capacity(M)) as fresh:
        zf, _, _ = fresh.polar(M)
        fresh_state = fresh.state()
    with Stream(st1, capacity(M)) as s:
        z1, _, _ = s.polar(M)
        assert np.array_equal(bits(z1), bits(reference(st1, M)[0]))
        s.consume(M)
        s.prefetch(M)  # left pending: the import must not let it extend the new state
        s.reimport(st2)
        z, _, _ = s.polar(M)
        assert np.array_equal(bits(z), bits(zref)) and np.array_equal(bits(z), bits(zf))
        assert s.state() == fresh_state
        s.consume(M)
        assert s.export() == after and s.state()["errors"] == 0


# ----------------------------------------------------------- (l) host checks
@pytest.mark.parametrize("mti", [-1, 625])
def test_l_mti_out_of_range_is_refused(mti):
    from korali_amd.native import lib
    mt, _ = S.state_words(S.with_words_at({}, 0, 90))
    h = C.c_void_p()
    assert lib().kg_debug_mt_open(0, 16384, S.state_bytes(mt, mti), C.byref(h)) != 0
    assert not h.value and b"mti" in lib().kg_last_error()
    with Stream(S.with_words_at({}, 0, 90), 16384) as s:
        before = s.export()
        assert lib().kg_debug_mt_import(s.h, S.state_bytes(mt, mti)) != 0
        assert s.export() == before  # the refused import left the stream alone


def test_l_request_beyond_the_ring_sets_underrun(mode):
    with Stream(S.plain_states()["l"][0], 1329) as s:
        R_ = s.state()["ring"]
        assert s.state()["errors"] == 0
        s.uniforms(R_ + 1, peek=True)  # returns; the words past the ring are not the stream's
        assert s.state()["errors"] & ERR_UNDERRUN
