"""CPU helpers for the device mt19937 stream's tests (test_mt_states_cpu.py,
test_gpu_mt_stream.py): GSL generator states whose output stream holds
chosen words (zero words above all) at chosen positions.

The recurrence s_j = s_{j-227} ^ twist(top(s_{j-624}), low31(s_{j-623}))
is invertible: s_j ^ s_{j-227} gives the top bit of s_{j-624} and the low 31
bits of s_{j-623}.  A 624-word window placed over the target positions is
filled freely and run backwards to the words the state imports.  Only the
window's first word is not free: its low 31 bits follow from the window's own
last word, so all targets of one state lie within 623 consecutive words.
test_mt_states_cpu.py pins every state built here to the oracle's generator.
"""
import functools

import numpy as np

import refcpu as R

N, LAG, MAGIC = 624, 227, 0x9908B0DF
M32 = 0xFFFFFFFF


def temper(y):
    y = int(y) & M32
    y ^= y >> 11
    y ^= (y << 7) & 0x9D2C5680
    y ^= (y << 15) & 0xEFC60000
    y ^= y >> 18
    return y & M32


def untemper(y):
    y = int(y) & M32
    y ^= y >> 18
    x = y
    for _ in range(2):  # y = x ^ ((x << 15) & C): fifteen more bits right per pass
        x = (y ^ ((x << 15) & 0xEFC60000)) & M32
    y = x
    for _ in range(5):  # y = x ^ ((x << 7) & B)
        x = (y ^ ((x << 7) & 0x9D2C5680)) & M32
    y = x
    for _ in range(3):  # y = x ^ (x >> 11)
        x = y ^ (x >> 11)
    return x & M32


def temper_np(s):
    y = s.astype(np.uint64)
    y ^= y >> np.uint64(11)
    y ^= (y << np.uint64(7)) & np.uint64(0x9D2C5680)
    y ^= (y << np.uint64(15)) & np.uint64(0xEFC60000)
    y ^= y >> np.uint64(18)
    return (y & np.uint64(M32)).astype(np.uint32)


def state_bytes(mt, mti):
    b = bytearray(R.RNG_BYTES)
    b[: N * 8] = np.asarray(mt, dtype="<u8").tobytes()
    b[N * 8: N * 8 + 4] = np.int32(mti).tobytes()
    return bytes(b)


def state_words(state):
    mt = np.frombuffer(state[: N * 8], dtype="<u8").astype(np.uint32)
    mti = int(np.frombuffer(state[N * 8: N * 8 + 4], dtype="<i4")[0])
    return mt, mti


def forward(state, n):
    """Untempered words of the n outputs after the import point (position p
    is absolute index mti + p; indices below 624 are mt[] itself)."""
    mt, mti = state_words(state)
    total = mti + n
    s = np.zeros(max(total, N), dtype=np.uint64)
    s[:N] = mt
    mag = np.uint64(MAGIC)
    for j0 in range(N, total, LAG):
        j1 = min(j0 + LAG, total)
        y = (s[j0 - 624:j1 - 624] & np.uint64(0x80000000)) | (s[j0 - 623:j1 - 623] & np.uint64(0x7FFFFFFF))
        s[j0:j1] = s[j0 - LAG:j1 - LAG] ^ (y >> np.uint64(1)) ^ np.where((y & np.uint64(1)) == 1, mag, np.uint64(0))
    return s[mti:total].astype(np.uint32)


def with_words_at(words, mti, seed):
    """A 5000-byte GSL state with index mti whose output word at position p
    (counted from the import point; negative: a word of mt[] below mti) has
    the tempered value words[p]; every other word is pseudo-random."""
    rs = np.random.RandomState(seed)
    target = {mti + int(p): untemper(v) for p, v in words.items()}
    assert all(j >= 0 for j in target)
    top = max(target) if target else 0
    if top < N:
        mt = [int(x) for x in rs.randint(0, 2 ** 32, size=N, dtype=np.uint64)]
        for j, v in target.items():
            mt[j] = v
        return state_bytes(mt, mti)
    T = top - 400  # window s[T .. T + 624); s[T + 1 ..] is free
    assert T >= 1 and min(target) >= T + 1, "targets must lie within 623 consecutive words"
    s = [0] * (T + N)
    s[T:] = [int(x) for x in rs.randint(0, 2 ** 32, size=N, dtype=np.uint64)]
    for j, v in target.items():
        s[j] = v
    s[0] = int(rs.randint(0, 2 ** 31))  # its low 31 bits reach no later word
    for j in range(T + N - 1, N - 1, -1):
        t = s[j] ^ s[j - LAG]
        y = (((t ^ MAGIC) << 1) | 1) if t & 0x80000000 else (t << 1)
        y &= M32
        a, b = j - 624, j - 623  # (b == T at the first step: the window's first word keeps its free top bit)
        s[a] = (s[a] & 0x7FFFFFFF) | (y & 0x80000000)
        s[b] = (s[b] & 0x80000000) | (y & 0x7FFFFFFF)
    return state_bytes(s[:N], mti)


def seeded(seed):
    """the state gsl_rng_set leaves (mti = 624)"""
    return R.Rng(seed=seed).get_bytes()


def rng_of(state):
    r = R.Rng()
    r.set_bytes(state)
    return r


def polar_attempts(rng, M):
    """gsl_ran_gaussian's loop restated on rng.get() words (rng is advanced
    past M normals).  Returns (attempts, words): the attempt index of every
    accepted normal (an attempt is one pair of non-zero words, counted from
    0) and the number of words drawn up to and including its last word."""
    attempts, words = [], []
    a, w = -1, 0
    for _ in range(M):
        while True:
            pair = []
            while len(pair) < 2:  # gsl_rng_uniform_pos: a zero word is skipped
                v = rng.get()
                w += 1
                if v:
                    pair.append(v)
            a += 1
            x = -1 + 2 * (pair[0] / 4294967296.0)
            y = -1 + 2 * (pair[1] / 4294967296.0)
            r2 = x * x + y * y
            if not (r2 > 1.0 or r2 == 0):
                break
        attempts.append(a)
        words.append(w)
    return attempts, words


def polar_attempts_np(state, M):
    """polar_attempts from forward()'s words at once (for draws too long for
    a Python loop; pinned to polar_attempts in test_mt_states_cpu.py)."""
    n = int(M * 2.6) + 4096
    while True:
        w = temper_np(forward(state, n))
        pos = np.flatnonzero(w != 0)
        pos = pos[: len(pos) // 2 * 2]
        u = w[pos].astype(np.float64) / 4294967296.0
        x, y = -1 + 2 * u[0::2], -1 + 2 * u[1::2]
        r2 = x * x + y * y
        acc = np.flatnonzero(~((r2 > 1.0) | (r2 == 0)))
        if len(acc) >= M:
            acc = acc[:M]
            return acc, pos[2 * acc + 1] + 1
        n *= 2


def gaussians(state, M):
    """(M normals in stream order, the oracle's state after them)"""
    r = rng_of(state)
    z = np.empty(M)
    R.lib().kr_ran_gaussian_n.argtypes = [R.C.c_void_p, R.C.c_size_t, R.C.POINTER(R.C.c_double)]
    R.lib().kr_ran_gaussian_n.restype = None
    R.lib().kr_ran_gaussian_n(r.ptr, M, z.ctypes.data_as(R.C.POINTER(R.C.c_double)))
    return z, r.get_bytes()


# ------------------------------------------------------------------ states
# Every state the GPU tests draw from, by name: (state, {position: tempered
# value}, words the test consumes at most).  test_mt_states_cpu.py checks each
# against the oracle: the values stand where requested and no other zero word
# lies in the consumed range.
MTI = 5
HALF = 0x80000000  # tempered word of u = 1/2: x = y = 0, r2 == 0
W15 = 1 << 15


def _find(predicate, build, seeds=range(1, 200)):
    for seed in seeds:
        st = build(seed)
        if predicate(st):
            return st
    raise AssertionError("no seed gives the wanted state")


def _accepted_ends_at(state, p, M=300):
    """some normal's last word is word p - 1 (so word p follows it directly)"""
    return p in polar_attempts(rng_of(state), M)[1]


@functools.lru_cache(maxsize=None)
def case_a():
    """zero words in (and just past) the imported block, mti = 5, M = 300"""
    out = {}
    out["at_mti"] = ({0: 0}, with_words_at({0: 0}, MTI, 11))
    out["second_of_pair"] = ({41: 0}, with_words_at({41: 0}, MTI, 12))
    # both words of attempt 20, after an accepted attempt 19
    z = {40: 0, 41: 0}
    out["both_of_attempt"] = (z, _find(lambda s: _accepted_ends_at(s, 40), lambda sd: with_words_at(z, MTI, sd)))
    out["straddling"] = ({41: 0, 42: 0}, with_words_at({41: 0, 42: 0}, MTI, 14))
    # mt[623] (position 618) and the first word the device produces
    z623 = {623 - MTI: 0}
    out["word_623"] = (z623, _find(lambda s: _accepted_ends_at(s, 618), lambda sd: with_words_at(z623, MTI, sd)))
    z624 = {623 - MTI: 0, 624 - MTI: 0}
    out["words_623_624"] = (z624, _find(lambda s: _accepted_ends_at(s, 618), lambda sd: with_words_at(z624, MTI, sd)))
    return out


def case_a_below_mti():
    return {-3: 0}, with_words_at({-3: 0}, MTI, 17)


@functools.lru_cache(maxsize=None)
def case_b():
    """both words of one attempt are 0x80000000 (r2 == 0): in the imported
    block, and across the block's end"""
    return {"in_block": ({60: HALF, 61: HALF}, with_words_at({60: HALF, 61: HALF}, MTI, 21)),
            "device_made": ({700: HALF, 701: HALF}, with_words_at({700: HALF, 701: HALF}, MTI, 22))}


@functools.lru_cache(maxsize=None)
def case_c():
    """zero words at every device recording site (M = 30 000, chunks of 2^15)"""
    groups = {"first_produce": [624 + 5], "serial": [2000], "chunk_edge": [W15 - 1, W15, W15 + 100],
              "rolling_tail": [W15 + 25000], "second_chunk_edge": [2 * W15]}
    return {k: ({p: 0 for p in v}, with_words_at({p: 0 for p in v}, MTI, 30 + i))
            for i, (k, v) in enumerate(groups.items())}


@functools.lru_cache(maxsize=None)
def case_d():
    """the zero list's capacity: 64 and 65 pending zeros from mti on, and 64
    in the imported block with the 65th made by the device"""
    z64 = {p: 0 for p in range(64)}
    z65 = {p: 0 for p in range(65)}
    zdev = {p: 0 for p in range(560 - MTI, 624 - MTI)}
    zdev[700 - MTI] = 0
    return {"exactly_64": (z64, with_words_at(z64, MTI, 41)), "imported_65": (z65, with_words_at(z65, MTI, 42)),
            "device_65th": (zdev, with_words_at(zdev, MTI, 43))}


E_SEED = 1337


@functools.lru_cache(maxsize=None)
def plain_states():
    """states without special words, by the case that draws from them:
    name -> (state, words consumed at most)"""
    out = {"e": (seeded(E_SEED), 4_400_000), "f": (with_words_at({}, MTI, 51), 14_000), "g": (seeded(4242), 12_000),
           "h_mixed": (with_words_at({}, MTI, 66), 1_000), "i": (with_words_at({}, MTI, 70), 110_000),
           "j": (with_words_at({}, MTI, 75), 2_000), "l": (with_words_at({}, MTI, 91), 70_000)}
    for mti in (0, 1, 623, 624):
        out["h_%d" % mti] = (with_words_at({}, mti, 60 + mti), 2_000)
    return out


def all_states():
    """name -> (requested words, state, words consumed at most)"""
    out = {}
    for k, (z, st) in case_a().items():
        out["a_" + k] = (z, st, 2000)
    z, st = case_a_below_mti()
    out["a_below_mti"] = (z, st, 2000)
    for k, (z, st) in case_b().items():
        out["b_" + k] = (z, st, 2000)
    for k, (z, st) in case_c().items():
        out["c_" + k] = (z, st, 3 * W15)
    for k, (z, st) in case_d().items():
        out["d_" + k] = (z, st, 2000)
    return out
