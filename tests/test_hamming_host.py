"""Ungapped (Hamming) scoring, CPU side: nvbio_hip_hamming_score_host / nvbio_hip_hamming_score_qual_host -- the drop-in layer's
priv::hamming_score behind the C-ABI -- against a model kept here.

The model is the closed form of the pattern-blocking sweep: H(i,j) = H(i-1,j-1) + S with every border zero (LOCAL clamped at zero after
every cell), evaluated a column at a time; the values that cross a 16-column block boundary pass through the sweep's int16 column; after
every block but the last the job stops when max_i H(i, block end) + (M - block end) * match < min_score, and the sink keeps what it had
seen.  BestSink replaces on <=, so of equal scores the one reported LAST stays (LOCAL: block, then row, then column).  The model is
itself checked once against a literal port of the 16-column sweep.  tests/test_hamming_gpu.py runs the same cases on the device."""
import ctypes as C
import functools

import numpy as np
import pytest

import nvbio_amd
from nvbio_amd import _lib
from oracle import pyoracle as O

GLOBAL, LOCAL, SEMI = 0, 1, 2
MIN = -(1 << 30)                    # Field_traits<int32>::min(): a fresh BestSink's score, and the threshold of a job without one
INVALID = 0xFFFFFFFF
MS = (1, 15, 16, 17, 32, 33, 63, 64, 65, 150)


def text_lengths(M):
    return sorted({0, 1, M - 1, M, M + 1, 63, 64, 65, M + 64, 333})


def wrap16(v):
    return ((np.asarray(v, np.int64) + 32768) % 65536) - 32768


# ------------------------------------------------------------------------------------------------ the model
def model(typ, pat, pen, text, match, ms=None):
    """(ok, score, (sink.x, sink.y)).  pat: pattern symbols; pen[j]: the score of a mismatch at column j; text: 2-bit symbols."""
    ms = MIN if ms is None else int(ms)
    M, N = len(pat), len(text)
    S = np.where(np.asarray(text, np.int64)[:, None] == np.asarray(pat, np.int64)[None, :], np.int64(match), np.asarray(pen, np.int64)[None, :])
    score, sink = MIN, (INVALID, INVALID)
    n_blocks = max(1, (M + 15) // 16)
    h = np.zeros(N, np.int64)                              # H(., block start): zero border, then the int16 column
    for b in range(n_blocks):
        last = b == n_blocks - 1
        cols = []
        for j in range(16 * b, min(M, 16 * b + 16)):
            h = np.concatenate([[0], h[:-1]]) + S[:, j] if N else h
            if typ == LOCAL:
                h = np.maximum(h, 0)
            cols.append(h)
        if typ == LOCAL and N and cols:
            blk = np.stack(cols, axis=1)                   # rows x columns: the report order is row-major inside a block
            m = int(blk.max())
            if score <= m:
                i, k = np.argwhere(blk == m)[-1]
                score, sink = m, (int(i) + 1, 16 * b + int(k) + 1)
        if last:
            break
        edge = int(h.max()) if N else -(1 << 31)
        if edge + (M - 16 * (b + 1)) * match < ms:
            return False, score, sink
        h = wrap16(h)
    if typ == SEMI and N:
        m = int(h.max())
        if score <= m:
            score, sink = m, (int(np.flatnonzero(h == m)[-1]) + 1, M)
    if typ == GLOBAL:
        m = int(h[N - 1]) if N else 0
        if score <= m:
            score, sink = m, (N, M)
    return True, score, sink


def sweep_port(typ, pat, pen, text, match, ms=None):
    """priv::hamming_score<false, TYPE> statement for statement: 16-column blocks, an int16 column over the text."""
    ms = MIN if ms is None else int(ms)
    BL = 16
    M, N = len(pat), len(text)
    column = [0] * N
    score, sink = MIN, (INVALID, INVALID)

    def report(s, k):
        nonlocal score, sink
        if score <= s:
            score, sink = s, k
    sym, ql = [0] * BL, [0] * BL
    padded = BL * ((M + BL - 1) // BL)
    end_block = padded if padded > BL else BL
    H = [0] * (BL + 1)
    for block in range(0, end_block, BL):
        last = block + BL == end_block
        for t in range(BL):
            if block + t < M:
                sym[t], ql[t] = int(pat[block + t]), int(pen[block + t])
        H = [0] * (BL + 1)
        best_edge = -(1 << 31)
        carry = 0
        for i in range(N):
            diag = carry
            H[0] = carry = column[i]
            for j in range(1, BL + 1):
                h = diag + (match if int(text[i]) == sym[j - 1] else ql[j - 1])
                if typ == LOCAL:
                    h = max(h, 0)
                diag = H[j]
                H[j] = h
            column[i] = int(wrap16(H[BL]))
            best_edge = max(best_edge, H[BL])
            if typ == LOCAL:
                for j in range(1, BL + 1):
                    if not last or block + j <= M:
                        report(H[j], (i + 1, block + j))
            elif last and typ == SEMI:
                report(H[((M - 1) & (BL - 1)) + 1], (i + 1, M))
        if not last and best_edge + (M - block - BL) * match < ms:
            return False, score, sink
    if typ == GLOBAL:
        report(H[((M - 1) & (BL - 1)) + 1], (N, M))
    return True, score, sink


# ------------------------------------------------------------------------------------------------ the cases
# pattern formats: (name, bits, pattern big-endian, text big-endian, alphabet size, symbols that equal no text symbol)
FORMATS = {
    "2bit-binary": (2, True, True, 2, ()),                  # two letters: LOCAL maxima tie all over the matrix
    "4bit": (4, True, False, 4, (4,)),
    "8bit": (8, False, False, 4, (4, 78, 255)),
}
QUALS = ("simple", "constant", "phred", "distinct")


def scheme_of(kind, typ):
    """(match, lut[256] or None, flat mismatch)"""
    if kind == "simple":
        return (2 if typ == LOCAL else 1), None, -3
    if kind == "constant":
        lut = np.full(256, -4, np.int32)
        return (2 if typ == LOCAL else 0), lut, 0
    if kind == "phred":                                     # nvBowtie's QualCost(2, 6): 2 + int(min(q, 40) / 40 * 4)
        lut = np.array([-(2 + int(np.float32(np.float32(min(q, 40)) / np.float32(40.0)) * np.float32(4))) for q in range(256)], np.int32)
        return (2 if typ == LOCAL else 0), lut, 0
    lut = np.array([-(1 + q) if q <= 40 else -50 for q in range(256)], np.int32)      # 41 used entries, all different
    return 3, lut, 0


@functools.lru_cache(maxsize=None)
def make_case(fmt, qual, seed=0, fixed=None):
    """One batch: every (M, N) of the matrix (or `fixed` = (M, N) for all), three kinds of text per shape.  Returns a dict of host arrays."""
    bits, pbe, tbe, sigma, odd = FORMATS[fmt]
    rng = np.random.default_rng(1000 + seed + 17 * list(FORMATS).index(fmt) + 101 * QUALS.index(qual))
    shapes = [(M, N) for M in MS for N in text_lengths(M)] if fixed is None else [fixed] * 40
    pats, texts, quals = [], [], []
    for M, N in shapes:
        for kind in range(3):
            p = rng.integers(0, sigma, M).astype(np.uint8)
            t = rng.integers(0, sigma, N).astype(np.uint8)
            if kind < 2 and N:                              # plant the pattern (0-5 substitutions), anywhere it overlaps the text
                off = int(rng.integers(-min(M - 1, 20), max(N - M, 0) + min(M - 1, 20) + 1)) if kind else int(rng.integers(0, max(N - M, 0) + 1))
                src = p.copy()
                for _ in range(int(rng.integers(0, 6))):
                    src[int(rng.integers(0, M))] = rng.integers(0, sigma)
                lo, hi = max(off, 0), min(off + M, N)
                if hi > lo:
                    t[lo:hi] = src[lo - off:hi - off]
            if odd and M > 2 and rng.random() < 0.5:
                p[int(rng.integers(0, M))] = odd[int(rng.integers(0, len(odd)))]
            pats.append(p); texts.append(t)
            quals.append(rng.integers(2, 41, M).astype(np.uint8) if qual != "constant" else np.full(M, 30, np.uint8))
    hp, ht = O.StringSet.from_lists(pats, bits, pbe), O.StringSet.from_lists(texts, 2, tbe)
    return dict(pats=pats, texts=texts, quals=quals, hp=hp, ht=ht, qcat=np.concatenate(quals), fixed=fixed)


@functools.lru_cache(maxsize=None)
def expected(fmt, qual, typ, seed=0, fixed=None):
    """The model's answers for the four kinds of threshold: {kind: (min_score array or None, ok, score, sink)}"""
    c = make_case(fmt, qual, seed, fixed)
    match, lut, flat = scheme_of(qual, typ)
    pens = [(lut[q].astype(np.int64) if lut is not None else np.full(len(q), flat, np.int64)) for q in c["quals"]]
    n = len(c["pats"])

    def run(ms):
        r = [model(typ, c["pats"][i], pens[i], c["texts"][i], match, None if ms is None else ms[i]) for i in range(n)]
        return (ms, np.array([x[0] for x in r], np.uint8), np.array([x[1] for x in r], np.int32), np.array([x[2] for x in r], np.uint32))
    free = run(None)
    own = np.where(free[1] == 1, free[2], MIN).astype(np.int32)            # a job that even NULL declines (empty text) keeps MIN
    return {"null": free, "best": run(own), "best+1": run((own.astype(np.int64) + 1).astype(np.int32)), "-1e6": run(np.full(n, -10 ** 6, np.int32))}


def sset(hs, fixed_length=None):
    s = _lib.StringSetStruct()
    s.words, s.n_words, s.bits, s.big_endian = hs.words.ctypes.data, hs.words.size, hs.bits, hs.big_endian
    s.begin = hs.begin.ctypes.data
    s.length, s.fixed_length = (hs.length.ctypes.data, 0) if fixed_length is None else (None, fixed_length)
    return s


def qual_struct(match, lut):
    s = _lib.GotohQualSchemeStruct()
    s.match = int(match)
    s.pattern_gap_open = s.pattern_gap_ext = s.text_gap_open = s.text_gap_ext = -1000        # never read
    for q in range(256):
        s.mismatch[q] = int(lut[q])
    return s


def run_host(c, qual, typ, ms, algorithm=0):
    L = nvbio_amd.lib()
    match, lut, flat = scheme_of(qual, typ)
    n = len(c["pats"])
    fx = c["fixed"]
    sp, st = sset(c["hp"], None if fx is None else fx[0]), sset(c["ht"], None if fx is None else fx[1])
    score = np.full(n, 77, np.int32); sink = np.full((n, 2), 77, np.uint32); ok = np.full(n, 77, np.uint8)
    msp = None if ms is None else ms.ctypes.data
    if lut is None:
        sc = _lib.GotohSchemeStruct(match, flat, -1000, -1000)
        e = L.nvbio_hip_hamming_score_host(C.byref(sc), algorithm, typ, C.byref(sp), C.byref(st), msp, n, score.ctypes.data, sink.ctypes.data, ok.ctypes.data, 2)
    else:
        sc = qual_struct(match, lut)
        e = L.nvbio_hip_hamming_score_qual_host(C.byref(sc), algorithm, typ, C.byref(sp), c["qcat"].ctypes.data, c["qcat"].size, C.byref(st), msp, n,
                                                score.ctypes.data, sink.ctypes.data, ok.ctypes.data, 2)
    assert e == 0
    return ok, score, sink


def check(got, want, what):
    ok, score, sink = got
    _, eok, escore, esink = want
    bad = np.flatnonzero((ok != eok) | (score != escore) | (sink != esink).any(axis=1))
    assert bad.size == 0, "%s: %d jobs differ, first %d: got %s %s %s, model %s %s %s" % (
        what, bad.size, bad[0], ok[bad[0]], score[bad[0]], sink[bad[0]], eok[bad[0]], escore[bad[0]], esink[bad[0]])


def assert_thresholds_bind(exp):
    """with min_score = the job's own best, the early exit must both fire and not fire (it is no bound: it declines reachable scores)"""
    ok = exp["best"][1]
    assert 0.05 * ok.size <= int((ok == 0).sum()) and 0.05 * ok.size <= int((ok == 1).sum()), (int((ok == 0).sum()), ok.size)
    assert (exp["-1e6"][1][exp["null"][1] == 1] == 1).all()


# ------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("typ", [GLOBAL, LOCAL, SEMI])
def test_model_is_the_sweep(typ):
    """the closed form against the literal port, thresholds included, on every shape of the matrix"""
    for fmt, qual in (("2bit-binary", "simple"), ("4bit", "distinct")):
        c = make_case(fmt, qual)
        exp = expected(fmt, qual, typ)
        match, lut, flat = scheme_of(qual, typ)
        for i in range(0, len(c["pats"]), 2):
            pen = lut[c["quals"][i]] if lut is not None else np.full(len(c["pats"][i]), flat)
            for kind in ("null", "best", "best+1"):
                ms, eok, es, ek = exp[kind]
                got = sweep_port(typ, c["pats"][i], pen, c["texts"][i], match, None if ms is None else ms[i])
                assert got == (bool(eok[i]), int(es[i]), (int(ek[i][0]), int(ek[i][1]))), (fmt, qual, kind, i, len(c["pats"][i]), len(c["texts"][i]))


def test_early_exit_is_not_a_bound():
    """M = 17, N = 1: the one cell of the second block starts from the top border, and the exit after the first block never sees it"""
    pat, text = np.zeros(17, np.uint8), np.zeros(1, np.uint8)
    pat[15] = 1                                                       # H(0, 16) mismatches: the first block's edge is -3
    pen = np.full(17, -3)
    ok, score, sink = model(SEMI, pat, pen, text, 1)
    assert (ok, score, sink) == (True, 1, (1, 17))
    assert model(SEMI, pat, pen, text, 1, ms=1)[0] is False and sweep_port(SEMI, pat, pen, text, 1, ms=1)[0] is False


@pytest.mark.parametrize("typ", [GLOBAL, LOCAL, SEMI])
@pytest.mark.parametrize("qual", QUALS)
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_host_twin_ragged(fmt, qual, typ):
    c, exp = make_case(fmt, qual), expected(fmt, qual, typ)
    assert_thresholds_bind(exp)
    for kind, want in exp.items():
        check(run_host(c, qual, typ, want[0]), want, "%s %s type %d min_score %s" % (fmt, qual, typ, kind))


@pytest.mark.parametrize("typ", [GLOBAL, LOCAL, SEMI])
@pytest.mark.parametrize("shape", [(17, 1), (64, 64), (150, 333)])
def test_host_twin_fixed_length(shape, typ):
    fmt, qual = "4bit", "phred"
    c, exp = make_case(fmt, qual, 5, shape), expected(fmt, qual, typ, 5, shape)
    for kind, want in exp.items():
        check(run_host(c, qual, typ, want[0]), want, "fixed %s type %d min_score %s" % (shape, typ, kind))


# values beyond int16: the column between two blocks holds their low 16 bits, in the sweep and therefore in the model and the kernels
WIDE = dict(match=400, flat=-700)


@functools.lru_cache(maxsize=None)
def wide_case(typ):
    c = make_case("4bit", "simple", 9)
    pens = [np.full(len(p), WIDE["flat"], np.int64) for p in c["pats"]]
    r = [model(typ, c["pats"][i], pens[i], c["texts"][i], WIDE["match"]) for i in range(len(pens))]
    return c, (None, np.array([x[0] for x in r], np.uint8), np.array([x[1] for x in r], np.int32), np.array([x[2] for x in r], np.uint32))


@pytest.mark.parametrize("typ", [GLOBAL, LOCAL, SEMI])
def test_host_twin_beyond_int16(typ):
    c, want = wide_case(typ)
    assert int(want[2].max()) > 32767 or typ == GLOBAL
    L = nvbio_amd.lib()
    n = len(c["pats"])
    sp, st = sset(c["hp"]), sset(c["ht"])
    score = np.zeros(n, np.int32); sink = np.zeros((n, 2), np.uint32); ok = np.zeros(n, np.uint8)
    sc = _lib.GotohSchemeStruct(WIDE["match"], WIDE["flat"], 0, 0)
    assert L.nvbio_hip_hamming_score_host(C.byref(sc), 0, typ, C.byref(sp), C.byref(st), None, n, score.ctypes.data, sink.ctypes.data, ok.ctypes.data, 2) == 0
    check((ok, score, sink), want, "wide type %d" % typ)


def test_host_twin_text_blocking_runs_and_arguments_are_checked():
    """TextBlockingTag: the same matrix in another order -- LOCAL scores agree with the pattern-blocking ones; bad arguments are refused"""
    c, exp = make_case("4bit", "phred"), expected("4bit", "phred", LOCAL)
    ok, score, _ = run_host(c, "phred", LOCAL, None, algorithm=1)
    has_text = np.array([len(t) > 0 for t in c["texts"]])
    assert (ok == 1).all() and (score[has_text] == exp["null"][2][has_text]).all()
    L = nvbio_amd.lib()
    sp, st = sset(c["hp"]), sset(c["ht"])
    sc = _lib.GotohSchemeStruct(1, -1, 0, 0)
    assert L.nvbio_hip_hamming_score_host(None, 0, LOCAL, C.byref(sp), C.byref(st), None, 1, None, None, None, 1) == 1
    assert L.nvbio_hip_hamming_score_host(C.byref(sc), 2, LOCAL, C.byref(sp), C.byref(st), None, 1, score.ctypes.data, score.ctypes.data, None, 1) == 1
    # the device entries check their arguments before anything touches a GPU
    assert L.nvbio_hip_hamming_score(None, 0, LOCAL, C.byref(sp), C.byref(st), 150, 333, None, 1, None, None, None, None) == 1
    assert L.nvbio_hip_hamming_score(C.byref(sc), 0, LOCAL, C.byref(sp), C.byref(st), 150, 333, None, 0, None, None, None, None) == 0
    assert L.nvbio_hip_hamming_score(C.byref(sc), 1, LOCAL, C.byref(sp), C.byref(st), 150, 333, None, 1, score.ctypes.data, score.ctypes.data, None, None) == 801
    assert L.nvbio_hip_hamming_score(C.byref(sc), 0, LOCAL, C.byref(sp), C.byref(st), 4097, 333, None, 1, score.ctypes.data, score.ctypes.data, None, None) == 801
