"""The max3 cell of the pair kernel in the column frame (nvbio_amd/csrc/banded_gotoh_pair.h: PD3), modelled in numpy on the packed words
the kernel holds: job A in bits 0-15 and job B in bits 16-31 of every register, constants added and subtracted as one 32-bit operation,
maxima taken per half.  The model follows the kernel's own steps -- the ring of the row's zeros at index (2 i + j) & 15 and its two
scalar adds per row, the keys' constants K_j, column 0's S' handed to column 1 as E', the last column's max3(E', diagonal, Z) and the
sink fold -- and checks on every operation what the header comment argues: every operand of a maximum lies in 0x0400 ... 0x7BFF, no add
carries out of a half, no subtract borrows.  Its results must equal a plain banded Gotoh LOCAL model (score, row, column; a later row,
then a larger column, wins a tie), at the host's admission limit and at the largest D + G and the largest G the byte table admits."""
import numpy as np
import pytest

BAND = 15
FLOOR, TOP = 0x0400, 0x7BFF
PM3_ROW_LIMIT = (0x7BFF - 255 - 0x0400 - 448) // 32
NEG = -(1 << 40)


# ---- the host's admission (banded_gotoh.hip: pair_admitted, pair_max3_admitted, pair_column_admitted)
def pd3_top(D, G, M, s_plus):
    return 0x0400 + D + G + G * (2 * M + BAND - 1) + 32 * M * s_plus + 255


def column_admitted(scheme, M):
    match, mismatch, go, ge = scheme
    if ge > 0 or go > ge or match < 0 or mismatch < go or match < go or max(match, mismatch) - go > 7:
        return False
    s_plus = max(match, mismatch, 0)
    if M * (s_plus - ge) > min(PM3_ROW_LIMIT, 1022):
        return False
    if max(match, mismatch) - go - ge > 7:
        return False
    return pd3_top(32 * (ge - go), -32 * ge, M, s_plus) <= TOP


def column_limit(scheme, cap=2000):
    """the longest pattern the column frame takes, None if there is no limit below cap"""
    assert column_admitted(scheme, 1)
    M = 1
    while M <= cap and column_admitted(scheme, M + 1):
        M += 1
    return None if M > cap else M


# ---- a plain banded Gotoh LOCAL model, one job per array row
def plain_model(pats, txts, scheme):
    match, mismatch, go, ge = scheme
    n, M = pats.shape
    H = np.zeros((n, BAND), np.int64)
    F = np.full((n, BAND), NEG, np.int64)
    best = np.zeros(n, np.int64); brow = np.zeros(n, np.int64); bcol = np.zeros(n, np.int64)
    for i in range(M):
        p = pats[:, i]
        Hn = np.empty_like(H); Fn = np.full_like(F, NEG)
        E = np.full(n, NEG, np.int64)
        for j in range(BAND):
            t = txts[:, i + j]
            s = np.where((p == t) & (p < 4), match, mismatch)
            if j + 1 < BAND:
                Fn[:, j] = np.maximum(F[:, j + 1] + ge, H[:, j + 1] + go)
            if j > 0:
                E = np.maximum(E + ge, Hn[:, j - 1] + go)
            Hn[:, j] = np.maximum(np.maximum(0, H[:, j] + s), np.maximum(E, Fn[:, j]))
        H, F = Hn, Fn
        rb = H.max(1)
        rc = (BAND - 1) - np.argmax(H[:, ::-1] == rb[:, None], axis=1)            # the largest column that holds the row's best
        upd = rb >= best
        best = np.where(upd, rb, best); brow = np.where(upd, i, brow); bcol = np.where(upd, rc, bcol)
    return best, brow, bcol


# ---- the packed model
class Packed:
    """32-bit words of two 16-bit halves, with the checks the kernel's arithmetic relies on; lo / hi: the extreme operands of the maxima"""

    def __init__(self):
        self.lo, self.hi = 1 << 16, 0

    @staticmethod
    def rep(c):
        assert 0 <= c <= 0xFFFF, c
        return np.uint32(c * 0x10001)

    @staticmethod
    def halves(x):
        x = np.asarray(x, np.uint32)
        return (x & np.uint32(0xFFFF)).astype(np.int64), (x >> np.uint32(16)).astype(np.int64)

    def add(self, a, b):
        (al, ah), (bl, bh) = self.halves(a), self.halves(b)
        assert (al + bl).max() <= 0xFFFF and (ah + bh).max() <= 0xFFFF, "an add carries out of its half"
        return (np.asarray(a, np.uint64) + np.asarray(b, np.uint64)).astype(np.uint32)

    def sub(self, a, b):
        (al, ah), (bl, bh) = self.halves(a), self.halves(b)
        assert (al - bl).min() >= 0 and (ah - bh).min() >= 0, "a subtract borrows"
        return (np.asarray(a, np.int64) - np.asarray(b, np.int64)).astype(np.uint32)

    def mx(self, *ops):
        """v_pk_max_u16 / v_pk_maximum3_f16: exact only on the positive normal f16 patterns"""
        lo = hi = None
        for x in ops:
            xl, xh = self.halves(x)
            self.lo = min(self.lo, int(xl.min()), int(xh.min())); self.hi = max(self.hi, int(xl.max()), int(xh.max()))
            lo = xl if lo is None else np.maximum(lo, xl); hi = xh if hi is None else np.maximum(hi, xh)
        return (lo | (hi << 16)).astype(np.uint32)


def column_model(pats, txts, scheme):
    """jobs 2k and 2k + 1 share lane k; returns (score, row, column) per job and the Packed that saw every operation"""
    match, mismatch, go, ge = scheme
    n, M = pats.shape
    assert n % 2 == 0 and txts.shape[1] >= M + BAND - 1
    G, D = -32 * ge, 32 * (ge - go)
    P = Packed()
    bias = D + G + FLOOR
    sub_m, sub_x = 32 * (match - go) + G, 32 * (mismatch - go) + G                # the table's bytes
    assert 0 <= sub_x <= 255 and 0 <= sub_m <= 255
    # PD3::open
    z = [P.rep(bias + G * (2 + (s if s <= BAND - 3 else s - 16))) for s in range(16)]
    K = [P.rep(j + (BAND - 1 - j) * G) for j in range(BAND)]
    Dp, step = P.rep(D), P.rep(16 * G)
    L = n // 2
    S = [np.full(L, P.rep(G + FLOOR + G * j), np.uint32) for j in range(BAND)]
    F = [np.full(L, P.rep(FLOOR), np.uint32) for j in range(BAND - 1)]
    best = [np.zeros(L, np.uint32), np.zeros(L, np.uint32)]
    besti = [np.zeros(L, np.uint32), np.zeros(L, np.uint32)]
    pa, pb, ta, tb = pats[0::2], pats[1::2], txts[0::2], txts[1::2]

    def subst(i, j):
        a = np.where((pa[:, i] == ta[:, i + j]) & (pa[:, i] < 4), sub_m, sub_x).astype(np.uint32)
        b = np.where((pb[:, i] == tb[:, i + j]) & (pb[:, i] < 4), sub_m, sub_x).astype(np.uint32)
        return a | (b << np.uint32(16))

    for i in range(M):
        for s in ((2 * i + BAND - 2) & 15, (2 * i + BAND - 1) & 15):              # the row's prologue: two scalar adds
            z[s] = P.add(z[s], step)
        Z = [z[(2 * i + j) & 15] for j in range(BAND)]
        for j in range(BAND):                                                      # the ring holds this row's zeros
            assert int(Z[j]) == int(P.rep(bias + G * (2 * i + j + 2))), (i, j)
        oS, oF = list(S), list(F)
        # column 0
        F[0] = P.mx(oF[1], oS[1], Z[0])
        h = P.mx(F[0], P.add(oS[0], subst(i, 0)))
        S[0] = P.sub(h, Dp)
        rowkey = P.add(h, K[0])
        E = S[0]
        keys = []
        for j in range(1, BAND):
            d = P.add(oS[j], subst(i, j))
            if j < BAND - 2:
                F[j] = P.mx(oF[j + 1], oS[j + 1], Z[j]); h = P.mx(F[j], d, E)
            elif j == BAND - 2:
                F[j] = P.mx(oS[j + 1], Z[j]); h = P.mx(F[j], d, E)
            else:
                h = P.mx(E, d, Z[j])
            S[j] = P.sub(h, Dp)
            keys.append(P.add(h, K[j]))
            if j < BAND - 1:
                E = P.mx(E, S[j])
            if len(keys) == 2:
                rowkey = P.mx(rowkey, keys[0], keys[1]); keys = []
        assert not keys
        rk = P.halves(P.sub(rowkey, Z[BAND - 1]))                                  # the sink: the key stands in the last column's frame
        for hf in range(2):
            r = rk[hf].astype(np.uint32)
            upd = (r | np.uint32(31)) >= best[hf]
            best[hf] = np.where(upd, r, best[hf]); besti[hf] = np.where(upd, np.uint32(i), besti[hf])
    score = np.empty(n, np.int64); row = np.empty(n, np.int64); col = np.empty(n, np.int64)
    for hf in range(2):
        score[hf::2] = best[hf] >> 5; row[hf::2] = besti[hf]; col[hf::2] = best[hf] & 31
    return (score, row, col), P


def agree(pats, txts, scheme):
    pats, txts = np.asarray(pats, np.uint8), np.asarray(txts, np.uint8)
    assert column_admitted(scheme, pats.shape[1]), (scheme, pats.shape[1])
    got, P = column_model(pats, txts, scheme)
    want = plain_model(pats, txts, scheme)
    for g, w, what in zip(got, want, ("score", "row", "column")):
        bad = np.nonzero(g != w)[0]
        assert bad.size == 0, "%s %s M %d: %d jobs differ, first %d: packed %d plain %d" % (what, scheme, pats.shape[1], bad.size, bad[0], g[bad[0]], w[bad[0]])
    assert FLOOR <= P.lo and P.hi <= TOP, (scheme, pats.shape[1], hex(P.lo), hex(P.hi))
    return want, P


def reads_near(rng, n, M, N):
    """texts and reads cut out of them a few columns into the band, with mutations (an N among them) and an indel"""
    txts = rng.integers(0, 4, (n, N), dtype=np.uint8)
    pats = np.empty((n, M), np.uint8)
    for k in range(n):
        off = int(rng.integers(0, BAND))
        p = np.resize(txts[k, off:off + M], M).copy()
        mut = rng.random(M) < 0.1
        p[mut] = rng.integers(0, 5, int(mut.sum()), dtype=np.uint8)
        if M > 20 and rng.random() < 0.4:
            cut = int(rng.integers(5, M - 5))
            p = np.concatenate([p[:cut], p[cut + 2:], rng.integers(0, 4, 2, dtype=np.uint8)])
        pats[k] = p
    return pats, txts


def extremes(rng, M, N):
    """perfect matches beside jobs that score nothing, in both halves and together; homopolymers; reads of N only"""
    txts = rng.integers(0, 3, (8, N), dtype=np.uint8)
    pats = np.full((8, M), 3, np.uint8)                                            # score 0
    for k in (0, 3, 4, 5):                                                         # (perfect, zero), (zero, perfect), (perfect, perfect)
        pats[k] = txts[k, 14:14 + M]
    pats[6] = 1; txts[6] = 1                                                       # every cell of the band matches
    pats[7] = 4
    return pats, txts


SCHEMES = [(2, -1, -2, -1), (1, -3, -4, -2), (2, -1, -1, -1), (0, 0, 0, 0), (3, -2, -3, 0), (1, -1, -5, -1), (1, 0, -5, -1)]


@pytest.mark.parametrize("scheme", SCHEMES)
def test_equals_plain_model(scheme):
    rng = np.random.default_rng(71000 + sum(abs(v) * 5 ** k for k, v in enumerate(scheme)))
    for M in (1, 2, 3, 15, 16, 17, 33, 100):
        pats, txts = reads_near(rng, 40, M, M + 14 + int(rng.integers(0, 3)))
        agree(pats, txts, scheme)
        agree(*extremes(rng, M, M + 20), scheme)


@pytest.mark.parametrize("scheme", [
    (2, -1, -2, -1),     # the headline scheme: M = 234 meets the top exactly
    (5, -1, -2, -1),     # the largest substitution byte but one (7 * 32 + 32 would pass 255: 5 + 2 + 1 = 8 is refused, see below)
    (4, -1, -2, -1),     # 4 + 2 + 1 = 7: the byte is 255
    (1, 0, -5, -1),      # 7 by the gap costs
    (1, 0, -3, -3),      # the largest G the byte admits beside a positive match: G = 96, D = 0
    (0, -1, -4, -3),     # D + G = 128 with G = 96
    (3, -2, -3, 0),      # G = 0: every column's zero is the same
])
def test_admission_limit(scheme):
    """M at the column frame's limit: the perfect matches drive a half to the top of the range beside a half at the row's zero"""
    rng = np.random.default_rng(72000 + sum(abs(v) * 5 ** k for k, v in enumerate(scheme)))
    if scheme == (5, -1, -2, -1):
        assert not column_admitted(scheme, 1)
        return
    L = column_limit(scheme)
    assert L is not None and not column_admitted(scheme, L + 1)
    pats, txts = extremes(rng, L, L + 20)
    (score, row, col), P = agree(pats, txts, scheme)
    assert score[0] == scheme[0] * L and score[1] == 0 and (row[0], col[0]) == (L - 1, 14)
    match, mismatch, go, ge = scheme
    bound = pd3_top(32 * (ge - go), -32 * ge, L, max(match, mismatch, 0))
    # the bound is the last row's largest h' plus a whole byte, and the perfect match reaches that h' in column 14 (its key adds 14)
    assert bound - 255 + 14 <= P.hi <= bound <= TOP
    pats, txts = reads_near(rng, 20, L, L + 16)
    agree(pats, txts, scheme)


@pytest.mark.parametrize("scheme", [
    (0, 0, -7, 0),       # the largest D + G the row-frame byte admits, all of it in D: D = 224, G = 0
    (0, -1, -6, -1),     # D = 160, G = 32: 6 + 1 = 7
    (0, -3, -5, -2),     # D = 96, G = 64
    (0, 0, -4, -3),      # D = 32, G = 96
    (1, -1, -3, -3),     # D = 0, G = 96
])
def test_largest_gap_costs(scheme):
    """the largest D + G the column frame admits, shared between D and G in every way: the bottom of the range (jobs that score nothing
    hold S' = Z - D in every column) and its top at the scheme's own limit, or at M = 300 where it has none"""
    match, mismatch, go, ge = scheme
    assert max(match, mismatch) - go - ge == 7
    rng = np.random.default_rng(73000 + sum(abs(v) * 5 ** k for k, v in enumerate(scheme)))
    L = column_limit(scheme) or 300
    for M in (1, 2, 17, L):
        _, P = agree(*extremes(rng, M, M + 20), scheme)
        assert P.lo == FLOOR                                                       # F' of row -1
        pats, txts = reads_near(rng, 20, M, M + 14)
        agree(pats, txts, scheme)


def test_not_admitted():
    """one more than the byte admits, and gap costs the pair form never takes"""
    assert column_admitted((1, 0, -5, -1), 100) and not column_admitted((2, 0, -5, -1), 100)
    assert not column_admitted((0, 0, -7, -1), 1)                                  # the row frame's byte holds (7), the column frame's does not (8)
    assert not column_admitted((2, -1, -1, -2), 1) and not column_admitted((2, -1, -2, 1), 1)
    assert column_limit((2, -1, -2, -1)) == 234
    assert pd3_top(32, 32, 234, 2) == TOP


def test_ties_later_row_larger_column():
    """the best score in several rows and several columns: all-mismatch, homopolymers, a read that matches at two offsets"""
    M, N = 33, 53
    pats, txts = [], []
    pats.append(np.full(M, 3)); txts.append(np.zeros(N))                           # nothing matches: score 0, the last row, column 14
    pats.append(np.full(M, 2)); txts.append(np.full(N, 2))                         # every column of the last row holds 2 M
    for period in (1, 2):
        for c in (0, 5, 12):
            unit = np.array([0, 1][:period])
            run = 8
            p = np.full(M, 4); p[:run] = np.resize(unit, run); p[M - run:] = np.resize(unit, run)
            t = np.full(N, 2); t[c:c + run + period] = np.resize(unit, run + period); t[c + M - run:c + M + period] = np.resize(unit, run + period)
            pats.append(p); txts.append(t)
    (score, row, col), _ = agree(np.array(pats), np.array(txts), (2, -1, -2, -1))
    assert (score[0], row[0], col[0]) == (0, M - 1, 14)
    assert (score[1], row[1], col[1]) == (2 * M, M - 1, 14)
    k = 2
    for period in (1, 2):
        for c in (0, 5, 12):
            assert (score[k], row[k], col[k]) == (16, M - 1, c + period), (k, score[k], row[k], col[k])
            k += 1
