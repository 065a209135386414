"""The pair fold of the column frame's row (nvbio_amd/csrc/banded_gotoh_pair.h, PF_FOLD2: "The pair fold"), modelled in numpy on the packed
words the kernel holds, with the checks of test_pair_column_frame.py's Packed on every operation: every operand of a packed maximum lies
in 0x0400 ... 0x7BFF, no add carries out of a half, no subtract borrows.

A row's key stands in its last column's frame, rk(i) = 32 score + Z(i,14) + j.  Rows i (even) and i + 1 share one fold:
    q = max(rk(i) + 2 G, rk(i+1) + 16) - Z(i+1,14) = 32 score + 16 (odd row) + j,       replace when (q | 31) >= best,
with the even row's number beside it; a last row without a partner is folded alone, its zero worked out from M.  The decoded (score, row,
column) must equal the per-row fold's -- the higher score, then the later row, then the larger column -- for the keys of real jobs at
the column frame's admission limits, for random key sequences and for constructed ties."""
import numpy as np
import pytest

from test_pair_column_frame import BAND, FLOOR, TOP, NEG, Packed, column_admitted, column_limit, extremes, pd3_top, reads_near


def zero(scheme, i, j):
    """Z(i,j) of the column frame"""
    _, _, go, ge = scheme
    G, D = -32 * ge, 32 * (ge - go)
    return D + G + FLOOR + G * (2 * i + j + 2)


def row_bests(pats, txts, scheme):
    """a plain banded Gotoh LOCAL model: per row, the best score and the largest column that holds it (M x n each)"""
    match, mismatch, go, ge = scheme
    n, M = pats.shape
    H = np.zeros((n, BAND), np.int64)
    F = np.full((n, BAND), NEG, np.int64)
    rs, rc = np.empty((M, n), np.int64), np.empty((M, n), np.int64)
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
        rs[i] = H.max(1)
        rc[i] = (BAND - 1) - np.argmax(H[:, ::-1] == rs[i][:, None], axis=1)
    return rs, rc


def per_row_fold(rs, rc):
    """the fold the kernel had: p = 32 score + j, replace when (p | 31) >= best"""
    M, n = rs.shape
    best = np.zeros(n, np.int64); besti = np.zeros(n, np.int64)
    for i in range(M):
        p = 32 * rs[i] + rc[i]
        upd = (p | 31) >= best
        best = np.where(upd, p, best); besti = np.where(upd, i, besti)
    return best >> 5, besti, best & 31


def pair_fold(rs, rc, scheme):
    """the packed pair fold over the rows' framed keys; jobs 2k and 2k + 1 share lane k.  Returns (score, row, column) and the Packed"""
    M, n = rs.shape
    assert n % 2 == 0
    _, _, go, ge = scheme
    G = -32 * ge
    P = Packed()

    def pack(v):
        v = np.asarray(v, np.int64)
        assert v.min() >= 0 and v.max() <= 0xFFFF
        return (v[0::2] | (v[1::2] << 16)).astype(np.uint32)

    def fold(q, i, best, besti):
        for hf, r in enumerate(P.halves(q)):
            upd = (r | 31) >= best[hf]
            best[hf] = np.where(upd, r, best[hf]); besti[hf] = np.where(upd, i, besti[hf])

    best = [np.zeros(n // 2, np.int64), np.zeros(n // 2, np.int64)]
    besti = [np.zeros(n // 2, np.int64), np.zeros(n // 2, np.int64)]
    rk2 = None
    for i in range(M):
        rk = pack(32 * rs[i] + rc[i] + zero(scheme, i, BAND - 1))                  # what tail2 leaves: the last column's frame
        if i % 2 == 0:
            rk2 = rk
        else:
            q = P.sub(P.mx(P.add(rk2, P.rep(2 * G)), P.add(rk, P.rep(16))), P.rep(zero(scheme, i, BAND - 1)))
            fold(q, i - 1, best, besti)
    if M % 2:                                                                      # PD3::fold_last: the zero from M, in scalars
        fold(P.sub(rk2, P.rep(zero(scheme, M - 1, BAND - 1))), M - 1, best, besti)
    score = np.empty(n, np.int64); row = np.empty(n, np.int64); col = np.empty(n, np.int64)
    for hf in range(2):
        score[hf::2] = best[hf] >> 5; row[hf::2] = besti[hf] + ((best[hf] >> 4) & 1); col[hf::2] = best[hf] & 15
    return (score, row, col), P


def agree(rs, rc, scheme, packed_range=True):
    got, P = pair_fold(rs, rc, scheme)
    want = per_row_fold(rs, rc)
    for g, w, what in zip(got, want, ("score", "row", "column")):
        bad = np.nonzero(g != w)[0]
        assert bad.size == 0, "%s %s M %d: %d jobs differ, first %d: pair %d per-row %d" % (what, scheme, rs.shape[0], bad.size, bad[0], g[bad[0]], w[bad[0]])
    if rs.shape[0] > 1:
        assert FLOOR <= P.lo and P.hi <= TOP, (scheme, rs.shape[0], hex(P.lo), hex(P.hi))
    return want, P


@pytest.mark.parametrize("scheme", [
    (2, -1, -2, -1),     # the headline scheme: M = 234 meets the frame's top exactly
    (4, -1, -2, -1),     # the table's byte at its limit, 255
    (1, 0, -5, -1),      # ... by the gap costs
    (3, -2, -3, 0),      # gap_ext == 0: both rows of a pair stand in one frame
    (1, 0, -1, 0),
])
def test_admission_limit(scheme):
    """real jobs at the column frame's limit and one row short of it (odd and even M): perfect matches beside jobs that score nothing.
    The largest operand is the last pair's key, which stays inside what the frame's bound leaves above the largest h': 16 + 14 of its 255"""
    rng = np.random.default_rng(81000 + sum(abs(v) * 5 ** k for k, v in enumerate(scheme)))
    L = column_limit(scheme) or 300
    match, mismatch, go, ge = scheme
    for M in (L, L - 1):
        assert column_admitted(scheme, M)
        pats, txts = extremes(rng, M, M + 20)
        rs, rc = row_bests(pats, txts, scheme)
        (score, row, col), P = agree(rs, rc, scheme)
        assert score[0] == match * M and (row[0], col[0]) == (M - 1, 14) and score[1] == 0 and (row[1], col[1]) == (M - 1, 14)
        bound = pd3_top(32 * (ge - go), -32 * ge, M, max(match, mismatch, 0))
        assert P.hi <= bound - 255 + 30 <= TOP
        pats, txts = reads_near(rng, 20, M, M + 16)
        agree(*row_bests(pats, txts, scheme), scheme)


def test_all_zero_scheme():
    """(0,0,0,0): every key of every row is the frame's floor plus its column, Z = 0x0400 itself; the last row's last column wins"""
    scheme = (0, 0, 0, 0)
    rng = np.random.default_rng(82000)
    for M in (1, 2, 3, 16, 17, 100):
        pats, txts = reads_near(rng, 6, M, M + 14)
        (score, row, col), P = agree(*row_bests(pats, txts, scheme), scheme)
        assert (score == 0).all() and (row == M - 1).all() and (col == 14).all()
        if M > 1:
            assert P.lo == FLOOR + 14 and P.hi == FLOOR + 14 + 16


@pytest.mark.parametrize("scheme", [(2, -1, -2, -1), (3, -2, -3, 0), (1, -3, -4, -2)])
@pytest.mark.parametrize("M", [1, 2, 3, 4, 15, 16, 17, 33, 100])
def test_random_keys(scheme, M):
    """random (score, column) sequences, few distinct scores so that ties are the rule: the fold sees every order of equal and unequal
    neighbours inside a pair and across pairs, with and without a lone last row"""
    rng = np.random.default_rng(83000 + 7 * M + scheme[0])
    n = 400
    rs = rng.integers(0, 4, (M, n)).astype(np.int64) * rng.integers(1, 1 + scheme[0] * M // 3 + 1)
    rs = np.minimum(rs, scheme[0] * M)
    rc = rng.integers(0, BAND, (M, n)).astype(np.int64)
    agree(rs, rc, scheme)


def test_constructed_ties():
    scheme = (2, -1, -2, -1)
    S = 40

    def case(rows):
        """rows: (score, column) per row for one job; the other half of the lane holds the reverse order"""
        a = np.array(rows, np.int64)
        rs = np.stack([a[:, 0], a[::-1, 0]], 1); rc = np.stack([a[:, 1], a[::-1, 1]], 1)
        (score, row, col), _ = agree(rs, rc, scheme)
        return int(score[0]), int(row[0]), int(col[0])

    low = (3, 7)
    # equal scores in both rows of a pair, the smaller column in the later row: the later row wins
    assert case([low, low, (S, 12), (S, 2), low, low]) == (S, 3, 2)
    assert case([low, low, (S, 12), (S, 2), low]) == (S, 3, 2)                     # odd M
    # ... the larger column in the later row
    assert case([(S, 2), (S, 12), low, low]) == (S, 1, 12)
    # the even row higher: it wins whatever the columns; the odd row higher
    assert case([low, low, (S + 1, 0), (S, 14)]) == (S + 1, 2, 0)
    assert case([low, low, (S, 14), (S + 1, 0)]) == (S + 1, 3, 0)
    # equal scores in rows of different pairs: the later pair wins, in its even and in its odd row
    assert case([(S, 14), low, low, low, (S, 0), low]) == (S, 4, 0)
    assert case([low, (S, 14), low, low, low, (S, 0)]) == (S, 5, 0)
    assert case([low, (S, 14), low, low, (S, 1), low, low]) == (S, 4, 1)
    # ... and a lone last row wins over every pair before it
    assert case([low, (S, 14), (S, 13), low, (S, 0)]) == (S, 4, 0)
    assert case([(S, 3)]) == (S, 0, 3)
    # two columns of one row hold the best: the row's key names the larger (row_bests picks it; here the key is given)
    pats = np.zeros((2, 6), np.uint8); txts = np.zeros((2, 6 + 14), np.uint8)      # homopolymers: every column of the last row holds 2 M
    rs, rc = row_bests(pats, txts, scheme)
    (score, row, col), _ = agree(rs, rc, scheme)
    assert (score == 12).all() and (row == 5).all() and (col == 14).all()
