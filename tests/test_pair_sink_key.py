"""The pair kernel's sink as one 32-bit key per job (nvbio_amd/csrc/banded_gotoh_pair.h, "The sink": PF_SINK_KEY, a form the library
does not launch and tools/pair_row_probe.hip times), modelled in numpy: folding
W = p << 15 | 31 << 15 | i << 5 | (p & 31) with a plain maximum and decoding once at the end gives the score, row and column of the
compare-and-select fold it replaces -- replace when (p | 31) >= best, so that a later row wins on an equal score -- for every sequence
of row keys p = score * 32 + column with score <= 1023 and at most 1024 rows."""
import numpy as np
import pytest

ROWS_MAX, SCORE_MAX = 1024, 1023


def fold_select(keys):
    """the fold on compare and select: keys[n, rows] -> (score, row, column) per sequence"""
    n, rows = keys.shape
    best = np.zeros(n, np.uint32)
    besti = np.zeros(n, np.uint32)
    for i in range(rows):
        rk = keys[:, i]
        upd = (rk | np.uint32(31)) >= best
        best = np.where(upd, rk, best)
        besti = np.where(upd, np.uint32(i), besti)
    return best >> 5, besti, best & 31


def fold_key(keys):
    """the fold on one key: a running unsigned maximum, decoded once"""
    n, rows = keys.shape
    p = keys.astype(np.uint64)
    i = np.arange(rows, dtype=np.uint64)[None, :]
    w = (p << 15) | (31 << 15) | (i << 5) | (p & 31)
    assert int(w.max()) < 1 << 32                              # one register
    best = np.maximum.accumulate(np.concatenate([np.zeros((n, 1), np.uint64), w], axis=1), axis=1)[:, -1].astype(np.uint32)
    return best >> 20, (best >> 5) & 1023, best & 31


def agree(keys):
    keys = np.ascontiguousarray(keys, np.uint32)
    assert keys.shape[1] <= ROWS_MAX and int(keys.max()) >> 5 <= SCORE_MAX
    a, b = fold_select(keys), fold_key(keys)
    for x, y, what in zip(a, b, ("score", "row", "column")):
        bad = np.nonzero(x != y)[0]
        assert bad.size == 0, "%s: %d sequences differ, first %d: select %d key %d" % (what, bad.size, bad[0], x[bad[0]], y[bad[0]])
    return a


def keys_of(score, col):
    return (np.asarray(score, np.uint32) << 5) | np.asarray(col, np.uint32)


@pytest.mark.parametrize("rows", [1, 2, 16, 100, 1024])
@pytest.mark.parametrize("top", [0, 1, 3, 200, SCORE_MAX])
def test_random_sequences(rows, top):
    """random scores below a small or a large top (a small one makes equal scores the rule) and random columns 0 ... 14"""
    rng = np.random.default_rng(61000 + rows * 7 + top)
    agree(keys_of(rng.integers(0, top + 1, (500, rows)), rng.integers(0, 15, (500, rows))))


def test_equal_score_later_row_smaller_column():
    """the best score again in later rows, in a smaller column each time: the last of those rows wins, with its own column"""
    rows = 40
    score = np.full((15, rows), 5, np.uint32)
    col = np.zeros((15, rows), np.uint32)
    for k in range(15):
        hits = [3, 9, 20, 31][:1 + k % 4]
        for r, i in enumerate(hits):
            score[k, i] = 77
            col[k, i] = 14 - r - k % 3
    s, i, j = agree(keys_of(score, col))
    for k in range(15):
        last = [3, 9, 20, 31][k % 4]
        assert (s[k], i[k], j[k]) == (77, last, col[k, last])


@pytest.mark.parametrize("rows", [1, 17, 1024])
def test_all_zero_rows(rows):
    """every row's key is score 0 in the last column: the sink is the last row"""
    s, i, j = agree(keys_of(np.zeros((3, rows)), np.full((3, rows), 14)))
    assert (s == 0).all() and (i == rows - 1).all() and (j == 14).all()


def test_best_in_first_and_last_row():
    rows = 100
    rng = np.random.default_rng(62000)
    score = rng.integers(0, 50, (8, rows)).astype(np.uint32)
    col = rng.integers(0, 15, (8, rows)).astype(np.uint32)
    score[:4, 0] = 60                                          # row 0 holds the only best
    score[4:, rows - 1] = 60                                   # the last row does
    score[6:, 0] = 60                                          # ... and row 0 equals it: the last row still wins
    s, i, j = agree(keys_of(score, col))
    assert (s == 60).all() and (i[:4] == 0).all() and (i[4:] == rows - 1).all()
    assert (j[:4] == col[:4, 0]).all() and (j[4:] == col[4:, rows - 1]).all()


def test_fields_at_their_tops():
    """score 1023 and row 1023, alone and together, in columns 0, 14 and 31 (the five bits' top)"""
    rows = 1024
    cases = []
    for c in (0, 14, 31):
        for at in (0, 1022, 1023):
            score = np.zeros(rows, np.uint32); col = np.full(rows, 14, np.uint32)
            score[at] = SCORE_MAX; col[at] = c
            cases.append(keys_of(score, col))
        score = np.full(rows, SCORE_MAX, np.uint32)            # the top score in every row: row 1023 wins
        cases.append(keys_of(score, np.full(rows, c)))
    s, i, j = agree(np.stack(cases))
    assert (s == SCORE_MAX).all()
    assert list(i) == [0, 1022, 1023, 1023] * 3
    assert list(j) == [0] * 4 + [14] * 4 + [31] * 4
