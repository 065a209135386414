"""The max3 cell of the pair kernel in the column frame (nvbio_amd/csrc/banded_gotoh_pair.h: PD3): the horizontal gap step costs no
subtract, the row's zeros are a ring of scalars indexed by (2 i + j) & 15.  Every case is bit-exact against the CPU oracle, score and
sink, with NVBIO_HIP_BANDED_PAIR at 0 (the column frame where the host admits it), 3 (the row-frame cells only), 2 (the u16 cell only)
and 1 (the single-job kernel); nvbio_hip_last_kernel_frame() and nvbio_hip_last_kernel_cell() are asserted on every launch, so no case
is silently routed away from the cell it is about.  tests/test_pair_column_frame.py holds the cell's arithmetic on the CPU.

The cases: the first rows, the ring's wrap at row 8 and the 16-row block seams; 1, 2, 3, 129 and 257 jobs; the tightest text and longer
ones; gap_ext == 0, linear gaps, the all-zero scheme, the byte table's limit and one past it; M at the column frame's own limit and one
above it under a small and a large G; equal best scores in several rows and columns; every string format the pair form takes."""
import numpy as np
import pytest

import nvbio_amd as nvb
from oracle import pyoracle as O
from test_banded_pair_max3_gpu import BAND, SCHEME, Batch, max3_limit, reads_near, run_gpu
from test_banded_pair_row_gpu import scattered

pytestmark = pytest.mark.gpu
SWITCHES = (0, 3, 2, 1)
COUNTS = (1, 2, 3, 129, 257)


def column_admitted(scheme, M):
    """banded_gotoh.hip, pair_column_admitted (for schemes and lengths the max3 cell takes)"""
    match, mismatch, go, ge = scheme
    G, D, s_plus = -32 * ge, 32 * (ge - go), max(match, mismatch, 0)
    return (M <= max3_limit(scheme) and max(match, mismatch) - go - ge <= 7
            and 0x0400 + D + G + G * (2 * M + 14) + 32 * M * s_plus + 255 <= 0x7BFF)


def column_limit(scheme):
    M = 1
    while column_admitted(scheme, M + 1):
        M += 1
    return M


def frame():
    return nvb.lib().nvbio_hip_last_kernel_frame().decode()


def check(b, dev, scheme=SCHEME, expect=("max3", "column"), fetch=None):
    """expect: the (cell, frame) the default launch must run; fetch: how the pair form's launches must read their strings, if given"""
    es, ek = O.batch_banded_gotoh_score(BAND, O.LOCAL, scheme, b.hp, b.ht)
    cell0, frame0 = expect
    want = {0: (cell0, frame0), 3: (cell0, "row" if cell0 else ""), 2: ("u16" if cell0 else "", "row" if cell0 else ""), 1: ("", "")}
    for pair_switch in SWITCHES:
        with nvb.test_switch("NVBIO_HIP_BANDED_PAIR", pair_switch):
            gs, gk, d, c = run_gpu(b, dev, scheme, pair_switch)
            f, ft = frame(), nvb.lib().nvbio_hip_last_kernel_fetch().decode()
        bad = np.nonzero((es != gs) | (ek != gk).any(1))[0]
        assert bad.size == 0, "scheme %s M %d N %d n %d switch %d [%s %s %s]: %d mismatches, first %d: cpu (%d,%s) gpu (%d,%s)" % (
            scheme, b.M, b.N, b.n, pair_switch, d, c, f, bad.size, bad[0], es[bad[0]], ek[bad[0]], gs[bad[0]], gk[bad[0]])
        assert (c, f) == want[pair_switch], (c, f, want[pair_switch], pair_switch, scheme, b.M, b.N)
        assert d == ("pair" if c else ""), (d, c, pair_switch)
        if fetch is not None:
            assert ft == (fetch if c else ""), (ft, fetch, pair_switch)
    return es, ek


@pytest.mark.parametrize("M", [1, 2, 3, 15, 16, 17, 32, 33, 49])
def test_shapes(cuda, M):
    """the first rows, the ring's wrap (row 8 takes the slots row 0 used) and the block seams, at the tightest text and longer ones;
    odd counts leave the last lane with one job in both halves, 129 and 257 jobs are more than one block"""
    rng = np.random.default_rng(81000 + M)
    for n in COUNTS:
        for N in (M + BAND - 1, M + BAND + 6):
            pats, txts = reads_near(rng, n, M, N)
            check(Batch.from_arrays(pats, txts), cuda, fetch="stream")


@pytest.mark.parametrize("scheme,expect", [
    ((2, -1, -2, -1), ("max3", "column")),
    ((2, -1, -2, 0), ("max3", "column")),        # G_e = 0: every column of every row has the same zero, the ring never moves
    ((2, -1, -1, -1), ("max3", "column")),       # D = 0 (linear gaps)
    ((0, 0, 0, 0), ("max3", "column")),
    ((1, 0, -5, -1), ("max3", "column")),        # max(match, mismatch) - G_o + |G_e| = 7: the table's byte is 255, G = 32 of it
    ((2, 0, -5, -1), ("max3", "row")),           # ... 8: the row frame, whose byte is 224
])
def test_schemes(cuda, scheme, expect):
    rng = np.random.default_rng(82000 + sum(abs(v) * 7 ** k for k, v in enumerate(scheme)))
    for M in (1, 17, 100):
        pats, txts = reads_near(rng, 66, M, M + 20)
        pats[0] = txts[0, 14:14 + M]; pats[1] = 3; txts[1] = rng.integers(0, 3, M + 20)      # a perfect match beside a read that matches nothing
        pats[2] = 4; pats[3] = txts[3, :M]
        es, _ = check(Batch.from_arrays(pats, txts), cuda, scheme, expect=expect)
        assert es[0] == scheme[0] * M and es[1] == 0 and es[2] == 0


@pytest.mark.parametrize("scheme", [(2, -1, -2, -1), (1, 0, -3, -3)])          # G = 32: M <= 234;  G = 96: M <= 129
def test_range(cuda, scheme):
    """M at the column frame's limit: a perfect match drives one half to the top of the f16 range while the other stays at the row's
    zero, in both orders; one symbol more falls to the max3 cell in the row frame"""
    L = column_limit(scheme)
    assert L == {32: 234, 96: 129}[-32 * scheme[3]] and L + 1 <= max3_limit(scheme)
    rng = np.random.default_rng(83000 + scheme[0])
    for M, expect in ((L, ("max3", "column")), (L + 1, ("max3", "row"))):
        N = M + BAND + 3
        txts = rng.integers(0, 3, (6, N), dtype=np.uint8)
        pats = np.full((6, M), 3, np.uint8)                                      # score 0
        for i in (0, 3, 4):                                                      # (perfect, zero), (zero, perfect), (perfect, zero)
            pats[i] = txts[i, 14:14 + M]
        es, ek = check(Batch.from_arrays(pats, txts), cuda, scheme, expect=expect)
        assert list(es) == [scheme[0] * M, 0, 0, scheme[0] * M, scheme[0] * M, 0]
        assert tuple(ek[0]) == (M + 14, M)
        pats, txts = reads_near(rng, 33, M, M + BAND - 1)
        check(Batch.from_arrays(pats, txts), cuda, scheme, expect=expect)


@pytest.mark.parametrize("M", [17, 33])
def test_ties(cuda, M):
    """the best score in several rows and several columns: nothing matches (every cell holds 0: the last row, column 14), homopolymer
    read and text (every column of the last row holds 2 M), and reads that match at two offsets in two rows: the later row, then the
    larger column, wins"""
    rng = np.random.default_rng(84000 + M)
    N = M + 20
    run = (M - 1) // 4
    pats, txts, want = [], [], []
    pats.append(np.full(M, 3, np.uint8)); txts.append(rng.integers(0, 3, N, dtype=np.uint8)); want.append((0, M - 1, 14))
    pats.append(np.full(M, 2, np.uint8)); txts.append(np.full(N, 2, np.uint8)); want.append((2 * M, M - 1, 14))
    for period in (1, 2):
        for c in range(BAND - period):
            unit = np.array([0, 1][:period], np.uint8)
            p = np.full(M, 4, np.uint8)
            p[:run] = np.resize(unit, run); p[M - run:] = np.resize(unit, run)
            t = np.full(N, 2, np.uint8)
            t[c:c + run + period] = np.resize(unit, run + period)
            t[c + M - run:c + M + period] = np.resize(unit, run + period)
            pats.append(p); txts.append(t); want.append((2 * run, M - 1, c + period))
    es, ek = check(Batch.from_arrays(pats, txts), cuda)
    for k, (score, row, col) in enumerate(want):
        assert es[k] == score and tuple(ek[k]) == (row + col + 1, row + 1), (k, es[k], ek[k], score, row, col)


@pytest.mark.parametrize("pbits,pbe", [(2, False), (2, True), (4, False), (4, True), (8, False), (8, True)])
def test_formats(cuda, pbits, pbe):
    """2-, 4- and 8-bit patterns (4 and 8 bits hold symbols that equal no text symbol), both byte orders of pattern and text, strings
    at every offset in their words and ending in their arrays' last words: the eight streamed instances and the generic one"""
    rng = np.random.default_rng(85000 + 2 * pbits + pbe)
    for M, n in ((17, 129), (49, 3)):
        for tbe in (False, True):
            b = scattered(rng, n, M, M + BAND - 1, pbits, pbe, tbe)
            check(b, cuda, fetch="generic" if pbits == 8 else "stream")
