"""The row around the column frame's cells (nvbio_amd/csrc/banded_gotoh_pair.h: PF_FOLD2, the sink folded once per two rows), bit-exact
against the CPU oracle, score and sink.  Every case runs with
NVBIO_HIP_PAIR_ROW at 0 (the new row) and at 1 (the row as it was), and nvbio_hip_last_kernel_row() is asserted on every launch, so no
case is silently routed elsewhere.

Shapes: M on both sides of every 16-row seam (no pair straddles one), a lone row and odd tails
(the pair fold's last row without a partner), 1, 2, 3, 129 and 257 jobs, N = M + 14 and M + 21.  Ties: the all-zero scheme, and equal
bests constructed in both rows of a pair and across pairs, which a small numpy DP confirms.  The table's sixteen entries through 4-bit
patterns with symbols 4 ... 15; 2-bit patterns in both byte orders of pattern and text; 8-bit patterns on the generic fetches.  The
column frame's limit, M = 234 under (2,-1,-2,-1), and one row past it, which keeps the row frame and its row."""
import numpy as np
import pytest
import torch

import nvbio_amd as nvb
from oracle import pyoracle as O
from test_banded_pair_max3_gpu import BAND, Batch, reads_near, run_gpu
from test_banded_pair_row_gpu import scattered

pytestmark = pytest.mark.gpu
HEADLINE = (2, -1, -2, -1)
COUNTS = (1, 2, 3, 129, 257)
LENGTHS = (1, 2, 3, 4, 15, 16, 17, 18, 31, 32, 33, 47, 48, 49)
NEW_ROW = "fold2"


def launch_facts():
    L = nvb.lib()
    return (L.nvbio_hip_last_kernel_detail().decode(), L.nvbio_hip_last_kernel_frame().decode(), L.nvbio_hip_last_kernel_row().decode(),
            L.nvbio_hip_last_kernel_fetch().decode())


def check(b, dev, scheme=HEADLINE, frame="column", fetch="stream"):
    """both rows against the oracle; frame: the frame the default launch must take ("column": the new row is the default's)"""
    es, ek = O.batch_banded_gotoh_score(BAND, O.LOCAL, scheme, b.hp, b.ht)
    for row_switch in (0, 1):
        with nvb.test_switch("NVBIO_HIP_PAIR_ROW", row_switch):
            gs, gk, _, _ = run_gpu(b, dev, scheme, 0)
            torch.cuda.synchronize()
            facts = launch_facts()
        want = ("pair", frame, NEW_ROW if frame == "column" and row_switch == 0 else "plain", fetch)
        assert facts == want, (facts, want, scheme, b.M, b.N, b.n)
        bad = np.nonzero((es != gs) | (ek != gk).any(1))[0]
        assert bad.size == 0, "scheme %s M %d N %d n %d row switch %d: %d mismatches, first %d: cpu (%d,%s) gpu (%d,%s)" % (
            scheme, b.M, b.N, b.n, row_switch, bad.size, bad[0], es[bad[0]], ek[bad[0]], gs[bad[0]], gk[bad[0]])
    return es, ek


@pytest.mark.parametrize("M", LENGTHS)
def test_seams_and_tails(cuda, M):
    rng = np.random.default_rng(91000 + M)
    for n in COUNTS:
        for N in (M + 14, M + 21):
            pats, txts = reads_near(rng, n, M, N)
            check(Batch.from_arrays(pats, txts), cuda)


@pytest.mark.parametrize("M", LENGTHS)
def test_all_zero_scheme(cuda, M):
    """every cell of every row ties at 0: the last row's last column must win, with and without a partner for the last row"""
    rng = np.random.default_rng(92000 + M)
    pats, txts = reads_near(rng, 129, M, M + 14)
    es, ek = check(Batch.from_arrays(pats, txts), cuda, (0, 0, 0, 0))
    assert (es == 0).all() and (ek == (M + 14, M)).all()


def row_bests(p, t, scheme=HEADLINE):
    """a plain banded Gotoh LOCAL DP of one job: the best score of every row and the columns that hold it"""
    match, mismatch, go, ge = scheme
    NEG = -(1 << 30)
    H = np.zeros(BAND, np.int64); F = np.full(BAND, NEG, np.int64)
    out = []
    for i in range(len(p)):
        Hn = np.zeros(BAND, np.int64); Fn = np.full(BAND, NEG, np.int64); E = NEG
        for j in range(BAND):
            s = match if p[i] == t[i + j] and p[i] < 4 else mismatch
            if j + 1 < BAND:
                Fn[j] = max(F[j + 1] + ge, H[j + 1] + go)
            if j > 0:
                E = max(E + ge, Hn[j - 1] + go)
            Hn[j] = max(0, H[j] + s, E, Fn[j])
        H, F = Hn, Fn
        out.append((int(H.max()), [j for j in range(BAND) if H[j] == H.max()]))
    return out


def two_runs(M, first_end, c1, last_end, c2, run=6):
    """a read of symbol 4 (matches nothing) with two runs of `run` distinct-neighbour symbols ending in rows first_end and last_end,
    which the text holds on band columns c1 and c2: the best score 2 * run stands in exactly those two cells"""
    N = M + 21
    unit = np.array([0, 1, 2, 0, 2, 1, 0], np.uint8)
    p = np.full(M, 4, np.uint8); t = np.full(N, 3, np.uint8)
    if last_end == first_end + 1:
        # neighbouring rows: one run of run + 1 symbols, whose first `run` the text holds on column c1 and whose last `run` on column c2
        lo = first_end - run + 1
        p[lo:last_end + 1] = unit[:run + 1]
        t[lo + c1:first_end + 1 + c1] = unit[:run]
        t[lo + 1 + c2:last_end + 1 + c2] = unit[1:run + 1]
        return p, t
    for end, c in ((first_end, c1), (last_end, c2)):
        p[end - run + 1:end + 1] = unit[:run]
        t[end - run + 1 + c:end + 1 + c] = unit[:run]
    return p, t


@pytest.mark.parametrize("M", [32, 33])
def test_constructed_ties(cuda, M):
    """equal bests in the even and the odd row of one pair with the later row's column smaller, the same with the pair's rows the other
    way round in time (odd then even: different pairs), and pairs apart; in both halves of a lane"""
    run = 6
    cases = [
        (12, 11, 13, 2),      # rows 12 and 13: one pair, the later row's column smaller
        (12, 2, 13, 11),      # ... larger
        (13, 11, 14, 2),      # rows 13 and 14: neighbouring rows of different pairs
        (6, 13, 27, 5),       # pairs apart, the later one in its odd row
        (7, 12, 28, 6),       # ... in its even row
        (9, 13, M - 1, 1),    # the last row: the odd row of the last pair (M = 32) or a row without a partner (M = 33)
    ]
    pats, txts, want = [], [], []
    for first_end, c1, last_end, c2 in cases:
        p, t = two_runs(M, first_end, c1, last_end, c2, run)
        rows = row_bests(p, t)
        top = max(s for s, _ in rows)
        holders = [(i, cols) for i, (s, cols) in enumerate(rows) if s == top]
        assert top == 2 * run and holders == [(first_end, [c1]), (last_end, [c2])], (holders, top)     # the tie is really there
        pats.append(p); txts.append(t); want.append((top, last_end, c2))
    pats, txts = np.array(pats), np.array(txts)
    for order in (np.arange(len(cases)), np.arange(len(cases))[::-1], np.array([0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 0])):
        es, ek = check(Batch.from_arrays(pats[order], txts[order]), cuda)
        for k, c in enumerate(order):
            score, row, col = want[c]
            assert es[k] == score and tuple(ek[k]) == (row + col + 1, row + 1), (k, c, es[k], ek[k], want[c])


@pytest.mark.parametrize("M", [16, 17, 33])
def test_table_entries_4_to_15(cuda, M):
    """4-bit patterns with symbols 4 ... 15 among them: the rows index every entry of the table"""
    rng = np.random.default_rng(93000 + M)
    for n in (3, 129):
        pats, txts = reads_near(rng, n, M, M + 14)
        hit = rng.random(pats.shape) < 0.3
        pats[hit] = rng.integers(4, 16, int(hit.sum()), dtype=np.uint8)
        assert set(range(4, 16)) <= set(pats.reshape(-1).tolist()) or n == 3
        for pbe in (False, True):
            check(Batch.from_arrays(pats, txts, pbits=4, pbe=pbe), cuda)


@pytest.mark.parametrize("M", [15, 17, 32, 49])
@pytest.mark.parametrize("pbits,pbe", [(2, False), (2, True), (8, False), (8, True)])
def test_pattern_widths(cuda, M, pbits, pbe):
    """2-bit patterns in both byte orders of pattern and text (four more streamed instances), 8-bit patterns on the generic fetches;
    strings that begin at every symbol offset within a word"""
    rng = np.random.default_rng(94000 + 100 * M + 2 * pbits + pbe)
    for n in (3, 129):
        for tbe in (False, True):
            check(scattered(rng, n, M, M + BAND - 1, pbits, pbe, tbe), cuda, fetch="generic" if pbits == 8 else "stream")


@pytest.mark.parametrize("scheme", [
    HEADLINE,
    (2, -1, -2, 0),       # gap_ext == 0: both rows of a pair stand in one frame
    (2, -1, -1, -1),      # linear gaps, D = 0
    (4, -1, -2, -1),      # the table's byte at its limit, 255
    (1, 0, -5, -1),       # ... by the gap costs
])
def test_schemes(cuda, scheme):
    rng = np.random.default_rng(95000 + sum(abs(v) * 5 ** k for k, v in enumerate(scheme)))
    for M in (17, 48, 49):
        pats, txts = reads_near(rng, 129, M, M + 14)
        check(Batch.from_arrays(pats, txts), cuda, scheme)


def test_column_frame_limit(cuda):
    """M = 234, the column frame's limit under the headline scheme (an even M at the top of the range: the last pair's key is the largest
    operand the fold sees), and M = 235, which keeps the row frame and the row it had"""
    rng = np.random.default_rng(96000)
    for M, frame in ((234, "column"), (235, "row")):
        N = M + BAND + 3
        txts = rng.integers(0, 3, (6, N), dtype=np.uint8)
        pats = np.full((6, M), 3, np.uint8)
        for i in (0, 3, 4):                                                      # (perfect, zero), (zero, perfect), (perfect, zero)
            pats[i] = txts[i, 14:14 + M]
        es, ek = check(Batch.from_arrays(pats, txts), cuda, frame=frame)
        assert list(es) == [2 * M, 0, 0, 2 * M, 2 * M, 0] and tuple(ek[0]) == (M + 14, M)
        pats, txts = reads_near(rng, 5, M, M + 14)
        check(Batch.from_arrays(pats, txts), cuda, frame=frame)
