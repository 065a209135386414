"""What a row of the two-jobs-per-lane banded Gotoh kernel does outside its cells (nvbio_amd/csrc/banded_gotoh_pair.h): the block loop's
streamed word fetches (common.h: GroupStream) and the sink fold.  Every case is bit-exact against the CPU oracle, score and sink, with
NVBIO_HIP_BANDED_PAIR at 0, 2 and 1, and checks which cell the launch ran (the helpers of test_banded_pair_max3_gpu.py); the fetch
cases also check which fetch it took (nvbio_hip_last_kernel_fetch), so none passes on the generic fetches alone; the batches have 1, 2, 3, 129 and 257 jobs: one lane with one job, odd counts, more than one block.

Fetch: M around the 16-row block with the tightest text the pair form takes (N = M + 14), patterns and texts that begin at every
symbol offset within a word, patterns of 2, 4 and 8 bits in both byte orders, and a last job whose strings end in the last word of
their arrays, so that every word the loop asks for past them is the clamped one.
Sink: nothing matches (the last row, column 14), equal best scores in several rows and columns, rows and scores up to 1022, and 1023
and 1024 rows under a scheme with no 16-bit limit."""
import numpy as np
import pytest

import width_limits as W
from oracle import pyoracle as O
import nvbio_amd as nvb
from test_banded_pair_max3_gpu import BAND, Batch, check, max3_limit, run_gpu

pytestmark = pytest.mark.gpu
COUNTS = (1, 2, 3, 129, 257)


def scattered(rng, n, M, N, pbits, pbe, tbe):
    """n jobs whose patterns begin at symbol offset k mod (symbols per word) of a word and whose texts begin at offset 5 k mod 16, packed
    with no spare word: the last job's strings end in the last word of their arrays.  Reads are cut from their texts a few columns into
    the band and mutated (with symbols that equal no text symbol where the pattern's width has any)"""
    pper, top = 32 // pbits, 4 if pbits == 2 else 5
    txts = rng.integers(0, 4, (n, N), dtype=np.uint8)
    pats = np.empty((n, M), np.uint8)
    for k in range(n):
        off = int(rng.integers(0, BAND))
        p = np.resize(txts[k, off:off + M], M).copy()
        mut = rng.random(M) < 0.1
        p[mut] = rng.integers(0, top, int(mut.sum()), dtype=np.uint8)
        pats[k] = p
    pbegin, tbegin, ppos, tpos = [], [], 0, 0
    for k in range(n):
        ppos += (k % pper - ppos) % pper
        tpos += (5 * k % 16 - tpos) % 16
        pbegin.append(ppos); tbegin.append(tpos)
        ppos += M; tpos += N
    psym = np.zeros(ppos, np.uint8); tsym = np.zeros(tpos, np.uint8)
    for k in range(n):
        psym[pbegin[k]:pbegin[k] + M] = pats[k]
        tsym[tbegin[k]:tbegin[k] + N] = txts[k]
    pw, tw = O.pack(psym, pbits, pbe, pad_words=0), O.pack(tsym, 2, tbe, pad_words=0)
    assert pw.size == (ppos + pper - 1) // pper and tw.size == (tpos + 15) // 16
    return Batch(pw, pbits, pbe, pbegin, M, tw, tbe, tbegin, N)


@pytest.mark.parametrize("M", [1, 15, 16, 17, 31, 32, 33, 100])
@pytest.mark.parametrize("pbits,pbe", [(2, False), (2, True), (4, False), (4, True), (8, False), (8, True)])
def test_fetch(cuda, M, pbits, pbe):
    rng = np.random.default_rng(71000 + 100 * M + 2 * pbits + pbe)
    for n in COUNTS:
        for tbe in (False, True):
            b = scattered(rng, n, M, M + BAND - 1, pbits, pbe, tbe)
            check(b, cuda)
            # which fetch the pair form's launch took: the streamed one for 2 and 4 bits, the generic one for 8, none off the pair form
            for pair_switch, want in ((0, "generic" if pbits == 8 else "stream"), (1, "")):
                run_gpu(b, cuda, (2, -1, -2, -1), pair_switch)
                assert nvb.lib().nvbio_hip_last_kernel_fetch().decode() == want, (pair_switch, pbits, pbe, tbe, M, n)


@pytest.mark.parametrize("scheme", [(2, -1, -2, -1), (1, 0, -1, 0)])
def test_nothing_matches(cuda, scheme):
    """every row's best is 0 in every column: the sink is the last row, column 14"""
    rng = np.random.default_rng(72000 + scheme[0])
    for n in COUNTS:
        for M in (1, 16, 100):
            N = M + 17
            txts = rng.integers(0, 3, (n, N), dtype=np.uint8)
            pats = np.full((n, M), 3 if scheme[1] < 0 else 4, np.uint8)
            es, ek = check(Batch.from_arrays(pats, txts), cuda, scheme)
            assert (es == 0).all() and (ek == (M + 14, M)).all()


@pytest.mark.parametrize("scheme", [(2, -1, -2, -1), (2, -1, -2, 0)])
def test_equal_best_scores(cuda, scheme):
    """periodic reads against periodic texts, two runs either side of symbols that match nothing: the best score stands in several
    columns of several rows, and the later row, then the higher column, must win -- whichever half of the lane the job sits in"""
    rng = np.random.default_rng(73000 - scheme[3])
    M, N = 48, 70
    for n in COUNTS:
        pats, txts = [], []
        for k in range(n):
            period, run = 1 + k % 4, 8 + k % 9
            unit = rng.permutation(4)[:period].astype(np.uint8)
            p = np.full(M, 4, np.uint8)
            p[:run] = np.resize(unit, run); p[M - run:] = np.resize(unit, run)
            t = np.resize(unit, N) if k % 3 else np.concatenate([np.resize(unit, N // 2), np.full(N - N // 2, (int(unit[0]) + 1) & 3, np.uint8)])
            pats.append(p); txts.append(t)
        es, _ = check(Batch.from_arrays(pats, txts), cuda, scheme)
        assert (es > 0).all()


def long_batch(rng, n, M):
    """jobs of M rows: perfect matches at band columns 0, 7 and 14, reads that match nothing, and noise"""
    N = M + BAND + 2
    txts = rng.integers(0, 3, (n, N), dtype=np.uint8)
    pats = np.full((n, M), 3, np.uint8)
    for k in range(n):
        if k % 5 < 3:
            c = (0, 7, 14)[k % 5]
            pats[k] = txts[k, c:c + M]
        elif k % 5 == 4:
            pats[k] = rng.integers(0, 4, M, dtype=np.uint8)
    return Batch.from_arrays(pats, txts)


def test_row_field_max3_limit(cuda):
    """(1,-1,-1,0) at the max3 cell's limit, M = 938: a perfect match ends in row 937 with score 938"""
    scheme, M = (1, -1, -1, 0), 938
    assert max3_limit(scheme) == M
    rng = np.random.default_rng(74000)
    for n in COUNTS:
        es, ek = check(long_batch(rng, n, M), cuda, scheme, expect="max3")
        assert es[0] == M and tuple(ek[0]) == (M, M)


def test_row_field_u16_limit(cuda):
    """the same scheme at the u16 cell's limit, M = 1022: rows and scores up to 1021 and 1022"""
    scheme, M = (1, -1, -1, 0), 1022
    lim16, _ = W.banded_limits(W.Scheme.gotoh(*scheme), W.LOCAL, BAND)
    assert lim16 == M
    rng = np.random.default_rng(75000)
    for n in COUNTS:
        es, ek = check(long_batch(rng, n, M), cuda, scheme, expect="u16")
        assert es[0] == M and tuple(ek[0]) == (M, M)
        if n > 2:
            assert es[2] == M and tuple(ek[2]) == (M + 14, M)


def test_rows_past_ten_bits(cuda):
    """(0,-1,-1,0) scores nothing and has no 16-bit limit, so the pair form takes it at any length: the sink's row is a register of its
    own and 1023 and 1024 rows both end in their last row"""
    scheme = (0, -1, -1, 0)
    lim16, _ = W.banded_limits(W.Scheme.gotoh(*scheme), W.LOCAL, BAND)
    assert lim16 == W.ALWAYS
    rng = np.random.default_rng(76000)
    for M in (1023, 1024):
        for n in COUNTS:
            es, ek = check(long_batch(rng, n, M), cuda, scheme, expect="max3")
            assert (es == 0).all() and (ek == (M + 14, M)).all()
