"""The two cells of the two-jobs-per-lane banded Gotoh score kernel (nvbio_amd/csrc/banded_gotoh_pair.h): PM3, which takes its maxima three
at a time with v_pk_maximum3_f16 on halves kept inside the positive normal f16 patterns 0x0400 ... 0x7BFF, and P16, the v_pk_max_u16
cell it falls back to above its range.  Every case is bit-exact against the CPU oracle, score and sink, with NVBIO_HIP_BANDED_PAIR at
0 (the max3 cell where the host admits it), 2 (the pair form with the u16 cell only) and 1 (the single-job kernel);
nvbio_hip_last_kernel_cell() says which cell a launch ran, so no case is silently routed away from the cell it is about.

The values the cases drive: the top of the f16 range (M at the host's own limit, a perfect match beside a zero), its bottom (nothing
matches, under the schemes with the largest and the smallest frame offsets), equal zeros in consecutive rows (gap_ext == 0: the clamp
folded into F), the best cell in every band column and repeated in neighbouring columns and later rows (the row key takes two columns
at a time), the first rows and the 16-row block edges."""
import numpy as np
import pytest
import torch

import nvbio_amd as nvb
import width_limits as W
from oracle import pyoracle as O

pytestmark = pytest.mark.gpu
BAND = 15
SCHEME = (2, -1, -2, -1)
SWITCHES = (0, 2, 1)
PM3_ROW_LIMIT = (0x7BFF - 255 - 0x0400 - 448) // 32          # banded_gotoh_pair.h: the largest M (S+ + |G_e|) of the max3 cell


def max3_limit(scheme):
    """banded_gotoh.hip, pair_max3_admitted: the longest pattern the max3 cell takes"""
    match, mismatch, _, ge = scheme
    per_row = max(match, mismatch, 0) - ge
    return W.ALWAYS if per_row == 0 else PM3_ROW_LIMIT // per_row


def detail():
    return nvb.lib().nvbio_hip_last_kernel_detail().decode()


def cell():
    return nvb.lib().nvbio_hip_last_kernel_cell().decode()


class Batch:
    """n fixed-length jobs over one pattern stream and one text stream; the oracle reads the same words through per-job lengths"""

    def __init__(self, pwords, pbits, pbe, pbegin, M, twords, tbe, tbegin, N):
        n = len(pbegin)
        self.M, self.N, self.n = M, N, n
        self.hp = O.StringSet(pwords, pbits, pbe, np.asarray(pbegin, np.uint64), np.full(n, M, np.uint32))
        self.ht = O.StringSet(twords, 2, tbe, np.asarray(tbegin, np.uint64), np.full(n, N, np.uint32))

    @staticmethod
    def from_arrays(pats, txts, pbits=4, pbe=True, tbe=False):
        """pats / txts: n x M and n x N symbol arrays, stored back to back"""
        pats, txts = np.asarray(pats, np.uint8), np.asarray(txts, np.uint8)
        n, M = pats.shape
        N = txts.shape[1]
        return Batch(O.pack(pats.reshape(-1), pbits, pbe), pbits, pbe, np.arange(n) * M, M, O.pack(txts.reshape(-1), 2, tbe), tbe, np.arange(n) * N, N)

    def device(self, dev):
        p = nvb.PackedStringSet.from_host(self.hp.words, self.hp.bits, self.hp.big_endian, self.hp.begin, None, self.M, device=dev)
        t = nvb.PackedStringSet.from_host(self.ht.words, 2, self.ht.big_endian, self.ht.begin, None, self.N, device=dev)
        return p, t


def run_gpu(b, dev, scheme, pair_switch):
    p, t = b.device(dev)
    with nvb.test_switch("NVBIO_HIP_BANDED_PAIR", pair_switch):
        score, sink = nvb.batch_banded_alignment_score(BAND, nvb.make_gotoh_aligner(nvb.LOCAL, nvb.SimpleGotohScheme(*scheme)), p, t)
        torch.cuda.synchronize()
        d, c = detail(), cell()
    return score.cpu().numpy(), sink.cpu().numpy().view(np.uint32), d, c


def check(b, dev, scheme=SCHEME, expect="max3"):
    """expect: the cell the default launch must run -- "max3", "u16", or "" for a batch the pair form does not admit"""
    es, ek = O.batch_banded_gotoh_score(BAND, O.LOCAL, scheme, b.hp, b.ht)
    for pair_switch in SWITCHES:
        gs, gk, d, c = run_gpu(b, dev, scheme, pair_switch)
        bad = np.nonzero((es != gs) | (ek != gk).any(1))[0]
        assert bad.size == 0, "scheme %s M %d N %d n %d switch %d [%s %s]: %d mismatches, first %d: cpu (%d,%s) gpu (%d,%s)" % (
            scheme, b.M, b.N, b.n, pair_switch, d, c, bad.size, bad[0], es[bad[0]], ek[bad[0]], gs[bad[0]], gk[bad[0]])
        want = {0: expect, 2: "u16" if expect else "", 1: ""}[pair_switch]
        assert c == want, (c, want, pair_switch, scheme, b.M, b.N)
        assert d == ("pair" if want else ""), (d, want, pair_switch, scheme, b.M, b.N)
    return es, ek


def reads_near(rng, n, M, N, band=BAND, sym=4):
    """texts of N symbols and reads of M cut out of them a few columns into the band, with mutations (an N among them) and an indel"""
    txts = rng.integers(0, 4, (n, N), dtype=np.uint8)
    pats = np.empty((n, M), np.uint8)
    for i in range(n):
        off = int(rng.integers(0, band))
        p = np.resize(txts[i, off:off + M], M).copy()
        mut = rng.random(M) < 0.08
        p[mut] = rng.integers(0, sym + 1, int(mut.sum()), dtype=np.uint8)
        if M > 20 and rng.random() < 0.3:
            cut = int(rng.integers(5, M - 5))
            p = np.concatenate([p[:cut], p[cut + 2:], rng.integers(0, 4, 2, dtype=np.uint8)])
        pats[i] = p
    return pats, txts


@pytest.mark.parametrize("scheme", [SCHEME, (5, -1, -2, -1)])          # the headline scheme; the largest substitution byte, 224
def test_range_top(cuda, scheme):
    """M at the max3 cell's limit: a perfect match drives one half to the largest value the cell admits, 0x0400 + BIAS + 32 M (S+ +
    |G_e|), with a full substitution byte on top in the diagonal, while the other half stays at the row's zero, in both orders; one
    symbol more takes the u16 cell, still in the pair form"""
    L = max3_limit(scheme)
    lim16, _ = W.banded_limits(W.Scheme.gotoh(*scheme), W.LOCAL, BAND)
    assert 0 < L < lim16
    rng = np.random.default_rng(51000 + scheme[0])
    for M, expect in ((L, "max3"), (L + 1, "u16")):
        N = M + BAND + 3
        txts = rng.integers(0, 3, (6, N), dtype=np.uint8)
        pats = np.full((6, M), 3, np.uint8)                                      # score 0
        for i in (0, 3, 4):                                                      # (perfect, zero), (zero, perfect), (perfect, zero)
            pats[i] = txts[i, 14:14 + M]
        es, ek = check(Batch.from_arrays(pats, txts), cuda, scheme, expect=expect)
        assert list(es) == [scheme[0] * M, 0, 0, scheme[0] * M, scheme[0] * M, 0]
        assert tuple(ek[0]) == (M + 14, M)


@pytest.mark.parametrize("scheme,expect", [
    ((0, -1, -7, -7), "max3"),      # the largest D + G the byte table admits (match - gap_open = 7), all of it in G: D = 0, G = 224
    ((0, 0, -7, 0), "max3"),        # ... all of it in D: D = 224, G = 0, every row has the same zero
    ((0, -3, -7, -1), "max3"),      # D = 192, G = 32
    ((2, -1, -1, -1), "max3"),      # D = 0 (linear gaps)
    ((0, 0, 0, 0), "max3"),         # D = G = 0: every value of every row is the frame's floor
    ((2, -1, -7, -7), ""),          # match - gap_open = 9 does not fit the byte table: the single-job kernel
])
def test_range_bottom(cuda, scheme, expect):
    """reads that match nothing and reads of N only: h stays at the row's zero and S, E at Z - D, Z - D - G, the lowest values of the frame"""
    rng = np.random.default_rng(52000 + sum(abs(v) * 7 ** k for k, v in enumerate(scheme)))
    for M in (1, 2, 100):
        N = M + 20
        txts = rng.integers(0, 3, (9, N), dtype=np.uint8)
        pats = np.full((9, M), 3, np.uint8)                                      # all-mismatch
        pats[1::3] = 4                                                           # all-N
        pats[2::3] = txts[2::3, 5:5 + M]                                         # (a match beside them)
        es, _ = check(Batch.from_arrays(pats, txts), cuda, scheme, expect=expect)
        assert (es[0::3] == 0).all() and (es[1::3] == 0).all() and (es[2::3] == scheme[0] * M).all()


@pytest.mark.parametrize("scheme", [(2, -1, -2, 0), (1, 0, -1, 0)])
def test_gap_ext_zero(cuda, scheme):
    """gap_ext == 0: consecutive rows have equal zeros, the case of equality in F' = max(F, Z_i); the periodic reads of the sink-tie
    test, whose gaps cost no more however long they are"""
    rng = np.random.default_rng(53000 + scheme[0])
    for M in (16, 33, 100):
        pats, txts = [], []
        for period in (1, 2, 3, 4, 7):
            unit = rng.integers(0, 4, period, dtype=np.uint8)
            for cutmid in (False, True):
                p = np.resize(unit, M).copy()
                if cutmid and period > 1:
                    p[M // 2] = (p[M // 2] + 1) & 3                              # two equal runs either side of a mismatch
                pats.append(p); txts.append(np.resize(unit, M + 20))
        pats.append(np.zeros(M, np.uint8)); txts.append(np.full(M + 20, 1, np.uint8))
        pats.append(np.full(M, 4, np.uint8)); txts.append(rng.integers(0, 4, M + 20, dtype=np.uint8))
        es, _ = check(Batch.from_arrays(pats, txts), cuda, scheme)
        assert (es == 0).any() and (es > 0).any()


@pytest.mark.parametrize("M", [16, 33])
def test_key_pairing(cuda, M):
    """the row key is folded two columns at a time -- (1,2) ... (11,12), (13,14), column 0 alone.  A read cut from the text at offset c
    has its best cell in column c of the last row; reads of two runs of a period-1 or period-2 unit, against a text that holds each run
    with `period` symbols to spare, reach their best score in columns c and c + period of the first run's last row AND of the last row:
    the later row, then the higher column, must win"""
    rng = np.random.default_rng(54000 + M)
    N = M + 20
    pats, txts, want = [], [], []
    for c in range(BAND):                                                        # one best cell, in column c
        t = rng.integers(0, 4, N, dtype=np.uint8)
        pats.append(t[c:c + M].copy()); txts.append(t); want.append((2 * M, c))
    run = (M - 1) // 4                                                           # two runs of `run` symbols around >= 2 run symbols of N
    for period in (1, 2):
        for c in range(BAND - period):                                           # the best score in columns c and c + period
            unit = np.array([0, 1][:period], np.uint8)
            p = np.full(M, 4, np.uint8)
            p[:run] = np.resize(unit, run); p[M - run:] = np.resize(unit, run)
            t = np.full(N, 2, np.uint8)
            t[c:c + run + period] = np.resize(unit, run + period)
            t[c + M - run:c + M + period] = np.resize(unit, run + period)
            pats.append(p); txts.append(t); want.append((2 * run, c + period))
    es, ek = check(Batch.from_arrays(pats, txts), cuda)
    for k, (score, col) in enumerate(want):
        assert es[k] == score and tuple(ek[k]) == (M + col, M), (k, es[k], ek[k], score, col)


@pytest.mark.parametrize("M", [1, 2, 15, 16, 17])
def test_first_rows_and_block_edges(cuda, M):
    """the first rows (F' and S still at their starting values) and M around the 16-row block, at the tightest text the pair form takes;
    67 jobs: the last lane holds one job in both halves"""
    rng = np.random.default_rng(55000 + M)
    pats, txts = reads_near(rng, 67, M, M + 14)
    check(Batch.from_arrays(pats, txts), cuda)


def test_three_routes_agree(cuda):
    """4 096 jobs of extreme and ordinary kinds, as given and with neighbours swapped: the max3 cell, the u16 cell and the single-job
    kernel return the same arrays, whichever job shares a lane and whichever half it sits in"""
    rng = np.random.default_rng(56000)
    M, N, n = 100, 150, 4096
    pats, txts = reads_near(rng, n, M, N)
    for i in range(n):
        kind = i % 5 if i < 3000 else int(rng.integers(0, 5))
        if kind == 0:
            pats[i] = txts[i, 7:7 + M]                                           # perfect match: 2 M
        elif kind == 1:
            txts[i] = rng.integers(0, 3, N); pats[i] = 3                         # nothing matches
        elif kind == 2:
            pats[i] = 4                                                          # a read of N only
        elif kind == 3:
            pats[i] = i % 4; txts[i] = i % 4                                     # homopolymers
    order = rng.permutation(n)                                                   # (so that unlike kinds share lanes)
    pats, txts = pats[order], txts[order]
    swap = np.arange(n) ^ 1
    es, ek = check(Batch.from_arrays(pats, txts), cuda)                          # (check compares every route with the oracle's arrays)
    assert es.max() == 2 * M and es.min() == 0
    ps, ks = check(Batch.from_arrays(pats[swap], txts[swap]), cuda)
    assert (ps == es[swap]).all() and (ks == ek[swap]).all()
