"""The two-jobs-per-lane form of the 16-bit LOCAL banded Gotoh score kernel (nvbio_amd/csrc/banded_gotoh_pair.h), against the CPU oracle
bit for bit, score and sink.  Every case runs with NVBIO_HIP_BANDED_PAIR at 0 (the pair form where the host admits it) and at 1 (never);
nvbio_hip_last_kernel_detail() says which form a launch took.  Fixed-length batches throughout: the pair form takes nothing else.

Band 15 is the one instantiated band.  The kernel has one block size (128 lanes = 256 jobs per workgroup), so the lane and block edges
below are its only ones."""
import numpy as np
import pytest
import torch

import nvbio_amd as nvb
import width_limits as W
from oracle import pyoracle as O

pytestmark = pytest.mark.gpu
BAND = 15
SCHEME = (2, -1, -2, -1)


def detail():
    return nvb.lib().nvbio_hip_last_kernel_detail().decode()


class Batch:
    """n fixed-length jobs over one pattern stream and one text stream; the oracle reads the same words through per-job lengths"""

    def __init__(self, pwords, pbits, pbe, pbegin, M, twords, tbe, tbegin, N):
        n = len(pbegin)
        self.M, self.N, self.n = M, N, n
        self.hp = O.StringSet(pwords, pbits, pbe, np.asarray(pbegin, np.uint64), np.full(n, M, np.uint32))
        self.ht = O.StringSet(twords, 2, tbe, np.asarray(tbegin, np.uint64), np.full(n, N, np.uint32))

    @staticmethod
    def from_arrays(pats, txts, pbits=4, pbe=True, tbe=False, lead_p=0, lead_t=0):
        """pats / txts: n x M and n x N symbol arrays, stored back to back after lead_p / lead_t symbols (begins off the word grid)"""
        pats, txts = np.asarray(pats, np.uint8), np.asarray(txts, np.uint8)
        n, M = pats.shape
        N = txts.shape[1]
        pcat = np.concatenate([np.zeros(lead_p, np.uint8), pats.reshape(-1)])
        tcat = np.concatenate([np.zeros(lead_t, np.uint8), txts.reshape(-1)])
        return Batch(O.pack(pcat, pbits, pbe), pbits, pbe, lead_p + np.arange(n) * M, M, O.pack(tcat, 2, tbe), tbe, lead_t + np.arange(n) * N, N)

    def device(self, dev):
        p = nvb.PackedStringSet.from_host(self.hp.words, self.hp.bits, self.hp.big_endian, self.hp.begin, None, self.M, device=dev)
        t = nvb.PackedStringSet.from_host(self.ht.words, 2, self.ht.big_endian, self.ht.begin, None, self.N, device=dev)
        return p, t


def run_gpu(b, dev, scheme, pair_switch, no_staging=0, band=BAND):
    p, t = b.device(dev)
    with nvb.test_switch("NVBIO_HIP_BANDED_PAIR", pair_switch), nvb.test_switch("NVBIO_HIP_NO_STAGING", no_staging):
        score, sink = nvb.batch_banded_alignment_score(band, nvb.make_gotoh_aligner(nvb.LOCAL, nvb.SimpleGotohScheme(*scheme)), p, t)
        torch.cuda.synchronize()
        d = detail()
    return score.cpu().numpy(), sink.cpu().numpy().view(np.uint32), d


def check(b, dev, scheme=SCHEME, expect=None, staging=(0,), band=BAND):
    """expect: the detail the default launch must report ("pair" / ""), None = either route"""
    es, ek = O.batch_banded_gotoh_score(band, O.LOCAL, scheme, b.hp, b.ht)
    for pair_switch in (0, 1):
        for no_staging in staging:
            gs, gk, d = run_gpu(b, dev, scheme, pair_switch, no_staging, band)
            bad = np.nonzero((es != gs) | (ek != gk).any(1))[0]
            assert bad.size == 0, "scheme %s M %d N %d n %d switch %d no_staging %d [%s]: %d mismatches, first %d: cpu (%d,%s) gpu (%d,%s)" % (
                scheme, b.M, b.N, b.n, pair_switch, no_staging, d, bad.size, bad[0], es[bad[0]], ek[bad[0]], gs[bad[0]], gk[bad[0]])
            if pair_switch == 1:
                assert d == "", d
            elif expect is not None:
                assert d == expect, (d, expect, scheme, b.M, b.N)
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


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 255, 256, 257, 513])
def test_lane_and_block_edges(cuda, n):
    """odd n: the last lane holds one job; 255 / 256 / 257 jobs: the last workgroup's edge"""
    rng = np.random.default_rng(41000 + n)
    pats, txts = reads_near(rng, n, 100, 150)
    es, _ = check(Batch.from_arrays(pats, txts), cuda, expect="pair", staging=(0, 1))
    assert es.max() > 100


@pytest.mark.parametrize("M", [1, 2, 15, 16, 17, 31, 32, 33, 100])
def test_block_and_row_edges(cuda, M):
    """M around the 16-row blocks; N = M + 14 is the tightest text the pair form takes, N = M + 13 lets the last row see past the end"""
    rng = np.random.default_rng(42000 + M)
    for N in (M + 14, M + 15, 150):
        pats, txts = reads_near(rng, 67, M, N)
        check(Batch.from_arrays(pats, txts), cuda, expect="pair")
    pats, txts = reads_near(rng, 67, M, M + 13)
    check(Batch.from_arrays(pats, txts), cuda, expect="")


def test_halves_are_independent(cuda):
    """512 jobs of extreme and ordinary kinds, as given, reversed and with neighbours swapped: every job has the same result whichever
    job shares its lane and whichever half it sits in (a carry or borrow across bit 16 would change a neighbour)"""
    rng = np.random.default_rng(43000)
    M, N, n = 100, 150, 512
    pats, txts = reads_near(rng, n, M, N)
    for i in range(n):
        kind = i % 5 if i < 400 else int(rng.integers(0, 5))
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
    es, ek = check(Batch.from_arrays(pats, txts), cuda, expect="pair")
    assert es.max() == 2 * M and es.min() == 0
    swap = np.arange(n) ^ 1
    for perm in (np.arange(n)[::-1], swap):
        ps, ks = check(Batch.from_arrays(pats[perm], txts[perm]), cuda, expect="pair")
        assert (ps == es[perm]).all() and (ks == ek[perm]).all()


def test_range_at_the_row_frame_limit(cuda):
    """M = lim16: a perfect match drives one half to the largest value the frame reaches while the other half stays at the row's zero,
    in both orders; one symbol more leaves the pair form"""
    lim16, _ = W.banded_limits(W.Scheme.gotoh(*SCHEME), W.LOCAL, BAND)
    rng = np.random.default_rng(44000)
    for M, expect in ((lim16, "pair"), (lim16 + 1, "")):
        N = M + BAND + 3
        txts = rng.integers(0, 3, (6, N), dtype=np.uint8)
        pats = np.full((6, M), 3, np.uint8)                                      # score 0
        for i in (0, 3, 4):                                                      # (perfect, zero), (zero, perfect), (perfect, zero)
            pats[i] = txts[i, 14:14 + M]
        es, ek = check(Batch.from_arrays(pats, txts), cuda, expect=expect)
        assert list(es) == [2 * M, 0, 0, 2 * M, 2 * M, 0]
        assert tuple(ek[0]) == (M + 14, M)


def test_sink_ties(cuda):
    """the LAST best cell wins: the later row, then the higher column.  Periodic reads against periodic texts repeat the best score along
    a row and in later rows; all-mismatch reads score 0 everywhere"""
    rng = np.random.default_rng(45000)
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
        for scheme in (SCHEME, (2, -1, -1, -1), (1, 0, -1, 0)):
            es, _ = check(Batch.from_arrays(pats, txts), cuda, scheme, expect="pair")
        assert (es == 0).any() and (es > 0).any()


@pytest.mark.parametrize("pbits,pbe,tbe", [(2, True, False), (2, False, True), (4, True, False), (4, False, True), (8, False, False), (8, True, True)])
def test_formats_and_memory(cuda, pbits, pbe, tbe):
    """2-, 4- and 8-bit patterns in both word orders (4-bit ones with codes 4-15, 8-bit ones with bytes up to 255), begins off the word
    grid, a last job that ends at the last symbol of each array, overlapping text windows; staged and unstaged"""
    rng = np.random.default_rng(46000 + pbits * 4 + pbe * 2 + tbe)
    for M, N, n in ((100, 150, 131), (37, 51, 300)):
        pats, txts = reads_near(rng, n, M, N, sym=3 if pbits == 2 else 4)
        if pbits == 2:
            pats = np.minimum(pats, 3)
        else:
            wild = rng.random(pats.shape) < 0.03
            pats[wild] = rng.integers(4, 16 if pbits == 4 else 256, int(wild.sum()))
        for lead_p, lead_t in ((0, 0), (5, 9), (13, 31)):
            check(Batch.from_arrays(pats, txts, pbits, pbe, tbe, lead_p, lead_t), cuda, expect="pair", staging=(0, 1))
        # windows of one text, a few symbols apart; the last one ends at the text's last symbol
        text = rng.integers(0, 4, 3 * (n - 1) + N + 2, dtype=np.uint8)
        tbegin = 2 + 3 * np.arange(n)
        wp = np.stack([text[b + 6:b + 6 + M] for b in tbegin])
        wp[rng.random(wp.shape) < 0.05] = 1
        b = Batch(O.pack(wp.reshape(-1), pbits, pbe), pbits, pbe, np.arange(n) * M, M, O.pack(text, 2, tbe), tbe, tbegin, N)
        check(b, cuda, expect="pair", staging=(0, 1))


@pytest.mark.parametrize("scheme,expect", [
    ((5, -1, -2, -1), "pair"),      # match - gap_open = 7: the largest byte entry, 224
    ((6, -1, -2, -1), ""),          # 8: 256 does not fit a byte
    ((2, -2, -2, -1), "pair"),      # mismatch == gap_open: the entry 0
    ((2, -3, -2, -1), ""),          # mismatch < gap_open
    ((1, 1, -2, -1), None),         # match == mismatch
    ((2, -1, -2, 0), None),         # gap_ext = 0
    ((1, 3, -2, -1), None),         # mismatch > match
    ((2, -1, -1, -1), None),        # linear gaps (what the SW entry forwards)
    ((2, -1, -7, -7), None),
    ((0, 0, 0, 0), None),
])
def test_admission_edges_over_schemes(cuda, scheme, expect):
    rng = np.random.default_rng(47000 + sum(abs(v) * 7 ** k for k, v in enumerate(scheme)))
    pats, txts = reads_near(rng, 130, 100, 150)
    pats[0] = txts[0, 3:103]; pats[1] = 4; pats[2] = 0; txts[2] = 1
    check(Batch.from_arrays(pats, txts), cuda, scheme, expect=expect)


def test_sw_entry_forwards_to_the_pair_form(cuda):
    """nvbio_hip_banded_sw_score with deletion == insertion is the plain Gotoh entry"""
    rng = np.random.default_rng(48000)
    pats, txts = reads_near(rng, 77, 100, 150)
    b = Batch.from_arrays(pats, txts)
    es, ek = O.batch_banded_gotoh_score(BAND, O.LOCAL, (2, -1, -1, -1), b.hp, b.ht)
    p, t = b.device(cuda)
    for pair_switch, want in ((0, "pair"), (1, "")):
        with nvb.test_switch("NVBIO_HIP_BANDED_PAIR", pair_switch):
            gs, gk = nvb.batch_banded_alignment_score(BAND, nvb.make_smith_waterman_aligner(nvb.LOCAL, nvb.SimpleSmithWatermanScheme(2, -1, -1, -1)), p, t)
            torch.cuda.synchronize()
            assert detail() == want
        assert (gs.cpu().numpy() == es).all() and (gk.cpu().numpy().view(np.uint32) == ek).all()


def test_other_types_and_ragged_batches_keep_their_kernels(cuda):
    rng = np.random.default_rng(49000)
    pats, txts = reads_near(rng, 40, 100, 150)
    b = Batch.from_arrays(pats, txts)
    p, t = b.device(cuda)
    for ty in (nvb.GLOBAL, nvb.SEMI_GLOBAL):
        es, ek = O.batch_banded_gotoh_score(BAND, ty, SCHEME, b.hp, b.ht)
        gs, gk = nvb.batch_banded_alignment_score(BAND, nvb.make_gotoh_aligner(ty, nvb.SimpleGotohScheme(*SCHEME)), p, t)
        torch.cuda.synchronize()
        assert detail() == ""
        assert (gs.cpu().numpy() == es).all() and (gk.cpu().numpy().view(np.uint32) == ek).all()
    rp = nvb.PackedStringSet.from_host(b.hp.words, 4, True, b.hp.begin, b.hp.length, device=cuda)
    es, ek = O.batch_banded_gotoh_score(BAND, O.LOCAL, SCHEME, b.hp, b.ht)
    gs, gk = nvb.batch_banded_alignment_score(BAND, nvb.make_gotoh_aligner(nvb.LOCAL, nvb.SimpleGotohScheme(*SCHEME)), rp, t, max_pattern_length=100)
    torch.cuda.synchronize()
    assert detail() == ""
    assert (gs.cpu().numpy() == es).all() and (gk.cpu().numpy().view(np.uint32) == ek).all()
