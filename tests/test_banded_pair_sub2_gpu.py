"""How many cells one LDS read of the pair kernel serves (nvbio_amd/csrc/banded_gotoh_pair.h, "Two cells per read"): two, a ds_read_b64
from the table of pairs (PF_SUBLDS2, the default of the literal form), one (NVBIO_HIP_PAIR_SUB = 2), or none, the v_perm_b32 lookup
(NVBIO_HIP_PAIR_SUB = 1).  Every case is bit-exact against the CPU oracle, score and sink, under all three, and the launch's facts,
nvbio_hip_last_kernel_sub() and nvbio_hip_last_kernel_subread() among them, are asserted on every launch.

Shapes: M = 1, 2, 3 (no pair formed by a row yet: every pair read comes from the prologue), 14 ... 17 and 31 ... 33 (the 16-row seams, where the
block's words are rebuilt and a pair straddles two blocks), 100; odd M for the pair fold's last row; n = 1, 2, 3, 255, 256, 257 (the
half-used last lane, the 128-lane block seam).  4-bit patterns in both byte orders and 2-bit ones, texts in both byte orders, an 8-bit
pattern on the generic fetch.  Nibbles 4 ... 15 scattered, one all-N job in each lane half.  The table's extremes: identical jobs (every
lane reads one entry), job pairs complemented in every symbol, texts whose adjacent symbols are all equal (d = 0 in every pair) and all
different (d != 0 in every pair).  The four |G_e| instances."""
import numpy as np
import pytest
import torch

import nvbio_amd as nvb
from oracle import pyoracle as O
from test_banded_pair_max3_gpu import BAND, Batch, reads_near, run_gpu
from test_banded_pair_row_gpu import scattered

pytestmark = pytest.mark.gpu
HEADLINE = (2, -1, -2, -1)
LENGTHS = (1, 2, 3, 14, 15, 16, 17, 31, 32, 33, 100)
COUNTS = (1, 2, 3, 255, 256, 257)
GE_SCHEMES = [(2, -1, -2, 0), HEADLINE, (1, -1, -2, -2), (1, -1, -3, -3)]          # |G_e| = 0, 1, 2, 3: one instance each
SWITCHES = ((0, "lds", "pair"), (2, "lds", "single"), (1, "perm", ""))             # NVBIO_HIP_PAIR_SUB, _sub(), _subread()


def check(b, dev, scheme=HEADLINE):
    es, ek = O.batch_banded_gotoh_score(BAND, O.LOCAL, scheme, b.hp, b.ht)
    for sub_switch, sub, subread in SWITCHES:
        with nvb.test_switch("NVBIO_HIP_PAIR_SUB", sub_switch):
            gs, gk, _, _ = run_gpu(b, dev, scheme, 0)
            torch.cuda.synchronize()
            L = nvb.lib()
            facts = (L.nvbio_hip_last_kernel_detail().decode(), L.nvbio_hip_last_kernel_frame().decode(), L.nvbio_hip_last_kernel_const().decode(),
                     L.nvbio_hip_last_kernel_sub().decode(), L.nvbio_hip_last_kernel_subread().decode())
        assert facts == ("pair", "column", "literal", sub, subread), (facts, sub_switch, scheme, b.M, b.N, b.n)
        bad = np.nonzero((es != gs) | (ek != gk).any(1))[0]
        assert bad.size == 0, "scheme %s M %d N %d n %d sub switch %d: %d mismatches, first %d: cpu (%d,%s) gpu (%d,%s)" % (
            scheme, b.M, b.N, b.n, sub_switch, bad.size, bad[0], es[bad[0]], ek[bad[0]], gs[bad[0]], gk[bad[0]])
    return es, ek


@pytest.mark.parametrize("M", LENGTHS)
def test_lengths_and_counts(cuda, M):
    rng = np.random.default_rng(93000 + M)
    for n in COUNTS:
        pats, txts = reads_near(rng, n, M, M + BAND - 1)
        check(Batch.from_arrays(pats, txts), cuda)


@pytest.mark.parametrize("pbits,pbe", [(4, False), (4, True), (2, False), (2, True)])
@pytest.mark.parametrize("tbe", [False, True])
def test_widths_and_byte_orders(cuda, pbits, pbe, tbe):
    """every streamed instance, strings beginning at every symbol offset of a word"""
    rng = np.random.default_rng(94000 + 4 * pbits + 2 * pbe + tbe)
    for M in (17, 33):
        check(scattered(rng, 257, M, M + BAND - 1, pbits, pbe, tbe), cuda)


def test_generic_fetch(cuda):
    """an 8-bit pattern keeps the generic fetches; its code 15 matches nothing"""
    rng = np.random.default_rng(94500)
    b = scattered(rng, 129, 33, 33 + BAND - 1, 8, False, True)
    check(b, cuda)
    assert nvb.lib().nvbio_hip_last_kernel_fetch().decode() == "generic"
    pats, txts = reads_near(rng, 5, 33, 33 + BAND - 1)
    pats[rng.random(pats.shape) < 0.2] = 15
    check(Batch.from_arrays(pats, txts, pbits=8, pbe=False), cuda)


@pytest.mark.parametrize("M", [16, 33, 100])
def test_high_nibbles(cuda, M):
    """nibbles 4 ... 15 scattered over the patterns, and one job of each lane half that is all N: none of them matches any symbol"""
    rng = np.random.default_rng(95000 + M)
    n = 131
    pats, txts = reads_near(rng, n, M, M + BAND - 1)
    hit = rng.random(pats.shape) < 0.15
    pats[hit] = rng.integers(4, 16, int(hit.sum()), dtype=np.uint8)
    pats[6] = 4                                                                  # job A of lane 3
    pats[9] = 4                                                                  # job B of lane 4
    pats[10] = pats[11] = 15
    es, ek = check(Batch.from_arrays(pats, txts), cuda)
    assert es[6] == 0 and es[9] == 0 and es[10] == 0 and es[11] == 0
    assert es.max() > 0


@pytest.mark.parametrize("M", [17, 100])
def test_identical_jobs(cuda, M):
    """256 identical jobs: every lane reads one entry of the table in every read"""
    rng = np.random.default_rng(96000 + M)
    pats, txts = reads_near(rng, 1, M, M + BAND - 1)
    check(Batch.from_arrays(np.repeat(pats, 256, 0), np.repeat(txts, 256, 0)), cuda)


@pytest.mark.parametrize("M", [17, 100])
def test_pairs_complemented(cuda, M):
    """job B's symbols are job A's complemented, pattern and text alike, and then its pattern is all N where A's matches"""
    rng = np.random.default_rng(97000 + M)
    n = 129
    pats, txts = reads_near(rng, 2 * n, M, M + BAND - 1, sym=3)
    pats[1::2] = 3 - pats[0::2]
    txts[1::2] = 3 - txts[0::2]
    check(Batch.from_arrays(pats, txts), cuda)
    pats[1::2] = 4
    es, _ = check(Batch.from_arrays(pats, txts), cuda)
    assert (es[1::2] == 0).all() and es[0::2].max() > 0


@pytest.mark.parametrize("M", [17, 100])
@pytest.mark.parametrize("differ", [False, True])
def test_adjacent_text_symbols(cuda, M, differ):
    """texts whose adjacent symbols are all equal (every pair's d is 0: both words of an entry are one cell's) or all different (no
    pair's d is 0); the reads are cut from them and mutated"""
    rng = np.random.default_rng(98000 + 2 * M + differ)
    n, N = 131, M + BAND - 1
    steps = rng.integers(1, 4, (n, N), dtype=np.uint8) if differ else np.zeros((n, N), np.uint8)
    steps[:, 0] = rng.integers(0, 4, n, dtype=np.uint8)
    txts = (np.cumsum(steps, 1) & 3).astype(np.uint8)
    d = txts[:, 1:] ^ txts[:, :-1]
    assert (d != 0).all() if differ else (d == 0).all()
    pats = np.empty((n, M), np.uint8)
    for i in range(n):
        off = int(rng.integers(0, BAND))
        p = txts[i, off:off + M].copy()
        mut = rng.random(M) < 0.1
        p[mut] = rng.integers(0, 5, int(mut.sum()), dtype=np.uint8)
        pats[i] = p
    es, _ = check(Batch.from_arrays(pats, txts), cuda)
    assert es.max() > 0


@pytest.mark.parametrize("scheme", GE_SCHEMES)
def test_ge_instances(cuda, scheme):
    rng = np.random.default_rng(99000 - scheme[3])
    for M, n in ((3, 3), (17, 257), (33, 129)):
        pats, txts = reads_near(rng, n, M, M + BAND - 1)
        check(Batch.from_arrays(pats, txts), cuda, scheme)
