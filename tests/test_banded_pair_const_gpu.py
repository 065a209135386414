"""Where the column frame's cell keeps its key constants (nvbio_amd/csrc/banded_gotoh_pair.h: PF_KLIT, the K_j and 2 G as literals, one
kernel instance per |G_e|), bit-exact against the CPU oracle, score and sink.  Every case runs with NVBIO_HIP_PAIR_CONST at 0 (literals)
and at 1 (scalar registers, as it was), and nvbio_hip_last_kernel_const(), _frame(), _row() and _fetch() are asserted on every launch, so
no case is silently routed elsewhere.

Shapes, the smallest at which a misplaced constant can show: M = 1, 2, 3 (a lone row, the first pair, an odd tail), 15, 16, 17 and 33 (the
16-row seam, where the ring of zeros wraps), N = M + 14, and 1, 2, 3, 129 and 257 jobs.  Schemes: the headline's, the all-zero one,
G = 0 (K_j = j), the table's byte at its limit, and |G_e| = 2 and 3 -- with |G_e| = 0 and 1 above, each of the four literal instances
runs.  M = 234 and 235 under the headline's scheme: at 235 the row frame runs and keeps its scalars under both switch values.  4-bit
streamed patterns throughout, one 2-bit case, one 8-bit case on the generic fetches."""
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
LENGTHS = (1, 2, 3, 15, 16, 17, 33)
SCHEMES = [
    HEADLINE,
    (0, 0, 0, 0),
    (2, -1, -2, 0),       # G = 0: K_j = j
    (3, -2, -3, -1),      # the table's byte at its limit, 3 + 3 + 1 = 7
    (1, -1, -2, -2),      # |G_e| = 2
    (1, -1, -3, -3),      # |G_e| = 3, at the byte's limit, 1 + 3 + 3 = 7
]


def launch_facts():
    L = nvb.lib()
    return (L.nvbio_hip_last_kernel_detail().decode(), L.nvbio_hip_last_kernel_frame().decode(), L.nvbio_hip_last_kernel_row().decode(),
            L.nvbio_hip_last_kernel_fetch().decode(), L.nvbio_hip_last_kernel_const().decode())


def check(b, dev, scheme=HEADLINE, frame="column", fetch="stream"):
    """both placements against the oracle; frame: the frame the launch must take (only the column frame's row has the literals)"""
    es, ek = O.batch_banded_gotoh_score(BAND, O.LOCAL, scheme, b.hp, b.ht)
    for const_switch in (0, 1):
        with nvb.test_switch("NVBIO_HIP_PAIR_CONST", const_switch):
            gs, gk, _, _ = run_gpu(b, dev, scheme, 0)
            torch.cuda.synchronize()
            facts = launch_facts()
        column = frame == "column"
        want = ("pair", frame, "fold2" if column else "plain", fetch, "literal" if column and const_switch == 0 else "scalar")
        assert facts == want, (facts, want, scheme, b.M, b.N, b.n)
        bad = np.nonzero((es != gs) | (ek != gk).any(1))[0]
        assert bad.size == 0, "scheme %s M %d N %d n %d const switch %d: %d mismatches, first %d: cpu (%d,%s) gpu (%d,%s)" % (
            scheme, b.M, b.N, b.n, const_switch, bad.size, bad[0], es[bad[0]], ek[bad[0]], gs[bad[0]], gk[bad[0]])
    return es, ek


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("M", LENGTHS)
def test_schemes_and_seams(cuda, M, scheme):
    rng = np.random.default_rng(97000 + 100 * M + sum(abs(v) * 5 ** k for k, v in enumerate(scheme)))
    for n in COUNTS:
        pats, txts = reads_near(rng, n, M, M + 14)
        es, ek = check(Batch.from_arrays(pats, txts), cuda, scheme)
        if scheme == (0, 0, 0, 0):
            assert (es == 0).all() and (ek == (M + 14, M)).all()


def test_column_frame_limit(cuda):
    """M = 234, the column frame's limit under the headline scheme, where the largest key the literals build stands; M = 235 keeps the
    row frame, whose constants no switch moves"""
    rng = np.random.default_rng(98000)
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


@pytest.mark.parametrize("pbits,pbe,tbe", [(2, True, False), (8, False, True)])
def test_pattern_widths(cuda, pbits, pbe, tbe):
    """a 2-bit pattern (another streamed instance) and an 8-bit one on the generic fetches, strings beginning at every symbol offset"""
    rng = np.random.default_rng(99000 + pbits)
    for M in (17, 33):
        for scheme in (HEADLINE, (1, -1, -3, -3)):
            check(scattered(rng, 129, M, M + BAND - 1, pbits, pbe, tbe), cuda, scheme, fetch="generic" if pbits == 8 else "stream")
