"""The row loop's paths of the banded Gotoh score kernels (nvbio_amd/csrc/banded_gotoh_impl.h), against the CPU oracle bit for bit, score
and sink, through the C-ABI route of tests/test_banded_gpu.py and in both arithmetic widths: pattern lengths on either side of the
16-row block edges, waves of mixed lengths, texts that end inside the band (table rows and compare rows inside one job), staged and
unstaged lanes in one wave, jobs at the very end of the word arrays, 2-, 4- and 8-bit patterns, sink ties, and the quality kernels
(which build the substitution table per row) under reversed / complemented views."""
import numpy as np
import pytest
import torch

import nvbio_amd as nvb
from oracle import pyoracle as O

pytestmark = pytest.mark.gpu
SCHEMES = [(2, -1, -2, -1), (0, -5, -8, -3), (2, -1, -1, -1)]
LENGTHS = [1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 100]
BANDS = [3, 5, 7, 15, 31]
TYPES = [nvb.GLOBAL, nvb.LOCAL, nvb.SEMI_GLOBAL]


def run_gpu(band, ty, scheme, hp, ht, dev, force32, hint):
    p = nvb.PackedStringSet.from_host(hp.words, hp.bits, hp.big_endian, hp.begin, hp.length, device=dev)
    t = nvb.PackedStringSet.from_host(ht.words, ht.bits, ht.big_endian, ht.begin, ht.length, device=dev)
    nvb.set_test_switch("NVBIO_HIP_FORCE_32BIT", "1" if force32 else "0")
    try:
        score, sink = nvb.batch_banded_alignment_score(band, nvb.make_gotoh_aligner(ty, nvb.SimpleGotohScheme(*scheme)), p, t,
                                                       max_pattern_length=hint)
        torch.cuda.synchronize()
    finally:
        nvb.set_test_switch("NVBIO_HIP_FORCE_32BIT", "0")
    return score.cpu().numpy(), sink.cpu().numpy().view(np.uint32)


def check(band, ty, scheme, hp, ht, dev, hints):
    """hints: max_pattern_length values (0 = unknown: no staging; the longest pattern: every lane staged; less: the longer lanes read HBM)"""
    es, ek = O.batch_banded_gotoh_score(band, ty, scheme, hp, ht)
    for hint in hints:
        for force32 in (False, True):
            gs, gk = run_gpu(band, ty, scheme, hp, ht, dev, force32, hint)
            bad = np.nonzero((es != gs) | (ek != gk).any(1))[0]
            assert bad.size == 0, "band %d type %d scheme %s hint %d force32=%s: %d mismatches, first %d (M %d N %d): cpu (%d,%s) gpu (%d,%s)" % (
                band, ty, scheme, hint, force32, bad.size, bad[0], hp.length[bad[0]], ht.length[bad[0]], es[bad[0]], ek[bad[0]], gs[bad[0]], gk[bad[0]])
    return es, ek


def pair(rng, M, N, band, sym=4):
    """a text of N symbols and a pattern of M cut out of it a few columns into the band, with mutations (an N among them) and an indel"""
    t = rng.integers(0, 4, N, dtype=np.uint8)
    off = int(rng.integers(0, band))
    p = np.resize(t[off:off + M], M).copy() if N > off else rng.integers(0, 4, M, dtype=np.uint8)
    mut = rng.random(M) < 0.08
    p[mut] = rng.integers(0, sym + 1, int(mut.sum()), dtype=np.uint8)
    if M > 20 and rng.random() < 0.3:
        cut = int(rng.integers(5, M - 5))
        p = np.concatenate([p[:cut], p[cut + 2:], rng.integers(0, 4, 2, dtype=np.uint8)])
    return p, t


def edge_batch(rng, band, lengths=LENGTHS, sym=4):
    """every length with every text length M .. M + band (the text ends inside the band: the block's choice between table rows and
    compare rows flips inside a job, also in a block all of whose rows exist) and a text that covers the band; shuffled, so that a
    wave holds all the lengths"""
    pats, txts = [], []
    for M in lengths:
        for N in list(range(M, M + band + 1)) + [M + band + 20, M + 2 * band + 3]:
            p, t = pair(rng, M, N, band, sym)
            pats.append(p); txts.append(t)
    order = rng.permutation(len(pats))
    return [pats[i] for i in order], [txts[i] for i in order]


@pytest.mark.parametrize("band", BANDS)
@pytest.mark.parametrize("ty", TYPES)
def test_block_edges_and_text_ends_inside_the_band(cuda, band, ty):
    rng = np.random.default_rng(31000 + band * 3 + ty)
    pats, txts = edge_batch(rng, band)
    pats.append(pats[0][:100]); txts.append(txts[0])                       # (the last job ends where the word arrays end)
    hp, ht = O.StringSet.from_lists(pats, 4, True), O.StringSet.from_lists(txts, 2, False)
    for k, scheme in enumerate(SCHEMES):
        check(band, ty, scheme, hp, ht, cuda, [(0, 100, 40)[k]])


@pytest.mark.parametrize("band", [7, 15, 31])
@pytest.mark.parametrize("ty", TYPES)
def test_mixed_lengths_in_one_wave(cuda, band, ty):
    """64 consecutive jobs of lengths 16 / 17 / 48 / 100 in turn (then 15 / 16 / 32 / 33): a block is whole in some lanes of the wave, cut or
    absent in others.  The hint 20 stages the short lanes and leaves the long ones on HBM in the same wave."""
    rng = np.random.default_rng(32000 + band * 3 + ty)
    pats, txts = [], []
    for cyc in ((16, 17, 48, 100), (15, 16, 32, 33), (100, 1, 100, 49)):
        for i in range(128):
            M = cyc[i % 4]
            N = M + (band - 1 if i % 3 else int(rng.integers(0, band))) + (i % 5)
            p, t = pair(rng, M, N, band)
            pats.append(p); txts.append(t)
    hp, ht = O.StringSet.from_lists(pats, 4, True), O.StringSet.from_lists(txts, 2, True)
    check(band, ty, SCHEMES[0], hp, ht, cuda, [0, 100, 20])


@pytest.mark.parametrize("bits,big_endian", [(2, True), (2, False), (4, False), (8, False), (8, True)])
def test_staged_and_unstaged_lanes_and_array_ends(cuda, bits, big_endian):
    """2-, 4- and 8-bit patterns; one job of a workgroup much longer than the hint (its lane reads HBM among staged lanes); the batch's last
    jobs end exactly where the pattern and text word arrays end (their staging loads are clamped, the other lanes' are not), once with a
    long last job and once with a one-symbol one."""
    sym = 3 if bits == 2 else 4
    for band, ty in ((15, nvb.LOCAL), (31, nvb.SEMI_GLOBAL), (5, nvb.GLOBAL)):
        rng = np.random.default_rng(33000 + bits * 10 + band + int(big_endian))
        pats, txts = [], []
        for i in range(255):
            M = int(rng.integers(20, 31))
            p, t = pair(rng, M, M + band + int(rng.integers(0, 6)), band, sym)
            pats.append(p); txts.append(t)
        p, t = pair(rng, 300, 300 + band + 2, band, sym)
        pats.insert(130, p); txts.insert(130, t)
        for last in (100, 1):
            p, t = pair(rng, last, last + band - 1, band, sym)
            pp, tt = pats + [p], txts + [t]
            if bits == 2:
                pp = [np.minimum(x, 3) for x in pp]
            hp, ht = O.StringSet.from_lists(pp, bits, big_endian), O.StringSet.from_lists(tt, 2, not big_endian)
            check(band, ty, SCHEMES[0], hp, ht, cuda, [32, 300] if last == 100 else [0, 32])


@pytest.mark.parametrize("band", [15, 31])
def test_sink_ties(cuda, band):
    """LOCAL's best cell is the LAST one with the best score: the later row, then the larger column (sink_inl.h:57-68).  Periodic reads
    against periodic windows repeat the best score in later rows and in several columns of a row; all-mismatch reads score 0 everywhere."""
    rng = np.random.default_rng(34000 + band)
    pats, txts = [], []
    for M in LENGTHS + [64, 96]:
        for period in (1, 2, 3, 4, 7):
            unit = rng.integers(0, 4, period, dtype=np.uint8)
            for extra in (0, band // 2, band - 1, band + 9):
                t = np.resize(unit, M + extra)
                p = np.resize(unit, M).copy()
                if M > 8 and period > 1:
                    p[M // 2] = (p[M // 2] + 1) & 3                        # two equal runs either side of a mismatch
                pats.append(p); txts.append(t)
        for extra in (0, band - 1, band + 9):                             # nothing matches: score 0, the reference's cell
            pats.append(np.zeros(M, np.uint8)); txts.append(np.full(M + extra, 1, np.uint8))
            pats.append(np.full(M, 4, np.uint8)); txts.append(rng.integers(0, 4, M + extra, dtype=np.uint8))
    hp, ht = O.StringSet.from_lists(pats, 4, True), O.StringSet.from_lists(txts, 2, False)
    for scheme in SCHEMES:
        es, ek = check(band, nvb.LOCAL, scheme, hp, ht, cuda, [0, 100])
    assert (es == 0).any() and (es > 0).any()
    for ty in (nvb.SEMI_GLOBAL, nvb.GLOBAL):
        check(band, ty, SCHEMES[0], hp, ht, cuda, [100])


@pytest.mark.parametrize("band", [15, 31])
def test_local_at_the_longest_16_bit_length(cuda, band):
    """LOCAL (2,-1,-2,-1) runs in 16 bits up to 340 rows in the row frame and up to 511 in the reference's own frame: perfect and periodic reads
    of those lengths and their neighbours, whose best cell lies in the last rows -- the largest row numbers and scores the 16-bit fold sees."""
    rng = np.random.default_rng(35000 + band)
    pats, txts = [], []
    for L in (339, 340, 341, 510, 511, 512):
        t = rng.integers(0, 4, L + 2 * band, dtype=np.uint8)
        off = int(rng.integers(0, band))
        pats.append(t[off:off + L].copy()); txts.append(t)
        unit = rng.integers(0, 4, 3, dtype=np.uint8)
        pats.append(np.resize(unit, L)); txts.append(np.resize(unit, L + band + 5))
    hp, ht = O.StringSet.from_lists(pats, 4, True), O.StringSet.from_lists(txts, 2, False)
    es, ek = check(band, nvb.LOCAL, SCHEMES[0], hp, ht, cuda, [0, 512])
    assert es.max() == 1024 and int(ek[:, 1].max()) == 512


@pytest.mark.parametrize("band", [15, 31])
@pytest.mark.parametrize("ty", TYPES)
def test_quality_kernels_keep_the_row_table(cuda, band, ty):
    """The QualArgs kernels (per-row mismatch score: the table is built in every row) on the block-edge lengths, with reversed and / or
    complemented views of the stored reads, against the oracle on the materialised strings and qualities."""
    rng = np.random.default_rng(36000 + band * 3 + ty)
    pats, txts = edge_batch(rng, band)
    stored = O.StringSet.from_lists(pats, 4, True)
    ht = O.StringSet.from_lists(txts, 2, True)
    total = int(stored.begin[-1] + stored.length[-1])
    quals = rng.integers(0, 60, total + 3, dtype=np.uint8)
    quals[::89] = 255
    flags = rng.integers(0, 4, len(pats)).astype(np.uint8)
    mats, mquals = [], quals.copy()
    for i, pt in enumerate(pats):
        b, m = int(stored.begin[i]), len(pt)
        v, q = np.asarray(pt, np.uint8), quals[b:b + m]
        if flags[i] & 1:
            v, q = v[::-1], q[::-1]
        if flags[i] & 2:
            v = np.where(v < 4, 3 - v, v).astype(np.uint8)
        mats.append(v.copy()); mquals[b:b + m] = q
    hm = O.StringSet.from_lists(mats, 4, True)
    scheme = nvb.SmithWatermanScoringScheme.local() if ty == nvb.LOCAL else nvb.SmithWatermanScoringScheme()
    st = scheme.struct()
    lut = np.array([st.mismatch[q] for q in range(256)], dtype=np.int32)
    s6 = (st.match, st.pattern_gap_open, st.pattern_gap_ext, st.text_gap_open, st.text_gap_ext, 0)
    es, ek = O.batch_banded_gotoh_score_qual(band, ty, s6, lut, mquals, hm, ht)
    p = nvb.PackedStringSet.from_host(stored.words, 4, True, stored.begin, stored.length, device=cuda)
    t = nvb.PackedStringSet.from_host(ht.words, 2, True, ht.begin, ht.length, device=cuda)
    dq, df = torch.from_numpy(quals).to(cuda), torch.from_numpy(flags).to(cuda)
    for force32, hint in (("0", 100), ("1", 100), ("0", 0), ("0", 40)):
        nvb.set_test_switch("NVBIO_HIP_FORCE_32BIT", force32)
        try:
            gs, gk = nvb.batch_banded_alignment_score(band, nvb.make_gotoh_aligner(ty, scheme), p, t, quals=dq, pattern_flags=df, max_pattern_length=hint)
            torch.cuda.synchronize()
        finally:
            nvb.set_test_switch("NVBIO_HIP_FORCE_32BIT", "0")
        gs, gk = gs.cpu().numpy(), gk.cpu().numpy().view(np.uint32)
        bad = np.nonzero((es != gs) | (ek != gk).any(1))[0]
        assert bad.size == 0, (band, ty, force32, hint, bad[:5], flags[bad[:5]], es[bad[:3]], gs[bad[:3]])
