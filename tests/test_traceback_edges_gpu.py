"""The tracebacks at the edges of the scorers' contract: linear gap costs with deletion != insertion
(sw_banded_inl.h:405-470, sw_inl.h:475-500) and 8-bit pattern strings, banded and full matrix, through every layer that reaches them.
Each case compares score, sink, source, cigar_len and the CIGAR words with the oracle's restatement on every job, and names the
traceback kernel that ran."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import nvbio_amd as nvb
from oracle import pyoracle as O
from test_traceback_gpu import compare, to_dev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu
TYPES = [nvb.GLOBAL, nvb.LOCAL, nvb.SEMI_GLOBAL]
BANDS = [3, 5, 7, 15, 31]
ASYM = [(2, -1, -2, -3), (1, -1, -3, -1), (0, -1, -1, -2)]
EDGE_LENGTHS = (1, 15, 16, 17, 32, 33)          # around the kernels' 16-row fetch groups
ODD_BYTES = np.array([4, 7, 15, 200, 255], np.uint8)
FULL_STRIDE = 192                               # ... and of the full-matrix jobs (GLOBAL walks the whole text)
STRIDE = 48                                     # holds every CIGAR of the banded jobs (asserted): all their words are compared


def last_kernel():
    return nvb.lib().nvbio_hip_last_kernel().decode()


def padded_texts(txts, big_endian):
    """a 2-bit text set with defined symbols after its last string (the band's first window is read unchecked)"""
    ht = O.StringSet.from_lists(txts + [np.zeros(64, np.uint8)], 2, big_endian)
    return O.StringSet(ht.words, 2, big_endian, ht.begin[:-1], ht.length[:-1])


def swapped(scheme):
    return (scheme[0], scheme[1], scheme[3], scheme[2])


def cigars_differ(a, b):
    return bool((a["cigar_len"] != b["cigar_len"]).any() or (a["cigar"] != b["cigar"]).any())


# ------------------------------------------------------------------------------------------------ banded
def banded_jobs(rng, n, band):
    """Ragged jobs for a band: pattern lengths 1..70 (EDGE_LENGTHS among them), texts of about M + band - 1 symbols -- some a few
    short, so that the past-the-end symbol enters the band, one in five shorter than the pattern (no sink) --, patterns cut from their
    text with substitutions, an N now and then, and in a third of them a 2-symbol deletion (gapped walks)."""
    pats, txts = [], []
    for i in range(n):
        M = EDGE_LENGTHS[(i // 5) % len(EDGE_LENGTHS)] if i % 5 == 0 and i < 60 else int(rng.integers(1, 71))
        if i % 5 == 4:
            N = max(0, M - int(rng.integers(1, 4)))
        else:
            N = max(M, M + band - 1 + int(rng.integers(-4, 5)))
        t = rng.integers(0, 4, N, dtype=np.uint8)
        gap = 2 if i % 3 == 0 and M > 6 else 0
        off = int(rng.integers(0, band // 2 + 1))
        p = t[off:off + M + gap].copy()
        if p.size < M + gap:
            p = np.concatenate([p, rng.integers(0, 4, M + gap - p.size, dtype=np.uint8)])
        if gap:
            cut = int(rng.integers(2, M - 2))
            p = np.concatenate([p[:cut], p[cut + 2:]])
        mut = rng.random(M) < 0.06
        p[mut] = rng.integers(0, 5, int(mut.sum()), dtype=np.uint8)
        pats.append(p.astype(np.uint8)); txts.append(t)
    lens = {len(p) for p in pats}
    assert all(m in lens for m in EDGE_LENGTHS)
    return pats, txts


@functools.lru_cache(maxsize=None)
def banded_case(band, ty):
    """the jobs of one (band, type) and the oracle's tracebacks of the asymmetric schemes over them -- computed once, shared"""
    rng = np.random.default_rng(9900 + band * 3 + ty)
    pats, txts = banded_jobs(rng, 600, band)
    hp, ht = O.StringSet.from_lists(pats, 4, True), padded_texts(txts, True)
    exp = {s: O.batch_sw_traceback(band, ty, s, hp, ht, STRIDE) for s in ASYM}
    return pats, txts, exp


@gpu
@pytest.mark.parametrize("band", BANDS)
@pytest.mark.parametrize("ty", TYPES)
def test_banded_sw_traceback_with_direction_dependent_gaps(cuda, band, ty):
    """sw_banded_inl.h:405-470: top + deletion, left + insertion, GLOBAL's row zero j * deletion; 4-bit patterns, 2-bit texts of both
    byte orders."""
    pats, txts, exp = banded_case(band, ty)
    gapped = no_sink = 0
    for pbe, tbe in ((True, True), (False, False)):
        hp, ht = O.StringSet.from_lists(pats, 4, pbe), padded_texts(txts, tbe)
        dp, dt = to_dev(hp, cuda), to_dev(ht, cuda)
        for scheme in ASYM:
            al = nvb.make_smith_waterman_aligner(ty, nvb.SimpleSmithWatermanScheme(*scheme))
            got = nvb.batch_banded_alignment_traceback(band, al, dp, dt, max_pattern_length=int(hp.length.max()), cigar_stride=STRIDE)
            torch.cuda.synchronize()
            assert "traceback" in last_kernel()
            compare(exp[scheme], got, (band, ty, scheme, pbe))
    for scheme in ASYM:
        # the oracle's traceback agrees with the oracle's score pass (the yardstick holds together) ...
        es, ek = O.batch_sw_score(band, ty, scheme, O.StringSet.from_lists(pats, 4, True), padded_texts(txts, True))
        assert (es == exp[scheme]["score"]).all() and (ek == exp[scheme]["sink"]).all()
        gapped += int((((exp[scheme]["cigar"] & 3) % 3 != 0) & (np.arange(STRIDE)[None, :] < exp[scheme]["cigar_len"][:, None])).any(1).sum())
        no_sink += int((exp[scheme]["source"][:, 0] == 0xFFFFFFFF).sum())
    assert gapped > 30 and no_sink > 200
    assert max(int(exp[s]["cigar_len"].max()) for s in ASYM) <= STRIDE
    # ... and the two directions really differ on this data: swapping the costs changes some job's CIGAR, for every scheme.  (Not LOCAL
    # with match 0: no cell is worth more than 0, every H is 0, so top = deletion and left = insertion never beat the diagonal's 0 or
    # mismatch = -1 under the strict tests -- both costs are <= -1 -- and every walk is one run of M whatever the gaps cost.)
    hp, ht = O.StringSet.from_lists(pats, 4, True), padded_texts(txts, True)
    for scheme in ASYM:
        if not (ty == nvb.LOCAL and scheme[0] == 0):
            assert cigars_differ(exp[scheme], O.batch_sw_traceback(band, ty, swapped(scheme), hp, ht, STRIDE)), scheme


def byte_patterns(rng, pats):
    """the same patterns as bytes: about 5 % of them values no 2-bit text symbol equals, 255 -- what the reference compares a text
    position past the end as -- among them, and at the end of every ninth pattern (where a short text lets the two meet)"""
    out = []
    for i, p in enumerate(pats):
        b = p.astype(np.uint8).copy()
        odd = rng.random(b.size) < 0.05
        b[odd] = rng.choice(ODD_BYTES, int(odd.sum()))
        if i % 9 == 0:
            b[-1] = 255
        out.append(b)
    return out


@gpu
@pytest.mark.parametrize("band", BANDS)
@pytest.mark.parametrize("ty", TYPES)
def test_banded_tracebacks_with_8bit_patterns(cuda, band, ty):
    """every banded entry on byte patterns (begins at every byte offset mod 4): Gotoh, the quality scheme (quality bytes stay at the
    patterns' offsets) with and without known sinks, SW, ED, and SW with direction-dependent gaps"""
    rng = np.random.default_rng(9950 + band * 3 + ty)
    pats, txts = banded_jobs(rng, 600, band)
    bp = byte_patterns(rng, pats)
    begins = np.cumsum([0] + [len(p) for p in bp[:-1]])
    assert {int(b) & 3 for b in begins} == {0, 1, 2, 3}
    assert any((b == 255).any() for b in bp)
    total = int(sum(len(p) for p in bp))
    quals = rng.integers(0, 60, total + 3, dtype=np.uint8)
    quals[::97] = 255
    dq = torch.from_numpy(quals).to(cuda)
    qs = nvb.SmithWatermanScoringScheme.local()
    st = qs.struct()
    lut = np.array([st.mismatch[q] for q in range(256)], dtype=np.int32)
    s5 = (st.match, st.pattern_gap_open, st.pattern_gap_ext, st.text_gap_open, st.text_gap_ext)
    ht = padded_texts(txts, True)
    h8 = O.StringSet.from_lists(bp, 8, False)
    maxM = int(h8.length.max())
    cases = [("gotoh", (2, -1, -2, -1)), ("gotoh", (2, -6, -8, -3)), ("qual", s5), ("sw", (2, -1, -1, -1)), ("ed", (0, -1, -1, -1)), ("sw", (2, -1, -2, -3))]
    exp = []
    for kind, scheme in cases:
        if kind == "gotoh":
            exp.append(O.batch_banded_gotoh_traceback(band, ty, scheme, h8, ht, STRIDE))
        elif kind == "qual":
            exp.append(O.batch_banded_gotoh_traceback(band, ty, scheme, h8, ht, STRIDE, lut, quals))
        else:
            exp.append(O.batch_sw_traceback(band, ty, scheme, h8, ht, STRIDE))
    for be in (False, True):
        hp = O.StringSet.from_lists(bp, 8, be)
        dp, dt = to_dev(hp, cuda), to_dev(ht, cuda)
        for (kind, scheme), e in zip(cases, exp):
            kw = {}
            if kind == "gotoh":
                al = nvb.make_gotoh_aligner(ty, nvb.SimpleGotohScheme(*scheme))
            elif kind == "qual":
                al, kw = nvb.make_gotoh_aligner(ty, qs), dict(quals=dq)
            elif kind == "ed":
                al = nvb.make_edit_distance_aligner(ty)
            else:
                al = nvb.make_smith_waterman_aligner(ty, nvb.SimpleSmithWatermanScheme(*scheme))
            got = nvb.batch_banded_alignment_traceback(band, al, dp, dt, max_pattern_length=maxM, cigar_stride=STRIDE, **kw)
            torch.cuda.synchronize()
            assert "traceback" in last_kernel()
            compare(e, got, (band, ty, kind, scheme, be))
            if kind == "qual":
                known = (torch.from_numpy(e["score"].copy()).to(cuda), torch.from_numpy(e["sink"].view(np.int32).copy()).to(cuda))
                got = nvb.batch_banded_alignment_traceback(band, al, dp, dt, max_pattern_length=maxM, cigar_stride=STRIDE, known=known, **kw)
                torch.cuda.synchronize()
                assert "traceback" in last_kernel()
                compare(e, got, (band, ty, "known sinks", be))
    # the bytes matter on this data (the oracle alone): cut to two bits some jobs score differently; and so does byte 255 where the
    # alignment has to end on the band's last diagonal (GLOBAL), which a text a few symbols short puts past its end
    h2 = O.StringSet.from_lists([b & 3 for b in bp], 4, True)
    assert (exp[0]["score"] != O.batch_banded_gotoh_traceback(band, ty, cases[0][1], h2, ht, STRIDE)["score"]).any()
    if ty == nvb.GLOBAL:
        h254 = O.StringSet.from_lists([np.where(b == 255, 254, b).astype(np.uint8) for b in bp], 8, False)
        assert (exp[0]["score"] != O.batch_banded_gotoh_traceback(band, ty, cases[0][1], h254, ht, STRIDE)["score"]).any()


# ------------------------------------------------------------------------------------------------ full matrix
def full_jobs(rng, n, near):
    """M 1..120 (never 0: the oracle's full-matrix pass reads uninitialised cells for an empty pattern), N 1..260, or within +-8 of M"""
    pats, txts = [], []
    for i in range(n):
        M = int(rng.integers(1, 121))
        N = max(1, M + int(rng.integers(-8, 9))) if near else int(rng.integers(1, 261))
        t = rng.integers(0, 4, N).astype(np.uint8)
        p = np.resize(t[int(rng.integers(0, N)):], M).copy()
        mut = rng.random(M) < 0.08
        p[mut] = rng.integers(0, 4, int(mut.sum()))
        if M > 12 and i % 3 == 0:
            cut = int(rng.integers(3, M - 5))
            p = np.concatenate([p[:cut], p[cut + 2:], rng.integers(0, 4, 2).astype(np.uint8)])
        pats.append(p.astype(np.uint8)); txts.append(t)
    return pats, txts


@functools.lru_cache(maxsize=None)
def full_case(ty, near):
    rng = np.random.default_rng(9970 + ty * 2 + int(near))
    pats, txts = full_jobs(rng, 400, near)
    hp, ht = O.StringSet.from_lists(pats, 4, True), O.StringSet.from_lists(txts, 2, False)
    exp = {s: O.batch_sw_traceback(0, ty, s, hp, ht, FULL_STRIDE) for s in ASYM}
    return pats, txts, hp, ht, exp


@gpu
@pytest.mark.parametrize("lanes", [0, 1])
@pytest.mark.parametrize("near", [False, True])
@pytest.mark.parametrize("ty", TYPES)
def test_full_sw_traceback_with_direction_dependent_gaps(cuda, ty, near, lanes):
    """sw_inl.h:475-500: `deletion` along the text, `insertion` down the pattern -- the other way round than in the band; both
    executions of the kernel (one job per wave segment / per lane)"""
    pats, txts, hp, ht, exp = full_case(ty, near)
    dp, dt = to_dev(hp, cuda), to_dev(ht, cuda)
    maxM, maxN = int(hp.length.max()), int(ht.length.max())
    nvb.set_test_switch("NVBIO_HIP_TRACEBACK_LANES", lanes)
    for scheme in ASYM:
        al = nvb.make_smith_waterman_aligner(ty, nvb.SimpleSmithWatermanScheme(*scheme))
        got = nvb.batch_alignment_traceback(al, dp, dt, maxM, maxN, cigar_stride=FULL_STRIDE)
        torch.cuda.synchronize()
        assert last_kernel() == ("full_gotoh_traceback_kernel" if lanes else "full_gotoh_traceback_wave_kernel")
        compare(exp[scheme], got, (ty, near, lanes, scheme))
        assert int(exp[scheme]["cigar_len"].max()) <= FULL_STRIDE
        # the oracle's traceback and its pattern-blocking score pass agree
        es, ek, _ = O.batch_score_pattern_blocking(1, ty, scheme, hp, ht)
        assert (es == exp[scheme]["score"]).all() and (ek == exp[scheme]["sink"]).all()
    for scheme in ASYM:
        other = O.batch_sw_traceback(0, ty, swapped(scheme), hp, ht, FULL_STRIDE)
        if ty == nvb.GLOBAL:
            # both ends are pinned, #I - #D = M - N: the swap shifts a job's score by (N - M) * (deletion - insertion) and leaves the walk alone
            ragged = hp.length != ht.length
            assert ragged.any() and (exp[scheme]["score"][ragged] != other["score"][ragged]).all(), scheme
        elif not (ty == nvb.LOCAL and scheme[0] == 0):          # (LOCAL with match 0: every H is 0 and every cell SINK, see the banded case)
            assert cigars_differ(exp[scheme], other), scheme


@gpu
@pytest.mark.parametrize("lanes", [0, 1])
@pytest.mark.parametrize("ty", TYPES)
def test_full_tracebacks_with_8bit_patterns(cuda, ty, lanes):
    """every full-matrix entry on byte patterns: Gotoh and the quality scheme (8-symbol blocks, the ungapped fast path included),
    their _known_score forms, SW with direction-dependent gaps and ED (16-symbol blocks)"""
    rng = np.random.default_rng(9990 + ty)
    pats, txts = full_jobs(rng, 400, False)
    bp = byte_patterns(rng, pats)
    hp, ht = O.StringSet.from_lists(bp, 8, bool(lanes)), padded_texts(txts, True)
    dp, dt = to_dev(hp, cuda), to_dev(ht, cuda)
    maxM, maxN = int(hp.length.max()), int(ht.length.max())
    quals = rng.integers(0, 60, int(hp.begin[-1] + hp.length[-1]) + 3, dtype=np.uint8)
    dq = torch.from_numpy(quals).to(cuda)
    qs = nvb.SmithWatermanScoringScheme.local()
    st = qs.struct()
    lut = np.array([st.mismatch[q] for q in range(256)], dtype=np.int32)
    s5 = (st.match, st.pattern_gap_open, st.pattern_gap_ext, st.text_gap_open, st.text_gap_ext)
    nvb.set_test_switch("NVBIO_HIP_TRACEBACK_LANES", lanes)
    name = "full_gotoh_traceback_kernel" if lanes else "full_gotoh_traceback_wave_kernel"
    for kind, scheme in (("gotoh", (2, -6, -8, -3)), ("qual", s5), ("sw", (2, -1, -2, -3)), ("ed", (0, -1, -1, -1))):
        kw, okw = {}, {}
        if kind == "gotoh":
            al = nvb.make_gotoh_aligner(ty, nvb.SimpleGotohScheme(*scheme), nvb.PATTERN_BLOCKING)
        elif kind == "qual":
            al, kw, okw = nvb.make_gotoh_aligner(ty, qs), dict(quals=dq), dict(mm_lut=lut, quals=quals)
        elif kind == "ed":
            al = nvb.make_edit_distance_aligner(ty)
        else:
            al = nvb.make_smith_waterman_aligner(ty, nvb.SimpleSmithWatermanScheme(*scheme))
        linear = kind in ("sw", "ed")
        exp = O.batch_sw_traceback(0, ty, scheme, hp, ht, FULL_STRIDE) if linear else O.batch_gotoh_traceback(ty, scheme, hp, ht, FULL_STRIDE, **okw)
        got = nvb.batch_alignment_traceback(al, dp, dt, maxM, maxN, cigar_stride=FULL_STRIDE, **kw)
        torch.cuda.synchronize()
        assert last_kernel() == name
        compare(exp, got, (ty, lanes, kind))
        if linear or ty == nvb.GLOBAL:
            continue
        # the _known_score forms over windows that end at the scoring pass's sinks (the premise of those entries)
        keep = np.nonzero(exp["sink"][:, 0].view(np.int32) > 0)[0]
        wl = exp["sink"][keep, 0].astype(np.uint32)
        sub_p = O.StringSet(hp.words, 8, hp.big_endian, hp.begin[keep], hp.length[keep])
        sub_t = O.StringSet(ht.words, 2, True, ht.begin[keep], wl)
        exp_w = O.batch_gotoh_traceback(ty, scheme, sub_p, sub_t, FULL_STRIDE, **okw)
        assert (exp_w["score"] == exp["score"][keep]).all() and (exp_w["sink"][:, 0] == wl).all()
        known = torch.from_numpy(exp["score"][keep].astype(np.int32)).to(cuda)
        got = nvb.batch_alignment_traceback(al, to_dev(sub_p, cuda), to_dev(sub_t, cuda), maxM, maxN, cigar_stride=FULL_STRIDE, known_score=known, **kw)
        torch.cuda.synchronize()
        assert "traceback" in last_kernel()
        compare(exp_w, got, (ty, lanes, kind, "known score"))


# ------------------------------------------------------------------------------------------------ relation to what exists
@gpu
@pytest.mark.parametrize("ty", TYPES)
def test_8bit_packing_of_a_2bit_alphabet_equals_its_4bit_packing(cuda, ty):
    """patterns over 0..3: the same jobs as 4-bit and as 8-bit strings give the same outputs, banded and full matrix"""
    rng = np.random.default_rng(9995 + ty)
    pats, txts = banded_jobs(rng, 300, 15)
    pats = [np.minimum(p, 3) for p in pats]
    ht = padded_texts(txts, True)
    dt = to_dev(ht, cuda)
    h4, h8 = O.StringSet.from_lists(pats, 4, True), O.StringSet.from_lists(pats, 8, False)
    maxM, maxN = int(h4.length.max()), max(1, int(ht.length.max()))
    outs = []
    for hp in (h4, h8):
        dp = to_dev(hp, cuda)
        o = []
        for band in (15, 31):
            o.append(nvb.batch_banded_alignment_traceback(band, nvb.make_gotoh_aligner(ty, nvb.SimpleGotohScheme(2, -1, -2, -1)), dp, dt,
                                                          max_pattern_length=maxM, cigar_stride=STRIDE))
            o.append(nvb.batch_banded_alignment_traceback(band, nvb.make_smith_waterman_aligner(ty, nvb.SimpleSmithWatermanScheme(2, -1, -1, -1)), dp, dt,
                                                          max_pattern_length=maxM, cigar_stride=STRIDE))
        o.append(nvb.batch_alignment_traceback(nvb.make_gotoh_aligner(ty, nvb.SimpleGotohScheme(2, -6, -8, -3), nvb.PATTERN_BLOCKING), dp, dt, maxM, maxN, cigar_stride=48))
        o.append(nvb.batch_alignment_traceback(nvb.make_edit_distance_aligner(ty), dp, dt, maxM, maxN, cigar_stride=48))
        torch.cuda.synchronize()
        assert "traceback" in last_kernel()
        outs.append(o)
    for a, b in zip(*outs):
        for k in ("score", "sink", "source", "cigar_len", "cigar"):
            assert torch.equal(a[k], b[k]), k
    compare(O.batch_banded_gotoh_traceback(15, ty, (2, -1, -2, -1), h4, ht, STRIDE), outs[1][0], (ty, "8-bit vs oracle"))


# ------------------------------------------------------------------------------------------------ drop-in layer
@gpu
@pytest.mark.parametrize("typ", TYPES)
@pytest.mark.parametrize("band", [15, 31, 0])
def test_drop_in_traceback_stream_with_asymmetric_gaps_stays_tuned(cuda, typ, band):
    """a packed-text traceback stream with SimpleSmithWatermanScheme(2,-1,-2,-3) through the drop-in layer's
    Batched(Banded)AlignmentTraceback (tests/compat/aln_callers.hip, compat_traceback): the library's traceback kernel runs it"""
    from test_compat_alignment_gpu import Batch, dev, make_jobs
    path = os.path.join(ROOT, "tests", "compat", "libaln_callers.so")
    assert os.path.exists(path), "build with python -c 'import __graft_entry__ as g; g.build()'"
    L = C.CDLL(path)
    L.compat_traceback.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    reads, quals, wins = make_jobs(4300 + 10 * typ + band, 600, max_read=120, band=band or 31, max_sym=3, full=(band == 0))
    b = Batch(reads, quals, wins, packed=True, on_device=True)
    stride, scheme = 200, (2, -1, -2, -3)
    sc = np.array(scheme, dtype=np.int32)
    # a score call first, so that the last kernel's name is not a traceback's from an earlier test
    nvb.batch_banded_alignment_score(15, nvb.make_gotoh_aligner(typ, nvb.SimpleGotohScheme(2, -1, -2, -1)),
                                     to_dev(O.StringSet.from_lists([np.zeros(4, np.uint8)], 4, True), cuda), to_dev(padded_texts([np.zeros(20, np.uint8)], True), cuda), max_pattern_length=4)
    assert "traceback" not in last_kernel()
    score = dev(np.full(b.n, 12345, np.int32)); sink = dev(np.full((b.n, 2), 777, np.int32)); source = dev(np.full((b.n, 2), 777, np.int32))
    cigar = dev(np.zeros((b.n, stride), np.int16)); clen = dev(np.full(b.n, 999, np.int32))
    rc = L.compat_traceback(1, typ, band, sc.ctypes.data, b.n, b.ptr("ro"), b.ptr("r"), b.longest_read, b.ptr("wo"), b.ptr("w"), b.longest_win,
                            C.c_void_p(score.data_ptr()), C.c_void_p(sink.data_ptr()), C.c_void_p(source.data_ptr()), C.c_void_p(cigar.data_ptr()), stride,
                            C.c_void_p(clen.data_ptr()))
    assert rc == 0
    torch.cuda.synchronize()
    assert "traceback" in last_kernel()
    exp = O.batch_sw_traceback(band, typ, scheme, b.hr, b.hw, stride)
    gs, gk, gsrc = score.cpu().numpy(), sink.cpu().numpy().view(np.uint32), source.cpu().numpy().view(np.uint32)
    gc, gl = cigar.cpu().numpy().view(np.uint16), clen.cpu().numpy().view(np.uint32)
    declined = (np.arange(b.n) % 53) == 52
    live = ~declined & ((np.diff(b.ro) > 0) | (band != 0))
    assert (gs[declined] == -77).all() and (gk[declined] == 7).all() and (gl[declined] == 0).all()
    assert (gs[live] == exp["score"][live]).all(), (typ, band)
    assert (gk[live] == exp["sink"][live]).all() and (gsrc[live] == exp["source"][live]).all(), (typ, band)
    assert (gl[live] == exp["cigar_len"][live]).all(), (typ, band)
    mask = (np.arange(stride)[None, :] < exp["cigar_len"][:, None]) & live[:, None]
    assert ((gc == exp["cigar"]) | ~mask).all(), (typ, band)
    assert int(exp["cigar_len"][live].max()) < stride


# ------------------------------------------------------------------------------------------------ C++ host layer
def test_cxx_traceback_classes_compile_for_the_linear_gap_aligners():
    """BatchedBandedAlignmentTraceback / BatchedAlignmentTraceback over SmithWatermanAligner and EditDistanceAligner streams
    (tests/cxx/traceback_edges_test.cpp): a CPU test -- the overloads have to exist"""
    import __graft_entry__ as g
    assert os.path.exists(g.build_traceback_edges_test())


def fnv1a_words(exp, stride):
    """the checksum of tests/cxx/traceback_edges_test.cpp over the oracle's outputs"""
    h = 14695981039346656037
    for i in range(exp["score"].size):
        words = [int(exp["score"][i]) & 0xFFFFFFFF, *map(int, exp["sink"][i]), *map(int, exp["source"][i]), int(exp["cigar_len"][i])]
        words += [int(w) for w in exp["cigar"][i, :min(int(exp["cigar_len"][i]), stride)]]
        for w in words:
            h = ((h ^ w) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


@gpu
@pytest.mark.parametrize("ty", TYPES)
def test_cxx_traceback_classes_with_the_linear_gap_aligners(cuda, ty):
    """a 200-job batch through both classes of include/nvbio_hip/alignment.h, SW (2,-1,-2,-3) and ED: the checksum of their outputs
    equals the checksum of the oracle's"""
    path = os.path.join(ROOT, "tests", "cxx", "libtraceback_edges_test.so")
    assert os.path.exists(path), "build with python -c 'import __graft_entry__ as g; g.build()'"
    L = C.CDLL(path)
    L.nvbio_traceback_edges_check.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_uint32, C.c_void_p, C.c_void_p]
    rng = np.random.default_rng(9999 + ty)
    pats, txts = banded_jobs(rng, 200, 15)
    txts = [t if len(t) else np.zeros(1, np.uint8) for t in txts]
    hp, ht = O.StringSet.from_lists(pats, 4, True), O.StringSet.from_lists(txts, 2, True)
    cat_p, cat_t = np.concatenate(pats), np.concatenate(txts)
    stride = 48
    for kind, scheme in ((0, (2, -1, -2, -3)), (1, (0, -1, -1, -1))):
        expect = np.array([fnv1a_words(O.batch_sw_traceback(15, ty, scheme, hp, ht, stride), stride),
                           fnv1a_words(O.batch_sw_traceback(0, ty, scheme, hp, ht, stride), stride)], dtype=np.uint64)
        sums = np.zeros(2, dtype=np.uint64)
        sc = np.array(scheme, dtype=np.int32)
        rc = L.nvbio_traceback_edges_check(kind, ty, sc.ctypes.data, len(pats), cat_p.ctypes.data, hp.begin.ctypes.data, hp.length.ctypes.data,
                                           cat_t.ctypes.data, ht.begin.ctypes.data, ht.length.ctypes.data, stride, expect.ctypes.data, sums.ctypes.data)
        assert rc == 0 and (sums == expect).all(), (ty, kind, rc, sums, expect)
        assert "traceback" in last_kernel()
