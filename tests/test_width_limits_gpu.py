"""The DP kernels at their 16-bit admission limits, over the scheme corpus of tests/width_limits.py.

Every case drives jobs to the values the host's width proofs bound (a perfect match or an all-best-pair read scores M x best_pair, the
all-mismatch read and the widest gaps the band allows go the other way), at the last length a rule admits and one symbol past it, and
compares score and sink (and CIGAR, for tracebacks) with the oracle once on the 16-bit kernels and once with NVBIO_HIP_FORCE_32BIT=1.
Fixed-length batches pin the mirror to the library: nvbio_hip_last_kernel() names the width or route the mirror predicts."""
import contextlib

import numpy as np
import pytest
import torch

import nvbio_amd as nvb
import width_limits as W
from nvbio_amd._lib import GotohQualSchemeStruct
from nvbio_amd.alignment import batch_banded_alignment_score_wave
from oracle import pyoracle as O

pytestmark = pytest.mark.gpu
INT32_MIN = np.iinfo(np.int32).min
NO_ALN = -(1 << 30)
BY_NAME = {s.name: s for s in W.CORPUS}


@contextlib.contextmanager
def switches(**kv):
    """several nvb.test_switch at once: each switch is restored to its earlier value on exit"""
    with contextlib.ExitStack() as stack:
        for k, v in kv.items():
            stack.enter_context(nvb.test_switch(k, v))
        yield


class LutScheme(nvb.SmithWatermanScoringScheme):
    """The quality scheme with an arbitrary mismatch LUT (a corpus W.Scheme of kind "qual")."""

    def __init__(self, s):
        super().__init__()
        self.s = s

    def struct(self):
        st = GotohQualSchemeStruct()
        st.match, st.pattern_gap_open, st.pattern_gap_ext, st.text_gap_open, st.text_gap_ext = self.s.match, self.s.go, self.s.ge, self.s.tgo, self.s.tge
        for q in range(256):
            st.mismatch[q] = self.s.lut[q]
        return st


def aligner(s, ty, algorithm=nvb.TEXT_BLOCKING):
    if s.kind == "gotoh":
        return nvb.make_gotoh_aligner(ty, nvb.SimpleGotohScheme(s.match, s.mismatch, s.go, s.ge), algorithm)
    if s.kind == "sw":
        return nvb.make_smith_waterman_aligner(ty, nvb.SimpleSmithWatermanScheme(s.match, s.mismatch, s.go, s.ge), algorithm)
    return nvb.make_gotoh_aligner(ty, LutScheme(s), algorithm)


def last_kernel():
    return nvb.lib().nvbio_hip_last_kernel().decode()


def best_pair_of(s):
    return W.banded_inputs(s)[1]


# ---------------------------------------------------------------------------------------------------------------------------------
# probe jobs
# ---------------------------------------------------------------------------------------------------------------------------------
class Probes:
    """Jobs of the given pattern lengths for one band: per length a perfect match, the best-pair read (all-mismatch at the LUT's best
    quality when a mismatch or LUT entry beats match), an all-mismatch read at the worst quality, a read of N symbols, band - 1 text
    symbols inserted / deleted at the start, middle and end, and a window cut by the text's end.  `best` marks the best-pair jobs."""

    def __init__(self, s, band, lengths, seed):
        rng = np.random.default_rng(seed)
        lut = s.lut_array()
        bp = best_pair_of(s)
        q_best, q_worst = int(np.argmax(lut)), int(np.argmin(lut))
        best_by_mismatch = bp > s.match
        pats, txts, quals, best = [], [], [], []
        g = band - 1

        def add(p, t, q, is_best=False):
            pats.append(np.asarray(p, np.uint8)); txts.append(np.asarray(t, np.uint8))
            quals.append(np.full(len(p), q, np.uint8) if np.isscalar(q) else np.asarray(q, np.uint8)); best.append(is_best)

        for L in lengths:
            t = rng.integers(0, 4, L + 2 * band + 2, dtype=np.uint8)
            off = int(rng.integers(0, band))
            src = t[off:off + L]
            add(src, t, q_best, not best_by_mismatch)                                  # perfect match
            add(3 - src, t, q_best, best_by_mismatch)                                  # every pair a mismatch at the best quality
            add(3 - src, t, q_worst)                                                   # ... at the worst quality
            add(np.full(L, 4, np.uint8), t, rng.integers(0, 256, L))                   # N symbols
            if L > g + 2:
                for cut in (0, L // 2, L - 1):
                    ins = np.concatenate([t[:cut], t[cut + g:]])[:L]                   # the text holds g symbols the read skips
                    add(ins if ins.size == L else np.resize(ins, L), t, rng.integers(0, 256, L))
                    dl = np.concatenate([t[g:g + cut], rng.integers(0, 4, g, dtype=np.uint8), t[g + cut:]])[:L]     # the read holds g extra
                    add(dl, t, rng.integers(0, 256, L))
            add(src, t[:max(0, off + L - 2)], q_best)                                  # the window cut by the text's end
            add(src, t[:off + L + band // 2], rng.integers(0, 256, L))
        self.pats, self.txts, self.best = pats, txts, np.array(best)
        self.hp = O.StringSet.from_lists(pats, 4, True)
        self.ht = padded_texts(txts)
        total = int(self.hp.begin[-1] + self.hp.length[-1])
        self.quals = np.zeros(total + 4, np.uint8)
        for i, q in enumerate(quals):
            b = int(self.hp.begin[i]); self.quals[b:b + q.size] = q
        self.lengths = np.array([len(p) for p in pats])
        self.maxp = int(self.lengths.max())

    def dev(self, cuda):
        p = nvb.PackedStringSet.from_host(self.hp.words, 4, True, self.hp.begin, self.hp.length, device=cuda)
        t = nvb.PackedStringSet.from_host(self.ht.words, 2, True, self.ht.begin, self.ht.length, device=cuda)
        return p, t, torch.from_numpy(self.quals).to(cuda)

    def fixed(self, L, cuda):
        """the jobs of pattern length L as a fixed-length batch (patterns->length == NULL)"""
        idx = np.nonzero(self.lengths == L)[0]
        p = nvb.PackedStringSet(torch.from_numpy(self.hp.words.view(np.int32)).to(cuda), 4, True,
                                torch.from_numpy(self.hp.begin[idx].view(np.int64)).to(cuda), None, L)
        t = nvb.PackedStringSet(torch.from_numpy(self.ht.words.view(np.int32)).to(cuda), 2, True,
                                torch.from_numpy(self.ht.begin[idx].view(np.int64)).to(cuda),
                                torch.from_numpy(self.ht.length[idx].view(np.int32)).to(cuda))
        return idx, p, t


def padded_texts(txts):
    """the texts' stream with 64 spare symbols after the last one (the stream a caller's reference window lives in)"""
    ht = O.StringSet.from_lists(list(txts) + [np.zeros(64, np.uint8)], 2, True)
    return O.StringSet(ht.words, 2, True, ht.begin[:-1], ht.length[:-1])


def oracle_banded(s, ty, band, pr):
    if s.kind == "gotoh":
        return O.batch_banded_gotoh_score(band, ty, (s.match, s.mismatch, s.go, s.ge), pr.hp, pr.ht, n_threads=16)
    if s.kind == "sw":
        return O.batch_sw_score(band, ty, (s.match, s.mismatch, s.go, s.ge), pr.hp, pr.ht, n_threads=16)
    return O.batch_banded_gotoh_score_qual(band, ty, (s.match, s.go, s.ge, s.tgo, s.tge, 0), s.lut_array(), pr.quals, pr.hp, pr.ht, n_threads=16)


def assert_reaches_extremes(s, ty, pr, es):
    """the best-pair jobs score M x best_pair (LOCAL and SEMI_GLOBAL, the full read inside the band): the probe reaches the bound"""
    bp = best_pair_of(s)
    if ty == W.GLOBAL or bp <= 0 or max(s.go, s.ge, s.tgo, s.tge) > 0:          # (a gap that earns score beats any read of pairs)
        return
    idx = np.nonzero(pr.best)[0]
    assert idx.size > 0
    for i in idx:
        assert es[i] == pr.lengths[i] * bp, (s.name, ty, pr.lengths[i], es[i], bp)


def entry_tags(entry):
    return {"plain": ("banded_gotoh_score_kernel<A16>", "banded_gotoh_score_kernel<A32>"),
            "qual": ("banded_gotoh_score_kernel<A16,qual>", "banded_gotoh_score_kernel<A32,qual>"),
            "views": ("banded_gotoh_score_kernel<A16,qual,views>", "banded_gotoh_score_kernel<A32,qual,views>"),
            "bounded": ("banded_gotoh_score_kernel<A16,qual>", "banded_gotoh_score_kernel<A32,qual>"),
            "asym": ("banded_gotoh_score_kernel<A16X>", "banded_gotoh_score_kernel<A32X>")}[entry]


def run_banded(entry, s, ty, band, p, t, dq, n, maxp, flags=None):
    al = aligner(s, ty)
    if entry == "bounded":
        ns = torch.empty(n, dtype=torch.int32, device=p.words.device)
        nk = torch.empty((n, 2), dtype=torch.int32, device=p.words.device)
        n_dev = torch.tensor([n], dtype=torch.int32, device=p.words.device)
        nvb.BatchedBandedAlignmentScore(band).enact(al, p, t, ns, nk, maxp, 0, dq, None, None, n_dev, None)
        gs, gk = ns, nk
    elif entry in ("qual", "views"):
        gs, gk = nvb.batch_banded_alignment_score(band, al, p, t, quals=dq, pattern_flags=flags, max_pattern_length=maxp)
    else:
        gs, gk = nvb.batch_banded_alignment_score(band, al, p, t, max_pattern_length=maxp)
    torch.cuda.synchronize()
    return gs.cpu().numpy(), gk.cpu().numpy().view(np.uint32)


def probe_lengths(s, ty, band, entry_kind):
    lim16, lim16p = W.banded_limits(s, ty, band, entry_kind)
    Ls = W.probe_lengths([lim16, lim16p])
    if not Ls:                                      # never 16-bit, or beyond 2 000 symbols: the 32-bit kernel (or A16 at any length)
        Ls = [1, 37] if lim16 == 0 else [1, 300]
    return Ls


def check_banded_case(cuda, entry, s, ty, band, seed, nostage=False):
    kind = "asym" if entry == "asym" else "score"
    Ls = probe_lengths(s, ty, band, kind)
    pr = Probes(s, band, Ls, seed)
    p, t, dq = pr.dev(cuda)
    flags = None
    if entry == "views":
        # the same probes stored reversed and / or complemented: the kernel applies the view back as it fetches
        f = np.arange(len(pr.pats)) % 4
        stored, sq = [], pr.quals.copy()
        for i, v in enumerate(pr.pats):
            b, m = int(pr.hp.begin[i]), v.size
            w, q = v, pr.quals[b:b + m]
            if f[i] & 2:
                w = np.where(w < 4, 3 - w, w).astype(np.uint8)
            if f[i] & 1:
                w, q = w[::-1], q[::-1]
            stored.append(w.copy()); sq[b:b + m] = q
        hs = O.StringSet.from_lists(stored, 4, True)
        p = nvb.PackedStringSet.from_host(hs.words, 4, True, hs.begin, hs.length, device=cuda)
        dq = torch.from_numpy(sq).to(cuda)
        flags = torch.from_numpy(f.astype(np.uint8)).to(cuda)
    es, ek = oracle_banded(s, ty, band, pr)
    assert_reaches_extremes(s, ty, pr, es)
    n = len(pr.pats)
    tag16, tag32 = entry_tags(entry)
    for force32 in (0, 1):
        with switches(NVBIO_HIP_FORCE_32BIT=force32, NVBIO_HIP_NO_STAGING=int(nostage)):
            # ragged: every probe length in one batch, split per job across A16 / A16P / A32
            gs, gk = run_banded(entry, s, ty, band, p, t, dq, n, pr.maxp, flags)
            bad = np.nonzero((gs != es) | (gk != ek).any(1))[0]
            assert bad.size == 0, (entry, s.name, ty, band, force32, bad[:4], pr.lengths[bad[:4]], es[bad[:4]], gs[bad[:4]], ek[bad[:4]], gk[bad[:4]])
            if nostage:
                continue
            # fixed lengths: the tag names the width the mirror predicts
            for L in Ls:
                idx, fp, ft = pr.fixed(L, cuda)
                if entry == "views":
                    fp = nvb.PackedStringSet(p.words, 4, True, fp.begin, None, L)
                fs, fk = run_banded(entry, s, ty, band, fp, ft, dq, idx.size, L, flags[torch.from_numpy(idx).to(cuda)] if flags is not None else None)
                want = tag32 if force32 or W.banded_route(s, ty, band, L, kind) == "A32" else tag16
                assert last_kernel() == want, (entry, s.name, ty, band, L, W.banded_limits(s, ty, band, kind), last_kernel())
                assert (fs == es[idx]).all() and (fk == ek[idx]).all(), (entry, s.name, ty, band, L, force32)


# ---------------------------------------------------------------------------------------------------------------------------------
# banded score
# ---------------------------------------------------------------------------------------------------------------------------------
PLAIN = [s for s in W.CORPUS if s.kind == "gotoh"]
QUAL = [s for s in W.CORPUS if s.kind == "qual"]
ASYM = [s for s in W.CORPUS if s.kind == "sw"]


@pytest.mark.parametrize("band", W.BANDS)
@pytest.mark.parametrize("ty", W.TYPES)
def test_banded_plain_entry_at_the_limits(cuda, ty, band):
    """nvbio_hip_banded_gotoh_score over every plain corpus scheme, all five bands."""
    for k, s in enumerate(PLAIN):
        check_banded_case(cuda, "plain", s, ty, band, 100 * band + 10 * ty + k)


@pytest.mark.parametrize("entry", ["qual", "views", "bounded"])
@pytest.mark.parametrize("band", [3, 15, 31])
@pytest.mark.parametrize("ty", W.TYPES)
def test_banded_quality_entries_at_the_limits(cuda, ty, band, entry):
    """_qual, _qual_views (reversed / complemented views) and _qual_bounded without thresholds over the corpus's quality schemes: the
    LUT's best and worst entries along whole reads."""
    for k, s in enumerate(QUAL):
        check_banded_case(cuda, entry, s, ty, band, 200 * band + 10 * ty + k)


@pytest.mark.parametrize("band", [3, 15, 31])
@pytest.mark.parametrize("ty", W.TYPES)
def test_banded_sw_asymmetric_at_the_limits(cuda, ty, band):
    """nvbio_hip_banded_sw_score with deletion != insertion (A16X / A32X) over the corpus's asymmetric SW schemes: two cheap ones
    (only LOCAL's limits fall below 2 000 symbols) and a mid-cost one whose GLOBAL / SEMI_GLOBAL limits (245 / 233 / 217) are probed."""
    for k, s in enumerate(ASYM):
        check_banded_case(cuda, "asym", s, ty, band, 300 * band + 10 * ty + k)


@pytest.mark.parametrize("ty", W.TYPES)
def test_banded_without_staging(cuda, ty):
    """one pass with NVBIO_HIP_NO_STAGING=1 (the words fetched from global memory, not LDS)"""
    for k, s in enumerate(PLAIN[:17] + QUAL):
        check_banded_case(cuda, "plain" if s.kind == "gotoh" else "qual", s, ty, 15, 400 + 10 * ty + k, nostage=True)


# ---------------------------------------------------------------------------------------------------------------------------------
# the bounded scorer with thresholds
# ---------------------------------------------------------------------------------------------------------------------------------
BOUNDED_SCHEMES = QUAL + [W.Scheme.qual(1, -700, -600, -700, -600, np.full(256, -900), "infimum_crossing_qual")]


@pytest.mark.parametrize("band", [3, 15, 31])
@pytest.mark.parametrize("ty", W.TYPES)
def test_bounded_scorer_at_the_limits(cuda, ty, band):
    """nvbio_hip_banded_gotoh_score_qual_bounded with thresholds score - 1, score, score + 1 and INT32_MIN for every probe job: a job above
    its threshold is exact; a job given up reports an upper bound of its score at or below its threshold and the sink (-1, -1).  The
    schemes include match 0 in SEMI_GLOBAL (cap 0), a positive LUT entry (cap > match) and an infimum-crossing one."""
    for k, s in enumerate(BOUNDED_SCHEMES):
        Ls = probe_lengths(s, ty, band, "bounded")
        pr = Probes(s, band, Ls, 500 + 100 * band + 10 * ty + k)
        es, ek = oracle_banded(s, ty, band, pr)
        n = len(pr.pats)
        p, t, dq = pr.dev(cuda)
        # four copies of the jobs: thresholds score - 1, score, score + 1, INT32_MIN
        reps = 4
        idx = np.tile(np.arange(n), reps)
        pp = nvb.PackedStringSet(p.words, 4, True, p.begin[torch.from_numpy(idx).to(cuda)].contiguous(), p.length[torch.from_numpy(idx).to(cuda)].contiguous())
        tt = nvb.PackedStringSet(t.words, 2, True, t.begin[torch.from_numpy(idx).to(cuda)].contiguous(), t.length[torch.from_numpy(idx).to(cuda)].contiguous())
        E, EK = es[idx].astype(np.int64), ek[idx]
        thr = np.concatenate([E[:n] - 1, E[:n], E[:n] + 1, np.full(n, INT32_MIN)])
        thr[(E == NO_ALN) & (thr != INT32_MIN)] = -50
        thr = thr.clip(INT32_MIN, 1 << 24).astype(np.int32)
        al = aligner(s, ty)
        gaps_ok, cap = W.bounded_args(s)
        for force32 in (0, 1):
            with switches(NVBIO_HIP_FORCE_32BIT=force32):
                gs, gk = nvb.batch_banded_alignment_score(band, al, pp, tt, quals=dq, max_pattern_length=pr.maxp, min_score=torch.from_numpy(thr).to(cuda))
                torch.cuda.synchronize()
                assert "bounded" in last_kernel()
            gs, gk = gs.cpu().numpy().astype(np.int64), gk.cpu().numpy().view(np.uint32)
            above = E > thr
            bad = np.nonzero(above & ((gs != E) | (gk != EK).any(1)))[0]
            assert bad.size == 0, (s.name, ty, band, force32, bad[:4], E[bad[:4]], gs[bad[:4]], thr[bad[:4]])
            gave_up = ~above & (gk == 0xFFFFFFFF).all(1) & (E != NO_ALN)
            ran = ~above & ~gave_up
            assert (gs[ran] == E[ran]).all() and (gk[ran] == EK[ran]).all(), (s.name, ty, band, force32)
            assert (gs[gave_up] >= E[gave_up]).all() and (gs[gave_up] <= thr[gave_up]).all(), (s.name, ty, band, force32)
            if not gaps_ok:
                assert not gave_up.any()
        # the tag of a fixed-length batch at each probe length
        for L in Ls:
            fidx, fp, ft = pr.fixed(L, cuda)
            nvb.batch_banded_alignment_score(band, al, fp, ft, quals=dq, max_pattern_length=L,
                                             min_score=torch.full((fidx.size,), INT32_MIN, dtype=torch.int32, device=cuda))
            torch.cuda.synchronize()
            want = "banded_gotoh_score_bounded_kernel<A%d,qual>" % (16 if W.banded_route(s, ty, band, L, "bounded") != "A32" else 32)
            assert last_kernel() == want, (s.name, ty, band, L, last_kernel())


# ---------------------------------------------------------------------------------------------------------------------------------
# the wave kernel
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("band", [3, 15, 31])
@pytest.mark.parametrize("ty", W.TYPES)
def test_wave_kernel_on_the_corpus(cuda, ty, band):
    """batch_banded_alignment_score_wave over the quality corpus at the probe lengths up to its 512 rows."""
    for k, s in enumerate(QUAL):
        Ls = [L for L in probe_lengths(s, ty, band, "score") if L <= 512] or [1, 200]
        pr = Probes(s, band, Ls, 600 + 100 * band + 10 * ty + k)
        es, ek = oracle_banded(s, ty, band, pr)
        p, t, dq = pr.dev(cuda)
        ws, wk = batch_banded_alignment_score_wave(band, aligner(s, ty), p, t, dq, max_pattern_length=pr.maxp)
        torch.cuda.synchronize()
        assert last_kernel() == "banded_gotoh_wave_kernel"
        ws, wk = ws.cpu().numpy(), wk.cpu().numpy().view(np.uint32)
        bad = np.nonzero((ws != es) | (wk != ek).any(1))[0]
        assert bad.size == 0, (s.name, ty, band, bad[:4], es[bad[:4]], ws[bad[:4]])


def test_wave_kernel_lut_range(cuda):
    """LUT entries of -32768 and 32767 are accepted (and exact); -32769 and 32768 are refused."""
    rng = np.random.default_rng(77)
    for lo, hi, ok in ((-32768, 32767, True), (-32769, 0, False), (0, 32768, False)):
        lut = np.full(256, -3); lut[0], lut[1] = lo, hi
        s = W.Scheme.qual(0, -5, -3, -5, -3, lut, "range")
        assert W.wave_lut_ok(s.lut) == ok
        pr = Probes(s, 15, [20, 60], 7000 + int(ok))
        pr.quals[:] = rng.integers(0, 3, pr.quals.size)
        p, t, dq = pr.dev(cuda)
        for ty in W.TYPES:
            if not ok:
                with pytest.raises(RuntimeError):
                    batch_banded_alignment_score_wave(15, aligner(s, ty), p, t, dq, max_pattern_length=pr.maxp)
                continue
            es, ek = oracle_banded(s, ty, 15, pr)
            ws, wk = batch_banded_alignment_score_wave(15, aligner(s, ty), p, t, dq, max_pattern_length=pr.maxp)
            torch.cuda.synchronize()
            assert (ws.cpu().numpy() == es).all() and (wk.cpu().numpy().view(np.uint32) == ek).all(), ty


# ---------------------------------------------------------------------------------------------------------------------------------
# the full-matrix score gates
# ---------------------------------------------------------------------------------------------------------------------------------
def full_jobs(rng, M, N, n=24, short_n=None):
    """n jobs: patterns of M symbols (the first a perfect match, then all-mismatch, N symbols, gapped and random ones), texts of N"""
    pats, txts = [], []
    for i in range(n):
        Ni = N if i % 3 != 2 else (short_n or max(1, N // 2))
        t = rng.integers(0, 4, Ni, dtype=np.uint8)
        off = int(rng.integers(0, max(1, Ni - M + 1)))
        src = np.resize(t[off:off + M] if Ni > off else t, M)
        k = i % 6
        p = src if k == 0 else (3 - src) if k == 1 else np.full(M, 4, np.uint8) if k == 2 else rng.integers(0, 4, M, dtype=np.uint8)
        if k == 3 and M > 12:
            p = np.concatenate([src[:M // 2], src[M // 2 + 5:], rng.integers(0, 4, 5, dtype=np.uint8)])
        pats.append(np.asarray(p, np.uint8)); txts.append(t)
    return pats, txts


def oracle_full(s, ty, hp, ht, quals=None, pattern_blocking=False):
    if s.kind == "qual":
        es, ek, ok = O.batch_gotoh_score_qual(0 if pattern_blocking else 1, ty, (s.match, s.go, s.ge, s.tgo, s.tge), s.lut_array(), quals, hp, ht, n_threads=16)
    elif pattern_blocking:
        es, ek, ok = O.batch_score_pattern_blocking(1 if s.kind == "sw" else 0, ty, (s.match, s.mismatch, s.go, s.ge), hp, ht, n_threads=16)
    elif s.kind == "sw":
        es, ek = O.batch_sw_score(0, ty, (s.match, s.mismatch, s.go, s.ge), hp, ht, n_threads=16)
        ok = np.ones(es.size, np.uint8)
    else:
        es, ek, ok = O.batch_gotoh_score(ty, (s.match, s.mismatch, s.go, s.ge), hp, ht, n_threads=16)
    return es, ek, ok


ROUTE_TAG = {"sweep16": lambda k: "16-bit" in k, "generic": lambda k: k == "full_gotoh_score_kernel", "trunc": lambda k: k == "full_gotoh_score_kernel",
             "ed": lambda k: k == "edit_distance_bitvector_kernel", "striped": lambda k: k.startswith("full_gotoh_striped_kernel")}


def check_full(cuda, s, ty, M, N, seed, pattern_blocking=False, n=24, exact=True):
    """announce maxM = M, maxN = N (the longest job of each), run, compare with the oracle and the route tag with the mirror"""
    route = W.full_route(s, ty, M, N, pattern_blocking)
    rng = np.random.default_rng(seed)
    pats, txts = full_jobs(rng, M, N, n)
    hp, ht = O.StringSet.from_lists(pats, 4, True), padded_texts(txts)
    quals = rng.integers(0, 256, int(hp.begin[-1] + hp.length[-1]) + 4).astype(np.uint8)
    if s.kind == "qual":                                         # half the symbols at the LUT's best entry
        quals[rng.random(quals.size) < 0.5] = int(np.argmax(s.lut))
        for i in range(1, n, 6):                                 # the all-mismatch reads wholly at it
            quals[int(hp.begin[i]):int(hp.begin[i]) + len(pats[i])] = int(np.argmax(s.lut))
    p = nvb.PackedStringSet.from_host(hp.words, 4, True, hp.begin, hp.length, device=cuda)
    t = nvb.PackedStringSet.from_host(ht.words, 2, True, ht.begin, ht.length, device=cuda)
    al = aligner(s, ty, nvb.PATTERN_BLOCKING if pattern_blocking else nvb.TEXT_BLOCKING)
    dq = torch.from_numpy(quals).to(cuda)
    if route == "refused":
        with pytest.raises(RuntimeError):
            nvb.batch_alignment_score(al, p, t, M, N, quals=dq)
        return route, None
    es, ek, eok = oracle_full(s, ty, hp, ht, quals, pattern_blocking)
    gs, gk, gok = nvb.batch_alignment_score(al, p, t, M, N, quals=dq)
    torch.cuda.synchronize()
    if s.kind == "sw" and s.go == s.ge and route in ("sweep16", "generic"):
        # nvbio_hip_sw_score names every run that is neither the bit-vector nor the striped kernel "<16-bit,sw>" (full_gotoh.hip:1203),
        # the int32 sweep included: on this entry the tag tells only those two kernels apart (the Gotoh entry pins sweep16 / generic)
        assert last_kernel() == "full_gotoh_score_kernel<16-bit,sw>", (s.name, ty, M, N, route, last_kernel())
    else:
        assert ROUTE_TAG[route](last_kernel()), (s.name, ty, M, N, route, last_kernel())
    gs, gk, gok = gs.cpu().numpy(), gk.cpu().numpy().view(np.uint32), gok.cpu().numpy()
    assert (gs == es).all(), (s.name, ty, M, N, route, np.nonzero(gs != es)[0][:4], es[:4], gs[:4])
    if ty != W.LOCAL or pattern_blocking or s.kind != "sw":
        assert (gk == ek).all(), (s.name, ty, M, N, route)
    assert (gok == eok).all(), (s.name, ty, M, N, route)
    return route, es


def test_full_local_best_pair_gate(cuda):
    """LOCAL's maxM * best_pair < 2048, with the best pair from match, from a mismatch and from the LUT: 89 x 23 = 2047 runs the 16-bit
    sweep, 64 x 32 = 2048 does not; the best-pair read reaches maxM x best_pair"""
    for bp, M, admitted in ((23, 89, True), (32, 64, False)):
        assert (M * bp < 2048) == admitted
        lut = np.r_[np.full(255, -4), [bp]]
        for s in (W.Scheme.gotoh(bp, -3, -5, -2, "m"), W.Scheme.gotoh(0, bp, -5, -2, "x"), W.Scheme.qual(1, -5, -2, -6, -3, lut, "lut")):
            route, es = check_full(cuda, s, W.LOCAL, M, 120, 11 + bp)
            assert route == ("sweep16" if admitted else "refused" if s.kind == "qual" else "generic"), (s.name, M, route)
            if route != "refused":
                assert es.max() == M * bp
    s = BY_NAME["bench"]
    assert check_full(cuda, s, W.LOCAL, 1023, 1100, 13, n=6)[0] == "sweep16"
    assert check_full(cuda, s, W.LOCAL, 1024, 1100, 14, n=6)[0] == "generic"


def test_full_cost_and_span_gates(cuda):
    """LOCAL's A * 3 < 2000 (666 / 667), and span * A < 30000: (maxM + 4) * 30 = 29 970 / 30 000 for SEMI_GLOBAL and LOCAL, plain and
    quality schemes (the latter have no form beyond int16: refused)"""
    assert check_full(cuda, W.Scheme.gotoh(1, -666, -10, -10, "A666"), W.LOCAL, 40, 60, 21)[0] == "sweep16"
    assert check_full(cuda, W.Scheme.gotoh(1, -667, -10, -10, "A667"), W.LOCAL, 40, 60, 22)[0] == "generic"
    q = W.Scheme.qual(0, -30, -29, -30, -30, np.full(256, -3), "A30q")
    for ty in (W.LOCAL, W.SEMI_GLOBAL):
        for s in (W.Scheme.gotoh(0, -30, -29, -30, "A30"), q):
            assert check_full(cuda, s, ty, 995, 1000, 23, n=8)[0] == "sweep16"
            assert check_full(cuda, s, ty, 996, 1000, 24, n=8)[0] == ("refused" if s.kind == "qual" else "trunc")


def test_full_global_tighter_bound(cuda):
    """GLOBAL's own admission of the 16-bit sweep: `low` (the boundary lines, and reaching a cell by one gap run) just under and just
    over 32 000, with jobs of N = maxN that walk the boundary row."""
    s = W.Scheme.gotoh(1, -2, -12, -10, "glob")
    found = []
    for N in range(2900, 3300):
        low, high = W.global_bounds(s, 40, N)
        if low < 32000 <= W.global_bounds(s, 40, N + 1)[0]:
            found.append(N)
            break
    assert found
    N = found[0]
    assert check_full(cuda, s, W.GLOBAL, 40, N, 31, n=12)[0] == "sweep16"
    assert check_full(cuda, s, W.GLOBAL, 40, N + 1, 32, n=12)[0] == "trunc"


def test_full_global_tighter_bound_with_a_lut_entry_above_match(cuda):
    """GLOBAL's `high` on the quality entry: match 0, every gap -1, LUT[1] = 100, every other entry -1.  The best pair is the LUT entry
    (the entry's own mismatch is the LUT's most negative one), so high = maxM * 100 + 108: M = N = 318 runs the 16-bit sweep and its
    all-best-pair read scores 31 800 exactly; 319 is refused (the quality scheme has no int32 sweep), and so is M = N = 400, whose
    all-best-pair read scores 33 372 in the reference (above what the int16 sweep can report)."""
    lut = np.full(256, -1); lut[1] = 100
    s = W.Scheme.qual(0, -1, -1, -1, -1, lut, "lut100")
    route, es = check_full(cuda, s, W.GLOBAL, 318, 318, 35, n=12)
    assert route == "sweep16" and es[1] == 318 * 100
    assert check_full(cuda, s, W.GLOBAL, 319, 319, 36, n=12)[0] == "refused"
    assert check_full(cuda, s, W.GLOBAL, 400, 400, 37, n=12)[0] == "refused"


def test_full_text_length_and_order_key_gates(cuda):
    """maxN = 2^20 - 1 against 2^20 (one job with a short pattern), and the 32-bit order-key refusals announced on a tiny batch"""
    s = W.Scheme.gotoh(1, -1, -1, -1, "one")
    assert W.full_route(s, W.SEMI_GLOBAL, 8, (1 << 20) - 1) == "sweep16" and W.full_route(s, W.SEMI_GLOBAL, 8, 1 << 20) == "generic"
    rng = np.random.default_rng(41)
    for N in ((1 << 20) - 1, 1 << 20):
        t = rng.integers(0, 4, N, dtype=np.uint8)
        p = t[N - 9:N - 1].copy()
        hp, ht = O.StringSet.from_lists([p], 4, True), padded_texts([t])
        es, ek, eok = O.batch_gotoh_score(W.SEMI_GLOBAL, (1, -1, -1, -1), hp, ht, n_threads=16)
        dp = nvb.PackedStringSet.from_host(hp.words, 4, True, hp.begin, hp.length, device=cuda)
        dt = nvb.PackedStringSet.from_host(ht.words, 2, True, ht.begin, ht.length, device=cuda)
        route = W.full_route(s, W.SEMI_GLOBAL, 8, N)
        gs, gk, gok = nvb.batch_alignment_score(aligner(s, W.SEMI_GLOBAL), dp, dt, 8, N)
        torch.cuda.synchronize()
        assert ROUTE_TAG[route](last_kernel()), (N, route, last_kernel())
        assert int(gs[0]) == int(es[0]) == 8 and (gk.cpu().numpy().view(np.uint32) == ek).all()
    # order keys: maxN * 64 * 8 >= 2^32 is refused before any launch (nothing is read past the tiny batch)
    hp, ht = O.StringSet.from_lists([np.zeros(4, np.uint8)], 4, True), O.StringSet.from_lists([np.zeros(8, np.uint8)], 2, True)
    dp = nvb.PackedStringSet.from_host(hp.words, 4, True, hp.begin, hp.length, device=cuda)
    dt = nvb.PackedStringSet.from_host(ht.words, 2, True, ht.begin, ht.length, device=cuda)
    for M, N in ((100, (1 << 32) // 512), (600, (1 << 32) // 1024)):
        assert W.full_route(s, W.SEMI_GLOBAL, M, N) == "refused"
        with pytest.raises(RuntimeError):
            nvb.batch_alignment_score(aligner(s, W.SEMI_GLOBAL), dp, dt, M, N)


def test_full_edit_distance_and_striped_routes(cuda):
    """maxM 512 / 513 on the edit-distance scheme (bit-vector kernel / sweep), 1 024 / 1 025 into the striped kernel, and the SW
    asymmetric striped route at its inside16 edge (pattern blocking admitted inside int16 only)"""
    ed = W.Scheme.sw(0, -1, -1, -1, "ed")
    for ty in (W.GLOBAL, W.SEMI_GLOBAL):
        assert check_full(cuda, ed, ty, 512, 560, 51, n=8)[0] == "ed"
        assert check_full(cuda, ed, ty, 513, 560, 52, n=8)[0] == "sweep16"               # (the SW entry: not the bit-vector kernel)
        assert check_full(cuda, W.Scheme.gotoh(0, -1, -1, -1, "ed_gotoh"), ty, 513, 560, 52, n=8)[0] == "sweep16"       # the sweep itself
    g = W.Scheme.gotoh(2, -1, -2, -1, "bench")
    for ty in W.TYPES:
        assert check_full(cuda, g, ty, 1024, 1100, 53, n=6)[0] in ("sweep16", "generic", "trunc")
        assert check_full(cuda, g, ty, 1025, 1100, 54, n=6)[0] == "striped"
    a = W.Scheme.sw(3, -4, -5, -2, "asym")
    assert check_full(cuda, a, W.SEMI_GLOBAL, 300, 340, 55, n=6)[0] == "striped"
    assert check_full(cuda, a, W.SEMI_GLOBAL, 300, 340, 56, n=6, pattern_blocking=True)[0] == "striped"
    b = W.Scheme.sw(3, -4, -100, -2, "asym100")             # SEMI_GLOBAL inside16: (M + 4) * 100 < 30000 up to M = 295
    assert W.sw_asym_inside16(b, W.SEMI_GLOBAL, 295, 340) and not W.sw_asym_inside16(b, W.SEMI_GLOBAL, 296, 340)
    assert check_full(cuda, b, W.SEMI_GLOBAL, 295, 340, 59, n=6, pattern_blocking=True)[0] == "striped"      # 299 * 100 = 29 900
    assert check_full(cuda, b, W.SEMI_GLOBAL, 296, 340, 58, n=6, pattern_blocking=True)[0] == "refused"      # 300 * 100 = 30 000
    assert check_full(cuda, b, W.SEMI_GLOBAL, 296, 340, 57, n=6)[0] == "striped"                             # text blocking runs on


# ---------------------------------------------------------------------------------------------------------------------------------
# tracebacks
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("band", [3, 15, 31])
def test_banded_traceback_at_its_limit(cuda, band):
    """(maxM + band + 2) * A < 32000: at the last admitted maxM the extreme jobs' score, sink, source and CIGAR equal the oracle's; one
    symbol more is refused (RuntimeError), not approximated"""
    from test_traceback_gpu import compare
    for k, s in enumerate([W.Scheme.gotoh(3, -40, -60, -30, "A60"), W.Scheme.gotoh(5, 6, -40, -20, "x6"),
                           W.Scheme.qual(2, -8, -3, -11, -7, W.nvbowtie_lut(2, 90), "q90")]):
        A = W.banded_inputs(s)[0]
        M = 32000 // A - band - 2
        while (M + band + 2) * A >= 32000:
            M -= 1
        assert W.banded_traceback_ok(s, band, M) and not W.banded_traceback_ok(s, band, M + 1)
        pr = Probes(s, band, [M - 1, M], 900 + band + k)
        p, t, dq = pr.dev(cuda)
        al = aligner(s, W.SEMI_GLOBAL)
        stride = 64
        if s.kind == "qual":
            exp = O.batch_banded_gotoh_traceback(band, W.SEMI_GLOBAL, (s.match, s.go, s.ge, s.tgo, s.tge), pr.hp, pr.ht, stride, mm_lut=s.lut_array(), quals=pr.quals)
        else:
            exp = O.batch_banded_gotoh_traceback(band, W.SEMI_GLOBAL, (s.match, s.mismatch, s.go, s.ge), pr.hp, pr.ht, stride)
        got = nvb.batch_banded_alignment_traceback(band, al, p, t, max_pattern_length=M, quals=dq, cigar_stride=stride)
        torch.cuda.synchronize()
        compare(exp, got, (s.name, band, M))
        with pytest.raises(RuntimeError):
            nvb.batch_banded_alignment_traceback(band, al, p, t, max_pattern_length=M + 1, quals=dq, cigar_stride=stride)


@pytest.mark.parametrize("lanes", [0, 1])
def test_full_traceback_at_its_limit(cuda, lanes):
    """span * A < 30000 for the full-matrix traceback, both tb_kernel modes: exact at the last admitted maxM, refused one symbol past it"""
    from test_traceback_gpu import compare
    with switches(NVBIO_HIP_TRACEBACK_LANES=lanes):
        for k, (s, ty) in enumerate(((W.Scheme.gotoh(2, -60, -80, -40, "A80"), W.SEMI_GLOBAL), (W.Scheme.gotoh(2, -60, -80, -40, "A80"), W.LOCAL),
                                     (W.Scheme.gotoh(1, -3, -30, -20, "A30g"), W.GLOBAL))):
            N0 = 500 if ty == W.GLOBAL else 420
            M = next(m for m in range(2000, 0, -1) if W.full_traceback_ok(s, ty, m, N0))
            assert not W.full_traceback_ok(s, ty, M + 1, N0)
            rng = np.random.default_rng(990 + k + 10 * lanes)
            pats, txts = full_jobs(rng, M, N0, n=8, short_n=N0 - 20)
            hp, ht = O.StringSet.from_lists(pats, 4, True), padded_texts(txts)
            p = nvb.PackedStringSet.from_host(hp.words, 4, True, hp.begin, hp.length, device=cuda)
            t = nvb.PackedStringSet.from_host(ht.words, 2, True, ht.begin, ht.length, device=cuda)
            exp = O.batch_gotoh_traceback(ty, (s.match, s.mismatch, s.go, s.ge), hp, ht, 64)
            got = nvb.batch_alignment_traceback(aligner(s, ty), p, t, M, N0, cigar_stride=64)
            torch.cuda.synchronize()
            compare(exp, got, (s.name, ty, M, lanes))
            with pytest.raises(RuntimeError):
                nvb.batch_alignment_traceback(aligner(s, ty), p, t, M + 1, N0, cigar_stride=64)
