"""A plain-Python mirror of the host rules that choose each DP kernel's arithmetic width or route, and a corpus of edge schemes.

Every DP family in nvbio_amd/csrc decides on the host, from the scheme, the type, the band and the announced lengths, whether a job may
run in 16-bit lanes (whose adds wrap), in 32-bit lanes, on the reference's int16-truncating form, on another kernel, or not at all.  The
functions below restate those rules line for line (each docstring names the C lines it mirrors); tests/test_width_limits_gpu.py pins
them to the library through nvbio_hip_last_kernel() on fixed-length batches, and then drives jobs to the values the rules bound.

Schemes are `Scheme` tuples: kind "gotoh" (SimpleGotohScheme), "sw" (SimpleSmithWatermanScheme: gap_open = deletion, gap_ext = insertion)
or "qual" (nvBowtie's quality scheme: pattern / text gap costs and a 256-entry mismatch LUT indexed by quality).
"""
from collections import namedtuple

import numpy as np

GLOBAL, LOCAL, SEMI_GLOBAL = 0, 1, 2
TYPES = (GLOBAL, LOCAL, SEMI_GLOBAL)
BANDS = (3, 5, 7, 15, 31)
NEVER = 0
ALWAYS = 0xFFFFFFFF          # max_len_16bit's "every length"


class Scheme(namedtuple("Scheme", "kind match mismatch go ge tgo tge lut name")):
    """kind "gotoh": (match, mismatch, go, ge), text gaps = pattern gaps.  kind "sw": go = deletion, ge = insertion.
    kind "qual": go / ge = pattern gap costs, tgo / tge = text gap costs, lut[256] = mismatch(quality), mismatch unused."""

    @staticmethod
    def gotoh(m, x, go, ge, name=None):
        return Scheme("gotoh", m, x, go, ge, go, ge, None, name or "g%s" % str((m, x, go, ge)))

    @staticmethod
    def sw(m, x, deletion, insertion, name=None):
        return Scheme("sw", m, x, deletion, insertion, deletion, insertion, None, name or "sw%s" % str((m, x, deletion, insertion)))

    @staticmethod
    def qual(m, pgo, pge, tgo, tge, lut, name):
        lut = np.asarray(lut, dtype=np.int64)
        assert lut.shape == (256,)
        return Scheme("qual", m, None, pgo, pge, tgo, tge, tuple(int(v) for v in lut), name)

    def costs(self):
        """Every cost the scheme can charge (for the |c| <= 2^13 corpus bound)."""
        c = [self.match, self.go, self.ge, self.tgo, self.tge]
        return c + list(self.lut) if self.kind == "qual" else c + [self.mismatch]

    def lut_array(self):
        """The mismatch of each quality (the plain schemes' constant one for every quality)."""
        return np.array(self.lut if self.kind == "qual" else [self.mismatch] * 256, dtype=np.int32)


# ---------------------------------------------------------------------------------------------------------------------------------
# banded score: csrc/banded_gotoh.hip
# ---------------------------------------------------------------------------------------------------------------------------------
def max_len_16bit(match, best_pair, A, gap_open, gap_ext, ty, band, row_step):
    """banded_gotoh.hip:113-126: the longest pattern the 16-bit kernel is exact for (NEVER = 0, ALWAYS = 2^32 - 1)."""
    if gap_open > 0 or gap_ext > 0:
        return NEVER
    if A == 0:
        return ALWAYS
    if ty == LOCAL:
        if match < 0 or A > 100:
            return NEVER
        per_row = max(best_pair, 0) + row_step
        if per_row <= 0:
            return ALWAYS
        return 1022 // per_row
    lim = (15000 // A - band - 2)
    lim = int(lim / (2 if row_step else 1))          # C division truncates toward zero
    return max(lim, 0)


def banded_inputs(s):
    """A (the largest |cost|) and best_pair (the largest substitution score) as each entry computes them:
    banded_gotoh.hip:232-233 (plain), :273-276 (qual / views), :311-314 (bounded), :365-366 (SW, deletion != insertion)."""
    if s.kind == "qual":
        A = max(abs(v) for v in (s.match, s.go, s.ge, s.tgo, s.tge) + s.lut)
        return A, max((s.match,) + s.lut)
    return max(abs(s.match), abs(s.mismatch), abs(s.go), abs(s.ge)), max(s.match, s.mismatch)


def banded_limits(s, ty, band, entry="score"):
    """banded_gotoh.hip:137-145 -> (lim16, lim16p): jobs of up to lim16 symbols run the row-frame 16-bit kernel (A16), jobs in
    (lim16, lim16p] the 16-bit instance of the recurrence as written (A16P, LOCAL only), longer ones the 32-bit kernel.
    entry: "score" (plain, qual, views, bounded without thresholds), "bounded" (with thresholds) or "asym" (SW, deletion != insertion);
    the last two are not in the row frame.  The SW entry with deletion == insertion is the plain Gotoh one (banded_gotoh.hip:344-348)."""
    A, best_pair = banded_inputs(s)
    if s.kind == "sw":
        # p.gap_open = p.gap_ext = insertion, p.txt_gap_* = deletion (banded_gotoh.hip:360-362)
        pgo = pge = s.ge
        tgo = tge = s.go
        if s.go == s.ge:
            entry = "score"
    else:
        pgo, pge, tgo, tge = s.go, s.ge, s.tgo, s.tge
    rt = entry == "score"
    go, ge = max(pgo, tgo), max(pge, tge)
    lim_plain = max_len_16bit(s.match, best_pair, A, go, ge, ty, band, 0)
    if not rt:
        return lim_plain, lim_plain
    lim16 = max_len_16bit(s.match, best_pair, A, go, ge, ty, band, -pge if pge < 0 else 0)
    lim16p = lim_plain if (ty == LOCAL and lim_plain > lim16) else lim16
    return lim16, lim16p


def banded_route(s, ty, band, L, entry="score"):
    """banded_gotoh.hip:172-190 for a fixed-length batch of L symbols: "A16", "A16P" or "A32"."""
    lim16, lim16p = banded_limits(s, ty, band, entry)
    if lim16 > 0 and L <= lim16:
        return "A16"
    if lim16p > lim16 and lim16 < L <= lim16p:
        return "A16P"
    return "A32"


def bounded_args(s):
    """banded_gotoh.hip:325-328 -> (gaps_ok, cap): thresholds are honoured only if no pattern gap scores above zero; cap is what one
    more row can add to a job's score in the give-up bound (banded_gotoh_bounded.h:239-251)."""
    _, best_pair = banded_inputs(s)
    return (s.go <= 0 and s.ge <= 0), max(best_pair, 0)


def wave_lut_ok(lut):
    """banded_gotoh_wave.hip:187: every LUT entry must fit int16."""
    return all(-32768 <= int(v) <= 32767 for v in lut)


# ---------------------------------------------------------------------------------------------------------------------------------
# full-matrix score: csrc/full_gotoh.hip
# ---------------------------------------------------------------------------------------------------------------------------------
ED = (0, -1, -1, -1)


def full_route(s, ty, maxM, maxN, pattern_blocking=False, min_score=False, bits=4):
    """full_gotoh.hip:1058-1157 (and the entries :1176-1233) -> one of "refused", "striped", "ed" (edit_distance_bitvector_kernel),
    "sweep16" (the 16-bit sweep), "trunc" (the reference's int16-truncating form) or "generic" (the int32 sweep).
    s.kind "gotoh" = nvbio_hip_gotoh_score / alignment_score; "sw" with deletion == insertion = nvbio_hip_sw_score (block 16);
    "sw" with deletion != insertion = the asymmetric striped kernel (sw_asym_route); "qual" = nvbio_hip_alignment_score_qual."""
    if s.kind == "sw" and s.go != s.ge:
        return sw_asym_route(s, ty, maxM, maxN, pattern_blocking)
    qual = s.kind == "qual"
    if qual:
        # alignment_score_qual (:1215-1217): the scheme's mismatch is the LUT's most negative entry, or 0
        g = (s.match, min([0] + list(s.lut)), s.go, s.ge)
    else:
        g = (s.match, s.mismatch, s.go, s.ge)
    blk4 = s.kind == "sw"
    if maxM == 0 or maxN == 0:
        return "refused"
    striped = maxM > 1024
    if not striped and maxN * 64 * (8 if maxM <= 512 else 16) >= (1 << 32):
        return "refused"                                     # LOCAL order keys are 32-bit (:1060)
    A = max(abs(v) for v in g)
    if qual:
        A = max([A] + [abs(v) for v in s.lut] + [abs(s.tgo), abs(s.tge)])
    span = maxM + maxN + 4 if ty == GLOBAL else maxM + 4
    gaps_cost = g[2] <= 0 and g[3] <= 0 and (not qual or (s.tgo <= 0 and s.tge <= 0))
    trunc = not (gaps_cost and span * A < 30000)
    if trunc and gaps_cost and ty == GLOBAL and global_lines_fit(s, maxM, maxN, pattern_blocking):
        trunc = False
    if striped:
        if qual:
            return "refused"
        if pattern_blocking and (min_score or trunc):
            return "refused"
        return "striped"
    best_pair = max(g[0], g[1])
    if qual:
        best_pair = max([best_pair] + list(s.lut))
    fast = (not trunc) and maxN < (1 << 20) and (ty != LOCAL or (g[0] >= 0 and maxM * best_pair < 2048 and A * 3 < 2000))
    ed = (not qual) and blk4 and g == ED
    if ed and not trunc and ty != LOCAL and not min_score and maxM <= 512 and bits != 8:
        return "ed"
    if fast:
        return "sweep16"
    if trunc and blk4:
        return "refused"                                     # :1162
    if pattern_blocking or qual:
        return "refused"                                     # :1163-1164
    return "trunc" if trunc else "generic"


def global_bounds(s, maxM, maxN, pattern_blocking=False):
    """full_gotoh.hip:1070-1089: (low, high) of GLOBAL's tighter admission of the 16-bit sweep.  `high` bounds the interior H by
    maxM times the best pair score, a mismatch or a LUT entry above match included (on the quality entry the scheme's own mismatch is
    the LUT's most negative entry, so the LUT is consulted directly)."""
    qual = s.kind == "qual"
    g = (s.match, min([0] + list(s.lut)), s.go, s.ge) if qual else (s.match, s.mismatch, s.go, s.ge)
    tgo, tge = (s.tgo, s.tge) if qual else (g[2], g[3])
    col_go, col_ge = (g[2], g[3]) if pattern_blocking else (tgo, tge)
    row_go, row_ge = (tgo, tge) if pattern_blocking else (g[2], g[3])
    row_line = abs(row_go) + abs(row_ge) * maxN
    col_line = abs(col_go) + abs(col_ge) * maxM
    via_top = row_line + abs(g[2]) + abs(g[3]) * maxM
    via_left = col_line + abs(g[2]) + abs(g[3]) * maxN
    worst_sub = max(abs(g[0]), abs(g[1]))
    if qual:
        worst_sub = max([worst_sub] + [abs(v) for v in s.lut])
    low = max(row_line, col_line, min(via_top, via_left)) + abs(g[2]) + abs(g[3]) + worst_sub + 8
    best_pair = max([g[0], g[1]] + (list(s.lut) if qual else []))
    high = maxM * max(0, best_pair) + worst_sub + 8
    return low, high


def global_lines_fit(s, maxM, maxN, pattern_blocking=False):
    low, high = global_bounds(s, maxM, maxN, pattern_blocking)
    return low < 32000 and high < 32000


def sw_asym_route(s, ty, maxM, maxN, pattern_blocking=False):
    """full_gotoh.hip:988-1010: SW with deletion != insertion -> "striped", or "refused" for pattern blocking outside int16."""
    if maxM == 0 or maxN == 0:
        return "refused"
    A = max(abs(s.match), abs(s.mismatch), abs(s.go), abs(s.ge))
    span = maxM + maxN + 4 if ty == GLOBAL else maxM + 4
    inside16 = s.go <= 0 and s.ge <= 0 and span * A < 30000
    if pattern_blocking and not inside16:
        return "refused"
    return "striped"


def sw_asym_inside16(s, ty, maxM, maxN):
    A = max(abs(s.match), abs(s.mismatch), abs(s.go), abs(s.ge))
    span = maxM + maxN + 4 if ty == GLOBAL else maxM + 4
    return s.go <= 0 and s.ge <= 0 and span * A < 30000


# ---------------------------------------------------------------------------------------------------------------------------------
# tracebacks: csrc/banded_traceback.hip, csrc/full_traceback.hip
# ---------------------------------------------------------------------------------------------------------------------------------
def banded_traceback_ok(s, band, maxM):
    """banded_traceback.hip:411-412 with A from :486 (plain), :509-511 (qual), :536 (SW): the int16 checkpoints are lossless."""
    if s.kind == "sw":
        A = max(abs(s.match), abs(s.mismatch), abs(s.go))
    else:
        A, _ = banded_inputs(s)
    return (maxM + band + 2) * A < 32000 and maxM < (1 << 14)


def full_traceback_ok(s, ty, maxM, maxN):
    """full_traceback.hip:556-564: 14-bit lengths, no gap move that earns score, span * A < 30000."""
    if maxM >= (1 << 14) or maxN >= (1 << 14):
        return False
    qual = s.kind == "qual"
    A = max(abs(s.match), abs(s.go), abs(s.ge))
    A = max([A] + ([abs(v) for v in s.lut] + [abs(s.tgo), abs(s.tge)] if qual else [abs(s.mismatch)]))
    span = maxM + maxN + 4 if ty == GLOBAL else maxM + 4
    gaps_cost = s.go <= 0 and s.ge <= 0 and (not qual or (s.tgo <= 0 and s.tge <= 0))
    return gaps_cost and span * A < 30000


# ---------------------------------------------------------------------------------------------------------------------------------
# the scheme corpus
# ---------------------------------------------------------------------------------------------------------------------------------
COST_BOUND = 1 << 13


def _lut(base, **at):
    v = np.full(256, base, dtype=np.int64)
    for q, c in at.items():
        v[int(q[1:])] = c
    return v


def nvbowtie_lut(mmp_min=2, mmp_max=6):
    """QualCost(min, max) as nvBowtie writes it (scoring.h:86-104), negated."""
    q = np.minimum(np.arange(256), 40).astype(np.float32) / np.float32(40.0)
    return -(mmp_min + (q * np.float32(mmp_max - mmp_min)).astype(np.int64))


FIXED_SCHEMES = [
    Scheme.gotoh(0, 0, 0, 0, "zero"),                                   # A == 0: 16-bit at any length, every cell ties
    Scheme.gotoh(-1, -2, -3, -1, "match_negative"),                     # LOCAL with match < 0: never 16-bit
    Scheme.gotoh(2, -1, 1, -1, "gap_open_positive"),                    # a gap that earns score: 32 bits
    Scheme.gotoh(2, -3, -5, 0, "gap_ext_zero"),                         # G_e == 0: no row step
    Scheme.gotoh(2, -3, 0, -2, "gap_open_zero"),
    Scheme.gotoh(1, -2, -2, -6, "ext_above_open"),                      # |G_e| > |G_o|
    Scheme.gotoh(3, 5, -4, -2, "mismatch_above_match"),                 # best_pair from the mismatch: LOCAL 146 / 204
    Scheme.gotoh(5, -40, -60, -30, "mid_cost"),                         # LOCAL 29 / 204
    Scheme.gotoh(10, -100, -100, -100, "A100"),                         # LOCAL admitted at A = 100 ...
    Scheme.gotoh(10, -101, -20, -5, "A101"),                            # ... and refused at A = 101
    Scheme.gotoh(0, -1, -1, -1, "edit_distance"),
    Scheme.gotoh(0, -1000, -1500, -500, "limit_1_or_2"),                # GLOBAL / SEMI_GLOBAL limit 2 at band 3, 1 at band 5
    Scheme.gotoh(0, -300, -400, -200, "limit_small"),                   # 16 / 10 / 2 at bands 3 / 15 / 31
    Scheme.gotoh(0, 0, -4, -1, "match0_mismatch0"),                     # LOCAL: per-row step from G_e alone, A16P takes every length above
    Scheme.gotoh(0, -5, -8, -3, "zero_match"),                          # LOCAL match 0: A16P has no limit
    Scheme.gotoh(2, -1, -2, -1, "bench"),
    Scheme.gotoh(1, -900, -700, -600, "infimum_crossing"),
    Scheme.sw(2, -1, -3, -1, "sw_asym"),                                # SW, deletion != insertion (A16X)
    Scheme.sw(1, -3, -2, -4, "sw_asym2"),
    Scheme.sw(5, -40, -60, -30, "sw_asym_mid"),                          # A16X's GLOBAL / SEMI_GLOBAL limits below 2 000: 245 / 233 / 217
    Scheme.qual(2, -8, -3, -8, -3, nvbowtie_lut(), "nvbowtie_local"),
    Scheme.qual(0, -8, -3, -8, -3, nvbowtie_lut(), "nvbowtie_e2e"),
    Scheme.qual(1, -6, -2, -30, -9, _lut(-4, q30=3, q31=-2), "lut_above_match"),        # a LUT entry above match; text gaps != pattern gaps
    Scheme.qual(0, -5, -3, -9, -4, _lut(-3, q255=-60), "lut_min_at_255"),               # the most negative entry only at quality 255
    Scheme.qual(3, -2, -1, -11, -7, _lut(-5, q7=-1, q200=6), "gaps_differ"),             # text gaps cost more than pattern gaps; entry 6 > match
    Scheme.qual(0, -5, -3, -5, -3, _lut(-6, q10=4), "positive_lut_e2e"),               # a positive LUT entry in SEMI_GLOBAL: cap > match
]


def random_schemes(n=20, seed=20261016):
    """Seeded random schemes: plain Gotoh ones of every cost scale, a few with a positive mismatch or zero gap costs."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        scale = int(rng.choice([4, 16, 64, 256, 1024]))
        m = int(rng.integers(0, scale + 1))
        x = -int(rng.integers(0, scale + 1)) if k % 7 else int(rng.integers(0, m + 2))
        go = -int(rng.integers(0, 2 * scale + 1))
        ge = -int(rng.integers(0, scale + 1))
        out.append(Scheme.gotoh(m, x, go, ge, "rand%02d" % k))
    return out


CORPUS = FIXED_SCHEMES + random_schemes()


def limits_table(bands=(3, 15, 31)):
    """{(scheme name, type, band): (lim16, lim16p)} for the plain-entry limits of every corpus scheme."""
    return {(s.name, ty, b): banded_limits(s, ty, b) for s in CORPUS for ty in TYPES for b in bands}


def probe_lengths(lims, cap=2000):
    """L - 1, L, L + 1 for every finite limit L <= cap (at least 1 symbol)."""
    out = set()
    for L in lims:
        if 0 < L <= cap:
            out.update(v for v in (L - 1, L, L + 1) if v >= 1)
    return sorted(out)
