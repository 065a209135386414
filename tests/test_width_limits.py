"""CPU half of the width-limit tests: the scheme corpus and its table of 16-bit limits (tests/width_limits.py), and an independent int64
model of the full-matrix Gotoh score (tests/dp_reference.py) held against the known answers and then against the oracle on the corpus,
at shapes where the reference's int16 boundary column cannot truncate.  The GPU half is tests/test_width_limits_gpu.py."""
import json
import os

import numpy as np
import pytest

import dp_reference as R
import width_limits as W
from oracle import pyoracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
KAT = json.load(open(os.path.join(HERE, "golden", "kat.json")))
G, L, S = W.GLOBAL, W.LOCAL, W.SEMI_GLOBAL
BY_NAME = {s.name: s for s in W.CORPUS}


def dna(s):
    return np.array(["ACGT".index(c) for c in s], dtype=np.uint8)


def test_corpus_costs_stay_inside_the_reference_int32():
    """|cost| <= 2^13 for every corpus scheme, so that no job the tests build can overflow the reference's int32 arithmetic: the
    longest jobs they run (patterns up to 2 001 symbols against texts of up to 2^20 symbols) stay far inside int32, counted in int64."""
    assert len(W.FIXED_SCHEMES) >= 20 and len(W.CORPUS) >= 40
    assert len({s.name for s in W.CORPUS}) == len(W.CORPUS)
    for s in W.CORPUS:
        A = max(abs(int(c)) for c in s.costs())
        assert A <= W.COST_BOUND, s.name
        assert np.int64(2001 + (1 << 20) + 4) * np.int64(A) < np.int64(2 ** 31 - 1), s.name


def test_corpus_holds_the_edge_schemes():
    kinds = {s.kind for s in W.CORPUS}
    assert kinds == {"gotoh", "sw", "qual"}
    assert any(s.costs()[:5] == [0, 0, 0, 0, 0] for s in W.CORPUS)
    assert any(s.match < 0 for s in W.CORPUS)
    assert any(s.go > 0 or s.ge > 0 for s in W.CORPUS)
    assert any(s.ge == 0 and s.go < 0 for s in W.CORPUS) and any(s.go == 0 and s.ge < 0 for s in W.CORPUS)
    assert any(abs(s.ge) > abs(s.go) for s in W.CORPUS)
    quals = [s for s in W.CORPUS if s.kind == "qual"]
    assert any(max(s.lut) > s.match for s in quals)
    assert any(min(s.lut) == s.lut[255] and s.lut.count(min(s.lut)) == 1 for s in quals)
    assert any((s.go, s.ge) != (s.tgo, s.tge) for s in quals)


def test_limits_table_literals():
    """A few entries of the corpus's table of 16-bit limits (lim16 = the row-frame kernel's, lim16p = the A16P instance's), so that a
    reader sees the numbers the GPU module drives jobs to."""
    T = W.limits_table()
    assert T[("mismatch_above_match", L, 15)] == (146, 204)                 # best_pair 5 from the mismatch: 1022 / (5 + 2), 1022 / 5
    assert T[("mid_cost", L, 15)] == (29, 204)                              # 1022 / (5 + 30), 1022 / 5
    assert T[("mid_cost", S, 15)] == (116, 116) and T[("mid_cost", S, 31)] == (108, 108)     # (15000 / 60 - band - 2) / 2
    assert T[("A100", L, 3)] == (9, 102) and T[("A101", L, 3)] == (0, 0)   # LOCAL's A > 100 cut-off
    assert T[("limit_1_or_2", G, 3)] == (2, 2) and T[("limit_1_or_2", G, 15)] == (0, 0)
    assert W.banded_limits(BY_NAME["limit_1_or_2"], S, 5) == (1, 1)
    assert T[("zero", L, 31)] == (W.ALWAYS, W.ALWAYS) and T[("zero", G, 31)] == (W.ALWAYS, W.ALWAYS)
    assert T[("match_negative", L, 15)] == (0, 0) and T[("match_negative", S, 15)] == (2491, 2491)
    assert T[("gap_open_positive", S, 3)] == (0, 0)
    assert T[("zero_match", L, 31)] == (340, W.ALWAYS)                      # match 0: the per-row step of the recurrence as written is 0
    assert T[("bench", L, 15)] == (340, 511) and T[("bench", S, 31)] == (3733, 3733)
    assert T[("nvbowtie_local", L, 15)] == (204, 511) and T[("nvbowtie_e2e", S, 15)] == (929, 929)
    assert T[("lut_above_match", L, 15)] == (204, 340)                      # best_pair 3 from the LUT, not match 1
    assert T[("gaps_differ", L, 15)] == (146, 170)                          # the row frame's step is the pattern's G_e only
    # the entries that are not in the row frame: the bounded scorer and SW with deletion != insertion
    assert W.banded_limits(BY_NAME["nvbowtie_local"], L, 15, "bounded") == (511, 511)
    assert W.banded_limits(BY_NAME["sw_asym"], L, 15, "asym") == (511, 511)
    assert W.banded_limits(BY_NAME["sw_asym"], S, 15, "asym") == (4983, 4983)             # 15000 / 3 - 17, no row step
    assert W.bounded_args(BY_NAME["positive_lut_e2e"]) == (True, 4)
    assert W.bounded_args(BY_NAME["nvbowtie_e2e"]) == (True, 0)


def test_full_matrix_route_literals():
    """The full-matrix gates at the values the GPU module places its announced lengths on."""
    bench, ed = BY_NAME["bench"], BY_NAME["edit_distance"]
    # LOCAL: maxM * best_pair < 2048
    assert W.full_route(bench, L, 1023, 64) == "sweep16" and W.full_route(bench, L, 1024, 64) == "generic"
    # span * A < 30000 (SEMI_GLOBAL: span = maxM + 4)
    s = W.Scheme.gotoh(2, -3, -10, -5, "span")
    assert W.full_route(s, S, 2995, 64) == "striped"
    assert W.full_route(W.Scheme.gotoh(0, -30, -30, -30, "A30"), S, 995, 64) == "sweep16"      # 999 * 30 = 29 970
    assert W.full_route(W.Scheme.gotoh(0, -30, -30, -30, "A30"), S, 996, 64) == "trunc"        # 1000 * 30 = 30 000
    # LOCAL's A * 3 < 2000
    assert W.full_route(W.Scheme.gotoh(0, -666, -10, -10, "A666"), L, 40, 40) == "sweep16"
    assert W.full_route(W.Scheme.gotoh(0, -667, -10, -10, "A667"), L, 40, 40) == "generic"
    # edit distance: the bit-vector kernel up to 512 pattern symbols, the striped sweep beyond 1 024
    assert W.full_route(W.Scheme.sw(0, -1, -1, -1), S, 512, 600) == "ed" and W.full_route(W.Scheme.sw(0, -1, -1, -1), S, 513, 600) == "sweep16"
    assert W.full_route(W.Scheme.sw(0, -1, -1, -1), S, 1025, 1100) == "striped"
    # the 32-bit order keys refuse before anything runs
    assert W.full_route(ed, S, 100, (1 << 32) // (64 * 8)) == "refused" and W.full_route(ed, S, 100, (1 << 32) // (64 * 8) - 1) != "refused"
    assert W.full_route(ed, S, 600, (1 << 32) // (64 * 16)) == "refused"
    # GLOBAL's high: maxM * best_pair, the best pair from a LUT entry above match (100) on the quality entry
    q = W.Scheme.qual(0, -1, -1, -1, -1, np.r_[[-1, 100], np.full(254, -1)], "lut100")
    assert W.global_bounds(q, 318, 318) == (748, 31908) and W.full_route(q, G, 318, 318) == "sweep16"
    assert W.global_bounds(q, 319, 319)[1] == 32008 and W.full_route(q, G, 319, 319) == "refused"
    # tracebacks
    assert W.banded_traceback_ok(bench, 15, 32000 // 2 - 18) and not W.banded_traceback_ok(bench, 15, 32000 // 2 - 17)
    assert W.full_traceback_ok(bench, S, 14995, 64) and not W.full_traceback_ok(bench, S, 14996, 64)            # (M + 4) * 2 < 30000
    assert W.wave_lut_ok([-32768, 32767] * 128) and not W.wave_lut_ok([-32769] + [0] * 255) and not W.wave_lut_ok([32768] + [0] * 255)


def test_dp_model_against_the_known_answers():
    """The model against the full-matrix literals of the reference's functional test (alignment_test.cu:788-792, re-scored CIGARs:
    GLOBAL 1M2D3M1D3M10D = 14 - 2 - 1 - 10, LOCAL and SEMI_GLOBAL 4M1D3M = 14 - 1) and the kat.json cases on real_p / real_t: the full
    matrix scores at least what a band reports, and exactly that for the band-31 ones, whose window holds the best path."""
    p, t = dna(KAT["strings"]["short_p"]), dna(KAT["strings"]["short_t"])
    sc = (2, -1, -1, -1)
    for ty, cigar_score in ((G, 1 * 2 + 3 * 2 - 1 + 3 * 2 - 1 - 1 - 1 - 9), (L, 4 * 2 - 1 + 3 * 2), (S, 4 * 2 - 1 + 3 * 2)):
        got = int(R.gotoh_score(ty, *sc[:1], sc[2], sc[3], sc[2], sc[3], p[None], t[None], np.full((1, p.size), sc[1]))[0])
        assert got == cigar_score == O.ref_sw_gotoh(ty, sc, p, t), (ty, got, cigar_score)
    for case in KAT["gotoh"]:
        if case["p"] != "real_p" or case["type"] == G:
            continue
        p, t = dna(KAT["strings"][case["p"]]), dna(KAT["strings"][case["t"]])
        m, x, go, ge = case["scheme"]
        got = int(R.gotoh_score(case["type"], m, go, ge, go, ge, p[None], t[None], np.full((1, p.size), x))[0])
        full = int(O.batch_gotoh_score(case["type"], case["scheme"], O.StringSet.from_lists([p], 4, True), O.StringSet.from_lists([t], 2, False))[0][0])
        assert got == full >= case["score"], case
        if case["band"] == 31:
            assert got == case["score"], case


def _jobs(rng, B, M, N):
    """B jobs of one shape, each kind a probe of some extreme: a perfect match (the best-pair score), an all-mismatch pattern (the
    complement of its text), a pattern of N symbols, long gaps either way, and random pairs."""
    t = rng.integers(0, 4, (B, N)).astype(np.int64)
    p = rng.integers(0, 4, (B, M)).astype(np.int64)
    for b in range(B):
        kind = b % 6
        off = int(rng.integers(0, max(1, N - M + 1)))
        src = np.resize(t[b, off:], M) if N > off else p[b]
        if kind == 0:
            p[b] = src
        elif kind == 1:
            p[b] = 3 - np.resize(t[b], M)
        elif kind == 2:
            p[b] = 4
        elif kind == 3 and M > 6:
            cut = int(rng.integers(1, M - 3))
            p[b] = np.concatenate([src[:cut], src[cut + 3:], [0, 1, 2]])[:M]
        elif kind == 4 and M > 6:
            cut = int(rng.integers(1, M - 3))
            p[b] = np.concatenate([src[:cut], [3, 3, 3], src[cut:]])[:M]
    return p, t


def _shapes(s, ty):
    """Two shapes per scheme and type where the route mirror says the reference's int16 column cannot truncate (not "trunc"), the
    larger one as close to the span * A < 30000 gate as the CPU budget allows."""
    out = []
    for M, N in ((40, 52), (24, 30), (12, 15), (6, 8), (2, 3)):
        if len(out) == 2:
            break
        if W.full_route(s, ty, M, N) in ("sweep16", "generic", "ed"):
            out.append((M, N))
    return out


@pytest.mark.parametrize("ty", [G, L, S])
def test_dp_model_against_the_oracle_on_the_corpus(ty):
    """The int64 model and the oracle's full-matrix score (plain scheme: O.batch_gotoh_score; quality scheme: batch_gotoh_score_qual, text
    blocking) agree on every corpus scheme (SW schemes are the plain form with equal gap costs), on perfect, all-mismatch, all-N, gapped
    and random jobs, where no int16 column can truncate."""
    rng = np.random.default_rng(4100 + ty)
    checked = 0
    for s in W.CORPUS:
        if s.kind == "sw":
            continue
        for M, N in _shapes(s, ty):
            B = 48
            p, t = _jobs(rng, B, M, N)
            hp = O.StringSet.from_lists(list(p.astype(np.uint8)), 4, True)
            ht = O.StringSet.from_lists(list(t.astype(np.uint8)), 2, False)
            if s.kind == "qual":
                quals = rng.integers(0, 256, B * M + 3).astype(np.uint8)
                quals[: B * M : 7] = 255
                lut = s.lut_array()
                es, _, ok = O.batch_gotoh_score_qual(1, ty, (s.match, s.go, s.ge, s.tgo, s.tge), lut, quals, hp, ht, n_threads=16)
                mm = lut[quals[: B * M].reshape(B, M)]
            else:
                es, _, ok = O.batch_gotoh_score(ty, (s.match, s.mismatch, s.go, s.ge), hp, ht, n_threads=16)
                mm = np.full((B, M), s.mismatch)
            got = R.gotoh_score(ty, s.match, s.go, s.ge, s.tgo, s.tge, p, t, mm)
            bad = np.nonzero(got != es.astype(np.int64))[0]
            assert bad.size == 0, (s.name, ty, M, N, bad[:4], got[bad[:4]], es[bad[:4]])
            if ty != G and s.match > 0 and s.match >= max(s.lut_array()):
                assert got[0] == M * s.match                                # the perfect job reaches M * best_pair
            checked += 1
    assert checked >= 60
