"""Two independent models of MEM re-seeding (split_len / split_width) over those of tests/mem_reference.py, and
the parameter grid the re-seeding tests share.  Not a test; does not import the product.

For a string P and (min_intv, max_intv, min_span, split_len, split_width): B = the reported MEMs; a MEM [b, e) of B with
e - b >= split_len and occ <= split_width occurrences is a candidate; its re-seeds are the (occ + 1)-SMEMs of P that cover
m = (b + e) >> 1 and pass min_span and max_intv; the output is B and all re-seeds, every span once, ordered by begin, then end.

(a) split_brute: the definition -- brute_mems for B, brute_mems at occ + 1 filtered to the spans over m for the re-seeds.
(b) split_bidir: the corrected walk over the oracle's FMIndex -- one group of bidir_mems from x = m at occ + 1.
"""
from tests import mem_reference as M

NO_MAX = M.NO_MAX
TEXTS = tuple(M.RUN)                                                                # 77, 1003, 20000
PARAMS = [(1, NO_MAX, 1), (2, NO_MAX, 1), (1, 5, 1), (1, NO_MAX, 19)]               # (min_intv, max_intv, min_span)
SPLITS = [(8, 3), (28, 10), (12, 1), (1, NO_MAX), (NO_MAX, NO_MAX)]                 # (split_len, split_width)
_cache = {}


def cells(n_text):
    """the grid cells run on the text of n_text symbols: the brute model needs about 23 s for one cell on the longest text"""
    return [(p, s) for p in PARAMS for s in SPLITS if not (n_text == 20000 and p == (2, NO_MAX, 1) and s == (1, NO_MAX))]


def is_candidate(b, e, occ, split):
    return e - b >= split[0] and occ <= split[1]


# ----------------------------------------------------------------------------------------- (a) the definition
def split_brute(text, pattern, params, split, stats=None, memo=None):
    """[(begin, end, sorted occurrence positions)], begin then end ascending.  stats, a dict, gains the counts of candidates,
    added spans, duplicates removed and candidates with no surviving re-seed; memo, a dict of this (text, pattern), keeps the
    reported k-SMEMs of the whole pattern per (k, max_intv, min_span) across calls"""
    memo = {} if memo is None else memo

    def smems(k):
        key = (k, params[1], params[2])
        if key not in memo:
            memo[key] = M.brute_mems(text, pattern, *key)
        return memo[key]

    base = smems(params[0])
    spans = {(b, e): occ for b, e, occ in base}
    for b, e, occ in base:
        if split[0] == NO_MAX or not is_candidate(b, e, len(occ), split):
            continue
        m = (b + e) >> 1
        reseeds = [s for s in smems(len(occ) + 1) if s[0] <= m < s[1]]
        if stats is not None:
            stats["candidates"] = stats.get("candidates", 0) + 1
            stats["empty"] = stats.get("empty", 0) + (0 if reseeds else 1)
        for rb, re_, rocc in reseeds:
            if (rb, re_) in spans:
                if stats is not None:
                    stats["duplicates"] = stats.get("duplicates", 0) + 1
            else:
                spans[(rb, re_)] = rocc
                if stats is not None:
                    stats["added"] = stats.get("added", 0) + 1
    return [(b, e, spans[(b, e)]) for b, e in sorted(spans)]


# ----------------------------------------------------------------------------------------- (b) the corrected walk
def _group(f, r, pat, x, k, max_intv, min_span):
    """the k-SMEMs that cover symbol x, as bidir_mems finds one group: [(begin, end, sa_begin, sa_end)]"""
    right, f_range, r_range, i = [], (0, f.length), (0, r.length), x
    while i < len(pat) and pat[i] <= 3:
        nf, nr = M.extend_forward(f, r, f_range, r_range, pat[i])
        if nf[1] - nf[0] + 1 < k:
            break
        if i > x and nf[1] - nf[0] != f_range[1] - f_range[0]:
            right.append((f_range, i))
        f_range, r_range = nf, nr
        i += 1
    if i > x:
        right.append((f_range, i))
    group, leftmost = [], x + 1
    for rng, end in reversed(right):
        l = x - 1
        while l >= 0 and pat[l] <= 3:
            lo, hi = f.rank_range([(rng[0] - 1) & 0xFFFFFFFF, rng[1]], [pat[l]])[0]
            nxt = (int(f.L2[pat[l]]) + int(lo) + 1, int(f.L2[pat[l]]) + int(hi))
            if nxt[1] - nxt[0] + 1 < k:
                break
            rng, l = nxt, l - 1
        if l + 1 < leftmost:
            leftmost = l + 1
            group.append((l + 1, end, rng[0], rng[1]))
    return [g for g in group if g[1] - g[0] >= min_span and g[3] - g[2] + 1 <= max_intv]


def split_bidir(f, r, pattern, params, split):
    """[(begin, end, sa_begin, sa_end)], begin then end ascending"""
    pat = [int(c) for c in pattern]
    walks = _cache.setdefault(("walks", f.length, bytes(bytearray(pat))), {})        # the walks of this (text, pattern), shared by the grid's cells
    if ("base", params) not in walks:
        walks[("base", params)] = M.bidir_mems(f, r, pattern, *params)[0]
    base = walks[("base", params)]
    spans = {(b, e): (lo, hi) for b, e, lo, hi in base}
    for b, e, lo, hi in base:
        occ = hi - lo + 1
        if split[0] == NO_MAX or not is_candidate(b, e, occ, split):
            continue
        key = ((b + e) >> 1, occ + 1, params[1], params[2])
        if key not in walks:
            walks[key] = _group(f, r, pat, *key)
        for rb, re_, rlo, rhi in walks[key]:
            assert spans.setdefault((rb, re_), (rlo, rhi)) == (rlo, rhi)
    return [(b, e) + spans[(b, e)] for b, e in sorted(spans)]


# ----------------------------------------------------------------------------------------- shared, computed once
def expected(n_text, params, split, with_n=True):
    """(per pattern model (a)'s [(begin, end, occurrences)], the cell's stats) -- once per (text, cell)"""
    key = (n_text, params, split, with_n)
    if key not in _cache:
        t, stats = M.text_of(n_text), {"candidates": 0, "added": 0, "duplicates": 0, "empty": 0}
        _cache[key] = ([split_brute(t, p, params, split, stats, _cache.setdefault(("smems", n_text, with_n, i), {}))
                        for i, p in enumerate(M.patterns_of(n_text, with_n))], stats)
    return _cache[key]
