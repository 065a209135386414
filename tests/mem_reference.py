"""Two independent models of the MEM seeding contract, and the cases the MEM tests share.  Not a test.

(a) brute_mems: straight from the definition, counting occurrences with bytes.find.
(b) bidir_mems: the reference's walk (nvbio/fmindex/mem_inl.h:36-171 over bidir_inl.h:48-87), corrected, over the oracle's FMIndex
    (rank_range, L2, primary): it also returns the SA ranges and the number of right ranges it recorded.
Neither imports the product.
"""
import numpy as np

from oracle import pyoracle as O

NO_MAX = 0xFFFFFFFF
N = 4           # a symbol that matches nothing


# ----------------------------------------------------------------------------------------- (a) the definition
def occurrences(text_b, sub_b, limit=None):
    """start positions of sub in text (overlapping), the first `limit` of them"""
    out, at = [], text_b.find(sub_b)
    while at >= 0 and (limit is None or len(out) < limit):
        out.append(at)
        at = text_b.find(sub_b, at + 1)
    return out


def ell(text_b, pat_b, p, k, at_least=0):
    """ell_k(p): the largest l such that P[p, p+l) holds no symbol > 3 and occurs at least k times; `at_least` is a length already
    known to do so (a substring of an occurring string occurs at least as often)"""
    ln = at_least
    while p + ln < len(pat_b) and pat_b[p + ln] <= 3 and len(occurrences(text_b, pat_b[p:p + ln + 1], k)) >= k:
        ln += 1
    return ln


def brute_mems(text, pattern, min_intv=1, max_intv=NO_MAX, min_span=1):
    """[(begin, end, sorted occurrence positions)] of the reported k-SMEMs, begin ascending"""
    text_b, pat_b = bytes(bytearray(text)), bytes(bytearray(pattern))
    out, prev = [], 0
    for p in range(len(pat_b)):
        ln = ell(text_b, pat_b, p, min_intv, max(prev - 1, 0))
        if ln >= 1 and (p == 0 or p + ln > p - 1 + prev):
            occ = occurrences(text_b, pat_b[p:p + ln])
            if ln >= min_span and len(occ) <= max_intv:
                out.append((p, p + ln, occ))
        prev = ln
    return out


# ----------------------------------------------------------------------------------------- (b) the corrected walk
def _step(index, rng, c):
    """(the range of cS in `index` from the range of S, the rows of S that sort before Sc in the other index)"""
    x, y = rng
    before = 1 if x <= index.primary <= y else 0          # the row of the suffix that is exactly S: the term the reference lacks
    for d in range(c):
        lo, hi = index.rank_range([(x - 1) & 0xFFFFFFFF, y], [d])[0]
        before += int(hi) - int(lo)
    lo, hi = index.rank_range([(x - 1) & 0xFFFFFFFF, y], [c])[0]
    return (int(index.L2[c]) + int(lo) + 1, int(index.L2[c]) + int(hi)), before


def extend_forward(f, r, f_range, r_range, c):
    r_new, x = _step(r, r_range, c)
    size = r_new[1] - r_new[0] + 1
    return (f_range[0] + x, f_range[0] + x + size - 1), r_new


def extend_backwards(f, r, f_range, r_range, c):
    f_new, x = _step(f, f_range, c)
    size = f_new[1] - f_new[0] + 1
    return f_new, (r_range[0] + x, r_range[0] + x + size - 1)


def bidir_mems(f, r, pattern, min_intv=1, max_intv=NO_MAX, min_span=1):
    """([(begin, end, sa_begin, sa_end)], number of right ranges recorded)"""
    pat = [int(c) for c in pattern]
    out, recorded, x = [], 0, 0
    while x < len(pat):
        right = []                      # (f range, end)
        f_range, r_range = (0, f.length), (0, r.length)
        i = x
        while i < len(pat) and pat[i] <= 3:
            nf, nr = extend_forward(f, r, f_range, r_range, pat[i])
            if nf[1] - nf[0] + 1 < min_intv:
                break
            if i > x and nf[1] - nf[0] != f_range[1] - f_range[0]:
                right.append((f_range, i))
            f_range, r_range = nf, nr
            i += 1
        if i > x:
            right.append((f_range, i))          # also when no earlier range was recorded (the reference drops this one)
        recorded += len(right)
        group, leftmost = [], x + 1
        for rng, end in reversed(right):        # from the longest down, as the reference does
            l = x - 1
            while l >= 0 and pat[l] <= 3:
                lo, hi = f.rank_range([(rng[0] - 1) & 0xFFFFFFFF, rng[1]], [pat[l]])[0]
                nxt = (int(f.L2[pat[l]]) + int(lo) + 1, int(f.L2[pat[l]]) + int(hi))
                if nxt[1] - nxt[0] + 1 < min_intv:
                    break
                rng, l = nxt, l - 1
            if l + 1 < leftmost:                # not inside a longer one (min_span does not enter: it filters, it does not define)
                leftmost = l + 1
                group.append((l + 1, end, rng[0], rng[1]))
        out += [g for g in reversed(group) if g[1] - g[0] >= min_span and g[3] - g[2] + 1 <= max_intv]
        x = max(right[-1][1], x + 1) if right else x + 1
    return out, recorded


# ----------------------------------------------------------------------------------------- shared cases
RUN = {77: 0, 1003: 200, 20000: 300}            # length of the run of symbol 0 planted in each text
PARAMS = [(1, NO_MAX, 1), (2, NO_MAX, 1), (3, NO_MAX, 19), (1, 1, 1), (1, 5, 1), (1, NO_MAX, 19)]      # (min_intv, max_intv, min_span)
_cache = {}


def text_of(n):
    """the test text of n symbols: random; the 77-symbol one never holds symbol 3; the longer ones hold a run of symbol 0"""
    rng = np.random.default_rng(1000 + n)
    t = rng.integers(0, 3 if n == 77 else 4, n, dtype=np.uint8)
    if RUN[n]:
        at = n // 3
        t[at:at + RUN[n]] = 0
        t[at - 1] = 1; t[at + RUN[n]] = 2
    return t


def indices_of(n):
    """(text, forward oracle index, oracle index of the reversed text), built once"""
    if ("idx", n) not in _cache:
        t = text_of(n)
        _cache[("idx", n)] = (t, O.FMIndex(t, sa_int=4), O.FMIndex(np.ascontiguousarray(t[::-1]), sa_int=4))
    return _cache[("idx", n)]


def patterns_of(n, with_n=True):
    """the patterns of the contract's case list for the text of n symbols; with_n = False leaves out those that need a symbol > 3
    (a 2-bit string cannot hold one)"""
    t = text_of(n)
    rng = np.random.default_rng(77 + n)

    def piece(ln):
        at = int(rng.integers(0, max(n - ln, 1)))
        return t[at:at + ln].copy()

    def read(ln):           # pieces of the text joined, with a substitution now and then
        s = np.concatenate([piece(min(int(rng.integers(5, 60)), n)) for _ in range(ln // 5 + 1)])[:ln]
        for at in rng.integers(0, ln, ln // 40):
            s[at] = (s[at] + 1) & 3
        return s

    pats = [read(ln) for ln in (1, 2, 19, 150, 256, 300)]
    pats += [np.array([3] * 5, np.uint8) if n == 77 else rng.integers(0, 4, 40, dtype=np.uint8)]      # occurs nowhere (as a whole)
    pats += [t[-30:].copy(), t[:30].copy()]                     # the primary rows of both indices
    pats += [np.array([int(t[5])], np.uint8)]                   # an extension that never changes size: the reference drops it
    if n == 77:
        pats += [t.copy(), np.concatenate([t[40:], t[:20]])]
    if RUN[n]:
        run = min(RUN[n] // 2, 150)
        pats += [np.zeros(run, np.uint8),
                 np.concatenate([np.zeros(100, np.uint8), [1], np.zeros(155, np.uint8)]).astype(np.uint8)]
        pats += [np.concatenate([piece(20), np.zeros(RUN[n] + 5, np.uint8)])[:300]]       # begins past 255 cannot occur here, but the run overshoots
        pats += [np.concatenate([read(270), piece(30)])]                                 # a match whose begin is past 255
    if with_n:
        a, b, c = piece(30), piece(25), piece(10)
        pats += [np.concatenate([[N], a]).astype(np.uint8), np.concatenate([a, [N]]).astype(np.uint8),
                 np.concatenate([c, [N], b, [N], c]).astype(np.uint8), np.array([int(t[7]), N], np.uint8), np.array([N, N, N], np.uint8)]
    return [np.ascontiguousarray(p, dtype=np.uint8) for p in pats]


def expected(n, params, with_n=True):
    """per pattern, model (a)'s [(begin, end, occurrences)] -- computed once per (text, parameters)"""
    key = ("exp", n, params, with_n)
    if key not in _cache:
        t = text_of(n)
        _cache[key] = [brute_mems(t, p, *params) for p in patterns_of(n, with_n)]
    return _cache[key]
