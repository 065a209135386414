"""The checks the host and the GPU wavelet tests share: every one takes the device ("cpu" runs the library's host twins) and compares the
Python layer's answers byte for byte with tests/wavelet_reference.py."""
import functools

import numpy as np

import nvbio_amd as nvb
from nvbio_amd import sufsort
from tests import wavelet_cases as WC
from tests import wavelet_reference as R

SA_INTS = (1, 4, 16, 64)


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def u8(t):
    return t.cpu().numpy().view(np.uint8)


@functools.lru_cache(maxsize=None)
def tree_expectation(case_id):
    case = {c.id: c for c in WC.tree_cases()}[case_id]
    bits, splits, occ = R.tree_arrays(case.text, case.S)
    for a in (bits, splits, occ):
        a.setflags(write=False)
    counts = R.prefix_counts(case.text, case.S)
    counts.setflags(write=False)
    return case, bits, splits, occ, counts


def rank_queries(case, seed=3):
    """(positions, symbols): every pair for n <= 100, else 20 000 random pairs that include absent symbols; then the edges"""
    n, K = case.text.size, 1 << case.S
    r = np.random.default_rng(seed)
    if n <= 100:
        p, c = np.meshgrid(np.arange(n, dtype=np.uint32), np.arange(K, dtype=np.uint32), indexing="ij")
        p, c = p.reshape(-1), c.reshape(-1)
    else:
        p = r.integers(0, n, 20000).astype(np.uint32)
        c = r.integers(0, K, 20000).astype(np.uint32)                 # uniform over the alphabet: absent symbols included
    edge_p = np.array([0xFFFFFFFF, n - 1, n, n + 5, 0xFFFFFFFE], dtype=np.uint32)
    edge_c = np.unique(np.concatenate((R.mask(case.text, case.S)[:3].astype(np.uint32), [0, K - 1, K // 2])))
    ep, ec = np.meshgrid(edge_p, edge_c, indexing="ij")
    return np.concatenate((p, ep.reshape(-1))).astype(np.uint32), np.concatenate((c, ec.reshape(-1))).astype(np.uint8)


def check_tree(case_id, device):
    case, bits, splits, occ, counts = tree_expectation(case_id)
    n, S = case.text.size, case.S
    tree = nvb.WaveletTree.build(case.text, S, device=device)
    assert tree.size == n and tree.symbol_size == S
    assert (u32(tree.bits) == bits).all(), "bits"
    assert (u32(tree.splits) == splits).all(), "splits"
    assert (u32(tree.occ) == occ).all(), "occ"
    # text: the whole text, then explicit positions with some past the end
    assert (u8(tree.text()) == R.mask(case.text, S)).all()
    pos = np.concatenate((np.arange(n)[::-1], [n, n + 5, 0xFFFFFFFF])).astype(np.uint32)
    assert (u8(tree.text(pos)) == R.text_at(case.text, S, pos)).all()
    # rank
    p, c = rank_queries(case)
    assert (u32(tree.rank(p, c)) == R.rank(counts, n, p, c, S)).all()
    # symbols with bits above S set are read masked
    if S < 8:
        high = (c | np.uint8(1 << S)).astype(np.uint8)
        assert (u32(tree.rank(p[:500], high[:500])) == R.rank(counts, n, p[:500], c[:500], S)).all()
    # ranges: (x - 1, y) as the backward search forms them, x = 0 wrapping to 0xFFFFFFFF
    r = np.random.default_rng(11)
    m = 2000 if n > 100 else 200
    x = r.integers(0, n + 1, m).astype(np.uint32)
    x[:m // 4] = 0
    y = r.integers(0, n + 2, m).astype(np.uint32)
    rc = r.integers(0, 1 << S, m).astype(np.uint8)
    ranges = np.stack((x - np.uint32(1), y), axis=1)
    got = u32(tree.rank_range(ranges, rc))
    assert (got[:, 0] == R.rank(counts, n, ranges[:, 0], rc, S)).all() and (got[:, 1] == R.rank(counts, n, ranges[:, 1], rc, S)).all()
    return tree


def check_known_ranks(device):
    case = tree_expectation("known_ranks")[0]
    assert (case.text[:5] == (41, 59, 59, 41, 59)).all() and not (case.text[:6] == 0).any() and case.text.size == 1000
    tree = nvb.WaveletTree.build(case.text, 8, device=device)
    got = u32(tree.rank(np.array(WC.KNOWN_P, dtype=np.uint32), np.array(WC.KNOWN_C, dtype=np.uint8)))
    assert got.tolist() == list(WC.KNOWN_R)


@functools.lru_cache(maxsize=None)
def fm_expectation(case_id):
    case = {c.id: c for c in WC.fm_cases()}[case_id]
    sa = R.suffix_array(case.text, case.S)
    bwt, primary = R.bwt(case.text, case.S, sa)
    patterns = WC.fm_patterns(case)
    rows = [R.match_rows(case.text, case.S, sa, p) for p in patterns]
    sa.setflags(write=False)
    bwt.setflags(write=False)
    return case, sa, bwt, primary, R.L2(case.text, case.S), patterns, rows


def check_fm(case_id, device):
    case, sa, bwt, primary, L2, patterns, rows = fm_expectation(case_id)
    n, S = case.text.size, case.S
    assert (u32(nvb.suffix_sort_bytes(case.text, S, device=device)) == sa).all(), "SA"
    if device != "cpu" and case_id == "repeat13x400":
        assert len(sufsort.last_rounds()) > 1
    fmi = None
    for sa_int in SA_INTS:
        got_bwt, got_primary, got_ssa, got_sa = nvb.bwt_bytes(case.text, S, sa_int, keep_sa=True, device=device)
        assert (u8(got_bwt) == bwt).all() and got_primary == primary, "BWT"
        assert (u32(got_ssa) == R.ssa(sa, sa_int)).all() and (u32(got_sa) == sa).all(), "SSA"
        fmi = nvb.WaveletFMIndex.build(case.text, S, sa_int, device=device)
        assert fmi.primary == primary and fmi.length == n and (u32(fmi.L2) == L2).all(), "L2"
        bits, splits, occ = R.tree_arrays(bwt, S)
        assert (u32(fmi.bwt.bits) == bits).all() and (u32(fmi.bwt.splits) == splits).all() and (u32(fmi.bwt.occ) == occ).all()
        ranges = u32(fmi.match(patterns))
        located = []
        for k, (p, want) in enumerate(zip(patterns, rows)):
            x, y = int(ranges[k, 0]), int(ranges[k, 1])
            if want is None:
                assert x > y, (case_id, k, x, y)
            else:
                assert (x, y) == want, (case_id, k, x, y, want)
                if p.size:
                    located.append(np.arange(x, y + 1, dtype=np.uint32))
        # a symbol >= K ends the search with exactly (1, 0), whatever follows it
        if (1 << S) < 256:
            bad = np.array([1 << S], dtype=np.uint8)
            assert u32(fmi.match([bad, np.concatenate((case.text[:3] & np.uint8((1 << S) - 1), bad))])).tolist() == [[1, 0], [1, 0]]
        assert u32(fmi.match([np.zeros(0, dtype=np.uint8)])).tolist() == [[0, n]]
        all_rows = np.concatenate(located + [np.array([0, primary, n, n + 1, 0xFFFFFFFF], dtype=np.uint32)])[-5000:]
        want_pos = np.where(all_rows <= n, sa[np.minimum(all_rows, n)], 0xFFFFFFFF).astype(np.uint32)
        want_pos[all_rows == 0] = 0xFFFFFFFF                          # row 0: what nvbio_hip_fm_locate gives for it, ssa[0]
        assert (u32(fmi.locate(all_rows)) == want_pos).all(), "locate"
    return fmi, ranges, patterns


def check_fm_against_oracle(device):
    """the i.i.d. 4-symbol text, indexed at S = 8 and at S = 2: ranges and located positions equal the 2-bit FM-index oracle's"""
    from oracle import pyoracle as O
    for case_id in ("iid4_s8", "iid4_s2"):
        case = fm_expectation(case_id)[0]
        host = O.FMIndex(case.text)
        r = np.random.default_rng(5)
        pats = [case.text[q:q + int(r.integers(1, 12))] for q in r.integers(0, case.text.size - 12, 200)]
        pats += [r.integers(0, 4, 8, dtype=np.uint8) for _ in range(50)]
        want = host.match(O.StringSet.from_lists(pats, 2, True))
        fmi = nvb.WaveletFMIndex.build(case.text, case.S, 16, device=device)
        got = u32(fmi.match(pats))
        found = want[:, 0] <= want[:, 1]
        assert ((got[:, 0] <= got[:, 1]) == found).all() and (got[found] == want[found]).all()
        rows = np.concatenate([np.arange(x, y + 1, dtype=np.uint32) for x, y in want[found]])[:5000]
        assert (u32(fmi.locate(rows)) == host.locate(rows)).all()


def check_protein_example(device):
    """the reference's examples/waveletfm: every suffix of the 24-letter text matches exactly once, at its own row"""
    case, sa, bwt, primary, L2, _, _ = fm_expectation("protein24")
    fmi = nvb.WaveletFMIndex.build(case.text, 8, 4, device=device)
    assert nvb.alphabet.decode(u8(fmi.bwt.text())) == nvb.alphabet.decode(bwt)
    suffixes = [case.text[i:] for i in range(case.text.size)]
    ranges = u32(fmi.match(suffixes))
    assert (ranges[:, 0] == ranges[:, 1]).all()
    assert (u32(fmi.locate(ranges[:, 0])) == np.arange(case.text.size)).all()
