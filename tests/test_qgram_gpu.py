"""The device q-gram entries (nvbio_amd/csrc/qgram.hip through nvbio_amd.qgram) against the definitions in plain numpy
(tests/qgram_reference.py) and against the host twins, byte for byte: the cases of tests/test_qgram_host.py again on the GPU, and one
medium case that crosses block and rocPRIM-tile boundaries.  Every order is total, so every comparison is exact."""
import numpy as np
import pytest
import torch

import nvbio_amd as nvb
from tests import qgram_cases as QC
from tests import qgram_reference as R
from tests import qgram_checks as H

pytestmark = pytest.mark.gpu


def last_kernel():
    return nvb.lib().nvbio_hip_last_kernel().decode()


def assert_same_index(a, b):
    """a device index and its host twin: the same bytes"""
    for x, y in zip(H.index_arrays(a), H.index_arrays(b)):
        assert (x is None) == (y is None)
        if x is not None:
            assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("big_endian", [True, False], ids=["be", "le"])
@pytest.mark.parametrize("q", QC.QS)
def test_string_index_and_generate(cuda, q, big_endian):
    built = H.check_string_builds(q, big_endian, cuda)
    assert last_kernel() == "qgram_lut_kernel"
    for (name, ql), (ix, e) in built.items():
        sym = dict(QC.strings(q))[name]
        assert_same_index(ix, nvb.QGramIndex.build(H.packed(sym, big_endian, "cpu"), q, ql, device="cpu"))


@pytest.mark.parametrize("big_endian", [True, False], ids=["be", "le"])
@pytest.mark.parametrize("q", QC.QS)
def test_set_index_and_generate(cuda, q, big_endian):
    built = H.check_set_builds(q, big_endian, cuda)
    cases = {case.id: case for case in QC.sets()}
    for (name, interval, ql), (ix, e) in built.items():
        assert_same_index(ix, nvb.QGramSetIndex.build(H.packed_set(cases[name], big_endian, "cpu"), q, interval, ql, device="cpu"))


@pytest.mark.parametrize("q", QC.QS)
def test_string_queries_and_filter(cuda, q):
    for (ix, e, queries), (hx, _, _) in zip(H.string_filter_cases(q, q % 2 == 0, cuda), H.string_filter_cases(q, q % 2 == 0, "cpu")):
        H.check_queries(ix, e, queries, cuda)
        hits = H.check_filter(ix, e, queries, cuda)
        assert H.u32(hits).tobytes() == H.u32(H.check_filter(hx, e, queries, "cpu")).tobytes()


@pytest.mark.parametrize("q", QC.QS)
def test_set_queries_and_filter(cuda, q):
    for (ix, e, queries), (hx, _, _) in zip(H.set_filter_cases(q, q % 2 == 1, cuda), H.set_filter_cases(q, q % 2 == 1, "cpu")):
        H.check_queries(ix, e, queries, cuda)
        hits = H.check_filter(ix, e, queries, cuda)
        assert H.u32(hits).tobytes() == H.u32(H.check_filter(hx, e, queries, "cpu")).tobytes()


def test_merge_edges(cuda):
    H.check_merge_edges(cuda)
    assert last_kernel() == "qgram_set_diagonals_kernel"                 # the merge before the empty one, which launches nothing


def test_zero_queries_rank_is_zero(cuda):
    ix = nvb.QGramIndex.build(torch.arange(40, device=cuda) % 4, 5, 1)
    f = nvb.QGramFilter()
    assert f.rank(ix, np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint32)) == 0
    assert f.locate(0, 0).shape == (0, 2)


@pytest.fixture(scope="module")
def medium():
    """the medium inputs and their reference, computed once: a 100 000-symbol text with 10 % planted repeats, 2 000 reads of 50 to 150
    symbols, 50 000 query q-grams (three in four from the reads, the rest random words)"""
    q = 20
    text = QC.medium_text()
    reads = QC.medium_reads(text)
    rng = np.random.default_rng(99)
    ids = rng.integers(0, len(reads), 37500)
    coords = np.stack([ids, [rng.integers(0, len(reads[i]) - q + 1) for i in ids]], axis=1).astype(np.uint32)
    queries = np.concatenate([R.set_qgrams_at(reads, coords, q), rng.integers(0, 1 << 40, 12500, dtype=np.uint64)])
    queries = queries[rng.permutation(queries.size)]
    indices = rng.integers(0, 100000, queries.size).astype(np.uint32)
    return dict(q=q, text=text, reads=reads, coords=coords, queries=queries, indices=indices,
                string=R.string_index(text, q, 6), set=R.set_index(reads, q, 10, 6))


def run_filter(ix, e, m, locate_kernel, merge_kernel):
    f = nvb.QGramFilter()
    total = f.rank(ix, m["queries"], m["indices"])
    assert last_kernel() == "qgram_range_kernel"
    ranges, slots, etotal = R.rank(e, m["queries"])
    assert total == etotal and total > 50000
    assert (H.u32(f.ranges) == ranges).all() and (H.u64(f.slots) == slots).all()
    expect = R.locate(e, ranges, slots, m["indices"], 0, total)
    cuts = [0, 1023, total // 2 + 517, total]                            # three uneven batches, none on a block border
    parts = [f.locate(a, b) for a, b in zip(cuts[:-1], cuts[1:])]
    assert last_kernel() == locate_kernel
    hits = torch.cat(parts)
    assert (H.u32(hits) == expect).all()
    for interval in (1, 10, 16):
        merged, counts = f.merge(interval, hits)
        assert last_kernel() == merge_kernel
        em, ec = R.merge(expect, interval)
        assert H.u32(merged).shape == em.shape and (H.u32(merged) == em).all() and (H.u32(counts) == ec).all()


def test_medium_string_index_and_filter(cuda, medium):
    m = medium
    text = torch.from_numpy(m["text"]).to(cuda)
    assert (H.u64(nvb.generate_qgrams(text, m["q"])) == R.qgrams_at(m["text"], np.arange(len(m["text"])), m["q"])).all()
    assert last_kernel() == "qgram_generate_kernel"
    where = m["indices"][:5000]
    assert (H.u64(nvb.generate_qgrams(text, m["q"], where)) == R.qgrams_at(m["text"], where, m["q"])).all()
    assert last_kernel() == "qgram_generate_coords_kernel"
    ix = nvb.QGramIndex.build(text, m["q"], 6)
    assert last_kernel() == "qgram_lut_kernel"
    H.assert_index(ix, m["string"])
    assert (H.u32(ix.range(m["queries"])) == m["string"].ranges(m["queries"])).all()
    assert last_kernel() == "qgram_range_kernel"
    run_filter(ix, m["string"], m, "qgram_locate_kernel", "qgram_diagonals_kernel")


def test_medium_set_index_and_filter(cuda, medium):
    m = medium
    reads = [torch.from_numpy(t).to(cuda) for t in m["reads"]]
    assert (H.u64(nvb.generate_qgrams(reads, m["q"], m["coords"])) == R.set_qgrams_at(m["reads"], m["coords"], m["q"])).all()
    assert last_kernel() == "qgram_generate_coords_kernel"
    ix = nvb.QGramSetIndex.build(reads, m["q"], 10, 6)
    assert last_kernel() == "qgram_lut_kernel"
    H.assert_index(ix, m["set"])
    assert_same_index(ix, nvb.QGramSetIndex.build(m["reads"], m["q"], 10, 6, device="cpu"))
    dense = nvb.QGramSetIndex.build(reads, m["q"], 1, 6)                  # every position of every read: about 160 000 q-grams
    e = R.set_index(m["reads"], m["q"], 1, 6)
    H.assert_index(dense, e)
    run_filter(dense, e, m, "qgram_set_locate_kernel", "qgram_set_diagonals_kernel")
