"""The byte-alphabet entries on the device: suffix sort and BWT of a byte text, the wavelet tree and the FM-index over it, through the
Python layer, against the definitions in plain numpy (tests/wavelet_reference.py) -- the checks of tests/test_wavelet_host.py again,
and the device results against the host twins' byte for byte."""
import numpy as np
import pytest
import torch

import nvbio_amd as nvb
from tests import wavelet_cases as WC
from tests.wavelet_checks import (u32, u8, check_tree, check_known_ranks, check_fm, check_fm_against_oracle, check_protein_example,
                                  tree_expectation, rank_queries)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case_id", [c.id for c in WC.tree_cases()])
def test_tree(case_id):
    check_tree(case_id, "cuda")


def test_known_ranks_of_the_reference():
    check_known_ranks("cuda")


@pytest.mark.parametrize("lanes", [1, 2, 4])
@pytest.mark.parametrize("case_id", ["s5_n33", "s8_two_values", "s8_n20011", "s4_n300007"])
def test_rank_and_text_with_every_count_of_queries_per_lane(case_id, lanes):
    """NVBIO_HIP_WAVELET_LANES = 1, 2, 4: the rank and text kernels with that many queries a lane give the host twin's bytes"""
    case = tree_expectation(case_id)[0]
    host = nvb.WaveletTree.build(case.text, case.S, device="cpu")
    p, c = rank_queries(case)
    pos = np.concatenate((np.arange(case.text.size)[::-3], [case.text.size, 0xFFFFFFFF])).astype(np.uint32)
    with nvb.test_switch("NVBIO_HIP_WAVELET_LANES", lanes):
        tree = nvb.WaveletTree.build(case.text, case.S, device="cuda")
        assert (u32(tree.rank(p, c)) == u32(host.rank(p, c))).all()
        assert nvb.lib().nvbio_hip_last_kernel() == b"wavelet_rank_kernel"
        assert (u8(tree.text()) == u8(host.text())).all() and (u8(tree.text(pos)) == u8(host.text(pos))).all()


@pytest.mark.parametrize("case_id", [c.id for c in WC.fm_cases()])
def test_fm_index(case_id):
    fmi, ranges, patterns = check_fm(case_id, "cuda")
    case = {c.id: c for c in WC.fm_cases()}[case_id]
    host = nvb.WaveletFMIndex.build(case.text, case.S, fmi.sa_int, device="cpu")
    assert (ranges == u32(host.match(patterns))).all()            # the failed searches too: the same (x, y) with x > y


def test_fm_index_equals_the_2bit_oracle():
    check_fm_against_oracle("cuda")


def test_protein_example():
    check_protein_example("cuda")


def test_setup_is_ordered_on_the_callers_stream():
    """setup does not wait: queries queued behind it on the same side stream see the finished tree"""
    case, bits, splits, occ, counts = tree_expectation("s4_n300007")
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        tree = nvb.WaveletTree.build(torch.from_numpy(case.text).cuda(), case.S)
        got = tree.text()
    stream.synchronize()
    assert (u8(got) == (case.text & 15)).all() and (u32(tree.bits) == bits).all() and (u32(tree.occ) == occ).all()
