"""--ungapped-mates: the paired drivers' Params.ungapped_mates against the unchanged nvBowtie binary (oracle/_ref/ref_nvBowtie) run with the same
flag, SAM record for SAM record.  The binary is held on the drop-in layer's generic lane (NVBIO_HIP_COMPAT_GENERIC=full), so the records compared
against come from the per-thread priv::hamming_score; one case is repeated with the binary on its default route, where its opposite-mate batches
reach the tuned kernel.  The C++ paired driver must equal the Python one slot for slot."""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import nvbio_amd as nvb
from nvbio_amd import aligner as A, pipeline as P, select as S, workloads as W
from oracle import pyoracle as O

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.path.join(ROOT, "oracle", "_ref")

CASES = [dict(extra="--ungapped-mates", own="ungapped_mates=True", seed=101, reads=4000),
         dict(extra="--local --ungapped-mates", own="local=True,ungapped_mates=True", seed=102, reads=3000),
         dict(extra="--scoring ed --ungapped-mates", own="scoring_mode=ed,ungapped_mates=True", seed=103, reads=3000)]
IDS = ["end-to-end", "local", "edit-distance"]


def _tool():
    if not os.path.exists(os.path.join(REF, "ref_nvBowtie")):
        pytest.skip("oracle/_ref/ref_nvBowtie not built (needs /root/reference in the build container)")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import nvbowtie_compare
    return nvbowtie_compare


def _args(case, **kw):
    args = dict(mode="paired", reads=3000, seed=5, indels=0.3, pair_indels=True, show=3, len=100, ns=0.0, quals="random", repeats=0.0, extra="", own="")
    args.update(case); args.update(kw)
    return argparse.Namespace(**args)


def _own_records(tool, case, own):
    _, run, buf, _ = tool.prepare(_args(case, own=own))
    run()
    return tool.records(buf.getvalue())


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_ungapped_mates_equal_reference_nvbowtie(case, cuda, monkeypatch):
    """every SAM record identical to the binary's on its generic lane; and the flag does something in Smith-Waterman mode (some pair's records
    differ from the run without it -- 30 % of the mates carry an indel) and nothing in edit-distance mode"""
    tool = _tool()
    monkeypatch.setenv("NVBIO_HIP_COMPAT_GENERIC", "full")
    same, n_ref, n_own = tool.compare(_args(case))
    assert n_ref == n_own and n_ref >= 2 * case["reads"]
    assert same == n_ref, (case, same, n_ref)
    with_flag = _own_records(tool, case, case["own"])
    without = _own_records(tool, case, case["own"].replace(",ungapped_mates=True", "").replace("ungapped_mates=True", ""))
    differing = sum(1 for a, b in zip(with_flag, without) if a != b)
    print("records that differ with / without the flag: %d of %d" % (differing, len(with_flag)))
    assert len(with_flag) == len(without)
    assert (differing == 0) if "scoring_mode=ed" in case["own"] else (differing > 0)


def test_ungapped_mates_equal_reference_nvbowtie_on_its_tuned_route(cuda, monkeypatch):
    """the same binary on its default route: BatchedAlignmentScore sends its HammingDistanceAligner streams to nvbio_hip_hamming_score_qual"""
    tool = _tool()
    monkeypatch.delenv("NVBIO_HIP_COMPAT_GENERIC", raising=False)
    same, n_ref, n_own = tool.compare(_args(CASES[0]))
    assert n_ref == n_own and n_ref >= 2 * CASES[0]["reads"]
    assert same == n_ref, (same, n_ref)


class _ShimParams(C.Structure):
    _fields_ = [(k, C.c_uint32) for k in ("local", "randomized", "top_seed", "max_effort_init", "max_effort", "min_ext", "max_ext", "max_reseed", "rep_seeds",
                                          "max_hits", "allow_sub", "subseed_len", "seed_len", "seed_freq_type", "min_read_len", "max_dist", "no_multi_hits",
                                          "batch_size", "hits_stride")] + \
               [("seed_freq_k", C.c_float), ("seed_freq_m", C.c_float), ("match", C.c_int32), ("score_min_type", C.c_int32),
                ("score_min_k", C.c_float), ("score_min_m", C.c_float), ("finish", C.c_uint32), ("edit_distance", C.c_uint32)]


class _ShimPeParams(C.Structure):
    _fields_ = [("pe_policy", C.c_int32)] + [(k, C.c_uint32) for k in ("pe_overlap", "pe_unpaired", "pe_discordant", "min_frag_len", "max_frag_len")]


def _pairs_with_indels(rng, text, n, L):
    """FR pairs from 200-420 bp fragments, 2 % substitutions, an indel in the middle of 40 % of the second mates"""
    s1 = np.zeros((n, L), np.uint8); s2 = np.zeros((n, L), np.uint8)
    for i in range(n):
        f = int(rng.integers(200, 420)); p = int(rng.integers(0, text.size - f - 8))
        a = text[p:p + L].copy()
        frag_end = text[p + f - L - 4:p + f].copy()
        if rng.random() < 0.4:
            k, g = int(rng.integers(30, 70)), int(rng.integers(1, 3))
            frag_end = np.concatenate([frag_end[:k], frag_end[k + g:]]) if rng.random() < 0.5 else np.concatenate([frag_end[:k], rng.integers(0, 4, g).astype(np.uint8), frag_end[k:]])
        b = (3 - frag_end[-L:])[::-1].copy()
        for m in (a, b):
            flip = rng.random(L) < 0.02
            m[flip] = rng.integers(0, 4, int(flip.sum()))
        s1[i], s2[i] = a, b
    return s1, s2


@pytest.mark.parametrize("mode", ["end-to-end", "local", "edit-distance"])
def test_cxx_paired_driver_with_ungapped_mates_equals_the_python_driver(cuda, mode):
    """Aligner::best_approx over a PairedReadBatch with Params::ungapped_mates (tests/cxx/ungapped_mates_shim.cpp) against
    nvbio_amd.aligner.best_approx_paired with Params.ungapped_mates: both slot sets, both MAPQs, CIGARs and MD strings"""
    shim = C.CDLL(os.path.join(HERE, "cxx", "libungapped_mates_shim.so"))
    rng = np.random.default_rng(987)
    text = rng.integers(0, 4, 1 << 17).astype(np.uint8)
    host, rhost = O.FMIndex(text), O.FMIndex(text[::-1].copy())
    fmi, rfmi = nvb.FMIndexDevice.from_host(host, cuda), nvb.FMIndexDevice.from_host(rhost, cuda)
    n, L = 900, 100
    s1, s2 = _pairs_with_indels(rng, text, n, L)
    names = ["pair.%d" % i for i in range(n)]
    kw = dict(local=True) if mode == "local" else dict(scoring_mode="ed") if mode == "edit-distance" else {}
    params = A.Params(ungapped_mates=True, **kw)
    scheme = nvb.SmithWatermanScoringScheme.local() if mode == "local" else nvb.SmithWatermanScoringScheme()
    gw = W._pack_chunked(torch.from_numpy(text), 2, True)
    d1, d2, d_gw = torch.from_numpy(s1).to(cuda), torch.from_numpy(s2).to(cuda), gw.to(cuda)
    e = A.best_approx_paired(fmi, rfmi, d1, d2, d_gw, text.size, params, scheme, names, finish=True)
    plain = A.best_approx_paired(fmi, rfmi, d1, d2, d_gw, text.size, A.Params(**kw), scheme, names, finish=True)
    packed = [P.pack_read_streams(x) for x in (d1, d2)]
    quals = torch.full((2 * n * L + 8,), 30, dtype=torch.uint8, device=cuda)
    both = torch.cat([packed[0][1], packed[1][1]]); mate_offset = packed[0][1].numel() * 8
    both_q = torch.full((mate_offset + 2 * n * L + 8,), 30, dtype=torch.uint8, device=cuda)
    arena, idx = S.pack_names(names, cuda)
    sp = _ShimParams(int(params.local), int(params.randomized), params.top_seed, params.max_effort_init, params.max_effort, params.min_ext, params.max_ext,
                     params.max_reseed, params.rep_seeds, params.max_hits, params.allow_sub, params.subseed_len, params.seed_len, params.seed_freq[0],
                     params.min_read_len, params.max_dist, int(params.no_multi_hits), params.batch_size, params.hits_stride or 0,
                     params.seed_freq[1], params.seed_freq[2], scheme.m_match, scheme.m_score_min[0], scheme.m_score_min[1], scheme.m_score_min[2], 1,
                     1 if mode == "edit-distance" else 0)
    pp = _ShimPeParams(params.pe_policy, int(params.pe_overlap), int(params.pe_unpaired), int(params.pe_discordant), params.min_frag_len, params.max_frag_len)
    out = dict(best=[np.zeros((2, n), np.uint64) for _ in range(2)], mapq=[np.zeros(n, np.uint8) for _ in range(2)], cigar=[np.zeros((n, 64), np.uint16) for _ in range(2)],
               cigar_len=[np.zeros(n, np.uint32) for _ in range(2)], source=[np.zeros((n, 2), np.uint32) for _ in range(2)], sink=[np.zeros((n, 2), np.uint32) for _ in range(2)],
               mds=[np.zeros((n, 256), np.uint8) for _ in range(2)], mds_len=[np.zeros(n, np.uint32) for _ in range(2)])
    pair_ptrs = lambda ts: (C.c_void_p * 2)(*[t.data_ptr() for t in ts])
    pair_host = lambda arrs: (C.c_void_p * 2)(*[a.ctypes.data for a in arrs])
    u64x2 = lambda v: (C.c_uint64 * 2)(*v)
    fs, rs = fmi.struct(), rfmi.struct()
    vp = lambda t: C.c_void_p(t.data_ptr())
    torch.cuda.synchronize()
    rc = shim.nvbio_aligner_best_approx_paired_ungapped(
        C.byref(fs), C.byref(rs), C.c_uint32(n), C.c_uint32(L),
        pair_ptrs([packed[0][0].words, packed[1][0].words]), u64x2([packed[0][0].words.numel(), packed[1][0].words.numel()]), pair_ptrs([packed[0][0].begin, packed[1][0].begin]),
        pair_ptrs([packed[0][1], packed[1][1]]), u64x2([packed[0][1].numel(), packed[1][1].numel()]), vp(quals), C.c_uint64(quals.numel()), vp(arena), vp(idx),
        vp(both), C.c_uint64(both.numel()), C.c_uint64(mate_offset), vp(both_q), C.c_uint64(both_q.numel()),
        vp(d_gw), C.c_uint64(d_gw.numel()), C.c_uint32(text.size), C.byref(sp), C.byref(pp),
        pair_host(out["best"]), pair_host(out["mapq"]), pair_host(out["cigar"]), pair_host(out["cigar_len"]), pair_host(out["source"]), pair_host(out["sink"]),
        pair_host(out["mds"]), pair_host(out["mds_len"]), C.c_uint32(1), None)
    assert rc == 0
    u64 = lambda t: t.cpu().numpy().view(np.uint64)
    assert (out["best"][0] == u64(e["best"])).all() and (out["best"][1] == u64(e["best_o"])).all()
    assert (out["mapq"][0] == e["mapq1"].cpu().numpy()).all() and (out["mapq"][1] == e["mapq2"].cpu().numpy()).all()
    for slot, key, md in ((0, "tb1", "mds1"), (1, "tb2", "mds2")):
        assert (out["cigar_len"][slot] == e[key]["cigar_len"].cpu().numpy().view(np.uint32)).all(), key
        assert (out["cigar"][slot] == e[key]["cigar"].cpu().numpy().view(np.uint16)).all(), key
        assert (out["source"][slot] == e[key]["source"].cpu().numpy().view(np.uint32)).all(), key
        assert (out["mds_len"][slot] == e[md + "_len"].cpu().numpy().view(np.uint32)).all(), md
    changed = bool((u64(e["best"]) != u64(plain["best"])).any() or (u64(e["best_o"]) != u64(plain["best_o"])).any())
    assert changed == (mode != "edit-distance")             # the flag was exercised: it moves some pair in Smith-Waterman mode, none in edit-distance mode
