#!/usr/bin/env python3
"""Times ungapped (Hamming) scoring at the paired driver's own shape and writes the figures to a file.

Job set: --jobs (500 k) jobs of one 150-bp 4-bit read with random qualities against a 650-bp 2-bit genome window (max_frag_len + L),
half of the windows holding the read with a few substitutions, per-job thresholds (nvBowtie's score-min of the mode).  For SEMI_GLOBAL and
LOCAL, alternating in one process, --reps (20) repetitions each after a warm-up, device events around each call:
  (a) nvbio_hip_hamming_score_qual                                    the new entry
  (b) nvbio_hip_alignment_score_qual, pattern blocking                the gapped scorer the flag replaces, on the same jobs
  (c) BatchedAlignmentScore over the HammingDistanceAligner stream    the drop-in layer's generic lane (NVBIO_HIP_COMPAT_GENERIC=full): the
      of tests/compat/hamming_callers.hip                             only route this aligner had before
  (d) the same stream on the layer's default route                    (staging + the new entry)
Required: (a) faster than (b) and than (c) by more than the spread (max - min) of the repetitions.  Then the paired Python driver's
opposite_score stage clock with Params.ungapped_mates on and off on one batch of config 5's shape (2 x 150 bp FR pairs, --local) over a
small genome.  Usage: python tools/ungapped_time.py [--out profiles/ungapped/ungapped_time.txt]"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nvbio_amd as nvb                      # noqa: E402
from nvbio_amd import _lib, aligner as A     # noqa: E402


def pack_be(sym, bits):
    per = 32 // bits
    pad = np.zeros((-len(sym)) % per + 4 * per, np.uint8)
    v = np.concatenate([sym, pad]).astype(np.uint32).reshape(-1, per)
    sh = (32 - bits - bits * np.arange(per)).astype(np.uint32)
    return (v << sh).sum(axis=1).astype(np.uint32)


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=500_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=100_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ungapped", "ungapped_time.txt"))
    ap.add_argument("--kernel-only", action="store_true", help="only (a), a few repetitions: for a kernel trace")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    L_, W_ = 150, 650
    rng = np.random.default_rng(2024)
    n, G = a.jobs, 1 << 24
    genome = rng.integers(0, 4, G).astype(np.uint8)
    lo = rng.integers(0, G - W_ - 1, n).astype(np.int64)
    at = lo + rng.integers(0, W_ - L_ + 1, n)
    reads = genome[(at[:, None] + np.arange(L_)[None, :])]
    unrelated = rng.random(n) < 0.5
    reads[unrelated] = rng.integers(0, 4, (int(unrelated.sum()), L_))
    flips = rng.random((n, L_)) < 0.02
    reads[flips] = rng.integers(0, 4, int(flips.sum()))
    quals = rng.integers(2, 41, n * L_).astype(np.uint8)
    d_reads = torch.from_numpy(pack_be(reads.reshape(-1), 4).view(np.int32)).to(dev)
    d_genome = torch.from_numpy(pack_be(genome, 2).view(np.int32)).to(dev)
    d_quals = torch.from_numpy(quals).to(dev)
    pats = nvb.PackedStringSet(d_reads, 4, True, torch.arange(n, dtype=torch.int64, device=dev) * L_, None, L_)
    txts = nvb.PackedStringSet(d_genome, 2, True, torch.from_numpy(lo).to(dev), None, W_)
    d_offsets = (torch.arange(n + 1, dtype=torch.int64, device=dev) * L_).to(torch.int32)
    d_windows = torch.from_numpy(np.stack([lo, lo + W_], axis=1).astype(np.uint32).view(np.int32)).to(dev)
    score = torch.empty(n, dtype=torch.int32, device=dev); sink = torch.empty((n, 2), dtype=torch.int32, device=dev); ok = torch.empty(n, dtype=torch.uint8, device=dev)
    caller = C.CDLL(os.path.join(ROOT, "tests", "compat", "libhamming_callers.so"))
    lines = ["ungapped scoring, %d jobs of %d x %d, %d repetitions each (ms: median, min .. max)" % (n, L_, W_, a.reps)]
    L = nvb.lib()
    verdict = True
    for typ, name in ((nvb.SEMI_GLOBAL, "SEMI_GLOBAL"), (nvb.LOCAL, "LOCAL")):
        scheme = nvb.SmithWatermanScoringScheme.local() if typ == nvb.LOCAL else nvb.SmithWatermanScoringScheme()
        ms = torch.full((n,), int(scheme.min_score(L_)), dtype=torch.int32, device=dev)
        sc = scheme.struct()
        ps, ts = pats.struct(), txts.struct()
        tail = (L_, W_, C.c_void_p(ms.data_ptr()), n, C.c_void_p(score.data_ptr()), C.c_void_p(sink.data_ptr()), C.c_void_p(ok.data_ptr()), None)

        def run_a():
            nvb.check(L.nvbio_hip_hamming_score_qual(C.byref(sc), 0, typ, C.byref(ps), C.c_void_p(d_quals.data_ptr()), d_quals.numel(), C.byref(ts), *tail), "hamming")

        def run_b():
            nvb.check(L.nvbio_hip_alignment_score_qual(C.byref(sc), 0, typ, C.byref(ps), C.c_void_p(d_quals.data_ptr()), d_quals.numel(), C.byref(ts), *tail), "gotoh")
        path = C.create_string_buffer(16)

        def run_layer():
            assert caller.hamming_views(typ, 0, scheme.match(), scheme.m_mmp_min, scheme.m_mmp_max, n, C.c_void_p(d_offsets.data_ptr()), C.c_void_p(d_reads.data_ptr()),
                                        C.c_void_p(d_quals.data_ptr()), L_, C.c_void_p(d_genome.data_ptr()), C.c_void_p(d_windows.data_ptr()), W_,
                                        C.c_void_p(ms.data_ptr()), C.c_void_p(score.data_ptr()), C.c_void_p(sink.data_ptr()), path) == 0
        if a.kernel_only:
            timed(run_a, 3, warm=1)
            continue
        run_a(); torch.cuda.synchronize()
        sa, ka, oka = score.clone(), sink.clone(), ok.clone()
        os.environ["NVBIO_HIP_COMPAT_GENERIC"] = "full"
        run_layer(); assert path.value == b"generic"
        same = bool((score == sa).all()) and bool((sink == ka).all())
        t = {"a": [], "b": [], "c": [], "d": []}
        for r in range(a.reps):                     # alternating: one repetition of each per round (the first round's are the warm-up's)
            os.environ.pop("NVBIO_HIP_COMPAT_GENERIC", None)
            t["a"] += timed(run_a, 1, warm=1 if r == 0 else 0)
            t["b"] += timed(run_b, 1, warm=1 if r == 0 else 0)
            t["d"] += timed(run_layer, 1, warm=1 if r == 0 else 0)
            os.environ["NVBIO_HIP_COMPAT_GENERIC"] = "full"
            t["c"] += timed(run_layer, 1, warm=1 if r == 0 else 0)
        os.environ.pop("NVBIO_HIP_COMPAT_GENERIC", None)
        f = lambda v: "%8.3f  (%.3f .. %.3f)" % (float(np.median(v)), min(v), max(v))
        lines.append("%s  accepted %d of %d jobs; generic lane gives the same sinks: %s" % (name, int(oka.sum()), n, same))
        lines.append("  (a) nvbio_hip_hamming_score_qual              %s" % f(t["a"]))
        lines.append("  (b) nvbio_hip_alignment_score_qual (gapped)   %s" % f(t["b"]))
        lines.append("  (c) layer, generic lane                       %s" % f(t["c"]))
        lines.append("  (d) layer, default route                      %s" % f(t["d"]))
        spread = max(max(v) - min(v) for v in (t["a"], t["b"], t["c"]))
        ok_b = np.median(t["b"]) - np.median(t["a"]) > spread
        ok_c = np.median(t["c"]) - np.median(t["a"]) > spread
        verdict = verdict and ok_b and ok_c and same
        lines.append("  b / a = %.2f   c / a = %.2f   largest spread %.3f ms   (a) faster than (b): %s, than (c): %s" % (
            np.median(t["b"]) / np.median(t["a"]), np.median(t["c"]) / np.median(t["a"]), spread, ok_b, ok_c))
    if not a.kernel_only and a.pairs:
        from oracle import pyoracle as O
        text = rng.integers(0, 4, 1 << 20).astype(np.uint8)
        host = O.FMIndex(text)
        fmi = nvb.FMIndexDevice.from_host(host, dev)
        npairs, PL = a.pairs, 150
        frag = rng.integers(250, 450, npairs); pos = rng.integers(0, text.size - 460, npairs)
        s1 = text[pos[:, None] + np.arange(PL)[None, :]]
        s2 = (3 - text[(pos + frag - PL)[:, None] + np.arange(PL)[None, :]])[:, ::-1].copy()
        for m in (s1, s2):
            fl = rng.random(m.shape) < 0.02
            m[fl] = rng.integers(0, 4, int(fl.sum()))
        from nvbio_amd import workloads as W
        gw = W._pack_chunked(torch.from_numpy(text), 2, True).to(dev)
        d1, d2 = torch.from_numpy(s1).to(dev), torch.from_numpy(s2).to(dev)
        q1 = torch.from_numpy(rng.integers(2, 41, s1.shape).astype(np.uint8)).to(dev); q2 = torch.from_numpy(rng.integers(2, 41, s2.shape).astype(np.uint8)).to(dev)
        lines.append("paired Python driver, %d pairs of 2 x %d bp, --local, 1 Mbp genome: opposite_score stage clock, ms (second of two batches)" % (npairs, PL))
        for flag in (False, True):
            prm = A.Params(local=True, ungapped_mates=flag)
            for _ in range(2):
                r = A.best_approx_paired(fmi, None, d1, d2, gw, text.size, prm, stage_times=True, traceback=False, quals1=q1, quals2=q2)
            lines.append("  ungapped_mates=%-5s  opposite_score %8.2f   opposite DP jobs %d   all stages %8.2f" % (
                flag, r["stats"]["ms"]["opposite_score"], r["stats"].get("opposite_dp_jobs", 0), sum(r["stats"]["ms"].values())))
    if not a.kernel_only:
        lines.append("requirement met: %s" % verdict)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0 if verdict else 1


if __name__ == "__main__":
    sys.exit(main())
