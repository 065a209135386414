#!/usr/bin/env python3
"""Times MEM seeding (nvbio_hip_fm_mem_rank, nvbio_hip_fm_mem_rank_split / nvbio_amd.MEMFilter) and writes the figures to a file.

Workload: --reads (1 M) reads of 150 bp sampled from a random genome of 2^--text-log2 (2^28) symbols with 2 % substitutions, 4-bit
big-endian, against the forward index and the index of the reversed genome, both built on the device; min_intv 1, min_span 19,
max_intv 10 000 (the defaults of the reference's examples/mem/mem.cu).  After a warm-up, --reps (7) timed calls with device events
around each; the median and the spread are reported as reads/s, with MEMs per read, the index records gathered per read as the
`_host` twin counts them (what the kernel loads: one or two per step), and that gather rate as a fraction of the chip's random-line rate -- measured here as
nvbio_hip_fm_rank over 2^24 random rows of the same index, one 32-byte record each.  The only other implementation is the `_host`
twin on 16 threads: it is timed on the first --host-reads (100 k) reads of the same set (--host-reps (5) calls after a warm-up), whose
ranks must equal the device's.
With --split-len / --split-width (nvmem's are 28 and 10) the same run then times nvbio_hip_fm_mem_rank_split on the same reads and reports,
next to the plain figures, the MEMs per read after re-seeding, the extra index records the re-seed walks read (the two host twins'
counts on the first --host-reads reads) and the gather rate of that added work, extra records over extra time; the default output file
is then profiles/mem/mem_split_time.txt.
Usage: python tools/mem_time.py [--split-len 28 --split-width 10] [--out profiles/mem/mem_time.txt]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nvbio_amd as nvb                      # noqa: E402
from nvbio_amd import _lib, workloads as W   # noqa: E402


def timed(fn, reps, warm=1):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def host_struct(fmi, keep):
    """the C-ABI description of a device index copied to host memory"""
    bo, ssa = fmi.bwt_occ.cpu().numpy(), fmi.ssa.cpu().numpy()
    keep += [bo, ssa]
    s = _lib.FMIndexStruct()
    s.length, s.primary, s.sa_int = fmi.length, fmi.primary, fmi.sa_int
    for i in range(5):
        s.L2[i] = fmi.L2[i]
    s.bwt_occ, s.ssa = bo.ctypes.data, ssa.ctypes.data
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--text-log2", type=int, default=28)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-reads", type=int, default=100_000)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--split-len", type=lambda v: int(v, 0), default=0xFFFFFFFF)
    ap.add_argument("--split-width", type=lambda v: int(v, 0), default=0xFFFFFFFF)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    split = a.split_len != 0xFFFFFFFF
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "mem", "mem_split_time.txt" if split else "mem_time.txt")
    dev = torch.device("cuda:0")
    n, ln, G = a.reads, 150, 1 << a.text_log2
    min_intv, max_intv, min_span = 1, 10000, 19
    g = torch.Generator(device=dev); g.manual_seed(2025)
    text = torch.randint(0, 4, (G,), dtype=torch.uint8, generator=g, device=dev)
    t0 = time.time()
    f = W.build_fm_index(text)
    r = W.build_fm_index(torch.flip(text, [0]).contiguous())
    torch.cuda.synchronize()
    t_build = time.time() - t0
    at = torch.randint(0, G - ln, (n,), generator=g, device=dev)
    reads = text[at.unsqueeze(1) + torch.arange(ln, device=dev).unsqueeze(0)]
    flips = torch.rand(reads.shape, generator=g, device=dev) < 0.02
    reads = torch.where(flips, (reads + torch.randint(1, 4, reads.shape, dtype=torch.uint8, generator=g, device=dev)) & 3, reads)
    words = W._pack_chunked(reads.reshape(-1), 4, True)
    begin = torch.arange(n, dtype=torch.int64, device=dev) * ln
    reads_set = nvb.PackedStringSet(words, 4, True, begin, None, ln)
    del text, reads, flips

    L = nvb.lib()
    cap = 16 * n
    tb = int(L.nvbio_hip_fm_mem_temp_bytes(n, ln))
    temp = torch.empty(tb, dtype=torch.uint8, device=dev)
    ranges = torch.empty((cap, 4), dtype=torch.int32, device=dev)
    slots = torch.empty(cap, dtype=torch.int64, device=dev)
    index = torch.empty(n + 1, dtype=torch.int64, device=dev)
    found = C.c_uint64(0)
    fs, rs, ss = f.struct(), r.struct(), reads_set.struct()
    vp = lambda t: C.c_void_p(t.data_ptr())

    def run():
        nvb.check(L.nvbio_hip_fm_mem_rank(C.byref(fs), C.byref(rs), C.byref(ss), n, ln, min_intv, max_intv, min_span, vp(ranges), cap, vp(index), vp(slots),
                                          C.byref(found), vp(temp), tb, _lib.current_stream_ptr()), "nvbio_hip_fm_mem_rank")
    ms = timed(run, a.reps)
    n_mems = int(found.value)
    n_hits = int(slots[n_mems - 1].item()) if n_mems else 0

    # the chip's random-line rate on this index: one 32-byte record per query
    nq = 1 << 24
    k = torch.randint(0, G, (nq,), generator=g, device=dev).to(torch.int32)
    c = torch.randint(0, 4, (nq,), dtype=torch.uint8, generator=g, device=dev)
    out = torch.empty(nq, dtype=torch.int32, device=dev)
    ms_rank = timed(lambda: nvb.check(L.nvbio_hip_fm_rank(C.byref(fs), vp(k), vp(c), nq, vp(out), _lib.current_stream_ptr()), "nvbio_hip_fm_rank"), a.reps)
    line_rate = nq / (float(np.median(ms_rank)) * 1e-3)

    # the host twin, on the first reads of the same set
    hn = min(a.host_reads, n)
    keep = []
    hfs, hrs = host_struct(f, keep), host_struct(r, keep)
    hw, hb = words.cpu().numpy(), begin[:hn].cpu().numpy()
    hss = _lib.StringSetStruct()
    hss.words, hss.n_words, hss.bits, hss.big_endian = hw.ctypes.data, hw.size, 4, 1
    hss.begin, hss.length, hss.fixed_length = hb.ctypes.data, None, ln
    h_ranges, h_slots, h_index = np.zeros((16 * hn, 4), np.uint32), np.zeros(16 * hn, np.uint64), np.zeros(hn + 1, np.uint64)
    h_found, h_records = C.c_uint64(0), C.c_uint64(0)
    h_s = []
    for rep in range(1 + a.host_reps):      # the first call is the warm-up
        t0 = time.time()
        nvb.check(L.nvbio_hip_fm_mem_rank_host(C.byref(hfs), C.byref(hrs), C.byref(hss), hn, ln, min_intv, max_intv, min_span, h_ranges.ctypes.data, 16 * hn,
                                               h_index.ctypes.data, h_slots.ctypes.data, C.byref(h_found), C.byref(h_records), a.host_threads), "nvbio_hip_fm_mem_rank_host")
        if rep:
            h_s.append(time.time() - t0)
    k_h = int(h_found.value)
    same = bool((ranges[:k_h].cpu().numpy().view(np.uint32) == h_ranges[:k_h]).all()) and bool((index[:hn + 1].cpu().numpy().view(np.uint64) == h_index).all())
    rec_per_read = h_records.value / hn

    med = float(np.median(ms))
    reads_s = n / (med * 1e-3)
    # rank walks every read twice (count, then write)
    gather_rate = 2.0 * rec_per_read * reads_s
    lines = [
        "MEM seeding: %d reads of %d bp, 2 %% substitutions, genome 2^%d (two indices built on the device in %.1f s); min_intv %d, max_intv %d, min_span %d" % (
            n, ln, a.text_log2, t_build, min_intv, max_intv, min_span),
        "nvbio_hip_fm_mem_rank      %d calls, ms: median %.2f  (min %.2f .. max %.2f)   %.3g reads/s" % (a.reps, med, min(ms), max(ms), reads_s),
        "  MEMs per read %.2f   occurrences per read %.2f   temp %.0f MB" % (n_mems / n, n_hits / n, tb / 1e6),
        "  records gathered per read (host twin's count, one walk) %.1f = %.0f algorithmic bytes; the entry walks twice: %.3g records/s" % (
            rec_per_read, 32 * rec_per_read, gather_rate),
        "  random-line rate of this index (nvbio_hip_fm_rank, 2^24 random rows): median %.3f ms = %.3g lines/s   ->   MEM gather rate / line rate = %.2f" % (
            float(np.median(ms_rank)), line_rate, gather_rate / line_rate),
        "nvbio_hip_fm_mem_rank_host %d threads, first %d reads, %d calls after a warm-up, s: median %.2f  (min %.2f .. max %.2f)   %.3g reads/s   device / host = %.1f" % (
            a.host_threads, hn, a.host_reps, float(np.median(h_s)), min(h_s), max(h_s), hn / float(np.median(h_s)), reads_s / (hn / float(np.median(h_s)))),
        "  device ranks of those reads equal the host twin's: %s" % same,
    ]
    if split:
        # the same reads through the re-seeding entry: its own scratch, the same output arrays
        tb_s = int(L.nvbio_hip_fm_mem_split_temp_bytes(n, ln, cap))
        del temp
        temp_s = torch.empty(tb_s, dtype=torch.uint8, device=dev)

        def run_split():
            nvb.check(L.nvbio_hip_fm_mem_rank_split(C.byref(fs), C.byref(rs), C.byref(ss), n, ln, min_intv, max_intv, min_span, a.split_len, a.split_width,
                                                    vp(ranges), cap, vp(index), vp(slots), C.byref(found), vp(temp_s), tb_s, _lib.current_stream_ptr()),
                      "nvbio_hip_fm_mem_rank_split")
        ms_s = timed(run_split, a.reps)
        n_mems_s = int(found.value)
        s_found, s_records = C.c_uint64(0), C.c_uint64(0)
        nvb.check(L.nvbio_hip_fm_mem_rank_split_host(C.byref(hfs), C.byref(hrs), C.byref(hss), hn, ln, min_intv, max_intv, min_span, a.split_len, a.split_width,
                                                     h_ranges.ctypes.data, 16 * hn, h_index.ctypes.data, h_slots.ctypes.data, C.byref(s_found), C.byref(s_records),
                                                     a.host_threads), "nvbio_hip_fm_mem_rank_split_host")
        k_s = int(s_found.value)
        same_s = bool((ranges[:k_s].cpu().numpy().view(np.uint32) == h_ranges[:k_s]).all()) and bool((index[:hn + 1].cpu().numpy().view(np.uint64) == h_index).all())
        same = same and same_s
        med_s = float(np.median(ms_s))
        extra_rec = (s_records.value - h_records.value) / hn            # per read, one walk
        extra_ms = med_s - med
        added_rate = 2.0 * extra_rec * n / (extra_ms * 1e-3) if extra_ms > 0 else float("inf")
        lines += [
            "nvbio_hip_fm_mem_rank_split  split_len %d, split_width %d   %d calls, ms: median %.2f  (min %.2f .. max %.2f)   %.3g reads/s   split / plain = %.2f" % (
                a.split_len, a.split_width, a.reps, med_s, min(ms_s), max(ms_s), n / (med_s * 1e-3), med_s / med),
            "  MEMs per read %.2f (plain %.2f)   temp %.0f MB" % (n_mems_s / n, n_mems / n, tb_s / 1e6),
            "  extra records gathered per read by the re-seed walks (host twins' counts, one walk) %.1f (plain %.1f); both passes walk: %.3g records in %.2f ms extra = %.3g records/s" % (
                extra_rec, rec_per_read, 2.0 * extra_rec * n, extra_ms, added_rate),
            "  gather rate of the added work / the plain entry's gather rate in this run = %.2f" % (added_rate / gather_rate),
            "  device ranks of the first %d reads equal the split host twin's: %s" % (hn, same_s),
        ]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
