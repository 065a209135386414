"""Traceback timings of two builds of libnvbio_hip.so -- this tree's and another one's (the parent commit's) -- alternately in one process
on the same seeded data, device events around each call:
    python tools/traceback_edges_time.py /path/to/other/libnvbio_hip.so
1 M jobs x 100 bp x band 15 through nvbio_hip_banded_gotoh_traceback_qual_known, 500 K jobs of 150 in 650 through
nvbio_hip_gotoh_traceback_qual; on this tree's build SW (2,-1,-2,-2) against (2,-1,-2,-3) and 4-bit against 8-bit patterns."""
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import nvbio_amd as nvb
from nvbio_amd import _lib, workloads as W

REPS = 7
dev = "cuda"
new = _lib.lib()
_lib._lib = None
_lib.LIB_PATH = os.path.abspath(sys.argv[1])
parent = _lib.lib()
_lib._lib = new
assert parent is not new
stream = _lib.current_stream_ptr()


def vp(t):
    return C.c_void_p(t.data_ptr())


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); err = fn(); b.record(); torch.cuda.synchronize()
    assert err == 0, err
    return a.elapsed_time(b)


def alternate(name, calls, outs):
    """calls: {label: fn}; outs(): the tensors to compare between labels"""
    times = {k: [] for k in calls}
    snaps = {}
    for k, fn in calls.items():          # warm-up, and what each computes
        timed(fn); snaps[k] = [t.clone() for t in outs()]
    for r in range(REPS):
        for k, fn in calls.items():
            times[k].append(timed(fn))
    for k, v in times.items():
        print("%-44s %-10s median %8.3f ms  min %8.3f  max %8.3f  spread %6.3f  all %s" % (name, k, statistics.median(v), min(v), max(v), max(v) - min(v), " ".join("%.3f" % x for x in v)), flush=True)
    return times, snaps


def same(snaps, a, b):
    return all(torch.equal(x, y) for x, y in zip(snaps[a], snaps[b]))


def bytes_set(read, n, M):
    flat = read.reshape(-1)
    pad = torch.zeros((-flat.numel()) % 4 + 32, dtype=torch.uint8, device=dev)
    words = torch.cat([flat, pad]).view(torch.int32)
    idx = torch.arange(n, dtype=torch.int64, device=dev)
    return nvb.PackedStringSet(words, 8, False, idx * M, None, M)


# ---- banded: 1 M jobs x 100 bp x band 15 through nvbio_hip_banded_gotoh_traceback_qual_known
n, M, band, ty = 1_000_000, 100, 15, nvb.LOCAL
read, ref = W.make_sw_symbols(n, M, M + band, 5, dev)
p, t = W.make_sw_batch(n, M, M + band, device=dev, seed=5)
p8 = bytes_set(read, n, M)
qs = nvb.SmithWatermanScoringScheme.local().struct()
quals = torch.full((n * M + 8,), 30, dtype=torch.uint8, device=dev)
score = torch.empty(n, dtype=torch.int32, device=dev); sink = torch.empty((n, 2), dtype=torch.int32, device=dev)
source = torch.empty((n, 2), dtype=torch.int32, device=dev); cigar = torch.zeros((n, 32), dtype=torch.int16, device=dev); clen = torch.empty(n, dtype=torch.int32, device=dev)
temp = torch.empty(int(new.nvbio_hip_banded_gotoh_traceback_temp_bytes(band, M, n)), dtype=torch.uint8, device=dev)
ps, ts, p8s = p.struct(), t.struct(), p8.struct()
assert new.nvbio_hip_banded_gotoh_score_qual(C.byref(qs), ty, band, C.byref(ps), vp(quals), quals.numel(), C.byref(ts), M, M + band, n, vp(score), vp(sink), stream) == 0
torch.cuda.synchronize()
outs = lambda: [score, sink, source, cigar, clen]


def known(L, pset):
    return lambda: L.nvbio_hip_banded_gotoh_traceback_qual_known(C.byref(qs), ty, band, C.byref(pset), vp(quals), quals.numel(), C.byref(ts), M, M + band, n,
                                                                 vp(score), vp(sink), vp(source), vp(cigar), 32, vp(clen), vp(temp), temp.numel(), stream)


tm, sn = alternate("banded qual_known 1M x 100 x band 15", {"parent": known(parent, ps), "new": known(new, ps)}, outs)
print("  parent and new outputs equal:", same(sn, "parent", "new"), flush=True)
tm, sn = alternate("  new: 4-bit vs 8-bit patterns", {"4-bit": known(new, ps), "8-bit": known(new, p8s)}, outs)
print("  4-bit and 8-bit outputs equal:", same(sn, "4-bit", "8-bit"), flush=True)


def sw(L, scheme, pset):
    sc = _lib.GotohSchemeStruct(*scheme)
    return lambda: L.nvbio_hip_banded_sw_traceback(C.byref(sc), ty, band, C.byref(pset), C.byref(ts), M, M + band, n,
                                                   vp(score), vp(sink), vp(source), vp(cigar), 32, vp(clen), vp(temp), temp.numel(), stream)


alternate("banded SW, symmetric", {"parent(2,-1,-2,-2)": sw(parent, (2, -1, -2, -2), ps), "new(2,-1,-2,-2)": sw(new, (2, -1, -2, -2), ps)}, outs)
alternate("  new: SW (2,-1,-2,-2) vs (2,-1,-2,-3)", {"(2,-1,-2,-2)": sw(new, (2, -1, -2, -2), ps), "(2,-1,-2,-3)": sw(new, (2, -1, -2, -3), ps)}, outs)
alternate("  new: SW (2,-1,-2,-3), 4-bit vs 8-bit", {"4-bit": sw(new, (2, -1, -2, -3), ps), "8-bit": sw(new, (2, -1, -2, -3), p8s)}, outs)
del temp, quals, score, sink, source, cigar, clen, p, t, p8, read, ref
torch.cuda.empty_cache()

# ---- full matrix: 500 K jobs of 150 in 650 through nvbio_hip_gotoh_traceback_qual
n, M, N = 500_000, 150, 650
p, t = W.make_sw_batch(n, M, N, device=dev, seed=7, offset=400)
quals = torch.full((n * M + 8,), 30, dtype=torch.uint8, device=dev)
score = torch.empty(n, dtype=torch.int32, device=dev); sink = torch.empty((n, 2), dtype=torch.int32, device=dev)
source = torch.empty((n, 2), dtype=torch.int32, device=dev); cigar = torch.zeros((n, 32), dtype=torch.int16, device=dev); clen = torch.empty(n, dtype=torch.int32, device=dev)
temp = torch.empty(int(new.nvbio_hip_gotoh_traceback_temp_bytes(M, N, n)), dtype=torch.uint8, device=dev)
ps, ts = p.struct(), t.struct()


def full(L):
    return lambda: L.nvbio_hip_gotoh_traceback_qual(C.byref(qs), ty, C.byref(ps), vp(quals), quals.numel(), C.byref(ts), M, N, n,
                                                    vp(score), vp(sink), vp(source), vp(cigar), 32, vp(clen), vp(temp), temp.numel(), stream)


tm, sn = alternate("full qual 500K x 150 in 650", {"parent": full(parent), "new": full(new)}, outs)
print("  parent and new outputs equal:", same(sn, "parent", "new"), flush=True)
print("last kernel:", new.nvbio_hip_last_kernel().decode())
