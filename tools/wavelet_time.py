#!/usr/bin/env python3
"""Times the wavelet tree and the FM-index over it on the device (nvbio_amd.wavelet over nvbio_amd/csrc/wavelet.hip and sufsort.hip,
DESIGN.md 3.15) and writes the figures to a file.

Stages: setup of a 64 M-symbol text at S = 8 (i.i.d. bytes) and S = 5 (24 values), beside the reference's algorithm in torch library
calls on the same data (per level: pack the level's bit plane, then a stable sort by the leading bits); rank with 1, 2 and 4 queries a
lane (NVBIO_HIP_WAVELET_LANES), rank_range and text over 16 M queries, shuffled and sorted, each beside the chip's random-line rate
(a rate to compare with, not a bound: the tree's top levels stay in cache) recorded in profiles/mem/mem_time.txt divided by the lines a query touches; match of 4 M patterns of 30 symbols; locate of 16 M rows at
sa_int = 16; bwt_bytes of the text beside the 2-bit sorter on a text of the same length.

Lines a query touches: a level reads one word of occ and one of bits, two distinct 128-byte lines; on an i.i.d. text far longer than
its alphabet no node on a path is empty, so rank and text touch 2 S lines, rank_range and a match step at most 4 S.

Every stage runs once unrecorded and then --reps (5) times between two device events; the median, the least and the greatest are listed.

Usage: python tools/wavelet_time.py [--text 67108864] [--queries 16777216] [--patterns 4194304] [--out profiles/wavelet/wavelet_time.txt]"""
import argparse
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps):
    """-> (result of the last call, [milliseconds])"""
    import torch
    out = fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        del out
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return out, times


def recorded_line_rate():
    """the chip's random-line rate as profiles/mem/mem_time.txt has it, or None"""
    try:
        with open(os.path.join(ROOT, "profiles", "mem", "mem_time.txt")) as f:
            m = re.search(r"random-line rate[^\n]*?=\s*([0-9.]+e[+-]?[0-9]+) lines/s", f.read())
        return float(m.group(1)) if m else None
    except OSError:
        return None


def stat(t):
    s = sorted(t)
    return s[len(s) // 2], s[0], s[-1]


def torch_setup(text, S):
    """the reference's setup in torch library calls: per level, the bit plane packed into big-endian words, then a stable sort by the
    leading l + 1 bits.  -> the packed planes, one tensor per level (a level is padded to whole words here: the cost, not the layout)"""
    import torch
    weights = (1 << torch.arange(31, -1, -1, device=text.device, dtype=torch.int64))
    cur, planes = text, []
    for l in range(S):
        bit = ((cur >> (S - 1 - l)) & 1).to(torch.int64)
        pad = (-bit.numel()) % 32
        if pad:
            bit = torch.cat([bit, torch.zeros(pad, dtype=torch.int64, device=text.device)])
        planes.append((bit.view(-1, 32) * weights).sum(1).to(torch.int32))
        if l + 1 < S:
            cur = cur[torch.sort(cur >> (S - 1 - l), stable=True).indices]
    return planes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--text", type=int, default=1 << 26)
    ap.add_argument("--queries", type=int, default=1 << 24)
    ap.add_argument("--patterns", type=int, default=1 << 22)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wavelet", "wavelet_time.txt"))
    a = ap.parse_args()

    import torch
    import nvbio_amd as nvb
    from nvbio_amd import sufsort
    assert torch.cuda.is_available(), "wavelet_time.py measures on the GPU; there is nothing to time without one"
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(0x5EED0021)
    rate = recorded_line_rate()
    n, m = a.text, a.queries
    lines = ["wavelet tree and FM-index over it on the device (nvbio_amd.wavelet): %s" % torch.cuda.get_device_name(dev),
             "one unrecorded call, then %d calls between two device events: median [least, greatest] in ms" % a.reps,
             "random-line rate recorded in profiles/mem/mem_time.txt: %s lines/s" % ("%.3e" % rate if rate else "not found"), ""]

    def row(stage, items, unit, t, per_query_lines=None):
        med, lo, hi = stat(t)
        r = items / (med * 1e-3)
        s = "%-64s %9.3f [%9.3f, %9.3f] ms   %.3e %s/s" % (stage, med, lo, hi, r, unit)
        if per_query_lines and rate:
            s += "   %d lines a query: %.2f of the reference line rate" % (per_query_lines, r * per_query_lines / rate)
        lines.append(s)
        print(s, flush=True)
        return med

    texts = {8: torch.randint(0, 256, (n,), dtype=torch.uint8, generator=g, device=dev),
             5: torch.randint(0, 24, (n,), dtype=torch.uint8, generator=g, device=dev)}
    trees = {}
    for S, text in texts.items():
        trees[S], t = timed(lambda: nvb.WaveletTree.build(text, S), a.reps)
        ours = row("setup, %d symbols, S = %d" % (n, S), n, "symbols", t)
        planes, tb = timed(lambda: torch_setup(text, S), a.reps)
        base = row("  torch: S bit planes packed, S - 1 stable sorts", n, "symbols", tb)
        same = n % 32 == 0 and bool(torch.equal(torch.cat(planes), trees[S].bits))
        lines.append("  torch / this library = %.2f   same bits: %s" % (base / ours, same if n % 32 == 0 else "not compared (levels padded)"))
        del planes

    for S in (8, 5):
        tree = trees[S]
        pos = torch.randint(0, n, (m,), generator=g, device=dev).to(torch.int32)
        sym = torch.randint(0, 256 if S == 8 else 24, (m,), dtype=torch.uint8, generator=g, device=dev)
        spos = torch.sort(pos.to(torch.int64)).values.to(torch.int32)
        ranges = torch.stack([pos, (pos.to(torch.int64) + 1000).clamp(max=n - 1).to(torch.int32)], dim=1).contiguous()
        sranges = torch.stack([spos, (spos.to(torch.int64) + 1000).clamp(max=n - 1).to(torch.int32)], dim=1).contiguous()
        for name, p, rg in (("shuffled", pos, ranges), ("sorted", spos, sranges)):
            ref = None
            for lanes in (1, 2, 4):
                with nvb.test_switch("NVBIO_HIP_WAVELET_LANES", lanes):
                    out, t = timed(lambda: tree.rank(p, sym), a.reps)
                    row("rank, S = %d, %d %s queries, %d a lane" % (S, m, name, lanes), m, "queries", t, 2 * S)
                    _, t = timed(lambda: tree.text(p), a.reps)
                    row("text, S = %d, %d %s queries, %d a lane" % (S, m, name, lanes), m, "queries", t, 2 * S)
                assert ref is None or torch.equal(ref, out)
                ref = out
            _, t = timed(lambda: tree.rank_range(rg, sym), a.reps)
            row("rank_range, S = %d, %d %s ranges 1000 wide" % (S, m, name), m, "ranges", t, 4 * S)
        del pos, sym, spos, ranges, sranges
    del trees

    # ---- the FM-index: bwt_bytes beside the 2-bit sorter, then match and locate ----
    for S, text in texts.items():
        (bwt, primary, ssa, _), t = timed(lambda: nvb.bwt_bytes(text, S, 16), a.reps)
        med = row("bwt_bytes, %d symbols, S = %d (%d rounds)" % (n, S, len(sufsort.last_rounds())), n, "suffixes", t)
        lines.append("  %.2f ns a suffix" % (med * 1e6 / n))
        del bwt, ssa
    dna = torch.randint(0, 4, (n,), dtype=torch.uint8, generator=g, device=dev)
    packed = (sufsort._pack_text(dna), n, True)
    del dna
    _, t = timed(lambda: sufsort.bwt(packed, 16), a.reps)
    med = row("bwt of a 2-bit text, %d symbols (%d rounds)" % (n, len(sufsort.last_rounds())), n, "suffixes", t)
    lines.append("  %.2f ns a suffix" % (med * 1e6 / n))
    del packed
    for S, text in texts.items():
        fmi = nvb.WaveletFMIndex.build(text, S, 16)
        P, plen = a.patterns, 30
        starts = torch.randint(0, n - plen, (P,), generator=g, device=dev)
        ps = nvb.ByteStringSet(text, starts, None, plen)              # patterns cut from the text, in place
        rg, t = timed(lambda: fmi.match(ps), a.reps)
        row("match, S = %d, %d patterns of %d symbols from the text" % (S, P, plen), P, "patterns", t)
        assert bool((rg[:, 0] <= rg[:, 1]).all())
        rows = torch.randint(1, n + 1, (m,), generator=g, device=dev).to(torch.int32)
        _, t = timed(lambda: fmi.locate(rows), a.reps)
        row("locate, S = %d, %d random rows, sa_int = 16" % (S, m), m, "rows", t)
        del fmi, ps, rg, rows

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
