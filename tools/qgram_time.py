#!/usr/bin/env python3
"""Times the q-gram index and filter on the device (nvbio_amd.qgram over nvbio_amd/csrc/qgram.hip) stage by stage, each
beside a baseline made of torch library calls on the same data, and writes the figures to a file.

Stages: the build of a string index over a 64 M-symbol i.i.d. text at q = 20, QL = 12; the build of a set index over 1 M reads of 150 bp
at q = 20, interval 10; range queries over 16 M q-grams of the text, unsorted and sorted; the filter's rank, locate and merge on those
queries (about one hit a query, so 16 M-hit batches).  Baselines: torch.sort + torch.unique_consecutive for the builds and for merge,
torch.searchsorted on the distinct q-grams for range (plus a cumsum for rank), torch.repeat_interleave for locate.

Every stage runs once unrecorded (code objects, scratch, rocPRIM's choices) and then --reps (5) times between two device events; the
median, the least and the greatest time are listed.  A stage "loses" when its least time is above the baseline's greatest, "wins" when
its greatest is below the baseline's least, and is "within the spread" otherwise.  The results of a stage and of its baseline are compared
where they are the same thing (distinct q-grams, ranges, merged diagonals).

Usage: python tools/qgram_time.py [--text 67108864] [--reads 1000000] [--queries 16777216] [--out profiles/qgram/qgram_time.txt]"""
import argparse
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

Q, QL, READ_LEN, INTERVAL = 20, 12, 150, 10


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--text", type=int, default=1 << 26)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=1 << 24)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qgram", "qgram_time.txt"))
    a = ap.parse_args()

    import torch
    import nvbio_amd as nvb
    from nvbio_amd import sufsort as S
    from nvbio_amd.strings import PackedStringSet
    assert torch.cuda.is_available(), "qgram_time.py measures on the GPU; there is nothing to time without one"
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(0x5EED0020)
    rows = []          # (stage, items, unit, ours [ms], baseline [ms], same results or None)

    def stat(t):
        s = sorted(t)
        return s[len(s) // 2], s[0], s[-1]

    # ---- the string index ----
    n = a.text
    text = (S._pack_text(torch.randint(0, 4, (n,), dtype=torch.uint8, generator=g, device=dev)), n, True)
    keys = nvb.generate_qgrams(text, Q)
    _, t_gen = timed(lambda: nvb.generate_qgrams(text, Q), a.reps)
    rows.append(("generate_qgrams, every position of the text", n, "q-grams", t_gen, None, None))
    ix, t_build = timed(lambda: nvb.QGramIndex.build(text, Q, QL), a.reps)

    def base_build(k):
        v, order = torch.sort(k)
        u, c = torch.unique_consecutive(v, return_counts=True)
        return u, c, order
    (u, c, order), t_base = timed(lambda: base_build(keys), a.reps)
    same = bool(torch.equal(u, ix.qgrams)) and bool(torch.equal(torch.cumsum(c, 0).to(torch.int32), ix.slots[1:]))
    rows.append(("QGramIndex.build, %d-symbol text, q = %d, QL = %d" % (n, Q, QL), n, "q-grams", t_build, t_base, same))
    del c, order

    # ---- the set index ----
    N = a.reads
    reads = torch.randint(0, 4, (N * READ_LEN,), dtype=torch.uint8, generator=g, device=dev)
    ss = PackedStringSet(S._pack_text(reads), 2, True, torch.arange(N, dtype=torch.int64, device=dev) * READ_LEN, None, READ_LEN)
    six, t_sbuild = timed(lambda: nvb.QGramSetIndex.build(ss, Q, INTERVAL, QL), a.reps)
    per = (READ_LEN - Q) // INTERVAL + 1
    coords = torch.stack([torch.arange(N, device=dev).repeat_interleave(per), (torch.arange(per, device=dev) * INTERVAL).repeat(N)], dim=1).to(torch.int32)
    skeys = nvb.generate_qgrams(ss, Q, coords)
    (su, sc, _), t_sbase = timed(lambda: base_build(skeys), a.reps)
    same = bool(torch.equal(su, six.qgrams)) and six.n_qgrams == N * per
    rows.append(("QGramSetIndex.build, %d reads of %d bp, q = %d, interval %d, QL = %d" % (N, READ_LEN, Q, INTERVAL, QL), N * per, "q-grams",
                 t_sbuild, t_sbase, same))
    del six, su, sc, skeys, coords, reads, ss

    # ---- range queries: q-grams of random text positions, so nearly all are present ----
    m = a.queries
    queries = keys[torch.randint(0, n, (m,), generator=g, device=dev)].contiguous()
    squeries = torch.sort(queries).values
    del keys

    def base_range(qs):
        i = torch.searchsorted(u, qs)
        i = i.clamp(max=u.numel() - 1)
        found = u[i] == qs
        lo = torch.where(found, ix.slots[i], torch.zeros_like(ix.slots[i]))
        hi = torch.where(found, ix.slots[i + 1], torch.zeros_like(lo))
        return torch.stack([lo, hi], dim=1)
    for name, qs in (("unsorted", queries), ("sorted", squeries)):
        r, t_ours = timed(lambda: ix.range(qs), a.reps)
        rb, t_b = timed(lambda: base_range(qs), a.reps)
        rows.append(("QGramIndex.range, %d %s queries" % (m, name), m, "queries", t_ours, t_b, bool(torch.equal(r, rb))))
        del r, rb
    sorted_rate = m / (stat(rows[-1][3])[0] * 1e-3)

    # ---- the filter ----
    indices = torch.randint(0, 1 << 20, (m,), generator=g, device=dev).to(torch.int32)
    f = nvb.QGramFilter()
    total, t_rank = timed(lambda: f.rank(ix, queries, indices), a.reps)

    def base_rank():
        r = base_range(queries)
        return r, torch.cumsum((r[:, 1] - r[:, 0]).to(torch.int64), 0)
    (rb, sb), t_brank = timed(base_rank, a.reps)
    rows.append(("QGramFilter.rank, %d queries -> %d hits" % (m, total), m, "queries", t_rank, t_brank, bool(torch.equal(sb, f.slots))))
    batch = min(total, 1 << 24)
    hits, t_loc = timed(lambda: f.locate(0, batch), a.reps)

    def base_locate():
        sizes = (rb[:, 1] - rb[:, 0]).to(torch.int64)
        slot = torch.repeat_interleave(torch.arange(m, device=dev), sizes)[:batch]
        at = rb[slot, 0].to(torch.int64) + (torch.arange(batch, device=dev) - (sb[slot] - sizes[slot]))
        return torch.stack([ix.index[at], indices[slot]], dim=1)
    hb, t_bloc = timed(base_locate, a.reps)
    rows.append(("QGramFilter.locate, a batch of %d hits" % batch, batch, "hits", t_loc, t_bloc, bool(torch.equal(hits, hb))))
    del hb, rb, sb
    (merged, counts), t_merge = timed(lambda: f.merge(INTERVAL, hits), a.reps)

    def base_merge():
        d = (hits[:, 1] - hits[:, 0]).to(torch.int64) & 0xFFFFFFFF
        r = (d // INTERVAL) * INTERVAL
        d = torch.where(((d - r) * 2 & 0xFFFFFFFF) > INTERVAL, r + 1, r)
        return torch.unique_consecutive(torch.sort(d).values, return_counts=True)
    (mb, cb), t_bmerge = timed(base_merge, a.reps)
    same = bool(torch.equal(mb, merged.to(torch.int64) & 0xFFFFFFFF)) and bool(torch.equal(cb.to(torch.int32), counts))
    rows.append(("QGramFilter.merge, %d hits, interval %d -> %d diagonals" % (batch, INTERVAL, merged.numel()), batch, "hits", t_merge, t_bmerge, same))

    lines = ["q-gram index and filter on the device (nvbio_amd.qgram) beside torch library calls on the same data: %s" % torch.cuda.get_device_name(dev),
             "one unrecorded call, then %d calls between two device events: median [least, greatest] in ms" % a.reps, ""]
    lost = []
    for stage, items, unit, ours, base, same in rows:
        med, lo, hi = stat(ours)
        lines.append(stage)
        lines.append("  this library: %9.3f [%9.3f, %9.3f] ms   %.3e %s/s" % (med, lo, hi, items / (med * 1e-3), unit))
        if base is None:
            continue
        bmed, blo, bhi = stat(base)
        verdict = "wins" if hi < blo else "LOSES" if lo > bhi else "within the spread"
        if verdict == "LOSES":
            lost.append(stage)
        lines.append("  torch:        %9.3f [%9.3f, %9.3f] ms   torch / this library = %.2f   %s   same results: %s" % (bmed, blo, bhi, bmed / med, verdict, same))
    rate = recorded_line_rate()
    lines.append("")
    if rate:
        lines.append("sorted range queries: %.3e queries/s = %.3f of the chip's random-line rate recorded in profiles/mem/mem_time.txt (%.3e lines/s)" % (
            sorted_rate, sorted_rate / rate, rate))
    else:
        lines.append("sorted range queries: %.3e queries/s (no random-line rate found under profiles/mem/mem_time.txt)" % sorted_rate)
    lines.append("stages that lose to their baseline: %s" % (", ".join(lost) if lost else "none"))
    lines.append("(supposed, not traced kernel by kernel: a build is more than its baseline; it also enumerates the seeds, generates the q-grams and fills the 4^QL + 1 = %d words of the LUT, one" % (4 ** QL + 1))
    lines.append(" lower bound each -- at QL = %d more searches than the set index has q-grams --, and waits for the stream to learn n_unique)" % QL)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
