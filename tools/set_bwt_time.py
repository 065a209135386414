#!/usr/bin/env python3
"""Times the string-set suffix sorter and BWT on the device: nvbio_amd.sufsort.set_suffix_sort / set_bwt (the set entries of
nvbio_amd/csrc/sufsort.hip) on a read set, against the plain nvbio_amd.sufsort.suffix_sort of an i.i.d. text with the same
number of suffixes, timed in the same run, and writes the figures to a file.

Inputs: (a) 10 M i.i.d. reads of 100 bp; (b) 10 M reads of 100 bp drawn at 30x from a 33 Mbp i.i.d. genome, whose overlaps force doubling
rounds.  The yardstick (p) is an i.i.d. text of as many symbols as the read sets have slots.

Every step -- one input -- is a child process of its own under its own time limit; a child that fails or runs out of time ends the run
(nothing more is started on the device), and what was measured so far is written.  A child draws its input, makes a small call first
(library start-up), then times --reps (3) calls, each between two device synchronisations with the host clock: every time is listed (the
first call of a process also pays for the first use of its scratch), and the median is compared.  A set child then checks its result
without the full oracle: the sorted global indices are a permutation of 0..n_suffixes-1 whose first n_strings rows are the empty suffixes in
id order; on --rows (1 M) sampled adjacent rows the suffixes are in order (compared to 128 symbols within their strings, equal ones by
string id); the BWT holds 255 on exactly the n_strings dollar rows, which ascend and name each string once, and every symbol as often as the
reads do.  It reports the sorting rounds with the slots left unresolved after each, and the bytes of scratch.

Usage: python tools/set_bwt_time.py [--inputs a,b,p] [--out profiles/sufsort/set_bwt_time.txt]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

READ_LEN = 100
INPUTS = {
    "a": dict(name="10 M i.i.d. reads of 100 bp", reads=10_000_000, genome=0, seed=0x5EED0011, limit=300),
    "b": dict(name="10 M reads of 100 bp at 30x from a 33 Mbp i.i.d. genome", reads=10_000_000, genome=33_333_333, seed=0x5EED0012, limit=300),
    "p": dict(name="plain suffix_sort of an i.i.d. text with as many suffixes", reads=10_000_000, genome=0, seed=0x5EED0013, limit=300),
}


def make_reads(spec, n_reads, dev):
    """-> uint8 [n_reads, READ_LEN] on the device"""
    import torch
    g = torch.Generator(device=dev)
    g.manual_seed(spec["seed"])
    if not spec["genome"]:
        return torch.randint(0, 4, (n_reads, READ_LEN), dtype=torch.uint8, generator=g, device=dev)
    glen = max(2 * READ_LEN, int(spec["genome"] * (n_reads / spec["reads"])))             # the coverage stays when --reads shrinks the set
    genome = torch.randint(0, 4, (glen,), dtype=torch.uint8, generator=g, device=dev)
    out = torch.empty((n_reads, READ_LEN), dtype=torch.uint8, device=dev)
    span = torch.arange(READ_LEN, device=dev)
    for s in range(0, n_reads, 1 << 22):
        pos = torch.randint(0, glen - READ_LEN, (min(1 << 22, n_reads - s),), generator=g, device=dev)
        out[s:s + pos.numel()] = genome[pos.unsqueeze(1) + span]
    return out


def make_set(reads):
    import torch
    from nvbio_amd import sufsort as S
    from nvbio_amd.strings import PackedStringSet
    n_reads, dev = reads.shape[0], reads.device
    words = S._pack_text(reads.reshape(-1))
    begin = torch.arange(n_reads, dtype=torch.int64, device=dev) * READ_LEN
    length = torch.full((n_reads,), READ_LEN, dtype=torch.int32, device=dev)
    return PackedStringSet(words, 2, True, begin, length)


def check_result(reads, ds, bwt_out, rows, out):
    import torch
    from nvbio_amd import sufsort as S
    n_reads, dev = reads.shape[0], reads.device
    n = n_reads * (READ_LEN + 1)
    suffixes, string_ids, cum = S.set_suffix_sort(ds)
    suffixes = suffixes.to(torch.int64) & 0xFFFFFFFF
    seen = torch.zeros(n, dtype=torch.bool, device=dev)
    seen[suffixes] = True
    expect_first = (torch.arange(n_reads, dtype=torch.int64, device=dev) + 1) * (READ_LEN + 1) - 1
    out["is_permutation"] = bool(seen.all().item())
    out["empty_suffixes_first"] = bool(torch.equal(suffixes[:n_reads], expect_first))
    del seen
    g = torch.Generator(device=dev); g.manual_seed(7)
    ok, span = True, torch.arange(128, device=dev, dtype=torch.int64).unsqueeze(0)
    flat = reads.reshape(-1)
    for c0 in range(0, rows, 1 << 18):
        r = torch.randint(0, n - 1, (min(1 << 18, rows - c0),), generator=g, device=dev)
        def window(row):
            gidx = suffixes[row]
            sid, p = gidx // (READ_LEN + 1), gidx % (READ_LEN + 1)
            at = p.unsqueeze(1) + span
            sym = flat[(sid.unsqueeze(1) * READ_LEN + at.clamp(max=READ_LEN - 1))].to(torch.int16)
            return torch.where(at < READ_LEN, sym, torch.full_like(sym, -1)), sid
        (a, sa), (b, sb) = window(r), window(r + 1)
        diff = a != b
        first = torch.argmax(diff.to(torch.uint8), dim=1, keepdim=True)
        ordered = torch.where(diff.any(1), (a.gather(1, first) < b.gather(1, first)).squeeze(1), sa < sb)
        ok = ok and bool(ordered.all().item())
    out["sampled_rows_in_order"], out["sampled_rows"] = ok, rows
    bwt, drows, dids, _ = bwt_out
    drows64 = drows.to(torch.int64) & 0xFFFFFFFF
    hist = torch.bincount(bwt.to(torch.int64), minlength=256)
    want = torch.bincount(flat.to(torch.int64), minlength=4)
    out["bwt_symbol_counts_equal"] = bool(torch.equal(hist[:4], want)) and int(hist[255].item()) == n_reads and int(hist[4:255].sum().item()) == 0
    out["dollar_rows_ok"] = (bool((drows64[1:] > drows64[:-1]).all().item()) and bool((bwt[drows64] == 255).all().item())
                             and bool(torch.equal(torch.sort(dids.to(torch.int64)).values, torch.arange(n_reads, device=dev))))


def child(a):
    import torch
    import nvbio_amd as nvb
    from nvbio_amd import sufsort as S
    spec = INPUTS[a.child]
    n_reads = a.reads or spec["reads"]
    n = n_reads * (READ_LEN + 1)
    dev = torch.device("cuda:0")
    out = dict(input=a.child, n_strings=n_reads, n=n)
    median = lambda t: sorted(t)[len(t) // 2]
    if a.child == "p":
        S.suffix_sort(torch.randint(0, 4, (1 << 20,), dtype=torch.uint8, device=dev))
        g = torch.Generator(device=dev); g.manual_seed(spec["seed"])
        text = (S._pack_text(torch.randint(0, 4, (n,), dtype=torch.uint8, generator=g, device=dev)), n, True)
        torch.cuda.synchronize()
        times = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            sa = S.suffix_sort(text)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
            del sa
        out["sort_times"], out["sort_seconds"], out["rounds"] = times, median(times), S.last_rounds()
        out["temp_bytes"] = int(nvb.lib().nvbio_hip_suffix_sort_temp_bytes(n))
        print("RESULT " + json.dumps(out), flush=True)
        return 0
    S.set_bwt([torch.randint(0, 4, (50,), dtype=torch.uint8, device=dev) for _ in range(64)])        # start-up
    reads = make_reads(spec, n_reads, dev)
    ds = make_set(reads)
    torch.cuda.synchronize()
    sort_times, bwt_times, res = [], [], None
    for _ in range(a.reps):
        t0 = time.perf_counter()
        r = S.set_suffix_sort(ds)
        torch.cuda.synchronize()
        sort_times.append(time.perf_counter() - t0)
        del r
    for _ in range(a.reps):
        del res
        t0 = time.perf_counter()
        res = S.set_bwt(ds)
        torch.cuda.synchronize()
        bwt_times.append(time.perf_counter() - t0)
    out["sort_times"], out["sort_seconds"] = sort_times, median(sort_times)
    out["bwt_times"], out["bwt_seconds"] = bwt_times, median(bwt_times)
    out["rounds"] = S.last_rounds()
    out["temp_bytes"] = int(nvb.lib().nvbio_hip_set_bwt_temp_bytes(n, n_reads))
    out["sort_temp_bytes"] = int(nvb.lib().nvbio_hip_set_suffix_sort_temp_bytes(n, n_reads))
    out["peak_GB"] = torch.cuda.max_memory_allocated(dev) / 1e9
    check_result(reads, ds, res, a.rows, out)
    print("RESULT " + json.dumps(out), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="a,b,p")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sufsort", "set_bwt_time.txt"))
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reads", type=int, default=0, help="override the number of reads of every input (for trying the tool out)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.child:
        return child(a)
    results, stopped = {}, None
    for key in a.inputs.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", key, "--rows", str(a.rows), "--reads", str(a.reads), "--reps", str(a.reps)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=INPUTS[key]["limit"])
            rc, text = r.returncode, r.stdout + r.stderr
        except subprocess.TimeoutExpired as e:
            rc, text = 124, (e.stdout or b"").decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or "")
        res = [json.loads(ln[7:]) for ln in text.splitlines() if ln.startswith("RESULT ")]
        if rc != 0 or not res:
            stopped = "(%s): the child ended with status %d; nothing more was started\n%s" % (key, rc, text[-1500:])
            break
        results[key] = res[0]
        print("(%s): sort %.3f s" % (key, res[0]["sort_seconds"]), flush=True)
    fmt = lambda t: " ".join("%.3f" % x for x in t)
    lines = ["suffix sort and BWT of a string set on the device: nvbio_amd.sufsort.set_suffix_sort / set_bwt against the plain suffix_sort",
             "%d timed calls per function and input in a process of its own, host clock between two device synchronisations; every time is listed, medians are compared" % a.reps]
    plain = results.get("p")
    for key in a.inputs.split(","):
        r = results.get(key)
        if not r:
            continue
        lines.append("")
        if key == "p":
            lines.append("(p) %s, n = %d" % (INPUTS[key]["name"], r["n"]))
            lines.append("  suffix_sort: %s s (median %.3f, %.3f ns a suffix)   scratch %d bytes (%.1f bytes a symbol)   rounds: %s" % (
                fmt(r["sort_times"]), r["sort_seconds"], 1e9 * r["sort_seconds"] / r["n"], r["temp_bytes"], r["temp_bytes"] / r["n"], r["rounds"]))
            continue
        lines.append("(%s) %s: %d strings, n_suffixes = %d" % (key, INPUTS[key]["name"], r["n_strings"], r["n"]))
        lines.append("  set_suffix_sort: %s s (median %.3f, %.3f ns a slot)   scratch %d bytes (%.1f bytes a slot)" % (
            fmt(r["sort_times"]), r["sort_seconds"], 1e9 * r["sort_seconds"] / r["n"], r["sort_temp_bytes"], r["sort_temp_bytes"] / r["n"]))
        lines.append("  set_bwt:         %s s (median %.3f, %.3f ns a slot)   scratch %d bytes (%.1f bytes a slot)   peak device memory %.1f GB" % (
            fmt(r["bwt_times"]), r["bwt_seconds"], 1e9 * r["bwt_seconds"] / r["n"], r["temp_bytes"], r["temp_bytes"] / r["n"], r["peak_GB"]))
        lines.append("  rounds: %d   unresolved slots after each: %s" % (len(r["rounds"]), r["rounds"]))
        lines.append("  checks: permutation: %s   empty suffixes first, by id: %s   %d sampled adjacent rows in order: %s   BWT symbol counts: %s   dollar rows: %s" % (
            r["is_permutation"], r["empty_suffixes_first"], r["sampled_rows"], r["sampled_rows_in_order"], r["bwt_symbol_counts_equal"], r["dollar_rows_ok"]))
        if plain:
            lines.append("  set_suffix_sort / plain suffix_sort, time per suffix: %.2f" % ((r["sort_seconds"] / r["n"]) / (plain["sort_seconds"] / plain["n"])))
    if stopped:
        lines += ["", stopped]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 1 if stopped else 0


if __name__ == "__main__":
    sys.exit(main())
