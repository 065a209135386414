#!/usr/bin/env python3
"""Times index construction on the device: nvbio_amd.sufsort.build_fm_index (nvbio_amd/csrc/sufsort.hip) against
nvbio_amd.workloads.build_fm_index (prefix doubling on whole-array torch sorts) on the same device text, and writes the figures to a file.

Inputs: (a) i.i.d. 2^28 symbols; (b) the bench's i.i.d. 3 Gbp genome (bench.py fm_legs: seed 0x5EED0003); (c) the repeat-rich 3 Gbp genome
of tools/nvbowtie_3gbp.py (60 % diverged copies of three repeat families, seed 0x5EED0009).

Every step -- one builder on one input -- is a child process of its own under its own time limit; a child that fails or runs out of time
ends the run (nothing more is started on the device), and what was measured so far is written.  A child draws the text, builds a small
index first (library start-up), then times --reps (3) builds of the text, each between two device synchronisations with the host clock:
every time is listed (the first build of a process also pays for the first use of its scratch), and the median is compared.  The child of
the new builder then checks its result without the full oracle: the suffix array (built again, untimed, to be kept) is a permutation of
0..n; T[SA[r]:] <= T[SA[r+1]:] on --rows (1 M) sampled adjacent rows, compared to 256 symbols; locate(match(seed)) returns a position
where the text equals the seed for --seeds (100 k) 22-mers cut from the text.  It reports the sorting rounds and the suffixes left
unresolved after each, and the bytes of scratch.  If the old builder raises, the message is recorded and only the new one is timed.

Usage: python tools/sufsort_time.py [--inputs a,b,c] [--out profiles/sufsort/sufsort_time.txt]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

INPUTS = {
    "a": dict(name="i.i.d. 2^28", n=1 << 28, kind="iid", seed=0x5EED0003, limit=240),
    "b": dict(name="i.i.d. 3 Gbp (the bench's genome)", n=3_000_000_000, kind="iid", seed=0x5EED0003, limit=400),
    "c": dict(name="repeat-rich 3 Gbp (tools/nvbowtie_3gbp.py)", n=3_000_000_000, kind="repeats", seed=0x5EED0009, limit=400),
}


def make_text(spec, n, dev):
    import torch
    if spec["kind"] == "repeats":
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import nvbowtie_3gbp as T
        return T.make_genome(n, 0.6, spec["seed"], dev)[0]
    g = torch.Generator(device=dev)
    g.manual_seed(spec["seed"])
    return torch.randint(0, 4, (n,), dtype=torch.uint8, generator=g, device=dev)


def check_result(text, fmi, rows, seeds, out):
    import torch
    import nvbio_amd as nvb
    from nvbio_amd import sufsort as S, workloads as W
    from nvbio_amd.strings import PackedStringSet
    n, dev = text.numel(), text.device
    words = S._pack_text(text)
    sa = S.suffix_sort((words, n, True))
    del words
    # a permutation of 0..n
    seen = torch.zeros(n + 1, dtype=torch.bool, device=dev)
    for s in range(0, n + 1, 1 << 29):
        seen[sa[s:s + (1 << 29)].to(torch.int64) & 0xFFFFFFFF] = True
    out["sa_is_permutation"] = bool(seen.all().item()) and int(sa[0].item()) & 0xFFFFFFFF == n
    del seen
    # sampled adjacent rows are in order, to 256 symbols; past the end sorts first
    g = torch.Generator(device=dev); g.manual_seed(7)
    ok, span = True, torch.arange(256, device=dev, dtype=torch.int64).unsqueeze(0)
    for c0 in range(0, rows, 1 << 18):
        r = torch.randint(0, n, (min(1 << 18, rows - c0),), generator=g, device=dev)
        def window(row):
            idx = (sa[row].to(torch.int64) & 0xFFFFFFFF).unsqueeze(1) + span
            return torch.where(idx < n, text[idx.clamp(max=n - 1)].to(torch.int16), torch.full_like(idx, -1, dtype=torch.int16))
        a, b = window(r), window(r + 1)
        diff = a != b
        first = torch.argmax(diff.to(torch.uint8), dim=1, keepdim=True)
        ok = ok and bool((~diff.any(1) | (a.gather(1, first) < b.gather(1, first)).squeeze(1)).all().item())
    out["sampled_rows_in_order"], out["sampled_rows"] = ok, rows
    del sa
    # seeds cut from the text are found where the text equals them
    pos = torch.randint(0, n - 22, (seeds,), generator=g, device=dev)
    sym = text[pos.unsqueeze(1) + torch.arange(22, device=dev).unsqueeze(0)]
    ds = PackedStringSet(W._pack_chunked(sym.reshape(-1), 2, True), 2, True, torch.arange(seeds, dtype=torch.int64, device=dev) * 22, None, 22)
    rg = nvb.match(fmi, ds)
    at = nvb.locate(fmi, rg[:, 0].contiguous()).to(torch.int64) & 0xFFFFFFFF
    found = (rg[:, 0].to(torch.int64) & 0xFFFFFFFF) <= (rg[:, 1].to(torch.int64) & 0xFFFFFFFF)
    hit = (text[at.clamp(max=n - 22).unsqueeze(1) + torch.arange(22, device=dev).unsqueeze(0)] == sym).all(1)
    out["seeds_located"], out["seeds"] = int((found & hit).sum().item()), seeds


def child(a):
    import torch
    import nvbio_amd as nvb
    from nvbio_amd import sufsort as S, workloads as W
    spec = INPUTS[a.child]
    n = a.n or spec["n"]
    dev = torch.device("cuda:0")
    out = dict(input=a.child, builder=a.builder, n=n)
    build = S.build_fm_index if a.builder == "new" else W.build_fm_index
    build(torch.randint(0, 4, (1 << 20,), dtype=torch.uint8, device=dev))           # start-up
    text = make_text(spec, n, dev)
    torch.cuda.synchronize()
    try:
        times, fmi = [], None
        for _ in range(a.reps):
            del fmi
            t0 = time.perf_counter()
            fmi = build(text)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        out["times"], out["seconds"] = times, sorted(times)[len(times) // 2]
        out["primary"] = fmi.primary
    except RuntimeError as e:
        out["raised"] = str(e).splitlines()[0][:200]
        print("RESULT " + json.dumps(out), flush=True)
        return 0
    out["peak_GB"] = torch.cuda.max_memory_allocated(dev) / 1e9
    if a.builder == "new":
        out["rounds"] = S.last_rounds()
        out["temp_bytes"] = int(nvb.lib().nvbio_hip_bwt_temp_bytes(n))
        check_result(text, fmi, a.rows, a.seeds, out)
    print("RESULT " + json.dumps(out), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="a,b,c")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sufsort", "sufsort_time.txt"))
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--seeds", type=int, default=100_000)
    ap.add_argument("--n", type=int, default=0, help="override the length of every input (for trying the tool out)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--child", default="")
    ap.add_argument("--builder", default="new")
    a = ap.parse_args()
    if a.child:
        return child(a)
    lines, results, stopped = [], [], None
    for key in a.inputs.split(","):
        spec = INPUTS[key]
        for builder in ("new", "old"):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", key, "--builder", builder, "--rows", str(a.rows), "--seeds", str(a.seeds), "--n", str(a.n), "--reps", str(a.reps)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=spec["limit"])
                rc, text = r.returncode, r.stdout + r.stderr
            except subprocess.TimeoutExpired as e:
                rc, text = 124, (e.stdout or b"").decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or "")
            res = [json.loads(ln[7:]) for ln in text.splitlines() if ln.startswith("RESULT ")]
            if rc != 0 or not res:
                stopped = "(%s) %s builder: the child ended with status %d; nothing more was started\n%s" % (key, builder, rc, text[-1500:])
                break
            results.append(res[0])
            print("(%s) %s: %s" % (key, builder, "raised" if "raised" in res[0] else "%.3f s" % res[0]["seconds"]), flush=True)
        if stopped:
            break
    by = {(r["input"], r["builder"]): r for r in results}
    lines.append("index construction on the device: nvbio_amd.sufsort.build_fm_index (new) against nvbio_amd.workloads.build_fm_index (old)")
    lines.append("%d timed builds per builder and input in a process of its own, host clock between two device synchronisations; every time is listed, medians are compared" % a.reps)
    for key in a.inputs.split(","):
        new, old = by.get((key, "new")), by.get((key, "old"))
        if not new:
            continue
        lines.append("")
        lines.append("(%s) %s, n = %d" % (key, INPUTS[key]["name"], new["n"]))
        fmt = lambda r: " ".join("%.3f" % t for t in r["times"])
        lines.append("  new: %s s (median %.3f)   peak device memory %.1f GB   scratch %d bytes (%.1f bytes a symbol)" % (fmt(new), new["seconds"], new["peak_GB"], new["temp_bytes"], new["temp_bytes"] / new["n"]))
        lines.append("  rounds: %d   unresolved suffixes after each: %s" % (len(new["rounds"]), new["rounds"]))
        lines.append("  checks: SA is a permutation: %s   %d sampled adjacent rows in order: %s   seeds located: %d of %d" % (
            new["sa_is_permutation"], new["sampled_rows"], new["sampled_rows_in_order"], new["seeds_located"], new["seeds"]))
        if old and "raised" in old:
            lines.append("  old: raised \"%s\"" % old["raised"])
        elif old:
            lines.append("  old: %s s (median %.3f)   peak device memory %.1f GB   primary equal: %s   new / old time: %.2f" % (
                fmt(old), old["seconds"], old["peak_GB"], old["primary"] == new["primary"], new["seconds"] / old["seconds"]))
    if stopped:
        lines += ["", stopped]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 1 if stopped else 0


if __name__ == "__main__":
    sys.exit(main())
