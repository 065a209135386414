"""From a FASTA file to the index files the loaders read -- what the reference's nvBWT tool (or `bwa index`) is needed for
otherwise.  The suffix sorting and the BWT run on the device (nvbio_amd.sufsort); parsing and file writing are
host work and go through the writers of nvbio_amd.io.

    python -m nvbio_amd.index ref.fa prefix [--sa-int K] [--no-reverse]

writes prefix.pac .wpac .ann .amb .bwt .sa and, unless --no-reverse, .rbwt .rsa (the index of the reversed text, which MEM seeding
and nvBowtie's reverse mapper use)."""
import gzip
import os

import numpy as np
import torch

from . import io
from . import sufsort

ANN_SEED = 11           # the seed BWA and nvBWT print into .ann


def hole_bases(first, count, seed=ANN_SEED):
    """The bases that replace the ambiguous symbols number first .. first + count - 1 of a reference (counted over the whole input,
    in order): base k = top two bits of splitmix64's output function applied to seed + (k + 1) * 0x9E3779B97F4A7C15 (Steele, Lea &
    Flood 2014) -- a counter-based generator, so any slice can be computed on its own."""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + (np.arange(first, first + count, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(62)).astype(np.uint8)


def read_fasta(path):
    """-> [(name, comment, sequence bytes as a uint8 array)] of a FASTA file, plain or gzip"""
    opener = gzip.open if path.endswith(".gz") else open
    records, chunks, head = [], [], None

    def flush():
        if head is not None:
            parts = head.split(None, 1)
            name = parts[0] if parts else ""
            records.append((name, parts[1] if len(parts) > 1 else "", np.frombuffer(b"".join(chunks), dtype=np.uint8)))

    with opener(path, "rb") as f:
        for line in f:
            if line.startswith(b">"):
                flush()
                head, chunks = line[1:].strip().decode(), []
            elif head is not None:
                chunks.append(line.strip())
    flush()
    return records


def _holes_of(codes, chars, offset):
    """runs of one ambiguous character -> [(genome offset, length, character)]"""
    amb = np.flatnonzero(codes > 3)
    if amb.size == 0:
        return []
    c = chars[amb]
    c = np.where((c >= 97) & (c <= 122), c - 32, c)            # 'n' and 'N' are one character
    start = np.ones(amb.size, dtype=bool)
    start[1:] = (amb[1:] != amb[:-1] + 1) | (c[1:] != c[:-1])
    first = np.flatnonzero(start)
    length = np.diff(np.append(first, amb.size))
    return [(int(offset + amb[s]), int(l), chr(int(c[s])).upper()) for s, l in zip(first, length)]


def encode_records(source):
    """source: a FASTA path or a list of (name, symbols) with symbols a string / bytes of letters or an array of codes 0..4.
    -> (text uint8 codes 0..3 with the holes filled, names, comments, lengths, holes)"""
    if isinstance(source, (str, os.PathLike)):
        records = read_fasta(os.fspath(source))
    else:
        records = []
        for name, sym in source:
            if isinstance(sym, str):
                sym = sym.encode()
            if isinstance(sym, (bytes, bytearray)):
                records.append((name, "", np.frombuffer(bytes(sym), dtype=np.uint8)))
            else:
                codes = np.asarray(sym, dtype=np.uint8)
                records.append((name, "", np.frombuffer(b"ACGTN", dtype=np.uint8)[np.minimum(codes, 4)]))
    if not records:
        raise ValueError("build_index: no sequence in the input")
    names, annos, lengths, holes, parts = [], [], [], [], []
    offset, n_amb = 0, 0
    for name, anno, chars in records:
        codes = io._NT4[chars]
        holes += _holes_of(codes, chars, offset)
        amb = np.flatnonzero(codes > 3)
        if amb.size:
            codes = codes.copy()
            codes[amb] = hole_bases(n_amb, amb.size)
            n_amb += amb.size
        names.append(name); annos.append(anno); lengths.append(int(codes.size)); parts.append(codes)
        offset += codes.size
    return np.concatenate(parts), names, annos, lengths, holes


def _write_one(prefix, bwt_ext, sa_ext, d_text, cum, sa_int):
    n = d_text.numel()
    words, primary, ssa, _ = sufsort.bwt(d_text, sa_int=sa_int)
    rounds = sufsort.last_rounds()
    io.write_bwt(prefix + bwt_ext, primary, cum, words.cpu().numpy().view(np.uint32), n)
    io.write_sa(prefix + sa_ext, primary, cum, ssa.cpu().numpy().view(np.uint32), n, sa_int)
    return primary, rounds


def build_index(source, prefix, sa_int=16, reverse=True, device="cuda"):
    """Build the FM-index of a reference on the device and write it as <prefix>.pac .wpac .ann .amb .bwt .sa (+ .rbwt .rsa of
    the reversed text when `reverse`), the files io.FMIndexDataDevice, io.load_genome, io.read_bns and the reference's loaders read.

    source: a FASTA path (plain or .gz, any number of records, upper or lower case) or a list of (name, symbols).  The records
    are laid end to end.  Every symbol other than ACGT is recorded as a hole in .amb and replaced by a base from hole_bases(), a
    counter-based generator seeded with the .ann seed (11).  nvBWT (like bwa) draws these bases from libc's rand48 instead, so the
    files of a genome that contains N are not byte-equal to nvBWT's; the files of an N-free genome are.
    The loaders accept only sa_int = 16 for .sa / .rsa (io.read_sa); other intervals are for callers that read the files themselves.
    -> dict(length, n_seqs, n_holes, primary, rprimary, rounds, rrounds)"""
    text, names, annos, lengths, holes = encode_records(source)
    n = int(text.size)
    if not 1 <= n <= sufsort.MAX_LENGTH:
        raise ValueError("build_index: the reference must hold between 1 and 2^32 - 2 symbols")
    d_text = torch.from_numpy(text).to(device)
    genome = sufsort._pack_text(d_text).cpu().numpy().view(np.uint32)
    io.write_pac(prefix + ".pac", n, genome)
    io.write_wpac(prefix + ".wpac", n, genome)
    io.write_bns(prefix, names, lengths, annos, holes, seed=ANN_SEED)
    cum = np.cumsum(np.bincount(text, minlength=4)[:4]).astype(np.uint32)
    out = dict(length=n, n_seqs=len(names), n_holes=len(holes), rprimary=None, rrounds=None)
    out["primary"], out["rounds"] = _write_one(prefix, ".bwt", ".sa", d_text, cum, sa_int)
    if reverse:
        out["rprimary"], out["rrounds"] = _write_one(prefix, ".rbwt", ".rsa", torch.flip(d_text, [0]), cum, sa_int)
    return out


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m nvbio_amd.index", description="FASTA -> FM-index files, built on the device")
    ap.add_argument("fasta")
    ap.add_argument("prefix")
    ap.add_argument("--sa-int", type=int, default=16)
    ap.add_argument("--no-reverse", action="store_true")
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args(argv)
    r = build_index(a.fasta, a.prefix, sa_int=a.sa_int, reverse=not a.no_reverse, device=a.device)
    print("%s: %d symbols in %d sequences, %d holes; primary %d, unresolved per round %s%s" % (
        a.prefix, r["length"], r["n_seqs"], r["n_holes"], r["primary"], r["rounds"],
        "" if r["rprimary"] is None else "; reverse primary %d, unresolved per round %s" % (r["rprimary"], r["rrounds"])))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
