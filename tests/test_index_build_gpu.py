"""nvbio_amd.index.build_index: from a FASTA file to the .pac .wpac .ann .amb .bwt .sa .rbwt .rsa files, read back through the readers
of nvbio_amd.io and searched through io.FMIndexDataDevice."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import nvbio_amd as nvb
from nvbio_amd import index as IDX
from nvbio_amd import io as nio
from oracle import pyoracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def letters(codes, lower=False):
    s = "".join("ACGT"[c] for c in codes)
    return s.lower() if lower else s


def write_fasta(path, records, width=60):
    opener = gzip.open if path.endswith(".gz") else open
    with opener(path, "wt") as f:
        for head, seq in records:
            f.write(">%s\n" % head)
            for s in range(0, len(seq), width):
                f.write(seq[s:s + width] + "\n")


@pytest.fixture(scope="module")
def three_records():
    """chr1: 3 000 bases, lower case from 500 to 900, a run of 37 N at 1 200; tiny: 11 bases; chr2: 2 017 bases"""
    rng = np.random.default_rng(4242)
    a, b, c = rng.integers(0, 4, 3000), rng.integers(0, 4, 11), rng.integers(0, 4, 2017)
    s1 = letters(a[:500]) + letters(a[500:900], lower=True) + letters(a[900:1200]) + "N" * 37 + letters(a[1237:])
    return [("chr1 first record", s1), ("tiny", letters(b)), ("chr2", letters(c))], (a, b, c)


def test_fasta_to_index_files_and_back(cuda, tmp_path, three_records):
    records, (a, b, c) = three_records
    fasta = str(tmp_path / "ref.fa")
    write_fasta(fasta, records)
    prefix = str(tmp_path / "ref")
    info = IDX.build_index(fasta, prefix, device=cuda)
    n = 3000 + 11 + 2017
    assert info["length"] == n and info["n_seqs"] == 3 and info["n_holes"] == 1

    # .ann / .amb: names, comments, offsets, lengths, the hole
    bns = nio.read_bns(prefix)
    assert (bns.l_pac, bns.seed, bns.names, bns.annos) == (n, 11, ["chr1", "tiny", "chr2"], ["first record", "", ""])
    assert (bns.offsets, bns.lengths, bns.n_ambs, bns.holes) == ([0, 3000, 3011], [3000, 11, 2017], [1, 0, 0], [(1200, 37, "N")])

    # .pac / .wpac: what went in, the hole filled by the documented generator
    text = np.concatenate([a, b, c]).astype(np.uint8)
    text[1200:1237] = IDX.hole_bases(0, 37)
    for length, words in (nio.read_wpac(prefix + ".wpac"), nio.read_pac(prefix + ".pac")):
        assert length == n and (O.unpack(words, 0, n, 2, True) == text).all()

    # .bwt / .sa / .rbwt / .rsa: the oracle's index of that text and of its reversal
    for bwt_ext, sa_ext, t in ((".bwt", ".sa", text), (".rbwt", ".rsa", np.ascontiguousarray(text[::-1]))):
        host = O.FMIndex(t)
        primary, cum, length, words = nio.read_bwt(prefix + bwt_ext)
        assert (primary, length) == (host.primary, n) and cum.tolist() == np.cumsum(np.bincount(t, minlength=4)).tolist()
        assert (O.unpack(words, 0, n, 2, True) == host.bwt).all()
        assert (nio.read_sa(prefix + sa_ext, n, primary) == host.ssa).all()

    # the loader takes the prefix; seeds cut from the text are found where the text equals them
    data = nio.FMIndexDataDevice(prefix, device=cuda, hbm_rich=False)
    fmi, rfmi = data.index(), data.rindex()
    rng = np.random.default_rng(7)
    pos = rng.integers(0, n - 22, 2000)
    hs = O.StringSet.from_lists([text[q:q + 22] for q in pos], 2, True)
    ds = nvb.PackedStringSet.from_host(hs.words, 2, True, hs.begin, hs.length, device=cuda)
    rg = u32(nvb.match(fmi, ds)).astype(np.int64)
    assert (rg[:, 0] <= rg[:, 1]).all()                                   # every seed occurs
    for rows in (rg[:, 0], rg[:, 1]):
        at = u32(nvb.locate(fmi, torch.from_numpy(rows.astype(np.uint32).view(np.int32)).to(cuda))).astype(np.int64)
        assert all((text[p:p + 22] == text[q:q + 22]).all() for p, q in zip(at, pos))

    # MEM seeding on the pair of indices: a copied 40-mer is one MEM, its range the match range
    pos = rng.integers(0, n - 40, 64)
    hs = O.StringSet.from_lists([text[q:q + 40] for q in pos], 2, True)
    ds = nvb.PackedStringSet.from_host(hs.words, 2, True, hs.begin, hs.length, device=cuda)
    flt = nvb.MEMFilter()
    flt.rank(fmi, rfmi, ds, min_span=40)
    mems = u32(flt.ranges)
    assert mems.shape[0] == 64 and (mems[:, 2] == np.arange(64)).all() and (mems[:, 3] == 40 << 16).all()
    assert (mems[:, :2] == u32(nvb.match(fmi, ds))).all()


def test_n_free_files_are_byte_equal_to_the_existing_writers(cuda, tmp_path):
    rng = np.random.default_rng(99)
    text = rng.integers(0, 4, 4099, dtype=np.uint8)
    text[700:1400] = text[0:700]                                          # a repeat, so the doubling rounds run
    prefix, ref = str(tmp_path / "dev"), str(tmp_path / "host")
    info = IDX.build_index([("only", text)], prefix, device=cuda)
    assert info["n_holes"] == 0 and len(info["rounds"]) > 1
    nio.save_fmindex(ref, O.FMIndex(text))
    nio.save_fmindex(ref, O.FMIndex(np.ascontiguousarray(text[::-1])), reverse=True)
    for ext in (".bwt", ".sa", ".rbwt", ".rsa"):
        assert open(prefix + ext, "rb").read() == open(ref + ext, "rb").read(), ext
    assert nio.read_bns(prefix).holes == []


def test_command_line(cuda, tmp_path, three_records):
    records, _ = three_records
    fasta = str(tmp_path / "ref.fa.gz")
    write_fasta(fasta, records)
    prefix = str(tmp_path / "cli")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "nvbio_amd.index", fasta, prefix, "--no-reverse"], env=env, cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "5028 symbols in 3 sequences, 1 holes" in r.stdout
    assert all(os.path.exists(prefix + e) for e in (".pac", ".wpac", ".ann", ".amb", ".bwt", ".sa"))
    assert not os.path.exists(prefix + ".rbwt") and not os.path.exists(prefix + ".rsa")
    # the same bytes as the library call on the plain file
    plain = str(tmp_path / "ref.fa")
    write_fasta(plain, records)
    IDX.build_index(plain, str(tmp_path / "lib"), reverse=False, device=cuda)
    for e in (".pac", ".wpac", ".ann", ".amb", ".bwt", ".sa"):
        assert open(prefix + e, "rb").read() == open(str(tmp_path / "lib") + e, "rb").read(), e
