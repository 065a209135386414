"""The host half of nvbio_amd.index (no GPU): FASTA parsing, hole detection and the documented hole generator."""
import gzip

import numpy as np

from nvbio_amd import index as IDX


def test_records_holes_and_case(tmp_path):
    rng = np.random.default_rng(3)
    a = rng.integers(0, 4, 100)
    seq = "".join("ACGT"[c] for c in a[:30]) + "NNNnnRR" + "".join("acgt"[c] for c in a[37:])
    for name, opener in (("a.fa", open), ("a.fa.gz", gzip.open)):
        path = str(tmp_path / name)
        with opener(path, "wt") as f:
            f.write(">x y z\n")
            for s in range(0, len(seq), 13):
                f.write(seq[s:s + 13] + "\n")
            f.write(">t\nACGT\n\n")
        text, names, annos, lengths, holes = IDX.encode_records(path)
        assert (names, annos, lengths) == (["x", "t"], ["y z", ""], [100, 4])
        assert holes == [(30, 5, "N"), (35, 2, "R")]                      # 'n' and 'N' are one character; a run ends where it changes
        assert (text[:30] == a[:30]).all() and (text[37:100] == a[37:]).all() and text[100:].tolist() == [0, 1, 2, 3]
        assert (text[30:37] == IDX.hole_bases(0, 7)).all() and text.max() <= 3


def test_hole_generator_is_a_function_of_the_counter():
    whole = IDX.hole_bases(0, 5000)
    assert (IDX.hole_bases(1234, 100) == whole[1234:1334]).all()
    assert whole[:8].tolist() == IDX.hole_bases(0, 8, seed=IDX.ANN_SEED).tolist()
    assert sorted(np.unique(whole).tolist()) == [0, 1, 2, 3]
    assert abs(np.bincount(whole, minlength=4) / 5000.0 - 0.25).max() < 0.03       # four sigma of a fair base at 5 000 draws is 0.024
    assert not (IDX.hole_bases(0, 64, seed=12) == whole[:64]).all()


def test_list_source_and_holes_do_not_span_records():
    text, names, _, lengths, holes = IDX.encode_records([("p", "ACNN"), ("q", np.array([4, 4, 0, 1], dtype=np.uint8))])
    assert (names, lengths) == (["p", "q"], [4, 4])
    assert holes == [(2, 2, "N"), (4, 2, "N")]
    assert text[[0, 1, 6, 7]].tolist() == [0, 1, 0, 1]
