"""Alphabets wider than DNA: the reference's 24-letter protein alphabet (nvbio/strings/alphabet.h, PROTEIN), 8 bits a symbol in its
packed vectors and 5 bits of information: symbol k is letter k of PROTEIN_LETTERS, and any other character encodes as X."""
import numpy as np

PROTEIN_LETTERS = "ACDEFGHIKLMNOPQRSTVWYBZX"
PROTEIN_SYMBOL_SIZE = 8       # AlphabetTraits<PROTEIN>::SYMBOL_SIZE
PROTEIN_SYMBOL_COUNT = 24

_ENCODE = np.full(256, PROTEIN_LETTERS.index("X"), dtype=np.uint8)
for _k, _ch in enumerate(PROTEIN_LETTERS):
    _ENCODE[ord(_ch)] = _k
_DECODE = np.full(256, ord("X"), dtype=np.uint8)
_DECODE[:PROTEIN_SYMBOL_COUNT] = np.frombuffer(PROTEIN_LETTERS.encode(), dtype=np.uint8)


def encode(string):
    """the protein symbols of a str / bytes: a uint8 array (from_string<PROTEIN>)"""
    raw = string.encode("latin-1") if isinstance(string, str) else bytes(string)
    return _ENCODE[np.frombuffer(raw, dtype=np.uint8)]


def decode(symbols):
    """the letters of an array of protein symbols: a str (to_string<PROTEIN>); a symbol above 23 reads as X"""
    return _DECODE[np.asarray(symbols, dtype=np.uint8)].tobytes().decode("latin-1")
