"""The LDS substitution table of the pair kernel's PF_SUBLDS form (nvbio_amd/csrc/banded_gotoh_pair.h, "Where the substitution comes
from"), in numpy: the table's fill, the row words a 16-row block builds from both jobs' pattern nibbles, the column words it builds from
both jobs' text symbols, and the index their xor gives.  For all 16 x 16 x 4 x 4 combinations of (nibble A, nibble B, symbol A,
symbol B), at every row of a block, the word the form reads equals the word the lookup form computes,
v_perm_b32(s_tab[nibble B], s_tab[nibble A], selector), under every scheme of the literal form's GPU test.  The layout's condition is
asserted too: the sixteen entries two A/C/G/T codes reach lie in sixteen different LDS banks.  No GPU."""
import numpy as np
import pytest

from test_banded_pair_const_gpu import SCHEMES

SEL_BASE = 0x0C040C00
U32 = np.uint32


def score_bytes(scheme):
    """the column frame's match and mismatch bytes, 32 (s - G_o) + G"""
    match, mismatch, go, ge = scheme
    sm, sx = (match - go) * 32 - ge * 32, (mismatch - go) * 32 - ge * 32
    assert 0 <= sx <= 255 and 0 <= sm <= 255
    return sm, sx


def s_tab(scheme):
    """the lookup form's table: by pattern symbol q, entry v = the match byte where v == q, the mismatch byte elsewhere"""
    sm, sx = score_bytes(scheme)
    t = np.full(16, sx * 0x01010101, np.uint64)
    for q in range(4):
        t[q] = (int(t[q]) & ~(0xFF << (8 * q))) | (sm << (8 * q))
    return t.astype(U32)


def v_perm_b32(s0, s1, sel):
    """byte k of the result: selector byte 0 ... 3 takes that byte of s1, 4 ... 7 that byte of s0, 0x0C is zero"""
    src = (int(s0) << 32) | int(s1)
    out = 0
    for k in range(4):
        b = (sel >> (8 * k)) & 0xFF
        assert b < 8 or b == 0x0C
        out |= (0 if b == 0x0C else (src >> (8 * b)) & 0xFF) << (8 * k)
    return out


def sub_code_a(index):
    return (index & 3) | ((index >> 6) << 2)


def sub_code_b(index):
    return (index >> 2) & 15


def s_sub(scheme):
    """the kernel's fill of the 256 words"""
    sm, sx = score_bytes(scheme)
    k = np.arange(256)
    return (np.where(sub_code_a(k) == 0, sm, sx) | (np.where(sub_code_b(k) == 0, sm, sx) << 16)).astype(U32)


def bfi(mask, a, b):
    return (a & mask) | (b & ~mask & 0xFFFFFFFF)


def row_words(PA, PB):
    """sub_row_words: byte k of RE / RO is the row word of row 2 k / 2 k + 1, from the block's nibbles (row r's at bit 4 r)"""
    RE = RO = 0
    for h in range(2):
        a, b = (PA >> (32 * h)) & 0xFFFFFFFF, (PB >> (32 * h)) & 0xFFFFFFFF
        re = bfi(0x03030303, a, bfi(0x3C3C3C3C, (b << 2) & 0xFFFFFFFF, (a << 4) & 0xFFFFFFFF))
        ro = bfi(0x03030303, a >> 4, bfi(0x3C3C3C3C, b >> 2, a))
        RE |= re << (32 * h)
        RO |= ro << (32 * h)
    return RE, RO


def row_word(RE, RO, r):
    """PairRows::run: row r's word as a byte offset"""
    k = r >> 1
    zw = ((RO if r & 1 else RE) >> (32 * (k >> 2))) & 0xFFFFFFFF
    return (zw << 2) & 0x3FC if k & 3 == 0 else (zw >> (8 * (k & 3) - 2)) & 0x3FC


def column_word(TA, TB, r):
    """the block's entering column word of row r as a byte offset, from the two jobs' 16 text symbols (symbol r at bit 2 r)"""
    XT = (bfi(0x33333333, TA, (TB << 2) & 0xFFFFFFFF), bfi(0x33333333, TA >> 2, TB))
    k, xw = r >> 1, XT[r & 1]
    return (xw << 2) & 0x3C if k == 0 else (xw >> (4 * k - 2)) & 0x3C


def first_column_word(TA, TB, j):
    """the ring's words before row 0"""
    return (((TA >> (2 * j)) & 3) | (((TB >> (2 * j)) & 3) << 2)) << 2


@pytest.mark.parametrize("scheme", SCHEMES)
def test_table_word_is_the_lookups(scheme):
    rng = np.random.default_rng(4100 + sum(abs(v) * 5 ** k for k, v in enumerate(scheme)))
    tab, sub = s_tab(scheme), [int(v) for v in s_sub(scheme)]
    lookup = {(nA, nB, tA, tB): v_perm_b32(tab[nB], tab[nA], SEL_BASE | tA | (tB << 16))
              for nA in range(16) for nB in range(16) for tA in range(4) for tB in range(4)}
    for r in range(16):
        # the other rows' nibbles and symbols are noise the words must not pick up
        PA0, PB0 = (int(v) & ~(0xF << (4 * r)) for v in rng.integers(0, 1 << 63, 2, dtype=np.uint64) * 2 + rng.integers(0, 2, 2, dtype=np.uint64))
        TA0, TB0 = (int(v) & ~(3 << (2 * r)) for v in rng.integers(0, 1 << 32, 2, dtype=np.uint64))
        for nA in range(16):
            for nB in range(16):
                RE, RO = row_words(PA0 | (nA << (4 * r)), PB0 | (nB << (4 * r)))
                rw = row_word(RE, RO, r)
                for tA in range(4):
                    for tB in range(4):
                        TA, TB = TA0 | (tA << (2 * r)), TB0 | (tB << (2 * r))
                        want = lookup[nA, nB, tA, tB]
                        for cw in (column_word(TA, TB, r), first_column_word(TA, TB, r)):
                            index = rw ^ cw
                            assert index % 4 == 0 and index < 1024
                            assert sub[index // 4] == want, (scheme, r, nA, nB, tA, tB)
                            assert sub_code_a(index // 4) == nA ^ tA and sub_code_b(index // 4) == nB ^ tB


def test_acgt_entries_lie_in_sixteen_banks():
    banks = set()
    for nA in range(4):
        for nB in range(4):
            for tA in range(4):
                for tB in range(4):
                    RE, RO = row_words(nA, nB)
                    address = row_word(RE, RO, 0) ^ column_word(tA, tB, 0)
                    banks.add((address // 4) % 32)
    assert len(banks) == 16


def test_table_word_layout():
    """{0, sub(c_B), 0, sub(c_A)}: a match byte exactly where a code is 0, so a nibble of 4 or more matches no symbol"""
    for scheme in SCHEMES:
        sm, sx = score_bytes(scheme)
        sub = s_sub(scheme)
        for k in range(256):
            assert int(sub[k]) == (sm if sub_code_a(k) == 0 else sx) | ((sm if sub_code_b(k) == 0 else sx) << 16)
        for n in range(4, 16):
            for t in range(4):
                assert n ^ t >= 4
