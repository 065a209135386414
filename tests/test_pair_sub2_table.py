"""The table of pairs of the pair kernel's PF_SUBLDS2 form (nvbio_amd/csrc/banded_gotoh_pair.h, "Two cells per read"), in numpy mirrors of
the header's functions: the table's fill (sub2_word), the index (sub2_index) as the xor of a row byte and a column pair byte, the words a
16-row block builds (sub2_row_words, sub2_col_words, the carried symbols out of the ring's slot 12), what PairRows::run extracts from
them, and the ring's schedule (PD3::row).  The single-cell table of tests/test_pair_sub_table.py is the reference for the words.
The bank model of the form's estimate is kept here as a function and printed, not asserted.  No GPU."""
import numpy as np
import pytest

from test_banded_pair_sub_gpu import GE_SCHEMES
from test_pair_sub_table import bfi, column_word, row_word, row_words, s_sub, score_bytes

BAND = 15
M32 = 0xFFFFFFFF


# ---- the header's functions
def sub2_index(c0a, c0b, da, db, na, nb):
    return da | (c0a << 2) | (c0b << 4) | (db << 6) | (na << 8) | (nb << 9)


def sub2_row_byte(nib_a, nib_b):
    return (nib_a & 3) | ((nib_b & 3) << 2) | (64 if nib_a >= 4 else 0) | (128 if nib_b >= 4 else 0)


def sub2_col_byte(t0a, t0b, t1a, t1b):
    return (t0a ^ t1a) | (t0a << 2) | (t0b << 4) | ((t0b ^ t1b) << 6)


def sub2_word(index, h, sm, sx):
    ca = ((index >> 2) & 3) ^ ((index & 3) if h else 0)
    cb = ((index >> 4) & 3) ^ (((index >> 6) & 3) if h else 0)
    return (sm if ca == 0 and not index & 256 else sx) | ((sm if cb == 0 and not index & 512 else sx) << 16)


def s_sub2(scheme):
    """the kernel's fill: 1 024 entries of two words"""
    sm, sx = score_bytes(scheme)
    return np.array([[sub2_word(k, 0, sm, sx), sub2_word(k, 1, sm, sx)] for k in range(1024)], np.uint32)


def sub2_row_words(PA, PB):
    RE = RO = 0
    for h in range(2):
        a, b = (PA >> (32 * h)) & M32, (PB >> (32 * h)) & M32
        na, nb = (a | (a >> 1)) & 0x44444444, (b | (b >> 1)) & 0x44444444
        re = (a & 0x03030303) | ((b << 2) & 0x0C0C0C0C) | ((na << 4) & 0x40404040) | ((nb << 5) & 0x80808080)
        ro = ((a >> 4) & 0x03030303) | ((b >> 2) & 0x0C0C0C0C) | (na & 0x40404040) | ((nb << 1) & 0x80808080)
        RE |= re << (32 * h)
        RO |= ro << (32 * h)
    return RE, RO


def sub2_col_words(TA, TB, prev_a, prev_b):
    PA, PB = ((TA << 2) & M32) | prev_a, ((TB << 2) & M32) | prev_b
    DA, DB = TA ^ PA, TB ^ PB
    ue, uo = bfi(0x33333333, DA, (PA << 2) & M32), bfi(0x33333333, DA >> 2, PA)
    ve, vo = bfi(0x33333333, PB, (DB << 2) & M32), bfi(0x33333333, PB >> 2, DB)
    return [bfi(0x0F0F0F0F, ue, (ve << 4) & M32), bfi(0x0F0F0F0F, uo, (vo << 4) & M32), bfi(0x0F0F0F0F, ue >> 4, ve), bfi(0x0F0F0F0F, uo >> 4, vo)]


def sub2_row_offset(RE, RO, r):
    """PairRows::run: row r's byte as a byte offset, times 32"""
    k = r >> 1
    zw = ((RO if r & 1 else RE) >> (32 * (k >> 2))) & M32
    return (zw << 5) & 0x1FE0 if k & 3 == 0 else (zw >> (8 * (k & 3) - 5)) & 0x1FE0


def sub2_col_offset(CW, r):
    """PairRows::run: row r's entering pair byte as a byte offset, times 8"""
    q, xw = r >> 2, CW[r & 3]
    return (xw << 3) & 0x7F8 if q == 0 else (xw >> (8 * q - 3)) & 0x7F8


def carried(tc12):
    """the kernel's block loop: the symbols that entered the row before the block's first, out of the ring's slot 12"""
    last = tc12 ^ (tc12 >> 2)
    return (last >> 3) & 3, (last >> 7) & 3


def first_pairs(TA, TB):
    """the ring before row 0: pair t = 0 ... 12 of the band's first fourteen symbols in slot t, the rest empty"""
    sym = lambda T, t: (T >> (2 * t)) & 3
    return [sub2_col_byte(sym(TA, t), sym(TB, t), sym(TA, t + 1), sym(TB, t + 1)) << 3 if t < BAND - 2 else 0 for t in range(16)]


# ---- the table
@pytest.mark.parametrize("scheme", GE_SCHEMES)
def test_entry_holds_both_cells_single_words(scheme):
    """every nibble pair and every (t0_A, t0_B, t1_A, t1_B): the entry at (row offset xor pair offset) is the two words the single-cell
    table gives for (nibbles, t0) and (nibbles, t1); N and an 8-bit pattern's code 15 match nothing"""
    sm, sx = score_bytes(scheme)
    single, pairs = [int(v) for v in s_sub(scheme)], s_sub2(scheme)
    seen = set()
    for nA in range(16):
        for nB in range(16):
            RE, RO = row_words(nA, nB)
            rw1 = row_word(RE, RO, 0)
            rw2 = sub2_row_byte(nA, nB) << 5
            for t0A in range(4):
                for t0B in range(4):
                    want0 = single[(rw1 ^ column_word(t0A, t0B, 0)) // 4]
                    for t1A in range(4):
                        for t1B in range(4):
                            want1 = single[(rw1 ^ column_word(t1A, t1B, 0)) // 4]
                            off = rw2 ^ (sub2_col_byte(t0A, t0B, t1A, t1B) << 3)
                            assert off % 8 == 0 and off < 8192
                            assert off // 8 == sub2_index((nA & 3) ^ t0A, (nB & 3) ^ t0B, t0A ^ t1A, t0B ^ t1B, int(nA >= 4), int(nB >= 4))
                            got = pairs[off // 8]
                            assert (int(got[0]), int(got[1])) == (want0, want1), (scheme, nA, nB, t0A, t0B, t1A, t1B)
                            if nA >= 4:
                                assert got[0] & 0xFFFF == sx and got[1] & 0xFFFF == sx
                            if nB >= 4:
                                assert got[0] >> 16 == sx and got[1] >> 16 == sx
                            seen.add(off // 8)
    assert len(seen) == 1024                                                       # every entry is reached: the table has no spare


# ---- the words of a block
def test_block_words_match_their_definitions():
    """random strings through the prologue and three 16-row blocks: every row's extracted row word and entering pair word are their
    definitions, the pairs across the 16-row seams (the carried symbols come out of the ring) and the prologue's included"""
    rng = np.random.default_rng(5200)
    for trial in range(50):
        rows = 48
        pat = rng.integers(0, 16, (2, rows))
        if trial % 2:
            pat[rng.random(pat.shape) < 0.5] &= 3
        txt = rng.integers(0, 4, (2, rows + BAND - 1 + 16))
        word = lambda sym, at, count, bits: sum(int(sym[at + k]) << (bits * k) for k in range(count))
        tc = first_pairs(word(txt[0], 0, 16, 2), word(txt[1], 0, 16, 2))
        for t in range(BAND - 2):
            assert tc[t] == sub2_col_byte(txt[0][t], txt[1][t], txt[0][t + 1], txt[1][t + 1]) << 3
        for i0 in range(0, rows, 16):
            RE, RO = sub2_row_words(word(pat[0], i0, 16, 4), word(pat[1], i0, 16, 4))
            prev = carried(tc[12])
            assert prev == (txt[0][i0 + BAND - 2], txt[1][i0 + BAND - 2])
            CW = sub2_col_words(word(txt[0], i0 + BAND - 1, 16, 2), word(txt[1], i0 + BAND - 1, 16, 2), *prev)
            for r in range(16):
                i = i0 + r
                assert sub2_row_offset(RE, RO, r) == sub2_row_byte(pat[0][i], pat[1][i]) << 5
                t = i + BAND - 2                                                   # the entering pair (i + 13, i + 14)
                g_new = sub2_col_offset(CW, r)
                assert g_new == sub2_col_byte(txt[0][t], txt[1][t], txt[0][t + 1], txt[1][t + 1]) << 3
                tc[(r + BAND - 2) & 15] = g_new


# ---- the ring
def test_ring_schedule():
    """PD3::row's slots: row i writes pair i + 13 and reads pair i (column 0, its first word) and pairs i + 1, i + 3, ..., i + 13.
    Each pair is formed before its first use, read as a pair by seven rows and once more by column 0, and no row overwrites a live one"""
    rows = 64
    slot = {t: t for t in range(BAND - 2)}                                         # slot -> the pair it holds; the prologue's thirteen
    formed = {t: -1 for t in range(BAND - 2)}
    pair_reads, single_reads, last_use = {}, {}, {}
    for i in range(rows):
        r = i & 15
        t_new = i + BAND - 2
        victim = slot.get((r + BAND - 2) & 15)
        if victim is not None:
            assert last_use.get(victim, -1) < i and victim < i, "row %d overwrites pair %d, still to be read" % (i, victim)
        slot[(r + BAND - 2) & 15] = t_new
        formed[t_new] = i
        assert slot[r & 15] == i                                                   # column 0
        single_reads.setdefault(i, []).append(i)
        last_use[i] = i
        for k in range(1, 8):                                                      # columns 2 k - 1 and 2 k: text positions i + 2 k - 1, i + 2 k
            t = i + 2 * k - 1
            assert slot[(r + 2 * k - 1) & 15] == t, (i, k)
            assert formed[t] <= i
            pair_reads.setdefault(t, []).append(i)
            last_use[t] = max(last_use.get(t, -1), i)
    for t in range(BAND - 2, rows - 1):                                            # the pairs whose whole life lies in the rows simulated
        assert pair_reads[t] == list(range(t - 13, t, 2)) and len(pair_reads[t]) == 7
        assert single_reads[t] == [t]
        assert formed[t] == t - 13 == pair_reads[t][0]
    live = max(sum(1 for t in formed if formed[t] <= i <= last_use.get(t, -1)) for i in range(16, rows - 16))
    assert live == 14                                                              # the ring of 16 holds them


# ---- the bank model of the estimate (printed, not asserted)
def bank_model(entries, lanes=32, draws=20000, seed=1):
    """a ds_read_b64 is served in groups of 32 lanes; an 8-byte entry's bank pair is entry mod 32; a group costs the largest number of
    distinct entries it reads on one bank pair.  Mean cost of a group whose lanes draw uniformly from `entries`"""
    rng = np.random.default_rng(seed)
    entries = np.asarray(sorted(entries))
    total = 0
    for _ in range(draws):
        picked = np.unique(entries[rng.integers(0, entries.size, lanes)])
        total += np.bincount(picked % 32, minlength=32).max()
    return total / draws


def test_bank_model_prints():
    acgt = {sub2_index(c0a, c0b, da, db, 0, 0) for c0a in range(4) for c0b in range(4) for da in range(4) for db in range(4)}
    assert len(acgt) == 256
    per_pair = np.bincount(np.array(sorted(acgt)) % 32, minlength=32)
    print("A/C/G/T entries per bank pair: min %d max %d; modelled LDS cycles per group of 32 lanes: %.2f (per ds_read_b64: %.2f)"
          % (per_pair.min(), per_pair.max(), bank_model(acgt), 2 * bank_model(acgt)))
