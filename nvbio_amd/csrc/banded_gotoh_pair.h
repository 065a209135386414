// banded_gotoh_pair.h -- the 16-bit LOCAL banded Gotoh score with TWO jobs per lane (no qualities, fixed-length strings).
//
// The row-frame recurrence of A16 (banded_gotoh_impl.h: A32::cell_rt has the derivation), with job A's value in bits 0-15 of every state
// register and job B's in bits 16-31.  Both halves are UNSIGNED numbers: the row frame plus one constant BIAS.  Then
//   * an add or subtract of a constant is one 32-bit op on c * 0x10001, as long as no half carries or borrows;
//   * only the maxima need a packed instruction (v_pk_max_u16);
//   * one v_perm_b32 delivers both jobs' substitution scores, which fit a byte each.
//
// Range.  With G = 32 |G_e|, D = 32 (G_e - G_o) >= 0 (the host admits G_o <= G_e <= 0 only) and S+ = max(match, mismatch, 0), row i holds
//   zero  Z_i = BIAS + (i + 1) G                 h  in [Z_i, BIAS + 32 (i + 1) (S+ + |G_e|)]       key = h + j, j <= 30
//   S = h - D >= Z_i - D                         E = max(E, S) - G >= Z_i - D - G                  diag = S(i-1) + sub, 0 <= sub <= 255
// and the band starts at S(-1) = BIAS - D.  BIAS = D + G keeps every minuend at or above what is taken from it (Z_i - D - G >= 0,
// S(-1) >= 0; the sink fold takes Z_i from a key >= Z_i).  The host admits 7 >= match - G_o, so D + G <= 448; with the row-frame limit
// M (S+ + |G_e|) <= 1022 (max_len_16bit) the largest value is 448 + 32 * 1022 + 30 = 33182, and 255 more still fit 16 bits: the limit
// of the signed kernel carries over unchanged.
//
// The infimum.  The reference's infimum stands in F of row -1 and in F[BAND-1] of every row.  In LOCAL every H is >= 0, so every real
// S = H + G_o - G_e (in any row's frame) lies far above it -- and F only ever meets it next to a real S: F(i,j) = max(F(i-1,j+1),
// S(i-1,j+1)).  E never sees it (E starts from the row's own S).  So the infimum never wins a maximum, and the frame's lowest value,
// 0, takes its place: max(0, S) = S.
//
// Two cells.  P16 is the cell above: two-input v_pk_max_u16 throughout, six per interior cell.  PM3 takes the same maxima three at a
// time with v_pk_maximum3_f16 (gfx950).  For bit patterns in 0x0400 ... 0x7BFF -- the positive normal halves -- the order of f16 is the
// order of the unsigned 16-bit patterns, there is no NaN, infinity or subnormal among them, and a maximum returns one of its operands
// unchanged: over that range the instruction IS an exact packed three-input unsigned maximum (and v_pk_max_u16 agrees with it, so the
// two mix freely).  PM3 keeps every operand of every maximum inside the range:
//   * the frame is raised by FLOOR = 0x0400: BIAS' = D + G + 0x0400, S(-1) = BIAS' - D = G + 0x0400, and F starts at the frame's lowest
//     value 0x0400 in place of 0.  Every bound of "Range" moves up by 0x0400 with it: the smallest value any register holds is
//     E >= Z_i - D - G = 0x0400 + i G >= 0x0400, and S, z, diag, h, F, key and the row key lie above it.
//   * no carry, no borrow, as before with 0x0400 to spare: S = h - D with h >= Z_i >= BIAS' > D;  E = max(E, S) - G with
//     S >= Z_i - D = 0x0400 + (i + 2) G > G;  the sink fold takes Z_i from a row key >= h(i,0) >= Z_i;  the adds (z + G, S + sub,
//     h + j) stay at or below the top, which is below 2^15.
//   * the top: the largest operand is a diagonal, S(i-1) + sub <= BIAS' + 32 M (S+ + |G_e|) + 255 (a key adds j <= 14 to an h instead),
//     and must not pass 0x7BFF = 31743.  With the largest BIAS the byte table admits, D + G = 448, that is
//     32 M (S+ + |G_e|) <= 31743 - 255 - 1024 - 448 = 30016, M (S+ + |G_e|) <= 938 (PM3_ROW_LIMIT; the host's pair_admitted sends longer
//     jobs, up to the 1022 of P16, to P16).
// What the three-input form buys:
//   * F' = max(F, Z_i), the zero clamp folded into F:  F'(i,j) = max3(F'(i-1,j+1), S(i-1,j+1), Z_i).  The row's zero never falls
//     (Z_(i-1) <= Z_i, equal when G_e = 0), so by induction on i, with F'(-1,.) = 0x0400 <= Z_0:
//       F'(i,j) = max(max(F(i-1,j+1), Z_(i-1)), S(i-1,j+1), Z_i) = max(F(i-1,j+1), S(i-1,j+1), Z_i) = max(F(i,j), Z_i),
//     and h = max3(F', diag, E) = max(F, Z_i, diag, E) is the h of P16: two instructions where P16 has four.  Next to the band's edge
//     F' = max(S(i-1,j+1), Z_i); column 0 (no E) takes h = max(F', diag); the last column (no F) takes h = max3(E, diag, Z_i).
//   * the row key takes two columns' keys at a time: rowkey = max3(rowkey, key_j, key_(j+1)).
//   * E = max(E, S) stays a two-input maximum.
// An interior cell is then 8.5 vector instructions, 3.5 of them maxima, where P16 has 11 and 6.
//
// The column frame.  PD3 is PM3 in a frame that also rises along the row: phi(i,j) = BIAS' + G (2 (i + 1) + j), so the zero of row i,
// column j is Z(i,j) = BIAS' + G (2 i + j + 2) and h' = 32 H + Z(i,j), S' = h' - D as before.  The three steps of the recurrence:
//   * horizontal, (i,j) -> (i,j+1): phi rises by G, the cost of the step, so E'(i,j+1) = max(E'(i,j), S'(i,j)) with no subtract; column 0
//     has no E and hands its S' to column 1 as E'(i,1);
//   * vertical, (i-1,j+1) -> (i,j): phi rises by 2 G - G = G, free as in the row frame: F'(i,j) = max3(F'(i-1,j+1), S'(i-1,j+1), Z(i,j));
//   * diagonal, (i-1,j) -> (i,j): phi rises by 2 G, one G more than in the row frame, which the substitution byte carries:
//     32 (s - G_o) + G.  It fits while max(match, mismatch) - G_o + |G_e| <= 7 (PD3_BYTE_LIMIT).
//   * F' = max(F, Z) carries over: the zero along the F path does not fall, Z(i-1,j+1) = Z(i,j) - G <= Z(i,j), so with
//     F'(-1,.) = 0x0400 <= Z(0,.) the induction of PM3 reads the same with Z(i,j) for Z_i:
//       F'(i,j) = max(max(F(i-1,j+1), Z(i-1,j+1)), S'(i-1,j+1), Z(i,j)) = max(F(i,j), Z(i,j)).
//     The infimum argument is unchanged (every S' is a real value at or above Z - D >= 0x0400).
//   * the row key must compare columns in one frame: key_j = h'(i,j) + K_j with K_j = j + (14 - j) G is 32 H + Z(i,14) + j, column 14's
//     frame -- the add the tag j costs anyway, with another constant (and one more add, for column 0, whose K_0 = 14 G is not zero).  The
//     sink takes Z(i,14) off the row key and folds p = score * 32 + j as before.
//   * Z(i,j) depends on 2 i + j alone and is wave-uniform: a ring of 16 scalar registers at index (2 i + j) & 15.  Row i holds
//     2 i ... 2 i + 14; its prologue adds 16 G to the two slots no row reads any more (2 i - 3 and 2 i - 2 become 2 i + 13 and 2 i + 14),
//     two scalar adds where the row frame has one vector add.  The rows are unrolled 16 to a block and 2 * 16 = 0 (mod 16), so every
//     index is static.  K_j and D are scalars too: every instruction of the cell takes at most one of them.
//   * start: S'(-1,j) = Z(-1,j) - D = BIAS' + G j - D (H = 0 in row -1), F' = 0x0400, Z(0,j) = BIAS' + G (2 + j).
//   * no carry, no borrow: the only subtracts left are S' = h' - D with h' >= Z(i,j) >= BIAS' > D, and the sink's, Z(i,14) from a row
//     key >= key_0 = h'(i,0) + 14 G >= Z(i,0) + 14 G = Z(i,14).  The smallest value is F'(-1,.) = 0x0400; every S', E' >= Z - D >= 0x0400 + G.
//   * the top: h' <= Z(M-1,14) + 32 M S+ = BIAS' + G (2 M + 14) + 32 M S+; a key adds at most 14 to an h' (K_j <= 14 G moves column j's
//     value into column 14's frame, it does not pass that frame's top) and a diagonal adds a byte to an S' = h' - D of the row before, so
//     pd3_top() = 0x0400 + D + G + G (2 M + 14) + 32 M S+ + 255 <= 0x7BFF keeps every operand in range; the scalar adds stay below it too
//     (Z <= h', K_j <= 14 G <= Z(0,14)).  The frame costs range -- G (2 M + 14) where the row frame spends G M -- so the host admits it for
//     shorter jobs than PM3 (banded_gotoh.hip: pair_column_admitted; M <= 234 under (2,-1,-2,-1)) and PM3 takes the rest.
// A row loses 14 of its 30 subtracts (12 interior cells, the cell next to the edge and column 0) and the vector add of its zero, and
// gains column 0's key add: 128 vector instructions where PM3 has 142, and the chain E -> h -> S -> E is three instructions long, not four.
//
// The sink.  Un-framed (its row's zero taken off), a job's row key is p = score * 32 + j: the row's best score and the largest column
// that holds it, 16 bits.  The fold's rule is "replace when (p | 31) >= best": the higher score wins, and on an equal score the later
// row.  The library folds it with a compare and two selects per job (PF_SINK_VCC), the key in one register and its row in another.
// PF_SINK_KEY, which only tools/pair_row_probe.hip launches, folds one 32-bit key per job with a plain unsigned maximum instead:
//     W = p << 15 | 31 << 15 | i << 5 | (p & 31),     best = max(best, W),
// score in bits 20-29, the copy of j that the shift leaves in bits 15-19 saturated to a constant, the row i in bits 5-14, j in bits
// 0-4.  Unsigned order on W is the order of (score, row, column), and every row folds a different i, so the maximum over the rows is
// the fold's result; the epilogue decodes score = W >> 20, i = (W >> 5) & 1023, j = W & 31.  It needs score <= 1023 and i <= 1023,
// three instructions fewer per row, and measured no faster (profiles/banded_pair/README.md), so the library does not take it.
//
// The pair fold.  PF_FOLD2, which the library takes for PD3, folds once per two rows.  A column is at most 14, so bit 4 of the key is
// free: rows i (even) and i + 1 share the key q = score * 32 + 16 r + j, r the row's parity, and besti holds the even row.  A plain
// maximum over q is the fold's order inside a pair -- the higher score, on equal scores row i + 1 whatever the columns, inside a row
// the larger column -- and "(q | 31) >= best" keeps "the later row wins" across pairs.  The epilogue decodes j = best & 15,
// row = besti + ((best >> 4) & 1), score = best >> 5.
//   * frames: a row key stands in its row's last-column frame and Z(i+1,14) = Z(i,14) + 2 G, so the even row's key stays live across
//     the row boundary (one VGPR) and the odd row takes  q = max(rk(i) + 2 G, rk(i+1) + 16) - Z(i+1,14):  two adds and a packed
//     maximum per pair in place of one whole fold (the subtract is the fold's own).
//   * range: both operands of that maximum are row keys in the odd row's frame.  rk(i) + 2 G = 32 H + Z(i+1,14) + j is what row i + 1
//     would hold for the same H, and rk(i+1) + 16 adds the pair's bit to a key: at most 14 + 16 = 30 above an h' of row i + 1, where
//     "the top" leaves 255 above the largest h'; and both are at least Z(i+1,14) >= 0x0400 -- no key is lowered below its zero (in
//     the all-zero scheme Z is 0x0400 itself).  No add carries (the sums stay below 0x7BFF) and the subtract does not borrow (both
//     operands are >= Z(i+1,14)).  pair_column_admitted is unchanged.
//   * an odd number of rows: the last row has no partner.  Its key is still live behind the block loop and is folded there alone, as
//     its pair's even row (q = rk(M-1) - Z(M-1,14), bit 4 clear), with Z(M-1,14) = BIAS' + G (2 M + 14) worked out once per job.
//   tests/test_pair_fold2.py holds the arithmetic in numpy.
//
// Where the constants live.  D, the K_j and 2 G are wave-uniform, and the column frame's cell has two placements for them; both compute
// the same values from the same operations, so pair_column_admitted and the numpy models hold for either:
//   * scalar registers, as "The column frame" has them;
//   * PF_CONST2: D in a vector register, K_j = j + (14 - j) G and 2 G as 32-bit literals -- G = 32 |G_e| is then a template parameter,
//     the PF_GE bits; the column frame's byte admits |G_e| <= 3 for every scheme with max(match, mismatch) >= 0 -- and one s_nop behind
//     each of cell2's three groups of simple ops.
// A v_add_u32 or v_subrev_u32 with a scalar source issues at the rate of the packed ops, about 4.3 cycles, where the same op on vector
// registers or a literal takes 2.3 (tools/valu_probe.hip, `mix`), and it reaches that short issue only where a scalar instruction
// follows the group: hence the pad.  Literals plus pad are 5 % faster than the scalars and are what the library launches with the pair
// fold; NVBIO_HIP_PAIR_CONST = 1 keeps the scalars.  profiles/banded_pair/README.md has the figures, and those of the alternatives that
// were measured and are gone: other placements of the constants, the table words read a row ahead, the cells' chain links spread apart.
//
// Where the substitution comes from.  A diagonal adds one word to S'(i-1,j): job A's byte in bits 0-7, job B's in bits 16-23, each the
// match byte where the pattern's nibble equals the text's symbol and the mismatch byte elsewhere (in the column frame both carry the
// extra G).  Two ways to that word, the same bytes either way, so every bound above and pair_column_admitted hold for both:
//   * the lookup: the row reads two table words from LDS, s_tab[nibble A] and s_tab[nibble B] (entry q: the match byte in byte q where
//     q < 4, the mismatch byte in every other byte), and each column takes one v_perm_b32 of them with its selector {g_A, zero, 4 + g_B,
//     zero}, which the ring tc[] holds.  Fifteen v_perm_b32 per row, a slow op on the vector ALU (4.3 cycles), and six instructions for
//     the two words.  Every instance has it but the ones below.
//   * PF_SUBLDS, which the library launches with PF_FOLD2 | PF_CONST2: the LDS pipe does the lookup.  With c = nibble ^ symbol, a job's
//     byte is the match byte exactly where c == 0 (a nibble of 4 or more gives c >= 4 against every symbol: N and an 8-bit pattern's
//     code 15 match nothing, as s_tab[q >= 4] has it).  A 256-word table s_sub, filled once per block, holds {0, sub(c_B), 0, sub(c_A)} at
//     sub_index(c_A, c_B) = c_A & 3 | c_B << 2 | (c_A >> 2) << 6; the sixteen words two A/C/G/T codes reach are then words 0 ... 15, one
//     to a bank, where the plain c_A | c_B << 4 would put c_B = 0 and c_B = 2 into the same banks.  xor goes bit by bit, so the index
//     is the xor of a row word, both jobs' nibbles in that layout, and a column word, t_A | t_B << 2; both are kept times 4, as byte
//     offsets, and a cell costs one v_xor_b32 on two vector registers (a simple op) and one ds_read_b32.
//       - the row words: once per 16-row block, two shifts and two v_bfi_b32 per word put the block's rows into four words, a byte per
//         row (sub_row_words); a row takes its byte with one SDWA shift.
//       - the column words: the ring tc[] holds them in place of the selectors.  Once per block two v_bfi_b32 interleave the sixteen
//         entering symbols of both jobs, a nibble per row; a row takes its nibble with a shift and a mask.
//       - the reads: eight at the row's head, seven behind column 4 into the registers columns 0 ... 4 have given back (fifteen
//         landing registers at once do not fit the 96 of five waves), each batch in the order the cells take its words.  They are plain
//         loads; the compiler writes a counted s_waitcnt lgkmcnt before each cell block.
//     The row has 1 + 2 + 15 simple ops where the lookup has 7 simple and 15 slow ones and two reads; it is 4 to 5 % faster
//     (profiles/banded_pair/README.md).  NVBIO_HIP_PAIR_SUB = 1 keeps the lookup.
//
// Two cells per read.  PF_SUBLDS2 (with PF_SUBLDS) reads the words of two neighbouring columns with one ds_read_b64: eight address xors
// and eight reads per row where PF_SUBLDS has fifteen of each.  The cells (col0, cell2, tail2) are the same instructions on the same
// words, so every bound above holds unchanged.
//   * the table s_sub2: 1 024 entries of 8 bytes (8 KB a block; s_sub is not allocated).  Entry
//         index = d_A | c0_A << 2 | c0_B << 4 | d_B << 6 | N_A << 8 | N_B << 9
//     holds {0, sub(c0_B, N_B), 0, sub(c0_A, N_A)} and the same for c1 = c0 ^ d: c0 = (nibble & 3) ^ t0 is the first column's code,
//     d = t0 ^ t1 the xor of the two columns' text symbols (it depends on the columns alone, which is why the second field holds d and
//     not c1: the row's part stays at one byte), N = nibble >= 4; sub is the match byte where the code is 0 and N is clear -- the bytes
//     s_sub and s_tab give.  An entry's bank pair is index mod 32 = d_A, c0_A and the low bit of c0_B: the 256 entries A/C/G/T codes
//     reach lie 8 to a bank pair, as evenly as any layout has them.
//   * the row byte n_A & 3 | (n_B & 3) << 2 | N_A << 6 | N_B << 7 and the column pair byte d_A | t0_A << 2 | t0_B << 4 | d_B << 6 are
//     kept as byte offsets, times 32 and times 8: the fields are ordered so that each is one contiguous byte and a row takes either
//     with one SDWA shift.  A 16-row block builds four registers of row bytes (sub2_row_words) and four of pair bytes (sub2_col_words:
//     T ^ (T << 2 | carried symbol) gives a job's sixteen d in one op); the symbol carried across the block seam is the second of the
//     last pair formed, t0 ^ d of the ring's slot 12, where the prologue has put the pair (12, 13) of the band's first fourteen symbols.
//   * the ring tc[] holds pair words: slot t & 15 the pair of text positions (t, t + 1).  Row i forms the pair (i + 13, i + 14) from its
//     entering symbol and reads column 0 alone, a ds_read_b32 of the first word of pair (i, i + 1), and the pairs (i + 1, i + 2), ...,
//     (i + 13, i + 14) for columns 1 ... 14, which is how cell2 and tail2 take their columns.  A pair is formed in the row that first
//     reads it, read as a pair by seven rows and once more by column 0: fourteen live, the ring stays 16.
//   * the reads are plain loads, the compiler writes the waits.  Each pair is read one cell2 ahead of the cell that takes it: with the
//     landing registers two and two, the kernel has 95 VGPRs and no scratch, five waves.  The cells read the landing registers without
//     rewriting them (a half of a 64-bit pair rewritten in place costs a v_mov_b32), and the kernel's epilogue works the job numbers out
//     again from the lane's where the other forms keep them across the block loop.
//   tests/test_pair_sub2_table.py holds the table, the words and the ring's schedule in numpy.  NVBIO_HIP_PAIR_SUB = 2 keeps one read
//   per cell.  profiles/banded_pair/README.md has the probe's ceiling (sub-xor8), the form's figures and the counters.
#pragma once
#include "banded_gotoh_impl.h"

namespace nvb {

template <int BAND>
struct PairState {
    uint32_t S[BAND];        // S = H' + G_o - G_e of the previous row, both jobs
    uint32_t F[BAND - 1];
    uint32_t tc[16];         // the band's text symbols, as selectors or, under PF_SUBLDS, column words (a ring indexed by (row + column) & 15, like BandTraits)
    uint32_t z;              // the row's zero
    uint32_t best[2], besti[2];   // per job: the best key so far (score * 32 + j) and its row
};

// The kernel's forms, one template parameter.  The host picks the fetch (banded_gotoh.hip: launch_pair); the key sink and the
// knock-outs exist for tools/pair_row_probe.hip alone, which times the row with one part taken out and its inputs kept live.  No
// knock-out computes results.
enum PairForm : int {
    PF_SINK_VCC = 0, PF_SINK_KEY = 1,                                               // the sink fold: compare + select / one 32-bit key (probe only)
    PF_STREAM   = 4,                                                                // the block loop streams its words (GroupStream, common.h), and then:
    PF_PAT2     = 2,                                                                //   the pattern has 2 bits (else 4)
    PF_PBE      = 8, PF_TBE = 256,                                                  //   the pattern's / the text's words are big-endian
    PF_KO_SINK  = 16, PF_KO_TABLE = 32, PF_KO_FETCH = 64, PF_KO_BOUND = 128,        // probe only
    // the column frame's row (the header comment, "The pair fold"):
    PF_FOLD2    = 1024,                                                             //   the sink folds a pair of rows at a time
    // the column frame's constants as literals with the pad (the header comment, "Where the constants live"); else scalar registers.
    // Two bits, which were the literals and the pad apart: the forms keep their numbers and the kernels their names.  (512, 2048,
    // 4096 and 8192 were forms that are gone and stay unused.)
    PF_CONST2   = 16384 | 131072,
    PF_GE1      = 32768, PF_GE2 = 65536, PF_GE3 = PF_GE1 | PF_GE2,                  //   PF_CONST2's |G_e|, 0 ... 3 (pair_ge)
    // the substitution words read from LDS, one ds_read_b32 per cell, in place of the v_perm_b32 lookup (the header comment, "Where the
    // substitution comes from"); with PF_FOLD2 | PF_CONST2 only
    PF_SUBLDS   = 262144,
    PF_KO_PERM  = 524288,                                                           // probe only: PF_CONST2's row, a v_xor_b32 for each v_perm_b32
    // PF_SUBLDS with two cells' words to a read, ds_read_b64 from a table of 1 024 pairs ("Two cells per read"); with PF_SUBLDS only
    PF_SUBLDS2  = 1048576,
    // probe only, on PF_SUBLDS's rows: eight address xors and eight two-word reads per row, the second word the table's next one (no
    // results); one s_nop behind each run of address xors; PF_CONST2's pad in col0 and tail2 as well
    PF_KO_XOR8  = 2097152, PF_PAD_XOR = 4194304, PF_PAD_EDGE = 8388608,
    PF_AHEAD2   = 16777216                                                          // probe only: PF_SUBLDS2's reads two pairs ahead of the cells, not one
};
constexpr int pair_ge(int form)     { return (form / PF_GE1) & 3; }
constexpr int pair_ge_bits(int ge)  { return ge * PF_GE1; }
// the row the library launches for PD3 (banded_gotoh.hip: launch_pair; NVBIO_HIP_PAIR_ROW = 1 keeps the row without it).  With it the
// library launches PF_CONST2 (NVBIO_HIP_PAIR_CONST = 1 keeps the scalars), one instance per |G_e| 0 ... 3 (a scheme with a larger
// |G_e|, which only negative match scores admit, keeps the scalars too), and with PF_CONST2 it launches PF_SUBLDS
// (NVBIO_HIP_PAIR_SUB = 1 keeps the lookup), two cells to a read (PF_SUBLDS2; NVBIO_HIP_PAIR_SUB = 2 keeps one read per cell)
constexpr int PF_ROW2 = PF_FOLD2;
// the streamed forms the library holds: every pattern width and byte order it streams.  X(form), or Y(A, form) with one more argument
#define NVB_PAIR_STREAM_FORMS_(Y, A) \
    Y(A, PF_STREAM) Y(A, PF_STREAM | PF_PBE) Y(A, PF_STREAM | PF_TBE) Y(A, PF_STREAM | PF_PBE | PF_TBE) \
    Y(A, PF_STREAM | PF_PAT2) Y(A, PF_STREAM | PF_PAT2 | PF_PBE) Y(A, PF_STREAM | PF_PAT2 | PF_TBE) Y(A, PF_STREAM | PF_PAT2 | PF_PBE | PF_TBE)
#define NVB_PAIR_APPLY_(X, F) X(F)
#define NVB_PAIR_STREAM_FORMS(X) NVB_PAIR_STREAM_FORMS_(NVB_PAIR_APPLY_, X)
// every instance the library holds, as X(cell, form): the generic fetches and every streamed form, each for the three cells and PD3
// with PF_ROW2, and for PD3 with PF_ROW2 | PF_CONST2 and each |G_e|, with the v_perm_b32 lookup, with PF_SUBLDS and with PF_SUBLDS2.  In
// four parts, named for the four translation units that share their compile time (banded_gotoh_pair_b15.hip,
// banded_gotoh_pair_b15_lit.hip for the lookup, banded_gotoh_pair_b15_sub.hip for PF_SUBLDS, banded_gotoh_pair_b15_sub2.hip for PF_SUBLDS2)
#define NVB_PAIR_CELLS_(X, F) X(P16, (F)) X(PM3, (F)) X(PD3, (F)) X(PD3, (F) | PF_ROW2)
#define NVB_PAIR_GES_(X, F)   X(PD3, (F) | PF_ROW2 | PF_CONST2) X(PD3, (F) | PF_ROW2 | PF_CONST2 | PF_GE1) X(PD3, (F) | PF_ROW2 | PF_CONST2 | PF_GE2) X(PD3, (F) | PF_ROW2 | PF_CONST2 | PF_GE3)
#define NVB_PAIR_INSTANCES_B15(X)     NVB_PAIR_CELLS_(X, PF_SINK_VCC) NVB_PAIR_STREAM_FORMS_(NVB_PAIR_CELLS_, X)
#define NVB_PAIR_INSTANCES_B15_LIT(X) NVB_PAIR_GES_(X, PF_SINK_VCC) NVB_PAIR_STREAM_FORMS_(NVB_PAIR_GES_, X)
#define NVB_PAIR_SUBS_(X, F)  NVB_PAIR_GES_(X, (F) | PF_SUBLDS)
#define NVB_PAIR_INSTANCES_B15_SUB(X) NVB_PAIR_SUBS_(X, PF_SINK_VCC) NVB_PAIR_STREAM_FORMS_(NVB_PAIR_SUBS_, X)
#define NVB_PAIR_SUB2S_(X, F) NVB_PAIR_GES_(X, (F) | PF_SUBLDS | PF_SUBLDS2)
#define NVB_PAIR_INSTANCES_B15_SUB2(X) NVB_PAIR_SUB2S_(X, PF_SINK_VCC) NVB_PAIR_STREAM_FORMS_(NVB_PAIR_SUB2S_, X)
#define NVB_PAIR_INSTANCES(X)         NVB_PAIR_INSTANCES_B15(X) NVB_PAIR_INSTANCES_B15_LIT(X) NVB_PAIR_INSTANCES_B15_SUB(X) NVB_PAIR_INSTANCES_B15_SUB2(X)

// PF_SUBLDS's table index (the header comment, "Where the substitution comes from"): with c = nibble ^ symbol of job A and of job B,
//   index = c_A & 3 | c_B << 2 | (c_A >> 2) << 6,
// so the sixteen entries two A/C/G/T codes reach are words 0 ... 15, one to a bank.  xor goes bit by bit, so the index is the xor of a
// row word (both nibbles in that layout) and a column word (t_A | t_B << 2); both are kept as byte offsets, times 4.
__host__ __device__ constexpr uint32_t sub_index(uint32_t ca, uint32_t cb) { return (ca & 3u) | (cb << 2) | ((ca >> 2) << 6); }
__host__ __device__ constexpr uint32_t sub_code_a(uint32_t index)          { return (index & 3u) | ((index >> 6) << 2); }
__host__ __device__ constexpr uint32_t sub_code_b(uint32_t index)          { return (index >> 2) & 15u; }
__device__ __forceinline__ uint32_t sub_bfi(uint32_t mask, uint32_t a, uint32_t b) { return (a & mask) | (b & ~mask); }     // v_bfi_b32
// a 16-row block's row words, a byte each: byte k of RE is row 2 k's, byte k of RO row 2 k + 1's (PA, PB: the rows' nibbles, row r's at
// bit 4 r).  Two shifts and two v_bfi_b32 per word: the nibble's low pair, the other job's nibble, the nibble's high pair.
__device__ __forceinline__ void sub_row_words(const uint64_t PA, const uint64_t PB, uint64_t& RE, uint64_t& RO)
{
    uint32_t re[2], ro[2];
    #pragma unroll
    for (int h = 0; h < 2; ++h)
    {
        const uint32_t a = uint32_t(PA >> (32 * h)), b = uint32_t(PB >> (32 * h));
        re[h] = sub_bfi(0x03030303u, a,      sub_bfi(0x3C3C3C3Cu, b << 2, a << 4));
        ro[h] = sub_bfi(0x03030303u, a >> 4, sub_bfi(0x3C3C3C3Cu, b >> 2, a));
    }
    RE = re[0] | uint64_t(re[1]) << 32; RO = ro[0] | uint64_t(ro[1]) << 32;
}

// PF_SUBLDS2's table index (the header comment, "Two cells per read"): entry
//   index = d_A | c0_A << 2 | c0_B << 4 | d_B << 6 | N_A << 8 | N_B << 9
// holds the words of the cells with codes c0 and c0 ^ d.  It is the xor of a row byte shifted up by 2 and a column pair byte:
//   row byte    = n_A & 3 | (n_B & 3) << 2 | N_A << 6 | N_B << 7      (n: the row's nibble, N = n >= 4)
//   column byte = d_A | t0_A << 2 | t0_B << 4 | d_B << 6              (t0: the pair's first text symbol, d = t0 ^ t1)
// Both are kept as byte offsets of the 8-byte entries: the row byte times 32, the column byte times 8.
__host__ __device__ constexpr uint32_t sub2_index(uint32_t c0a, uint32_t c0b, uint32_t da, uint32_t db, uint32_t na, uint32_t nb)
{
    return da | (c0a << 2) | (c0b << 4) | (db << 6) | (na << 8) | (nb << 9);
}
__host__ __device__ constexpr uint32_t sub2_row_byte(uint32_t nib_a, uint32_t nib_b) { return (nib_a & 3u) | ((nib_b & 3u) << 2) | (nib_a >= 4u ? 64u : 0u) | (nib_b >= 4u ? 128u : 0u); }
__host__ __device__ constexpr uint32_t sub2_col_byte(uint32_t t0a, uint32_t t0b, uint32_t t1a, uint32_t t1b) { return (t0a ^ t1a) | (t0a << 2) | (t0b << 4) | ((t0b ^ t1b) << 6); }
// entry `index`, word h (0: the pair's first cell, 1: its second): {0, sub(c_B, N_B), 0, sub(c_A, N_A)}, the match byte sm where the code
// is 0 and N is clear, the mismatch byte sx elsewhere
__host__ __device__ constexpr uint32_t sub2_word(uint32_t index, uint32_t h, uint32_t sm, uint32_t sx)
{
    const uint32_t ca = ((index >> 2) & 3u) ^ (h ? index & 3u : 0u), cb = ((index >> 4) & 3u) ^ (h ? (index >> 6) & 3u : 0u);
    return ((ca == 0u && !(index & 256u)) ? sm : sx) | (((cb == 0u && !(index & 512u)) ? sm : sx) << 16);
}
// a 16-row block's row bytes: byte k of RE is row 2 k's, byte k of RO row 2 k + 1's, as sub_row_words has them
__device__ __forceinline__ void sub2_row_words(const uint64_t PA, const uint64_t PB, uint64_t& RE, uint64_t& RO)
{
    uint32_t re[2], ro[2];
    #pragma unroll
    for (int h = 0; h < 2; ++h)
    {
        const uint32_t a = uint32_t(PA >> (32 * h)), b = uint32_t(PB >> (32 * h));
        const uint32_t na = (a | (a >> 1)) & 0x44444444u, nb = (b | (b >> 1)) & 0x44444444u;     // N at bit 2 of every nibble
        re[h] = (a & 0x03030303u)        | ((b << 2) & 0x0C0C0C0Cu) | ((na << 4) & 0x40404040u) | ((nb << 5) & 0x80808080u);
        ro[h] = ((a >> 4) & 0x03030303u) | ((b >> 2) & 0x0C0C0C0Cu) | (na & 0x40404040u)        | ((nb << 1) & 0x80808080u);
    }
    RE = re[0] | uint64_t(re[1]) << 32; RO = ro[0] | uint64_t(ro[1]) << 32;
}
// a 16-row block's entering column pair bytes: byte m of CW[q] is row 4 m + q's, the pair of the symbol that entered a row before
// (TA / TB's symbol r - 1; prev_a / prev_b before symbol 0) and the row's own.  T ^ T' gives every d of a job in one op
__device__ __forceinline__ void sub2_col_words(const uint32_t TA, const uint32_t TB, const uint32_t prev_a, const uint32_t prev_b, uint32_t (&CW)[4])
{
    const uint32_t PA = (TA << 2) | prev_a, PB = (TB << 2) | prev_b, DA = TA ^ PA, DB = TB ^ PB;
    const uint32_t ue = sub_bfi(0x33333333u, DA, PA << 2), uo = sub_bfi(0x33333333u, DA >> 2, PA);       // nibble k: d_A | t0_A << 2 of row 2 k / 2 k + 1
    const uint32_t ve = sub_bfi(0x33333333u, PB, DB << 2), vo = sub_bfi(0x33333333u, PB >> 2, DB);       // nibble k: t0_B | d_B << 2
    CW[0] = sub_bfi(0x0F0F0F0Fu, ue, ve << 4); CW[2] = sub_bfi(0x0F0F0F0Fu, ue >> 4, ve);
    CW[1] = sub_bfi(0x0F0F0F0Fu, uo, vo << 4); CW[3] = sub_bfi(0x0F0F0F0Fu, uo >> 4, vo);
}

// what both cells share: the replicated constants, the substitution lookup and the sink
struct PairOps {
    static constexpr bool COLUMN = false;                                           // the row frame (PD3 alone holds the column frame)
    static __device__ __forceinline__ uint32_t rep(int32_t c)               { return (uint32_t(c) & 0xFFFFu) * 0x10001u; }
    static __device__ __forceinline__ uint32_t mx(uint32_t a, uint32_t b)   { uint32_t r; asm("v_pk_max_u16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
    // both jobs' text symbols of one band column as one byte selector: {g_A, zero, 4 + g_B, zero} picks entry g_A of tlo and g_B of thi
    static constexpr uint32_t SEL_BASE = 0x0C040C00u;
    static __device__ __forceinline__ uint32_t subst(uint32_t tlo, uint32_t thi, uint32_t sel) { return __builtin_amdgcn_perm(thi, tlo, sel); }

    // the sink (dp_row: a later cell with an equal score wins); the row's keys lose its zero here.  The fold, the probe's key form of it
    // (the header comment, "The sink") and the probe's knock-out, which keeps the row key live through one packed maximum
    template <int FORM, int BAND>
    static __device__ __forceinline__ void sink(PairState<BAND>& st, uint32_t rowkey, const uint32_t i) { fold<FORM>(st, rowkey - st.z, i); }
    // rowkey: un-framed
    template <int FORM, int BAND>
    static __device__ __forceinline__ void fold(PairState<BAND>& st, const uint32_t rowkey, const uint32_t i)
    {
        if (FORM & PF_KO_SINK) { st.best[0] = mx(st.best[0], rowkey); return; }
        if (FORM & PF_SINK_KEY)
        {
            // as C++ the compiler spends twelve instructions on it (an SDWA shift, the frame's two parts or-ed in one after the other),
            // so the eight are written out
            const uint32_t frame = (31u << 15) | (i << 5);                          // wave-uniform
            uint32_t a, b, wa, wb;
            asm("v_and_b32 %[a], 0xffff, %[rk]\n\t"
                "v_lshrrev_b32 %[b], 16, %[rk]\n\t"
                "v_lshl_or_b32 %[wa], %[a], 15, %[fr]\n\t"
                "v_lshl_or_b32 %[wb], %[b], 15, %[fr]\n\t"
                "v_and_or_b32 %[wa], %[a], 31, %[wa]\n\t"
                "v_and_or_b32 %[wb], %[b], 31, %[wb]\n\t"
                "v_max_u32 %[ba], %[ba], %[wa]\n\t"
                "v_max_u32 %[bb], %[bb], %[wb]"
                : [a] "=&v"(a), [b] "=&v"(b), [wa] "=&v"(wa), [wb] "=&v"(wb), [ba] "+&v"(st.best[0]), [bb] "+&v"(st.best[1])
                : [rk] "v"(rowkey), [fr] "s"(frame));
            return;
        }
        const uint32_t rk[2] = { rowkey & 0xFFFFu, rowkey >> 16 };
        #pragma unroll
        for (int h = 0; h < 2; ++h)
        {
            const bool upd = (rk[h] | 31u) >= st.best[h];
            st.best[h]  = upd ? rk[h] : st.best[h];
            st.besti[h] = upd ? i : st.besti[h];
        }
    }
};

// ---- the u16 cell: two-input maxima, the frame's lowest value is 0
struct P16 : PairOps {
    static constexpr int32_t FLOOR = 0;

    // one interior cell of both jobs (A16::cell_rt's block).  The serial chain per cell is E -> h -> S -> E (max, sub, max, sub); F, the
    // diagonal and the row's zero are folded before E joins.  EDGE: the cell next to the band's edge, whose F(i-1,j+1) is the infimum.
    template <int J, bool EDGE>
    static __device__ __forceinline__ void cell(uint32_t& Fj, const uint32_t Fnext, const uint32_t Snext, uint32_t& Sj, uint32_t& E, uint32_t& rowkey,
                                                const uint32_t g, const uint32_t D, const uint32_t G, const uint32_t tlo, const uint32_t thi, const uint32_t Z)
    {
        uint32_t d, h;
        if (EDGE)
            asm("v_perm_b32 %[d], %[thi], %[tlo], %[g]\n\t"
                "v_mov_b32 %[f], %[sn]\n\t"
                "v_add_u32 %[d], %[s], %[d]\n\t"
                "v_pk_max_u16 %[h], %[sn], %[z]\n\t"
                "v_pk_max_u16 %[h], %[h], %[d]\n\t"
                "v_pk_max_u16 %[h], %[h], %[e]\n\t"
                "v_sub_u32 %[s], %[h], %[dd]\n\t"
                "v_add_u32 %[d], %[sj], %[h]\n\t"
                "v_pk_max_u16 %[e], %[e], %[s]\n\t"
                "v_sub_u32 %[e], %[e], %[gg]\n\t"
                "v_pk_max_u16 %[rk], %[rk], %[d]"
                : [f] "=&v"(Fj), [d] "=&v"(d), [h] "=&v"(h), [s] "+v"(Sj), [e] "+v"(E), [rk] "+v"(rowkey)
                : [g] "v"(g), [tlo] "v"(tlo), [thi] "v"(thi), [sn] "v"(Snext), [dd] "v"(D), [gg] "v"(G), [z] "v"(Z), [sj] "n"(J * 0x10001));
        else
            asm("v_perm_b32 %[d], %[thi], %[tlo], %[g]\n\t"
                "v_pk_max_u16 %[f], %[fn], %[sn]\n\t"
                "v_add_u32 %[d], %[s], %[d]\n\t"
                "v_pk_max_u16 %[h], %[f], %[z]\n\t"
                "v_pk_max_u16 %[h], %[h], %[d]\n\t"
                "v_pk_max_u16 %[h], %[h], %[e]\n\t"
                "v_sub_u32 %[s], %[h], %[dd]\n\t"
                "v_add_u32 %[d], %[sj], %[h]\n\t"
                "v_pk_max_u16 %[e], %[e], %[s]\n\t"
                "v_sub_u32 %[e], %[e], %[gg]\n\t"
                "v_pk_max_u16 %[rk], %[rk], %[d]"
                : [f] "=&v"(Fj), [d] "=&v"(d), [h] "=&v"(h), [s] "+v"(Sj), [e] "+v"(E), [rk] "+v"(rowkey)
                : [g] "v"(g), [tlo] "v"(tlo), [thi] "v"(thi), [fn] "v"(Fnext), [sn] "v"(Snext), [dd] "v"(D), [gg] "v"(G), [z] "v"(Z), [sj] "n"(J * 0x10001));
    }

    template <int BAND, int R, int J, int END>
    struct Cells {
        static __device__ __forceinline__ void run(PairState<BAND>& st, uint32_t& E, uint32_t& rowkey, const uint32_t D, const uint32_t G, const uint32_t tlo, const uint32_t thi)
        {
            cell<J, J + 1 == BAND - 1>(st.F[J], st.F[J + 1 < BAND - 1 ? J + 1 : 0], st.S[J + 1], st.S[J], E, rowkey, st.tc[(R + J) & 15], D, G, tlo, thi, st.z);
            Cells<BAND, R, J + 1, END>::run(st, E, rowkey, D, G, tlo, thi);
        }
    };
    template <int BAND, int R, int END>
    struct Cells<BAND, R, END, END> {
        static __device__ __forceinline__ void run(PairState<BAND>&, uint32_t&, uint32_t&, uint32_t, uint32_t, uint32_t, uint32_t) {}
    };

    // row i0 + R of both jobs.  g_new: the entering text symbols' selector; {tlo, thi}: the row's table, four byte entries per job
    template <int BAND, int R, int FORM>
    static __device__ __forceinline__ void row(PairState<BAND>& st, const uint32_t i, const uint32_t D, const uint32_t G, const uint32_t g_new, const uint32_t tlo, const uint32_t thi)
    {
        st.z += G;                                                                     // this row's zero
        // j == 0
        st.F[0] = (1 == BAND - 1) ? st.S[1] : mx(st.F[1 < BAND - 1 ? 1 : 0], st.S[1]);
        uint32_t hi = mx(mx(st.F[0], st.S[0] + subst(tlo, thi, st.tc[R & 15])), st.z);
        uint32_t rowkey = hi;
        st.S[0] = hi - D;
        uint32_t E = st.S[0] - G;
        // 1 <= j <= BAND-2
        Cells<BAND, R, 1, BAND - 1>::run(st, E, rowkey, D, G, tlo, thi);
        st.tc[(R + BAND - 1) & 15] = g_new;
        // j == BAND-1
        hi = mx(mx(E, st.S[BAND - 1] + subst(tlo, thi, g_new)), st.z);
        rowkey = mx(rowkey, hi + uint32_t(BAND - 1) * 0x10001u);
        st.S[BAND - 1] = hi - D;
        sink<FORM>(st, rowkey, i);
    }
};

// ---- the max3 cell: three-input maxima on halves kept inside the positive normal f16 patterns (the header comment has the argument)
constexpr int32_t PM3_ROW_LIMIT = (0x7BFF - 255 - 0x0400 - 448) / 32;             // 938 >= M (S+ + |G_e|)
struct PM3 : PairOps {
    static constexpr int32_t FLOOR = 0x0400;
    static __device__ __forceinline__ uint32_t mx3(uint32_t a, uint32_t b, uint32_t c) { uint32_t r; asm("v_pk_maximum3_f16 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }

    // the interior cells J and J + 1 of both jobs, neither next to the band's edge.  F2 / S2: F'(i-1,J+2) and S(i-1,J+2).  F1 and S1 are
    // read as the previous row's (cell J's F', cell J + 1's diagonal) before cell J + 1 overwrites them.  The serial chain per cell is
    // E -> h -> S -> E as in P16 (max3, sub, max, sub); both F' and both diagonals are ready before E joins.
    template <int J>
    static __device__ __forceinline__ void cell2(uint32_t& F0, uint32_t& F1, const uint32_t F2, uint32_t& S0, uint32_t& S1, const uint32_t S2, uint32_t& E, uint32_t& rowkey,
                                                 const uint32_t g0, const uint32_t g1, const uint32_t D, const uint32_t G, const uint32_t tlo, const uint32_t thi, const uint32_t Z)
    {
        uint32_t d0, d1, h;
        asm("v_perm_b32 %[d0], %[thi], %[tlo], %[g0]\n\t"
            "v_perm_b32 %[d1], %[thi], %[tlo], %[g1]\n\t"
            "v_pk_maximum3_f16 %[f0], %[f1], %[s1], %[z]\n\t"
            "v_pk_maximum3_f16 %[f1], %[f2], %[s2], %[z]\n\t"
            "v_add_u32 %[d0], %[s0], %[d0]\n\t"
            "v_add_u32 %[d1], %[s1], %[d1]\n\t"
            "v_pk_maximum3_f16 %[h], %[f0], %[d0], %[e]\n\t"
            "v_sub_u32 %[s0], %[h], %[dd]\n\t"
            "v_add_u32 %[d0], %[j0], %[h]\n\t"
            "v_pk_max_u16 %[e], %[e], %[s0]\n\t"
            "v_sub_u32 %[e], %[e], %[gg]\n\t"
            "v_pk_maximum3_f16 %[h], %[f1], %[d1], %[e]\n\t"
            "v_sub_u32 %[s1], %[h], %[dd]\n\t"
            "v_add_u32 %[d1], %[j1], %[h]\n\t"
            "v_pk_max_u16 %[e], %[e], %[s1]\n\t"
            "v_sub_u32 %[e], %[e], %[gg]\n\t"
            "v_pk_maximum3_f16 %[rk], %[rk], %[d0], %[d1]"
            : [f0] "=&v"(F0), [f1] "+&v"(F1), [d0] "=&v"(d0), [d1] "=&v"(d1), [h] "=&v"(h), [s0] "+&v"(S0), [s1] "+&v"(S1), [e] "+&v"(E), [rk] "+&v"(rowkey)
            : [g0] "v"(g0), [g1] "v"(g1), [tlo] "v"(tlo), [thi] "v"(thi), [f2] "v"(F2), [s2] "v"(S2), [dd] "v"(D), [gg] "v"(G), [z] "v"(Z),
              [j0] "n"(J * 0x10001), [j1] "n"((J + 1) * 0x10001));
    }

    // the cell J next to the band's edge (F(i-1,J+1) is the infimum: F' = max(S(i-1,J+1), Z)) and the last column J + 1 (no F:
    // h = max3(E, diagonal, Z))
    template <int J>
    static __device__ __forceinline__ void tail2(uint32_t& F0, uint32_t& S0, uint32_t& S1, uint32_t& E, uint32_t& rowkey,
                                                 const uint32_t g0, const uint32_t g1, const uint32_t D, const uint32_t G, const uint32_t tlo, const uint32_t thi, const uint32_t Z)
    {
        uint32_t d0, d1, h;
        asm("v_perm_b32 %[d0], %[thi], %[tlo], %[g0]\n\t"
            "v_perm_b32 %[d1], %[thi], %[tlo], %[g1]\n\t"
            "v_pk_max_u16 %[f0], %[s1], %[z]\n\t"
            "v_add_u32 %[d0], %[s0], %[d0]\n\t"
            "v_add_u32 %[d1], %[s1], %[d1]\n\t"
            "v_pk_maximum3_f16 %[h], %[f0], %[d0], %[e]\n\t"
            "v_sub_u32 %[s0], %[h], %[dd]\n\t"
            "v_add_u32 %[d0], %[j0], %[h]\n\t"
            "v_pk_max_u16 %[e], %[e], %[s0]\n\t"
            "v_sub_u32 %[e], %[e], %[gg]\n\t"
            "v_pk_maximum3_f16 %[h], %[e], %[d1], %[z]\n\t"
            "v_sub_u32 %[s1], %[h], %[dd]\n\t"
            "v_add_u32 %[d1], %[j1], %[h]\n\t"
            "v_pk_maximum3_f16 %[rk], %[rk], %[d0], %[d1]"
            : [f0] "=&v"(F0), [d0] "=&v"(d0), [d1] "=&v"(d1), [h] "=&v"(h), [s0] "+&v"(S0), [s1] "+&v"(S1), [e] "+&v"(E), [rk] "+&v"(rowkey)
            : [g0] "v"(g0), [g1] "v"(g1), [tlo] "v"(tlo), [thi] "v"(thi), [dd] "v"(D), [gg] "v"(G), [z] "v"(Z),
              [j0] "n"(J * 0x10001), [j1] "n"((J + 1) * 0x10001));
    }

    template <int BAND, int R, int J, int END>
    struct Cells {
        static __device__ __forceinline__ void run(PairState<BAND>& st, uint32_t& E, uint32_t& rowkey, const uint32_t D, const uint32_t G, const uint32_t tlo, const uint32_t thi)
        {
            cell2<J>(st.F[J], st.F[J + 1], st.F[J + 2], st.S[J], st.S[J + 1], st.S[J + 2], E, rowkey, st.tc[(R + J) & 15], st.tc[(R + J + 1) & 15], D, G, tlo, thi, st.z);
            Cells<BAND, R, J + 2, END>::run(st, E, rowkey, D, G, tlo, thi);
        }
    };
    template <int BAND, int R, int END>
    struct Cells<BAND, R, END, END> {
        static __device__ __forceinline__ void run(PairState<BAND>&, uint32_t&, uint32_t&, uint32_t, uint32_t, uint32_t, uint32_t) {}
    };

    template <int BAND, int R, int FORM>
    static __device__ __forceinline__ void row(PairState<BAND>& st, const uint32_t i, const uint32_t D, const uint32_t G, const uint32_t g_new, const uint32_t tlo, const uint32_t thi)
    {
        static_assert(BAND % 2 == 1, "columns 1 ... BAND-3 go two at a time");
        st.z += G;                                                                     // this row's zero
        // j == 0: no E
        st.F[0] = (1 == BAND - 1) ? mx(st.S[1], st.z) : mx3(st.F[1 < BAND - 1 ? 1 : 0], st.S[1], st.z);
        const uint32_t hi = mx(st.F[0], st.S[0] + subst(tlo, thi, st.tc[R & 15]));
        uint32_t rowkey = hi;
        st.S[0] = hi - D;
        uint32_t E = st.S[0] - G;
        // 1 <= j <= BAND-3, then BAND-2 and BAND-1
        Cells<BAND, R, 1, BAND - 2>::run(st, E, rowkey, D, G, tlo, thi);
        st.tc[(R + BAND - 1) & 15] = g_new;
        tail2<BAND - 2>(st.F[BAND - 2], st.S[BAND - 2], st.S[BAND - 1], E, rowkey, st.tc[(R + BAND - 2) & 15], g_new, D, G, tlo, thi, st.z);
        sink<FORM>(st, rowkey, i);
    }
};

// ---- the max3 cell in the column frame: E pays no gap subtract, the row's zeros and the cell's constants are scalars (the header
// comment, "The column frame")
// the largest operand of a PD3 maximum (a diagonal of the last row's last column), which must not pass PD3_TOP; D, G times 32 as in the kernel
constexpr int32_t PD3_TOP = 0x7BFF, PD3_BYTE_LIMIT = 7;                            // 7 >= max(match, mismatch) - G_o + |G_e|: the table's byte
constexpr int64_t pd3_top(int64_t D, int64_t G, int64_t M, int64_t s_plus, int64_t band = 15)
{
    return 0x0400 + D + G + G * (2 * M + band - 1) + 32 * M * s_plus + 255;
}
// what a wave shares, all of it in scalar registers: the ring of the row's zeros, Z(i,j) at index (2 i + j) & 15; the keys' constants
// K_j = j + (BAND - 1 - j) G; D; the ring's step 16 G
template <int BAND>
struct ColumnFrame {
    uint32_t z[16];
    uint32_t k[BAND];
    uint32_t D, step;
    uint32_t pair;           // 2 G, what a row key gains on its way into the next row's frame (PF_FOLD2)
};
struct PD3 : PairOps {
    static constexpr bool COLUMN = true;
    static constexpr int32_t FLOOR = 0x0400;

    // PF_CONST2: K_j = j + (14 - j) G of band 15 for the form's |G_e|, both halves, as the signed 32-bit literal an "n" operand takes
    template <int FORM> static constexpr int32_t klit(int j)     { return int32_t(uint32_t(j + (14 - j) * 32 * pair_ge(FORM)) * 0x10001u); }
    template <int FORM> static constexpr int32_t pairlit()       { return int32_t(uint32_t(2 * 32 * pair_ge(FORM)) * 0x10001u); }

    // column 0 (no E): F' = max3(F'(i-1,1), S'(i-1,1), Z(i,0)), h = max(F', diagonal); its key seeds the row key, its S' is column 1's E'
    // (the asm texts are macros: PF_CONST2 runs the same instructions with other operand classes)
    // L: where the diagonals' substitution words come from (the header comment, "Where the substitution comes from"): the lookup, one
    // v_perm_b32 per column; nothing under PF_SUBLDS, whose words arrive from LDS in g0 / g1; the probe's PF_KO_PERM, a v_xor_b32 of two
    // resident registers in the lookup's place
#define NVB_PD3_PERM1 "v_perm_b32 %[d], %[thi], %[tlo], %[g0]\n\t"
#define NVB_PD3_PERM2 "v_perm_b32 %[d0], %[thi], %[tlo], %[g0]\n\t" "v_perm_b32 %[d1], %[thi], %[tlo], %[g1]\n\t"
#define NVB_PD3_XOR1  "v_xor_b32 %[d], %[tlo], %[g0]\n\t"
#define NVB_PD3_XOR2  "v_xor_b32 %[d0], %[tlo], %[g0]\n\t" "v_xor_b32 %[d1], %[tlo], %[g1]\n\t"
#define NVB_PD3_COL0_(L, P, Q) L \
            "v_pk_maximum3_f16 %[f0], %[f1], %[s1], %[z0]\n\t" \
            "v_add_u32 %[d], %[s0], %[d]\n\t" P \
            "v_pk_max_u16 %[h], %[f0], %[d]\n\t" \
            "v_subrev_u32 %[s0], %[dd], %[h]\n\t" \
            "v_add_u32 %[rk], %[k0], %[h]" Q
#define NVB_PD3_COL0(L) NVB_PD3_COL0_(L, "", "")
#define NVB_PD3_COL0_OUT [f0] "=&v"(F0), [d] "=&v"(d), [h] "=&v"(h), [s0] "+&v"(S0), [rk] "=&v"(rowkey)
#define NVB_PD3_COL0_IN  [g0] "v"(g0), [tlo] "v"(tlo), [thi] "v"(thi), [f1] "v"(F1), [s1] "v"(S1), [z0] "s"(Z0)
    template <int FORM>
    static __device__ __forceinline__ void col0(uint32_t& F0, const uint32_t F1, uint32_t& S0, const uint32_t S1, uint32_t& rowkey,
                                                const uint32_t g0, const uint32_t D, const uint32_t tlo, const uint32_t thi, const uint32_t Z0, const uint32_t K0)
    {
        uint32_t d = g0, h;
        if constexpr ((FORM & PF_PAD_EDGE) != 0)    asm(NVB_PD3_COL0_("", "s_nop 0\n\t", "\n\ts_nop 0") : [f0] "=&v"(F0), [d] "+&v"(d), [h] "=&v"(h), [s0] "+&v"(S0), [rk] "=&v"(rowkey)
                                                                         : [f1] "v"(F1), [s1] "v"(S1), [z0] "s"(Z0), [dd] "v"(D), [k0] "n"(klit<FORM>(0)));
        else if constexpr ((FORM & PF_SUBLDS) != 0) asm(NVB_PD3_COL0("") : [f0] "=&v"(F0), [d] "+&v"(d), [h] "=&v"(h), [s0] "+&v"(S0), [rk] "=&v"(rowkey)
                                                                         : [f1] "v"(F1), [s1] "v"(S1), [z0] "s"(Z0), [dd] "v"(D), [k0] "n"(klit<FORM>(0)));
        else if constexpr ((FORM & PF_KO_PERM) != 0) asm(NVB_PD3_COL0(NVB_PD3_XOR1) : NVB_PD3_COL0_OUT : NVB_PD3_COL0_IN, [dd] "v"(D), [k0] "n"(klit<FORM>(0)));
        else if constexpr ((FORM & PF_CONST2) != 0) asm(NVB_PD3_COL0(NVB_PD3_PERM1) : NVB_PD3_COL0_OUT : NVB_PD3_COL0_IN, [dd] "v"(D), [k0] "n"(klit<FORM>(0)));
        else                                        asm(NVB_PD3_COL0(NVB_PD3_PERM1) : NVB_PD3_COL0_OUT : NVB_PD3_COL0_IN, [dd] "s"(D), [k0] "s"(K0));
    }

    // PM3::cell2 without E's subtracts: E'(J+1) = max(E'(J), S'(J)).  Ein: E'(i,J), read only (column 1's is S'(i,0), which stays live as
    // the next row's diagonal); E: E'(i,J+2).  Z0, Z1: Z(i,J), Z(i,J+1); K0, K1: K_J, K_(J+1); they and D are scalars, one to an instruction.
    // P: PF_CONST2's pad behind each group of simple ops, or nothing
#define NVB_PD3_CELL2_(L, P, W0, W1) L \
            "v_pk_maximum3_f16 %[f0], %[f1], %[s1], %[z0]\n\t" \
            "v_pk_maximum3_f16 %[f1], %[f2], %[s2], %[z1]\n\t" \
            "v_add_u32 %[d0], %[s0], " W0 "\n\t" \
            "v_add_u32 %[d1], %[s1], " W1 "\n\t" P \
            "v_pk_maximum3_f16 %[h], %[f0], %[d0], %[ei]\n\t" \
            "v_subrev_u32 %[s0], %[dd], %[h]\n\t" \
            "v_add_u32 %[d0], %[k0], %[h]\n\t" P \
            "v_pk_max_u16 %[e], %[ei], %[s0]\n\t" \
            "v_pk_maximum3_f16 %[h], %[f1], %[d1], %[e]\n\t" \
            "v_subrev_u32 %[s1], %[dd], %[h]\n\t" \
            "v_add_u32 %[d1], %[k1], %[h]\n\t" P \
            "v_pk_max_u16 %[e], %[e], %[s1]\n\t" \
            "v_pk_maximum3_f16 %[rk], %[rk], %[d0], %[d1]"
// (W0, W1: where the diagonals' words stand: in d0 / d1 themselves, or, for the two halves of PF_SUBLDS2's 64-bit reads, in g0 / g1,
// which the cell only reads: a half of a register pair rewritten in place costs a v_mov_b32)
#define NVB_PD3_CELL2(L, P) NVB_PD3_CELL2_(L, P, "%[d0]", "%[d1]")
#define NVB_PD3_CELL2_OUT [f0] "=&v"(F0), [f1] "+&v"(F1), [d0] "=&v"(d0), [d1] "=&v"(d1), [h] "=&v"(h), [s0] "+&v"(S0), [s1] "+&v"(S1), [e] "=&v"(E), [rk] "+&v"(rowkey)
#define NVB_PD3_CELL2_IN  [g0] "v"(g0), [g1] "v"(g1), [tlo] "v"(tlo), [thi] "v"(thi), [f2] "v"(F2), [s2] "v"(S2), [ei] "v"(Ein), [z0] "s"(Z0), [z1] "s"(Z1)
    // J: the first of the two columns (PF_CONST2's literals are its and the next one's)
    template <int FORM, int J>
    static __device__ __forceinline__ void cell2(uint32_t& F0, uint32_t& F1, const uint32_t F2, uint32_t& S0, uint32_t& S1, const uint32_t S2, const uint32_t Ein, uint32_t& E,
                                                 uint32_t& rowkey, const uint32_t g0, const uint32_t g1, const uint32_t D, const uint32_t tlo, const uint32_t thi,
                                                 const uint32_t Z0, const uint32_t Z1, const uint32_t K0, const uint32_t K1)
    {
        uint32_t d0 = g0, d1 = g1, h;
        if constexpr ((FORM & PF_SUBLDS2) != 0)
            asm(NVB_PD3_CELL2_("", "s_nop 0\n\t", "%[g0]", "%[g1]")
                : [f0] "=&v"(F0), [f1] "+&v"(F1), [d0] "=&v"(d0), [d1] "=&v"(d1), [h] "=&v"(h), [s0] "+&v"(S0), [s1] "+&v"(S1), [e] "=&v"(E), [rk] "+&v"(rowkey)
                : [g0] "v"(g0), [g1] "v"(g1), [f2] "v"(F2), [s2] "v"(S2), [ei] "v"(Ein), [z0] "s"(Z0), [z1] "s"(Z1), [dd] "v"(D), [k0] "n"(klit<FORM>(J)), [k1] "n"(klit<FORM>(J + 1)));
        else if constexpr ((FORM & PF_SUBLDS) != 0)
            asm(NVB_PD3_CELL2("", "s_nop 0\n\t")
                : [f0] "=&v"(F0), [f1] "+&v"(F1), [d0] "+&v"(d0), [d1] "+&v"(d1), [h] "=&v"(h), [s0] "+&v"(S0), [s1] "+&v"(S1), [e] "=&v"(E), [rk] "+&v"(rowkey)
                : [f2] "v"(F2), [s2] "v"(S2), [ei] "v"(Ein), [z0] "s"(Z0), [z1] "s"(Z1), [dd] "v"(D), [k0] "n"(klit<FORM>(J)), [k1] "n"(klit<FORM>(J + 1)));
        else if constexpr ((FORM & PF_KO_PERM) != 0) asm(NVB_PD3_CELL2(NVB_PD3_XOR2, "s_nop 0\n\t") : NVB_PD3_CELL2_OUT : NVB_PD3_CELL2_IN, [dd] "v"(D), [k0] "n"(klit<FORM>(J)), [k1] "n"(klit<FORM>(J + 1)));
        else if constexpr ((FORM & PF_CONST2) != 0) asm(NVB_PD3_CELL2(NVB_PD3_PERM2, "s_nop 0\n\t") : NVB_PD3_CELL2_OUT : NVB_PD3_CELL2_IN, [dd] "v"(D), [k0] "n"(klit<FORM>(J)), [k1] "n"(klit<FORM>(J + 1)));
        else                                        asm(NVB_PD3_CELL2(NVB_PD3_PERM2, "") : NVB_PD3_CELL2_OUT : NVB_PD3_CELL2_IN, [dd] "s"(D), [k0] "s"(K0), [k1] "s"(K1));
    }

    // PM3::tail2 in the column frame: the cell J next to the band's edge (F' = max(S'(i-1,J+1), Z(i,J))) and the last column J + 1
    // (h = max3(E', diagonal, Z(i,J+1)))
#define NVB_PD3_TAIL2_(L, P, W0, W1) L \
            "v_pk_max_u16 %[f0], %[s1], %[z0]\n\t" \
            "v_add_u32 %[d0], %[s0], " W0 "\n\t" \
            "v_add_u32 %[d1], %[s1], " W1 "\n\t" P \
            "v_pk_maximum3_f16 %[h], %[f0], %[d0], %[ei]\n\t" \
            "v_subrev_u32 %[s0], %[dd], %[h]\n\t" \
            "v_add_u32 %[d0], %[k0], %[h]\n\t" P \
            "v_pk_max_u16 %[e], %[ei], %[s0]\n\t" \
            "v_pk_maximum3_f16 %[h], %[e], %[d1], %[z1]\n\t" \
            "v_subrev_u32 %[s1], %[dd], %[h]\n\t" \
            "v_add_u32 %[d1], %[k1], %[h]\n\t" P \
            "v_pk_maximum3_f16 %[rk], %[rk], %[d0], %[d1]"
#define NVB_PD3_TAIL2(L) NVB_PD3_TAIL2_(L, "", "%[d0]", "%[d1]")
#define NVB_PD3_TAIL2_OUT [f0] "=&v"(F0), [d0] "=&v"(d0), [d1] "=&v"(d1), [h] "=&v"(h), [e] "=&v"(e), [s0] "+&v"(S0), [s1] "+&v"(S1), [rk] "+&v"(rowkey)
#define NVB_PD3_TAIL2_IN  [g0] "v"(g0), [g1] "v"(g1), [tlo] "v"(tlo), [thi] "v"(thi), [ei] "v"(Ein), [z0] "s"(Z0), [z1] "s"(Z1)
    template <int FORM, int J>
    static __device__ __forceinline__ void tail2(uint32_t& F0, uint32_t& S0, uint32_t& S1, const uint32_t Ein, uint32_t& rowkey,
                                                 const uint32_t g0, const uint32_t g1, const uint32_t D, const uint32_t tlo, const uint32_t thi,
                                                 const uint32_t Z0, const uint32_t Z1, const uint32_t K0, const uint32_t K1)
    {
        uint32_t d0 = g0, d1 = g1, h, e;
        if constexpr ((FORM & PF_SUBLDS2) != 0 && (FORM & PF_PAD_EDGE) != 0)
            asm(NVB_PD3_TAIL2_("", "s_nop 0\n\t", "%[g0]", "%[g1]") : NVB_PD3_TAIL2_OUT
                : [g0] "v"(g0), [g1] "v"(g1), [ei] "v"(Ein), [z0] "s"(Z0), [z1] "s"(Z1), [dd] "v"(D), [k0] "n"(klit<FORM>(J)), [k1] "n"(klit<FORM>(J + 1)));
        else if constexpr ((FORM & PF_SUBLDS2) != 0)
            asm(NVB_PD3_TAIL2_("", "", "%[g0]", "%[g1]") : NVB_PD3_TAIL2_OUT
                : [g0] "v"(g0), [g1] "v"(g1), [ei] "v"(Ein), [z0] "s"(Z0), [z1] "s"(Z1), [dd] "v"(D), [k0] "n"(klit<FORM>(J)), [k1] "n"(klit<FORM>(J + 1)));
        else if constexpr ((FORM & PF_PAD_EDGE) != 0)
            asm(NVB_PD3_TAIL2_("", "s_nop 0\n\t", "%[d0]", "%[d1]")
                : [f0] "=&v"(F0), [d0] "+&v"(d0), [d1] "+&v"(d1), [h] "=&v"(h), [e] "=&v"(e), [s0] "+&v"(S0), [s1] "+&v"(S1), [rk] "+&v"(rowkey)
                : [ei] "v"(Ein), [z0] "s"(Z0), [z1] "s"(Z1), [dd] "v"(D), [k0] "n"(klit<FORM>(J)), [k1] "n"(klit<FORM>(J + 1)));
        else if constexpr ((FORM & PF_SUBLDS) != 0)
            asm(NVB_PD3_TAIL2("")
                : [f0] "=&v"(F0), [d0] "+&v"(d0), [d1] "+&v"(d1), [h] "=&v"(h), [e] "=&v"(e), [s0] "+&v"(S0), [s1] "+&v"(S1), [rk] "+&v"(rowkey)
                : [ei] "v"(Ein), [z0] "s"(Z0), [z1] "s"(Z1), [dd] "v"(D), [k0] "n"(klit<FORM>(J)), [k1] "n"(klit<FORM>(J + 1)));
        else if constexpr ((FORM & PF_KO_PERM) != 0) asm(NVB_PD3_TAIL2(NVB_PD3_XOR2) : NVB_PD3_TAIL2_OUT : NVB_PD3_TAIL2_IN, [dd] "v"(D), [k0] "n"(klit<FORM>(J)), [k1] "n"(klit<FORM>(J + 1)));
        else if constexpr ((FORM & PF_CONST2) != 0) asm(NVB_PD3_TAIL2(NVB_PD3_PERM2) : NVB_PD3_TAIL2_OUT : NVB_PD3_TAIL2_IN, [dd] "v"(D), [k0] "n"(klit<FORM>(J)), [k1] "n"(klit<FORM>(J + 1)));
        else                                        asm(NVB_PD3_TAIL2(NVB_PD3_PERM2) : NVB_PD3_TAIL2_OUT : NVB_PD3_TAIL2_IN, [dd] "s"(D), [k0] "s"(K0), [k1] "s"(K1));
    }

    template <int BAND, int R, int FORM, int J, int END>
    struct Cells {
        static __device__ __forceinline__ void run(PairState<BAND>& st, const ColumnFrame<BAND>& fr, const uint32_t Ein, uint32_t& E, uint32_t& rowkey, const uint32_t tlo, const uint32_t thi)
        {
            uint32_t En;
            cell2<FORM, J>(st.F[J], st.F[J + 1], st.F[J + 2], st.S[J], st.S[J + 1], st.S[J + 2], Ein, En, rowkey, st.tc[(R + J) & 15], st.tc[(R + J + 1) & 15], fr.D, tlo, thi,
                           fr.z[(2 * R + J) & 15], fr.z[(2 * R + J + 1) & 15], fr.k[J], fr.k[J + 1]);
            Cells<BAND, R, FORM, J + 2, END>::run(st, fr, En, E, rowkey, tlo, thi);
        }
    };
    template <int BAND, int R, int FORM, int END>
    struct Cells<BAND, R, FORM, END, END> {
        static __device__ __forceinline__ void run(PairState<BAND>&, const ColumnFrame<BAND>&, const uint32_t Ein, uint32_t& E, uint32_t&, uint32_t, uint32_t) { E = Ein; }
    };

    // PF_SUBLDS: the same cells on the row's words w[j], which its head has read from the block's table
    template <int BAND, int R, int FORM, int J, int END>
    struct SubCells {
        static __device__ __forceinline__ void run(PairState<BAND>& st, const ColumnFrame<BAND>& fr, const uint32_t Ein, uint32_t& E, uint32_t& rowkey, const uint32_t (&w)[BAND])
        {
            uint32_t En;
            cell2<FORM, J>(st.F[J], st.F[J + 1], st.F[J + 2], st.S[J], st.S[J + 1], st.S[J + 2], Ein, En, rowkey, w[J], w[J + 1], fr.D, 0u, 0u,
                           fr.z[(2 * R + J) & 15], fr.z[(2 * R + J + 1) & 15], fr.k[J], fr.k[J + 1]);
            SubCells<BAND, R, FORM, J + 2, END>::run(st, fr, En, E, rowkey, w);
        }
    };
    template <int BAND, int R, int FORM, int END>
    struct SubCells<BAND, R, FORM, END, END> {
        static __device__ __forceinline__ void run(PairState<BAND>&, const ColumnFrame<BAND>&, const uint32_t Ein, uint32_t& E, uint32_t&, const uint32_t (&)[BAND]) { E = Ein; }
    };

    // PF_SUBLDS2: pair k's read, the words of columns 2 k - 1 and 2 k of row R, and the cells with the reads sub2_ahead() pairs ahead of them
    template <int FORM> static constexpr int sub2_ahead() { return (FORM & PF_AHEAD2) ? 2 : 1; }   // (two: the probe's; 96 VGPRs and one register spilled around the block loop)
    template <int BAND, int R, int FORM>
    static __device__ __forceinline__ void sub2_read(const PairState<BAND>& st, uint32_t (&w)[BAND], const uint32_t rw, const uint32_t* sub, const int k)
    {
        uint32_t a = rw ^ st.tc[(R + 2 * k - 1) & 15];
        if constexpr ((FORM & PF_PAD_XOR) != 0) asm volatile("s_nop 0" : "+v"(a));
        const uint2 t = *reinterpret_cast<const uint2*>(reinterpret_cast<const char*>(sub) + a);
        w[2 * k - 1] = t.x; w[2 * k] = t.y;
    }
    template <int BAND, int R, int FORM, int K, int END>
    struct Sub2Cells {
        static __device__ __forceinline__ void run(PairState<BAND>& st, const ColumnFrame<BAND>& fr, const uint32_t Ein, uint32_t& E, uint32_t& rowkey, uint32_t (&w)[BAND],
                                                   const uint32_t rw, const uint32_t* sub)
        {
            uint32_t En;
            if constexpr (K + sub2_ahead<FORM>() <= (BAND - 1) / 2) sub2_read<BAND, R, FORM>(st, w, rw, sub, K + sub2_ahead<FORM>());
            SubCells<BAND, R, FORM, 2 * K - 1, 2 * K + 1>::run(st, fr, Ein, En, rowkey, w);
            Sub2Cells<BAND, R, FORM, K + 1, END>::run(st, fr, En, E, rowkey, w, rw, sub);
        }
    };
    template <int BAND, int R, int FORM, int END>
    struct Sub2Cells<BAND, R, FORM, END, END> {
        static __device__ __forceinline__ void run(PairState<BAND>&, const ColumnFrame<BAND>&, const uint32_t Ein, uint32_t& E, uint32_t&, uint32_t (&)[BAND], uint32_t, const uint32_t*) { E = Ein; }
    };

    // the wave's frame before row 0: slot s of the ring holds Z(0, s) = BIAS' + G (2 + s) for the columns row 0's prologue leaves alone and
    // 16 G less for the two it advances (and for slot 15, which row 1 advances before its first use)
    template <int BAND>
    static __device__ __forceinline__ void open(ColumnFrame<BAND>& fr, const int32_t d32, const int32_t g32)
    {
        #pragma unroll
        for (int s = 0; s < 16; ++s) fr.z[s] = rep(d32 + g32 + FLOOR + g32 * (2 + (s <= BAND - 3 ? s : s - 16)));
        #pragma unroll
        for (int j = 0; j < BAND; ++j) fr.k[j] = rep(j + (BAND - 1 - j) * g32);
        fr.D = rep(d32);
        fr.step = rep(16 * g32);
        fr.pair = rep(2 * g32);
    }

    // rk2 (PF_FOLD2): the even row's row key, which waits for the odd row's
    template <int BAND, int R, int FORM>
    static __device__ __forceinline__ void row(PairState<BAND>& st, ColumnFrame<BAND>& fr, const uint32_t i, const uint32_t g_new, const uint32_t tlo, const uint32_t thi, uint32_t& rk2,
                                               const uint32_t* sub = nullptr)
    {
        static_assert(BAND == 15, "a row's zeros, 2 i ... 2 i + BAND - 1, and the two the next row adds fill the ring of 16; columns go two at a time");
        // this row's zeros: Z(i, BAND-2) and Z(i, BAND-1) take the slots of Z(i-1, 0) - G and Z(i-1, 0); scalar adds
        fr.z[(2 * R + BAND - 2) & 15] += fr.step;
        fr.z[(2 * R + BAND - 1) & 15] += fr.step;
        uint32_t rowkey, E;
        if constexpr ((FORM & PF_SUBLDS2) != 0)
        {
            // g_new: the entering pair's column word, (i + 13, i + 14); tlo: the row word; sub: the block's table of pairs.  Column 0 reads
            // the first word of its pair (i, i + 1), columns 1 ... 14 go two to a read, pair k = 1 ... 7 for columns 2 k - 1 and 2 k.  The
            // reads run sub2_ahead() pairs ahead of the cells, one: a cell's pair is read while the cell before it runs (Sub2Cells)
            st.tc[(R + BAND - 2) & 15] = g_new;
            uint32_t w[BAND];
            uint32_t a0 = tlo ^ st.tc[R & 15];
            if constexpr ((FORM & PF_PAD_XOR) != 0) asm volatile("s_nop 0" : "+v"(a0));
            w[0] = *reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(sub) + a0);
            #pragma unroll
            for (int k = 1; k <= sub2_ahead<FORM>(); ++k) sub2_read<BAND, R, FORM>(st, w, tlo, sub, k);
            col0<FORM>(st.F[0], st.F[1], st.S[0], st.S[1], rowkey, w[0], fr.D, 0u, 0u, fr.z[(2 * R) & 15], fr.k[0]);
            Sub2Cells<BAND, R, FORM, 1, (BAND - 1) / 2>::run(st, fr, st.S[0], E, rowkey, w, tlo, sub);
            tail2<FORM, BAND - 2>(st.F[BAND - 2], st.S[BAND - 2], st.S[BAND - 1], E, rowkey, w[BAND - 2], w[BAND - 1], fr.D, 0u, 0u,
                                  fr.z[(2 * R + BAND - 2) & 15], fr.z[(2 * R + BAND - 1) & 15], fr.k[BAND - 2], fr.k[BAND - 1]);
        }
        else if constexpr ((FORM & PF_KO_XOR8) != 0)
        {
            // the probe's ceiling for the form above: PF_SUBLDS's row and table with a read of two adjacent words for every other column,
            // eight xors and eight reads; the second word is whatever follows the first in the table (the kernel pads it by one)
            struct alignas(4) W2 { uint32_t x, y; };
            constexpr int HEAD = 8, SPLIT = 5;
            st.tc[(R + BAND - 1) & 15] = g_new;
            uint32_t w[BAND], Em;
            #pragma unroll
            for (int j = 0; j < HEAD; j += 2) { const W2 t = *reinterpret_cast<const W2*>(reinterpret_cast<const char*>(sub) + (tlo ^ st.tc[(R + j) & 15])); w[j] = t.x; if (j + 1 < BAND) w[j + 1] = t.y; }
            col0<FORM>(st.F[0], st.F[1], st.S[0], st.S[1], rowkey, w[0], fr.D, 0u, 0u, fr.z[(2 * R) & 15], fr.k[0]);
            SubCells<BAND, R, FORM, 1, SPLIT>::run(st, fr, st.S[0], Em, rowkey, w);
            #pragma unroll
            for (int j = HEAD; j < BAND; j += 2) { const W2 t = *reinterpret_cast<const W2*>(reinterpret_cast<const char*>(sub) + (tlo ^ st.tc[(R + j) & 15])); w[j] = t.x; if (j + 1 < BAND) w[j + 1] = t.y; }
            SubCells<BAND, R, FORM, SPLIT, BAND - 2>::run(st, fr, Em, E, rowkey, w);
            tail2<FORM, BAND - 2>(st.F[BAND - 2], st.S[BAND - 2], st.S[BAND - 1], E, rowkey, w[BAND - 2], w[BAND - 1], fr.D, 0u, 0u,
                                  fr.z[(2 * R + BAND - 2) & 15], fr.z[(2 * R + BAND - 1) & 15], fr.k[BAND - 2], fr.k[BAND - 1]);
        }
        else if constexpr ((FORM & PF_SUBLDS) != 0)
        {
            // g_new: the entering column word; tlo: the row word; sub: the block's table.  The reads go out in two batches, each in the
            // order the cells take its words, so the counted waits fall before each cell block: columns 0 ... 7 at the row's head, the
            // rest behind column 4, into the registers columns 0 ... 4 have given back (fifteen landing registers do not fit 96)
            constexpr int HEAD = 8, SPLIT = 5;
            st.tc[(R + BAND - 1) & 15] = g_new;
            uint32_t w[BAND], Em;
            if constexpr ((FORM & PF_PAD_XOR) != 0)                                    // the probe's pad behind each run of xors
            {
                uint32_t a[HEAD];
                #pragma unroll
                for (int j = 0; j < HEAD; ++j) a[j] = tlo ^ st.tc[(R + j) & 15];
                asm volatile("s_nop 0" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(a[6]), "+v"(a[7]));
                #pragma unroll
                for (int j = 0; j < HEAD; ++j) w[j] = *reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(sub) + a[j]);
            }
            else
            {
                #pragma unroll
                for (int j = 0; j < HEAD; ++j) w[j] = *reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(sub) + (tlo ^ st.tc[(R + j) & 15]));
            }
            col0<FORM>(st.F[0], st.F[1], st.S[0], st.S[1], rowkey, w[0], fr.D, 0u, 0u, fr.z[(2 * R) & 15], fr.k[0]);
            SubCells<BAND, R, FORM, 1, SPLIT>::run(st, fr, st.S[0], Em, rowkey, w);
            if constexpr ((FORM & PF_PAD_XOR) != 0)
            {
                uint32_t a[BAND - HEAD];
                #pragma unroll
                for (int j = HEAD; j < BAND; ++j) a[j - HEAD] = tlo ^ st.tc[(R + j) & 15];
                asm volatile("s_nop 0" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(a[6]));
                #pragma unroll
                for (int j = HEAD; j < BAND; ++j) w[j] = *reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(sub) + a[j - HEAD]);
            }
            else
            {
                #pragma unroll
                for (int j = HEAD; j < BAND; ++j) w[j] = *reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(sub) + (tlo ^ st.tc[(R + j) & 15]));
            }
            SubCells<BAND, R, FORM, SPLIT, BAND - 2>::run(st, fr, Em, E, rowkey, w);
            tail2<FORM, BAND - 2>(st.F[BAND - 2], st.S[BAND - 2], st.S[BAND - 1], E, rowkey, w[BAND - 2], w[BAND - 1], fr.D, 0u, 0u,
                                  fr.z[(2 * R + BAND - 2) & 15], fr.z[(2 * R + BAND - 1) & 15], fr.k[BAND - 2], fr.k[BAND - 1]);
        }
        else
        {
            col0<FORM>(st.F[0], st.F[1], st.S[0], st.S[1], rowkey, st.tc[R & 15], fr.D, tlo, thi, fr.z[(2 * R) & 15], fr.k[0]);
            // 1 <= j <= BAND-3, then BAND-2 and BAND-1
            Cells<BAND, R, FORM, 1, BAND - 2>::run(st, fr, st.S[0], E, rowkey, tlo, thi);
            st.tc[(R + BAND - 1) & 15] = g_new;
            tail2<FORM, BAND - 2>(st.F[BAND - 2], st.S[BAND - 2], st.S[BAND - 1], E, rowkey, st.tc[(R + BAND - 2) & 15], g_new, fr.D, tlo, thi,
                                  fr.z[(2 * R + BAND - 2) & 15], fr.z[(2 * R + BAND - 1) & 15], fr.k[BAND - 2], fr.k[BAND - 1]);
        }
        if constexpr ((FORM & PF_FOLD2) != 0)
        {
            // the header comment, "The pair fold": the even row's key moves into the odd row's frame (2 G up), the odd row's takes the
            // pair's bit, and one fold serves both under the even row's number
            if constexpr ((R & 1) == 0) rk2 = rowkey;
            else fold<FORM>(st, mx(rk2 + ((FORM & PF_CONST2) ? uint32_t(pairlit<FORM>()) : fr.pair), rowkey + rep(16)) - fr.z[(2 * R + BAND - 1) & 15], i - 1u);
        }
        else fold<FORM>(st, rowkey - fr.z[(2 * R + BAND - 1) & 15], i);               // the row key stands in the last column's frame
    }

    // PF_FOLD2, an odd number of rows: the last row has no partner and is folded alone as its pair's even row.  Its zero Z(M-1, BAND-1)
    // is worked out here, once per job
    template <int BAND, int FORM>
    static __device__ __forceinline__ void fold_last(PairState<BAND>& st, const uint32_t rk2, const uint32_t M, const int32_t d32, const int32_t g32)
    {
        fold<FORM>(st, rk2 - rep(d32 + g32 + FLOOR + g32 * int32_t(2u * M + BAND - 1)), M - 1u);
    }
};

template <typename CELL, int BAND, int FORM, int R, int END>
struct PairRows {
    // XT[0] / XT[1]: the block's entering text symbols 0-7 / 8-15, job A's in the low half and job B's in the high half
    // (KT: the resident table of the probe's PF_KO_TABLE, otherwise unused)
    // fr: the column frame's scalars (CELL::COLUMN; the row-frame cells take D and G instead)
    // rk2: the even row's row key, which the column frame's row carries to the odd row (PF_FOLD2; unused otherwise)
    // (NX: 2, or PF_SUBLDS2's 4)
    template <int NX>
    static __device__ __forceinline__ void run(PairState<BAND>& st, ColumnFrame<BAND>& fr, const uint32_t i0, const uint32_t M, const uint32_t D, const uint32_t G,
                                               const uint64_t PA, const uint64_t PB, const uint32_t (&XT)[NX], const uint32_t* tab, const uint32_t (&KT)[2], uint32_t& rk2)
    {
        if ((FORM & PF_KO_BOUND) || i0 + R < M)
        {
            if constexpr ((FORM & PF_SUBLDS2) != 0)
            {
                // PA / PB hold the block's row bytes of the even / the odd rows (sub2_row_words) and XT[q] the entering pair bytes of the
                // rows 4 m + q (sub2_col_words): both leave here as byte offsets, the row byte times 32 and the pair byte times 8
                constexpr int K = R >> 1, Q = R >> 2;
                const uint32_t zw = uint32_t(((R & 1) ? PB : PA) >> (32 * (K >> 2))), xw = XT[R & 3];
                uint32_t rw = (K & 3) == 0 ? (zw << 5) & 0x1FE0u : (zw >> ((8 * (K & 3) + 27) & 31)) & 0x1FE0u;
                uint32_t cw = Q == 0 ? (xw << 3) & 0x7F8u : (xw >> ((8 * Q + 29) & 31)) & 0x7F8u;
                asm("" : "+v"(rw)); asm("" : "+v"(cw));                               // whole words, as below
                CELL::template row<BAND, R, FORM>(st, fr, i0 + R, cw, rw, 0u, rk2, tab);
            }
            else if constexpr ((FORM & PF_SUBLDS) != 0)
            {
                // PA / PB hold the block's row words of the even / the odd rows, a byte each, and XT[0] / XT[1] the entering column
                // words of the even / the odd rows, a nibble each (sub_row_words; the kernel's block loop): both leave here as byte offsets
                constexpr int K = R >> 1;
                const uint32_t zw = uint32_t(((R & 1) ? PB : PA) >> (32 * (K >> 2))), xw = XT[R & 1];
                uint32_t rw = (K & 3) == 0 ? (zw << 2) & 0x3FCu : (zw >> ((8 * (K & 3) + 30) & 31)) & 0x3FCu;
                uint32_t cw = K == 0 ? (xw << 2) & 0x3Cu : (xw >> ((4 * K + 30) & 31)) & 0x3Cu;
                asm("" : "+v"(rw)); asm("" : "+v"(cw));                               // whole words: the cells' xors take no mask along (a three-source op, and a scalar)
                CELL::template row<BAND, R, FORM>(st, fr, i0 + R, cw, rw, 0u, rk2, tab);
            }
            else if constexpr (CELL::COLUMN)
            {
                const uint32_t g = ((XT[R >> 3] >> (2 * (R & 7))) & 0x00030003u) | CELL::SEL_BASE;
                if (FORM & PF_KO_TABLE) CELL::template row<BAND, R, FORM>(st, fr, i0 + R, g, KT[0], KT[1], rk2);
                else                    CELL::template row<BAND, R, FORM>(st, fr, i0 + R, g, tab[uint32_t(PA >> (4 * R)) & 15u], tab[uint32_t(PB >> (4 * R)) & 15u], rk2);
            }
            else
            {
                const uint32_t g = ((XT[R >> 3] >> (2 * (R & 7))) & 0x00030003u) | CELL::SEL_BASE;
                if (FORM & PF_KO_TABLE) CELL::template row<BAND, R, FORM>(st, i0 + R, D, G, g, KT[0], KT[1]);
                else                    CELL::template row<BAND, R, FORM>(st, i0 + R, D, G, g, tab[uint32_t(PA >> (4 * R)) & 15u], tab[uint32_t(PB >> (4 * R)) & 15u]);
            }
        }
        PairRows<CELL, BAND, FORM, R + 1, END>::run(st, fr, i0, M, D, G, PA, PB, XT, tab, KT, rk2);
    }
};
template <typename CELL, int BAND, int FORM, int END> struct PairRows<CELL, BAND, FORM, END, END> {
    template <int NX>
    static __device__ __forceinline__ void run(PairState<BAND>&, ColumnFrame<BAND>&, uint32_t, uint32_t, uint32_t, uint32_t, uint64_t, uint64_t, const uint32_t (&)[NX], const uint32_t*, const uint32_t (&)[2], uint32_t&) {}
};

// Lane k of the launch takes jobs 2k and 2k + 1 (with an odd n the last lane computes its one job in both halves).  The host has
// checked (banded_gotoh.hip: pair_admitted) that every job has M >= 1 rows, that no row sees a symbol past the text's end and that the
// scheme's scores fit the byte table, for CELL = PM3 and PD3 that M (S+ + |G_e|) <= PM3_ROW_LIMIT, and for PD3 its byte and its top (pair_column_admitted).  The strings are read from HBM per 16-row block: staging them in LDS as banded_gotoh_score_kernel
// does (two slots per lane) measured no faster with 256 lanes and slower with 128 (profiles/banded_pair/README.md), so there is none.
// FORM & PF_STREAM: the host has also checked that both word arrays are short enough for GroupStream's 32-bit byte offsets and has
// picked the instance of the pattern's width and the two byte orders (PF_PAT2, PF_PBE, PF_TBE), so the loop tests none of them; it
// loads three new words per job and block where fetch16_* loads five.
// PF_SUBLDS asks the compiler for five waves per SIMD (96 VGPRs), which its landing registers would otherwise pass by two; every other
// form keeps the default, 1, and the assembly it had.
constexpr int PAIR_LANES = 128;
template <int BAND, typename CELL, int FORM>
__global__ void __launch_bounds__(PAIR_LANES) __attribute__((amdgpu_waves_per_eu((FORM & PF_SUBLDS) ? 5 : 1)))
banded_gotoh_pair_kernel(const GotohParams p)
{
    static_assert(BAND >= 3 && BAND <= 16, "the ring of 16");
    constexpr bool STREAM = (FORM & PF_STREAM) != 0, KEY = (FORM & PF_SINK_KEY) != 0, FOLD2 = (FORM & PF_FOLD2) != 0, SUBLDS = (FORM & PF_SUBLDS) != 0, SUBLDS2 = (FORM & PF_SUBLDS2) != 0;
    static_assert(!(FORM & (PF_SUBLDS | PF_KO_PERM)) || ((FORM & PF_FOLD2) && (FORM & PF_CONST2) == PF_CONST2), "the LDS words and the probe's xor row are forms of the library's row");
    static_assert(!SUBLDS || !(FORM & (PF_KO_TABLE | PF_KO_PERM)), "the LDS words have no lookup to knock out");
    static_assert(!(FORM & (PF_SUBLDS2 | PF_KO_XOR8 | PF_PAD_XOR | PF_PAD_EDGE | PF_AHEAD2)) || SUBLDS, "the pair read, its ceiling and the pads are forms of the LDS words' row");
    static_assert(!SUBLDS2 || !(FORM & PF_KO_XOR8), "the ceiling is the single read's row");
    static_assert(!(FORM & (PF_FOLD2 | PF_CONST2)) || CELL::COLUMN, "the pair fold and the literals are the column frame's");
    static_assert(!FOLD2 || !(FORM & (PF_SINK_KEY | PF_KO_SINK | PF_KO_BOUND)), "the pair fold is the compare-and-select fold's, over the job's own rows");
    static_assert(!(FORM & PF_GE3) || (FORM & PF_CONST2), "|G_e| is the literal form's parameter");
    constexpr bool P4 = !(FORM & PF_PAT2), PBE = (FORM & PF_PBE) != 0, TBE = (FORM & PF_TBE) != 0;     // STREAM only: the host has matched them to the strings
    __shared__ uint32_t s_tab[16];           // by pattern symbol q: entry v = the pre-biased match score where v == q, the mismatch score elsewhere
    __shared__ uint32_t s_sub[(FORM & PF_KO_XOR8) ? 258 : 256];   // PF_SUBLDS: by sub_index of both jobs' codes nibble ^ symbol: {0, sub(c_B), 0, sub(c_A)}, sub(0) the match byte
    __shared__ uint2 s_sub2[1024];           // PF_SUBLDS2: by sub2_index, the words of two neighbouring cells (s_sub is not allocated then, nor s_sub2 elsewhere)
    if constexpr (SUBLDS2)
    {
        const uint32_t tg = uint32_t(-p.gap_ext * 32);
        const uint32_t sm = uint32_t((p.match - p.gap_open) * 32) + tg, sx = uint32_t((p.mismatch - p.gap_open) * 32) + tg;
        for (uint32_t k = threadIdx.x; k < 1024u; k += uint32_t(PAIR_LANES)) s_sub2[k] = make_uint2(sub2_word(k, 0u, sm, sx), sub2_word(k, 1u, sm, sx));
    }
    else if constexpr (SUBLDS)
    {
        if constexpr ((FORM & PF_KO_XOR8) != 0) { if (threadIdx.x < 2u) s_sub[256u + threadIdx.x] = 0u; }
        const uint32_t tg = uint32_t(-p.gap_ext * 32);
        const uint32_t sm = uint32_t((p.match - p.gap_open) * 32) + tg, sx = uint32_t((p.mismatch - p.gap_open) * 32) + tg;
        for (uint32_t k = threadIdx.x; k < 256u; k += uint32_t(PAIR_LANES))
            s_sub[k] = (sub_code_a(k) == 0u ? sm : sx) | ((sub_code_b(k) == 0u ? sm : sx) << 16);
    }
    else if (threadIdx.x < 16u)
    {
        // (the column frame's diagonal step rises by 2 G where the row frame's rises by G: the table carries the other G)
        const uint32_t tg = CELL::COLUMN ? uint32_t(-p.gap_ext * 32) : 0u;
        const uint32_t sm = uint32_t((p.match - p.gap_open) * 32) + tg, sx = uint32_t((p.mismatch - p.gap_open) * 32) + tg;
        uint32_t t = sx * 0x01010101u;
        if (threadIdx.x < 4u) t = (t & ~(0xFFu << (8u * threadIdx.x))) | (sm << (8u * threadIdx.x));
        s_tab[threadIdx.x] = t;
    }
    __syncthreads();
    const uint32_t lane = blockIdx.x * uint32_t(PAIR_LANES) + threadIdx.x;
    if (lane >= p.n / 2u + (p.n & 1u)) return;
    const uint32_t id[2] = { 2u * lane, 2u * lane + 1u < p.n ? 2u * lane + 1u : 2u * lane };
    const uint32_t M = (FORM & PF_KO_BOUND) ? 96u : p.pat.fixed_length;
    const Stream ps[2] = { p.pat.s, p.pat.s }, ts[2] = { p.txt.s, p.txt.s };
    const uint64_t pb[2] = { p.pat.begin[id[0]], p.pat.begin[id[1]] }, tb[2] = { p.txt.begin[id[0]], p.txt.begin[id[1]] };

    const int32_t d32 = (p.gap_ext - p.gap_open) * 32, g32 = -p.gap_ext * 32;
    uint32_t D = CELL::rep(d32), G = CELL::rep(g32);
    if (!CELL::COLUMN) { asm("" : "+v"(D)); asm("" : "+v"(G)); }                  // resident, like A16::pin (the column frame keeps its constants in scalars)
    uint32_t KT[2] = { 0u, 0u };
    if (FORM & PF_KO_TABLE) { KT[0] = s_tab[threadIdx.x & 3u]; KT[1] = s_tab[(threadIdx.x >> 2) & 3u]; asm("" : "+v"(KT[0])); asm("" : "+v"(KT[1])); }

    PairState<BAND> st;
    #pragma unroll
    for (int j = 0; j < BAND; ++j) st.S[j] = CELL::rep(g32 + CELL::FLOOR + (CELL::COLUMN ? g32 * j : 0));   // H = 0 in row -1: BIAS - D (+ G j in the column frame)
    #pragma unroll
    for (int j = 0; j < BAND - 1; ++j) st.F[j] = CELL::rep(CELL::FLOOR);
    st.z = CELL::rep(d32 + g32 + CELL::FLOOR);                                     // BIAS
    ColumnFrame<BAND> fr;
    if constexpr (CELL::COLUMN) CELL::open(fr, d32, g32);                          // (st.z is not used then)
    if constexpr ((FORM & PF_CONST2) != 0) asm("" : "+v"(fr.D));                   // PF_CONST2's D: a vector register, resident like the row frame's D and G
    st.best[0] = st.best[1] = 0u; st.besti[0] = st.besti[1] = 0u;
    uint32_t rk2 = 0u;                                                             // PF_FOLD2: the even row's row key
    {
        const uint32_t TA = fetch16_2bit(ts[0], tb[0]), TB = fetch16_2bit(ts[1], tb[1]);
        if constexpr (SUBLDS2)
        {
            // the pairs (t, t + 1) of the band's first fourteen symbols, t = 0 ... 12, and the last of them for the first block's first pair
            #pragma unroll
            for (int t = 0; t < 16; ++t)
                st.tc[t] = t < BAND - 2 ? sub2_col_byte((TA >> (2 * t)) & 3u, (TB >> (2 * t)) & 3u, (TA >> (2 * t + 2)) & 3u, (TB >> (2 * t + 2)) & 3u) << 3 : 0u;
        }
        else
        {
            #pragma unroll
            for (int j = 0; j < BAND - 1; ++j)
                st.tc[j] = SUBLDS ? (((TA >> (2 * j)) & 3u) | (((TB >> (2 * j)) & 3u) << 2)) << 2
                                  : CELL::SEL_BASE | ((TA >> (2 * j)) & 3u) | (((TB >> (2 * j)) & 3u) << 16);
        }
    }

    // this block's symbols and the cursors behind them (STREAM), or the generic fetches
    const uint32_t plast = stream_last_off(p.pat.s), tlast = stream_last_off(p.txt.s);
    GroupStream gp[2], gt[2];
    uint64_t PA, PB;
    uint32_t TA, TB;
    if (STREAM)
    {
        if (P4) { PA = stream_open_4bit<PBE>(ps[0], plast, pb[0], gp[0]); PB = stream_open_4bit<PBE>(ps[1], plast, pb[1], gp[1]); }
        else    { PA = expand_2to4(stream_open_2bit<PBE>(ps[0], plast, pb[0], gp[0])); PB = expand_2to4(stream_open_2bit<PBE>(ps[1], plast, pb[1], gp[1])); }
        TA = stream_open_2bit<TBE>(ts[0], tlast, tb[0] + BAND - 1, gt[0]); TB = stream_open_2bit<TBE>(ts[1], tlast, tb[1] + BAND - 1, gt[1]);
    }
    else
    {
        PA = fetch_pattern16(ps[0], pb[0]); PB = fetch_pattern16(ps[1], pb[1]);
        TA = fetch16_2bit(ts[0], tb[0] + BAND - 1); TB = fetch16_2bit(ts[1], tb[1] + BAND - 1);
    }
    for (uint32_t i0 = 0; i0 < M; i0 += 16u)
    {
        // the next block's symbols: loaded before this block's rows, put in order after them (STREAM), so that no wave sits waiting
        // for its words with the rows still to do; the generic fetches finish their groups here
        uint64_t PAn = 0, PBn = 0;
        uint32_t TAn = 0, TBn = 0;
        uint2 rp[2] = { make_uint2(0u, 0u), make_uint2(0u, 0u) };
        uint32_t rt[2] = { 0u, 0u };
        if (FORM & PF_KO_FETCH) {}
        else if (STREAM)
        {
            if (P4) { rp[0] = stream_load_4bit(ps[0], plast, gp[0]); rp[1] = stream_load_4bit(ps[1], plast, gp[1]); }
            else    { rp[0].x = stream_load_2bit(ps[0], plast, gp[0]); rp[1].x = stream_load_2bit(ps[1], plast, gp[1]); }
            rt[0] = stream_load_2bit(ts[0], tlast, gt[0]); rt[1] = stream_load_2bit(ts[1], tlast, gt[1]);
        }
        else
        {
            PAn = fetch_pattern16(ps[0], pb[0] + i0 + 16u); PBn = fetch_pattern16(ps[1], pb[1] + i0 + 16u);
            TAn = fetch16_2bit(ts[0], tb[0] + i0 + 16u + BAND - 1); TBn = fetch16_2bit(ts[1], tb[1] + i0 + 16u + BAND - 1);
        }
        if constexpr (SUBLDS2)
        {
            uint64_t RE, RO;
            sub2_row_words(PA, PB, RE, RO);
            uint32_t CW[4];
            // the symbols that entered a row before the block's first: the second of the last pair formed, (i0 + 12, i0 + 13), which slot
            // 12 of the ring holds (in the first block from the prologue): t0 ^ d, for job A in bits 3-4 and for job B in bits 7-8
            const uint32_t last = st.tc[12] ^ (st.tc[12] >> 2);
            sub2_col_words(TA, TB, (last >> 3) & 3u, (last >> 7) & 3u, CW);
            PairRows<CELL, BAND, FORM, 0, 16>::run(st, fr, i0, M, D, G, RE, RO, CW, reinterpret_cast<const uint32_t*>(s_sub2), KT, rk2);
        }
        else if constexpr (SUBLDS)
        {
            uint64_t RE, RO;
            sub_row_words(PA, PB, RE, RO);
            const uint32_t XT[2] = { sub_bfi(0x33333333u, TA, TB << 2), sub_bfi(0x33333333u, TA >> 2, TB) };   // the entering column words, nibble m: t_A | t_B << 2 of rows 2 m / 2 m + 1
            PairRows<CELL, BAND, FORM, 0, 16>::run(st, fr, i0, M, D, G, RE, RO, XT, s_sub, KT, rk2);
        }
        else
        {
            const uint32_t XT[2] = { (TA & 0xFFFFu) | (TB << 16), (TA >> 16) | (TB & 0xFFFF0000u) };
            PairRows<CELL, BAND, FORM, 0, 16>::run(st, fr, i0, M, D, G, PA, PB, XT, s_tab, KT, rk2);
        }
        if (FORM & PF_KO_FETCH)
        {
            PA = (PA << 4) | (PA >> 60); PB = (PB << 8) | (PB >> 56);
            TA = funnel(TA, TA, 2u); TB = funnel(TB, TB, 6u);
        }
        else if (STREAM)
        {
            if (P4) { PA = stream_group_4bit<PBE>(gp[0], rp[0]); PB = stream_group_4bit<PBE>(gp[1], rp[1]); }
            else    { PA = expand_2to4(stream_group_2bit<PBE>(gp[0], rp[0].x)); PB = expand_2to4(stream_group_2bit<PBE>(gp[1], rp[1].x)); }
            TA = stream_group_2bit<TBE>(gt[0], rt[0]); TB = stream_group_2bit<TBE>(gt[1], rt[1]);
        }
        else { PA = PAn; PB = PBn; TA = TAn; TB = TBn; }
    }

    if constexpr (FOLD2) { if (M & 1u) CELL::template fold_last<BAND, FORM>(st, rk2, M, d32, g32); }
    // (PF_SUBLDS2 works its job numbers out again from the lane's, one register across the block loop where the two 64-bit indices
    // are four: they are what would not fit five waves' 96)
    uint32_t lane_out = SUBLDS2 ? lane : 0u;
    if constexpr (SUBLDS2) asm volatile("" : "+v"(lane_out));
    const uint32_t id2[2] = { 2u * lane_out, 2u * lane_out + 1u < p.n ? 2u * lane_out + 1u : 2u * lane_out };
    const uint32_t (&od)[2] = SUBLDS2 ? id2 : id;
    #pragma unroll
    for (int h = 0; h < 2; ++h)
    {
        if (h == 1 && od[1] == od[0]) break;
        // the key sink's best is score << 20 | 31 << 15 | row << 5 | column; the pair fold's is score << 5 | odd row << 4 | column beside
        // the pair's even row
        const uint32_t j = st.best[h] & (FOLD2 ? 15u : 31u), i = KEY ? (st.best[h] >> 5) & 1023u : st.besti[h] + (FOLD2 ? (st.best[h] >> 4) & 1u : 0u);
        p.out_score[od[h]] = int32_t(st.best[h] >> (KEY ? 20 : 5));
        reinterpret_cast<uint2*>(p.out_sink)[od[h]] = make_uint2(i + j + 1u, i + 1u);
    }
}

template <int BAND, typename CELL, int FORM>
hipError_t launch_band_pair(const GotohParams& p, hipStream_t stream)
{
    const uint32_t n_lanes = p.n / 2u + (p.n & 1u);
    hipLaunchKernelGGL((banded_gotoh_pair_kernel<BAND, CELL, FORM>), dim3((n_lanes + PAIR_LANES - 1u) / PAIR_LANES), dim3(PAIR_LANES), 0, stream, p);
    return hipGetLastError();
}

// The library's instances (NVB_PAIR_INSTANCES) are compiled in banded_gotoh_pair_b15.hip, banded_gotoh_pair_b15_lit.hip, banded_gotoh_pair_b15_sub.hip and banded_gotoh_pair_b15_sub2.hip.  A translation unit that launches them and must not compile them again defines NVB_PAIR_EXTERN before
// it includes this header: banded_gotoh.hip does; the four instantiation files, and tools/pair_row_probe.hip with its own forms, do not
#ifdef NVB_PAIR_EXTERN
#define NVB_DECL(CELL, F) extern template hipError_t launch_band_pair<15, CELL, (F)>(const GotohParams&, hipStream_t);
NVB_PAIR_INSTANCES(NVB_DECL)
#undef NVB_DECL
#endif

} // namespace nvb
