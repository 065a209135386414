/*
 * nvbio_hip.h -- C-ABI of the MI355X (gfx950) seed-and-extend hot path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++ or torch types.
 * Every pointer is a DEVICE pointer into caller-owned HBM unless stated
 * otherwise; nothing is allocated, retained or freed by the library except
 * where a `temp` buffer is passed in explicitly.  All entry points enqueue work
 * on `stream` (a hipStream_t passed as void*; NULL = the null stream) and
 * return immediately with 0 or a hipError_t value; they never throw and never
 * fall back to the CPU.
 *
 * The reference (NVlabs/nvbio) has no ABI for this path -- it is C++ templates
 * (SURVEY.md 8b).  Each entry point below names the reference interface it
 * replaces; nvbio_amd/include/nvbio_hip/ *.h holds the C++ host layer that
 * mirrors those template names on top of this ABI.
 */
#ifndef NVBIO_HIP_H
#define NVBIO_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NVBIO_HIP_ABI_VERSION 2

/* nvbio::aln::AlignmentType (nvbio/alignment/alignment_base.h:54) */
enum { NVBIO_HIP_GLOBAL = 0, NVBIO_HIP_LOCAL = 1, NVBIO_HIP_SEMI_GLOBAL = 2 };

/* A set of strings stored in one packed word stream, i.e. what the reference
 * expresses as a string-set over nvbio::PackedStream<const uint32*,uint8,BITS,
 * BIG_ENDIAN> (nvbio/basic/packedstream.h, packedstream_inl.h:336-400):
 * string i = symbols [begin[i], begin[i]+length[i]) of the stream.
 *   words      the stream's uint32 words (device)
 *   n_words    number of words allocated; the kernels read whole 16-symbol
 *              groups and clamp every word load to [0,n_words), so a string may
 *              end anywhere in the stream without padding
 *   bits       2 or 4 (the production read / genome formats; 8-bit strings
 *              are packed by the host layer first)
 *   big_endian PackedStream's BIG_ENDIAN_T
 *   begin      n symbol offsets (uint64, device)
 *   length     n lengths (device), or NULL -> every string has `fixed_length` symbols */
typedef struct nvbio_hip_string_set {
    const uint32_t* words;
    uint64_t        n_words;
    uint32_t        bits;
    uint32_t        big_endian;
    const uint64_t* begin;
    const uint32_t* length;
    uint32_t        fixed_length;
    uint32_t        _pad;
} nvbio_hip_string_set;

/* nvbio::aln::SimpleGotohScheme (nvbio/alignment/utils.h:114-134) */
typedef struct nvbio_hip_gotoh_scheme {
    int32_t match, mismatch, gap_open, gap_ext;
} nvbio_hip_gotoh_scheme;

/* nvbio::aln::BestSink<int32> (nvbio/alignment/sink.h:68-89) is returned as
 * two arrays: score[n] and sink[2n] = {sink.x, sink.y}. */

/*
 * Replaces  BatchedBandedAlignmentScore<BAND_LEN, stream_type,
 *           DeviceThreadBlockScheduler<128,1>>::enact(stream)
 *           (nvbio/alignment/batched.h:333-353, batched_banded_inl.h:135-162) and
 *           batch_banded_alignment_score<BAND_LEN>(aligner, patterns, texts, sinks, ...)
 *           (nvbio/alignment/batched_inl.h:1074-1101)
 * for aligner = GotohAligner<TYPE, SimpleGotohScheme>, trivial qualities:
 * job i scores patterns[i] against texts[i] exactly as
 * priv::banded::gotoh_alignment_score_dispatch<BAND_LEN,TYPE>::run
 * (nvbio/alignment/gotoh/gotoh_banded_inl.h:415-658) into a fresh BestSink.
 * band_len in {3,5,7,15,31}.  A job whose text is shorter than its pattern
 * leaves the sink invalid (score = -(1<<30), sink = (0xFFFFFFFF,0xFFFFFFFF)).
 */
int nvbio_hip_banded_gotoh_score(
    const nvbio_hip_gotoh_scheme* scheme /* host */, int32_t type, uint32_t band_len,
    const nvbio_hip_string_set* patterns /* host struct, device arrays */,
    const nvbio_hip_string_set* texts    /* host struct, device arrays */,
    uint32_t max_pattern_len, uint32_t max_text_len /* the reference's max_pattern_length /
        max_text_length arguments (batched.h:217-231); 0 = unknown.  max_pattern_len only sizes
        the per-lane LDS staging of the strings (longer jobs read HBM directly): results never
        depend on either. */,
    uint32_t n, int32_t* out_score, uint32_t* out_sink, void* stream);

/*
 * Full-matrix (unbanded) Gotoh score.  Replaces
 *   BatchedAlignmentScore<stream, DeviceThreadScheduler>::enact (nvbio/alignment/batched.h:310-329,
 *   batched_inl.h:383-460) and batch_alignment_score(...) (batched.h:160-190)
 * for aligner = GotohAligner<TYPE, SimpleGotohScheme, TextBlockingTag> -- the instantiation of
 * sw-benchmark (sw-benchmark/sw-benchmark.cu:604-631): job i scores patterns[i] against the whole of
 * texts[i] exactly as priv::gotoh_alignment_score_dispatch<8,TYPE,TextBlockingTag,.>::run
 * (nvbio/alignment/gotoh/gotoh_inl.h:969-1489) does into a fresh BestSink, including its int16
 * boundary column, its tie order and its early exit against min_score[i] (NULL = never).
 * out_ok (nullable) receives that function's bool (0 = early-exited).  Patterns up to 1024 symbols
 * (max_pattern_len / max_text_len are required for ragged sets: they select the register layout). */
int nvbio_hip_gotoh_score(
    const nvbio_hip_gotoh_scheme* scheme /* host */, int32_t type,
    const nvbio_hip_string_set* patterns, const nvbio_hip_string_set* texts,
    uint32_t max_pattern_len, uint32_t max_text_len, const int32_t* min_score /* device, nullable */,
    uint32_t n, int32_t* out_score, uint32_t* out_sink, uint8_t* out_ok, void* stream);

/* nvbio::aln::SimpleSmithWatermanScheme (nvbio/alignment/utils.h:92-109): linear gap costs.
 * EditDistanceAligner is this scheme with {0,-1,-1,-1} (ed/ed_utils.h:44-51). */
typedef struct nvbio_hip_sw_scheme { int32_t match, mismatch, deletion, insertion; } nvbio_hip_sw_scheme;

/* As nvbio_hip_banded_gotoh_score / nvbio_hip_gotoh_score, for
 *   aligner = SmithWatermanAligner<TYPE, SimpleSmithWatermanScheme>  (sw/sw_banded_inl.h:340-520; sw/sw_inl.h:881-1222,
 *             TextBlockingTag, 16-column blocks, int16 boundary column, no early exit)
 *   aligner = EditDistanceAligner<TYPE>                              (ed/ed_banded_inl.h, ed/ed_inl.h:85-99: the same
 *             code with EditDistanceSWScheme) -- the second leg of sw-benchmark (sw-benchmark.cu:641-657).
 * Schemes with deletion != insertion are refused (801); the full-matrix form also refuses schemes/lengths whose
 * values could leave int16 ((M [+ N for GLOBAL] + 4) * max|cost| >= 30000). */
int nvbio_hip_banded_sw_score(
    const nvbio_hip_sw_scheme* scheme /* host */, int32_t type, uint32_t band_len,
    const nvbio_hip_string_set* patterns, const nvbio_hip_string_set* texts,
    uint32_t max_pattern_len, uint32_t max_text_len,
    uint32_t n, int32_t* out_score, uint32_t* out_sink, void* stream);
int nvbio_hip_sw_score(
    const nvbio_hip_sw_scheme* scheme /* host */, int32_t type,
    const nvbio_hip_string_set* patterns, const nvbio_hip_string_set* texts,
    uint32_t max_pattern_len, uint32_t max_text_len,
    uint32_t n, int32_t* out_score, uint32_t* out_sink, void* stream);

/* The general full-matrix score: aligner kind x algorithm tag (alignment_base.h:72-79), i.e.
 *   BatchedAlignmentScore<stream,...>::enact for GotohAligner / SmithWatermanAligner / EditDistanceAligner with
 *   PatternBlockingTag (the default of make_*_aligner<TYPE>(...); gotoh_inl.h:459-900, sw_inl.h:417-760) or TextBlockingTag.
 * scheme4 = {match, mismatch, gap_open, gap_ext} (Gotoh) or {match, mismatch, deletion, insertion} (SW; ED = {0,-1,-1,-1}).
 * The two tags compute the same matrix; they differ in the visiting order (which of several equal LOCAL maxima the sink
 * keeps), and in the early exit against min_score[i]: per block of 8 (16) pattern symbols for PatternBlockingTag
 * (max_i H[i][block end] + (M - block end) * match < min_score), per block of text columns for TextBlockingTag.
 * PatternBlockingTag runs on the 16-bit sweep only (values within int16, else 801) and needs patterns of >= 1 symbol. */
enum { NVBIO_HIP_GOTOH_ALIGNER = 0, NVBIO_HIP_SW_ALIGNER = 1 };
enum { NVBIO_HIP_PATTERN_BLOCKING = 0, NVBIO_HIP_TEXT_BLOCKING = 1 };
int nvbio_hip_alignment_score(
    int32_t aligner, int32_t algorithm, const int32_t* scheme4 /* host */, int32_t type,
    const nvbio_hip_string_set* patterns, const nvbio_hip_string_set* texts,
    uint32_t max_pattern_len, uint32_t max_text_len, const int32_t* min_score /* device, nullable */,
    uint32_t n, int32_t* out_score, uint32_t* out_sink, uint8_t* out_ok /* nullable */, void* stream);

/* nvBowtie's SmithWatermanScoringScheme<QualCost,ConstantCost> as the Gotoh aligner sees it
 * (nvBowtie/bowtie2/cuda/scoring.h:283-293): substitution(r,q,qq) = (r == q) ? match : mismatch[qq],
 * with mismatch[qq] = -m_mmp(qq) tabulated by the host for every quality byte (the float->int
 * truncation of QualCost, scoring.h:86-104, stays on the host), and the four gap accessors. */
typedef struct nvbio_hip_gotoh_qual_scheme {
    int32_t match;
    int32_t pattern_gap_open, pattern_gap_ext, text_gap_open, text_gap_ext;   /* as returned by the accessors (<= 0) */
    int32_t mismatch[256];
} nvbio_hip_gotoh_qual_scheme;

/* As nvbio_hip_banded_gotoh_score, for GotohAligner<TYPE, SmithWatermanScoringScheme<...>> with a
 * quality string per pattern: replaces the instantiation in nvBowtie's extension stage
 * (nvBowtie/bowtie2/cuda/score_best_inl.h:153-201).  quals[b + i] is the quality of symbol i of the
 * pattern that begins at stream index b (nvBowtie stores read qualities at the reads' own offsets);
 * n_quals = bytes allocated. */
int nvbio_hip_banded_gotoh_score_qual(
    const nvbio_hip_gotoh_qual_scheme* scheme /* host */, int32_t type, uint32_t band_len,
    const nvbio_hip_string_set* patterns, const uint8_t* quals, uint64_t n_quals,
    const nvbio_hip_string_set* texts,
    uint32_t max_pattern_len, uint32_t max_text_len,
    uint32_t n, int32_t* out_score, uint32_t* out_sink, void* stream);

/* The same with a per-job VIEW of each pattern, so that nvBowtie's unedited streams run in place.  nvBowtie never materialises
 * the string it aligns: AlignmentStrings::load (nvBowtie/bowtie2/cuda/alignment_utils.h:170-218) hands the DP an
 * nvbio::io::ReadStream (nvbio/io/utils.h:100-330) over the stored read -- reads are stored reversed, (REVERSE, STANDARD) shows
 * the forward strand and (FORWARD, COMPLEMENT) the reverse complement -- and the reference's per-thread DP reads it symbol by
 * symbol through operator[].  pattern_flags[i] (device, one byte per job, NULL = no views) describes job i's view of the stored
 * symbols [begin[i], begin[i] + length[i]):  bit 0 = walk them backwards (pattern symbol k is stored symbol begin + length - 1 - k,
 * and its quality is quals[begin + length - 1 - k]),  bit 1 = complement the bases (c < 4 -> 3 - c; N stays).  The kernels turn
 * each 16-symbol group round in registers as they fetch it; results are those of the materialised string, bit for bit. */
int nvbio_hip_banded_gotoh_score_qual_views(
    const nvbio_hip_gotoh_qual_scheme* scheme /* host */, int32_t type, uint32_t band_len,
    const nvbio_hip_string_set* patterns, const uint8_t* quals, uint64_t n_quals, const uint8_t* pattern_flags /* device, nullable */,
    const nvbio_hip_string_set* texts,
    uint32_t max_pattern_len, uint32_t max_text_len,
    uint32_t n, int32_t* out_score, uint32_t* out_sink, void* stream);

/* The same scorer with ONE WAVE PER JOB (nvbio_amd/csrc/banded_gotoh_wave.hip): lane j of a wave owns band cell j and the wave sweeps the
 * anti-diagonals 2 i + j = w -- 2 M + BAND steps instead of M * BAND cells in sequence.  For batches too small to fill the chip (a few
 * thousand jobs: nvBowtie's extension rounds after the first), where the lane-per-job kernel takes as long as one job's cells in sequence
 * whatever the batch size.  Same results bit for bit.  Job k (k < n, or < *n_on_device when given) is job_index[k] of the string sets
 * (job_index == NULL: k itself) and writes out_score / out_sink at that index -- a list of live jobs run in place -- or, with out_index, at
 * out_index[that index].  gate (device, optional): the launch does nothing unless *gate <= gate_limit -- the lane-per-job entry below takes the same
 * pair and runs when *gate > gate_limit, so a driver queues both and the device picks the form that suits the batch, with no host round trip.
 * Patterns up to 512 symbols (hipErrorNotSupported beyond; max_pattern_len announces the longest of a ragged set); no pattern views. */
int nvbio_hip_banded_gotoh_score_qual_wave(
    const nvbio_hip_gotoh_qual_scheme* scheme, int32_t type, uint32_t band_len,
    const nvbio_hip_string_set* patterns, const uint8_t* quals /* nullable: mismatch[0] throughout */, uint64_t n_quals,
    const nvbio_hip_string_set* texts, uint32_t max_pattern_len,
    uint32_t n, const uint32_t* n_on_device /* nullable */, const uint32_t* job_index /* nullable */, const uint32_t* out_index /* nullable */,
    const uint32_t* gate /* nullable */, uint32_t gate_limit,
    int32_t* out_score, uint32_t* out_sink, void* stream);

/* The same scorer with a threshold per job -- the reference's `min_score` argument of banded_alignment_score (alignment_inl.h; its windowed
 * form gives up on a job once max(H) < min_score + remaining_rows * match, gotoh_banded_inl.h:622-634), which nvBowtie's scoring stage sets to
 * the read's second-best score (score_best_inl.h:113-116) and whose reduction only asks whether a score is ABOVE that (reduce_inl.h:111-135).
 *   job i ends above min_score[i]:   out_score / out_sink are what nvbio_hip_banded_gotoh_score_qual_views reports, bit for bit;
 *   job i ends at or below it:       out_score[i] is SOME value <= min_score[i] (an upper bound of the true score), out_sink[i] = (-1, -1).
 * min_score == NULL or min_score[i] == INT32_MIN: exact.  Persistent waves pull jobs from *work_counter (device, 4 bytes, zeroed by the call):
 * a lane whose job is given up or done takes the next (nvbio_amd/csrc/banded_gotoh_bounded.h).  n_on_device (optional, device): the number
 * of jobs, read by the kernel -- `n` is then only an upper bound (array capacity), and the host need not know the count.  out_index (optional,
 * device): job i's results are written at out_score[out_index[i]] / out_sink[out_index[i]] -- a compacted batch of jobs (nvbio_hip_score_best_setup's
 * job_hit) writing straight back at its hits.  gate / gate_limit (min_score == NULL only): the launch does nothing unless *gate > gate_limit (see
 * nvbio_hip_banded_gotoh_score_qual_wave). */
int nvbio_hip_banded_gotoh_score_qual_bounded(
    const nvbio_hip_gotoh_qual_scheme* scheme, int32_t type, uint32_t band_len,
    const nvbio_hip_string_set* patterns, const uint8_t* quals, uint64_t n_quals, const uint8_t* pattern_flags,
    const nvbio_hip_string_set* texts,
    uint32_t max_pattern_len, uint32_t max_text_len,
    uint32_t n, const uint32_t* n_on_device, const int32_t* min_score, uint32_t* work_counter, const uint32_t* out_index,
    const uint32_t* gate /* nullable; with min_score == NULL only */, uint32_t gate_limit,
    int32_t* out_score, uint32_t* out_sink, void* stream);

/* Batched banded Gotoh traceback.  Replaces
 *   BatchedBandedAlignmentTraceback<BAND_LEN, CHECKPOINTS, stream, DeviceThreadScheduler>::enact
 *   (nvbio/alignment/batched.h:460-476, batched_banded_inl.h:250-420)
 * for aligner = GotohAligner<TYPE, scheme> and the CIGAR-forming backtracer nvBowtie passes
 * (Backtracker<io::Cigar*>, nvBowtie/bowtie2/cuda/alignment_utils.h:125-168), the instantiation of
 * nvBowtie's traceback stage (traceback_inl.h:205-262).  Job i re-scores patterns[i] in the band of
 * texts[i] (banded_alignment_traceback, nvbio/alignment/banded_inl.h:352-423) and walks the flow flags
 * back (gotoh_banded_inl.h:878-960):
 *   out_score[i], out_sink[2i..]     Alignment::score / ::sink   (== nvbio_hip_banded_gotoh_score's)
 *   out_source[2i..]                 Alignment::source           ((-1,-1) when there is no valid sink)
 *   out_cigar[i*cigar_stride + k]    io::Cigar as a uint16: type | len << 2 (nvbio/io/alignments.h:57-75;
 *                                    0 = M, 1 = I, 2 = D, 3 = soft clip), in the backtracer's order, i.e.
 *                                    the END of the alignment first, exactly what context->cigar holds
 *   out_cigar_len[i]                 backtracer.size; entries beyond cigar_stride are counted, not written
 * CHECKPOINTS has no equivalent: the flow flags of the whole band are kept in `temp`
 * (nvbio_hip_banded_gotoh_traceback_temp_bytes), which reproduces the reference for every interval
 * as long as the DP values fit its int16 checkpoints; schemes/lengths with
 * (max_pattern_len + band_len + 2) * max|cost| >= 32000 are refused with 801.
 * max_pattern_len is required for ragged pattern sets.
 * Strings (all three entries, and nvbio_hip_banded_sw_traceback): patterns of 2, 4 or 8 bits, texts of 2 bits (else 801).  Of an 8-bit
 * pattern's byte only which text symbol it equals matters: 0..3 are those symbols, 255 equals a text position past the end (the value the
 * reference compares it as) and nothing else, every other byte equals nothing.  Quality bytes stay one per pattern symbol at the
 * patterns' own offsets. */
uint64_t nvbio_hip_banded_gotoh_traceback_temp_bytes(uint32_t band_len, uint32_t max_pattern_len, uint32_t n);
int nvbio_hip_banded_gotoh_traceback(
    const nvbio_hip_gotoh_scheme* scheme /* host */, int32_t type, uint32_t band_len,
    const nvbio_hip_string_set* patterns, const nvbio_hip_string_set* texts,
    uint32_t max_pattern_len, uint32_t max_text_len, uint32_t n,
    int32_t* out_score, uint32_t* out_sink, uint32_t* out_source,
    uint16_t* out_cigar, uint32_t cigar_stride, uint32_t* out_cigar_len,
    void* temp, uint64_t temp_bytes, void* stream);
int nvbio_hip_banded_gotoh_traceback_qual(
    const nvbio_hip_gotoh_qual_scheme* scheme /* host */, int32_t type, uint32_t band_len,
    const nvbio_hip_string_set* patterns, const uint8_t* quals, uint64_t n_quals,
    const nvbio_hip_string_set* texts,
    uint32_t max_pattern_len, uint32_t max_text_len, uint32_t n,
    int32_t* out_score, uint32_t* out_sink, uint32_t* out_source,
    uint16_t* out_cigar, uint32_t cigar_stride, uint32_t* out_cigar_len,
    void* temp, uint64_t temp_bytes, void* stream);
/* the same, with score[] / sink[] filled by the caller with what nvbio_hip_banded_gotoh_score_qual reports for these jobs (skips the score pass) */
int nvbio_hip_banded_gotoh_traceback_qual_known(
    const nvbio_hip_gotoh_qual_scheme* scheme /* host */, int32_t type, uint32_t band_len,
    const nvbio_hip_string_set* patterns, const uint8_t* quals, uint64_t n_quals,
    const nvbio_hip_string_set* texts,
    uint32_t max_pattern_len, uint32_t max_text_len, uint32_t n,
    int32_t* score /* in/out */, uint32_t* sink /* in/out */, uint32_t* out_source,
    uint16_t* out_cigar, uint32_t cigar_stride, uint32_t* out_cigar_len,
    void* temp, uint64_t temp_bytes, void* stream);

/* Batched full-matrix Gotoh traceback.  Replaces
 *   BatchedAlignmentTraceback<CHECKPOINTS, stream, DeviceThreadScheduler>::enact (nvbio/alignment/batched.h:432-452)
 * for aligner = GotohAligner<TYPE, SimpleGotohScheme> with nvBowtie's CIGAR-forming backtracer: alignment_traceback
 * (alignment_inl.h:365-480) -- the sink of the pattern-blocking score pass, the flow flags of gotoh_inl.h:512-560 /
 * :407-425, the walk of gotoh_inl.h:1806-1870 and the driver's completion along the first row / column (:443-466).
 * Outputs as nvbio_hip_banded_gotoh_traceback (source/sink: x = text position, y = pattern position).
 * The flow flags of the whole matrix live in `temp` (nvbio_hip_gotoh_traceback_temp_bytes: 4 bytes per 8 cells + 4 bytes
 * per text symbol, per job); CHECKPOINTS has no equivalent.  Requires the int16-exact range of the full-matrix scorer.
 * Strings (this entry, the _qual and _known_score forms and nvbio_hip_sw_traceback): patterns of 2, 4 or 8 bits -- a byte other than
 * 0..3 equals no text symbol --, texts of 2 bits (else 801). */
uint64_t nvbio_hip_gotoh_traceback_temp_bytes(uint32_t max_pattern_len, uint32_t max_text_len, uint32_t n);
int nvbio_hip_gotoh_traceback(
    const nvbio_hip_gotoh_scheme* scheme /* host */, int32_t type,
    const nvbio_hip_string_set* patterns, const nvbio_hip_string_set* texts,
    uint32_t max_pattern_len, uint32_t max_text_len, uint32_t n,
    int32_t* out_score, uint32_t* out_sink, uint32_t* out_source,
    uint16_t* out_cigar, uint32_t cigar_stride, uint32_t* out_cigar_len,
    void* temp, uint64_t temp_bytes, void* stream);

/* nvbio_hip_gotoh_traceback with nvBowtie's quality-aware scheme (its opposite-mate traceback, traceback_inl.h): mismatch
 * penalties from the quality bytes, pattern gap costs in the recurrences, text gap costs on the column before the pattern. */
int nvbio_hip_gotoh_traceback_qual(
    const nvbio_hip_gotoh_qual_scheme* scheme /* host */, int32_t type,
    const nvbio_hip_string_set* patterns, const uint8_t* quals, uint64_t n_quals, const nvbio_hip_string_set* texts,
    uint32_t max_pattern_len, uint32_t max_text_len, uint32_t n,
    int32_t* out_score, uint32_t* out_sink, uint32_t* out_source,
    uint16_t* out_cigar, uint32_t cigar_stride, uint32_t* out_cigar_len,
    void* temp, uint64_t temp_bytes, void* stream);

/* The two full-matrix tracebacks for callers that know, per job, the score of the best alignment over the job's text AND that it ends
 * at the text's last symbol -- nvBowtie's opposite-mate tracebacks, whose windows are [alignment, alignment + sink) of a scoring pass
 * (traceback_inl.h:833-905).  The text rows no alignment of that score can reach (all but the last M + gaps-the-score-allows) are
 * dropped before any DP runs; score, sink, source and CIGAR are those of the plain forms (argument: full_traceback.hip,
 * crop_windows_kernel).  known_score: device int32[n].  The premise is checked per job on what the cropped DP found (score ==
 * known_score and the sink on the window's last row); a job that fails the check -- a known_score that is too high cuts the window too
 * short -- is traced again over its whole window, so its outputs are those of the plain form (one 4-byte read-back per call finds the
 * count; nvbio_hip_known_score_redone() totals it).  Under a TRUE premise the result is the plain form's in every case, ties included: a
 * tied cell the cropped DP visits first lies off the last row, fails the check, and the job is traced again.  Not detectable under a
 * FALSE premise: a window whose plain-order best alignment (of score known_score, or better in the dropped rows) is not the one the kept
 * rows hold with exactly known_score ending at the last row -- the caller then gets that other alignment.  GLOBAL: same as the plain forms.
 * Unlike the plain forms, these two BLOCK the host: the per-job check is read back (one device-to-host copy and a synchronisation of
 * `stream`), and a batch with failed checks allocates and frees a redo buffer before returning. */
int nvbio_hip_gotoh_traceback_known_score(
    const nvbio_hip_gotoh_scheme* scheme /* host */, int32_t type,
    const nvbio_hip_string_set* patterns, const nvbio_hip_string_set* texts, const int32_t* known_score,
    uint32_t max_pattern_len, uint32_t max_text_len, uint32_t n,
    int32_t* out_score, uint32_t* out_sink, uint32_t* out_source,
    uint16_t* out_cigar, uint32_t cigar_stride, uint32_t* out_cigar_len,
    void* temp, uint64_t temp_bytes, void* stream);
int nvbio_hip_gotoh_traceback_qual_known_score(
    const nvbio_hip_gotoh_qual_scheme* scheme /* host */, int32_t type,
    const nvbio_hip_string_set* patterns, const uint8_t* quals, uint64_t n_quals, const nvbio_hip_string_set* texts, const int32_t* known_score,
    uint32_t max_pattern_len, uint32_t max_text_len, uint32_t n,
    int32_t* out_score, uint32_t* out_sink, uint32_t* out_source,
    uint16_t* out_cigar, uint32_t cigar_stride, uint32_t* out_cigar_len,
    void* temp, uint64_t temp_bytes, void* stream);

uint64_t nvbio_hip_known_score_redone(void);     /* jobs the two forms above traced again since the library was loaded */

/* The tracebacks for SmithWatermanAligner / EditDistanceAligner, banded (sw_banded_inl.h:405-470, 748-800) and full matrix
 * (sw_inl.h:389-396, 475-500, 1660-1700): arguments, strings and temp sizes as the Gotoh forms.  deletion and insertion may differ, with
 * the reference's convention for each matrix: in the band `deletion` is paid for the move from the previous pattern row (and on GLOBAL's
 * row zero, j * deletion) and `insertion` along the row; in the full matrix `deletion` is paid along the text (the column before the
 * pattern is deletion * (i + 1) for GLOBAL) and `insertion` down the pattern (the row before the text is insertion * j for non-LOCAL).
 * The int16-range refusals (801) take the largest |cost| over all four.  The banded reference context does not mark zero cells, so its
 * LOCAL walk always reaches the first pattern row; reproduced. */
int nvbio_hip_banded_sw_traceback(
    const nvbio_hip_sw_scheme* scheme /* host */, int32_t type, uint32_t band_len,
    const nvbio_hip_string_set* patterns, const nvbio_hip_string_set* texts,
    uint32_t max_pattern_len, uint32_t max_text_len, uint32_t n,
    int32_t* out_score, uint32_t* out_sink, uint32_t* out_source,
    uint16_t* out_cigar, uint32_t cigar_stride, uint32_t* out_cigar_len,
    void* temp, uint64_t temp_bytes, void* stream);
int nvbio_hip_sw_traceback(
    const nvbio_hip_sw_scheme* scheme /* host */, int32_t type,
    const nvbio_hip_string_set* patterns, const nvbio_hip_string_set* texts,
    uint32_t max_pattern_len, uint32_t max_text_len, uint32_t n,
    int32_t* out_score, uint32_t* out_sink, uint32_t* out_source,
    uint16_t* out_cigar, uint32_t cigar_stride, uint32_t* out_cigar_len,
    void* temp, uint64_t temp_bytes, void* stream);

/* nvbio_hip_alignment_score for GotohAligner<TYPE, SmithWatermanScoringScheme<...>, algorithm_tag>: nvBowtie's full-matrix
 * scoring of the opposite mate (score_opposite_inl.h:266-269).  Mismatch penalties come from the quality bytes (as in
 * nvbio_hip_banded_gotoh_score_qual); the recurrences use the pattern gap costs, and one boundary line of the matrix is
 * initialised with the text gap costs -- which one depends on the tag, exactly as gotoh_inl.h:82-88 / :693-697 / :1171-1175
 * have it.  16-bit sweep only (801 otherwise). */
int nvbio_hip_alignment_score_qual(
    const nvbio_hip_gotoh_qual_scheme* scheme /* host */, int32_t algorithm, int32_t type,
    const nvbio_hip_string_set* patterns, const uint8_t* quals, uint64_t n_quals, const nvbio_hip_string_set* texts,
    uint32_t max_pattern_len, uint32_t max_text_len, const int32_t* min_score /* device, nullable */,
    uint32_t n, int32_t* out_score, uint32_t* out_sink, uint8_t* out_ok /* nullable */, void* stream);

/* ... with job control, for batches whose size only the device knows.  wave_form = 0: the same dispatch, run only when *gate > gate_limit
 * (gate == NULL: always).  wave_form = 1: ONE job per wave (64 lanes x ceil(M / 64) rows: the shortest sweep a job can have) over a list --
 * entry k < *n_on_device is job job_index[k] of the arrays and writes its outputs there -- run only when *gate <= gate_limit.  A driver queues
 * both with the same gate (the count of live jobs): many jobs take the throughput kernels, a few take the low-latency form, and the host never
 * waits for the count.  16-bit sweep only (801 otherwise). */
int nvbio_hip_alignment_score_qual_jobs(
    const nvbio_hip_gotoh_qual_scheme* scheme /* host */, int32_t algorithm, int32_t type,
    const nvbio_hip_string_set* patterns, const uint8_t* quals, uint64_t n_quals, const nvbio_hip_string_set* texts,
    uint32_t max_pattern_len, uint32_t max_text_len, const int32_t* min_score /* device, nullable */,
    uint32_t n, const uint32_t* n_on_device, const uint32_t* job_index, const uint32_t* gate, uint32_t gate_limit, int32_t wave_form,
    int32_t* out_score, uint32_t* out_sink, uint8_t* out_ok /* nullable */, void* stream);

/* Ungapped ("Hamming") scoring: BatchedAlignmentScore<stream,...>::enact for HammingDistanceAligner<TYPE, scheme, PatternBlockingTag>
 * (hamming/hamming_inl.h:413-720) -- the aligner nvBowtie scores the opposite mate with under --ungapped-mates (score_paired.cu:110-137).
 *   H(i,j) = H(i-1,j-1) + (text[i] == pattern[j] ? match : mismatch[q_j]),   clamped at 0 after every cell for LOCAL,
 * and EVERY border is zero, for all three types: the sum runs along the diagonal back to the top row or the left column, whichever
 * comes first, so a pattern may hang over the text's start and the part before it is free.  A pattern symbol that equals no text
 * symbol (codes >= 4) mismatches.  Reports go to a fresh BestSink (of equal scores the one reported last stays):
 *   LOCAL        every cell, by 16-column pattern block, then text row i, then column j inside the block; sink (i+1, j)
 *   SEMI_GLOBAL  H(i, M) for i = 0..N-1; sink (i+1, M)
 *   GLOBAL       H(N-1, M) alone, sink (N, M); an empty text reports the zero border.
 * Early exit: after every 16-column block except the last the job stops with out_ok = 0 when
 *   max_i H(i, block end) + (M - block end) * match < min_score[job]            (min_score == NULL: -(1<<30) for every job, which
 *                                                                                only an empty text's edge, INT32_MIN, falls below)
 * and its sink keeps what it had seen (nothing, for SEMI_GLOBAL and GLOBAL: score = -(1<<30), sink = (0xFFFFFFFF,0xFFFFFFFF)).
 * This test is NOT a bound: diagonals that enter a later block from the top border start at 0 there, so jobs whose final best does
 * meet min_score are declined too (M = 17, N = 1).  It is reproduced as it is -- nvBowtie's records depend on it.  Values are kept in
 * 32 bits; between blocks they pass through the reference's int16 column, which is modelled (the low 16 bits, sign-extended).
 * Every job writes its three outputs.  Limits (801 beyond them): texts 2-bit, patterns 2-, 4- or 8-bit; algorithm =
 * NVBIO_HIP_PATTERN_BLOCKING only; max_pattern_len <= 4096; |match|, |mismatch| <= 2^20; max_text_len as far as one job's working
 * set (2.25 bytes per text symbol + 4.5 per pattern symbol + 1 KB) fits the 160 KB of LDS a workgroup may have (65535 with
 * 1024-symbol patterns does: 152 KB).  The simple scheme reads `match` and `mismatch` only. */
int nvbio_hip_hamming_score(
    const nvbio_hip_sw_scheme* scheme /* host */, int32_t algorithm, int32_t type,
    const nvbio_hip_string_set* patterns, const nvbio_hip_string_set* texts,
    uint32_t max_pattern_len, uint32_t max_text_len, const int32_t* min_score /* device, nullable */,
    uint32_t n, int32_t* out_score, uint32_t* out_sink, uint8_t* out_ok /* nullable */, void* stream);
/* ... with nvBowtie's quality scheme: mismatch[quals[b + j]] for symbol j of the pattern that begins at stream index b (as in
 * nvbio_hip_banded_gotoh_score_qual); the gap fields are not read */
int nvbio_hip_hamming_score_qual(
    const nvbio_hip_gotoh_qual_scheme* scheme /* host */, int32_t algorithm, int32_t type,
    const nvbio_hip_string_set* patterns, const uint8_t* quals, uint64_t n_quals, const nvbio_hip_string_set* texts,
    uint32_t max_pattern_len, uint32_t max_text_len, const int32_t* min_score /* device, nullable */,
    uint32_t n, int32_t* out_score, uint32_t* out_sink, uint8_t* out_ok /* nullable */, void* stream);
/* ... with the job control of nvbio_hip_alignment_score_qual_jobs (the kernel is the same one wave per job in both forms):
 * wave_form = 0 runs jobs [0, n) when *gate > gate_limit (gate == NULL: always); wave_form = 1 runs entries [0, *n_on_device) of
 * job_index, each in place, when *gate <= gate_limit.  n bounds the launch; the host never reads a device-side count. */
int nvbio_hip_hamming_score_qual_jobs(
    const nvbio_hip_gotoh_qual_scheme* scheme /* host */, int32_t algorithm, int32_t type,
    const nvbio_hip_string_set* patterns, const uint8_t* quals, uint64_t n_quals, const nvbio_hip_string_set* texts,
    uint32_t max_pattern_len, uint32_t max_text_len, const int32_t* min_score /* device, nullable */,
    uint32_t n, const uint32_t* n_on_device, const uint32_t* job_index, const uint32_t* gate, uint32_t gate_limit, int32_t wave_form,
    int32_t* out_score, uint32_t* out_sink, uint8_t* out_ok /* nullable */, void* stream);

/* nvbio::fm_index<rank_dictionary<2,64,PackedStream<.,uint8,2,true>,.,.>, SSA_index_multiple_context<SA_INT>, const uint32*>
 * (nvbio/fmindex/fmindex.h:341-387) in the production interleaved layout
 * (nvbio/io/fmindex/fmindex.h:159-174, fmindex_impl.cu:305-327):
 *   bwt_occ  8 x uint32 per 64 BWT symbols: 4 words of big-endian 2-bit BWT,
 *            then #A,#C,#G,#T before the block
 *   ssa      ssa[k] = SA[k*sa_int], ssa[0] = 0xFFFFFFFF (nvbio/fmindex/ssa_inl.h:263-309)
 * This struct lives on the host; bwt_occ / ssa point to device memory. */
typedef struct nvbio_hip_fmindex {
    uint32_t        length;
    uint32_t        primary;
    uint32_t        L2[5];
    uint32_t        sa_int;     /* any power of two; 16 in the reference's files.  With 288 GB of HBM
                                   a denser SSA (down to 1 = the full SA) is affordable and shortens
                                   locate's LF walk from ~sa_int steps to none; results are identical */
    const uint32_t* bwt_occ;
    const uint32_t* ssa;
    const uint32_t* ktab;       /* optional accelerator, NULL = none: the match range (uint2) of every
                                   k-mer, built by nvbio_hip_fm_build_ktab; match() then resolves a
                                   seed's last ktab_k symbols with one lookup instead of ktab_k
                                   backward-search steps -- same ranges, bit for bit */
    uint32_t        ktab_k;
    uint32_t        _pad;
    const uint32_t* dimer;      /* optional, NULL = none: the MI355X line-native index built by
                                   nvbio_hip_fm_build_dimer_index (128-byte records holding a two-symbol BWT).
                                   When attached, match / the seed mappers / locate consume two symbols
                                   (two text positions) per 128-byte HBM line instead of one -- same SA ranges,
                                   iterators and positions, bit for bit.  Set by nvbio_hip_fm_attach_dimer_index,
                                   which also fills the constants below from the buffer's header */
    uint32_t        dimer_p1, dimer_fill1;
    uint32_t        dimer_S[4], dimer_T[4];
    const uint32_t* trimer;     /* optional, NULL = none; needs `dimer`: the three-symbol rank arrays built by
                                   nvbio_hip_fm_build_trimer_index (10.7 B per SA row).  Backward search then consumes three
                                   symbols per step -- same ranges, bit for bit */
} nvbio_hip_fmindex;

/* Replaces nvbio::rank(fmi, k, c) (nvbio/fmindex/fmindex_inl.h:36-57) over n
 * independent point queries: out[i] = rank(fmi, k[i], c[i]). */
int nvbio_hip_fm_rank(const nvbio_hip_fmindex* fmi, const uint32_t* k, const uint8_t* c,
                      uint32_t n, uint32_t* out, void* stream);

/* Replaces nvbio::rank4(fmi, k) (fmindex_inl.h:111-135): out[4i..4i+3]. */
int nvbio_hip_fm_rank4(const nvbio_hip_fmindex* fmi, const uint32_t* k,
                       uint32_t n, uint32_t* out, void* stream);

/* Replaces nvbio::rank(fmi, range, c) (fmindex_inl.h:66-99): range/out are uint2 arrays. */
int nvbio_hip_fm_rank_range(const nvbio_hip_fmindex* fmi, const uint32_t* range, const uint8_t* c,
                            uint32_t n, uint32_t* out, void* stream);

/* Replaces nvbio::match(fmi, pattern, len) (fmindex_inl.h:280-341) and
 * nvBowtie's match_range (nvBowtie/bowtie2/cuda/mapping_inl.h:83-97) over a
 * string-set: out_range[2i..2i+1] = inclusive SA range of seeds[i], (1,0) if
 * the seed holds a symbol > 3. */
int nvbio_hip_fm_match(const nvbio_hip_fmindex* fmi, const nvbio_hip_string_set* seeds,
                       uint32_t n, uint32_t* out_range, void* stream);

/* The line-native two-symbol index (layout: nvbio_amd/csrc/fmindex_dimer.h).  The reference's index spends one
 * 32-byte record per symbol and range end (nvbio/io/fmindex/fmindex_impl.cu:305-322), which on MI355X is one
 * 128-byte fabric request each; this one answers a backward-search step for TWO pattern symbols, or two LF steps
 * of locate, from one 128-byte record.  Built on the device from `fmi` (its bwt_occ; dimer/ktab fields ignored):
 *   out_dimer  nvbio_hip_fm_dimer_index_bytes(length) bytes, 128-byte aligned  (128 B header + 1 B per SA row)
 *   temp       nvbio_hip_fm_build_dimer_index_temp_bytes(length) bytes
 * nvbio_hip_fm_attach_dimer_index copies the header's constants into *fmi and sets fmi->dimer (synchronises
 * `stream` once; pass dimer = NULL to detach); it fails with hipErrorInvalidValue if the buffer was built
 * from a different index. */
uint64_t nvbio_hip_fm_dimer_index_bytes(uint32_t length);
uint64_t nvbio_hip_fm_build_dimer_index_temp_bytes(uint32_t length);
int nvbio_hip_fm_build_dimer_index(const nvbio_hip_fmindex* fmi, uint32_t* out_dimer, void* temp, uint64_t temp_bytes, void* stream);
int nvbio_hip_fm_attach_dimer_index(nvbio_hip_fmindex* fmi, const uint32_t* dimer, void* stream);

/* The three-symbol rank arrays on top of the two-symbol index: for each of the 64 trimers "abc" an array of 16-byte records
 * {C3[abc] + #rows before the record whose three preceding text symbols are abc, 96-bit mask of the record's rows holding abc},
 * so that one backward-search step consumes three pattern symbols for one 16-byte load per range end.  Built on the device
 * from `fmi`'s bwt_occ; out_trimer: nvbio_hip_fm_trimer_index_bytes(length) bytes, 128-byte aligned (a 128-byte header, then the
 * arrays); temp: nvbio_hip_fm_build_trimer_index_temp_bytes(length).  Attach with nvbio_hip_fm_attach_trimer_index, which checks the
 * header against `fmi` (magic, length, primary, stride, L2 check word) and that fmi->dimer is attached; NULL detaches. */
uint64_t nvbio_hip_fm_trimer_index_bytes(uint32_t length);
uint64_t nvbio_hip_fm_build_trimer_index_temp_bytes(uint32_t length);
int nvbio_hip_fm_build_trimer_index(const nvbio_hip_fmindex* fmi, uint32_t* out_trimer, void* temp, uint64_t temp_bytes, void* stream);
int nvbio_hip_fm_attach_trimer_index(nvbio_hip_fmindex* fmi, const uint32_t* trimer, void* stream);

/* ---- `_host` twins: the reference's HostThreadScheduler / host paths (batched_banded_inl.h:97-128,
 * batched_inl.h:236-300, the host fm_index functions) behind the same argument lists with HOST pointers everywhere and a
 * thread count (0 = OpenMP's default) instead of a stream.  Strings may be 2-, 4- or 8-bit packed.  Explicit entry points
 * for CPU-side callers; the device entry points never fall back to them. */
int nvbio_hip_banded_gotoh_score_host(const nvbio_hip_gotoh_scheme* scheme, int32_t type, uint32_t band_len,
                                      const nvbio_hip_string_set* patterns, const nvbio_hip_string_set* texts,
                                      uint32_t n, int32_t* out_score, uint32_t* out_sink, int32_t n_threads);
int nvbio_hip_banded_sw_score_host(const nvbio_hip_sw_scheme* scheme, int32_t type, uint32_t band_len,
                                   const nvbio_hip_string_set* patterns, const nvbio_hip_string_set* texts,
                                   uint32_t n, int32_t* out_score, uint32_t* out_sink, int32_t n_threads);
int nvbio_hip_alignment_score_host(int32_t aligner, int32_t algorithm, const int32_t* scheme4, int32_t type,
                                   const nvbio_hip_string_set* patterns, const nvbio_hip_string_set* texts, const int32_t* min_score /* nullable */,
                                   uint32_t n, int32_t* out_score, uint32_t* out_sink, uint8_t* out_ok /* nullable */, int32_t n_threads);
/* nvbio_hip_hamming_score / _qual: both algorithm tags, no shape limits (TextBlockingTag never exits early) */
int nvbio_hip_hamming_score_host(const nvbio_hip_sw_scheme* scheme, int32_t algorithm, int32_t type,
                                 const nvbio_hip_string_set* patterns, const nvbio_hip_string_set* texts, const int32_t* min_score /* nullable */,
                                 uint32_t n, int32_t* out_score, uint32_t* out_sink, uint8_t* out_ok /* nullable */, int32_t n_threads);
int nvbio_hip_hamming_score_qual_host(const nvbio_hip_gotoh_qual_scheme* scheme, int32_t algorithm, int32_t type,
                                      const nvbio_hip_string_set* patterns, const uint8_t* quals, uint64_t n_quals, const nvbio_hip_string_set* texts,
                                      const int32_t* min_score /* nullable */,
                                      uint32_t n, int32_t* out_score, uint32_t* out_sink, uint8_t* out_ok /* nullable */, int32_t n_threads);
int nvbio_hip_fm_rank_host(const nvbio_hip_fmindex* fmi, const uint32_t* k, const uint8_t* c, uint32_t n, uint32_t* out, int32_t n_threads);
int nvbio_hip_fm_match_host(const nvbio_hip_fmindex* fmi, const nvbio_hip_string_set* seeds, uint32_t n, uint32_t* out_range, int32_t n_threads);
int nvbio_hip_fm_locate_host(const nvbio_hip_fmindex* fmi, const uint32_t* sa_rows, uint32_t n, uint32_t* out_pos, int32_t n_threads);

/* Builds the optional k-mer table for `fmi` (fmi->ktab is ignored): out_ktab[2c..2c+1] =
 * match(fmi, kmer c), where kmer c has symbol t (0 = first) at bits [2t,2t+2) of c, for all
 * 4^k codes; 1 <= k <= 16; out_ktab holds 2*4^k words (k=12: 128 MiB, k=14: 2 GiB, k=15: 8 GiB, k=16: 32 GiB). */
int nvbio_hip_fm_build_ktab(const nvbio_hip_fmindex* fmi, uint32_t k, uint32_t* out_ktab, void* stream);
/* The suffix array sampled every sa_int_out rows (a power of two <= fmi->sa_int; 1 = the whole array), derived on the device from `fmi`'s own
 * sampled array: out_ssa[k] = locate(k * sa_int_out), nvbio_hip_fm_dense_ssa_entries(length, sa_int_out) = (length + sa_int_out) / sa_int_out
 * words (out_ssa[0] = 0xFFFFFFFF like every SSA, ssa_inl.h:263-309).  An index carrying it (ssa = out_ssa, sa_int = sa_int_out) locates with
 * at most sa_int_out - 1 LF steps -- none at 1 -- and returns the same positions: what 288 GB of HBM are for (12 GB at 3 Gbp). */
uint64_t nvbio_hip_fm_dense_ssa_entries(uint32_t length, uint32_t sa_int);
int nvbio_hip_fm_build_dense_ssa(const nvbio_hip_fmindex* fmi, uint32_t sa_int_out, uint32_t* out_ssa, void* stream);

/* nvBowtie's seeding parameters as map_queues_kernel reads them (nvBowtie/bowtie2/cuda/params.h:100-120). */
typedef struct nvbio_hip_map_params {
    uint32_t seed_len;       /* params.seed_len (22 end-to-end / 20 local)                       */
    uint32_t min_read_len;   /* shorter reads get no hits                                        */
    uint32_t max_hits;       /* per-read cap: beyond it the largest SA ranges are dropped (100)  */
    uint32_t max_reseed;     /* retry_stride = seed_freq / (max_reseed + 1)                      */
    uint32_t retry;          /* re-seeding round: seeds start at retry * retry_stride            */
    uint32_t rep_seeds;      /* reseed[] = no hit, or mean range size >= rep_seeds               */
    uint32_t fw, rc;         /* strands to map                                                   */
} nvbio_hip_map_params;

/* Replaces nvBowtie's exact seed mapping stage, map_queues_kernel<EXACT_MAPPING>
 * (nvBowtie/bowtie2/cuda/mapping_inl.h:511-592 with seed_mapper<EXACT_MAPPING>, :229-312, and
 * match_range, :83-97): for queue entry id (read in_queue[id], or id if in_queue is NULL) every seed
 * window of the read is searched on both strands and each non-empty SA range is stored as a SeedHit
 * word pair {range_begin; range_delta:20, pos_in_read:10, rc:1, index_dir:1} (seed_hit.h:54-223,
 * exclusive range) at out_hits[read * hits_stride + k], k < out_counts[read].  seed_freq_by_len[L] is
 * the host-tabulated params.seed_freq(L) (SimpleFunc, func.h:39-70) for every read length L that
 * occurs.  out_reseed (nullable) receives the reference's re-seeding predicate per queue entry. */
int nvbio_hip_map_exact(const nvbio_hip_fmindex* fmi, const nvbio_hip_string_set* reads,
                        const uint32_t* in_queue, uint32_t n, const nvbio_hip_map_params* params /* host */,
                        const uint32_t* seed_freq_by_len /* device */,
                        uint64_t* out_hits, uint32_t hits_stride, uint32_t* out_counts, uint8_t* out_reseed, void* stream);

/* nvBowtie's seed mapping algorithms (mapping_inl.h:118-123; chosen by map_t, :809-843, from
 * params.allow_sub / params.subseed_len). */
enum { NVBIO_HIP_EXACT_MAPPING = 0, NVBIO_HIP_APPROX_MAPPING = 1, NVBIO_HIP_CASE_PRUNING_MAPPING = 2 };

/* Replaces map_queues_kernel<ALGO> for all three algorithms (mapping_inl.h:511-592):
 *   EXACT         as nvbio_hip_map_exact (rfmi, subseed_len ignored)
 *   APPROX        seed_mapper<APPROX_MAPPING> (:318-365): per seed, map<CHECK_EXACT> of the stored seed and
 *                 map<IGNORE_EXACT> of its reversed complement on the forward index -- exact in the first
 *                 subseed_len scan symbols, one substitution (enumerated with rank4) in the rest
 *   CASE_PRUNING  seed_mapper<CASE_PRUNING_MAPPING> (:372-428): the four half-exact / half-one-mismatch
 *                 searches over the forward index fmi and the index of the reversed genome rfmi
 * with map<> as in mapping_inl.h:124-223 (N handling included).  Hits are SeedHit word pairs as in
 * nvbio_hip_map_exact, index_dir (bit 31) = 1 for hits found on rfmi.  Seeds up to 32 symbols.
 * A read's hits are stored in the array order of the reference's hit deque (see the selection stage below). */
int nvbio_hip_map(int32_t algorithm, uint32_t subseed_len,
                  const nvbio_hip_fmindex* fmi, const nvbio_hip_fmindex* rfmi /* CASE_PRUNING only */,
                  const nvbio_hip_string_set* reads, const uint32_t* in_queue, uint32_t n,
                  const nvbio_hip_map_params* params /* host */, const uint32_t* seed_freq_by_len /* device */,
                  uint64_t* out_hits, uint32_t hits_stride, uint32_t* out_counts, uint8_t* out_reseed, void* stream);

/* nvBowtie's reduction of extension results to the best two alignments per read: score_reduce_kernel
 * (nvBowtie/bowtie2/cuda/reduce_inl.h:71-160).  An io::Alignment (nvbio/io/alignments.h:80-131) is a uint64:
 * low word {score_sgn:1, score:17, ed:10, rc:1, mate:1, paired:1, discordant:1}, high word m_align;
 * best_alignments[read] is the best, best_alignments[read + best_stride] the second best (initialised by
 * nvbio_hip_init_alignments).  Active read t (read id read_ids[t], or t) owns the extension results
 * [hit_begin[t], hit_begin[t+1]) of hit_score / hit_loc / hit_rc, walked in that order: results at an already
 * recorded location are skipped, a higher score becomes the best (the old best the second), and a score above
 * the second best replaces it only if distinct_alignments(best, hit, read_len/2) (alignments_inl.h:35-47).
 * The context hooks of the reference (hit statistics / extension give-up counters) are not part of it. */
uint64_t nvbio_hip_alignment_invalid(void);
/* init_alignments (nvBowtie/bowtie2/cuda/aligner.h:323-366): best and second best of every read start unaligned
 * (pos -1, ed 255) with score worst_score_by_len[read length] = the scheme's threshold score (device table). */
int nvbio_hip_init_alignments(uint32_t n_reads, const uint32_t* read_len /* nullable */, uint32_t fixed_read_len,
                              const int32_t* worst_score_by_len /* device */, uint32_t mate,
                              uint64_t* best_alignments, uint32_t best_stride, void* stream);
int nvbio_hip_score_reduce(uint32_t n_active, const uint32_t* read_ids /* nullable */, const uint64_t* hit_begin,
                           const int32_t* hit_score, const uint32_t* hit_loc, const uint8_t* hit_rc,
                           const uint32_t* read_len /* by read id, nullable */, uint32_t fixed_read_len,
                           uint64_t* best_alignments, uint32_t best_stride, void* stream);

/* ---- nvBowtie hit selection and the per-round stages of its best-approx extension loop --------------------------
 * (driver: Aligner::best_approx_score, nvBowtie/bowtie2/cuda/aligner_best_approx.h:522-840.)
 *
 * The hit arena written by nvbio_hip_map* IS the reference's SeedHitDequeArray content: a read's SeedHits sit at
 * hits[read_id * hits_stride] in the array order of its priority_deque (interval heap, nvbio/basic/interval_heap.h;
 * slot 0 = a largest range, top() = slot 1, or slot 0 when alone), hit_counts[read_id] is the deque size.  The
 * probability tree of the randomized selection (SumTree<float*>, nvbio/basic/sum_tree.h) of read r lives at
 * probs[r * probs_stride] as its LEAVES: leaf i (i < hit_counts[r]) at probs[r * probs_stride + i].  Every other node of a SumTree is
 * the float sum of its two children, so the kernels rebuild them on chip -- bit for bit the values the reference keeps in memory -- and
 * a pick that exhausts a hit writes one zero instead of a leaf and four ancestors (the stage is bound by the lines it moves).
 * probs_stride >= hits_stride (a multiple of 4 lets the kernels use 16-byte accesses); rows wider than 32 hit slots are handled one
 * lane per read with the sums in the row itself, as scratch: probs_stride >= nvbio_hip_sum_tree_node_count(hits_stride) there.
 * Active reads are packed_read words (defs.h:152-162: read_id:31, top_flag:1); a selected hit is {read_id, loc, seed}
 * with seed a packed_seed word (defs.h:171-181: pos_in_read:12, index_dir:1, rc:1, top_flag:1).
 * Floating point: single precision, every operation rounded separately (the host-compiled arithmetic). */
uint32_t nvbio_hip_sum_tree_node_count(uint32_t size);
/* select_init_kernel (select.cu:36-103): trys[r] = max_effort_init (if trys); when randomized, rseeds[r] = hash of the
 * read's name (names NUL-terminated in read_names at read_names_idx[r]; with read_names NULL rseeds is left as the
 * caller set it), probs = the leaves: 1 / range_size^2 per hit (the first 0 if top_seed). */
int nvbio_hip_select_init(uint32_t n_reads, const char* read_names, const uint32_t* read_names_idx,
                          const uint64_t* hits, uint32_t hits_stride, const uint32_t* hit_counts,
                          float* probs, uint32_t probs_stride, uint32_t* trys /* nullable */, uint32_t* rseeds,
                          uint32_t max_effort_init, int32_t randomized, int32_t top_seed, void* stream);
/* The same for the reads of a queue only (queue: device uint32[n_queue] read ids): a re-seeding pass gives hits to its queue's reads
 * alone, and no read outside it is selected from before the next select_init reaches it, so the state the reference's whole-batch
 * kernel writes for the others is never read. */
int nvbio_hip_select_init_queued(uint32_t n_queue, const uint32_t* queue, const char* read_names, const uint32_t* read_names_idx,
                                 const uint64_t* hits, uint32_t hits_stride, const uint32_t* hit_counts,
                                 float* probs, uint32_t probs_stride, uint32_t* trys /* nullable */, uint32_t* rseeds,
                                 uint32_t max_effort_init, int32_t randomized, int32_t top_seed, void* stream);
/* select (select_inl.h:74-607; dispatch :744-795): one round of hit selection for the reads of active_in.  Reads whose
 * try counter is 0 or whose deque is empty leave the queue; the others hand out up to n_multi SA rows each (n_multi == 1:
 * select_kernel / rand_select_kernel, > 1: the *_multi_kernel forms), from the deque's top range downwards, or -- randomized
 * -- from hits sampled in proportion to probs with the read's LCG.  Outputs, in the order of active_in (the reference's
 * slot order is atomic-dependent): active_out[n_out], the selected hits grouped per read with hit_begin[n_out + 1]
 * offsets, out_sizes = {n_out, n_hits} (device).  active_out / hit_begin need n_active (+1) entries, the hit arrays
 * n_active * n_multi.  hits / hit_counts / probs / rseeds are updated in place.  n_multi <= 4096. */
uint64_t nvbio_hip_select_temp_bytes(uint32_t n_active, uint32_t n_multi);
int nvbio_hip_select(int32_t randomized, uint32_t n_multi, const uint32_t* active_in, uint32_t n_active,
                     uint64_t* hits, uint32_t hits_stride, uint32_t* hit_counts,
                     float* probs, uint32_t probs_stride, uint32_t* rseeds, const uint32_t* trys,
                     uint32_t* active_out, uint64_t* hit_begin, uint32_t* hit_read_id, uint32_t* hit_loc, uint32_t* hit_seed,
                     uint32_t* out_sizes, void* temp, uint64_t temp_bytes, void* stream);
/* Diagnostic: runs programs of deque operations (ops[i]: 0 = push vals[i], dropping the bottom first when the deque
 * holds caps[i] hits; 1 = pop_top; 2 = pop_bottom; program c = [case_start[c], case_start[c+1])) through the device's
 * hit deque and writes the deque's array after every operation from out_states[state_start[c]] on.  scratch: n_cases *
 * scratch_stride words.  Used to replay vectors recorded from the reference's interval heap. */
int nvbio_hip_hit_deque_replay(uint32_t n_cases, const uint32_t* case_start, const uint8_t* ops, const uint64_t* vals, const uint32_t* caps,
                               const uint64_t* state_start, uint64_t* scratch, uint32_t scratch_stride, uint64_t* out_states, void* stream);
/* locate_kernel (locate_inl.h:53-143): hit_loc[i] (an SA row of fmi, or of rfmi when the seed's index_dir is REVERSE)
 * becomes the read's start in genome coordinates: locate - pos_in_read, mirrored (length-1-locate) for rfmi; uint32
 * arithmetic, so a read hanging over the genome start wraps.  rfmi may be NULL when no hit uses it. */
int nvbio_hip_locate_hits(const nvbio_hip_fmindex* fmi, const nvbio_hip_fmindex* rfmi, uint32_t n,
                          uint32_t* hit_loc, const uint32_t* hit_seed, void* stream);
/* BestScoreStream::init_context (score_best_inl.h:95-126): per hit, the genome window [loc - band/2 (clamped at 0),
 * + band + read_len (clamped at genome_length)), the threshold max(second best score of the read, score_limit) and
 * the pattern (read r's forward copy at read_begin[r] -- or r * fixed_read_len -- or its reverse complement rc_offset
 * symbols further, by the seed's rc bit).  A window beginning at or beyond its end gets length 0 (the reference
 * would read out of bounds); the alignment then fails like any text shorter than its pattern. */
int nvbio_hip_score_best_setup(uint32_t n_hits, const uint32_t* hit_read_id, const uint32_t* hit_loc, const uint32_t* hit_seed,
                               const uint64_t* read_begin /* nullable */, const uint32_t* read_len /* nullable */, uint32_t fixed_read_len,
                               uint64_t rc_offset, uint32_t band_len, uint32_t genome_length,
                               const uint64_t* best_alignments, uint32_t best_stride, int32_t score_limit,
                               uint64_t* pattern_begin, uint32_t* pattern_len /* nullable iff fixed */,
                               uint64_t* text_begin, uint32_t* text_len, int32_t* min_score,
                               int32_t* known_score /* nullable, see below */,
                               uint32_t* job_count /* nullable, device */, uint32_t* job_hit /* nullable, n_hits */, void* stream);
/* known_score (optional, a pure saving): a hit whose (strand, read start) equals one of the read's two recorded alignments would be
 * scored over the same window again and get the recorded score.  With known_score != NULL such hits get known_score[i] = that score
 * and an empty window (INT32_MIN marks the others); handing the array to nvbio_hip_score_reduce_best_approx makes the reduction use
 * it in place of the (absent) DP result, so every output is what the reference computes by re-running the DP.
 * job_count / job_hit (optional, both or neither, need known_score): compacted jobs.  Only the hits that still need a DP are written,
 * at slots 0..*job_count-1 of pattern_begin / pattern_len / text_begin / text_len / min_score, with job_hit[slot] = the hit; run the DP
 * over *job_count jobs, scatter its scores into known_score (nvbio_hip_scatter_rows(n_jobs, job_hit, scores, known_score, 4)) and
 * hand known_score to the reduction as hit_score.  The slot order is not deterministic; everything indexed by hit is. */
/* score_reduce_kernel with ReduceBestApproxContext (reduce_inl.h:71-160, reduce.h:63-105): nvbio_hip_score_reduce over
 * packed active reads and packed seeds, plus the give-up counters: see reduce.hip.  hit_score is the raw DP score
 * (clamped to worst_score = scheme_type::worst_score here); n_ext = extensions done before this round. */
int nvbio_hip_score_reduce_best_approx(uint32_t n_active, const uint32_t* active_reads, const uint64_t* hit_begin,
                                       const int32_t* hit_score, const uint32_t* hit_loc, const uint32_t* hit_seed,
                                       const uint32_t* read_len /* nullable */, uint32_t fixed_read_len,
                                       uint64_t* best_alignments, uint32_t best_stride, int32_t worst_score,
                                       uint32_t* trys, uint32_t* hit_counts,
                                       uint32_t n_ext, uint32_t min_ext, uint32_t max_ext, uint32_t max_effort,
                                       const int32_t* known_score /* nullable: from nvbio_hip_score_best_setup */,
                                       const uint32_t* hit_sink /* nullable uint2[n_hits]: the DP sinks */, uint32_t* best_sink /* nullable uint2[n_reads] */,
                                       void* stream);
/* hit_sink / best_sink (optional, both or neither): whenever a hit becomes a read's best alignment its DP sink is kept in best_sink[read].
 * nvbio_hip_traceback_best_known then lays out, per traceback job, the score and sink the banded scorer would report over the job's
 * window (the same DP the extension ran; unaligned entries: a failed alignment, score -2^30, sink (-1,-1)), and
 * nvbio_hip_banded_gotoh_traceback_qual_known starts from them instead of scoring every job again.  Results are the traceback's. */
int nvbio_hip_traceback_best_known(uint32_t n, const uint32_t* idx /* nullable */, const uint64_t* best_alignments, const uint32_t* best_sink /* nullable */,
                                   int32_t* out_score, uint32_t* out_sink /* nullable with best_sink: scores only */, void* stream);

/* The paired-end form: score_reduce_paired_kernel (reduce_inl.h:355-500).  Per extension result the anchor mate's
 * {loc, sink (genome end), score, rc} and the opposite mate's {loc, sink, sink2, score, score2} (the stream's hit.* fields,
 * score_opposite_inl.h:203-235); the pair is `paired` when the opposite score exceeds score_limit.  best_alignments holds
 * the anchor (or, while no pair was found and pe_unpaired, mate 1) entries, best_alignments_o the opposite (mate 2) ones.
 * anchor: 0 / 1; pe_policy: io::PairedEndPolicy (FF 0, FR 1, RF 2, RR 3). */
int nvbio_hip_score_reduce_paired(uint32_t n_active, const uint32_t* read_ids /* nullable */, const uint64_t* hit_begin,
    const uint32_t* hit_loc, const uint32_t* hit_sink, const int32_t* hit_score, const uint8_t* hit_rc,
    const uint32_t* opposite_loc, const uint32_t* opposite_sink, const uint32_t* opposite_sink2,
    const int32_t* opposite_score, const int32_t* opposite_score2,
    const uint32_t* read_len /* nullable */, uint32_t fixed_read_len, uint32_t anchor, int32_t pe_policy, int32_t pe_unpaired, int32_t score_limit,
    uint64_t* best_alignments, uint64_t* best_alignments_o, uint32_t best_stride, void* stream);

/* The paired-end parameters the opposite-mate stage reads (nvBowtie/bowtie2/cuda/params.h: pe_policy, min_frag_len,
 * max_frag_len, pe_overlap) plus the pipeline's score_limit, anchor (0 / 1) and genome_length. */
typedef struct nvbio_hip_pe_params {
    int32_t  pe_policy, min_frag_len, max_frag_len, pe_overlap, score_limit;
    uint32_t anchor, genome_length;
} nvbio_hip_pe_params;

/* BestOppositeScoreStream::init_context (nvBowtie/bowtie2/cuda/score_opposite_inl.h:92-200) for every scored anchor hit:
 * the opposite mate's score threshold (compute_target_score, alignment_utils.h:100-111, clamped by the mate's own worst score
 * and score_limit), its strand (frame_opposite_mate), and the genome window [begin, end) allowed by the fragment-length limits
 * and max_text_gaps (utils_inl.h:181-204).  out_valid = the function's bool (threshold reachable, window inside the genome and
 * non-empty, location not already recorded in the best pairs).  The windows + thresholds feed nvbio_hip_alignment_score_qual. */
int nvbio_hip_opposite_mate_windows(uint32_t n_hits, const uint32_t* hit_read_id, const uint8_t* hit_rc, const uint32_t* hit_loc, const int32_t* hit_score,
    const uint32_t* a_read_len /* nullable */, const uint32_t* o_read_len /* nullable */, uint32_t a_fixed_len, uint32_t o_fixed_len,
    const uint64_t* best_alignments, const uint64_t* best_alignments_o, uint32_t best_stride,
    int32_t match, const int32_t* min_score_by_len /* device */, int32_t text_gap_open, int32_t text_gap_ext, const nvbio_hip_pe_params* params /* host */,
    uint8_t* out_valid, int32_t* out_min_score, uint8_t* out_read_rc, uint32_t* out_genome_begin, uint32_t* out_genome_end, void* stream);

/* ---- the per-round stages of nvBowtie's PAIRED best-approx loop (Aligner::best_approx_score, aligner_best_approx_paired.h:455-700):
 * select / locate as in the single-end loop, then
 *   anchor_score_best    BestAnchorScoreStream (score_paired_inl.h:54-150): nvbio_hip_anchor_score_setup (window, pattern, threshold
 *                        from the read's best pairs; hits at recorded locations are skipped), the banded scorer, _finish (hit.score =
 *                        score >= threshold ? score : worst_score; hit.sink = window begin + sink.x)
 *   opposite_score_best  BestOppositeScoreStream (score_opposite_inl.h:54-235): nvbio_hip_opposite_score_setup = nvbio_hip_opposite_mate_windows
 *                        over packed seeds, valid only for hits whose anchor score is not worst_score (the opposite queue), the full-matrix
 *                        scorer over the valid hits, _finish (scatter of hit.opposite_* for those; the caller pre-fills worst_score)
 *   score_reduce_paired  with ReduceBestApproxContext: nvbio_hip_score_reduce_paired_best_approx
 * and after the loops nvbio_hip_mark_discordant (aligner_init.cu:457-480).  The reference's skip test of the anchor stream reads
 * context->min_score before setting it (score_paired_inl.h:128); that term is taken as false here. */
int nvbio_hip_anchor_score_setup(uint32_t n_hits, const uint32_t* hit_read_id, const uint32_t* hit_loc, const uint32_t* hit_seed,
    const uint64_t* a_read_begin /* nullable */, const uint32_t* a_read_len /* nullable */, const uint32_t* o_read_len /* nullable */,
    uint32_t a_fixed_len, uint32_t o_fixed_len, uint64_t rc_offset,
    uint32_t band_len, uint32_t genome_length, const uint64_t* best_alignments, const uint64_t* best_alignments_o, uint32_t best_stride,
    int32_t match, const int32_t* min_score_by_len /* device */, int32_t score_limit, uint32_t anchor,
    uint64_t* pattern_begin, uint32_t* pattern_len /* nullable iff fixed */, uint64_t* text_begin, uint32_t* text_len, int32_t* min_score, void* stream);
int nvbio_hip_anchor_score_finish(uint32_t n_hits, const int32_t* raw_score, const uint32_t* raw_sink /* uint2[n] */, const uint64_t* text_begin,
    const int32_t* min_score, int32_t worst_score, int32_t* hit_score, uint32_t* hit_sink, void* stream);
int nvbio_hip_opposite_score_setup(uint32_t n_hits, const uint32_t* hit_read_id, const uint32_t* hit_seed, const uint32_t* hit_loc, const int32_t* hit_score,
    int32_t worst_score, const uint32_t* a_read_len, const uint32_t* o_read_len, uint32_t a_fixed_len, uint32_t o_fixed_len,
    const uint64_t* best_alignments, const uint64_t* best_alignments_o, uint32_t best_stride,
    int32_t match, const int32_t* min_score_by_len /* device */, int32_t text_gap_open, int32_t text_gap_ext, const nvbio_hip_pe_params* params /* host */,
    uint8_t* out_valid, int32_t* out_min_score, uint8_t* out_read_rc, uint32_t* out_genome_begin, uint32_t* out_genome_end,
    /* optional (all NULL / 0 to skip): the full-matrix job of every hit -- pattern = the opposite mate's forward copy at o_read_begin[r]
     * (or r * o_fixed_len), its reverse complement o_rc_offset symbols further; text = the window, empty for invalid hits */
    const uint64_t* o_read_begin, uint64_t o_rc_offset, uint64_t* out_pattern_begin, uint64_t* out_text_begin, uint32_t* out_text_len, void* stream);
/* valid_idx != NULL: raw results of the n_valid scored hits valid_idx[k]; valid_idx == NULL: one raw result per hit (n_valid = n_hits) and
 * valid_flags[h] says whether hit h was scored (the others get worst_score) */
int nvbio_hip_opposite_score_finish(uint32_t n_valid, const uint32_t* valid_idx, const uint8_t* valid_flags, const int32_t* raw_score /* [n_valid] */, const uint32_t* raw_sink /* uint2[n_valid] */,
    const int32_t* min_score /* by hit */, const uint32_t* genome_begin /* by hit */, int32_t worst_score,
    int32_t* opposite_score, int32_t* opposite_score2, uint32_t* opposite_loc, uint32_t* opposite_sink, uint32_t* opposite_sink2, void* stream);
int nvbio_hip_score_reduce_paired_best_approx(uint32_t n_active, const uint32_t* active_reads, const uint64_t* hit_begin,
    const uint32_t* hit_loc, const uint32_t* hit_sink, const int32_t* hit_score, const uint32_t* hit_seed,
    const uint32_t* opposite_loc, const uint32_t* opposite_sink, const uint32_t* opposite_sink2, const int32_t* opposite_score, const int32_t* opposite_score2,
    const uint32_t* read_len /* nullable */, uint32_t fixed_read_len, uint32_t anchor, int32_t pe_policy, int32_t pe_unpaired, int32_t score_limit,
    uint64_t* best_alignments, uint64_t* best_alignments_o, uint32_t best_stride,
    uint32_t* trys, uint32_t* hit_counts, uint32_t n_ext, uint32_t min_ext, uint32_t max_ext, uint32_t max_effort, void* stream);
/* The anchor memo (optional, a pure saving).  The anchor's banded DP is a pure function of (pair, which mate, strand, window); the reference's skip test
 * (aligner_best_approx_paired.h: BestAnchorScoreStream::init_context compares a hit's position with the recorded alignments' window begins) almost
 * never fires, so every seed of a read that points at the placement the read already tried pays the DP again and absorbs the identical score.
 * memo: 6 words per pair, zero-initialised by the caller, holding the last job {window begin, strand, mate} and its raw score and sink.
 *   anchor_memo_mark (after anchor_score_setup, before the DP): text_len_out[i] = text_len[i], or 0 for a hit whose job equals the pair's entry
 *     (from_memo[i] = 1) or the job of the hit before it in this round (from_memo[i] = 2): the scorer's lane returns at once on an empty text.
 *     text_len_out must not alias text_len (the update reads the set-up lengths).  live_count / live_idx (optional): the hits left with a window,
 *     counted and listed on the device -- the job_index / gate of nvbio_hip_banded_gotoh_score_qual_wave for rounds that hold only a few.
 *   anchor_score_finish_memo: nvbio_hip_anchor_score_finish, a marked hit taking its raw score and sink from the entry / the hit it repeats.
 *   anchor_memo_update (after the finish): per active read, the last hit of the round that had a window becomes the pair's entry.
 * Every output equals what re-running the DP gives. */
int nvbio_hip_anchor_memo_mark(uint32_t n_hits, const uint32_t* hit_read_id, const uint32_t* hit_seed, const uint64_t* text_begin, const uint32_t* text_len,
    uint32_t anchor, const uint32_t* memo, uint8_t* from_memo, uint32_t* text_len_out,
    uint32_t* live_count /* nullable; device, zeroed by the call */, uint32_t* live_idx /* nullable with it: the hits that still need their DP */, void* stream);
int nvbio_hip_anchor_score_finish_memo(uint32_t n_hits, const int32_t* raw_score, const uint32_t* raw_sink, const uint64_t* text_begin, const int32_t* min_score,
    int32_t worst_score, const uint8_t* from_memo, const uint32_t* hit_read_id, const uint32_t* memo, int32_t* hit_score, uint32_t* hit_sink, void* stream);
int nvbio_hip_anchor_memo_update(uint32_t n_active, const uint32_t* active_reads, const uint64_t* hit_begin, const uint32_t* hit_read_id, const uint32_t* hit_seed,
    const uint64_t* text_begin, const uint32_t* text_len_setup, const uint8_t* from_memo, const int32_t* raw_score, const uint32_t* raw_sink, uint32_t anchor, uint32_t* memo, void* stream);
/* The opposite-mate memo (optional, a pure saving).  The opposite mate's DP is a pure function of (pair, opposite strand, window,
 * threshold); the reference re-runs it for every anchor hit landing on a placement it already tried and absorbs the identical result
 * (in the second anchor pass that is every seed of every read).  memo: 6 words per pair, zero-initialised by the caller, holding the
 * last scored job and its outputs.
 *   opposite_memo_lookup (after opposite_score_setup, before the DP): a valid hit whose job equals the pair's entry gets its
 *     opposite_* outputs from it, valid[i] = 2 and (if text_len != NULL) an empty text; nvbio_hip_opposite_score_finish leaves such
 *     hits alone (with the valid_idx form, pass only the hits with valid == 1).
 *   opposite_memo_update (after opposite_score_finish): per active read, the last hit with valid == 1 becomes the pair's entry.
 * Every output equals what re-running the DP gives; hits of one pair in the SAME round are not matched against each other. */
/* idx[0 .. *count) = the indices i < n with flags[i] == value (in no particular order); count is zeroed by the call.  The list of jobs a round
 * still has to score, for the job_index forms of the scorers. */
int nvbio_hip_list_flagged(uint32_t n, const uint8_t* flags, uint32_t value, uint32_t* count, uint32_t* idx, void* stream);
int nvbio_hip_opposite_memo_lookup(uint32_t n_hits, const uint32_t* hit_read_id, uint8_t* valid, const uint8_t* read_rc, const uint32_t* genome_begin,
    const uint32_t* genome_end, const int32_t* min_score, uint32_t anchor, const uint32_t* memo, int32_t worst_score,
    int32_t* opposite_score, int32_t* opposite_score2, uint32_t* opposite_loc, uint32_t* opposite_sink, uint32_t* opposite_sink2,
    uint32_t* text_len /* nullable */, void* stream);
int nvbio_hip_opposite_memo_update(uint32_t n_active, const uint32_t* active_reads, const uint64_t* hit_begin, const uint8_t* valid, const uint8_t* read_rc,
    const uint32_t* genome_begin, const uint32_t* genome_end, const int32_t* min_score, const int32_t* opposite_score, const uint32_t* opposite_sink,
    uint32_t anchor, uint32_t* memo, void* stream);
int nvbio_hip_mark_discordant(uint32_t n_reads, uint64_t* best_alignments, uint64_t* best_alignments_o, uint32_t best_stride, void* stream);

/* pack_read(top_seed) over a read queue (nvBowtie/bowtie2/cuda/defs.h:185-205): out[i] = {read_id:31 = queue[i], top_flag:1},
 * the form the active-read queues of the extension rounds hold.  queue == NULL stands for the identity queue 0 .. n-1 (with
 * top_flag 0: the initial seed queue of a batch, written on the device). */
int nvbio_hip_pack_read_queue(uint32_t n, const uint32_t* queue, uint32_t top_flag, uint32_t* out, void* stream);

/* ---- what nvBowtie's host drivers do between the stages (they use thrust / nvbio primitives for it) ----
 * mark_unaligned (aligner_init.cu:421-444): reseed[t] = 1 for every queued read whose best alignment is still unaligned.
 * copy_flagged (nvbio/basic/primitives.h, used at aligner_best_approx.h:273-280): out = the in[i] with flags[i] != 0, in
 * order; *out_count (device) = how many.
 * traceback_best_setup = BestTracebackStream::init_context (traceback_inl.h:104-136) over best_alignments[idx[i]] (or [i]):
 * want 0: every aligned entry, banded window [alignment - band/2, + band + read_len); want 1: concordant entries, the
 * opposite mate's window [alignment, alignment + sink) (opposite_traceback_best); want 2: aligned, not concordant, banded
 * window.  Patterns: the read's copy at read_begin[r] (or r * fixed_read_len), + rc_offset for reverse-complement
 * alignments, + mate_offset when the alignment's mate bit is set.  Entries that do not qualify get out_valid 0 and an
 * empty window. */
int nvbio_hip_mark_unaligned(uint32_t n_active, const uint32_t* active_reads, const uint64_t* best_alignments, uint8_t* reseed, void* stream);
uint64_t nvbio_hip_copy_flagged_temp_bytes(uint32_t n);
int nvbio_hip_copy_flagged(uint32_t n, const uint32_t* in, const uint8_t* flags, uint32_t* out, uint32_t* out_count /* device */,
                           void* temp, uint64_t temp_bytes, void* stream);
int nvbio_hip_scatter_rows(uint32_t n, const uint32_t* idx, const void* src, void* dst, uint32_t row_bytes /* multiple of 4 */, void* stream);   /* dst row idx[i] = src row i */
int nvbio_hip_gather_rows(uint32_t n, const uint32_t* idx, const void* src, void* dst, uint32_t row_bytes /* multiple of 4 */, void* stream);    /* dst row i = src row idx[i] */
int nvbio_hip_traceback_best_setup(uint32_t n, const uint32_t* idx /* nullable */, const uint64_t* best_alignments, uint32_t band_len, uint32_t genome_length,
                                   const uint64_t* read_begin /* nullable */, const uint32_t* read_len /* nullable */, uint32_t fixed_read_len,
                                   uint64_t rc_offset, uint64_t mate_offset, int32_t want,
                                   uint8_t* out_valid, uint64_t* pattern_begin, uint32_t* pattern_len /* nullable iff fixed */,
                                   uint64_t* text_begin, uint32_t* text_len, void* stream);
/* ... for pairs whose mates have their own lengths (the reference's paired driver takes them as they come, aligner_best_approx_paired.h): mate m's
 * reads sit at read_begin[m][r] (or r * fixed_read_len[m]) of ITS half of the pattern stream, reverse complements rc_offset[m] further; mate 1's
 * half starts mate_offset symbols into the stream.  The entry's mate bit picks the half.  pattern_len is always written. */
int nvbio_hip_traceback_best_setup_mates(uint32_t n, const uint32_t* idx /* nullable */, const uint64_t* best_alignments, uint32_t band_len, uint32_t genome_length,
                                         const uint64_t* const read_begin[2] /* host array of device pointers, each nullable */, const uint32_t* const read_len[2],
                                         const uint32_t fixed_read_len[2], const uint64_t rc_offset[2], uint64_t mate_offset, int32_t want,
                                         uint8_t* out_valid, uint64_t* pattern_begin, uint32_t* pattern_len, uint64_t* text_begin, uint32_t* text_len, void* stream);

/* finish_alignment_kernel + BestTracebackStream::finish (nvBowtie/bowtie2/cuda/traceback_inl.h:523-722, :177-189): for job i with
 * valid[i] != 0, replay its CIGAR (cigar[i * cigar_stride ..], cigar_len[i] words stored end first, first text column
 * cigar_source[2i] & 0xFFFF) over pattern i and text i (the window of nvbio_hip_traceback_best_setup) and write
 *   - out_mds[i * mds_stride ..]: the MD string in nvbio's byte code (io::MDS_OP, nvbio/io/alignments.h:46-52): bytes 0-1 its length,
 *     then {MDS_MATCH 0, run <= 255} / {MDS_MISMATCH 1, read symbol} / {MDS_INSERTION 2 | MDS_DELETION 3, length byte, symbols};
 *     out_mds_len[i] its length (bytes beyond mds_stride are counted, not stored);
 *   - the alignment best_alignments[idx ? idx[i] : i] rewritten: m_align = the text's begin, m_ed = mismatches + inserted / deleted
 *     symbols (soft clips excluded), m_score = sum over the SUBSTITUTION columns of scoring_scheme.score (scoring.h:301-311):
 *     -n_penalty when the read symbol is N, else match or mismatch_by_quality[q] (host table of -m_mmp(q)); minus, per INSERTION run of
 *     l read symbols, cumulative_deletion(l) = -(text_gap_open + (l - 1) text_gap_ext), and per DELETION run cumulative_insertion(l) =
 *     -(pattern_gap_open + (l - 1) pattern_gap_ext) (traceback_inl.h:664-665).  gap_costs (host, 4 ints): pattern_gap_open, pattern_gap_ext,
 *     text_gap_open, text_gap_ext as nvbio_hip_gotoh_qual_scheme holds them (<= 0).
 * Jobs with valid 0, no CIGAR, or a CIGAR longer than cigar_stride are skipped (out_mds_len 0, alignment untouched). */
int nvbio_hip_finish_alignment(uint32_t n, const uint8_t* valid, const nvbio_hip_string_set* patterns, const uint8_t* quals /* nullable */, uint64_t n_quals,
                               const nvbio_hip_string_set* texts, const uint16_t* cigar, uint32_t cigar_stride, const uint32_t* cigar_len,
                               const uint32_t* cigar_source /* uint2[n] */, int32_t match, const int32_t* mismatch_by_quality /* host, 256 */, int32_t n_penalty,
                               const int32_t* gap_costs /* host, 4 */, const uint32_t* idx /* nullable */, uint64_t* best_alignments, uint8_t* out_mds, uint32_t mds_stride, uint32_t* out_mds_len, void* stream);

/* ---- all-mapping mode (Aligner::all / score_all, nvBowtie/bowtie2/cuda/aligner_all.h:47-694) ----
 * Every row of every SA range in every read's hit deque is located, de-duplicated, extended, and reported when its score reaches
 * scoring_scheme.min_score(read_len).  The host driver (nvbio_amd.aligner.all_mapping) does the scans, sorts and compactions the
 * reference does with thrust; the device stages are:
 *   gather_ranges (mapping.cu:39-67): out_ranges[t] = the size of SA range t, ranges numbered read by read in deque array order
 *     (hit_count_scan = inclusive scan of the deque sizes).
 *   select_all (select.cu:175-219): hit begin + t, numbered through hit_range_scan (inclusive scan of out_ranges) ->
 *     out_loc = its SA row (range begin + row), out_seed = packed_seed(pos_in_read, index_dir, rc, 0), out_read_id.
 *   mark_straddling (locate_inl.h:213-244): flags[t] = 0 when hit idx_queue[t]'s seed [loc, loc + seed_len] crosses a boundary of
 *     sequence_index (n_sequences + 1 offsets) -- the indexing (hit idx_queue[t], flag t) is the reference's.
 *   score_all_setup (AllScoreStream::init_context, score_all_inl.h:99-127): job i = hit idx[i] (or i): window
 *     [loc - band/2, + band + read_len) clamped to the genome, pattern = the read's copy (+ rc_offset on the reverse strand).
 *   score_all_output (AllScoreStream::output, :131-153): out_flags[i] = score[i] >= min_score_by_len[read_len]; out_alignments[i] =
 *     io::Alignment(loc, 0, score, rc); out_read_id[i] (the reference appends the accepted ones to a ring buffer in atomic order;
 *     here the caller compacts by the flags, in job order).
 *   traceback_all_setup (AllTracebackStream::init_context, traceback_inl.h:361-385): the same windows from alignment words. */
int nvbio_hip_gather_ranges(uint32_t n_ranges, uint32_t n_reads, const uint64_t* hits, uint32_t hits_stride, const uint32_t* hit_count_scan,
                            uint64_t* out_ranges, void* stream);
int nvbio_hip_select_all(uint64_t begin, uint32_t count, uint32_t n_reads, uint32_t n_ranges, const uint64_t* hits, uint32_t hits_stride,
                         const uint32_t* hit_count_scan, const uint64_t* hit_range_scan, uint32_t* out_loc, uint32_t* out_seed, uint32_t* out_read_id,
                         void* stream);
int nvbio_hip_mark_straddling(uint32_t n, const uint32_t* idx_queue, uint32_t n_sequences, const uint32_t* sequence_index, const uint32_t* hit_loc,
                              uint32_t seed_len, uint8_t* flags, void* stream);
int nvbio_hip_score_all_setup(uint32_t n, const uint32_t* idx /* nullable */, const uint32_t* hit_read_id, const uint32_t* hit_loc, const uint32_t* hit_seed,
                              const uint64_t* read_begin /* nullable */, const uint32_t* read_len /* nullable */, uint32_t fixed_read_len, uint64_t rc_offset,
                              uint32_t band_len, uint32_t genome_length,
                              uint64_t* pattern_begin, uint32_t* pattern_len /* nullable iff fixed */, uint64_t* text_begin, uint32_t* text_len, void* stream);
int nvbio_hip_score_all_output(uint32_t n, const uint32_t* idx /* nullable */, const uint32_t* hit_read_id, const uint32_t* hit_loc, const uint32_t* hit_seed,
                               const int32_t* score, const int32_t* min_score_by_len /* device */, const uint32_t* read_len /* nullable */, uint32_t fixed_read_len,
                               uint8_t* out_flags, uint64_t* out_alignments, uint32_t* out_read_id, void* stream);
int nvbio_hip_traceback_all_setup(uint32_t n, const uint64_t* alignments, const uint32_t* read_id,
                                  const uint64_t* read_begin /* nullable */, const uint32_t* read_len /* nullable */, uint32_t fixed_read_len, uint64_t rc_offset,
                                  uint32_t band_len, uint32_t genome_length,
                                  uint64_t* pattern_begin, uint32_t* pattern_len /* nullable iff fixed */, uint64_t* text_begin, uint32_t* text_len, void* stream);

/* The library primitives score_all calls between those kernels (thrust::inclusive_scan, Aligner::sort_hi_bits / sort_64_bits of
 * aligner_sort.cu:39-92, the dedup transform of aligner_all.h:498-509), on hipCUB; temp: nvbio_hip_all_mapping_temp_bytes(n) bytes.
 *   sort_hi_bits: out_idx = the permutation that stably sorts keys[i] >> 16.
 *   sort_hits: out_idx = the permutation that stably sorts SortingKeys = loc + (read_id << 33) + (rc << 32);
 *     out_first[i] = 1 when sorted position i holds the first of a run of equal keys (the dedup flags before mark_straddling). */
uint64_t nvbio_hip_all_mapping_temp_bytes(uint32_t n);
int nvbio_hip_inclusive_scan_u32(uint32_t n, const uint32_t* in, uint32_t* out, void* temp, uint64_t temp_bytes, void* stream);
int nvbio_hip_inclusive_scan_u64(uint32_t n, const uint64_t* in, uint64_t* out, void* temp, uint64_t temp_bytes, void* stream);
int nvbio_hip_sort_hi_bits(uint32_t n, const uint32_t* keys, uint32_t* out_idx, void* temp, uint64_t temp_bytes, void* stream);
int nvbio_hip_sort_hits(uint32_t n, const uint32_t* hit_read_id, const uint32_t* hit_loc, const uint32_t* hit_seed, uint32_t* out_idx, uint8_t* out_first,
                        void* temp, uint64_t temp_bytes, void* stream);
/*   sort_hits_pingpong: sort_hits, and the index Aligner::all's mark_straddling actually reads (aligner_all.h:520): `pipeline.idx_queue` is the
 *     pointer sort_hi_bits returned (:465) -- one half of the ping-pong index buffer, which sort_64_bits (:500) has refilled and sorted through
 *     since.  Both sorts are replayed on one pair of halves as aligner_sort.cu:37-86 makes them; out_stale[n] = what the first sort's half holds
 *     after the second (the final index when both end in the same half, the last pass but one's otherwise). */
int nvbio_hip_sort_hits_pingpong(uint32_t n, const uint32_t* hit_read_id, const uint32_t* hit_loc, const uint32_t* hit_seed, uint32_t* out_idx, uint8_t* out_first,
                                 uint32_t* out_stale, void* temp, uint64_t temp_bytes, void* stream);

/* BowtieMapq2 / BowtieMapq3 (nvBowtie/bowtie2/cuda/mapq.h:42-330) for single-end reads:
 * out_mapq[r] from the best / second-best alignment of read r; perfect_score(len) = len * match,
 * min_score(len) = min_score_by_len[len] (the scheme's SimpleFunc tabulated by the host, scoring.h:272-281),
 * monotone = scheme.m_monotone (match bonus == 0).  Every read is evaluated, aligned or not, as the reference's MapqFunctorSE / PE
 * do: an unaligned read (Alignment::invalid(), score 2^17 - 1) gets the calculator's top no-second value and the reference's writers
 * zero it (output_sam.cpp:462).  version: 2 or 3. */
int nvbio_hip_mapq(int32_t version, int32_t match, int32_t monotone, const int32_t* min_score_by_len /* device */,
                   uint32_t n_reads, const uint64_t* best_alignments, uint32_t best_stride,
                   const uint32_t* read_len /* nullable */, uint32_t fixed_read_len, uint8_t* out_mapq, void* stream);

/* The same calculators over BestPairedAlignments(anchor pair, opposite pair) (mapq.h:56-58, 156-166): when the best alignment
 * is paired, scores and the score range are the sums over both mates (version 2) / the quality is 44 (version 3).  As for single-end
 * reads, an UNALIGNED mate is evaluated too and does not get 0 here (the reference's functors do the same; its writers print 0 for a read
 * they flag unmapped, output_sam.cpp:462): a consumer that wants "unaligned = 0" zeroes it itself, as this repository's SAM writers do
 * (include/nvbio_hip/sam.h, tools/align_fastq.py; tests/test_io_formats.py checks the records of unaligned reads). */
int nvbio_hip_mapq_paired(int32_t version, int32_t match, int32_t monotone, const int32_t* min_score_by_len /* device */,
                          uint32_t n_reads, const uint64_t* best_alignments, const uint64_t* best_alignments_o, uint32_t best_stride,
                          const uint32_t* read_len /* nullable */, const uint32_t* o_read_len /* nullable */,
                          uint32_t fixed_read_len, uint32_t o_fixed_read_len, uint8_t* out_mapq, void* stream);

/* Replaces nvbio::locate(fmi, i) (fmindex_inl.h:466-501) and nvBowtie's
 * locate_kernel (nvBowtie/bowtie2/cuda/locate_inl.h:122-148). */
int nvbio_hip_fm_locate(const nvbio_hip_fmindex* fmi, const uint32_t* sa_rows,
                        uint32_t n, uint32_t* out_pos, void* stream);

/* Two-pass form: locate_ssa_iterator / lookup_ssa_iterator (fmindex_inl.h:511-569;
 * nvBowtie locate_init_kernel / locate_lookup_kernel, locate_inl.h:153-208).
 * out_it / it are uint2 arrays {sampled row, steps}. */
int nvbio_hip_fm_locate_ssa_iterator(const nvbio_hip_fmindex* fmi, const uint32_t* sa_rows,
                                     uint32_t n, uint32_t* out_it, void* stream);
int nvbio_hip_fm_lookup_ssa_iterator(const nvbio_hip_fmindex* fmi, const uint32_t* it,
                                     uint32_t n, uint32_t* out_pos, void* stream);

/* Replaces FMIndexFilter<device_tag,fm_index>::rank(index, string_set)
 * (nvbio/fmindex/filter.h:139-170, filter_inl.h:268-300): out_range = match of
 * every seed, out_slots = inclusive scan of the range sizes (uint64).
 * temp: device scratch of nvbio_hip_fm_filter_temp_bytes(n) bytes.
 * The total number of hits is out_slots[n-1] (left on the device). */
uint64_t nvbio_hip_fm_filter_temp_bytes(uint32_t n);
int nvbio_hip_fm_filter_rank(const nvbio_hip_fmindex* fmi, const nvbio_hip_string_set* seeds,
                             uint32_t n, uint32_t* out_range, uint64_t* out_slots,
                             void* temp, uint64_t temp_bytes, void* stream);

/* Replaces FMIndexFilter<device_tag,fm_index>::locate(begin, end, hits)
 * (filter_inl.h:306-402): hits[2(h-begin)..] = {text position, seed id} for the
 * global hit indices h in [begin,end). */
int nvbio_hip_fm_filter_locate(const nvbio_hip_fmindex* fmi, const uint32_t* range, const uint64_t* slots,
                               uint32_t n_queries, uint64_t begin, uint64_t end,
                               uint32_t* out_hits, void* stream);

/* ---- Bidirectional search and maximal exact matches (nvbio/fmindex/bidir.h, mem.h).  f_fmi indexes the text, r_fmi the reversed
 * text; both must have the same length.  Only the reference-layout bwt_occ records are read: an index with dimer / ktab attached
 * gives the same results.
 *
 * Replaces extend_forward / extend_backwards (bidir_inl.h:48-144), batched: job i holds the forward range f_ranges[2i..] of a string
 * P and the range r_ranges[2i..] of P reversed in r_fmi; the outputs are the two ranges of P c[i] (NVBIO_HIP_EXTEND_FORWARD) or of
 * c[i] P (NVBIO_HIP_EXTEND_BACKWARDS).  The ranges of the empty string are (0, length).  Unlike the reference's, the ranges count
 * the row of the suffix that is P itself, so they equal what nvbio_hip_fm_match returns for the extended string.
 * A symbol > 3 gives (1, 0) for both. */
#define NVBIO_HIP_EXTEND_FORWARD   0
#define NVBIO_HIP_EXTEND_BACKWARDS 1
int nvbio_hip_fm_extend(int32_t direction, const nvbio_hip_fmindex* f_fmi, const nvbio_hip_fmindex* r_fmi,
                        const uint32_t* f_ranges, const uint32_t* r_ranges, const uint8_t* c, uint32_t n,
                        uint32_t* out_f_ranges, uint32_t* out_r_ranges, void* stream);

/* Replaces MEMFilter<device_tag,fm_index>::rank (mem.h:378-449, mem_inl.h:36-171).  For every string P (2- or 4-bit symbols;
 * symbols > 3 match nothing) and k = min_intv >= 1: ell(p) is the largest l such that P[p, p+l) holds no symbol > 3 and occurs at
 * least k times; the k-SMEMs are the spans [p, p + ell(p)) with ell(p) >= 1 that end past the span of p - 1.  One is reported iff
 * end - begin >= min_span and its SA range holds at most max_intv rows.  Reported MEMs are ordered by string, then by begin.
 *   out_ranges   4 words per MEM: {sa_begin, sa_end, string_id, begin | end << 16}, the inclusive range of P[begin, end) in f_fmi
 *   out_index    n + 1 words (uint64): the first MEM of every string, out_index[n] = the number of MEMs
 *   out_slots    inclusive scan of the range sizes of the stored MEMs (uint64)
 *   out_n_ranges HOST word: the number of MEMs found, whatever the capacity; the call synchronises the stream to learn it
 * At most `capacity` MEMs are stored (the sum of the string lengths always suffices); when more were found nothing is written past
 * it, *out_n_ranges still holds the true number and the call returns NVBIO_HIP_ERROR_CAPACITY: call again with that much room.
 * No string may be longer than max_pattern_len <= 65535, and n < 2^31: hipErrorInvalidValue (for a length array that holds a longer
 * string, after the first pass; nothing is stored then and *out_n_ranges is 0).
 * temp: device scratch of nvbio_hip_fm_mem_temp_bytes(n, max_pattern_len) bytes.  Nearly all of it holds the right ranges a lane keeps
 * while it walks: 12 * max_pattern_len bytes for each of min(n rounded up to 256, 524288) lanes in flight, whatever the strings'
 * actual lengths -- 0.95 GB at 150 symbols, 6 GB per 100 k strings of 5 000, and beyond a device's memory for a full grid near the
 * 65 535 limit.  The size is not negotiable per call: to spend less, rank a long-pattern set in batches of fewer strings. */
#define NVBIO_HIP_ERROR_CAPACITY 0x10001     /* outside hipError_t's values: never a code of the runtime's */
uint64_t nvbio_hip_fm_mem_temp_bytes(uint32_t n, uint32_t max_pattern_len);
int nvbio_hip_fm_mem_rank(const nvbio_hip_fmindex* f_fmi, const nvbio_hip_fmindex* r_fmi, const nvbio_hip_string_set* strings,
                          uint32_t n, uint32_t max_pattern_len, uint32_t min_intv, uint32_t max_intv, uint32_t min_span,
                          uint32_t* out_ranges, uint64_t capacity, uint64_t* out_index, uint64_t* out_slots, uint64_t* out_n_ranges,
                          void* temp, uint64_t temp_bytes, void* stream);

/* Replaces MEMFilter<device_tag,fm_index>::locate (mem_inl.h): out_hits[4(h-begin)..] = {text position, string id, begin, end} for
 * the global hit indices h in [begin,end) of the n_ranges stored MEMs. */
int nvbio_hip_fm_mem_locate(const nvbio_hip_fmindex* f_fmi, const uint32_t* ranges, const uint64_t* slots, uint64_t n_ranges,
                            uint64_t begin, uint64_t end, uint32_t* out_hits, void* stream);

/* Host twins of the three entries above: host pointers everywhere, OpenMP over the jobs, n_threads <= 0 = all.  The rank twin needs
 * no scratch; out_records, if not NULL, receives the number of 32-byte index records the walks read: per step one for each end of
 * the range that is a row of the BWT, one for both when they share a record -- what the device kernel loads. */
int nvbio_hip_fm_extend_host(int32_t direction, const nvbio_hip_fmindex* f_fmi, const nvbio_hip_fmindex* r_fmi,
                             const uint32_t* f_ranges, const uint32_t* r_ranges, const uint8_t* c, uint32_t n,
                             uint32_t* out_f_ranges, uint32_t* out_r_ranges, int32_t n_threads);
int nvbio_hip_fm_mem_rank_host(const nvbio_hip_fmindex* f_fmi, const nvbio_hip_fmindex* r_fmi, const nvbio_hip_string_set* strings,
                               uint32_t n, uint32_t max_pattern_len, uint32_t min_intv, uint32_t max_intv, uint32_t min_span,
                               uint32_t* out_ranges, uint64_t capacity, uint64_t* out_index, uint64_t* out_slots, uint64_t* out_n_ranges,
                               uint64_t* out_records, int32_t n_threads);
int nvbio_hip_fm_mem_locate_host(const nvbio_hip_fmindex* f_fmi, const uint32_t* ranges, const uint64_t* slots, uint64_t n_ranges,
                                 uint64_t begin, uint64_t end, uint32_t* out_hits, int32_t n_threads);

/* MEMFilter::rank with its last two arguments, split_len and split_width: BWA-MEM re-seeding over the contract above.
 * B = what nvbio_hip_fm_mem_rank reports for (min_intv, max_intv, min_span).  A MEM [b, e) of B with e - b >= split_len whose SA range
 * holds occ <= split_width rows is a candidate; its re-seeds are the (occ + 1)-SMEMs of the string that cover m = (b + e) >> 1
 * (begin <= m < end; they may reach outside [b, e)), kept iff end - begin >= min_span and at most max_intv rows.  Re-seeds are not split
 * again.  A string's output is B and the re-seeds of all its candidates, every span once, ordered by begin, then by end: begins can
 * repeat and ends are not monotone.  The split MEM stays (the reference replaces it).  Records, out_index and out_slots are as above,
 * and nvbio_hip_fm_mem_locate takes the result.
 * split_len == 0xFFFFFFFF: no re-seeding; the call IS nvbio_hip_fm_mem_rank, capacity protocol included.
 * Otherwise the sum of the string lengths no longer bounds the output, and the spans are staged in temp before duplicates go: the call
 * succeeds iff the number of spans found, a span counted once for every way it was found, is at most `capacity`; then *out_n_ranges is
 * the number stored.  If not, it returns NVBIO_HIP_ERROR_CAPACITY with that number in *out_n_ranges -- a capacity that suffices -- and
 * the contents of out_ranges, out_index and out_slots are unspecified; nothing is ever written past `capacity`.
 * temp: nvbio_hip_fm_mem_split_temp_bytes(n, max_pattern_len, capacity) bytes: twice the kept-range scratch of the plain entry (a
 * re-seed walks while its candidate's group is still being read) and 16 bytes per unit of capacity.
 * The host twin follows the same protocol, so the two agree in every word they return. */
uint64_t nvbio_hip_fm_mem_split_temp_bytes(uint32_t n, uint32_t max_pattern_len, uint64_t capacity);
int nvbio_hip_fm_mem_rank_split(const nvbio_hip_fmindex* f_fmi, const nvbio_hip_fmindex* r_fmi, const nvbio_hip_string_set* strings,
                                uint32_t n, uint32_t max_pattern_len, uint32_t min_intv, uint32_t max_intv, uint32_t min_span,
                                uint32_t split_len, uint32_t split_width,
                                uint32_t* out_ranges, uint64_t capacity, uint64_t* out_index, uint64_t* out_slots, uint64_t* out_n_ranges,
                                void* temp, uint64_t temp_bytes, void* stream);
int nvbio_hip_fm_mem_rank_split_host(const nvbio_hip_fmindex* f_fmi, const nvbio_hip_fmindex* r_fmi, const nvbio_hip_string_set* strings,
                                     uint32_t n, uint32_t max_pattern_len, uint32_t min_intv, uint32_t max_intv, uint32_t min_span,
                                     uint32_t split_len, uint32_t split_width,
                                     uint32_t* out_ranges, uint64_t capacity, uint64_t* out_index, uint64_t* out_slots, uint64_t* out_n_ranges,
                                     uint64_t* out_records, int32_t n_threads);

/* Replaces build_occurrence_table<2,64> (nvbio/fmindex/rank_dictionary_inl.h:42-77)
 * fused with the bwt|occ interleave of the loader (fmindex_impl.cu:305-327):
 * bwt_words = big-endian 2-bit BWT, 4*ceil(n/64) words (zero padded);
 * out_bwt_occ = 8*ceil(n/64) words; out_L2 = 5 device words.
 * temp: device scratch of nvbio_hip_build_bwt_occ_temp_bytes(n) bytes. */
uint64_t nvbio_hip_build_bwt_occ_temp_bytes(uint32_t n);
int nvbio_hip_build_bwt_occ(uint32_t n, const uint32_t* bwt_words, uint32_t* out_bwt_occ, uint32_t* out_L2,
                            void* temp, uint64_t temp_bytes, void* stream);

/* ---- Suffix sorting and BWT construction of one 2-bit text (nvbio/sufsort/sufsort.h: cuda::suffix_sort, cuda::bwt, cuda::find_primary
 * for a plain string).
 * words: the text, 2-bit packed in either PackedStream order (big_endian as in nvbio_hip_string_set), ceil(n / 16) words; bits must be 2;
 * 1 <= n <= 0xFFFFFFFE.  sa_out: uint32[n + 1] in the convention of compat/nvbio/fmindex/bwt.h: SA[0] = n is the empty suffix, and a
 * suffix that is a proper prefix of another sorts first.
 * nvbio_hip_bwt also writes what an FM-index is built from: bwt_words_out = the BWT with the '$' row dropped (bwt[row] = T[SA[row] - 1]),
 * big-endian 2-bit, 4 * ceil(n / 64) words, zero padded -- what nvbio_hip_build_bwt_occ takes; *primary_out (a HOST word) = the row whose
 * suffix is 0; ssa_out (may be NULL) = uint32[ceil((n + 1) / sa_int)], ssa[k] = SA[k * sa_int], ssa[0] = 0xFFFFFFFF; sa_out (may be NULL)
 * = the whole SA as above.
 * temp: device scratch of the matching _temp_bytes(n) bytes (36 bytes a symbol, 40 for nvbio_hip_bwt, plus rocPRIM's); nothing is
 * allocated inside.  Both entries wait for the stream once per sorting round -- the count of suffixes still unresolved has to reach the
 * host to end the loop -- and have finished when they return.  Invalid arguments (a null pointer, bits != 2, n == 0, n above the
 * maximum, too little temp) return hipErrorInvalidValue and launch nothing.
 * nvbio_hip_suffix_sort_last_rounds: the sorting rounds of this thread's last call, and in out_unresolved[r] (up to `capacity`; may be
 * NULL) the suffixes left unresolved after round r.
 * The host twins take host pointers and a thread count, and return the same bytes. */
uint64_t nvbio_hip_suffix_sort_temp_bytes(uint64_t n);
int nvbio_hip_suffix_sort(const uint32_t* words, uint32_t bits, uint32_t big_endian, uint64_t n, uint32_t* sa_out,
                          void* temp, uint64_t temp_bytes, void* stream);
uint32_t nvbio_hip_suffix_sort_last_rounds(uint64_t* out_unresolved, uint32_t capacity);
uint64_t nvbio_hip_bwt_temp_bytes(uint64_t n);
int nvbio_hip_bwt(const uint32_t* words, uint32_t bits, uint32_t big_endian, uint64_t n, uint32_t sa_int, uint32_t* bwt_words_out,
                  uint32_t* primary_out, uint32_t* ssa_out, uint32_t* sa_out, void* temp, uint64_t temp_bytes, void* stream);
int nvbio_hip_suffix_sort_host(const uint32_t* words, uint32_t bits, uint32_t big_endian, uint64_t n, uint32_t* sa_out, int32_t n_threads);
int nvbio_hip_bwt_host(const uint32_t* words, uint32_t bits, uint32_t big_endian, uint64_t n, uint32_t sa_int, uint32_t* bwt_words_out,
                       uint32_t* primary_out, uint32_t* ssa_out, uint32_t* sa_out, int32_t n_threads);

/* ---- Suffix sorting and BWT of a set of 2-bit strings (nvbio/sufsort/sufsort.h: cuda::suffix_sort(string_set, handler) and
 * cuda::bwt<SYMBOL_SIZE,BIG_ENDIAN>(ConcatenatedStringSet, handler), for a set that fits the device).
 * set: n_strings strings in any of the forms nvbio_hip_string_set allows (a length array, or fixed_length; begin offsets in any order,
 * at any position of a word, overlapping or not); bits must be 2.  The slots of the set are the pairs (s, p), 0 <= p <= length[s]: the
 * suffix of string s from symbol p on, the empty suffix p == length[s] included.  Slot (s, p) has the global suffix index
 * g = cum[s - 1] + p, where cum[s] = the inclusive sum of length + 1 and cum[-1] = 0; n_suffixes = cum[n_strings - 1] is passed by the
 * caller, whose buffers it sizes, and checked.  1 <= n_strings <= n_suffixes <= 0xFFFFFFFE.
 * Order: by the suffix's symbols, a suffix that is a proper prefix of another first ($ < A); equal suffixes by ascending string id.
 * Rows 0 .. n_strings - 1 are therefore the empty suffixes in id order.
 * nvbio_hip_set_suffix_sort: suffixes_out[row] = the global index on that row; string_ids_out[g] (may be NULL) = the string of global
 * index g; cum_lengths_out (may be NULL) = cum.
 * nvbio_hip_set_bwt: bwt_out[row] = symbol p - 1 of string s for the slot (s, p) on that row, 255 ('$') where p == 0; dollar_rows_out =
 * the n_strings rows that hold 255, ascending, dollar_ids_out = the string each of them starts; suffixes_out (may be NULL) = the pair
 * (p, s) of every row, the reference's uint2 (x = suffix, y = string).
 * temp: device scratch of the matching _temp_bytes(n_suffixes, n_strings) bytes; nothing is allocated inside.  Layout: the plain
 * sorter's seven arrays over n_suffixes (36 bytes a slot) | string_ids (4 bytes a slot) | cum as 64-bit sums (8 bytes a string) |
 * rocPRIM's scratch; nvbio_hip_set_bwt puts the sorted slots (4 bytes a slot) in front: 40 and 44 bytes a slot.
 * Both entries wait for the stream once per sorting round and have finished when they return.  A null pointer, bits != 2, a count out
 * of range or too little temp return hipErrorInvalidValue and launch nothing.  So does an n_suffixes that is not the sum of
 * fixed_length + 1; with a length array the sum is known on the device only: the first round runs inside the scratch, writes nothing
 * to the outputs unless the sum is n_suffixes, and its wait brings the sum to the host, where a wrong n_suffixes returns
 * hipErrorInvalidValue with the outputs untouched.  nvbio_hip_suffix_sort_last_rounds reports the rounds of a set call too.
 * The host twins take host pointers and a thread count, and return the same bytes; they take n_strings <= 0xFFFFFFFB (their first
 * ranks, n_strings + 1 + symbol, are 32-bit words) and return hipErrorInvalidValue above that. */
uint64_t nvbio_hip_set_suffix_sort_temp_bytes(uint64_t n_suffixes, uint32_t n_strings);
int nvbio_hip_set_suffix_sort(const nvbio_hip_string_set* set /* host struct, device arrays; bits must be 2 */,
                              uint32_t n_strings, uint64_t n_suffixes,
                              uint32_t* suffixes_out   /* [n_suffixes] global suffix indices in sorted order */,
                              uint32_t* string_ids_out /* [n_suffixes] string of global index g; may be NULL */,
                              uint32_t* cum_lengths_out/* [n_strings] inclusive sums of length + 1; may be NULL */,
                              void* temp, uint64_t temp_bytes, void* stream);
uint64_t nvbio_hip_set_bwt_temp_bytes(uint64_t n_suffixes, uint32_t n_strings);
int nvbio_hip_set_bwt(const nvbio_hip_string_set* set, uint32_t n_strings, uint64_t n_suffixes,
                      uint8_t*  bwt_out        /* [n_suffixes], 255 = '$' */,
                      uint32_t* dollar_rows_out/* [n_strings] */, uint32_t* dollar_ids_out /* [n_strings] */,
                      uint32_t* suffixes_out   /* [2 * n_suffixes]: (p, s) pairs in sorted order; may be NULL */,
                      void* temp, uint64_t temp_bytes, void* stream);
int nvbio_hip_set_suffix_sort_host(const nvbio_hip_string_set* set, uint32_t n_strings, uint64_t n_suffixes, uint32_t* suffixes_out,
                                   uint32_t* string_ids_out, uint32_t* cum_lengths_out, int32_t n_threads);
int nvbio_hip_set_bwt_host(const nvbio_hip_string_set* set, uint32_t n_strings, uint64_t n_suffixes, uint8_t* bwt_out,
                           uint32_t* dollar_rows_out, uint32_t* dollar_ids_out, uint32_t* suffixes_out, int32_t n_threads);

/* ---- Q-gram indices and the q-gram filter (nvbio/qgram/qgram.h: QGramIndexDevice, QGramSetIndexDevice, generate_qgrams;
 * nvbio/qgram/filter.h: QGramFilterDevice::rank / locate / merge).
 * Q-gram: over 2-bit symbols, 1 <= q <= 32, the q-gram at position i of a string of len symbols is the 64-bit word
 * sum_j sym(i + j) << 2j, j < q: the first symbol in the lowest bits, sym = 0 where i + j >= len (a truncated q-gram at the tail is
 * padded with A), and 0 where i >= len.  Q-grams are ordered as these integers, which is not the strings' lexicographic order.
 * Index: qgrams[n_unique] = the distinct q-grams, ascending; slots[n_unique + 1] = the exclusive sums of their counts,
 * slots[n_unique] = n_qgrams; index[n_qgrams] = the coordinates grouped by q-gram, inside one q-gram in enumeration order.  A string
 * index has one coordinate per position 0 .. len - 1 (the q - 1 truncated ones included), a uint32; a set index has the uint2
 * (string id, pos) for pos = 0, interval, .. while pos + q <= length[id], enumerated by string id and then by pos.  With QL = ql > 0,
 * lut[4^QL + 1]: lut[k] = the lower bound of k << 2 (q - QL) in qgrams, lut[4^QL] = n_unique.  0 <= ql <= min(q, 16).
 * Limits: bits == 2, n_words >= 1, at most 0xFFFFFFFF q-grams.  A violation, a null pointer or too little temp return
 * hipErrorInvalidValue and launch nothing.  Nothing is allocated inside: temp is device scratch of the matching _temp_bytes.
 * Scratch of a build over n q-grams of a set of N strings: keys A (8 n) | keys B (8 n) | coordinates in enumeration order (4 n; 8 n
 * for a set) | run counts (4 n) | the run count (256) | for a set, the 64-bit inclusive sums of the per-string seed counts (8 N) |
 * rocPRIM's; rank: rocPRIM's scan; merge: keys A | keys B (4 n each; 8 n for a set) | the run count (256) | rocPRIM's.
 * The builds, rank, merge and count_seeds with a length array wait for the stream (for n_unique, the total, n_merged, the count) and
 * have finished when they return; generate, range and locate are asynchronous. */
typedef struct nvbio_hip_qgram_index {
    const uint64_t* qgrams;     /* [n_unique] */
    const uint32_t* slots;      /* [n_unique + 1] */
    const uint32_t* index;      /* [n_qgrams] uint32, or [n_qgrams] uint2 for a set index */
    const uint32_t* lut;        /* [4^ql + 1], or NULL when ql == 0 */
    uint32_t        q, ql;
    uint32_t        n_unique, n_qgrams;
} nvbio_hip_qgram_index;

/* qgrams_out[i] = the q-gram at positions[i] of the string of len symbols that starts at symbol 0 of words; positions == NULL means
 * position i.  The set form takes n (string id, pos) pairs; an id >= n_strings gives 0. */
int nvbio_hip_qgram_generate(const uint32_t* words, uint64_t n_words, uint32_t bits, uint32_t big_endian, uint64_t len, uint32_t q,
                             const uint32_t* positions /* [n] or NULL */, uint64_t n, uint64_t* qgrams_out /* [n] */, void* stream);
int nvbio_hip_qgram_set_generate(const nvbio_hip_string_set* set, uint32_t n_strings, uint32_t q, const uint32_t* coords /* [2 n] */, uint64_t n,
                                 uint64_t* qgrams_out /* [n] */, void* stream);
uint64_t nvbio_hip_qgram_index_build_temp_bytes(uint64_t len);
int nvbio_hip_qgram_index_build(const uint32_t* words, uint64_t n_words, uint32_t bits, uint32_t big_endian, uint64_t len, uint32_t q, uint32_t ql,
                                uint64_t* qgrams_out /* [len] */, uint32_t* slots_out /* [len + 1] */, uint32_t* index_out /* [len] */,
                                uint32_t* lut_out /* [4^ql + 1]; NULL when ql == 0 */, uint32_t* n_unique_out /* host */,
                                void* temp, uint64_t temp_bytes, void* stream);
/* *n_qgrams_out (host) = the seeds of uniform_seeds_functor(q, interval) over the set; with fixed_length nothing is launched and temp
 * may be NULL. */
uint64_t nvbio_hip_qgram_set_count_seeds_temp_bytes(uint32_t n_strings);
int nvbio_hip_qgram_set_count_seeds(const nvbio_hip_string_set* set, uint32_t n_strings, uint32_t q, uint32_t interval, uint64_t* n_qgrams_out,
                                    void* temp, uint64_t temp_bytes, void* stream);
/* n_qgrams: the seed count the caller sized the buffers for; it is checked before anything but the scratch is written, and a wrong one
 * returns hipErrorInvalidValue.  index_out holds uint2 (string id, pos). */
uint64_t nvbio_hip_qgram_set_index_build_temp_bytes(uint64_t n_qgrams, uint32_t n_strings);
int nvbio_hip_qgram_set_index_build(const nvbio_hip_string_set* set, uint32_t n_strings, uint32_t q, uint32_t interval, uint32_t ql, uint64_t n_qgrams,
                                    uint64_t* qgrams_out /* [n_qgrams] */, uint32_t* slots_out /* [n_qgrams + 1] */, uint32_t* index_out /* [2 n_qgrams] */,
                                    uint32_t* lut_out, uint32_t* n_unique_out /* host */, void* temp, uint64_t temp_bytes, void* stream);
/* ranges_out[i] = the uint2 (slots[k], slots[k + 1]) of queries[i] = qgrams[k], (0, 0) where the q-gram is not in the index: the LUT
 * bucket if there is one, a lower bound inside it, two slot reads.  index->index is not read. */
int nvbio_hip_qgram_range(const nvbio_hip_qgram_index* index, const uint64_t* queries, uint64_t n_queries, uint32_t* ranges_out /* [2 n] */, void* stream);
/* the filter's rank: the ranges, slots_out = the inclusive 64-bit sums of their sizes, *total_out (host) = the last sum, 0 for no
 * queries */
uint64_t nvbio_hip_qgram_rank_temp_bytes(uint64_t n_queries);
int nvbio_hip_qgram_rank(const nvbio_hip_qgram_index* index, const uint64_t* queries, uint64_t n_queries, uint32_t* ranges_out /* [2 n] */,
                         uint64_t* slots_out /* [n] */, uint64_t* total_out, void* temp, uint64_t temp_bytes, void* stream);
/* the filter's locate over the outputs [begin, end): for output o, slot = the upper bound of o in slots, local = o - slots[slot - 1]
 * (64 bits), hit = (index[ranges[slot].x + local], indices[slot]): a uint2 (qgram pos, query idx) for a string index, a uint4
 * (string id, pos, query idx, 0) for a set index.  An output at or past the total gives a zero hit. */
int nvbio_hip_qgram_locate(const nvbio_hip_qgram_index* index, uint32_t n_queries, const uint32_t* ranges, const uint64_t* slots,
                           const uint32_t* indices /* [n_queries] */, uint64_t begin, uint64_t end, uint32_t* hits_out /* [2 (end - begin)] */, void* stream);
int nvbio_hip_qgram_set_locate(const nvbio_hip_qgram_index* index, uint32_t n_queries, const uint32_t* ranges, const uint64_t* slots,
                               const uint32_t* indices, uint64_t begin, uint64_t end, uint32_t* hits_out /* [4 (end - begin)] */, void* stream);
/* the filter's merge: diag = query idx - index pos in wrapping uint32, snapped as the reference's util::round(diag, interval) does it:
 * r = (diag / interval) * interval, and r + 1 (one, not interval) where uint32((diag - r) * 2) > interval.  The key of a string hit is
 * that word; of a set hit the uint2 (snapped diag, string id), ordered with the string id in the high half.  merged_out = the distinct
 * keys ascending, counts_out their counts, *n_merged_out (host) their number.  interval >= 1. */
uint64_t nvbio_hip_qgram_merge_temp_bytes(uint32_t n_hits);
int nvbio_hip_qgram_merge(const uint32_t* hits /* [2 n_hits] */, uint32_t n_hits, uint32_t interval, uint32_t* merged_out /* [n_hits] */,
                          uint32_t* counts_out /* [n_hits] */, uint32_t* n_merged_out, void* temp, uint64_t temp_bytes, void* stream);
uint64_t nvbio_hip_qgram_set_merge_temp_bytes(uint32_t n_hits);
int nvbio_hip_qgram_set_merge(const uint32_t* hits /* [4 n_hits] */, uint32_t n_hits, uint32_t interval, uint32_t* merged_out /* [2 n_hits] */,
                              uint32_t* counts_out /* [n_hits] */, uint32_t* n_merged_out, void* temp, uint64_t temp_bytes, void* stream);
/* The host twins: host pointers everywhere, a thread count instead of scratch and stream, the same bytes. */
int nvbio_hip_qgram_generate_host(const uint32_t* words, uint64_t n_words, uint32_t bits, uint32_t big_endian, uint64_t len, uint32_t q,
                                  const uint32_t* positions, uint64_t n, uint64_t* qgrams_out, int32_t n_threads);
int nvbio_hip_qgram_set_generate_host(const nvbio_hip_string_set* set, uint32_t n_strings, uint32_t q, const uint32_t* coords, uint64_t n,
                                      uint64_t* qgrams_out, int32_t n_threads);
int nvbio_hip_qgram_index_build_host(const uint32_t* words, uint64_t n_words, uint32_t bits, uint32_t big_endian, uint64_t len, uint32_t q, uint32_t ql,
                                     uint64_t* qgrams_out, uint32_t* slots_out, uint32_t* index_out, uint32_t* lut_out, uint32_t* n_unique_out,
                                     int32_t n_threads);
int nvbio_hip_qgram_set_count_seeds_host(const nvbio_hip_string_set* set, uint32_t n_strings, uint32_t q, uint32_t interval, uint64_t* n_qgrams_out,
                                         int32_t n_threads);
int nvbio_hip_qgram_set_index_build_host(const nvbio_hip_string_set* set, uint32_t n_strings, uint32_t q, uint32_t interval, uint32_t ql, uint64_t n_qgrams,
                                         uint64_t* qgrams_out, uint32_t* slots_out, uint32_t* index_out, uint32_t* lut_out, uint32_t* n_unique_out,
                                         int32_t n_threads);
int nvbio_hip_qgram_range_host(const nvbio_hip_qgram_index* index, const uint64_t* queries, uint64_t n_queries, uint32_t* ranges_out, int32_t n_threads);
int nvbio_hip_qgram_rank_host(const nvbio_hip_qgram_index* index, const uint64_t* queries, uint64_t n_queries, uint32_t* ranges_out,
                              uint64_t* slots_out, uint64_t* total_out, int32_t n_threads);
int nvbio_hip_qgram_locate_host(const nvbio_hip_qgram_index* index, uint32_t n_queries, const uint32_t* ranges, const uint64_t* slots,
                                const uint32_t* indices, uint64_t begin, uint64_t end, uint32_t* hits_out, int32_t n_threads);
int nvbio_hip_qgram_set_locate_host(const nvbio_hip_qgram_index* index, uint32_t n_queries, const uint32_t* ranges, const uint64_t* slots,
                                    const uint32_t* indices, uint64_t begin, uint64_t end, uint32_t* hits_out, int32_t n_threads);
int nvbio_hip_qgram_merge_host(const uint32_t* hits, uint32_t n_hits, uint32_t interval, uint32_t* merged_out, uint32_t* counts_out,
                               uint32_t* n_merged_out, int32_t n_threads);
int nvbio_hip_qgram_set_merge_host(const uint32_t* hits, uint32_t n_hits, uint32_t interval, uint32_t* merged_out, uint32_t* counts_out,
                                   uint32_t* n_merged_out, int32_t n_threads);

/* ---- Byte alphabets: suffix sort and BWT of a byte text, the wavelet tree, and an FM-index over the wavelet tree of a BWT
 * (nvbio/strings/wavelet_tree.h; fm_index<WaveletTree, ..> of nvbio/fmindex/fmindex.h).
 * A byte text holds one symbol per byte, 1 <= symbol_size <= 8 bits of it: every symbol is read as byte & (2^symbol_size - 1), so no
 * input byte can index outside the alphabet.
 *
 * nvbio_hip_suffix_sort_bytes / nvbio_hip_bwt_bytes: nvbio_hip_suffix_sort / nvbio_hip_bwt for such a text, 1 <= n <= 0xFFFFFFFE, with
 * the same conventions (SA[0] = n, a proper prefix first, primary, ssa[k] = SA[k * sa_int] with ssa[0] = 0xFFFFFFFF), the same scratch
 * and waits, the rounds reported by nvbio_hip_suffix_sort_last_rounds; bwt_out = the n BWT symbols, one byte each, the '$' row dropped.
 * A null pointer, symbol_size 0 or above 8, n == 0 or above the maximum, or too little temp return hipErrorInvalidValue and launch
 * nothing.
 *
 * The wavelet tree of n symbols, S = symbol_size, K = 2^S, W = ceil(n S / 32), n S <= 0xFFFFFFFF; the reference's layout bit for bit:
 *   bits[W]     a big-endian 1-bit stream: global bit g is bit 31 - g % 32 of word g / 32, zero padded.  Level l is bits
 *               [l n, (l + 1) n): bit S - 1 - l of the symbols after a stable sort by their top l bits.
 *   splits[K]   a heap of internal nodes: node j of level l has index 2^l - 1 + j and covers the symbols [j K / 2^l, (j + 1) K / 2^l);
 *               splits[node] = the text symbols smaller than the node's middle symbol; splits[K - 1] = 0.
 *   occ[K + W]  occ[node] = the 1 bits of the stream before bit l n + (the text symbols smaller than the node's first symbol),
 *               occ[K - 1] = 0; occ[K + w] = the 1 bits before word w.
 * nvbio_hip_wavelet_setup is asynchronous (no wait); temp: device scratch of nvbio_hip_wavelet_setup_temp_bytes (a 256-bin histogram
 * | n bytes of sorted symbols | rocPRIM's).
 * nvbio_hip_wavelet_text: out[i] = the symbol at positions[i] (positions == NULL: at i); a position >= n gives 0 without a read.
 * nvbio_hip_wavelet_rank: out[i] = the occurrences of symbols[i] & (K - 1) in [0, positions[i]]; a position in [n, 0xFFFFFFFE] counts as
 * n - 1 (the reference's clamp), 0xFFFFFFFF gives 0.  nvbio_hip_wavelet_rank_range: the same for both ends (x, y) of n_queries ranges.
 * n_queries <= 0xFFFFFFFF.  The queries are asynchronous.
 *
 * The FM-index: bwt = the tree of the n BWT symbols ('$' dropped), L2[K + 1] with L2[0] = 0 and L2[c + 1] = L2[c] + count(c)
 * (nvbio_hip_wavelet_fm_L2 reads it off the tree), ssa as nvbio_hip_bwt_bytes writes it for sa_int (any value >= 1), primary, and
 * length == bwt.size.
 * nvbio_hip_wavelet_fm_match: the reference's backward search from (0, n): x = L2[c] + rank(x - 1, c) + 1, y = L2[c] + rank(y, c) while
 * x <= y, over the pattern's symbols from the last to the first; an empty pattern gives (0, n).  A pattern symbol >= K ends the search
 * with (1, 0): pattern symbols are the one read that is not masked (the reference tests c > K, which lets c == K through to a rank of
 * symbol 0).  A pattern is clipped to the n_symbols the set declares.
 * nvbio_hip_wavelet_fm_locate: positions_out[i] = SA[rows[i]] by LF steps to a sampled row; row 0 gives ssa[0] = 0xFFFFFFFF, what
 * nvbio_hip_fm_locate gives for it; a row above n gives 0xFFFFFFFF without a read.  ssa == NULL or sa_int == 0 is refused.
 * A null pointer, a tree or index outside the limits above (primary must be in [1, length]) return hipErrorInvalidValue and launch nothing.
 * The host twins take host pointers and a thread count, and return the same bytes.  The query twins run their queries on n_threads
 * threads; nvbio_hip_wavelet_setup_host and nvbio_hip_wavelet_fm_L2_host are serial whatever n_threads says (the setup is the
 * definition itself: a stable sort of the symbols per level and a bit-by-bit fill, O(S n log n)). */
typedef struct nvbio_hip_wavelet_tree {
    const uint32_t* bits;       /* [W] */
    const uint32_t* splits;     /* [K] */
    const uint32_t* occ;        /* [K + W] */
    uint32_t        symbol_size, size;
} nvbio_hip_wavelet_tree;
typedef struct nvbio_hip_byte_string_set {
    const uint8_t*  symbols;    /* one symbol per byte */
    uint64_t        n_symbols;
    const uint64_t* begin;      /* [n] first symbol of each string */
    const uint32_t* length;     /* [n], or NULL -> fixed_length */
    uint32_t        fixed_length, _pad;
} nvbio_hip_byte_string_set;
typedef struct nvbio_hip_wavelet_fmindex {
    nvbio_hip_wavelet_tree bwt; /* over the n BWT symbols, '$' dropped */
    const uint32_t* L2;         /* [K + 1] */
    const uint32_t* ssa;        /* may be NULL: then locate is refused */
    uint32_t        length, primary, sa_int, _pad;
} nvbio_hip_wavelet_fmindex;
uint64_t nvbio_hip_suffix_sort_bytes_temp_bytes(uint64_t n);
int nvbio_hip_suffix_sort_bytes(const uint8_t* symbols, uint32_t symbol_size, uint64_t n, uint32_t* sa_out /* [n + 1] */,
                                void* temp, uint64_t temp_bytes, void* stream);
uint64_t nvbio_hip_bwt_bytes_temp_bytes(uint64_t n);
int nvbio_hip_bwt_bytes(const uint8_t* symbols, uint32_t symbol_size, uint64_t n, uint32_t sa_int, uint8_t* bwt_out /* [n] */,
                        uint32_t* primary_out /* host */, uint32_t* ssa_out /* may be NULL */, uint32_t* sa_out /* may be NULL */,
                        void* temp, uint64_t temp_bytes, void* stream);
int nvbio_hip_suffix_sort_bytes_host(const uint8_t* symbols, uint32_t symbol_size, uint64_t n, uint32_t* sa_out, int32_t n_threads);
int nvbio_hip_bwt_bytes_host(const uint8_t* symbols, uint32_t symbol_size, uint64_t n, uint32_t sa_int, uint8_t* bwt_out, uint32_t* primary_out,
                             uint32_t* ssa_out, uint32_t* sa_out, int32_t n_threads);
uint64_t nvbio_hip_wavelet_setup_temp_bytes(uint64_t n, uint32_t symbol_size);
int nvbio_hip_wavelet_setup(const uint8_t* symbols, uint32_t symbol_size, uint64_t n, uint32_t* bits_out /* [W] */, uint32_t* splits_out /* [K] */,
                            uint32_t* occ_out /* [K + W] */, void* temp, uint64_t temp_bytes, void* stream);
int nvbio_hip_wavelet_text(const nvbio_hip_wavelet_tree* tree, const uint32_t* positions /* [n] or NULL */, uint64_t n_queries, uint8_t* out, void* stream);
int nvbio_hip_wavelet_rank(const nvbio_hip_wavelet_tree* tree, const uint32_t* positions, const uint8_t* symbols, uint64_t n_queries, uint32_t* out, void* stream);
int nvbio_hip_wavelet_rank_range(const nvbio_hip_wavelet_tree* tree, const uint32_t* ranges /* [2 n] */, const uint8_t* symbols, uint64_t n_queries,
                                 uint32_t* out /* [2 n] */, void* stream);
int nvbio_hip_wavelet_fm_L2(const nvbio_hip_wavelet_tree* tree, uint32_t* L2_out /* [K + 1] */, void* stream);
int nvbio_hip_wavelet_fm_match(const nvbio_hip_wavelet_fmindex* fmi, const nvbio_hip_byte_string_set* patterns /* host struct, device arrays */, uint64_t n,
                               uint32_t* ranges_out /* [2 n] */, void* stream);
int nvbio_hip_wavelet_fm_locate(const nvbio_hip_wavelet_fmindex* fmi, const uint32_t* rows, uint64_t n_rows, uint32_t* positions_out, void* stream);
int nvbio_hip_wavelet_setup_host(const uint8_t* symbols, uint32_t symbol_size, uint64_t n, uint32_t* bits_out, uint32_t* splits_out, uint32_t* occ_out,
                                 int32_t n_threads);
int nvbio_hip_wavelet_text_host(const nvbio_hip_wavelet_tree* tree, const uint32_t* positions, uint64_t n_queries, uint8_t* out, int32_t n_threads);
int nvbio_hip_wavelet_rank_host(const nvbio_hip_wavelet_tree* tree, const uint32_t* positions, const uint8_t* symbols, uint64_t n_queries, uint32_t* out,
                                int32_t n_threads);
int nvbio_hip_wavelet_rank_range_host(const nvbio_hip_wavelet_tree* tree, const uint32_t* ranges, const uint8_t* symbols, uint64_t n_queries, uint32_t* out,
                                      int32_t n_threads);
int nvbio_hip_wavelet_fm_L2_host(const nvbio_hip_wavelet_tree* tree, uint32_t* L2_out, int32_t n_threads);
int nvbio_hip_wavelet_fm_match_host(const nvbio_hip_wavelet_fmindex* fmi, const nvbio_hip_byte_string_set* patterns, uint64_t n, uint32_t* ranges_out,
                                    int32_t n_threads);
int nvbio_hip_wavelet_fm_locate_host(const nvbio_hip_wavelet_fmindex* fmi, const uint32_t* rows, uint64_t n_rows, uint32_t* positions_out, int32_t n_threads);

/* Device-memory helpers for host code that has no HIP headers (the C++ host layer in
 * include/nvbio_hip/ uses them where the reference uses thrust::device_vector).
 * kind: 1 = host->device, 2 = device->host, 3 = device->device. */
int nvbio_hip_device_malloc(void** ptr, uint64_t bytes);
int nvbio_hip_device_free(void* ptr);             /* hipFree's contract: waits for the device */
int nvbio_hip_device_free_ordered(void* ptr);     /* opt-in, does not stop the host: see "Memory helpers" below */
int nvbio_hip_device_free_after(void* ptr, void* stream);   /* the same, for a block whose work was queued on `stream` (any stream of the caller's) */
int nvbio_hip_device_trim(void);                  /* hipFree every idle block of this device's cache */
int nvbio_hip_device_mem_info(uint64_t* free_bytes, uint64_t* total_bytes, uint64_t* idle_cached_bytes);
int nvbio_hip_memcpy(void* dst, const void* src, uint64_t bytes, int kind, void* stream);
int nvbio_hip_memset(void* dst, int value, uint64_t bytes, void* stream);
int nvbio_hip_stream_synchronize(void* stream);
int nvbio_hip_stream_query(void* stream);         /* hipStreamQuery: 0 = everything queued so far has finished, 600 (hipErrorNotReady) = not yet */
/* Pinned host memory the device writes to through the same pointer (hipHostMalloc): where a kernel leaves the few words its host thread is
 * waiting for -- the sizes of a selection round's queues (include/nvbio_hip/select.h) -- so that the thread reads them as they land instead of
 * going through a stream synchronisation and a copy per round. */
int nvbio_hip_host_malloc(void** ptr, uint64_t bytes);
int nvbio_hip_host_free(void* ptr);

/* Streams.  The reference runs one host thread per device on its default stream (nvBowtie.cpp:809-864, compute_thread.cu:74-117).
 * Every nvbio_hip_* entry takes the stream its work is queued on, so a driver object per host thread, each on its own non-blocking
 * stream, keeps several batches in flight on one device: one batch's fabric-bound seeding (map / locate: random 128-byte lines, idle
 * VALUs) overlaps another's VALU-bound extension / selection / traceback (+7-10 % measured, profiles/r03/cosched_two_streams.txt).
 * (Round 3 also exported a CU-masked stream, a grid cap for the seeding kernels and a seeding token; none of them beat two plain
 * streams in any measured configuration -- a saturated fabric taxes co-resident VALU kernels whichever CUs they sit on,
 * profiles/r03/cosched_cu_mask.txt, cosched_token_grid_limit.txt -- and they were removed.)  Results never depend on any of this. */
int nvbio_hip_stream_create(void** stream, uint32_t non_blocking);
int nvbio_hip_stream_destroy(void* stream);

/* Multi-GPU.  The reference runs one host thread per device over a replicated index, all writing into one shared
 * output (nvBowtie/nvBowtie.cpp:809-864, bowtie2/cuda/compute_thread.cu:74-117): no collective.  Here every device aligns a contiguous
 * block of the reads and the fixed-size result records (16 B per read, 32 B per pair; 4-12 B for the extension stage alone) are gathered
 * to one rank over RCCL / xGMI with grouped ncclSend / ncclRecv -- the ONLY collective of the path.  RCCL is bound at run time (dlopen);
 * nvbio_hip_comm_available() = 0 means it could not be, and the comm entries return hipErrorNotSupported (801).
 *   one process, one host thread per device:  nvbio_hip_comm_init_all(comms, n, devices)   (ncclCommInitAll)
 *   one process per device (a launcher):      rank 0 makes nvbio_hip_comm_unique_id(id), the launcher ships the 128 bytes to every rank,
 *                                             each rank calls nvbio_hip_comm_init_rank(&comm, world, rank, id) on its own device
 * nvbio_hip_gather_records: counts[r] records of record_bytes bytes from rank r (all ranks pass the same counts); the root's recv holds
 * them in rank order.  Device buffers, queued on `stream`.  RCCL failures are returned as 2000 + ncclResult_t. */
int nvbio_hip_comm_available(void);
int nvbio_hip_device_count(void);
int nvbio_hip_set_device(int device);
int nvbio_hip_get_device(void);
int nvbio_hip_comm_unique_id(uint8_t* id128);
int nvbio_hip_comm_init_rank(void** comm, int world, int rank, const uint8_t* id128);
int nvbio_hip_comm_init_all(void** comms, int n_devices, const int* devices /* nullable: 0..n-1 */);
int nvbio_hip_comm_destroy(void* comm);
int nvbio_hip_comm_rank(void* comm, int* rank, int* world);
int nvbio_hip_gather_records(void* comm, const void* send, const uint64_t* counts, uint32_t record_bytes, void* recv /* root only */, int root, void* stream);
/* after a local failure: unblock the peers waiting on this communicator (ncclCommAbort); it is unusable afterwards */
int nvbio_hip_comm_abort(void* comm);
/* The transport seam under nvbio_hip_gather_records.  The gather is a plan of sends / receives / one copy (nvbio_hip/gather_plan.h)
 * executed through these five operations; the default table is RCCL.  Installing another table (NULL restores RCCL) lets the CPU suite
 * run the plan over host memory at worlds of 2..8, and lets a deployment without RCCL keep the entry point.  `comm` is whatever the
 * table's owner made it; every function returns 0 or an error code. */
typedef struct nvbio_hip_comm_transport {
    int (*rank)(void* comm, int* rank, int* world);
    int (*group_start)(void* comm);
    int (*group_end)(void* comm);
    int (*send)(void* comm, const void* buf, uint64_t bytes, int peer, void* stream);
    int (*recv)(void* comm, void* buf, uint64_t bytes, int peer, void* stream);
    int (*copy)(void* comm, void* dst, const void* src, uint64_t bytes, void* stream);
    int (*abort)(void* comm);
} nvbio_hip_comm_transport;
void nvbio_hip_comm_set_transport(const nvbio_hip_comm_transport* transport);

/* Test switches.  A few named integers select alternative executions of the same results, for the parity suite to cover both
 * (NVBIO_HIP_FORCE_32BIT, NVBIO_HIP_NO_STAGING, NVBIO_HIP_FULL_GENERIC, NVBIO_HIP_FULL_SINGLE_JOB, NVBIO_HIP_FULL_ROWS, NVBIO_HIP_ED_SWEEP,
 * NVBIO_HIP_SELECT_LANES, NVBIO_HIP_TRACEBACK_LANES, NVBIO_HIP_BANDED_PAIR, NVBIO_HIP_PAIR_ROW, NVBIO_HIP_PAIR_CONST, NVBIO_HIP_PAIR_SUB, NVBIO_HIP_WAVELET_LANES).  Each is seeded ONCE per process from the environment variable of the same name and
 * changed afterwards only through nvbio_hip_set_test_switch (atomic; safe while other threads are inside library calls -- a call in flight
 * uses the value it read when it started).  0 = the default execution.  Production code leaves them alone. */
int nvbio_hip_set_test_switch(const char* name, int value);     /* hipErrorInvalidValue for an unknown name */
int nvbio_hip_get_test_switch(const char* name);                /* -1 for an unknown name */
const char* nvbio_hip_test_switch_name(int index);              /* the index-th switch's name, NULL past the last: how a binding enumerates them */
/* Memory helpers: nvbio_hip_device_malloc / nvbio_hip_device_free hand out hipMalloc'ed blocks kept in a per-device cache of the library's own
 * (a freed block is listed and reused for a request of at least half its size; up to NVBIO_HIP_POOL_KEEP_MB = 2048 MB stay listed;
 * nvbio_hip_device_trim hands the idle ones back, nvbio_hip_device_mem_info says how much is idle).  Not a hipMemPool: under two host threads
 * on one device -- the reference's nvBowtie --device 0 --device 0 -- ROCm 7.0's pool loses the contents of live blocks
 * (profiles/r05/two_threads_pool.txt).
 *   nvbio_hip_device_free          hipFree's contract (the reference's cudaFree): the device is idle before the block can change hands, whatever
 *                                  stream used it -- the caller's own non-blocking streams and torch's pool streams included.  What
 *                                  nvbio::vector<device_tag> / device_buffer of the drop-in layer call.
 *   nvbio_hip_device_free_ordered  opt-in, does not stop the host.  The caller vouches that all work on the block was queued, before the call, on the
 *                                  default stream, a blocking stream or a stream made by nvbio_hip_stream_create: the default stream is put
 *                                  behind what each of the latter holds now (hipStreamWaitEvent), and nvbio_hip_device_malloc returns after
 *                                  the default stream has drained, so the next owner never overlaps the previous one's work, whichever thread
 *                                  it is.  What this repository's C++ host layer uses (include/nvbio_hip/types.h).
 *   nvbio_hip_device_free_after    the ordered form for a block all of whose work was queued on ONE known stream of the caller's (registered or not):
 *                                  the default stream is put behind that stream too.  What a batch object's scratch (device_buffer, compat
 *                                  alignment/batched.h) uses: it dies right after enact(stream) returns, with its kernels still queued there.
 * Call them from a thread bound to the device the block lives on; per-batch storage lives in a hip::device_arena and comes through here once. */

/* Library / device introspection (host). */
int         nvbio_hip_abi_version(void);
const char* nvbio_hip_arch(void);           /* "gfx950" */
const char* nvbio_hip_last_kernel(void);    /* name of the last kernel variant launched by this thread */
const char* nvbio_hip_last_kernel_detail(void);  /* "pair" if that launch was the banded 16-bit LOCAL kernel in its two-jobs-per-lane form, else "" */
const char* nvbio_hip_last_kernel_cell(void);    /* the cell of a "pair" launch: "max3" (three-input maxima) or "u16" (two-input ones), else "" */
const char* nvbio_hip_last_kernel_frame(void);   /* the frame of a "pair" launch's cell: "column" (no gap subtract on the horizontal step) or "row", else "" */
const char* nvbio_hip_last_kernel_row(void);     /* the row of a "pair" launch around its cells: "fold2" (the sink folded once per two rows: the "column" frame unless NVBIO_HIP_PAIR_ROW is 1) or "plain", else "" */
const char* nvbio_hip_last_kernel_const(void);   /* where a "pair" launch's cell keeps its key constants: "literal" (in the instructions: the "fold2" row unless NVBIO_HIP_PAIR_CONST is 1 or |gap_ext| > 3), "vector" (no launch of the library's) or "scalar", else "" */
const char* nvbio_hip_last_kernel_sub(void);     /* where a "pair" launch's cell takes its substitution words from: "lds" (read from an LDS table, nvbio_hip_last_kernel_subread() says how many cells to a read: the "literal" form unless NVBIO_HIP_PAIR_SUB is 1) or "perm" (a v_perm_b32 lookup in two table words per row), else "" */
const char* nvbio_hip_last_kernel_subread(void); /* the cells one LDS read of an "lds" launch serves: "pair" (two, a ds_read_b64 from a table of pairs: the default) or "single" (NVBIO_HIP_PAIR_SUB is 2), else "" */
const char* nvbio_hip_last_kernel_fetch(void);   /* how a "pair" launch read its strings: "stream" (32-bit cursors, only new words loaded) or "generic", else "" */

#ifdef __cplusplus
}
#endif
#endif /* NVBIO_HIP_H */
