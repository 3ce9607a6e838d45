/*
 * pepper_hip.h — C-ABI of the MI355X-native PEPPER hot path.
 *
 * Two operator families live behind this boundary:
 *
 *   1. the pileup summary-image builder ("make_images" hot loop), replacing the pybind11 class
 *      PEPPER_VARIANT.RegionalSummaryGenerator
 *        reference: pepper_variant/modules/cpp/pybind_api.h:55-62 (binding),
 *                   pepper_variant/modules/cpp/region_summary.cpp:568-916 (generate_summary),
 *                   pepper_variant/modules/cpp/region_summary.cpp:337-566 (populate_summary_matrix)
 *   2. the recurrent-network inference step ("run_inference" hot loop), replacing
 *        transducer_model(images, False)   pepper_variant/modules/python/models/predict_distributed_gpu.py:65
 *        ort_session.run(...)              pepper_variant/modules/python/models/predict_distributed_cpu.py:85-88
 *      for plan P1 (pepper_variant 2x bi-LSTM + MLP head, models/simple_model.py:48-82) and
 *        transducer_model(image_chunk, hidden) in the sliding loop
 *                                          pepper/modules/python/models/predict.py:47-97
 *      for plan P2 (pepper polisher bi-GRU encoder/decoder, pepper/modules/python/models/simple_model.py:27-42).
 *
 * Conventions
 *   - plain C types only; every function returns 0 on success or a negative PV_ERR_* code;
 *     pv_last_error() returns a thread-local message for the last failure on this thread.
 *   - the caller owns every buffer. Entry points ending in _dev take DEVICE pointers and a HIP stream
 *     (hipStream_t passed as void*, NULL = the context's own stream) and never synchronise with the host;
 *     the others take HOST pointers, stage through the context's workspace and return when results are
 *     in the caller's host buffers.
 *   - one pv_ctx = one HIP device + one stream + one workspace. Calls on distinct contexts are
 *     independent; calls on one context must not overlap.
 *   - there is NO CPU fallback: if no HIP device is present pv_create fails with PV_ERR_NO_DEVICE.
 */
#ifndef PEPPER_HIP_H
#define PEPPER_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PV_OK 0
#define PV_ERR_INVALID (-1)      /* bad argument / malformed input            */
#define PV_ERR_NO_DEVICE (-2)    /* no HIP device or device id out of range   */
#define PV_ERR_HIP (-3)          /* a HIP runtime call failed                 */
#define PV_ERR_CAPACITY (-4)     /* caller output buffers too small (n_out / str_bytes hold the need) */
#define PV_ERR_LIMIT (-5)        /* an internal fixed limit was exceeded (message says which) */
#define PV_ERR_STATE (-6)        /* call order problem (e.g. forward before load) */

/* window geometry of the reference (pepper_variant/modules/python/Options.py:5-8,
 * region_summary.cpp:831 "candidate_window_size + 1") */
#define PV_WINDOW_ROWS 33
#define PV_FEATURES 26
#define PV_WINDOW_BYTES (PV_WINDOW_ROWS * PV_FEATURES)
#define PV_MAX_COLOR 125         /* region_summary.h:15-16 */
/* haplotag-aware variant (`-hp`): ImageSizeOptionsHP (Options.py:17-22): 48 planes, window 20 -> 21 rows
 * (region_summary_hp.cpp:946 "candidate_window_size + 1") */
#define PV_HP_WINDOW_ROWS 21
#define PV_HP_FEATURES 48
#define PV_HP_WINDOW_BYTES (PV_HP_WINDOW_ROWS * PV_HP_FEATURES)
#define PV_MAX_ALLELE_KEY 61     /* region_summary.cpp:461,511 "candidate_string.length() <= 61" */

/* CIGAR op codes = BAM codes = CIGAR_OPERATIONS (pepper_variant/modules/cpp/cigar.h:15-27) */
#define PV_CIGAR_MATCH 0
#define PV_CIGAR_IN 1
#define PV_CIGAR_DEL 2
#define PV_CIGAR_REF_SKIP 3
#define PV_CIGAR_SOFT_CLIP 4
#define PV_CIGAR_HARD_CLIP 5
#define PV_CIGAR_PAD 6
#define PV_CIGAR_EQUAL 7
#define PV_CIGAR_DIFF 8
#define PV_CIGAR_BACK 9

typedef struct pv_ctx pv_ctx;

/* ---- image builder ------------------------------------------------------------------------- */

/* The scalar arguments of RegionalSummaryGenerator::generate_summary
 * (region_summary.h:191-206; call site AlignmentSummarizer.py:223-238), same order, same types. */
typedef struct pv_params {
    double min_snp_baseq;
    double min_indel_baseq;
    double snp_freq_threshold;
    double insert_freq_threshold;
    double delete_freq_threshold;
    double min_coverage_threshold;
    double snp_candidate_freq_threshold;
    double indel_candidate_freq_threshold;
    double candidate_support_threshold;
    int32_t skip_indels;
    int32_t candidate_window_size; /* must be 32 */
    int32_t feature_size;          /* must be 26 */
    int32_t reserved;
} pv_params;

/* A batch of regions in flat SoA form. Region g owns reads [read_off[g], read_off[g+1]) and reference
 * bytes ref[ref_off[g] .. ref_off[g+1]). This replaces the by-value `vector<type_read>` argument
 * (read.h:60-108: pos, flags.is_reverse, mapping_quality, sequence, base_qualities, cigar_tuples) and
 * the constructor arguments (region_summary.cpp:9-17: region_start, region_end, reference_sequence).
 *   ref_end is INCLUSIVE; R = ref_end - ref_start + 1; ref_off[g+1]-ref_off[g] must be >= R.
 *   cigar words use BAM packing: (length << 4) | op.
 *   bases are normally the upper-case symbols bam_handler.cpp emits (seq_nt16_str "=ACMGRSVTWYHKDBN"),
 *   but ANY byte is handled exactly as the reference would (raw-byte SNP keys, toupper for planes). */
/* Limits: a region may hold at most 32767 reads (the per-column counters are 16-bit; the reference's caller keeps at most
 * MAX_READS_IN_REGION = 5000, pepper_variant/modules/python/Options.py:98, AlignmentSummarizer.py:191-208). Beyond that the
 * host-buffer forms return PV_ERR_LIMIT and the device-resident forms report status PV_ERR_LIMIT in d_counts[2]. */
typedef struct pv_batch_in {
    int32_t n_regions;
    int32_t reserved;
    const int64_t* ref_start;   /* [n_regions] */
    const int64_t* ref_end;     /* [n_regions] inclusive */
    const int64_t* cand_start;  /* [n_regions] candidate_region_start */
    const int64_t* cand_end;    /* [n_regions] candidate_region_end (inclusive) */
    const int64_t* ref_off;     /* [n_regions+1] */
    const uint8_t* ref;         /* reference bytes */
    const int64_t* read_off;    /* [n_regions+1] */
    const int64_t* read_pos;    /* [n_reads] type_read::pos */
    const uint8_t* read_flags;  /* [n_reads] bit0 = flags.is_reverse */
    const uint8_t* read_mapq;   /* [n_reads] type_read::mapping_quality */
    const int64_t* base_off;    /* [n_reads+1] into bases/quals */
    const uint8_t* bases;       /* type_read::sequence */
    const uint8_t* quals;       /* type_read::base_qualities (raw phred) */
    const int64_t* cigar_off;   /* [n_reads+1] into cigar */
    const uint32_t* cigar;      /* type_read::cigar_tuples */
} pv_batch_in;

/* One output record per surviving candidate allele = one CandidateImageSummary
 * (region_summary.h:88-111), in the reference's order (regions in batch order, sites ascending,
 * alleles in std::set<std::string> order). images are already cast to int8 with wrap-around as
 * DataStore.write_summary does (pepper_variant/modules/python/DataStore.py:68). */
typedef struct pv_batch_out {
    int64_t capacity;      /* in: number of windows the arrays below can hold */
    int64_t str_capacity;  /* in: bytes cand_str can hold */
    int32_t* region;       /* [capacity] index of the region in the batch */
    int64_t* position;     /* [capacity] CandidateImageSummary::position */
    uint8_t* depth;        /* [capacity] min(coverage,125) */
    uint8_t* cand_freq;    /* [capacity] candidate_frequency[0] = min(allele_depth,125) */
    int8_t* images;        /* [capacity][33][26] */
    int32_t* images_i32;   /* optional (may be NULL): the un-cast int values of image_matrix */
    char* cand_str;        /* allele keys, concatenated: "1T", "2AGG", "3CAA" ... (candidates[0]) */
    int64_t* cand_off;     /* [capacity+1] */
    int64_t n_out;         /* out: number of windows produced (or needed on PV_ERR_CAPACITY) */
    int64_t str_bytes;     /* out: bytes of cand_str produced (or needed) */
} pv_batch_out;

pv_ctx* pv_create(int device_id);
void pv_destroy(pv_ctx* ctx);
const char* pv_last_error(void);
/* returns the HIP stream (hipStream_t) the context launches on */
void* pv_stream(pv_ctx* ctx);
int pv_synchronize(pv_ctx* ctx);

/* generate_summary for a batch of regions, HOST buffers in and out. */
int pv_summarize_regions(pv_ctx* ctx, const pv_batch_in* in, const pv_params* params, pv_batch_out* out);

/* Device-resident form used by the fused pipeline and the benchmark: every pointer inside `in` and
 * `out` (the arrays, not the structs) is a DEVICE pointer; totals that the host form derives by
 * reading the offset arrays are passed explicitly. Asynchronous on `stream`; results counters are
 * written to the four-element DEVICE array `d_counts` = {n_out, str_bytes, status, reserved}
 * (out->n_out etc. are not touched). status is PV_OK or a PV_ERR_* code detected on the device
 * (malformed read, workspace limit). Windows beyond out->capacity are dropped (d_counts[0] still
 * holds the number needed). */
int pv_summarize_regions_dev(pv_ctx* ctx, const pv_batch_in* in, const pv_params* params,
                             int64_t n_reads, int64_t n_bases, int64_t n_cigar, int64_t n_ref_bytes,
                             int64_t max_region_len, pv_batch_out* out, int64_t* d_counts, void* stream);

/* Stage a HOST batch for the device-resident form: copies the arrays of `host` into the context's workspace (asynchronously
 * on `stream`, after validating the offset arrays on the host) and fills `dev` with the same struct holding DEVICE pointers,
 * valid until the next pv_upload_batch on this context; totals4 = {n_reads, n_bases, n_cigar, n_ref_bytes}, the totals
 * pv_summarize_regions_dev takes. With pv_summarize_regions_dev and pv_rnn_forward_p1_dev behind it this is the fused
 * call_variant step: reads in, probabilities out, windows never on the host. */
int pv_upload_batch(pv_ctx* ctx, const pv_batch_in* host, pv_batch_in* dev, int64_t* totals4, void* stream);
/* The same for a batch that arrives in n_parts host batches (e.g. one per interval from reader threads): their regions are laid
 * end to end in part order; the large arrays are copied part by part to their offsets on the device, so the caller never
 * concatenates them on the host. The previous upload's copies must have completed (synchronise the stream) before the next
 * call on the same context. */
int pv_upload_batches(pv_ctx* ctx, int n_parts, const pv_batch_in* const* parts, pv_batch_in* dev, int64_t* totals4, void* stream);

/* ---- haplotag-aware image builder (`make_images -hp`) --------------------------------------------
 * Replaces PEPPER_VARIANT.RegionalSummaryGeneratorHP (pybind_api.h:64-71; region_summary_hp.cpp:350-663 populate_summary_matrix,
 * :665-1012 generate_summary; call site AlignmentSummarizerHP.py:215-233). Same flat batch and scalar struct as
 * pv_summarize_regions plus one int per read, `read_hp` = type_read::hp_tag (the HP aux tag, 0 when absent; NULL = all 0):
 *   48 planes = {REF, SNP, INS, DEL overlays 0-3} + 4 x {REF count, A, C, G, T, I, D, *} for (HP1 fwd, HP1 rev, HP2 fwd,
 *   HP2 rev) with 3 overlay planes in front of each group; an untagged read (hp 0) counts in both haplotypes;
 *   params->candidate_window_size must be 20 and params->feature_size 48; out->images is [capacity][21][48]
 *   (images_i32 likewise); every plane is clamped to +-125 (region_summary_hp.cpp:762-767).
 * Results are bit-identical with the reference class on the same reads. */
int pv_summarize_regions_hp(pv_ctx* ctx, const pv_batch_in* in, const int32_t* read_hp, const pv_params* params,
                            pv_batch_out* out);
/* device-resident, asynchronous form: see pv_summarize_regions_dev; read_hp is a DEVICE pointer (or NULL) */
int pv_summarize_regions_hp_dev(pv_ctx* ctx, const pv_batch_in* in, const int32_t* read_hp, const pv_params* params,
                                int64_t n_reads, int64_t n_bases, int64_t n_cigar, int64_t n_ref_bytes,
                                pv_batch_out* out, int64_t* d_counts, void* stream);

/* ---- P2 (polisher) summary images -------------------------------------------------------------
 * Replaces SummaryGenerator::generate_summary + generate_image
 * (pepper/modules/src/pileup_summary/summary_generator.cpp:47-121, 274-304, 371-392) and
 * AlignmentSummarizer.chunk_images (pepper/modules/python/AlignmentSummarizer.py:19-56) for a batch of
 * regions. Input is the same pv_batch_in struct; quals, cand_start and cand_end are not read, and the reference
 * bytes are only needed for their length, as in the reference. Every reference position of a region
 * gives one image row followed by `longest insert anchored there` insert rows; a row is 10 uint8:
 *   0-3 A,C,G,T reverse  4-7 A,C,G,T forward  8 other/deleted reverse  9 other/deleted forward,
 *   value = (uint8) (count / max(1, coverage[position]) * 254), the double->uint8 conversion taken as
 *   truncation to int32 followed by the low byte (what the x86-64 build of the reference does; only
 *   reachable where deletions cover a column no read base covers).
 * The rows of a region are cut into chunks of seq_length rows that overlap by seq_overlap rows; the
 * last chunk is padded with zero rows whose position/index are -1. */
typedef struct pv_polish_out {
    int64_t chunk_capacity; /* in: chunks the chunk arrays can hold */
    int64_t row_capacity;   /* in: rows the flat arrays can hold (0 when the flat arrays are NULL) */
    uint8_t* images;        /* [chunk_capacity][seq_length][10] */
    int64_t* position;      /* [chunk_capacity][seq_length] genomic_pos.first */
    int32_t* index;         /* [chunk_capacity][seq_length] genomic_pos.second (0 = base row, k = k-th insert row) */
    int32_t* region;        /* [chunk_capacity] region of the batch */
    int32_t* chunk_id;      /* [chunk_capacity] chunk number inside its region */
    uint8_t* flat_images;   /* optional [row_capacity][10]: SummaryGenerator::image of all regions, concatenated */
    int64_t* flat_position; /* optional [row_capacity] */
    int32_t* flat_index;    /* optional [row_capacity] */
    int64_t* region_row_off;/* optional [n_regions+1] first flat row of every region */
    int64_t n_chunks;       /* out: chunks produced (or needed on PV_ERR_CAPACITY) */
    int64_t n_rows;         /* out: flat rows produced (or needed) */
    uint16_t* depth;        /* optional [chunk_capacity][seq_length] read depth of every row (below); NULL: nothing is written
                             * and nothing else changes. Behind the members of earlier builds, so their offsets stay */
    uint16_t* counts;       /* optional [chunk_capacity][seq_length][10] raw counts of every row (below), 4-byte aligned; NULL:
                             * nothing is written and nothing else changes. The last member, so the offsets above stay */
} pv_polish_out;
/* depth: for a base row (index 0) at position p, the sum of the column's ten counts before normalisation: the reads that hold
 * a base or a deleted column (D / N / P) at p, exactly as the builder counts them for the ten planes (so reads of mapping
 * quality 0, which the images leave out, are left out here too). It is not the normaliser `coverage` above, which carries
 * the reference's quirk of crediting a whole deletion to its first column. An insert row takes the depth of its anchor
 * position, a padding row 0. Values are clamped to 65535 (unreachable: a region holds at most 32767 reads). images,
 * position, index, region, chunk_id and the counters are byte for byte those of a call with depth == NULL. The plane is
 * gathered with the chunk rows, so it needs the chunk arrays; the flat arrays have no depth of their own. The library reads
 * the member in every call that takes the struct: zero the struct before filling it, as for every struct of this header.
 * counts: for a base row (index 0), the column's ten counts before normalisation, in the order of the image's ten features:
 * 0-3 A,C,G,T on reverse-strand reads, 4-7 A,C,G,T on forward-strand reads, 8 / 9 other or deleted on reverse / forward
 * reads (a read byte that is not ACGT after upper-casing, an N for instance, and every deleted column D / N / P). For an
 * insert row, that row's own ten counts: the reads that hold a base in this insert row, by base and strand (8 / 9: an
 * inserted byte that is not ACGT). A padding row is all zero. Reads of mapping quality 0 are left out, as in the images.
 * Each value is clamped to 65535 (unreachable, as for depth). Invariant: on a base row the ten counts sum to the row's
 * depth (wherever no clamp is met, which is everywhere in a region of at most 32767 reads). Every other output of the call (images, position, index, region, chunk_id, the counters, and depth where it was
 * asked for) is byte for byte that of a call with counts == NULL. Like depth, the plane is gathered with the chunk rows and
 * the flat arrays have none; the host form and the device form both fill it. */

/* HOST buffers in and out. */
int pv_polish_summarize_regions(pv_ctx* ctx, const pv_batch_in* in, int seq_length, int seq_overlap, pv_polish_out* out);
/* Device-resident, asynchronous form (see pv_summarize_regions_dev): d_counts = {n_chunks, n_rows, status, insert rows}. */
int pv_polish_summarize_regions_dev(pv_ctx* ctx, const pv_batch_in* in, int64_t n_reads, int64_t n_bases, int64_t n_cigar,
                                    int64_t n_ref_bytes, int seq_length, int seq_overlap, pv_polish_out* out,
                                    int64_t* d_counts, void* stream);

/* The polisher's stitch (pepper/modules/python/Stitch.py:37-86): labels of the chunks above -> polished bases.
 * chunks: position, index, region and chunk_id of n_chunks chunks as pv_polish_summarize_regions lays them out
 * (regions ascending; a region's chunks contiguous with chunk ids 0, 1, 2, ...; chunk_capacity >= n_chunks);
 * labels: uint8 [n_chunks][seq_length] (pv_rnn_forward_p2); region_start: int64 [n_regions] (pv_batch_in.ref_start).
 * Per region, a column is kept when position >= 0, index >= 0 and not (region_start > 0 and position <=
 * region_start + 200); a (position, index) two chunks share keeps the label of the chunk whose id is last in
 * decimal STRING order ("9" after "10"); labels 1..4 give 'A','C','G','T', 0 gives nothing.
 * Out: region_off int64 [n_regions+1] exclusive offsets of every region's bases in seq; seq uint8 [seq_capacity].
 * d_counts = {bases, status, first bad chunk (-1 if none), 0}; status PV_ERR_CAPACITY (seq_capacity < bases: nothing
 * written but region_off), PV_ERR_STATE (a kept label > 4, e.g. the 255 of a poisoned P2 call) or PV_ERR_INVALID
 * (chunk layout broken). Device-resident and asynchronous on `stream`; no global atomics, no host synchronisation. */
int pv_polish_stitch_dev(pv_ctx* ctx, const pv_polish_out* chunks, int64_t n_chunks, const uint8_t* labels,
                         const int64_t* region_start, int32_t n_regions, int seq_length, int seq_overlap,
                         int64_t* region_off, uint8_t* seq, int64_t seq_capacity, int64_t* d_counts, void* stream);
/* HOST buffers in and out; counts[4] as d_counts above; returns the status (PV_ERR_CAPACITY with counts[0] = bases needed). */
int pv_polish_stitch(pv_ctx* ctx, const pv_polish_out* chunks, int64_t n_chunks, const uint8_t* labels,
                     const int64_t* region_start, int32_t n_regions, int seq_length, int seq_overlap,
                     int64_t* region_off, uint8_t* seq, int64_t seq_capacity, int64_t* counts);

/* The polisher's per-base quality: the P2 labels and the accumulated softmax of pv_rnn_forward_p2[_dev] -> one Phred byte
 * per chunk row. It restates what the reference's caller means to store as phred_score, -10 log10(1 - value / counts)
 * (pepper/modules/python/models/predict_distributed_gpu.py:96-105; that code feeds the label in place of the value), as a
 * count of thresholds, so that host and device agree bit for bit and no logarithm is called. For row r of a chunk:
 *   cnt = 1.0f for r < seq_overlap or r >= seq_length - seq_overlap, else 2.0f (the windows that cover the row);
 *   err = 1.0f - acc[r][labels[r]] / cnt   (one float32 divide, one float32 subtract, not fused);
 *   q   = #{k in 1..93 : err <= T[k]},  T[k] = 10^(-k/10) rounded to float32, a literal table (pv_polish_qual_threshold).
 * So err <= 0 gives 93 (the FASTQ ceiling '~'), a NaN acc gives 0. A label above 4 gives q = 0 and status PV_ERR_STATE.
 * labels: uint8 [B][seq_length]; acc: float [B][seq_length][5]; qual: uint8 [B][seq_length], every row, label-0 rows included.
 * d_counts = {rows, status, first bad chunk (-1 if none), its first bad row}. Device-resident and asynchronous on `stream`;
 * no global atomics, no host synchronisation; capturable. */
int pv_polish_row_qual_dev(pv_ctx* ctx, const uint8_t* labels, const float* acc, int64_t B, int seq_length, int seq_overlap,
                           uint8_t* qual, int64_t* d_counts, void* stream);
/* HOST buffers in and out; counts[4] as d_counts above; returns the status (qual and counts are filled on PV_ERR_STATE too). */
int pv_polish_row_qual(pv_ctx* ctx, const uint8_t* labels, const float* acc, int64_t B, int seq_length, int seq_overlap,
                       uint8_t* qual, int64_t* counts);
/* T[k] of the rule above for k in 0..93 (T[0] = 1), 0 for any other k. Needs no device. */
float pv_polish_qual_threshold(int k);

/* pv_polish_stitch[_dev] with a second byte plane: row_qual uint8 [n_chunks][seq_length] (pv_polish_row_qual) in,
 * qual uint8 [seq_capacity] out. The same columns are kept, the same chunk wins a shared column and the same label-0
 * columns are dropped, so seq, region_off and d_counts are those of pv_polish_stitch[_dev]; qual[i] is the winning chunk's
 * row quality of the column that gave seq[i], stored raw (no +33). */
int pv_polish_stitch_qual_dev(pv_ctx* ctx, const pv_polish_out* chunks, int64_t n_chunks, const uint8_t* labels,
                              const int64_t* region_start, int32_t n_regions, int seq_length, int seq_overlap,
                              int64_t* region_off, uint8_t* seq, int64_t seq_capacity, int64_t* d_counts, void* stream,
                              const uint8_t* row_qual, uint8_t* qual);
int pv_polish_stitch_qual(pv_ctx* ctx, const pv_polish_out* chunks, int64_t n_chunks, const uint8_t* labels,
                          const int64_t* region_start, int32_t n_regions, int seq_length, int seq_overlap,
                          int64_t* region_off, uint8_t* seq, int64_t seq_capacity, int64_t* counts,
                          const uint8_t* row_qual, uint8_t* qual);

/* The polisher's edit list: what the labels of pv_polish_stitch[_dev]'s inputs change in the draft, one record per edited
 * column. A column (chunk k, row j) is KEPT under the stitch's rule: position >= 0, index >= 0 and not (region_start > 0 and
 * position <= region_start + 200). A kept column is OWNED by its chunk unless a neighbouring chunk of the same region holds
 * the same (position, index) and has an id later in decimal string order; ownership is decided before the label is looked
 * at, so the owned columns are exactly those whose label the stitch consults, and every kept (position, index) of the
 * builder's layout has one owner. An owned column with label b in 0..4 is an edit in these cases:
 *   index == 0: d = ref[ref_off[g] + position - region_start[g]], u = d with ASCII a..z upper-cased;
 *               b == 0 is a deletion (PV_EDIT_DEL); b >= 1 with "ACGT"[b-1] != u is a substitution (PV_EDIT_SUB), so a draft
 *               N or IUPAC byte under a base label is one, and a draft 'a' under label A is none;
 *   index  > 0: b >= 1 is an inserted base (PV_EDIT_INS); b == 0 is nothing.
 * Records of a region are in (position, index) order (chunk-major order of the owned columns), regions ascending.
 * Identity with the stitch: for every position p of region g with an owned index-0 column, ascending, take the
 * substitution's base, or nothing if p is deleted, or u if p has no index-0 record, then the bases of p's insert records in
 * index order; the concatenation is seq[region_off[g] .. region_off[g+1]) of pv_polish_stitch on the same inputs. */
#define PV_EDIT_SUB 1
#define PV_EDIT_DEL 2
#define PV_EDIT_INS 3
typedef struct pv_polish_edit {   /* 16 bytes, little-endian */
    int64_t position;
    int32_t index;
    uint8_t kind;   /* PV_EDIT_* */
    uint8_t draft;  /* the raw draft byte for index 0, 0 for an insert */
    uint8_t base;   /* 'A' 'C' 'G' 'T', 0 for a deletion */
    uint8_t qual;   /* the owned column's row quality when row_qual is given, else 255 */
} pv_polish_edit;

/* chunks, labels, region_start, seq_length, seq_overlap: as for pv_polish_stitch_dev (seq_length <= 4096, 2 * seq_overlap <=
 * seq_length); row_qual: uint8 [n_chunks][seq_length] from pv_polish_row_qual or NULL; ref_off int64 [n_regions+1] and ref:
 * the draft bytes of the batch (pv_batch_in.ref_off, pv_batch_in.ref).
 * Out: region_edit_off int64 [n_regions+1] exclusive offsets of every region's records (a region without chunks takes the
 * next region's offset); edits [edit_capacity], 16-byte aligned. d_counts = {edits, status, first bad chunk (-1 if none), 0}.
 * Status, with the stitch's precedence: PV_ERR_INVALID (chunk layout broken, or an owned column's position outside
 * [region_start[g], region_start[g] + ref_off[g+1] - ref_off[g]): checked before the draft byte is read, which is therefore
 * never read out of bounds), PV_ERR_STATE (an owned column's label above 4; on a losing or dropped column it is not an
 * error), PV_ERR_CAPACITY (edit_capacity < edits: region_edit_off and d_counts[0] are valid, no record is written).
 * ref == NULL with n_chunks > 0 is refused with PV_ERR_INVALID by the call itself. Device-resident and asynchronous on
 * `stream`; three launches, no global atomics, no host synchronisation; capturable. */
int pv_polish_edits_dev(pv_ctx* ctx, const pv_polish_out* chunks, int64_t n_chunks, const uint8_t* labels,
                        const uint8_t* row_qual, const int64_t* region_start, const int64_t* ref_off, const uint8_t* ref,
                        int32_t n_regions, int seq_length, int seq_overlap, int64_t* region_edit_off, pv_polish_edit* edits,
                        int64_t edit_capacity, int64_t* d_counts, void* stream);
/* HOST buffers in and out; counts[4] as d_counts above; returns the status (PV_ERR_CAPACITY with counts[0] = records needed
 * and region_edit_off filled). */
int pv_polish_edits(pv_ctx* ctx, const pv_polish_out* chunks, int64_t n_chunks, const uint8_t* labels,
                    const uint8_t* row_qual, const int64_t* region_start, const int64_t* ref_off, const uint8_t* ref,
                    int32_t n_regions, int seq_length, int seq_overlap, int64_t* region_edit_off, pv_polish_edit* edits,
                    int64_t edit_capacity, int64_t* counts);

/* The read evidence of every edit: pv_polish_edits[_dev] with one 8-byte record beside every edit record, taken from the
 * depth and the raw counts of the edit's own chunk row (pv_polish_out.depth and .counts, which the builder fills on request).
 * Write c[f] for the ten counts of that row, u for the upper-cased draft byte, k(x) = 0..3 for x in A, C, G, T:
 *   substitution to base b: alt_rev = c[k(b)], alt_fwd = c[4 + k(b)], ref = c[k(u)] + c[4 + k(u)] if u is in ACGT, else 0;
 *   deletion:               alt_rev = c[8],    alt_fwd = c[9],        ref as for a substitution. Planes 8 and 9 also count
 *                           read bytes that are not ACGT (an N in a read), so a deletion's support includes those reads;
 *   inserted base b:        alt_rev = c[k(b)], alt_fwd = c[4 + k(b)] of the insert row's own counts,
 *                           ref = max(0, depth - sum of c[0..9]): the reads over the anchor that hold nothing in this
 *                           insert row.
 * depth is chunks->depth of the edited column (an insert column carries its anchor's); ref is clamped to 65535. */
typedef struct pv_polish_evidence {   /* 8 bytes, little-endian; evidence[i] belongs to edits[i] */
    uint16_t depth;
    uint16_t ref;      /* reads that spell the draft there */
    uint16_t alt_fwd;  /* forward-strand reads that spell the edit */
    uint16_t alt_rev;  /* reverse-strand reads that spell the edit */
} pv_polish_evidence;
/* Arguments, edits, region_edit_off, d_counts, statuses and their precedence: those of pv_polish_edits_dev, byte for byte,
 * with and without row_qual. evidence [edit_capacity], 8-byte aligned. chunks->depth == NULL or chunks->counts == NULL with
 * n_chunks > 0, and a misaligned evidence, are refused with PV_ERR_INVALID by the call itself. Under any status but PV_OK no
 * evidence record is written. The counts row and the depth are loaded for edit columns only, after the classification; a
 * record leaves as one 8-byte store. Three launches (the count pass and the scan are those of pv_polish_edits_dev), no
 * global atomics, no host synchronisation; capturable. */
int pv_polish_edits_evidence_dev(pv_ctx* ctx, const pv_polish_out* chunks, int64_t n_chunks, const uint8_t* labels,
                                 const uint8_t* row_qual, const int64_t* region_start, const int64_t* ref_off,
                                 const uint8_t* ref, int32_t n_regions, int seq_length, int seq_overlap,
                                 int64_t* region_edit_off, pv_polish_edit* edits, pv_polish_evidence* evidence,
                                 int64_t edit_capacity, int64_t* d_counts, void* stream);
/* HOST buffers in and out (chunks->depth and chunks->counts too); otherwise as pv_polish_edits. */
int pv_polish_edits_evidence(pv_ctx* ctx, const pv_polish_out* chunks, int64_t n_chunks, const uint8_t* labels,
                             const uint8_t* row_qual, const int64_t* region_start, const int64_t* ref_off, const uint8_t* ref,
                             int32_t n_regions, int seq_length, int seq_overlap, int64_t* region_edit_off, pv_polish_edit* edits,
                             pv_polish_evidence* evidence, int64_t edit_capacity, int64_t* counts);

/* The polisher's minimum depth: where too few reads stand behind a row, its label is rewritten to spell the draft, before
 * the stitch, so that pv_polish_stitch[_qual] and pv_polish_edits on the rewritten labels keep the draft there (FASTA, FASTQ
 * and edit records stay consistent, and those kernels are untouched). The reference has no counterpart.
 * chunks: position, index, region, chunk_id and depth of n_chunks chunks (pv_polish_summarize_regions[_dev] with the depth
 * plane); labels, row_qual (or NULL), region_start, ref_off, ref: as for pv_polish_edits_dev. For row j of chunk k, g = region[k]:
 *   position < 0 (padding) or depth[k][j] >= min_depth: label and quality are copied unchanged - a label above 4 too, which
 *               the stitch still reports as today;
 *   otherwise the row is MASKED:
 *     index == 0: d = ref[ref_off[g] + position - region_start[g]], u = d with ASCII a..z upper-cased;
 *                 u in "ACGT": the label becomes 1 + its place in "ACGT" and the quality 0;
 *                 any other u (N, IUPAC): no label spells it, so label and quality are copied and the row counts as UNMASKABLE;
 *     index  > 0: the label becomes 0 (no inserted base) and the quality 0.
 * Every row is treated, owned or not: two chunks that share a (position, index) hold the same depth and the same draft byte,
 * so they receive the same label, and neither the stitch's string-order winner nor the ownership rule of the edits is
 * affected. labels_out == labels and row_qual_out == row_qual (in place) are allowed; row_qual and row_qual_out are given or
 * NULL together. min_depth == 0 is the identity.
 * d_counts = {masked rows (label rewritten), status, first bad chunk (-1 if none), unmaskable rows}. Status PV_ERR_INVALID:
 * the chunk layout is broken (as for the stitch), or a masked index-0 row's position lies outside [region_start[g],
 * region_start[g] + ref_off[g+1] - ref_off[g]) - checked before the draft byte is read, which is therefore never read out
 * of bounds; such a row is copied. chunks->depth == NULL, ref == NULL with n_chunks > 0 and min_depth outside 0..65535 are
 * refused with PV_ERR_INVALID by the call itself, before anything is launched. Device-resident and asynchronous on `stream`;
 * one workgroup per chunk and a one-block finish, no global atomics, no host synchronisation; capturable. */
int pv_polish_mask_low_depth_dev(pv_ctx* ctx, const pv_polish_out* chunks, int64_t n_chunks, const uint8_t* labels,
                                 const uint8_t* row_qual, const int64_t* region_start, const int64_t* ref_off, const uint8_t* ref,
                                 int32_t n_regions, int seq_length, int min_depth, uint8_t* labels_out, uint8_t* row_qual_out,
                                 int64_t* d_counts, void* stream);
/* HOST buffers in and out; counts[4] as d_counts above; returns the status (on PV_ERR_INVALID from the device, labels_out and
 * row_qual_out are left as they were). */
int pv_polish_mask_low_depth(pv_ctx* ctx, const pv_polish_out* chunks, int64_t n_chunks, const uint8_t* labels,
                             const uint8_t* row_qual, const int64_t* region_start, const int64_t* ref_off, const uint8_t* ref,
                             int32_t n_regions, int seq_length, int min_depth, uint8_t* labels_out, uint8_t* row_qual_out,
                             int64_t* counts);

/* The polisher's minimum quality: an edit whose quality is too low is taken back before the stitch, so that
 * pv_polish_stitch[_qual] and pv_polish_edits on the rewritten labels keep the draft there (FASTA, FASTQ and edit records stay
 * consistent, and those kernels are untouched). The reference has no counterpart. An edit is applied whole or not at all, so
 * the unit is a RUN of adjacent edited columns, which is what the VCF composer joins into one record.
 * chunks, labels, region_start, ref_off, ref, seq_length, seq_overlap: as for pv_polish_edits_dev; row_qual: uint8
 * [n_chunks][seq_length] from pv_polish_row_qual, mandatory; chunks->depth is not read.
 * Kept, owned and edit are the words of pv_polish_edits above: the owned edit columns of a region, in (position, index)
 * order, are exactly the records pv_polish_edits_dev would emit for these labels.
 *   RUN: a maximal stretch of a region's records in which consecutive records have equal or consecutive positions
 *        (position[i+1] - position[i] <= 1). Runs never cross a region boundary: a VCF block that straddles two regions is
 *        judged as two runs.
 *   m = the minimum of row_qual over the run's columns. The run is PINNED if one of its index-0 records stands over a draft
 *        byte whose upper-case form is not in "ACGT" (no label spells it, as for pv_polish_mask_low_depth).
 *   m < min_qual and not pinned: the run is REVERTED: its index-0 columns get the label that spells the upper-cased draft
 *        byte and quality 0, its insert columns label 0 and quality 0.
 *   A pinned run is copied unchanged whatever m is, and so is every run with m >= min_qual.
 * Every row that is not an owned edit column of a reverted run keeps its label and quality. That includes the non-owned
 * duplicate of a reverted column in the neighbouring chunk: nothing reads it, since the stitch and the edits consult owners
 * only and ownership does not depend on labels. Every surviving run has minimum >= min_qual, so every VCF record composed
 * from the edits of labels_out has QUAL >= min_qual. pv_polish_edits on labels_out gives the records of labels minus those of
 * the reverted runs; pv_polish_stitch[_qual] on labels_out gives the draft with exactly those records applied.
 * labels_out == labels and row_qual_out == row_qual (in place) are allowed. min_qual == 0 is the identity; min_qual == 94
 * reverts every run that is not pinned, because qualities stop at 93.
 * d_counts = {rows reverted, status, first bad chunk (-1 if none), rows of pinned runs whose minimum was below min_qual}.
 * Status, with the edits' precedence: PV_ERR_INVALID (chunk layout broken, or an owned column's position outside the
 * region's draft: checked before the draft byte is read), PV_ERR_STATE (an owned column's label above 4). Under any status
 * but PV_OK nothing but d_counts is written, in place or not. row_qual or row_qual_out == NULL, ref == NULL with n_chunks > 0,
 * min_qual outside 0..94 and 2 * seq_overlap > seq_length are refused with PV_ERR_INVALID by the call itself, before anything
 * is launched. Device-resident and asynchronous on `stream`; three launches (one workgroup per chunk, a one-block pass over
 * the chunk summaries that carries a run through any number of chunks, one workgroup per chunk), no global atomics, no host
 * synchronisation; capturable. */
int pv_polish_filter_low_qual_dev(pv_ctx* ctx, const pv_polish_out* chunks, int64_t n_chunks, const uint8_t* labels,
                                  const uint8_t* row_qual, const int64_t* region_start, const int64_t* ref_off, const uint8_t* ref,
                                  int32_t n_regions, int seq_length, int seq_overlap, int min_qual, uint8_t* labels_out,
                                  uint8_t* row_qual_out, int64_t* d_counts, void* stream);
/* HOST buffers in and out; counts[4] as d_counts above; returns the status (on an error status from the device, labels_out and
 * row_qual_out are left as they were). */
int pv_polish_filter_low_qual(pv_ctx* ctx, const pv_polish_out* chunks, int64_t n_chunks, const uint8_t* labels,
                              const uint8_t* row_qual, const int64_t* region_start, const int64_t* ref_off, const uint8_t* ref,
                              int32_t n_regions, int seq_length, int seq_overlap, int min_qual, uint8_t* labels_out,
                              uint8_t* row_qual_out, int64_t* counts);

/* The polisher's minimum support: an edit that too few reads spell is taken back before the stitch, for the reasons and with
 * the consequences of pv_polish_filter_low_qual above: the network sees normalised frequencies and carries state along the
 * sequence, so it can emit a base, a deletion or an inserted base where no read, or a single read, holds it. The reference
 * has no counterpart. KEPT, OWNED, edit, RUN and PINNED are the words of pv_polish_edits and pv_polish_filter_low_qual: the
 * owned edit columns of a region in (position, index) order are the records pv_polish_edits_dev would emit, a run is a
 * maximal stretch of them with position[i+1] - position[i] <= 1, runs never cross a region boundary, and a run is pinned if
 * one of its index-0 records stands over a draft byte whose upper-case form is not in "ACGT".
 * chunks, labels, region_start, ref_off, ref, seq_length, seq_overlap: as for pv_polish_edits_evidence_dev: chunks->counts
 * (4-byte aligned) and chunks->depth must be there; the counts row is loaded for edit columns only, after the
 * classification, as five dwords; the support does not depend on the depth, which is not loaded. row_qual, row_qual_out:
 * uint8 [n_chunks][seq_length], given or NULL together; they are not judged, only copied and zeroed.
 *   The SUPPORT of an edit column is alt_fwd + alt_rev of the pv_polish_evidence record pv_polish_edits_evidence writes for it,
 *        with c[f] the ten counts of its own row and k(x) = 0..3 for x in A, C, G, T:
 *          substitution to base b: c[k(b)] + c[4 + k(b)];
 *          deletion:               c[8] + c[9] (which also count read bytes that are not ACGT);
 *          inserted base b:        c[k(b)] + c[4 + k(b)] of the insert row's own counts.
 *        Each addend is a uint16; the sum (up to 131070) is compared as an int and is not clamped again. Reads of mapping
 *        quality 0 are in no count.
 *   s = the minimum support over the run's columns: the weakest column the evidence reports for the run's VCF record.
 *   s < min_support and not pinned: the run is REVERTED whole: its index-0 columns get the label that spells the upper-cased
 *        draft byte, its insert columns label 0, and every such row quality 0 where a quality plane is given.
 *   A pinned run is copied unchanged whatever s is, and so is every run with s >= min_support.
 * Every row that is not an owned edit column of a reverted run keeps its label and quality, the non-owned duplicate of a
 * reverted column included. min_support == 0 is the identity; the range is 0..65535; min_support == 1 is "no edit without a
 * read behind it". labels_out == labels and row_qual_out == row_qual (in place) are allowed.
 * Consequences: pv_polish_edits on labels_out gives the records of labels minus those of the reverted runs;
 * pv_polish_stitch[_qual] on labels_out gives the draft with exactly the surviving records applied; every VCF record composed
 * afterwards from pv_polish_edits_evidence has alt_fwd + alt_rev >= min_support in its weakest column (a VCF block that
 * straddles two regions is two runs, each >= min_support). The filter commutes with pv_polish_filter_low_qual: both revert
 * whole runs, and reverting one run neither splits nor joins another (the reverted columns stop being records, the others
 * keep their positions and the gaps between them only grow where a run is gone whole), so either order gives the union of
 * the reverted runs. It does not commute with pv_polish_mask_low_depth, which works per row and can split a run: the mask
 * goes first.
 * d_counts = {rows reverted, status, first bad chunk (-1 if none), rows of pinned runs whose support was below min_support}.
 * Statuses and their precedence: those of pv_polish_filter_low_qual; under any status but PV_OK nothing but d_counts is
 * written. chunks->counts == NULL or chunks->depth == NULL with n_chunks > 0, ref == NULL with n_chunks > 0, min_support
 * outside 0..65535, 2 * seq_overlap > seq_length and exactly one of row_qual and row_qual_out given are refused with
 * PV_ERR_INVALID by the call itself, before anything is launched. Device-resident and asynchronous on `stream`; the three
 * launches of pv_polish_filter_low_qual_dev (its run machinery and its one-block pass; the per-chunk kernels take the value
 * of a record from the counts row instead of the quality byte), no global atomics, no host synchronisation; capturable. */
int pv_polish_filter_low_support_dev(pv_ctx* ctx, const pv_polish_out* chunks, int64_t n_chunks, const uint8_t* labels,
                                     const uint8_t* row_qual, const int64_t* region_start, const int64_t* ref_off,
                                     const uint8_t* ref, int32_t n_regions, int seq_length, int seq_overlap, int min_support,
                                     uint8_t* labels_out, uint8_t* row_qual_out, int64_t* d_counts, void* stream);
/* HOST buffers in and out (chunks->depth and chunks->counts too); counts[4] as d_counts above; returns the status (on an error
 * status from the device, labels_out and row_qual_out are left as they were). */
int pv_polish_filter_low_support(pv_ctx* ctx, const pv_polish_out* chunks, int64_t n_chunks, const uint8_t* labels,
                                 const uint8_t* row_qual, const int64_t* region_start, const int64_t* ref_off, const uint8_t* ref,
                                 int32_t n_regions, int seq_length, int seq_overlap, int min_support, uint8_t* labels_out,
                                 uint8_t* row_qual_out, int64_t* counts);

/* The polisher without a model: a majority vote of the reads of every chunk row, from the builder's raw counts, that writes
 * the two planes pv_rnn_forward_p2[_dev] writes, labels and acc, so that everything behind the network (pv_polish_row_qual,
 * the mask, the filters, the stitch, the edits and their evidence) runs on it unchanged. It is the floor a trained network
 * is compared with, not a replacement: a pileup majority cannot mend systematic read errors (homopolymer lengths; the part
 * of them that comes from voting per column and not per read is what pv_polish_vote_runs below takes on). The
 * reference has no counterpart.
 * chunks: position, index, region, chunk_id, depth and counts (4-byte aligned) of n_chunks chunks (pv_polish_summarize_regions
 * [_dev] with both planes); region_start, ref_off, ref, seq_length, seq_overlap: as for pv_polish_edits_evidence_dev.
 * Out: labels uint8 [n_chunks][seq_length]; acc float [n_chunks][seq_length][5] or NULL, which is then not written.
 * For row j of chunk k write c[0..9] for counts[k][j], d for depth[k][j], g = region[k]:
 *   position < 0 or index < 0 (padding): label 0, acc all 0.
 *   index == 0 (a base row): n[b] = c[b-1] + c[4+b-1] for b = 1..4 (A, C, G, T on both strands); n[0] = c[8] + c[9] (deleted
 *               columns and read bytes that are not ACGT, as in the evidence rule); total = n[0] + ... + n[4], from the counts
 *               (d is not used); u = ref[ref_off[g] + position - region_start[g]] with ASCII a..z upper-cased, dl = 1 + its
 *               place in "ACGT", or none. The winner is the b with the largest n[b]: among equal bases dl if it is one of
 *               them, else the smallest of 1..4; label 0 (a deletion) wins only strictly ahead of every base. With total == 0
 *               the winner is dl, and label 0 where dl is none: a column without reads over a draft byte no label spells
 *               cannot be spelled and leaves the sequence.
 *   index  > 0 (an insert row): n[1..4] as above from the row's own counts; n[0] = max(0, d - (c[0] + ... + c[9])) + c[8] + c[9]:
 *               the reads over the anchor that hold nothing in this insert row, and those whose inserted byte is not ACGT;
 *               total = n[0] + ... + n[4]. The winner is the largest; on a tie label 0 (nothing, which is the draft) wins,
 *               then the smallest of 1..4.
 *   acc[k][j][b] = w(j) * ((float)n[b] / (float)max(total, 1)), w(j) = 1.0f for j < seq_overlap or j >= seq_length -
 *               seq_overlap, else 2.0f (the cnt of pv_polish_row_qual): one correctly rounded float32 divide and one multiply
 *               by a power of two, so pv_polish_row_qual sees n / total exactly, and its Phred byte is that of the fraction of
 *               reads that disagree with the winner (0 for a row without reads, 93 where all reads agree).
 * Every row is treated, owned or not: two chunks that share a (position, index) hold the same counts, depth and draft byte,
 * so they receive the same label.
 * d_counts = {rows that are not padding whose winner is not what the draft holds (a base row with label != dl - always so
 * where dl is none - or an insert row with label >= 1), status, first bad chunk (-1 if none), base rows with total == 0}.
 * Status PV_ERR_INVALID: the chunk layout is broken (as for the stitch), or a base row's position lies outside
 * [region_start[g], region_start[g] + ref_off[g+1] - ref_off[g]) - checked before the draft byte is read, which is therefore
 * never read out of bounds; then nothing but d_counts is written. chunks->depth == NULL, chunks->counts == NULL or ref == NULL
 * with n_chunks > 0, and 2 * seq_overlap > seq_length, are refused with PV_ERR_INVALID by the call itself, before anything
 * is launched. Device-resident and asynchronous on `stream`; three launches (one workgroup per chunk, a one-block finish, one
 * workgroup per chunk), no global atomics, no host synchronisation; capturable. */
int pv_polish_vote_dev(pv_ctx* ctx, const pv_polish_out* chunks, int64_t n_chunks, const int64_t* region_start,
                       const int64_t* ref_off, const uint8_t* ref, int32_t n_regions, int seq_length, int seq_overlap,
                       uint8_t* labels, float* acc, int64_t* d_counts, void* stream);
/* HOST buffers in and out (chunks->depth and chunks->counts too); counts[4] as d_counts above; returns the status (on
 * PV_ERR_INVALID from the device, labels and acc are left as they were). */
int pv_polish_vote(pv_ctx* ctx, const pv_polish_out* chunks, int64_t n_chunks, const int64_t* region_start,
                   const int64_t* ref_off, const uint8_t* ref, int32_t n_regions, int seq_length, int seq_overlap,
                   uint8_t* labels, float* acc, int64_t* counts);

/* The run vote (`polish --vote --runs`): behind pv_polish_vote[_dev], on the same labels / acc planes and in place, the
 * length of every homopolymer run of the draft is voted READ BY READ. The column vote sees the ten counts of a row, not which
 * read spelled what: deletions that the aligner left-aligns pile up in a run's first column though no length but the
 * draft's has a majority, and an inserted base that sits at several anchors never gathers one in any insert row. Here every
 * read measures the run once. What stays out of reach: a miscall most reads share, runs above 48 bytes, adjacent runs. The
 * reference has no counterpart.
 * chunks: position, index, region, chunk_id of n_chunks chunks (chunk_capacity >= n_chunks; depth and counts are not read);
 * in: the read batch the builder was given, DEVICE pointers (read_off, read_pos, read_mapq, base_off, bases, cigar_off, cigar
 * are read; in->n_regions must equal n_regions) with its totals n_reads, n_bases, n_cigar and n_ref_bytes = ref_off[n_regions],
 * as pv_polish_summarize_regions_dev takes them; region_start, ref_off, ref, n_regions, seq_length, seq_overlap: as for
 * pv_polish_vote_dev; min_run in 2..48, anything else is refused with PV_ERR_INVALID by the call itself.
 * STRETCHES AND CANDIDATES. In the draft bytes of region g, ref[ref_off[g] .. ref_off[g+1]), a stretch is a maximal sequence
 *   [s, e] of one letter b of A, C, G, T (ASCII a..z upper-cased first; any other byte ends a stretch), n = e - s + 1. It is a
 *   CANDIDATE when min_run <= n <= 48 and both flanks s-1 and e+1 lie inside the region's draft bytes. A candidate one of whose
 *   flanks lies in another candidate (the stretch that ends at s-1 or starts at e+1 is a candidate by the sentence before;
 *   the test is not repeated on what it leaves) is SKIPPED: the two would share the insert rows between them, so both stay
 *   with the column vote. The others are the runs voted on. Positions below are draft positions, region_start[g] + offset.
 * VOTERS. Walk a read's CIGAR from read_pos: M, = and X align a read base to every draft position they cover; I and S advance
 *   the read only; D, N and P the draft only (the builder's deleted columns); anything else nothing. A read of region g
 *   (read_off) with mapping quality above 0 (the builder's rule, so the voters are reads the images hold) SPANS a run when it
 *   has an aligned base at s-1 and at e+1, at read offsets q0 < q1; S is the number of spanning reads (mapping quality 0 is
 *   in neither S nor V). A spanning read is a VOTER when len = q1 - q0 - 1 <= 63, its bytes at q0 and q1, upper-cased,
 *   differ from b, and every byte strictly between them, upper-cased, equals b. len = 0 is valid: the read deleted the run.
 *   V is the number of voters, h[len] their number per length; both strands count together.
 * DECISION. A run is decided iff V >= 1 and 2 * V > S; an undecided run keeps the column vote's rows (an insertion of another
 *   base next to the run makes most reads impure, and that insertion must survive). The winner L is the length with the
 *   largest h; among equal ones n, else the closest to n, else the smaller.
 * ROWS. A decided run's span is every chunk row with position in [s, e] and the insert rows (index > 0) at position s-1, in
 *   every chunk that holds one, owned or not, in (position, index) order:
 *   L <= n: the first n - L base rows get label 0 (left-aligned, as VCF normalisation places a deletion), the other base rows
 *           b's label (1 + its place in "ACGT"), every insert row of the span 0.
 *   L >  n: every base row gets b's label, the first L - n insert rows of the span b's label, the others 0. Some voter holds
 *           L - n inserted bytes inside the span, so that many insert rows exist; where the chunks hold fewer the status is
 *           PV_ERR_STATE (never expected).
 *   acc (where not NULL) of a rewritten row j: w(j) * ((float)h[L] / (float)V) in the label's slot, w(j) as in the vote rule,
 *           and 0.0f in the other four. pv_polish_row_qual reads the label's slot only, so the row's Phred byte is that of the
 *           fraction of the run's voters whose length is not L, the same for every row of the span.
 *   The flat row of chunk c's row j inside its region is c * (seq_length - seq_overlap) + j (the builder's layout); the rank
 *   of an insert row inside its span follows from it and from the flat row of the left flank's base row.
 * d_counts[6] = {runs decided, status, first bad chunk (-1 if none), decided runs with L != n, candidates, candidates
 * skipped}. Status PV_ERR_INVALID: the chunk layout is broken exactly as for pv_polish_vote_dev; PV_ERR_STATE as above
 * (d_counts[2] = -1). Under either nothing but d_counts is written, and d_counts[0] and [3] are 0. With n_chunks == 0 or no
 * draft bytes nothing is looked at: d_counts = {0, PV_OK, -1, 0, 0, 0}. Device-resident and asynchronous on `stream`; six
 * launches, no global atomics (the histograms are LDS counters of the tile of 256 draft bytes a run starts in), no host
 * synchronisation; capturable; the result does not depend on the launch geometry. */
int pv_polish_vote_runs_dev(pv_ctx* ctx, const pv_polish_out* chunks, int64_t n_chunks, const pv_batch_in* in, int64_t n_reads,
                            int64_t n_bases, int64_t n_cigar, int64_t n_ref_bytes, const int64_t* region_start,
                            const int64_t* ref_off, const uint8_t* ref, int32_t n_regions, int seq_length, int seq_overlap,
                            int min_run, uint8_t* labels, float* acc, int64_t* d_counts, void* stream);
/* HOST buffers in and out: `in` is the host batch (its ref_start, ref_off and ref are the regions' and the draft's; it is staged
 * with pv_upload_batch, so it must pass the builder's checks); labels and acc (or NULL) hold the column vote's planes and are
 * rewritten in place; counts[6] as d_counts above; returns the status (on an error status labels and acc are left as they were). */
int pv_polish_vote_runs(pv_ctx* ctx, const pv_polish_out* chunks, int64_t n_chunks, const pv_batch_in* in, int seq_length,
                        int seq_overlap, int min_run, uint8_t* labels, float* acc, int64_t* counts);

/* The polisher's read realignment (AlignmentSummarizer.reads_to_reference_realignment, pepper/modules/python/
 * AlignmentSummarizer.py:159-177 -> ReadAligner::align_reads_to_reference, simple_aligner.cpp:66-107): every read of a region
 * is aligned to the draft with the reference's striped Smith-Waterman rules (match 4, mismatch 6, gap open 8, gap extend 2,
 * local; ends and CIGAR ties exactly as ssw.c / ssw_cpp.cpp break them).
 * in: the builder's batch, unchanged (ref_start, read_off, read_pos, base_off, bases, cigar_off, cigar are read);
 * win_off [n_regions+1], win: region g's realignment window win[win_off[g] .. win_off[g+1]) = draft [ref_start, ref_end + 20),
 * fewer bases at a contig end (AlingerOptions.ALIGNMENT_SAFE_BASES). It is kept apart from pv_batch_in.ref, whose length
 * defines the builder's columns.
 * Per read, in order: read_pos < ref_start: dropped (0 cigar words, state 2); empty query or read_pos at or past the window
 * end: unchanged (state 0); otherwise aligned against window[read_pos - ref_start ..]: score > 1 gives state 1, pos =
 * read_pos + ref_begin and the new cigar (S head, '=' and 'X' runs both written as MATCH and kept apart, I, D, S tail);
 * score <= 1 leaves the read unchanged. Bytes other than A/C/G/T/U (either case) are N; bytes >= 128 too.
 * The output with the input's bases, quals, flags and mapq is a realigned pv_batch_in for pv_polish_summarize_regions[_dev].
 * Limits: a query of at most 16384 bases and a window of at most 2047 bases from the read's pos; the direction bytes of the
 * traceback come from a bounded pool (option realign_scratch_kb, default 512 MB) that reads share in turn. A read beyond
 * them is status PV_ERR_LIMIT; nothing is truncated. */
typedef struct pv_realign_out {
    int64_t cigar_capacity; /* in: words cigar can hold */
    int64_t* read_pos;      /* [n_reads] new pos */
    int64_t* cigar_off;     /* [n_reads+1] */
    uint32_t* cigar;        /* [cigar_capacity] BAM packing */
    int32_t* score;         /* [n_reads] SSW score (0 for dropped reads and empty queries) */
    int32_t* ends;          /* [n_reads][4] ref_begin, ref_end, query_begin, query_end (0 unless realigned); ref_* count
                             * from the read's pos */
    uint8_t* state;         /* [n_reads] 0 unchanged, 1 realigned, 2 dropped */
    int32_t* band;          /* optional (may be NULL) [n_reads]: banded_sw's final band width w of a realigned read, else 0 */
    int64_t n_cigar;        /* out: cigar words produced (or needed on PV_ERR_CAPACITY) */
    int64_t n_realigned;    /* out */
    int64_t n_dropped;      /* out */
} pv_realign_out;

/* HOST buffers in and out (score, ends and state may be NULL). PV_ERR_CAPACITY: out->n_cigar holds the words needed. */
int pv_polish_realign(pv_ctx* ctx, const pv_batch_in* in, const int64_t* win_off, const uint8_t* win, pv_realign_out* out);
/* Device-resident, asynchronous form: every array is a DEVICE pointer; max_query_len bounds the longest read (it sizes the
 * kernels' LDS); d_counts = {n_cigar, status, reads realigned, reads dropped}; status PV_OK, PV_ERR_CAPACITY (nothing but
 * cigar_off and the per-read records written), PV_ERR_LIMIT or PV_ERR_STATE (a traceback left its band: never expected). */
int pv_polish_realign_dev(pv_ctx* ctx, const pv_batch_in* in, int64_t n_reads, int64_t n_bases, int64_t max_query_len,
                          const int64_t* win_off, const uint8_t* win, pv_realign_out* out, int64_t* d_counts, void* stream);

/* ---- selection of a flat batch by haplotype (`polish -hp`) -----------------------------------------------------------
 * `polish -hp` polishes once per haplotype, each pass on the reads of that haplotype. The builder and the realigner take a
 * batch whose offset arrays are contiguous, so a read cannot be left out in place: the batch is compacted on the device.
 * For a haplotype h >= 1 and one int per read, `read_hp` (the HP aux tag, 0 when absent; NULL = all 0):
 *   read r is KEPT iff read_hp == NULL, read_hp[r] == 0 (untagged: counts for every haplotype, as in pv_summarize_regions_hp)
 *   or read_hp[r] == h; any other value (the other haplotype, 3 and above, negative values) drops it.
 * The output is the input batch with the dropped reads removed and nothing else changed: kept reads stay in input order
 * inside their region; read_pos, read_flags, read_mapq, read_hp and each read's bytes of bases and quals and words of cigar
 * are the input's; read_off, base_off and cigar_off are rebuilt from 0 so that the arrays are contiguous again. The region
 * arrays (ref_start, ref_end, cand_*, ref_off, ref) are not copied: a pv_batch_in of the output points at the input's. A
 * region may end with no reads (read_off[g+1] == read_off[g] is a legal batch). If every read is kept, every output array
 * equals its input byte for byte (base_off[0] = cigar_off[0] = 0 given).
 * Every array of the output is caller-owned. quals is copied only where in->quals is given. */
typedef struct pv_select_out {
    int64_t read_capacity;  /* in: reads the per-read arrays can hold (base_off and cigar_off: one entry more) */
    int64_t base_capacity;  /* in: bytes bases (and quals) can hold */
    int64_t cigar_capacity; /* in: words cigar can hold */
    int64_t* read_off;      /* [n_regions+1] */
    int64_t* read_pos;      /* [read_capacity] */
    uint8_t* read_flags;    /* [read_capacity] */
    uint8_t* read_mapq;     /* [read_capacity] */
    int64_t* base_off;      /* [read_capacity+1] */
    uint8_t* bases;         /* [base_capacity] */
    uint8_t* quals;         /* [base_capacity] */
    int64_t* cigar_off;     /* [read_capacity+1] */
    uint32_t* cigar;        /* [cigar_capacity] */
    int32_t* read_hp;       /* optional (may be NULL) [read_capacity]: the kept reads' tags (0 where read_hp is NULL) */
    int64_t* src_read;      /* optional (may be NULL) [read_capacity]: the input index of every kept read */
    int64_t n_reads;        /* out (host form): reads kept, or needed on PV_ERR_CAPACITY */
    int64_t n_bases;        /* out (host form): bases kept, or needed */
    int64_t n_cigar;        /* out (host form): cigar words kept, or needed */
} pv_select_out;

/* Device-resident, asynchronous form: every array is a DEVICE pointer (read_hp may be NULL); n_reads, n_bases and n_cigar are
 * the lengths of the input's arrays. d_counts = {reads kept, bases kept, cigar words kept, status}. Status:
 *   PV_OK;
 *   PV_ERR_CAPACITY: a capacity is short; the three counts hold what is needed, read_off and the per-read records and offsets
 *     of the reads that fit are written, no payload (bases, quals, cigar) is written;
 *   PV_ERR_INVALID, found on the device before any payload byte is read: base_off or cigar_off decreasing or starting below
 *     0, base_off[n_reads] > n_bases or cigar_off[n_reads] > n_cigar, read_off decreasing, read_off[0] != 0 or
 *     read_off[n_regions] != n_reads; the counts are 0 and no output array is written.
 * haplotype < 1 and null required pointers are refused by the call itself. Whatever the offsets hold, nothing is read outside
 * the input arrays and nothing is written outside [0, kept total) of each output array (kept + 1 entries of base_off and
 * cigar_off). Two chunked scans over the reads (4096 per workgroup), one launch for the regions and a payload gather split
 * by 16 KB pieces of the output; no global atomics, no host synchronisation; workspace for n_reads indices. */
int pv_batch_select_hp_dev(pv_ctx* ctx, const pv_batch_in* in, const int32_t* read_hp, int64_t n_reads, int64_t n_bases,
                           int64_t n_cigar, int haplotype, pv_select_out* out, int64_t* d_counts, void* stream);
/* HOST buffers in and out; the totals come from the offset arrays, which are checked on the host first. Returns the status;
 * out->n_reads, n_bases and n_cigar hold the counts (on PV_ERR_CAPACITY what is needed; read_off is filled then too). */
int pv_batch_select_hp(pv_ctx* ctx, const pv_batch_in* in, const int32_t* read_hp, int haplotype, pv_select_out* out);

/* ---- BGZF block inflate (the BAM readers' opt-in GPU mode) ---------------------------------------------------------
 * A batch of BGZF blocks, one wavefront each: the raw-DEFLATE payloads (RFC 1951: stored, fixed and dynamic Huffman
 * blocks, any BFINAL chain) concatenated in `payload`; per block the payload offset in_off, its length clen, the gzip
 * trailer's ISIZE (<= 65536) and CRC32, and the output offset out_off. A block writes exactly isize bytes at out_off and
 * nothing outside [out_off, out_off + isize); it reads nothing outside [in_off, in_off + clen). status[i] is one of the
 * PV_BGZF_* codes below: the output length and the CRC32 are checked as the host reader checks them.
 * d_counts / counts = {bytes of the good blocks, PV_OK or PV_ERR_INVALID, first bad block (-1 if none), its status}. */
#define PV_BGZF_OK 0
#define PV_BGZF_BAD_BTYPE 1          /* BTYPE = 3 */
#define PV_BGZF_STORED_LEN 2         /* stored block: LEN != ~NLEN */
#define PV_BGZF_BAD_CODE_LENGTHS 3   /* dynamic header: over-subscribed / incomplete code, bad repeat, no end-of-block code */
#define PV_BGZF_BAD_SYMBOL 4         /* literal/length 286/287, distance 30/31, or bits that match no code */
#define PV_BGZF_DIST_TOO_FAR 5       /* a distance reaching before the block's first output byte */
#define PV_BGZF_OUTPUT_OVERFLOW 6    /* more output than isize */
#define PV_BGZF_OUTPUT_SHORT 7       /* the final block ended before isize bytes */
#define PV_BGZF_INPUT_OVERRUN 8      /* the stream needs bits past clen */
#define PV_BGZF_CRC_MISMATCH 9
#define PV_BGZF_BAD_ARGS 10          /* the block's entry lies outside the payload / output buffers or isize > 65536 */
/* Device-resident and asynchronous on `stream` (NULL = the context's own); every pointer is a DEVICE pointer. It uses no
 * context workspace, so it may run on a stream of its own while builder, RNN or other calls of the same context run on
 * theirs; two of these calls may overlap too as long as their outputs, status and d_counts arrays are distinct. A call on a
 * stream other than the context's own is not recorded in the context's event profile (pv_profile_begin), which is not
 * thread-safe; one on the context's own stream is, and then must not overlap other calls of the context. */
int pv_bgzf_inflate_dev(pv_ctx* ctx, const uint8_t* payload, int64_t payload_bytes, int64_t n_blocks, const int64_t* in_off,
                        const int32_t* clen, const int32_t* isize, const uint32_t* crc, const int64_t* out_off, uint8_t* out,
                        int64_t out_bytes, int32_t* status, int64_t* d_counts, void* stream);
/* HOST buffers in and out, staged through the context's workspace (so, like the other host forms, it must not overlap other
 * calls on the context). Bytes of `out` outside every block's range are left as they were. Returns PV_OK, or PV_ERR_INVALID
 * when a block failed (counts and status say which and why) or an argument is bad. */
int pv_bgzf_inflate(pv_ctx* ctx, const uint8_t* payload, int64_t payload_bytes, int64_t n_blocks, const int64_t* in_off,
                    const int32_t* clen, const int32_t* isize, const uint32_t* crc, const int64_t* out_off, uint8_t* out,
                    int64_t out_bytes, int32_t* status, int64_t* counts);

/* ---- BAM record decode and region clipping (the BAM readers' opt-in `--gpu_decode` mode) -----------------------------
 * From the bytes pv_bgzf_inflate_dev left in HBM to the image builder's flat batch, without the host touching a record:
 * what pvio_fill_batch (include/pepper_io.h) does on reader threads, byte for byte - records filtered by flag and MAPQ,
 * clipped to [rs, re] with the reference's rules (bam_handler.cpp:115-451), the CG:B,I long CIGAR resolved, SEQ unpacked to
 * "=ACMGRSVTWYHKDBN", the HP tag read. Two calls, because the host sizes the outputs (and decides down-sampling with
 * pvio_reservoir_indices) from the per-interval counts in between:
 *   pv_bam_scan_dev   walks every interval's records and measures them: d_iv_counts[i] = {reads kept, bases, CIGAR words,
 *                     status, virtual offset of the first offender (-1: none), detail, detail, records walked};
 *   pv_bam_fill_dev   writes the read arrays of `out` (read_pos, read_flags, read_mapq, base_off, bases, quals, cigar_off,
 *                     cigar) and read_hp for the regions the host kept: region g = interval reg_iv[g], output reads
 *                     [read_off[g], read_off[g+1]); sel_off[g] = -1 takes the interval's kept reads in record order (then
 *                     read_off[g+1] - read_off[g] must be its count), else output read k of the region is the interval's
 *                     kept read number sel[sel_off[g] + k] (the reservoir order). d_totals = {reads, bases, CIGAR words,
 *                     status}: PV_OK, PV_ERR_CAPACITY (bases / words beyond the capacities given; those reads are not
 *                     written) or PV_ERR_INVALID (an index outside the interval's kept reads).
 *                     The region arrays of `out` (ref_start .. read_off, ref) are the caller's and are not read.
 * Input (pv_bam_decode_in, every pointer a DEVICE pointer): the inflated bytes of all blocks (`data`), the block table of
 * pvio_plan_blocks with out_off made global to `data` (several reader groups may be packed: interval i uses the blocks
 * [iv_blk0[i], iv_blk1[i]) of its group, coffset ascending inside a group) and pv_bgzf_inflate_dev's per-block status, and
 * the interval table of pvio_plan_intervals (chunk virtual offsets as int64). iv_rec_off [n_intervals+1] gives every
 * interval its range of record slots; a range of (bytes of the group's blocks) / 36 + 1 slots always suffices. rec_slots =
 * iv_rec_off[n_intervals] < 2^31. Cost: the workspace takes 60 bytes per slot, so that worst-case range is about 1.7 bytes of
 * workspace per inflated byte of the group for EVERY interval of the group (26 MB for a 100 kb interval at 60x), although
 * real records are kilobytes long; a caller that knows a larger minimum record size may give fewer slots - an interval that
 * runs out of slots reports PV_BAMDEC_BAD_TABLE, nothing is overwritten.
 * Per-interval status (nothing is ever read outside `data` or outside a record's own block_size, whatever the file holds): */
#define PV_BAMDEC_OK 0
#define PV_BAMDEC_BAD_BLOCK 1     /* a block under a walked record failed to inflate; detail 0 = index of the block */
#define PV_BAMDEC_BAD_RECORD 2    /* a parse_record check: detail 1 = -1 negative l_seq, else the bytes the fields need; detail 0 = block_size */
#define PV_BAMDEC_CIGAR_LONGER 3  /* a kept CIGAR operation ends past l_seq */
#define PV_BAMDEC_BLOCK_SIZE 4    /* block_size outside [32, 2^30]; detail 0 = block_size */
#define PV_BAMDEC_PAST_PLAN 5     /* the walk needs a block that is not in the table (a record running past the planned bytes, a
                                   * chunk past the linear-index bound): not an error, the host reader takes that group */
#define PV_BAMDEC_SEEK 6          /* a chunk begins past the end of its block (the reader's "seek failed") */
#define PV_BAMDEC_BAD_TABLE 7     /* the block or interval table contradicts itself (ranges outside `data`, too few slots) */
typedef struct pv_bam_decode_in {
    const uint8_t* data;
    int64_t data_bytes;
    int64_t n_blocks;
    const int64_t *coffset, *next_coffset, *out_off; /* [n_blocks] */
    const int32_t *isize, *blk_status;               /* [n_blocks] */
    int32_t n_intervals;
    int32_t include_supplementary;
    int32_t min_mapq;
    int32_t reserved;
    const int32_t* iv_tid;                           /* [n_intervals] */
    const int64_t *iv_rs, *iv_re;                    /* [n_intervals] clip window, both ends inclusive */
    const int64_t *iv_blk0, *iv_blk1;                /* [n_intervals] block range of the interval's group */
    const int64_t* iv_chunk_off;                     /* [n_intervals+1] */
    const int64_t *chunk_beg, *chunk_end;            /* virtual offsets */
    const uint8_t* iv_dropped;                       /* [n_intervals] pvio_interval_plan.dropped */
    const int64_t* iv_rec_off;                       /* [n_intervals+1] */
    int64_t rec_slots;
    int64_t n_chunks;                                /* entries of chunk_beg / chunk_end */
} pv_bam_decode_in;
/* bytes of the caller-owned workspace `ws` (8-byte aligned) both calls take; the fill reads what the scan left there */
int64_t pv_bam_decode_ws_bytes(int64_t n_intervals, int64_t rec_slots);
/* Device-resident and asynchronous on `stream` (NULL = the context's own), like pv_bgzf_inflate_dev: no context workspace is
 * used (only `ws`), so the calls may run on a stream of their own beside builder and RNN calls of the context, and beside
 * other decodes whose ws and outputs are distinct. pv_bam_fill_dev must follow its pv_bam_scan_dev on the same stream (or
 * behind an event), with the same `in` and `ws`. No global atomics, no host synchronisation. */
int pv_bam_scan_dev(pv_ctx* ctx, const pv_bam_decode_in* in, void* ws, int64_t ws_bytes, int64_t* d_iv_counts, void* stream);
int pv_bam_fill_dev(pv_ctx* ctx, const pv_bam_decode_in* in, void* ws, int64_t ws_bytes, int32_t n_regions,
                    const int32_t* reg_iv, const int64_t* read_off, const int64_t* sel_off, const int64_t* sel, int64_t n_sel,
                    int64_t n_reads, int64_t base_capacity, int64_t cigar_capacity, const pv_batch_in* out, int32_t* read_hp,
                    int64_t* d_totals, void* stream);

/* ---- recurrent-network inference ------------------------------------------------------------ */

#define PV_PLAN_P1_LSTM 1 /* pepper_variant: 2x bi-LSTM(256) + 5xLinear(512)/SELU + Linear(3) + softmax */
#define PV_PLAN_P2_GRU 2  /* pepper polisher: bi-GRU(128) encoder+decoder + Linear(256->5), sliding 100/50 over 1000 */

/* PV_DTYPE_F32: fp32-accurate products. P1 calls below option p1_f32x6_min_batch (and every call with an explicit lstm_rows)
 * run on the f32 MFMA (== an fmaf chain). Larger P1 calls run the split-6 chain: each fp32 operand is split into three bf16
 * pieces (x = x0 + x1 + x2, exact) and a product is the six terms x0y0 + x0y1 + x1y0 + x1y1 + x0y2 + x2y0 on the bf16 MFMA
 * with fp32 accumulation (dropped terms below 2^-24 relative; byte inputs are one exact piece, three terms); cell updates,
 * biases, SELU and softmax stay fp32. Results then differ from the f32 MFMA form in the last bits (1e-6 on probabilities). */
#define PV_DTYPE_F32 0
#define PV_DTYPE_BF16_INPUT_GEMM 1 /* bf16 operands (fp32 accumulate) for the input-projection GEMMs only */

/* Weights in PyTorch state_dict layout (row-major, fp32), i.e. exactly the tensors
 * ModelHander.load_simple_model_for_training (pepper_variant/modules/python/models/ModelHander.py:18-44)
 * obtains from the checkpoint. Index [0] = forward direction, [1] = "_reverse". HOST pointers. */
typedef struct pv_rnn_dir {
    const float* w_ih; /* [G*H, K]  (G = 4 for LSTM gates i,f,g,o; 3 for GRU gates r,z,n) */
    const float* w_hh; /* [G*H, H] */
    const float* b_ih; /* [G*H] */
    const float* b_hh; /* [G*H] */
} pv_rnn_dir;

typedef struct pv_weights_p1 {
    pv_rnn_dir encoder[2]; /* LSTM(26 -> 256)  simple_model.py:23-27 */
    pv_rnn_dir decoder[2]; /* LSTM(512 -> 256) simple_model.py:28-32 */
    const float* linear_w[5]; /* linear_1 [512,16896], linear_2..5 [512,512]  simple_model.py:35-44 */
    const float* linear_b[5]; /* [512] each */
    const float* out_w;       /* output_layer_type [3,512] simple_model.py:46 */
    const float* out_b;       /* [3] */
} pv_weights_p1;

typedef struct pv_weights_p2 {
    pv_rnn_dir encoder[2]; /* GRU(10 -> 128)  pepper/modules/python/models/simple_model.py:12-16 */
    pv_rnn_dir decoder[2]; /* GRU(256 -> 128) :17-21 */
    const float* dense_w;  /* dense1 [5,256] :24 */
    const float* dense_b;  /* [5] */
} pv_weights_p2;

int pv_rnn_load_p1(pv_ctx* ctx, const pv_weights_p1* w, int dtype);
int pv_rnn_load_p2(pv_ctx* ctx, const pv_weights_p2* w, int dtype);

/* P1: images int8 [B,33,26] -> probs float [B,3] (softmax over {hom-ref, het, hom-alt}).
 * Equivalent to TransducerGRU.forward(images.float(), train_mode=False) in eval mode. */
int pv_rnn_forward_p1(pv_ctx* ctx, const int8_t* images, int64_t B, float* probs);
int pv_rnn_forward_p1_dev(pv_ctx* ctx, const int8_t* d_images, int64_t B, float* d_probs, void* stream);
/* optional taps for parity tests (device or host per the variant called): encoder/decoder outputs
 * [B,33,512]; either may be NULL */
int pv_rnn_forward_p1_debug(pv_ctx* ctx, const int8_t* images, int64_t B, float* probs,
                            float* enc_out, float* dec_out);

/* P2: images uint8 [B,1000,10] -> labels uint8 [B,1000] (argmax of the accumulated softmax) and,
 * optionally, the accumulated softmax acc float [B,1000,5] (may be NULL). Reproduces the 19-window
 * sliding loop with hidden carry of pepper/modules/python/models/predict.py:47-97. */
int pv_rnn_forward_p2(pv_ctx* ctx, const uint8_t* images, int64_t B, uint8_t* labels, float* acc);
int pv_rnn_forward_p2_dev(pv_ctx* ctx, const uint8_t* d_images, int64_t B, uint8_t* d_labels, float* d_acc,
                          void* stream);

/* P2, one model call: TransducerGRU.forward(x, hidden) (pepper/modules/python/models/simple_model.py:27-42,
 * called once per window by predict.py:65). images uint8 [B,100,10], hidden_in float [B,2,128] (NULL = zeros)
 * -> logits float [B,100,5] (before softmax), hidden_out float [B,2,128] (may be NULL). HOST pointers. */
int pv_rnn_forward_p2_window(pv_ctx* ctx, const uint8_t* images, const float* hidden_in, int64_t B, float* logits,
                             float* hidden_out);

/* ---- multi-GPU: the one exchange step ------------------------------------------------------------------------------
 * Regions shard across ranks (interval i -> rank i % world, pepper_variant/modules/python/ImageGenerationUI.py:211) with no
 * data-path collective; pv_gather moves every rank's per-window rows (probabilities, and whatever keys the caller packs next
 * to them) to ONE rank over RCCL: an all-gather of the row counts, then grouped point-to-point sends to `dst` (xGMI is
 * point-to-point: the sends of the other ranks run on different links). The reference has no counterpart (each caller process
 * writes its own prediction file, RunInference.py:101-106; its only process-group site is
 * pepper/modules/python/models/predict_distributed_gpu.py:124-129). RCCL (librccl.so.1) is opened with dlopen on first use.
 * One communicator per context; the 128-byte id is made by one rank (pv_comm_unique_id) and handed to the others by the
 * launcher (environment, file, TCP store, torch.distributed broadcast). */
typedef struct pv_comm pv_comm;
#define PV_COMM_ID_BYTES 128
int pv_comm_unique_id(pv_ctx* ctx, char* id128);
int pv_comm_create(pv_ctx* ctx, const char* id128, int rank, int world, pv_comm** out);
void pv_comm_destroy(pv_comm* comm);
/* Every rank passes its n_rows rows of row_bytes bytes (DEVICE memory). counts_out [world] (host, optional) receives the
 * per-rank row counts on every rank when the call returns; on `dst` the rows arrive rank-major in d_recv (DEVICE, capacity
 * recv_capacity_rows rows) asynchronously on `stream`; other ranks may pass NULL for d_recv.
 * The capacity test is COLLECTIVE: the counts are all-gathered together with the destination's capacity, so when the rows do
 * not fit EVERY rank returns PV_ERR_CAPACITY (counts_out filled) before any send or receive is posted - no rank is left
 * waiting for a partner that gave up. A destination that passes NULL for d_recv announces capacity 0. */
int pv_gather(pv_ctx* ctx, pv_comm* comm, const void* d_send, int64_t n_rows, int row_bytes, void* d_recv,
              int64_t recv_capacity_rows, int64_t* counts_out, int dst, void* stream);

/* The count exchange alone (one all-gather of an int64 per rank): lets the destination size its receive buffer for ragged
 * ranks before pv_gather. counts_out [world] on every rank. */
int pv_gather_counts(pv_ctx* ctx, pv_comm* comm, int64_t n_rows, int64_t* counts_out, void* stream);

/* Diagnostic (tests, tuning): C = A . W^T + bias through the 3-term split-bf16 MFMA GEMM of PV_DTYPE_BF16_INPUT_GEMM alone.
 * HOST pointers, fp32 row-major A [M,K], W [N,K], bias [N] or NULL; C [splits][M][N] row-major (quads = 0) or [M/4][N][4]
 * (quads = 1: four consecutive rows of a column adjacent, splits = 1). M % 4 == 0, N % 256 == 0, K % (32 * splits) == 0.
 * *ms (optional) receives the kernel's duration. Has no counterpart in the reference. */
int pv_debug_gemm_bf16x3(pv_ctx* ctx, const float* A, const float* W, const float* bias, int64_t M, int N, int K,
                         int splits, int quads, float* C, float* ms);
/* The same through the 6-term GEMM of the PV_DTYPE_F32 split-6 chain (A split into three bf16 pieces on the device, W on the
 * host before the upload, as the model load does), same arguments and shape rules. */
int pv_debug_gemm_bf16x6(pv_ctx* ctx, const float* A, const float* W, const float* bias, int64_t M, int N, int K,
                         int splits, int quads, float* C, float* ms);
/* The same product through k_gemm_x6_stream, the decoder projection's launch in the split-6 chain (48-row A tiles resident in
 * LDS, W streamed in the order made at load time): K = 512, N a multiple of 512 up to 2048, no split-K. C is bit-identical to
 * pv_debug_gemm_bf16x6's. */
int pv_debug_gemm_x6_stream(pv_ctx* ctx, const float* A, const float* W, const float* bias, int64_t M, int N, int K,
                            int quads, float* C, float* ms);

/* Per-kernel timing for the benchmark's roofline leg: between pv_profile_begin and pv_profile_end every
 * kernel the context launches is bracketed by HIP events on its launch stream. pv_profile_end
 * synchronises the device and returns the number of distinct kernels; names_buf receives their names
 * ('\n'-separated), ms_sum[i] / counts[i] the summed duration and launch count of kernel i. */
int pv_profile_begin(pv_ctx* ctx);
/* The same, for the kernels whose profile name starts with `prefix` only (NULL or "": all). Two events per launch put a few
 * microseconds between kernels, so a timed region that needs one kernel's launch durations brackets that kernel alone. */
int pv_profile_begin_only(pv_ctx* ctx, const char* prefix);
int pv_profile_end(pv_ctx* ctx, char* names_buf, int buf_len, float* ms_sum, int* counts, int max_kernels);

/* Small batches run in "split" kernel forms whose workgroups swap hidden state every time step (pv_rnn_forward_p1* up to
 * 1024 windows, pv_rnn_forward_p2* up to 2048 chunks); a launch needs all its workgroups resident at once, which holds
 * whenever it is chosen, except on a GPU that other work keeps busy for long stretches: a poll then gives up after a bounded
 * wait. A call in which that happened NEVER returns numbers that look like results: its last kernel overwrites the outputs
 * (P1 probabilities NaN; P2 labels 255, accumulated softmax / logits / hidden state NaN), and so does every later call on the
 * context until the host acknowledges the condition. The host-buffer entry points check for it themselves (PV_ERR_STATE, and
 * acknowledge); callers of the asynchronous *_dev forms call this at their own synchronisation points: it synchronises the
 * context's stream, acknowledges, and returns the number of polls that gave up since the last call (0 = every result is
 * good), or a negative PV_ERR_* code. A context that shares its GPU with other work sets option shared_device = 1. */
int pv_rnn_exchange_timeouts(pv_ctx* ctx);

/* Kernel-form options of a context. They replace process-environment lookups at call time: the environment only supplies
 * DEFAULTS, read once in pv_create (variable in brackets); a forward call reads the context's options and nothing else.
 *   lstm_split    [PV_LSTM_SPLIT]   1 (default) / 0: allow / never use the unit-split LSTM form (<= 1024 windows per call)
 *   lstm_rows     [PV_LSTM_ROWS]    0 auto / 16 / 32: tile form of the one-workgroup LSTM kernel (explicit: no unit split)
 *   tail_rows     [PV_TAIL_ROWS]    0 auto / 16 / 32;   head_splits [PV_HEAD_SPLITS] 0 auto / 1 / 3 / 11 / 33;   head_map [PV_HEAD_MAP] 1 / 0
 *   gru_rows      [PV_GRU_ROWS]     0 auto / 16 / 32
 *   gru_split     [PV_GRU_SPLIT]    1 / 0: allow the split GRU forms at all;   gru_usplit [PV_GRU_USPLIT] 1 / 0: the unit-split one
 *   p1_bf16_min_batch                 P1 in the PV_DTYPE_BF16_INPUT_GEMM mode: calls with fewer windows than this (default 513) run the
 *                                   fp32 kernels, which are faster there; 0 = always the bf16x3 kernels
 *   p1_f32x6_min_batch [PV_P1_F32X6_MIN_BATCH]  P1 in the PV_DTYPE_F32 mode: calls of at least this many windows (1..16777216,
 *                                   default 2048) and no explicit lstm_rows run the split-6 chain; smaller calls the f32 MFMA
 *                                   kernels, bit for bit as before. 16777216 (above any batch) turns the chain off
 *   p1_gemm6_stream                 1 (default) / 0: the split-6 chain's decoder input projection as k_gemm_x6_stream / as
 *                                   k_gemm_bf16x6; the results are the same bit for bit
 *   shared_device [PV_SHARED_DEVICE] 0 / 1: other streams or processes keep this GPU busy (e.g. several un-fused callers per
 *                                   GPU, RunInferenceArguments.py:67-74): never choose a form that needs co-resident workgroups
 *   exchange_spin_log2              2..22 (default 18): bounded polls give up after 2^n tries
 *   debug_drop_part                 -1 (off) / 0..3: diagnostic, one part of every unit-split group never runs (tests force a
 *                                   time-out with it and see the poison)
 *   realign_scratch_kb              1..4194304 (default 524288): the realigner's pool of traceback direction bytes, in KB
 * Unknown names and values outside these sets return PV_ERR_INVALID. */
int pv_set_option(pv_ctx* ctx, const char* name, int value);
int pv_get_option(pv_ctx* ctx, const char* name, int* value);

/* ---- hipGraph capture of a launch sequence ------------------------------------------------------------------------
 * Everything the *_dev entry points do is stream work with device-resident state (no host read-back, tags / counters of
 * the split forms kept on the device), so a sequence of them can be captured once and replayed:
 *     run the calls once (sizes the workspace)          pv_summarize_regions_dev(...); pv_rnn_forward_p1_dev(...);
 *     pv_graph_begin(ctx, stream);                       same calls, same pointers: recorded, not run
 *     pv_graph_end(ctx, &graph);
 *     per batch: refill the SAME input buffers, then     pv_graph_launch(graph, stream);
 * `stream` must be a created stream (NULL = the context's own; the legacy null stream cannot capture) and the one the calls
 * in between are given. A call that would have to grow the workspace inside a capture fails with PV_ERR_STATE. The
 * reference has no counterpart (its loop is eager PyTorch); BASELINE configs[4] names the technique. */
typedef struct pv_graph pv_graph;
int pv_graph_begin(pv_ctx* ctx, void* stream);
int pv_graph_end(pv_ctx* ctx, pv_graph** graph);
int pv_graph_launch(pv_graph* graph, void* stream);
void pv_graph_destroy(pv_graph* graph);

/* ---- assess: score an assembly against a truth sequence (`pepper assess`) ----------------------------------------------
 * Identity, QV and the error breakdown of a polished (or draft) assembly against a known true sequence, contig by contig.
 * Contigs are paired by the caller, in the same orientation, and taken to be colinear: no reverse complement and no
 * rearrangement is looked for. The reference has no counterpart (it leaves assessment to outside tools).
 * Constants: K = PV_ASSESS_K = 32 (anchor length), W = PV_ASSESS_W = 128 (band cells), L = `segment`. For one pair, A is the
 * assembly (n_A bytes) and B the truth (n_B bytes), both with a..z upper-cased by the caller; bytes are compared as they
 * stand, N included.
 * Anchors. For k = 1 .. floor(n_A / L) the candidates are a = k*L + 32*t, t = 0..7, while a + K <= n_A. A candidate is tried
 *   only if A[a, a+K) is ACGT-only; it is searched byte for byte in B at the start positions j in [max(0, c - max_shift),
 *   min(n_B - K, c + max_shift)], c = floor(a * n_B / n_A) in int64. The first t whose 32-mer occurs at exactly one such j
 *   gives anchor (a, j); if no t does, k has no anchor.
 * Chain. Left to right from (a_prev, b_prev) = (-K, -K): an anchor is kept iff a >= a_prev + K and b >= b_prev + K.
 * Segments. Between consecutive kept anchors: rows A[a_prev+K, a) against columns B[b_prev+K, b); the first starts at (0, 0),
 *   the last ends at (n_A, n_B). Every kept anchor contributes K matches (the `anchor` field of the segment it ends). All
 *   segments are global, both ends fixed; contig ends are not free. A pair has at most floor(n_A / L) + 1 segments.
 * Band. A segment of n rows and m columns, d = m - n. |d| > PV_ASSESS_MAX_DIFF = 96: status PV_ASSESS_SEG_UNALIGNED, counts
 *   zero, its lengths go to the unaligned totals; it is never guessed at. Else dlo = min(0, d) - floor((W - 1 - |d|) / 2);
 *   cell c of row i is column j = i + dlo + c, valid iff 0 <= j <= m. H[0][j] = j. For i >= 1: diag = H[i-1][j-1] +
 *   (A[i-1] != B[j-1]) for j >= 1; up = H[i-1][j] + 1; T = diag if diag <= up else up; H[i][j] = min(T, H[i][j-1] + 1), the
 *   direction being left iff that is strictly smaller than T, else T's own. Cells outside the band or the matrix are infinite.
 * Traceback from (n, m) by the stored directions; on row 0 every step is left. diag: a match or a substitution; up: an
 *   insertion (an assembly base the truth lacks); left: a deletion (a truth base the assembly lacks). edge = 1 iff the path
 *   visits band cell 0 or W-1. An inserted base x between truth bytes t[j-1] and t[j] (contig coordinates, each used where it
 *   exists) is hp_ins iff x equals either; a deleted truth byte t[j] is hp_del iff it equals t[j-1] or t[j+1].
 * The result is an alignment: sub + ins + del is an upper bound of the edit distance, and equals it when the optimal path
 * stays inside the band and runs through the anchors (sparse errors). `edge` and `unaligned` say when to distrust a line.
 *
 * pv_assess_dev: DEVICE pointers. A, B: the pairs' bytes, pair p at [a_off[p], a_off[p+1]) and [b_off[p], b_off[p+1]);
 * segment: a multiple of 32 in [256, 65536]; max_shift in [32, 1048576]; contigs shorter than 2^31 bytes.
 * Out: segs[seg_capacity], pair p's records at [pair_seg_off[p], pair_seg_off[p+1]) in order; pair_seg_off[n_pairs+1];
 * totals int64 [n_pairs][PV_ASSESS_TOTALS] = {segments, aligned, unaligned, with edge = 1, matches (anchors included),
 * substitutions, insertions, deletions, hp_ins, hp_del, unaligned assembly bases, unaligned truth bases, anchors kept, anchors
 * found, 0, 0}; d_counts = {records written, status, records needed, scratch bytes needed}.
 * scratch: scratch_bytes of device memory, 256-byte aligned, at least pv_assess_scratch_bytes(): the anchor and segment
 * tables and the direction bits (two per cell, 32 bytes per row, a lane's four bits of eight rows in one dword).
 * Status: null pointers, negative sizes, a segment or max_shift out of range are refused with PV_ERR_INVALID by the call
 * itself; offsets that decrease or a contig of 2^31 bytes or more are status PV_ERR_INVALID; seg_capacity below the sum of
 * floor(n_A / L) + 1, or scratch_bytes below the need, are PV_ERR_LIMIT. Under any status but PV_OK every output but d_counts
 * is poisoned: all seg_capacity records, pair_seg_off and totals hold -1 in every field. Asynchronous on `stream`, seven
 * launches, no global atomics, no host read-back. */
#define PV_ASSESS_K 32
#define PV_ASSESS_W 128
#define PV_ASSESS_MAX_DIFF 96
#define PV_ASSESS_TOTALS 16
#define PV_ASSESS_SEG_ALIGNED 0
#define PV_ASSESS_SEG_UNALIGNED 1
#define PV_ASSESS_SEG_BROKEN 2   /* the traceback left the band or the matrix: never expected; the counts are void */
typedef struct pv_assess_seg {   /* 64 bytes, little-endian */
    int64_t a_start, b_start;    /* the segment's first row / column, in contig coordinates */
    int32_t n_rows, n_cols;
    int32_t status;              /* PV_ASSESS_SEG_* */
    int32_t edge;
    int32_t match, sub, ins, del, hp_ins, hp_del;   /* of the segment's own cells (zero when unaligned) */
    int32_t anchor;              /* K if a kept anchor ends the segment, 0 for a pair's last */
    int32_t pair;
} pv_assess_seg;
int pv_assess_dev(pv_ctx* ctx, const uint8_t* A, const int64_t* a_off, const uint8_t* B, const int64_t* b_off, int64_t n_pairs,
                  int segment, int max_shift, int64_t seg_capacity, pv_assess_seg* segs, int64_t* pair_seg_off, int64_t* totals,
                  void* scratch, int64_t scratch_bytes, int64_t* d_counts, void* stream);
/* HOST buffers in and out (a_off[0] = b_off[0] = 0); the scratch is the context's own. counts[4] as d_counts above; returns the
 * status. On PV_ERR_LIMIT (seg_capacity too small; counts[2] holds the need) the outputs are poisoned as above. */
int pv_assess(pv_ctx* ctx, const uint8_t* A, const int64_t* a_off, const uint8_t* B, const int64_t* b_off, int64_t n_pairs,
              int segment, int max_shift, int64_t seg_capacity, pv_assess_seg* segs, int64_t* pair_seg_off, int64_t* totals,
              int64_t* counts);
/* bytes of scratch a batch needs, from the HOST offsets of its assemblies (negative: PV_ERR_INVALID) */
int64_t pv_assess_scratch_bytes(int64_t n_pairs, const int64_t* a_off, int segment);

/* ---- assess, the errors themselves and the calibration of a FASTQ's qualities (`pepper assess --errors / -q`) ------------
 * Anchors, chain, segments, band, tie-breaks and traceback are those of pv_assess, unchanged; segs, pair_seg_off and totals
 * are byte for byte what pv_assess_dev gives on the same inputs. What is added:
 * Error record. One per substitution, insertion and deletion that the traceback of a segment of status
 *   PV_ASSESS_SEG_ALIGNED meets; unaligned and broken segments give none. With i, j as in the traceback (the step leaves cell
 *   (i, j)), a0 = a_start, b0 = b_start, in contig coordinates:
 *     diag with unequal bytes (sub): a_pos = a0+i-1, b_pos = b0+j-1, both bases set
 *     up (ins):    a_pos = a0+i-1, b_pos = b0+j, the truth position the base stands before (may be n_B); b_base = 0
 *     left (del):  a_pos = a0+i, the assembly position the missing base would stand before (may be n_A), b_pos = b0+j-1;
 *                  a_base = 0
 *   hp is the hp_ins / hp_del test of pv_assess for that step, 0 for a substitution. A segment's records are in path order
 *   from (0, 0) to (n, m), segments in order, pairs in order: pair p's at [pair_err_off[p], pair_err_off[p+1]).
 * Qualities. Q, optional: uint8 parallel to A (the same a_off), raw Phred 0..93 without the +33. A substitution or insertion
 *   has qual = Q[a_pos]; a deletion the smaller of Q[a_pos-1] and Q[a_pos], each where it lies inside the contig (a FASTQ has
 *   no slot for a missing base: the weaker neighbour is charged), and 0 when the assembly contig is empty. Without Q, qual =
 *   255. The device form counts a byte above 93 as 93; the host form refuses it (PV_ERR_INVALID) before any launch.
 * Calibration table. qhist int64 [n_pairs][PV_ASSESS_QBINS][4] = {bases, sub, ins, del}: bases[q] counts the assembly bases
 *   of quality q inside aligned segments or kept anchors (the `anchor` bytes behind a segment, whatever its status); sub, ins
 *   and del count the error records by their qual. Over q, bases sums to the totals' match + sub + ins, and sub, ins, del to
 *   the totals' fields. Written only with Q; Q without qhist or the reverse is PV_ERR_INVALID by the call itself.
 *
 * pv_assess_errors_dev: DEVICE pointers; errs[err_capacity] aligned to 8 bytes (else PV_ERR_INVALID), pair_err_off
 * [n_pairs+1]; d_counts int64[8] = {segment records, status, slots needed, scratch needed, error records written, error
 * records needed, 0, 0}; scratch at least pv_assess_errors_scratch_bytes() (pv_assess's, plus a count and an offset per slot
 * and a partial table of 94 x 4 uint32 per slot).
 * Status, in this precedence: PV_ERR_INVALID and PV_ERR_LIMIT exactly as in pv_assess_dev; every output, the new ones
 * included, is then poisoned (-1 in every field, all err_capacity records bytes 0xFF; d_counts[4] = 0, d_counts[5] = -1).
 * Else PV_ERR_CAPACITY when err_capacity is below the records needed: every output but errs is valid, d_counts[4] = 0,
 * d_counts[5] holds the need and no error record is written (the buffer stays as it was). Asynchronous on `stream`: the seven
 * launches of pv_assess_dev and up to six more, no global atomics, no host read-back. */
#define PV_ASSESS_QBINS 94
#define PV_ASSESS_ERR_SUB 1
#define PV_ASSESS_ERR_INS 2
#define PV_ASSESS_ERR_DEL 3
typedef struct pv_assess_error {   /* 32 bytes, little-endian */
    int64_t a_pos, b_pos;          /* contig coordinates, 0-based */
    int32_t pair, segment;         /* segment = index within the pair */
    uint8_t kind;                  /* PV_ASSESS_ERR_* */
    uint8_t a_base, b_base;        /* 0 where the side has no base */
    uint8_t hp;
    uint8_t qual;                  /* 255 when Q is NULL */
    uint8_t pad[3];                /* 0 */
} pv_assess_error;
int pv_assess_errors_dev(pv_ctx* ctx, const uint8_t* A, const int64_t* a_off, const uint8_t* B, const int64_t* b_off,
                         int64_t n_pairs, int segment, int max_shift, int64_t seg_capacity, pv_assess_seg* segs,
                         int64_t* pair_seg_off, int64_t* totals, const uint8_t* Q, int64_t err_capacity, pv_assess_error* errs,
                         int64_t* pair_err_off, int64_t* qhist, void* scratch, int64_t scratch_bytes, int64_t* d_counts,
                         void* stream);
/* HOST buffers in and out, the scratch the context's own; counts[8] as d_counts. Returns the status. On PV_ERR_CAPACITY the
 * need is in counts[5], errs is untouched and every other output is filled; on PV_ERR_LIMIT all outputs are poisoned. */
int pv_assess_errors(pv_ctx* ctx, const uint8_t* A, const int64_t* a_off, const uint8_t* B, const int64_t* b_off, int64_t n_pairs,
                     int segment, int max_shift, int64_t seg_capacity, pv_assess_seg* segs, int64_t* pair_seg_off,
                     int64_t* totals, const uint8_t* Q, int64_t err_capacity, pv_assess_error* errs, int64_t* pair_err_off,
                     int64_t* qhist, int64_t* counts);
int64_t pv_assess_errors_scratch_bytes(int64_t n_pairs, const int64_t* a_off, int segment);

/* ---- assess, placement: which truth contig, strand and interval an assembly contig lies on (`pepper assess --place`) -------
 * pv_assess pairs contigs by the caller's word, in the truth's orientation, end to end. A real assembly's contigs have names
 * of their own, either strand, and each covers a piece of a chromosome. This stage decides, from content alone, where each
 * assembly contig belongs; the caller then orients the contig, slices the truth and hands the pair to pv_assess /
 * pv_assess_errors as they are. No rearrangement is looked for: one interval per contig.
 * A, a_off[n_asm+1]: the assembly contigs; B, b_off[n_truth+1]: the truth contigs; both with a..z upper-cased by the caller.
 * step: a multiple of 32 in [32, 65536]; min_hits in [1, 65535]; contigs shorter than 2^31 bytes; n_truth at most
 * PV_ASSESS_PLACE_MAX_TRUTH = 8192 (a workgroup tallies a contig's hits per truth contig and strand in LDS: 2 x 8192 uint32).
 * Keys. K = PV_ASSESS_K = 32. A 32-mer of A, C, G, T only has a 64-bit key: two bits per byte, A=0, C=1, G=2, T=3, the first
 *   byte in the highest bits; rc(x) is the key of its reverse complement. A 32-mer with any other byte has no key.
 * Samples. For assembly contig p the sample positions are a = k * step, k = 0, 1, ..., while a + K <= n_A. A sample is tried
 *   iff its 32-mer has a key x and x != rc(x) (a palindrome cannot tell the strand).
 * Occurrences are counted over every truth contig t and every j with j + K <= n_B[t] whose 32-mer has a key: f(x) is the
 *   number of (t, j) whose key is x, r(x) the number whose key is rc(x). A 32-mer never spans two truth contigs.
 * Hits. A tried sample is a hit iff f + r = 1; its record is (t, s, j) with strand s = 0 if f = 1 and s = 1 if r = 1. Its
 *   position in the oriented contig is a' = a for s = 0 and a' = n_A - K - a for s = 1. Two samples with the same key are two
 *   samples, each a hit or not on its own.
 * Decision. The contig's hits are counted per (t, s); the winner has the most, ties go to the smaller t, then to s = 0. With H
 *   the winner's count and N the number of all hits of the contig, the status is PV_ASSESS_PLACED iff H >= min_hits and
 *   2 H > N, else PV_ASSESS_UNPLACED.
 * Interval of a placed contig. Among the winner's hits, first has the smallest a' and last the largest:
 *   b_lo = clamp(j_first - a'_first, 0, n_B[t]), b_hi = clamp(j_last + (n_A - a'_last), 0, n_B[t]). If first != last and
 *   j_last <= j_first, or if b_hi <= b_lo, the status is PV_ASSESS_MISPLACED: the hits agree on a contig and a strand but not
 *   on an order. Such a contig is reported and never scored.
 * Out: one pv_assess_placement per assembly contig. An unplaced contig has truth = strand = b_lo = b_hi = -1; a misplaced one
 *   keeps what was computed. d_counts = {records written, status, first bad contig or -1, scratch bytes needed}.
 *
 * pv_assess_place_dev: DEVICE pointers; recs[n_asm] aligned to 8 bytes; scratch: scratch_bytes of device memory, 256-byte
 * aligned, at least pv_assess_place_scratch_bytes() (the contigs' sample offsets, a directory of 4097 uint32, and 56 bytes per
 * sample: two sorted table entries of key and tag, and per entry a count and a smallest position).
 * Status: null pointers, negative sizes, a step or min_hits out of range are refused with PV_ERR_INVALID by the call itself.
 * Offsets that decrease or a contig of 2^31 bytes or more are status PV_ERR_INVALID, d_counts[2] naming the first such contig
 * (assembly contig p as p, truth contig t as n_asm + t). scratch_bytes below the need, or 2^30 samples or more, are status
 * PV_ERR_LIMIT. More than PV_ASSESS_PLACE_MAX_TRUTH truth contigs, or a scratch that cannot hold even the sample offsets, are
 * PV_ERR_LIMIT too, in d_counts and as the call's own return value. Under any status but PV_OK every record is poisoned (-1 in
 * every field) and d_counts[0] = 0. With n_asm = 0 nothing is looked at: d_counts = {0, PV_OK, -1, 0}.
 * Asynchronous on `stream`, no host read-back, no dependence on the launch geometry (the counts and minima are integer
 * atomics). Launches: setup, keys, the sort, directory, the pass over the truth (workgroups of PV_ASSESS_PLACE_TILE truth
 * bytes each), decision: 5 + the sort's 1 + m + m (m + 1) / 2 with m = max(0, ceil(log2(entries)) - 11), where entries is two
 * per sample that scratch_bytes could hold (6 launches for a thousand samples, 26 for thirty thousand). */
#define PV_ASSESS_PLACE_TILE 4096
#define PV_ASSESS_PLACE_MAX_TRUTH 8192
#define PV_ASSESS_PLACED 0
#define PV_ASSESS_UNPLACED 1
#define PV_ASSESS_MISPLACED 2
typedef struct pv_assess_placement {   /* 40 bytes, little-endian */
    int64_t b_lo, b_hi;                /* the interval [b_lo, b_hi) of truth contig `truth`, in its coordinates */
    int32_t truth;                     /* index of the truth contig; -1 unless placed or misplaced */
    int32_t strand;                    /* 0: as given, 1: reverse-complemented */
    int32_t status;                    /* PV_ASSESS_PLACED / _UNPLACED / _MISPLACED */
    int32_t tried, hits, agree;        /* samples tried, hits N, hits of the winner H */
} pv_assess_placement;
int pv_assess_place_dev(pv_ctx* ctx, const uint8_t* A, const int64_t* a_off, int64_t n_asm, const uint8_t* B,
                        const int64_t* b_off, int64_t n_truth, int step, int min_hits, pv_assess_placement* recs, void* scratch,
                        int64_t scratch_bytes, int64_t* d_counts, void* stream);
/* HOST buffers in and out (a_off[0] = b_off[0] = 0; b_off holds one entry even with n_truth = 0); the scratch is the context's
 * own. counts[4] as d_counts above; returns the status. The offsets are checked on the host, with the same status, counts and
 * poison as the device form gives. */
int pv_assess_place(pv_ctx* ctx, const uint8_t* A, const int64_t* a_off, int64_t n_asm, const uint8_t* B, const int64_t* b_off,
                    int64_t n_truth, int step, int min_hits, pv_assess_placement* recs, int64_t* counts);
/* bytes of scratch a call needs, from the HOST offsets of the assembly (negative: PV_ERR_INVALID) */
int64_t pv_assess_place_scratch_bytes(int64_t n_asm, const int64_t* a_off, int step);

/* ---- kmer_qv: score an assembly by the support of its k-mers in the reads (`pepper kmer_qv`) ---------------------------------
 * Where no truth exists, a k-mer of the assembly that no read (or too few reads) contains is taken to be an error; from the
 * share of such k-mers follow an error rate and a QV, and their positions say where to look (the rule of Merqury and yak). The
 * reference has no counterpart.
 * Keys. k is odd, PV_KMER_MIN_K = 11 <= k <= PV_KMER_MAX_K = 31 (an odd k-mer is never its own reverse complement). A k-mer of
 *   upper-case A, C, G, T has a 2k-bit key: A=0, C=1, G=2, T=3, the first byte in the highest bits; rc(x) is the key of its
 *   reverse complement and canon(x) = min(x, rc(x)). A k-mer holding any other byte has no key; lower case is "other" (the
 *   caller upper-cases the assembly, as for pv_assess). A k-mer never spans two assembly contigs and never spans two reads.
 * Table. One entry per assembly position (p, i) with i + k <= n_p whose k-mer has a key. Duplicates, within a contig, across
 *   contigs or on the other strand, are entries of their own; each reports the full count of its canonical key.
 * Count. c(p, i) = min(cap, number of (read r, offset j) with j + k <= len_r whose k-mer has a key with the same canonical
 *   form), summed over every counting call made on the table since it was built; 1 <= cap <= PV_KMER_MAX_CAP = 2^30. The
 *   counters are integer atomics, and one that has reached cap is left alone (it cannot wrap): the value is exactly the one
 *   above, whatever the tile size, the workgroup count or the order of the calls. A position with i + k <= n_p whose k-mer has
 *   no key reports PV_KMER_NO_KEY.
 * Support. A keyed position is unsupported iff c < min_count, 1 <= min_count <= cap. The summary gives
 *   contig_counts int64 [n_asm][3] = {keyed positions, unsupported positions, positions without a key};
 *   segs: one int64 per `segment` bases of every contig (ceil(n_p / segment) of them, contig p's from seg_off[p]; segment a
 *     multiple of 32 in [32, 65536]): the unsupported positions that start in that segment;
 *   runs int64 [run_capacity][3] = {contig, first, last}: the maximal stretches of consecutive unsupported positions of one
 *     contig, in contig order, then by position; a position without a key ends a run;
 *   hist int64 [PV_KMER_HIST = 256]: keyed positions by count, hist[255] for c >= 255;
 *   pos_counts uint32 [summed assembly length], optional: c by flat position, PV_KMER_NO_KEY also for the last k - 1 bytes of
 *     a contig, which start no k-mer.
 *
 * pv_kmer_table_build_dev: DEVICE pointers. A, a_off[n_asm+1]: the assembly; table: table_bytes of device memory, 256-byte
 * aligned, at least pv_kmer_table_bytes() (a head, a directory of 4097 uint32 over the keys' own top 12 bits, 20 bytes per
 * assembly byte - sorted key, position, counter, gathered count - and four int64 per 2048 bytes for the run compaction).
 * d_counts int64[4] = {keyed entries, status, first bad contig or -1, table bytes needed}. Launches: setup, keys, the sort
 * (bitonic, spans of PV_KMER_SORT_SPAN entries in LDS: 1 + m + m (m + 1) / 2 launches with m = max(0, ceil(log2(entries)) -
 * 11), entries being the positions table_bytes could hold), directory.
 * pv_kmer_count_reads_dev: bases and base_off[n_reads+1] as pv_batch_in has them (a batch staged with pv_upload_batch can be
 * passed as it lies), n_bases the bytes `bases` holds, below 2^31: nothing outside them is read whatever the offsets hold. One
 * launch, workgroups of PV_KMER_TILE read bytes. On a table whose build did not end PV_OK nothing is counted.
 * pv_kmer_support_dev: a_off, n_asm as given to the build. d_counts int64[8] = {runs written, status, runs needed, segment
 * slots needed, summed assembly length (0 if the offsets decrease or it is 2^31 or more), 0, 0, 0}. Seven launches; the run list is a flag-and-scan
 * compaction, so it is ordered and takes no global atomics. May be called again after further counting calls.
 * Status. Null pointers and scalars out of range (k, cap, min_count, segment, negative sizes) are refused with PV_ERR_INVALID
 * by the call itself. Build: offsets that decrease are status PV_ERR_INVALID, d_counts[2] naming the first such contig; a
 * summed length of 2^31 or more, or table_bytes below the need, are PV_ERR_LIMIT with the need in d_counts[3] (a table too
 * small for its head is PV_ERR_LIMIT as the call's own return value, too). Support: a table that was not built with PV_OK or
 * that does not belong to these offsets, and min_count above the table's cap, are PV_ERR_INVALID; seg_capacity below the need
 * is PV_ERR_LIMIT. Under any of these every output of the summary holds -1 in every field (pos_counts PV_KMER_NO_KEY, over the
 * summed length where the offsets give one). PV_ERR_CAPACITY when run_capacity is below the runs needed: d_counts[0] = 0,
 * d_counts[2] holds the need, no run record is written and every other output is valid. Empty input (n_asm = 0, no reads) is
 * PV_OK with zero counts. Asynchronous on `stream`, no host read-back, capturable as one linear chain. */
#define PV_KMER_MIN_K 11
#define PV_KMER_MAX_K 31
#define PV_KMER_MAX_CAP (1 << 30)
#define PV_KMER_TILE 4096
#define PV_KMER_SORT_SPAN 2048
#define PV_KMER_HIST 256
#define PV_KMER_NO_KEY 0xFFFFFFFFu
int pv_kmer_table_build_dev(pv_ctx* ctx, const uint8_t* A, const int64_t* a_off, int64_t n_asm, int k, int64_t cap, void* table,
                            int64_t table_bytes, int64_t* d_counts, void* stream);
int pv_kmer_count_reads_dev(pv_ctx* ctx, void* table, int64_t table_bytes, const uint8_t* bases, const int64_t* base_off,
                            int64_t n_reads, int64_t n_bases, void* stream);
int pv_kmer_support_dev(pv_ctx* ctx, void* table, int64_t table_bytes, const int64_t* a_off, int64_t n_asm, int64_t min_count,
                        int segment, int64_t* contig_counts, int64_t* seg_off, int64_t seg_capacity, int64_t* segs,
                        int64_t run_capacity, int64_t* runs, int64_t* hist, uint32_t* pos_counts, int64_t* d_counts, void* stream);
/* HOST buffers in and out (a_off[0] = base_off[0] = 0; base_off holds one entry even with n_reads = 0): build, count this one
 * batch of reads, summarise; the table is the context's own. counts int64[8] = {runs written, status, runs needed, segment
 * slots needed, keyed entries, first bad contig or -1, table bytes needed, 0}; returns the status. The offsets are checked on
 * the host, with the status and the poison the device forms give (pos_counts is then left as it was). On PV_ERR_CAPACITY
 * `runs` is left as it was and every other output is filled. */
int pv_kmer_support(pv_ctx* ctx, const uint8_t* A, const int64_t* a_off, int64_t n_asm, const uint8_t* bases,
                    const int64_t* base_off, int64_t n_reads, int k, int64_t cap, int64_t min_count, int segment,
                    int64_t* contig_counts, int64_t* seg_off, int64_t seg_capacity, int64_t* segs, int64_t run_capacity,
                    int64_t* runs, int64_t* hist, uint32_t* pos_counts, int64_t* counts);
/* bytes of table an assembly needs, from its HOST offsets (negative: PV_ERR_INVALID) */
int64_t pv_kmer_table_bytes(int64_t n_asm, const int64_t* a_off);

/* ---- kmer_qv --completeness: the reads' k-mers that the assembly lacks ---------------------------------------------------------
 * The section above says which k-mers of the assembly the reads do not support; this one says which k-mers of the reads the
 * assembly does not hold (Merqury's completeness beside its QV). Keys, k, canonical form and "a k-mer lies inside one read" are
 * those of the section above; the assembly table is the one pv_kmer_table_build_dev makes. Restated on dicts in
 * tests/kmer_spectrum_ref.py.
 * Hash. mix is the splitmix64 finaliser on 64 bits: x ^= x >> 30; x *= 0xbf58476d1ce4e5b9; x ^= x >> 27;
 *   x *= 0x94d049bb133111eb; x ^= x >> 31.
 * Parts. A keyed read k-mer with canonical key x belongs to part (mix of x >> 32) % n_parts, 1 <= n_parts <= PV_KMER_MAX_PARTS =
 *   4096. A counting call with (part, n_parts) processes the instances of its part and ignores the rest, hits included: after one
 *   call per part over the same reads the assembly table's counters equal those of pv_kmer_count_reads_dev on these reads.
 * Reads-only table. `slots` entries, a power of two in [PV_KMER_READS_MIN_SLOTS = 1024, PV_KMER_READS_MAX_SLOTS = 2^34]: a
 *   256-byte head, keys uint64 [slots] (empty = all ones), counts uint32 [slots]; 256 + 12 slots bytes. Home slot: mix of x &
 *   (slots - 1); probing is linear, wraps at the end and tries at most PV_KMER_READS_PROBES = 1024 slots. An instance whose key
 *   is in the assembly table adds to that table as pv_kmer_count_reads_dev does. Any other instance claims or finds its key's
 *   slot (one 64-bit compare-and-swap on an empty slot; keys are never removed during a pass) and adds 1 there under the cap
 *   rule of the section above: load, add only below the cap, value = min(cap, instances). The cap is the one given to the init
 *   call: give it the build's.
 * Overflow. A key that finds no slot within the probe limit sets status PV_ERR_CAPACITY in the head and adds to a `dropped`
 *   counter. Lanes read the status once per tile; once they see it set they only count dropped instances (a full table costs a
 *   bounded amount of work, never a scan per instance). After an overflow the table's content is unspecified: only the status
 *   and dropped > 0 are promised.
 * Flush. For every occupied slot 1 is added to ro_hist[min(count, cap, 255)] (int64 [PV_KMER_HIST], accumulating over calls:
 *   the caller zeroes it once); d_counts int64[4] = {distinct keys flushed, status, dropped instances, slots}; the table is
 *   emptied and its status and dropped counter reset, so the next part can be counted. Under PV_ERR_CAPACITY ro_hist is left as
 *   it was.
 * Assembly spectrum. For every distinct key of the assembly table, with its multiplicity m (equal sorted entries) and its count
 *   c = min(cap, counter) as the summary gathers it, 1 is added to spectrum[min(m, 4) - 1][min(c, 255)] (int64 [4][PV_KMER_HIST],
 *   accumulating: the caller zeroes it). Column 0 holds the assembly k-mers that no read has. d_counts int64[2] = {distinct
 *   keys, status}.
 * Completeness at threshold s, 1 <= s <= 255, is the host's: found = the sum of spectrum[m][c] over all rows and c >= s; total =
 *   found + the sum of ro_hist[c] over c >= s; completeness = found / total.
 *
 * pv_kmer_reads_table_init_dev: rtable 256-byte aligned, rtable_bytes at least pv_kmer_reads_table_bytes of slots; one launch.
 * pv_kmer_count_reads_all_dev: pv_kmer_count_reads_dev's arguments, the reads-only table and (part, n_parts); one launch of
 * k_km_count_all, which walks the reads as k_km_count does (the tile walk of csrc/kmer_index.hpp, the tile and its halo staged
 * there, the directory in the kernel). pv_kmer_reads_flush_dev: two launches.
 * pv_kmer_spectrum_dev: two launches; the table's counters are read, not changed.
 * Status. Null pointers and scalars out of range (slots, cap, part, n_parts, negative sizes, rtable_bytes below the head or
 * below what slots need) are refused with PV_ERR_INVALID by the call itself. A reads-only table that was not initialised, or
 * whose rtable_bytes contradict its head, counts nothing and makes the flush report status PV_ERR_INVALID, {0, status, 0, 0},
 * with ro_hist untouched. An assembly table not built PV_OK counts nothing, in either table, and gives the spectrum status
 * PV_ERR_INVALID with `spectrum` untouched. Empty input is PV_OK with zeros. Asynchronous on `stream`, no host read-back,
 * capturable as one linear chain. */
#define PV_KMER_READS_MIN_SLOTS 1024
#define PV_KMER_READS_MAX_SLOTS (1ll << 34)
#define PV_KMER_READS_PROBES 1024
#define PV_KMER_MAX_PARTS 4096
/* bytes of a reads-only table of `slots` entries (negative: PV_ERR_INVALID) */
int64_t pv_kmer_reads_table_bytes(int64_t slots);
int pv_kmer_reads_table_init_dev(pv_ctx* ctx, void* rtable, int64_t rtable_bytes, int64_t slots, int64_t cap, void* stream);
int pv_kmer_count_reads_all_dev(pv_ctx* ctx, void* table, int64_t table_bytes, void* rtable, int64_t rtable_bytes,
                                const uint8_t* bases, const int64_t* base_off, int64_t n_reads, int64_t n_bases, int part,
                                int n_parts, void* stream);
int pv_kmer_reads_flush_dev(pv_ctx* ctx, void* rtable, int64_t rtable_bytes, int64_t* ro_hist, int64_t* d_counts, void* stream);
int pv_kmer_spectrum_dev(pv_ctx* ctx, void* table, int64_t table_bytes, int64_t* spectrum, int64_t* d_counts, void* stream);
/* HOST buffers in and out, as pv_kmer_support takes them: build, this one batch of reads counted part by part with a flush after
 * each, the spectrum; both tables are the context's own. spectrum int64 [4][256] and ro_hist int64 [256] are overwritten.
 * counts int64[8] = {distinct reads-only keys, status, dropped instances, slots, keyed entries, distinct assembly keys, 0, 0};
 * the status is the first of: the build's, a flush's, the spectrum's; it is returned too. Offsets that do not start at 0 or
 * decrease, and 2^31 bytes or more on either side, are refused on the host (PV_ERR_INVALID, PV_ERR_LIMIT) with the outputs left
 * as they were. */
int pv_kmer_spectrum(pv_ctx* ctx, const uint8_t* A, const int64_t* a_off, int64_t n_asm, const uint8_t* bases,
                     const int64_t* base_off, int64_t n_reads, int k, int64_t cap, int64_t slots, int n_parts, int64_t* spectrum,
                     int64_t* ro_hist, int64_t* counts);

/* bytes of device workspace the context currently holds (diagnostics) */
int64_t pv_workspace_bytes(pv_ctx* ctx);
/* library/ABI version: major*10000 + minor*100 + patch */
int pv_version(void);

#ifdef __cplusplus
}
#endif
#endif /* PEPPER_HIP_H */
