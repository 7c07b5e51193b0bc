/*
 * sfgpu.h -- C ABI of the MI355X-native Sailfish quantification core (libsfgpu.so).
 *
 * This is the drop-in boundary behind Sailfish's C++ host code: every entry point replaces one
 * seam of the reference (file:line under the reference tree given next to each declaration;
 * INTEGRATION.md shows the adaptor a maintainer would compile into `sailfish quant`).
 *
 * Conventions
 *   - plain C: opaque handles, plain pointers and sizes, int error codes, no exceptions.
 *   - pointers named d_* are DEVICE pointers (HBM of the current HIP device), h_* are HOST
 *     pointers.  All buffers are caller-owned; handles own only their internal scratch.
 *   - `stream` is a hipStream_t passed as void* (NULL = the HIP default stream).  Work is
 *     enqueued on that stream; functions documented as "synchronous" wait for it.
 *   - errors: 0 = ok, otherwise an SFGPU_ERR_* code; sfgpu_last_error() gives the text
 *     (thread-local).  Nothing here ever falls back to a CPU implementation: without a usable
 *     gfx950 device every compute entry point returns SFGPU_ERR_HIP.
 */
#ifndef SFGPU_H
#define SFGPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SFGPU_VERSION 100 /* 0.1.0 */
#define SFGPU_API __attribute__((visibility("default")))

enum {
    SFGPU_OK = 0,
    SFGPU_ERR_INVALID = 1,   /* bad argument */
    SFGPU_ERR_HIP = 2,       /* HIP runtime / device failure */
    SFGPU_ERR_NO_ACTIVE = 3, /* "no transcripts expressed" -- optimize() returns false,
                                src/CollapsedEMOptimizer.cpp:794-798 */
    SFGPU_ERR_ALPHA_SUM = 4, /* "total alpha weight was too small" -- :877-881 */
    SFGPU_ERR_RANGE = 5,     /* a size exceeds what the device layout holds (see each call) */
    SFGPU_ERR_STATE = 6,     /* call order violated (e.g. export before finish, sfgpu_samc_emit before sfgpu_samc_finish) */
    SFGPU_ERR_UNSUPPORTED = 7, /* reserved: an option of the reference this build does not implement (none at present) */
    SFGPU_ERR_FORMAT = 8,    /* malformed input (sfgpu_eq_add_text_host, sfgpu_reads_parse_host / _device, sfgpu_bgzf_inflate_host, sfgpu_gzrd_*, sfgpu_sam_parse_*, sfgpu_bam_parse_*, sfgpu_sam_collect_*, sfgpu_bam_collect_*, sfgpu_reads_write_*) */
    SFGPU_ERR_IO = 9,        /* the caller's sink refused the output (sfgpu_eqvec_write_text, sfgpu_quant_write_text, sfgpu_genes_write_text, sfgpu_sam_write_text, sfgpu_reads_write_text, sfgpu_gz_*, sfgpu_bgzw_*) */
    SFGPU_ERR_CAPACITY = 10  /* an output array of the caller is too small; the result says what is needed (sfgpu_sam_parse_*, sfgpu_bam_parse_*, sfgpu_samc_emit) */
};

typedef void* sfgpu_stream;          /* hipStream_t */
typedef struct sfgpu_eq sfgpu_eq;    /* EquivalenceClassBuilder on the device */
typedef struct sfgpu_em sfgpu_em;    /* CollapsedEMOptimizer state on the device */

SFGPU_API int sfgpu_version(void);
/* 1 in builds made with -DSFGPU_VARIANTS (tools/em_variants.sh, tools/eq_variants.sh): they also hold the kernel forms that lost their
 * measurements (the ring / quad / pipelined class build, the graph-replayed EM loops) and read the tuning switches; the product answers 0.
 * Environment switches the PRODUCT library reads (everything else is a variants-only tuning knob):
 *   SFGPU_EM_FUSED=0|1      0: sweep + update kernels per EM iteration; 1: one kernel per iteration wherever it can run
 *   SFGPU_EM_PERSIST=0      never run the EM loop as one persistent launch (also read when a problem's plan is made)
 *   SFGPU_EM_GATHER=0       phase C of the sweep scatters with LDS atomics (rounds 1 - 2) instead of the gather form
 *   SFGPU_EM_EXACT_NORM=1   VBEM: psi(sum alpha) from the summed vector instead of the constant psi(M prior + numMapped)
 *   SFGPU_EM_NO_RENUMBER=1  the EM plan keeps the caller's transcript order whatever the labels look like
 *   SFGPU_EM_COVER_SORT=1 / SFGPU_EM_COVER_CHECK=1   tests: cover lists by sorting / both forms compared
 *   SFGPU_EQ_SUBBATCH=n     reads per sub-batch of the class build; SFGPU_EQ_HOST_CHUNK=n reads per staged chunk of a host batch
 *   SFGPU_BS_LANES=n        concurrent bootstrap replicates (1 .. 8; default: 1 where a replicate's EM loop runs as one persistent launch, else 3)
 *   SFGPU_BS_PERSIST=1      several lanes keep the persistent loop (dev: they disturb each other's launches, profiles/r6_em_notes.md 4)
 *   SFGPU_EM_XBUF=pool      the persistent loop's exchange buffer in ordinary pool memory instead of uncached device memory
 *   SFGPU_EM_COOP=1         the persistent loop is launched with hipLaunchCooperativeKernel (a launch-time check of the grid's residency)
 *   SFGPU_MN_TREE=levels    the bootstrap's multinomial tree with one launch per level (tests: the two-launch form gives the same counts)
 *   SFGPU_POOL_LARGE_LIMIT_GB=g   cached device blocks >= 1 GiB kept per device
 *   SFGPU_TIMING=1          plans described on stderr */
SFGPU_API int sfgpu_has_variants(void);
SFGPU_API const char* sfgpu_last_error(void);
/* Forwarded to sopt.jointLog by the adaptor (level: 0 info, 1 warn, 2 error).  NULL = silent. */
SFGPU_API void sfgpu_set_logger(void (*log)(int level, const char* msg));
/* Scratch device memory is cached inside the library (hipMalloc/hipFree are slow and hipFree
 * synchronises the device); this returns every cached block to the driver. */
SFGPU_API int sfgpu_pool_trim(void);
/* Cached blocks of >= 1 GiB (the Gibbs sampler's chain state: 4 x nnz x chains bytes, 38 GB for 1.6 M classes and 1024
 * chains) are kept only up to this many bytes per device -- memory parked in this cache is invisible to other allocators in
 * the process (e.g. torch's).  Default: a quarter of the device's memory, at most 64 GiB (SFGPU_POOL_LARGE_LIMIT_GB overrides);
 * 0 = never cache them (every call pays the mapping: ~15 ms per GB); negative = back to the default. */
SFGPU_API int sfgpu_pool_set_large_limit(long long bytes);
/* Device name / CU count / HBM bytes of the current device (any pointer may be NULL). */
SFGPU_API int sfgpu_device_info(char* name, int name_len, int* n_cu, uint64_t* hbm_bytes);

/* ---------------------------------------------------------------------------------------------
 * a1. TranscriptGroup hash: XXH64(label bytes, 4*n, seed 0)
 *     replaces: TranscriptGroup::TranscriptGroup(std::vector<uint32_t>)  src/TranscriptGroup.cpp:9-12
 *               XXH64                                                    src/xxhash.c:346-455, 458-484
 * Packed batch: label r = d_ids[d_offsets[r] .. d_offsets[r+1]).  Asynchronous on `stream`.
 * ------------------------------------------------------------------------------------------- */
SFGPU_API int sfgpu_xxh64_labels(const uint32_t* d_ids, const uint32_t* d_offsets, uint32_t n_reads,
                       uint64_t* d_hashes, sfgpu_stream stream);

/* ---------------------------------------------------------------------------------------------
 * a2-a5. EquivalenceClassBuilder   include/EquivalenceClassBuilder.hpp:53-119
 * ------------------------------------------------------------------------------------------- */
/* ctor: reserves room for `expected_classes` (the reference reserves 1e6, :57). 0 = default. */
SFGPU_API int sfgpu_eq_create(sfgpu_eq** out, uint64_t expected_classes, sfgpu_stream stream);
SFGPU_API int sfgpu_eq_destroy(sfgpu_eq* eq);
/* start() :62 -- also clears any previous contents so a builder can be reused. */
SFGPU_API int sfgpu_eq_start(sfgpu_eq* eq);
/* addGroup() :90-108, batched: one call carries the hit lists of many reads (the reference's
 * unit is the <=1000-read parser job, src/SailfishQuantify.cpp:73,399-416,608-625).
 * label r = ids[offsets[r] .. offsets[r+1]); the ORDERED list is the key (equality ==
 * vector equality, src/TranscriptGroup.cpp:53-55); empty lists are skipped like the call
 * site's `if (txpIDs.size() > 0)` guard.  Thread-safe (calls are serialised per builder).
 * offsets are uint32: one batch holds < 2^32 ids and < 2^31 reads (else SFGPU_ERR_RANGE); a larger
 * experiment is handed over in several batches (counts are uint64 and accumulate across batches).
 * The EXPORT has the same ceiling: rowptr is uint32, so the finished table must hold < 2^32 label
 * ids in total (sum of class sizes; sfgpu_eq_export_* return SFGPU_ERR_RANGE beyond) -- ~460x the
 * 9.3 M of the 400 M-read / 200 k-transcript configuration.
 * _device reads a device-resident batch and returns after it has been folded in -- or, for a batch of fewer than 8 M
 * reads, after it has been copied (device to device) behind earlier small batches, which are built 16 M reads at a time: a
 * build costs ~0.25 ms of launches and round trips whatever its size (100 M reads in 1 M-read batches: 34 -> 17 ms).
 * _host takes the caller's (pageable or pinned) host arrays: small batches are copied into a pinned
 * accumulation buffer (thread-safe: only the reservation of the range is serialised) and built
 * 2 M reads at a time, large ones are staged directly; offsets may start at a non-zero base (the ids are
 * read from h_ids + h_offsets[0]).  Either way the caller may reuse its buffers on return, and
 * sfgpu_eq_finish() folds in whatever is still accumulated. */
SFGPU_API int sfgpu_eq_add_batch_host(sfgpu_eq* eq, const uint32_t* h_ids, const uint32_t* h_offsets, uint32_t n_reads);
SFGPU_API int sfgpu_eq_add_batch_device(sfgpu_eq* eq, const uint32_t* d_ids, const uint32_t* d_offsets, uint32_t n_reads);
/* insertGroup(TranscriptGroup, count) :82-88, batched and with upsert semantics: group g is added
 * with multiplicity d_counts[g] (equal labels accumulate).  Used to merge class tables built on
 * different GPUs; same limits and synchronisation as sfgpu_eq_add_batch_device. */
SFGPU_API int sfgpu_eq_add_weighted_device(sfgpu_eq* eq, const uint32_t* d_ids, const uint32_t* d_offsets,
                                 const uint64_t* d_counts, uint32_t n_groups);
/* loadEquivClasses (src/SailfishQuantify.cpp:1444-1494, commented out in the reference; --readEqClasses :1114): the CLASS
 * SECTION of an eq_classes.txt file -- the lines behind the header (M, C and the M names) that writeEquivCounts writes
 * (src/GZipWriter.cpp:51-92) -- parsed on the device and folded into the builder.  Each line is
 *     k \t id_1 \t ... \t id_k \t count \n
 * Strict: fields separated by single tabs, decimal digits only, k >= 1, exactly k ids, every id < n_transcripts, count < 2^64,
 * every line ends in '\n' except that the last line of the text may lack it.  Anything else (CR, spaces, an empty line or
 * field, ...) is SFGPU_ERR_FORMAT.  A label is the key exactly as written (ordered, not sorted, not deduplicated) and is folded
 * with upsert semantics through sfgpu_eq_add_weighted_device: equal labels add their counts, as insertGroup does (:82-88).
 * Counts of 2^31 and above are read and summed as uint64; the EM refuses them later (sfgpu_problem::d_counts).
 * The host text (pageable is fine) is staged through pinned memory in chunks of <= chunk_bytes bytes (0 = 32 MiB; otherwise
 * 16 .. 2^30) that end at a '\n'; a line longer than a chunk is SFGPU_ERR_RANGE.  The copy of chunk c + 1 overlaps the parse
 * of chunk c.  A chunk with an error folds nothing; chunks before it stay folded.  Synchronous; thread-safe like the other
 * add calls.  On an error `out` names the first bad line (0-based within the class section) and the kind; the text is in
 * sfgpu_last_error(). */
enum {
    SFGPU_EQTEXT_OK = 0,
    SFGPU_EQTEXT_BAD_CHAR = 1,     /* a byte that is not a digit, '\t' or '\n' (a CR of CRLF line ends included) */
    SFGPU_EQTEXT_EMPTY_FIELD = 2,  /* an empty line, or an empty field (two tabs in a row, a leading or trailing tab) */
    SFGPU_EQTEXT_BAD_K = 3,        /* k is 0, or the line does not hold exactly k ids and a count */
    SFGPU_EQTEXT_ID_RANGE = 4,     /* an id >= n_transcripts */
    SFGPU_EQTEXT_COUNT_RANGE = 5,  /* a count >= 2^64 */
    SFGPU_EQTEXT_LONG_LINE = 6     /* a line (with its '\n') longer than chunk_bytes */
};
typedef struct {
    uint64_t n_lines;     /* class lines folded */
    uint64_t n_ids;       /* label ids over those lines */
    uint64_t sum_counts;  /* sum of their counts (modulo 2^64) */
    uint64_t n_chunks;    /* chunks folded */
    uint64_t err_line;    /* 0-based class line of the first error; UINT64_MAX without one */
    int32_t err_kind;     /* SFGPU_EQTEXT_* */
    int32_t pad_;
    double stage_ms;      /* host: copies into the pinned staging buffers */
    double h2d_ms;        /* device events around the staged copies */
    double parse_ms;      /* device events around the parse kernels and scans */
    double fold_ms;       /* host clock around the folds (sfgpu_eq_add_weighted_device) */
} sfgpu_eqtext_result;
SFGPU_API int sfgpu_eq_add_text_host(sfgpu_eq* eq, const char* h_text, uint64_t n_bytes, uint64_t n_transcripts,
                                     uint64_t chunk_bytes, sfgpu_eqtext_result* out);
/* FASTA / FASTQ records parsed on the device: a piece of a transcript or read file in, the packed bases and offsets that
 * sfgpu_index_build and sfgpu_map_reads take out.  The C++ host of the reference keeps its own parsers; this
 * entry point serves hosts that have none.  The rules live in sailfish_amd/csrc/readfmt.h, in short:
 *   - h_text begins at a record start; its first byte fixes the format of the call ('>' FASTA, '@' FASTQ, else SFGPU_ERR_FORMAT
 *     at record 0).  Lines end at '\n'; one '\r' before it is dropped.
 *   - FASTQ: exactly four lines per record, the kind of a line is its index mod 4 (a quality line may begin with '@' or '+');
 *     line 0 begins with '@', line 2 with '+', the quality is as long as the sequence.  No multi-line FASTQ.
 *   - FASTA: a line that begins with '>' opens a record, all other lines up to the next one are its sequence (empty lines add
 *     nothing, a record may be empty).
 *   - bases are copied as they are (no case folding, N kept); the name is what follows '>' / '@' up to the first space or tab.
 *   - final == 0: only complete records are seen (FASTQ: the '\n' of the fourth line is there; FASTA: the next '>' line has
 *     begun).  final == 1: the last line may lack its '\n', an open FASTA record is complete, a FASTQ record with fewer than four
 *     lines is SFGPU_READS_TRUNCATED; empty lines behind the last record are allowed.
 * The call emits the longest prefix of the complete records that has at most max_reads records and at most cap_bases bases:
 * d_bases[0 .. n_bases) (16-byte aligned, else SFGPU_ERR_INVALID), d_off[0 .. n_reads] (int64, d_off[0] = 0), and, unless
 * d_name_span is NULL, (begin, length) of each name within h_text in d_name_span[2 r], [2 r + 1].  `consumed` is where the next
 * call's text begins: the caller presents h_text + consumed again with more bytes appended (carry-over is the caller's).
 * SFGPU_OK with n_reads == 0 and consumed == 0 on a text that is not final: no complete record yet, present more bytes.
 * A first record with more than cap_bases bases is SFGPU_ERR_RANGE, as is n_bytes > 2^30.  A malformed record among the
 * complete records of the text -- emitted or not -- is SFGPU_ERR_FORMAT: the smallest record wins, within it the first check
 * that fails, and nothing is emitted.  n_bytes == 0, or a text of nothing but line ends, is SFGPU_OK with no records (consumed
 * = n_bytes when final).
 * The text (pageable is fine) goes through the library's pinned double buffer in sub-chunks; the copy of sub-chunk c + 1 runs
 * while the newlines of sub-chunk c are counted; records are resolved over the whole text.  Synchronous, ordered behind the
 * work already on `stream`, thread-safe like the other text calls, no CPU path. */
enum {
    SFGPU_READS_NONE = 0,
    SFGPU_READS_FASTA = 1,
    SFGPU_READS_FASTQ = 2
};
enum {
    SFGPU_READS_OK = 0,
    SFGPU_READS_BAD_START = 1,       /* a record does not begin with '@' (or the text with neither '>' nor '@') */
    SFGPU_READS_MISSING_PLUS = 2,    /* the third line of a FASTQ record does not begin with '+' */
    SFGPU_READS_LENGTH_MISMATCH = 3, /* quality and sequence of a FASTQ record differ in length */
    SFGPU_READS_TRUNCATED = 4        /* final text: the last FASTQ record has fewer than four lines */
};
typedef struct {
    uint64_t n_reads;      /* records emitted */
    uint64_t n_bases;      /* their bases = d_off[n_reads] */
    uint64_t consumed;     /* bytes of h_text through the end of the last emitted record, its line end included */
    uint64_t n_lines;      /* lines of the text: its '\n' bytes, plus the last line of a final text */
    uint64_t error_record; /* 0-based record of the first error within this call's text; UINT64_MAX without one */
    uint64_t error_line;   /* ... and its 0-based line (TRUNCATED: the first line that is missing) */
    int32_t format;        /* SFGPU_READS_FASTA / _FASTQ */
    int32_t error_kind;    /* SFGPU_READS_* */
    double ms_copy;        /* device events around the staged host-to-device copies */
    double ms_kernels;     /* device events around the kernels and scans */
} sfgpu_reads_result;
SFGPU_API int sfgpu_reads_parse_host(const char* h_text, uint64_t n_bytes, int final, uint64_t max_reads, uint8_t* d_bases,
                                     uint64_t cap_bases, int64_t* d_off, uint64_t* d_name_span, sfgpu_reads_result* out,
                                     sfgpu_stream stream);
/* The same parse of a text that already lies in device memory (what sfgpu_bgzf_inflate_host wrote): nothing is staged and
 * ms_copy is 0.  d_text is 16-byte aligned and has room for cap_text >= round16(n_bytes + 1) + 16 bytes (else SFGPU_ERR_INVALID):
 * the call itself writes the '\n' and the zero padding behind the n_bytes of text, the text is otherwise not modified.  The
 * format is taken from the first byte (a one-byte copy back), a text of nothing but line ends is found by a reduction on the
 * device; every output and every result field is what sfgpu_reads_parse_host gives for the same bytes, name spans included
 * (they index d_text). */
SFGPU_API int sfgpu_reads_parse_device(uint8_t* d_text, uint64_t n_bytes, uint64_t cap_text, int final, uint64_t max_reads,
                                       uint8_t* d_bases, uint64_t cap_bases, int64_t* d_off, uint64_t* d_name_span,
                                       sfgpu_reads_result* out, sfgpu_stream stream);
/* The two parses with the qualities kept: d_qual (16-byte aligned, room for cap_bases bytes; NULL: exactly the calls above).  For a
 * FASTQ text the qualities of the emitted records are written so that record r's are d_qual[d_off[r] .. d_off[r + 1]) -- the bytes
 * of line 4r + 3 without its line end or the '\r' of a CRLF end, as many as the record has bases.  For a FASTA text d_qual is not
 * written.  Everything else -- the cut at max_reads / cap_bases, consumed, the errors, "a call that reports an error emits
 * nothing" -- is what the call without d_qual gives for the same bytes. */
SFGPU_API int sfgpu_reads_parse_host_q(const char* h_text, uint64_t n_bytes, int final, uint64_t max_reads, uint8_t* d_bases,
                                       uint8_t* d_qual, uint64_t cap_bases, int64_t* d_off, uint64_t* d_name_span, sfgpu_reads_result* out,
                                       sfgpu_stream stream);
SFGPU_API int sfgpu_reads_parse_device_q(uint8_t* d_text, uint64_t n_bytes, uint64_t cap_text, int final, uint64_t max_reads,
                                         uint8_t* d_bases, uint8_t* d_qual, uint64_t cap_bases, int64_t* d_off, uint64_t* d_name_span,
                                         sfgpu_reads_result* out, sfgpu_stream stream);
/* The two parses with the read names delivered on the device as well: d_names == NULL gives exactly the _q calls above (which are
 * these calls with NULLs).  Otherwise the names of the EMITTED records -- those in front of the max_reads / cap_bases cut -- are
 * written back to back to d_names[0 .. *n_name_bytes) and d_name_off[r] (64-bit, room for max_reads + 1 entries) is the exclusive
 * sum of their lengths: record r's name is d_names[d_name_off[r] .. d_name_off[r + 1]), d_name_off[0] = 0 and d_name_off[n_reads] =
 * *n_name_bytes (n_name_bytes may be NULL).  This is the (bytes, 64-bit offsets) pair sfgpu_sam_write_text and sfgpu_bam_write take
 * as read names.  A name is what d_name_span describes (up to the first space or tab, never the '\r' of a CRLF end, possibly
 * empty); spans and blob may be asked for together and agree.  d_names must be 16-byte aligned and cap_names a multiple of 16
 * (else SFGPU_ERR_INVALID): the call may write zeros up to the end of the blob's last 16-byte group.  Names that need more than
 * cap_names bytes are SFGPU_ERR_RANGE, and like every error that call emits nothing (n_reads == 0, consumed == 0); cap_names >=
 * n_bytes rounded up to 16 is always enough.  Everything else is what the _q call gives for the same bytes.  With names the call
 * waits for the device once more (the blob's size decides the range error and the gather's grid). */
SFGPU_API int sfgpu_reads_parse_host_n(const char* h_text, uint64_t n_bytes, int final, uint64_t max_reads, uint8_t* d_bases,
                                       uint8_t* d_qual, uint64_t cap_bases, int64_t* d_off, uint64_t* d_name_span, uint8_t* d_names,
                                       uint64_t cap_names, uint64_t* d_name_off, uint64_t* n_name_bytes, sfgpu_reads_result* out,
                                       sfgpu_stream stream);
SFGPU_API int sfgpu_reads_parse_device_n(uint8_t* d_text, uint64_t n_bytes, uint64_t cap_text, int final, uint64_t max_reads,
                                         uint8_t* d_bases, uint8_t* d_qual, uint64_t cap_bases, int64_t* d_off, uint64_t* d_name_span,
                                         uint8_t* d_names, uint64_t cap_names, uint64_t* d_name_off, uint64_t* n_name_bytes,
                                         sfgpu_reads_result* out, sfgpu_stream stream);
/* Do the mate files of a paired library run in step?  Two name blobs of n_reads names each (as the calls above write them; any
 * alignment) are compared read by read under the stem rule of sailfish_amd/csrc/readfmt.h: a trailing "/1" or "/2" is dropped
 * from either name, whichever digit it is, and the rest must be equal in length and bytes (x/1 ~ x/2 ~ x; x/3 is not x).
 * *first_mismatch (host) = the lowest read whose names disagree, UINT64_MAX when all agree (and for n_reads == 0).  Synchronous,
 * ordered behind the work already on `stream`. */
SFGPU_API int sfgpu_reads_names_match(const uint8_t* d_names1, const uint64_t* d_off1, const uint8_t* d_names2, const uint64_t* d_off2,
                                      uint64_t n_reads, uint64_t* first_mismatch, sfgpu_stream stream);
/* Blocked gzip (BGZF: what bgzip and the Illumina converters write) inflated on the device, one wavefront per member.  The
 * rules live in sailfish_amd/csrc/bgzfmt.h: a member is a gzip member with a 'B','C' extra subfield that holds its size, at
 * most 64 KB of payload, and no match that reaches before its first byte.
 * h_src[0 .. n_bytes) begins at a member.  The host reads the headers and trailers only and builds the member directory
 * (offset, size, offset of the payload = exclusive sum of the ISIZEs); the compressed bytes go through the library's pinned
 * double buffer in sub-chunks and the members of a sub-chunk are inflated while the next one is copied.  The call takes the
 * whole members in file order whose payloads fit in cap_bytes and writes them back to back to d_dst[0 .. n_bytes_out)
 * (any alignment: the caller may inflate behind a text it keeps); `consumed` is where the next call's input begins.  With final != 0 a trailing
 * partial member is SFGPU_BGZF_TRUNCATED, otherwise it is left for the next call.  d_dst == NULL sizes only: the directory is
 * built and `out` filled (n_members, consumed, n_bytes_out for the given cap_bytes), nothing is copied or inflated.
 * A member that fails a check is SFGPU_ERR_FORMAT with the first such member in file order and the first failed check in
 * stream order within it; d_dst is then unspecified.  No wave writes outside its member's [out_off, out_off + ISIZE).
 * n_bytes > 2^30 is SFGPU_ERR_RANGE.  Synchronous, ordered behind the work already on `stream`, no CPU path. */
enum {
    SFGPU_BGZF_OK = 0,
    SFGPU_BGZF_BAD_HEADER = 1,       /* not gzip / no BC subfield / BSIZE too small for header and trailer or not where the stream ends / ISIZE > 65536 */
    SFGPU_BGZF_TRUNCATED = 2,        /* the body ends before the end-of-block code of the final block; final: the input ends inside a member */
    SFGPU_BGZF_BAD_BLOCK_TYPE = 3,   /* BTYPE 3 */
    SFGPU_BGZF_STORED_LEN = 4,       /* LEN != ~NLEN */
    SFGPU_BGZF_BAD_CODE_LENGTHS = 5, /* a code-length set that zlib's inflate_table rejects, HLIT > 286, HDIST > 30, a bad repeat, no code for 256 */
    SFGPU_BGZF_BAD_SYMBOL = 6,       /* length symbol 286 / 287, distance symbol 30 / 31, or a code word nobody assigned */
    SFGPU_BGZF_DISTANCE_TOO_FAR = 7, /* a match reaches before the member's first byte */
    SFGPU_BGZF_SIZE_MISMATCH = 8,    /* the payload is not ISIZE bytes */
    SFGPU_BGZF_CRC_MISMATCH = 9
};
typedef struct {
    uint64_t n_members;        /* whole members taken */
    uint64_t consumed;         /* bytes of h_src through the last of them */
    uint64_t n_bytes_out;      /* their payload = the sum of their ISIZEs */
    uint64_t n_stored_blocks;  /* DEFLATE blocks by type, over all members */
    uint64_t n_fixed_blocks;
    uint64_t n_dynamic_blocks;
    uint64_t error_member;     /* 0-based first bad member of h_src in file order; UINT64_MAX without one */
    int32_t error_kind;        /* SFGPU_BGZF_* */
    int32_t pad_;
    double ms_copy;            /* device events around the staged host-to-device copies */
    double ms_kernels;         /* device events around the inflate kernels */
} sfgpu_bgzf_result;
SFGPU_API int sfgpu_bgzf_inflate_host(const void* h_src, uint64_t n_bytes, int final, uint8_t* d_dst, uint64_t cap_bytes,
                                      sfgpu_bgzf_result* out, sfgpu_stream stream);
/* ORDINARY gzip (gzip, pigz, fastq-dump --gzip: one serial DEFLATE stream per member, of any length) inflated on the device,
 * chunk by chunk.  The rules live in sailfish_amd/csrc/gzrdfmt.h.  The call's compressed bytes are cut into spans of chunk_bytes;
 * in every span but the first a FINDER looks for the first bit position at which the decoder accepts a dynamic block header
 * (a candidate; it may be false: there is no body check).  PASS A decodes from the known position and from every candidate, one
 * wavefront each, into a ring of 32768 sixteen-bit symbols in which a match that reaches before the chunk copies "byte i of my
 * predecessor's window"; a chunk stops where a block boundary is a candidate, behind a final block, or where the input ends.
 * The CHAIN follows end = next start from the known position: the chunks it reaches are the call's chunks, every other candidate
 * in front of its end is a false start whose work is discarded.  PROPAGATION resolves each chunk's window from its
 * predecessor's, PASS B decodes every chain chunk again with that window as preset dictionary and writes bytes at the chunk's
 * exact offset, and the chunks' CRC-32s are combined in order.  Behind a final block CRC-32 and ISIZE are compared and the call
 * ends (member_end = 1); the next call starts the next member, so a file of many small members costs one call per member.
 * Zero bytes behind a member are padding.
 *
 * A handle carries the stream's state from call to call: the last 32 KB emitted, the bit within the first unconsumed byte at
 * which the next block begins, the running CRC-32 and length.  sfgpu_gzrd_open: chunk_bytes = 0 takes the default (16384);
 * values below 64 are SFGPU_ERR_RANGE.
 * sfgpu_gzrd_plan_host: h_src[0 .. n_bytes) begins at the byte that holds the handle's bit position (n_bytes <= 2^30 and at
 * most 65536 spans, i.e. n_bytes <= 65536 * chunk_bytes, else SFGPU_ERR_RANGE).  The handle keeps device scratch for the emit:
 * the compressed bytes, 64 KB of ring per span (4 x the compressed bytes at the default chunk_bytes, 4 GiB at the most) and
 * 32 KB of resolved window per chain chunk; it grows to the largest call and goes back with sfgpu_gzrd_close.  It parses a member header when the handle is at one, stages the bytes, runs the finder, pass A, the chain
 * and the propagation, and fills `res` without writing any payload: the chain's longest prefix whose output fits cap_bytes.
 * need_cap != 0 says that not even the first chunk fits (its size).  n_chunks == 0 without an error and without need_cap says
 * that no block ends within these bytes: call again with more (`consumed` bytes, padding in front of a header, may be dropped).
 * A plan may be replaced by another plan; nothing advances until the emit.
 * sfgpu_gzrd_emit: pass B for the planned chunks into d_dst[0 .. n_bytes_out) (any alignment), then the trailer checks; the
 * handle advances and `res` is the plan's result with ms_emit and the final error_kind.
 * Errors are SFGPU_ERR_FORMAT with error_kind (SFGPU_BGZF_*; BAD_HEADER here: not a gzip member header, CM != 8 or a reserved
 * flag; TRUNCATED: with final != 0 the input ends inside a member) and error_offset, the byte of h_src at which the failing
 * chunk (or header) starts.  An error of the plan ends the chain in front of the failing chunk; the emit that follows writes
 * the chunks in front of it and returns the first error in stream order (DISTANCE_TOO_FAR shows in pass B only).  After an
 * error the handle is to be closed.  Both calls are synchronous and ordered behind the work already on `stream`; no CPU path. */
typedef struct sfgpu_gzrd sfgpu_gzrd;
typedef struct {
    uint64_t consumed;         /* whole bytes of h_src the caller may drop after the emit */
    uint64_t n_bytes_out;      /* payload of the planned chunks */
    uint64_t n_chunks;         /* chunks of the chain taken */
    uint64_t n_candidates;     /* spans in which the finder accepted a header */
    uint64_t n_false_starts;   /* candidates in front of the chain's end that the chain did not reach */
    uint64_t n_stored_blocks;  /* DEFLATE blocks by type in the planned chunks */
    uint64_t n_fixed_blocks;
    uint64_t n_dynamic_blocks;
    uint64_t need_cap;         /* the first chunk's payload when even that does not fit cap_bytes, else 0 */
    uint64_t error_offset;     /* UINT64_MAX without an error */
    int32_t member_end;        /* the planned chunks end a member */
    int32_t error_kind;        /* SFGPU_BGZF_* */
    double ms_copy;            /* device events around: the staged host-to-device copies, */
    double ms_find;            /* the finder, */
    double ms_decode;          /* pass A, */
    double ms_propagate;       /* the window propagation, */
    double ms_emit;            /* pass B */
} sfgpu_gzrd_result;
SFGPU_API int sfgpu_gzrd_open(sfgpu_gzrd** out, uint32_t chunk_bytes);
SFGPU_API int sfgpu_gzrd_plan_host(sfgpu_gzrd* z, const void* h_src, uint64_t n_bytes, int final, uint64_t cap_bytes,
                                   sfgpu_gzrd_result* res, sfgpu_stream stream);
SFGPU_API int sfgpu_gzrd_emit(sfgpu_gzrd* z, uint8_t* d_dst, sfgpu_gzrd_result* res, sfgpu_stream stream);
SFGPU_API int sfgpu_gzrd_close(sfgpu_gzrd* z);
/* writeEquivCounts (src/GZipWriter.cpp:77-88), the other direction: the CLASS SECTION of an eq_classes.txt file formatted on the
 * device from a class table in CSR form (the sfgpu_eq_export_device arrays, a table merged by sfgpu_eqvec_merge_disjoint, or
 * one the caller assembled).  For each class, in the order given,
 *     k \t id_1 \t ... \t id_k \t count \n
 * decimal, no padding, no sign.  The header of the file (M, C and the M names) is the host's business, as in the reader.
 * The arrays are formatted as they are: ids up to 2^32 - 1, counts up to 2^64 - 1 (20 digits), any k including 0
 * ("0 \t count \n"); nothing is checked against a transcript count.  rowptr must start at 0 and never decrease (else
 * SFGPU_ERR_INVALID); n_classes < 2^32 - 1 (SFGPU_ERR_RANGE).  The text may exceed 4 GB.
 * The text is handed to `sink` in consecutive chunks, in order.  Each chunk is a whole number of lines (it ends in '\n'), is at
 * most chunk_bytes long (0 = 32 MiB; otherwise 16 .. 2^30, else SFGPU_ERR_INVALID) and greedy: it holds as many whole lines as
 * fit, so n_chunks is a function of the table and chunk_bytes alone.  h_bytes points into a pinned staging buffer of the
 * library and is valid only during the call.  Chunk c + 1 is formatted and copied while the sink consumes chunk c (two staging
 * buffers).  All line lengths are known before a byte is formatted: a line longer than chunk_bytes fails the call with
 * SFGPU_ERR_RANGE before the first sink call (`out` holds the sizes).  A nonzero return of the sink ends the call with
 * SFGPU_ERR_IO and no further sink call.  sink == NULL sizes the text only: `out` is filled, nothing is formatted or copied.
 * n_classes == 0 is SFGPU_OK with zero bytes and no sink call.
 * Synchronous; ordered behind whatever is queued on `stream`; independent calls may run from several threads.  Scratch on the
 * device: 16 bytes per token (a table has n_ids + 2 n_classes tokens) and two chunk buffers. */
typedef int (*sfgpu_text_sink)(const char* h_bytes, uint64_t n_bytes, void* user);   /* nonzero = stop */
typedef struct {
    uint64_t n_bytes;         /* bytes of the class section */
    uint64_t n_lines;         /* = n_classes */
    uint64_t n_ids;           /* label ids over those lines (rowptr[n_classes]) */
    uint64_t n_chunks;        /* sink calls made */
    uint64_t max_line_bytes;  /* longest line, with its '\n' */
    double format_ms;         /* device events: sizing, scans, chunk plan, format kernels of all chunks */
    double d2h_ms;            /* device events around the staged copies */
    double sink_ms;           /* host clock inside the sink */
} sfgpu_eqtext_write_result;
SFGPU_API int sfgpu_eqvec_write_text(const uint32_t* d_rowptr, const uint32_t* d_ids, const uint64_t* d_counts,
                                     uint64_t n_classes, uint64_t chunk_bytes, sfgpu_text_sink sink, void* user,
                                     sfgpu_eqtext_write_result* out, sfgpu_stream stream);
/* writeAbundances (src/GZipWriter.cpp:234-245): the ROW SECTION of a quant.sf file formatted on the device from the columns where
 * they lie.  For each row, in the order given,
 *     name \t Length \t %g(eff) \t %g(tpm) \t %g(num_reads) \n
 * Length in decimal; the three doubles as printf("%g") prints them (the reference's cppformat "{}"): six significant digits,
 * correctly rounded with ties to even on the exact binary value, fixed notation for decimal exponents -4 .. 5 and d.ddddde+XX
 * otherwise, trailing zeros stripped; "inf" / "-inf", "nan" for a NaN of either sign, "-0" for -0.0.  The arithmetic is exact
 * for every double (csrc/gfmt.h): 128-bit integers for 2^-56 <= |x| < 2^127, which covers what a quant.sf holds, and a slow
 * multi-word path outside (n_slow counts its cells).  The header line of the file is the host's business.
 * Row r's name is the bytes d_names[d_name_off[r] .. d_name_off[r + 1]): copied verbatim, never inspected, of any length including
 * 0 (below 2^32 - 60, else SFGPU_ERR_RANGE).  d_name_off has n_rows + 1 entries, must start at 0 and never decrease (else
 * SFGPU_ERR_INVALID); n_rows < 2^32 - 1 (SFGPU_ERR_RANGE).  All pointers are device pointers.  The text may exceed 4 GB.
 * The text is handed to `sink` in consecutive chunks, in order.  Each chunk is a whole number of rows (it ends in '\n'), is at
 * most chunk_bytes long (0 = 32 MiB; otherwise 16 .. 2^30, else SFGPU_ERR_INVALID) and greedy: it holds as many whole rows as
 * fit, so n_chunks is a function of the table and chunk_bytes alone.  h_bytes points into a pinned staging buffer of the
 * library and is valid only during the call.  Chunk c + 1 is formatted and copied while the sink consumes chunk c (two staging
 * buffers).  All row lengths are known before a byte is formatted: a row longer than chunk_bytes fails the call with
 * SFGPU_ERR_RANGE before the first sink call (`out` holds the sizes).  A nonzero return of the sink ends the call with
 * SFGPU_ERR_IO and no further sink call.  sink == NULL sizes the text only: `out` is filled, nothing is formatted or copied.
 * n_rows == 0 is SFGPU_OK with zero bytes and no sink call.
 * Synchronous; ordered behind whatever is queued on `stream`; independent calls may run from several threads.  Scratch on the
 * device: 24 bytes per row and two chunk buffers. */
typedef struct {
    uint64_t n_bytes;         /* bytes of the row section */
    uint64_t n_rows;
    uint64_t n_chunks;        /* sink calls made */
    uint64_t max_row_bytes;   /* longest row, with its '\n' */
    uint64_t n_slow;          /* cells that left the 128-bit window */
    double format_ms;         /* device events: decode, sizing, scan, chunk plan, format kernels of all chunks */
    double d2h_ms;            /* device events around the staged copies */
    double sink_ms;           /* host clock inside the sink */
} sfgpu_quant_write_result;
SFGPU_API int sfgpu_quant_write_text(const char* d_names, const uint64_t* d_name_off, const uint32_t* d_length, const double* d_eff,
                                     const double* d_tpm, const double* d_num_reads, uint64_t n_rows, uint64_t chunk_bytes,
                                     sfgpu_text_sink sink, void* user, sfgpu_quant_write_result* out, sfgpu_stream stream);
/* aggregateEstimatesToGeneLevel (src/SailfishUtils.cpp:929-1037), the `--geneMap` step: the rows of a quant.sf folded into genes
 * on the device, from the columns where they lie (no file is read back).  Row r belongs to gene d_gene_of_row[r], an arbitrary
 * id below n_gene_ids (else SFGPU_ERR_INVALID: found on the device and reported before any output is written); ids need not be
 * dense, and a gene's rows may lie anywhere.  Output line g is the g-th gene in order of the genes' FIRST rows; d_gene_id_out[g]
 * is its id and the four double columns hold
 *     TPM, NumReads   the running sums of the gene's rows in row order, from 0.0
 *     Length, EffectiveLength   sum of length_i * frac_i and eff_i * frac_i with frac_i = tpm_i / totalTPM, where totalTPM
 *                     accumulates the RUNNING TPM sum after each row (the reference's quirk, kept) -- or frac_i = 1.0 / n when
 *                     totalTPM > denorm_min does not hold (unexpressed genes, a NaN total)
 * every gene one serial chain of IEEE additions in row order, one operation per operation of the reference and none fused
 * (csrc/genefold.h), so the doubles are the host loop's bit for bit.  as_printed = 1 folds what the reference reads from the
 * file: each of d_eff, d_tpm, d_num_reads first becomes the double strtod gives for its six-digit %g token (csrc/gfmt.h:
 * gfmt_decode -> gfmt_value, exact for every double; n_slow counts the cells that left the fast windows, none for the values a
 * quant.sf holds); as_printed = 0 folds the doubles as they are.  d_length is the integer Length column.
 * The five outputs need room for min(n_rows, n_gene_ids) entries; *out->n_genes of them are written.  n_rows < 2^32 - 1
 * (SFGPU_ERR_RANGE); n_rows == 0 is SFGPU_OK with zero genes.  All pointers are device pointers; the inputs are not modified.
 * Parallelism is across genes (one lane folds one gene), so a single gene that holds every row is folded by one lane: 0.20 s for
 * one gene of 1 000 000 rows on an MI355X (profiles/genes_probe.json); max_rows_per_gene reports the longest chain.
 * Synchronous; ordered behind whatever is queued on `stream`; independent calls may run from several threads.  Scratch on the
 * device: about 120 bytes per row. */
typedef struct {
    uint64_t n_rows;
    uint64_t n_genes;            /* output lines */
    uint64_t n_slow;             /* cells rounded through the multi-word paths (as_printed = 1) */
    uint64_t max_rows_per_gene;  /* the longest serial chain */
    double aggregate_ms;         /* device events from before the id check to after the fold: all kernels of the call and the two
                                    host round trips between them (the id check, the number of genes) */
} sfgpu_genes_result;
SFGPU_API int sfgpu_genes_aggregate(const uint32_t* d_gene_of_row, const uint32_t* d_length, const double* d_eff, const double* d_tpm,
                                    const double* d_num_reads, uint64_t n_rows, uint64_t n_gene_ids, int as_printed,
                                    uint32_t* d_gene_id_out, double* d_length_out, double* d_eff_out, double* d_tpm_out,
                                    double* d_num_reads_out, sfgpu_genes_result* out, sfgpu_stream stream);
/* The ROW SECTION of a quant.genes.sf file (src/SailfishUtils.cpp:1018-1031) formatted on the device.  For each row, in order,
 *     name \t %g(length) \t %g(eff) \t %g(tpm) \t %g(num_reads) \n
 * all four numeric columns doubles (the outputs of sfgpu_genes_aggregate).  Row g's name is entry d_gene_id[g] of a name table of
 * n_gene_ids names: the bytes d_names[d_name_off[i] .. d_name_off[i + 1]), i = d_gene_id[g]; an index that is not below
 * n_gene_ids is SFGPU_ERR_INVALID.  d_name_off has n_gene_ids + 1 entries.  The comment and header lines of the file are the
 * host's business.  In every other respect the contract is sfgpu_quant_write_text's (the same kernels, csrc/rowtext.h): names
 * of any length copied verbatim, whole-row greedy chunks and the chunk_bytes rules, sink == NULL sizes only, a sink refusal is
 * SFGPU_ERR_IO, a row longer than chunk_bytes is SFGPU_ERR_RANGE before the first sink call, n_rows == 0 is SFGPU_OK with no
 * sink call; the result carries n_slow, max_row_bytes and the three times.  Scratch: 28 bytes per row and two chunk buffers. */
SFGPU_API int sfgpu_genes_write_text(const char* d_names, const uint64_t* d_name_off, uint64_t n_gene_ids, const uint32_t* d_gene_id,
                                     const double* d_length, const double* d_eff, const double* d_tpm, const double* d_num_reads,
                                     uint64_t n_rows, uint64_t chunk_bytes, sfgpu_text_sink sink, void* user,
                                     sfgpu_quant_write_result* out, sfgpu_stream stream);
/* readTranscriptToGeneMap / transcriptGeneMapFromGTF (src/SailfishUtils.cpp:322-507) and TranscriptGeneMap::findTranscriptID: the
 * `--geneMap` file read on the device and joined to the transcript names there.  What the two forms of the file say is stated
 * once, serially, in csrc/gtffmt.h (the rules of genes.TranscriptGeneMap.from_gtf / .from_file); the kernels are csrc/genemap.hip.
 * A map is built from many text blocks, so it is a handle:
 *   open     kind = SFGPU_GMAP_GTF (records of 9 tab-separated columns; key[0 .. key_len) names the attribute that groups
 *            transcripts, any bytes, "gene_id" in the reference's default) or SFGPU_GMAP_TSV (`transcript gene` token pairs; the
 *            key is ignored and may be NULL).
 *   add_text_host / _device   the conventions of sfgpu_reads_parse_host / _device: the text begins at a line start, whole lines
 *            are consumed (`consumed` = one past the last '\n'; with final != 0 everything, a last line without '\n' included) and
 *            the caller carries the tail in front of the next block.  n_bytes <= 2^30 (SFGPU_ERR_RANGE); a text without any '\n'
 *            that is not final is SFGPU_ERR_RANGE with consumed = 0 (a line longer than the block: present more).  The device form
 *            wants d_text 16-byte aligned with cap_text >= round16(n_bytes + 1) + 16 bytes (else SFGPU_ERR_INVALID) and writes into
 *            that slack.  The names of the records are compacted into storage of the handle: the text is not needed after the call.
 *            needs_host != 0 (SFGPU_GMAP_HOST_* bits) says that the consumed text holds something the device rules do not parse --
 *            a byte >= 0x80, a NUL, a '\r' not followed by '\n', a name longer than 256 bytes; nothing of that text is stored then,
 *            the handle stays flagged and finish reports the same bits: the caller reads the file with the host reader.
 *   finish   sorts the transcripts bytewise (stable, so a GTF transcript takes the value of its first record in file order that
 *            carries the key, and equal names of a two-column map keep file order), removes the duplicate ids of a GTF, numbers
 *            the genes by first appearance (GTF: in sorted transcript order; two-column: in file order) and builds the tables.
 *            More than 2^32 - 1 records is SFGPU_ERR_RANGE (raised by the add call that passes it).
 *   export   copies the tables to the caller's device arrays: d_tnames / d_tname_off[n_transcripts + 1] the sorted transcript
 *            names back to back, d_t2g[n_transcripts], d_gnames / d_gname_off[n_genes + 1] the gene names in id order (the layout
 *            sfgpu_genes_write_text takes).  Any pointer may be NULL.
 *   lookup   findTranscriptID for every row: lower_bound (bytewise, a prefix first) of the row's name d_names[d_name_off[r] ..
 *            d_name_off[r + 1]) in the sorted transcript names, with NO equality test; d_gene_of_row[r] = t2g[position], or
 *            0xFFFFFFFF past the last name (such rows are counted in *n_past: the transcript is "its own gene").
 *   from_host   a finished handle from tables the host reader built (what the caller does with a needs_host file): names back to
 *            back with n + 1 offsets each (host arrays; t2g[i] < n_genes, the transcript names sorted bytewise, else
 *            SFGPU_ERR_INVALID), so that lookup and export serve either kind of map.
 * export and lookup before finish, add after it, and finish on a flagged handle are SFGPU_ERR_STATE.  All calls are synchronous and
 * ordered behind the work already on `stream`; one handle is used from one thread at a time.  No CPU path. */
typedef struct sfgpu_gmap sfgpu_gmap;
enum {
    SFGPU_GMAP_GTF = 0,
    SFGPU_GMAP_TSV = 1
};
enum {
    SFGPU_GMAP_HOST_HIGH_BYTE = 1,
    SFGPU_GMAP_HOST_NUL = 2,
    SFGPU_GMAP_HOST_LONE_CR = 4,
    SFGPU_GMAP_HOST_LONG_NAME = 8
};
typedef struct {
    uint64_t n_lines;      /* lines consumed by this call */
    uint64_t n_records;    /* GTF: records (lines with a transcript_id) stored; two-column: tokens stored */
    uint64_t consumed;     /* bytes of the text the caller may drop */
    uint32_t needs_host;   /* SFGPU_GMAP_HOST_* bits */
    uint32_t pad_;
    double ms_copy;        /* device events around the staged host-to-device copies (0 for the device form) */
    double ms_kernels;     /* device events around the kernels and scans of the call */
} sfgpu_gmap_add_result;
typedef struct {
    uint64_t n_records;       /* GTF records / two-column pairs the map is built from */
    uint64_t n_transcripts;
    uint64_t n_genes;
    uint64_t tname_bytes;     /* sizes of the two name blobs */
    uint64_t gname_bytes;
    uint32_t needs_host;
    uint32_t sort_rounds;     /* 8-byte refinement rounds of the transcript sort */
    double ms_kernels;
} sfgpu_gmap_result;
SFGPU_API int sfgpu_gmap_open(sfgpu_gmap** out, int kind, const char* key, uint32_t key_len);
SFGPU_API int sfgpu_gmap_from_host(sfgpu_gmap** out, const char* h_tnames, const uint64_t* h_tname_off, const uint32_t* h_t2g,
                                   uint64_t n_transcripts, const char* h_gnames, const uint64_t* h_gname_off, uint64_t n_genes);
SFGPU_API int sfgpu_gmap_add_text_host(sfgpu_gmap* m, const char* h_text, uint64_t n_bytes, int final, sfgpu_gmap_add_result* res,
                                       sfgpu_stream stream);
SFGPU_API int sfgpu_gmap_add_text_device(sfgpu_gmap* m, uint8_t* d_text, uint64_t n_bytes, uint64_t cap_text, int final,
                                         sfgpu_gmap_add_result* res, sfgpu_stream stream);
SFGPU_API int sfgpu_gmap_finish(sfgpu_gmap* m, sfgpu_gmap_result* res, sfgpu_stream stream);
SFGPU_API int sfgpu_gmap_export(sfgpu_gmap* m, char* d_tnames, uint64_t* d_tname_off, uint32_t* d_t2g, char* d_gnames,
                                uint64_t* d_gname_off, sfgpu_stream stream);
SFGPU_API int sfgpu_gmap_lookup(sfgpu_gmap* m, const char* d_names, const uint64_t* d_name_off, uint64_t n_rows,
                                uint32_t* d_gene_of_row, uint64_t* n_past, sfgpu_stream stream);
SFGPU_API int sfgpu_gmap_close(sfgpu_gmap* m);
/* A mapper's SAM text (what `rapmap quasimap -o`, bowtie2 or bwa write against a transcriptome) turned into the sfgpu_hit records and
 * read offsets that sfgpu_filter_hits and sfgpu_sample_bias take, on the device.  What a SAM file says to this library is stated once,
 * serially, in csrc/samfmt.h (the rules of samfile.read_sam_host: fields, flags, CIGAR, groups, pairs, order); the kernels are
 * csrc/samtext.hip.  In short: lines with byte-equal QNAME that follow each other are one fragment (name-grouped files, as mappers
 * write them; nothing is stripped from a name); '@' lines are counted and skipped; 0x4 / 0x800 lines yield no record; a mapped 0x40
 * line directly followed by a mapped 0x80 line on the same transcript is a PAIRED_END_PAIRED record (frag_len = max end - min start,
 * TLEN is not read), a fragment with a pair yields only its pairs, otherwise its mapped lines are orphans (left run, right run) or,
 * single end, status-0 records; each run ascending in tid, ties in file order.  pos = POS - 1 - the leading soft clip.
 *   open     d_names / d_name_off[M + 1]: the transcript names in index order, back to back (device arrays, copied into the handle);
 *            RNAME is looked up in an XXH64 table of them with a byte compare behind every hash match.  A name that occurs twice is
 *            SFGPU_ERR_INVALID.  paired != 0: the paired-end rules.  M < 2^32 - 1.
 *   parse_host / _device   the conventions of sfgpu_gmap_add_text_host / _device: the text begins at a line start, n_bytes <= 2^30
 *            (SFGPU_ERR_RANGE), the device form wants d_text 16-byte aligned with cap_text >= round16(n_bytes + 1) + 16 bytes (else
 *            SFGPU_ERR_INVALID) and writes into that slack; with final != 0 a last line without '\n' is read as if it had one.  The
 *            last fragment of a text that is not final is held back (the next line may carry its name): `consumed` ends in front of
 *            its first line, and consumed == 0 with n_reads == 0 means "present more".  Output: d_hits[0 .. n_hits), d_off[0 ..
 *            n_reads] (uint32, d_off[0] = 0 in every call).  n_hits > cap_hits or n_reads > cap_reads is SFGPU_ERR_CAPACITY with
 *            need_hits / need_reads set and nothing written: call again with room (d_off holds cap_reads + 1 entries).  A malformed
 *            line among the lines the call looked at (held back or not) is SFGPU_ERR_FORMAT: `bad` is the SFGPU_SAM_BAD_* bit of the
 *            first rule the LOWEST such line breaks (in the order of the bits), bad_line its index in this text; nothing is written.
 * All calls are synchronous and ordered behind the work already on `stream`; one handle is used from one thread at a time.  No CPU path. */
typedef struct sfgpu_sam sfgpu_sam;
struct sfgpu_hit;          /* (defined with sfgpu_filter_hits below) */
enum {
    SFGPU_SAM_BAD_FIELDS = 1,   /* fewer than 11 tab-separated fields (an empty line included) */
    SFGPU_SAM_BAD_NUMBER = 2,   /* FLAG is not 1-5 digits <= 65535; POS of a mapped line is not 1-10 digits in 1 .. 2^31 - 1 */
    SFGPU_SAM_BAD_FLAG = 4,     /* paired call: 0x1 missing, or not exactly one of 0x40 / 0x80; single-end call: 0x1 set */
    SFGPU_SAM_BAD_RNAME = 8,    /* a mapped line names no transcript of the handle */
    SFGPU_SAM_BAD_CIGAR = 16,   /* neither '*' nor a run of (1-9 digits, one of MIDNSHP=X) */
    SFGPU_SAM_BAD_LENGTH = 32,  /* the read is longer than 65535 bases, or SEQ and CIGAR disagree about its length */
    SFGPU_SAM_BAD_QNAME = 64    /* sfgpu_sam_collect_* only: QNAME is longer than 254 bytes; in a paired call PNEXT of a mapped line
                                   that is not 1-10 digits in 0 .. 2^31 - 1 is BAD_NUMBER there */
};
typedef struct {
    uint64_t n_lines;      /* lines consumed by this call, header lines included */
    uint64_t n_header;     /* '@' lines among them */
    uint64_t n_reads;      /* fragments (groups) emitted */
    uint64_t n_hits;       /* records emitted */
    uint64_t n_pairs;      /* PAIRED_END_PAIRED records among them */
    uint64_t consumed;     /* bytes of the text the caller may drop */
    uint64_t need_hits;    /* SFGPU_ERR_CAPACITY: the sizes the call needs */
    uint64_t need_reads;
    uint64_t bad_line;     /* SFGPU_ERR_FORMAT: the lowest malformed line (0-based, in this text) */
    uint32_t bad;          /* ... and its SFGPU_SAM_BAD_* bit */
    uint32_t pad_;
    double ms_copy;        /* device events around the staged host-to-device copies (0 for the device form) */
    double ms_kernels;     /* device events around the kernels, scans and the sort of the call */
} sfgpu_sam_result;
SFGPU_API int sfgpu_sam_open(sfgpu_sam** out, const char* d_names, const uint64_t* d_name_off, uint64_t M, int paired, sfgpu_stream stream);
SFGPU_API int sfgpu_sam_parse_host(sfgpu_sam* s, const char* h_text, uint64_t n_bytes, int final, struct sfgpu_hit* d_hits, uint64_t cap_hits,
                                   uint32_t* d_off, uint64_t cap_reads, sfgpu_sam_result* res, sfgpu_stream stream);
SFGPU_API int sfgpu_sam_parse_device(sfgpu_sam* s, uint8_t* d_text, uint64_t n_bytes, uint64_t cap_text, int final, struct sfgpu_hit* d_hits,
                                     uint64_t cap_hits, uint32_t* d_off, uint64_t cap_reads, sfgpu_sam_result* res, sfgpu_stream stream);
SFGPU_API int sfgpu_sam_close(sfgpu_sam* s);
/* The same records from a mapper's BAM file (`samtools view -b` of what the mapper wrote; grouped by read name).  The caller hands over
 * the INFLATED stream (what sfgpu_bgzf_inflate_host wrote, or gzip on the host) in consecutive texts; what it says is stated once,
 * serially, in csrc/bamfmt.h (the rules of samfile.read_bam_host), the kernels are csrc/bamtext.hip.  It is the SAM rule set with the
 * text syntax taken away, with the same SFGPU_SAM_BAD_* bits: FIELDS is a block_size below 32 or below what l_read_name, n_cigar_op
 * and l_seq need, an empty name or one without its NUL, or a final text that ends inside a record; NUMBER a mapped record whose pos is
 * outside 0 .. 2^31 - 2; RNAME a refID outside the header's references or a reference that is no name of the handle; CIGAR an op
 * code above 8; FLAG and LENGTH as in SAM (l_seq == 0 is SEQ '*', n_cigar_op == 0 is CIGAR '*').  Groups, pairs and the record
 * order are SAM's.  A record's start is known only from the block_size in front of it: that chain is resolved exactly and in
 * parallel (exit pointers per tile of the text by pointer doubling in LDS, then supertiles), never guessed.
 *   open     d_names / d_name_off[M + 1] as in sfgpu_sam_open (the same table); d_ref_names / d_ref_off[n_ref + 1]: the header's
 *            reference names in refID order, back to back (device arrays); they are joined to the names on the device, a reference
 *            that is no transcript of the run makes the records on it BAD_RNAME.  header_bytes: the length of the binary header
 *            ("BAM\1" .. the last l_ref) in the inflated stream.
 *   parse_host / _device   the argument lists, limits, alignment and slack of sfgpu_sam_parse_host / _device.  The text of a call
 *            begins at stream offset = the sum of the `consumed` values this handle has returned; the call skips
 *            max(0, header_bytes - that sum) bytes itself, so a header larger than a text needs no special call.  A record that the
 *            text does not hold whole, and everything behind it, is not looked at unless final != 0.  The last group of a text
 *            that is not final is held back, and such a call that emits no group consumes nothing (consumed == 0, n_reads == 0:
 *            "present more").  In the result n_lines counts the alignment records consumed, n_header is 0, bad_line is the 0-based
 *            index of the lowest malformed record among the records of this text.  SFGPU_ERR_CAPACITY and SFGPU_ERR_FORMAT as
 *            in sfgpu_sam_parse_*: nothing is written and nothing consumed.
 * All calls are synchronous and ordered behind the work already on `stream`; one handle is used from one thread at a time.  No CPU path. */
typedef struct sfgpu_bam sfgpu_bam;
SFGPU_API int sfgpu_bam_open(sfgpu_bam** out, const char* d_names, const uint64_t* d_name_off, uint64_t M, const char* d_ref_names,
                             const uint64_t* d_ref_off, uint64_t n_ref, uint64_t header_bytes, int paired, sfgpu_stream stream);
SFGPU_API int sfgpu_bam_parse_host(sfgpu_bam* b, const char* h_text, uint64_t n_bytes, int final, struct sfgpu_hit* d_hits, uint64_t cap_hits,
                                   uint32_t* d_off, uint64_t cap_reads, sfgpu_sam_result* res, sfgpu_stream stream);
SFGPU_API int sfgpu_bam_parse_device(sfgpu_bam* b, uint8_t* d_text, uint64_t n_bytes, uint64_t cap_text, int final, struct sfgpu_hit* d_hits,
                                     uint64_t cap_hits, uint32_t* d_off, uint64_t cap_reads, sfgpu_sam_result* res, sfgpu_stream stream);
SFGPU_API int sfgpu_bam_close(sfgpu_bam* b);
/* The COLLATED reading of the same files: for a SAM or BAM file whose lines stand in any order -- a position-sorted file, what
 * `samtools sort` leaves -- where sfgpu_sam_parse_* / sfgpu_bam_parse_* would see every line as a fragment of its own.  The alignment
 * lines of the WHOLE file are collected on the device as fixed-size line records plus their names; after the last text they are
 * grouped by QNAME exactly (a string sort over the name bytes: equal ranks are byte-equal names, nothing is hashed), paired through
 * their mate fields, and emitted in slices as the (d_hits, d_off) batches the name-grouped readers give.  The rules are stated
 * once, serially, in csrc/samcfmt.h (those of samfile.read_sam_collated_host / read_bam_collated_host); the kernels are
 * csrc/samcollate.hip, behind the line front ends of the name-grouped readers (csrc/samfront.h, csrc/bamfront.h).  In short: ALL
 * non-header lines with byte-equal QNAME are one fragment, numbered by their first lines, lines in file order inside; in a paired
 * call a mapped line also has RNEXT and PNEXT read and NAMES A MATE iff FLAG lacks 0x8, RNEXT is "=" or its RNAME, and PNEXT >= 1 (BAM:
 * next_refID == refID, next_pos >= 0); lines a (0x40) and b (0x80) of a fragment pair when both are mapped on one transcript, both
 * name a mate, a.PNEXT == b.POS and b.PNEXT == a.POS (the written POS); among lines with one (transcript, POS of mate 1, POS of
 * mate 2) the i-th 0x40 line in file order pairs with the i-th 0x80 line.  What a fragment yields and the record order are
 * sfgpu_sam_parse_*'s.
 *   samc_open   an empty collection; paired != 0: the paired-end rules.
 *   sam_collect_host / _device, bam_collect_host / _device   one text of the file, through the parser handle `s` / `b` that holds the
 *            transcript names (its `paired` must be the collection's, else SFGPU_ERR_INVALID).  The text conventions are those of
 *            sfgpu_sam_parse_* / sfgpu_bam_parse_*: alignment, slack, n_bytes <= 2^30, `final`, the BAM header skipped through the
 *            handle's stream position.  Nothing is held back: `consumed` ends behind the last complete line or record, consumed == 0
 *            means "present more".  Per non-header line 32 bytes and the QNAME's bytes are appended (the arrays grow by doubling);
 *            the result's n_lines / n_header count the lines consumed, n_reads, n_hits and n_pairs stay 0.  A malformed line is
 *            SFGPU_ERR_FORMAT with bad / bad_line as in sfgpu_sam_parse_* (lowest line, first rule; SFGPU_SAM_BAD_QNAME is the last
 *            rule), and nothing of that call is appended.  2^32 - 1 lines or more in one collection is SFGPU_ERR_RANGE.
 *   samc_finish   groups, orders and pairs: rank refinement over the names in rounds of 8 bytes (sort_rounds of them, at most 32),
 *            one stable sort by (first line of the fragment, file order), two by (fragment, transcript, POS of mate 1, POS of mate
 *            2, side) over the lines that name a mate.  `info` says what the collection holds; state_bytes is the device memory the
 *            handle keeps from here on.
 *   samc_emit   the fragments [first_read, first_read + n_reads) of the collection: d_hits[0 .. n_hits), d_off[0 .. n_reads] (uint32,
 *            d_off[0] = 0 in every call); the result's n_reads, n_hits, n_pairs and ms_kernels are the slice's.  n_hits > cap_hits is
 *            SFGPU_ERR_CAPACITY with need_hits set and nothing written; a slice that reaches beyond the collection's fragments is
 *            SFGPU_ERR_RANGE.
 * collect after finish, finish twice, and emit before finish are SFGPU_ERR_STATE.  All calls are synchronous and ordered behind the
 * work already on `stream`; one handle is used from one thread at a time.  No CPU path. */
typedef struct sfgpu_samc sfgpu_samc;
typedef struct {
    uint64_t n_lines;      /* alignment lines collected (header lines are not) */
    uint64_t n_reads;      /* fragments */
    uint64_t n_hits;       /* records all fragments yield */
    uint64_t n_pairs;      /* PAIRED_END_PAIRED records among them */
    uint64_t state_bytes;  /* device memory held by the handle */
    uint32_t sort_rounds;  /* rounds of the name sort */
    uint32_t pad_;
    double ms_collect;     /* device events around the kernels of all collect calls */
    double ms_finish;      /* ... and of finish */
} sfgpu_samc_info;
SFGPU_API int sfgpu_samc_open(sfgpu_samc** out, int paired, sfgpu_stream stream);
SFGPU_API int sfgpu_sam_collect_host(sfgpu_sam* s, sfgpu_samc* c, const char* h_text, uint64_t n_bytes, int final, sfgpu_sam_result* res,
                                     sfgpu_stream stream);
SFGPU_API int sfgpu_sam_collect_device(sfgpu_sam* s, sfgpu_samc* c, uint8_t* d_text, uint64_t n_bytes, uint64_t cap_text, int final,
                                       sfgpu_sam_result* res, sfgpu_stream stream);
SFGPU_API int sfgpu_bam_collect_host(sfgpu_bam* b, sfgpu_samc* c, const char* h_text, uint64_t n_bytes, int final, sfgpu_sam_result* res,
                                     sfgpu_stream stream);
SFGPU_API int sfgpu_bam_collect_device(sfgpu_bam* b, sfgpu_samc* c, uint8_t* d_text, uint64_t n_bytes, uint64_t cap_text, int final,
                                       sfgpu_sam_result* res, sfgpu_stream stream);
SFGPU_API int sfgpu_samc_finish(sfgpu_samc* c, sfgpu_samc_info* info, sfgpu_stream stream);
SFGPU_API int sfgpu_samc_emit(sfgpu_samc* c, uint64_t first_read, uint64_t n_reads, struct sfgpu_hit* d_hits, uint64_t cap_hits, uint32_t* d_off,
                              sfgpu_sam_result* res, sfgpu_stream stream);
SFGPU_API int sfgpu_samc_close(sfgpu_samc* c);
/* The other direction (what `rapmap quasimap -o` offers): the ALIGNMENT LINES of a SAM file formatted on the device from one batch of
 * hit records in CSR form, as sfgpu_map_reads and sfgpu_sam_parse_* leave it.  What the lines say is stated once, serially, in
 * csrc/samwfmt.h (the bytes of samfile._sam_text); the kernels are csrc/samtext_write.hip.  In short, per read in order: a pair
 * record (mate_status 3) gives its 0x40 and its 0x80 line, any other record one line (orphans with 0x8, single-end records
 * without 0x1), 0x100 from the read's second record on; a read without records gives 77 / 141 (paired != 0) or one 4 line.
 * MAPQ 255, CIGAR <len>M or <clip>S<rest>M, QUAL '*'; SEQ is written as given, also on 0x10 lines.  The @HD / @SQ header is the
 * host's business.
 * The batch is one sfgpu_samw_batch of device pointers, the same for every destination: sfgpu_sam_write_text (a sink),
 * sfgpu_sam_write_bgzf (a BGZF handle) and sfgpu_bamsort_collect (a sorted record store); batch == NULL is SFGPU_ERR_INVALID.
 * Brace-initialise it: a group below left NULL (0) is not written, and every byte is then what it is without that group.
 *   hits / hit_off[n_reads + 1]   the batch (uint32 offsets, starting at 0, never decreasing, else SFGPU_ERR_INVALID).  paired
 *            decides what a read without records gives and whether mate 2 is read.
 *   ref_names / ref_name_off[n_refs + 1]   the transcript names back to back, uint64 offsets (quantfile.names_blob).
 *   qnames / qname_off[n_reads + 1]   the read names, likewise; qname_off == NULL: read r is named r<read_index_base + r>.
 *   seq1 / seq1_off[n_reads + 1]   the bases of mate 1 (of the reads, single end) back to back with int64 offsets, as
 *            sfgpu_reads_parse_* and sfgpu_map_reads take them; seq1_off == NULL: SEQ is '*'.  seq2 / seq2_off: mate 2, read
 *            only when paired != 0.  Names and bases are copied verbatim, never inspected, of any length including 0.
 *   qual1 / qual2   the qualities of mate 1 / mate 2 (qual2 read only when paired != 0): bytes back to back that share the
 *            mate's base offsets, so quality r is qual1[seq1_off[r] .. seq1_off[r + 1]).  NULL: QUAL is '*'.  Qualities of a
 *            mate whose bases are not given (seq?_off == NULL) are SFGPU_ERR_INVALID.  QUAL is those bytes on every line that
 *            carries the mate's SEQ, 0x100 lines and the lines of record-less reads included; a read of 0 bases has an empty QUAL.
 *            (A 1-base read whose quality byte is '*' reads as "no qualities": the format's ambiguity, written as it is.)
 *            BAM: QUAL is the quality bytes - 33 (0xff without qualities).
 *   oriented != 0   a line whose FLAG has 0x10 stores SEQ and QUAL on the reference's strand, as the SAM specification has it: SEQ
 *            reverse-complemented (A<->T, C<->G, U->A, R<->Y, K<->M, B<->V, D<->H, either case kept, every other byte as it is),
 *            QUAL reversed.  Lines without 0x10, every line of a record-less read among them, are as given.  BAM: on a 0x10 record
 *            the bases are complemented and packed from the last to the first, the qualities reversed: the record
 *            samfile.sam_to_bam makes of the oriented text.
 *   aln_pos / aln_op_off / aln_ops   the gapped alignment (sfgpu_hits_align_gapped's d_pos, d_op_off, d_ops for the same records:
 *            slot 2 h + which is line `which` of record h).  A mapped line's POS is aln_pos[slot] + 1, its CIGAR the slot's
 *            operations (len << 4 | op, MIDNSHP=X), PNEXT the other line's POS written this way; FLAG and TLEN are unchanged.  A
 *            line whose slot has no operation has no base on the transcript: error_kind 1, and the record's own pos is not
 *            consulted.  The three go together (SFGPU_ERR_INVALID otherwise).  BAM: the CIGAR words are the slot's; bin and
 *            error_kind 5 take the reference span (M + D), error_kind 4 compares the bases given with S + M + I and covers more
 *            than 65 535 operations.
 *   tag_nm / tag_md_off / tag_md   the NM / MD tags (sfgpu_hits_md_tags' d_nm, d_md_off, d_md for the same records and the same
 *            alignment, slots as above).  A mapped line ends ... QUAL \t NM:i:<nm> \t MD:Z:<md> \t NH:i:<nh> \n, nh being the read's
 *            record count hit_off[r + 1] - hit_off[r]; the lines of a read without records carry no tags.  The three go together,
 *            and tags need the mates' bases (seq1_off, and seq2_off of a paired batch): SFGPU_ERR_INVALID otherwise.  BAM: a
 *            mapped line's record ends, behind QUAL, NM <t> <nm> | MD Z <md> NUL | NH <t> <nh>, <t> being the first of c C s S i I
 *            that holds the value, and block_size counts them: the bytes of sam_to_bam of the tagged text.
 *   tag_zw_rec / tag_zw_f32   the posteriors (sfgpu_hits_posteriors' d_rec and d_f32 for the same records: one entry per record,
 *            so both lines of a pair carry the record's value).  A mapped line ends ... QUAL [\t NM ... \t MD ... \t NH ...]
 *            \t ZW:f:<token> \n, the token being printf("%g") of the record's posterior probability, placed from tag_zw_rec; the
 *            lines of a read without records carry nothing.  The two go together (SFGPU_ERR_INVALID otherwise); tags and
 *            posteriors are independent of each other.  BAM: a mapped line's record ends, behind NH where there is one, Z W f and
 *            the four bytes of tag_zw_f32's float, and block_size counts those seven bytes: the bytes of sam_to_bam of the text
 *            with its ZW:f: tokens.
 * A batch that breaks a rule fails with SFGPU_ERR_INVALID before anything is written; error_read / error_record name the lowest
 * such (read, record) of the batch and error_kind says which rule: 1 no base on the transcript (a record with pos < 0 and
 * -pos >= read_len; for a pair record either mate), 2 tid >= n_refs, 6 a quality byte outside '!' .. '~' (33 .. 126; a tab or a
 * newline would break the text), reported as (read, record 0) for the lowest read that holds one.  BAM records add 3 a read name
 * not of 1 .. 254 bytes, 4 bases given whose number differs from the record's read length, or more than 65 535 of them, 5 an
 * alignment that ends beyond 2^29 (a record-less read counts as record 0).  The kinds are merged by the lowest (read, record),
 * then the lowest kind. */
typedef struct sfgpu_samw_batch {
    const struct sfgpu_hit* hits;
    const uint32_t* hit_off;         /* [n_reads + 1] */
    uint32_t n_reads;
    int paired;
    const char* ref_names;
    const uint64_t* ref_name_off;    /* [n_refs + 1] */
    uint32_t n_refs;
    const char* qnames;
    const uint64_t* qname_off;       /* [n_reads + 1] */
    const uint8_t* seq1;
    const int64_t* seq1_off;         /* [n_reads + 1] */
    const uint8_t* seq2;
    const int64_t* seq2_off;         /* [n_reads + 1] */
    uint64_t read_index_base;
    const uint8_t* qual1;
    const uint8_t* qual2;
    int oriented;
    const int32_t* aln_pos;          /* [2 records] */
    const uint64_t* aln_op_off;      /* [2 records + 1] */
    const uint32_t* aln_ops;
    const uint32_t* tag_nm;          /* [2 records] */
    const uint64_t* tag_md_off;      /* [2 records + 1] */
    const uint8_t* tag_md;
    const uint32_t* tag_zw_rec;      /* [records] */
    const float* tag_zw_f32;         /* [records] */
} sfgpu_samw_batch;
/* sfgpu_sam_write_text hands the text to `sink` as sfgpu_quant_write_text hands over its rows: consecutive chunks of at most
 * chunk_bytes (0 = 32 MiB; otherwise 16 .. 2^30, else SFGPU_ERR_INVALID), greedy, each a whole number of UNITS -- a unit is what
 * one record or one record-less read produces, so the two lines of a pair are never split -- from a pinned staging buffer that is
 * valid only during the call, chunk c + 1 formatted and copied while the sink consumes chunk c.  A batch that breaks a rule fails
 * before any sink call.  A unit longer than chunk_bytes is SFGPU_ERR_RANGE before the first sink call (`out` holds the sizes); a
 * nonzero return of the sink ends the call with SFGPU_ERR_IO and no further sink call; sink == NULL sizes (and checks) only;
 * n_reads == 0 is SFGPU_OK with zero bytes and no sink call.
 * Synchronous; ordered behind whatever is queued on `stream`; independent calls may run from several threads.  Scratch on the
 * device: 8 bytes per read, 16 bytes per unit and two chunk buffers. */
typedef struct {
    uint64_t n_bytes;         /* bytes of the alignment lines */
    uint64_t n_lines;
    uint64_t n_chunks;        /* sink calls made */
    uint64_t max_unit_bytes;  /* longest unit, with its '\n's */
    uint64_t error_read;      /* SFGPU_ERR_INVALID with error_kind != 0: the lowest (read, record) that cannot be written */
    uint64_t error_record;
    uint32_t error_kind;      /* 0 none, 1 no base on the transcript, 2 tid >= n_refs, 3 .. 5 sfgpu_sam_write_bgzf's, 6 a quality byte outside '!' .. '~' */
    uint32_t pad_;
    double format_ms;         /* device events: checks, sizing, scans, chunk plan, format kernels of all chunks */
    double d2h_ms;            /* device events around the staged copies */
    double sink_ms;           /* host clock inside the sink */
} sfgpu_samwrite_result;
SFGPU_API int sfgpu_sam_write_text(const sfgpu_samw_batch* batch, uint64_t chunk_bytes, sfgpu_text_sink sink, void* user,
                                   sfgpu_samwrite_result* out, sfgpu_stream stream);
/* GZipWriter::writeBootstrap<T> (src/GZipWriter.cpp:249-285): the reference appends every sample as raw little-endian binary to ONE
 * gzip stream (boost::iostreams::gzip_compressor), aux/bootstrap/bootstraps.gz.  Here the stream is produced on the device from the
 * sample matrix where it lies (the d_out of sfgpu_bootstrap / sfgpu_gibbs_sample): a gzip (RFC 1952) writer whose DEFLATE
 * (RFC 1951) blocks come from HIP kernels (csrc/gzwrite.hip; the arithmetic is csrc/gzfmt.h).  The contract of the file is "one
 * gzip member whose payload is the bytes written, in order"; the compressed bytes differ from zlib's.
 *   open   emits the 10-byte header through `sink`.  chunk_bytes: the largest piece handed to the sink (0 = 32 MiB; otherwise
 *          16 .. 2^30, else SFGPU_ERR_INVALID); pieces end anywhere, also inside a DEFLATE block.  Takes the handle's streams and
 *          8 KB of device memory for the per-block CRCs (SFGPU_ERR_HIP where it cannot), also for a handle that never writes.
 *   write  n_bytes at d_src (any alignment; n_bytes == 0 is legal and emits nothing) are cut into independent 64 KB blocks, each
 *          coded as one dynamic-Huffman block over literals and distance-1 run matches of length 3 .. 258 (the token class of
 *          zlib's Z_RLE) and padded to a byte by an empty stored block -- or as stored blocks where that is not shorter: a block
 *          never exceeds its payload by more than 10 bytes.  CRC-32 is computed on the device per block and combined on the
 *          host (x^(8 n) mod P), also from one write to the next.  The output is a function of the bytes and of the way
 *          they are split into writes, nothing else.  Compressed pieces are staged through two pinned buffers; the next batch
 *          (64 MiB of payload) is encoded, and the next piece copied, while the sink holds a piece.  h_bytes is valid only
 *          during the sink call.  Synchronous; ordered behind whatever is queued on `stream`; d_src may be reused on return.
 *          A nonzero return of the sink ends the call with SFGPU_ERR_IO and no further sink call; the stream is then broken
 *          (further writes: SFGPU_ERR_STATE) and close only releases it.
 *   close  emits the final (empty stored) block, CRC-32 and ISIZE (total bytes modulo 2^32), fills *res (may be NULL) and frees
 *          the handle, whatever it returns.  open + close gives a valid empty gzip file.
 * A handle belongs to one thread at a time and to the device that was current at open.  Device scratch: ~200 MB for writes of
 * 64 MiB and more. */
typedef struct sfgpu_gz sfgpu_gz;
typedef struct {
    uint64_t n_bytes_in;        /* payload bytes written */
    uint64_t n_bytes_out;       /* bytes accepted by the sink, header and trailer included */
    uint64_t n_blocks;          /* 64 KB blocks coded */
    uint64_t n_stored_blocks;   /* of those, laid out as stored blocks */
    uint64_t n_chunks;          /* sink calls made, header and trailer included */
    double encode_ms;           /* device events: encode, scan and compaction kernels of all batches */
    double d2h_ms;              /* device events around the staged copies */
    double sink_ms;             /* host clock inside the sink */
} sfgpu_gz_result;
SFGPU_API int sfgpu_gz_open(sfgpu_gz** out, sfgpu_text_sink sink, void* user, uint64_t chunk_bytes);
SFGPU_API int sfgpu_gz_write_device(sfgpu_gz* z, const void* d_src, uint64_t n_bytes, sfgpu_stream stream);
SFGPU_API int sfgpu_gz_close(sfgpu_gz* z, sfgpu_gz_result* res);
/* Blocked gzip (BGZF, the container of BAM and of bgzip'ed text: what samtools, IGV and htslib read) from device memory.  The
 * file is "BGZF members whose payloads are the bytes written, in order, and the 28-byte EOF member"; any gzip reader inflates it,
 * and sfgpu_bgzf_inflate_host reads it back on the device.  What a member says is stated once, serially, in csrc/bgzwfmt.h; the
 * kernels are csrc/bgzf_write.hip.  Unlike sfgpu_gz_* the DEFLATE blocks carry real (length, distance) matches: alignment files
 * repeat names, bases and columns a few hundred bytes apart, which the run matches of sfgpu_gz_* cannot say.
 *   open   emits nothing.  chunk_bytes: the largest piece handed to the sink (0 = 32 MiB; otherwise 16 .. 2^30, else
 *          SFGPU_ERR_INVALID); pieces end anywhere, also inside a member.
 *   write  n_bytes at d_src (any alignment; n_bytes == 0 is legal and emits nothing) are cut into members of 32 768 payload
 *          bytes, the write's last member short.  A member is the 18-byte BGZF header with BSIZE, ONE final DEFLATE block, CRC-32
 *          and ISIZE, all written by the kernel.  The block is dynamic-Huffman over literals and matches of length 3 .. 258 at
 *          distance 1 .. 32 768 within the member (the parse: a 4-byte hash per position against the greatest earlier position of
 *          the same bucket in 256-position steps, distance 1 and the previous distance as second candidates, greedy, restarted at
 *          every 64-byte slice), or one stored block where that is not shorter: a member never exceeds its payload by more than
 *          31 bytes.  The output is a function of the bytes and of the way they are split into writes, nothing else.  Staging,
 *          overlap, the sink's rights and SFGPU_ERR_IO / SFGPU_ERR_STATE are those of sfgpu_gz_write_device.
 *   close  emits the EOF member, fills *res (may be NULL) and frees the handle, whatever it returns.  open + close gives the
 *          28-byte empty BGZF file.
 * A handle belongs to one thread at a time and to the device that was current at open.  Device scratch: ~200 MB for writes of
 * 64 MiB and more. */
typedef struct sfgpu_bgzw sfgpu_bgzw;
typedef struct {
    uint64_t n_bytes_in;        /* payload bytes written */
    uint64_t n_bytes_out;       /* bytes accepted by the sink, the EOF member included */
    uint64_t n_members;         /* members coded, the EOF member not counted */
    uint64_t n_stored_members;  /* of those, laid out as a stored block */
    uint64_t n_matches;         /* tokens of the coded members, summed by the kernel */
    uint64_t n_literals;
    uint64_t n_chunks;          /* sink calls made */
    double encode_ms;           /* device events: encode, scan and compaction kernels of all batches */
    double d2h_ms;              /* device events around the staged copies */
    double sink_ms;             /* host clock inside the sink */
} sfgpu_bgzw_result;
SFGPU_API int sfgpu_bgzw_open(sfgpu_bgzw** out, sfgpu_text_sink sink, void* user, uint64_t chunk_bytes);
SFGPU_API int sfgpu_bgzw_write_device(sfgpu_bgzw* z, const void* d_src, uint64_t n_bytes, sfgpu_stream stream);
SFGPU_API int sfgpu_bgzw_close(sfgpu_bgzw* z, sfgpu_bgzw_result* res);
/* sfgpu_sam_write_text into a BGZF file: the same batch, the same checks and the same bytes, but the chunks never visit the host
 * uncompressed -- every chunk of at most chunk_bytes (0 = 32 MiB) is formatted into a device buffer and handed to `z`
 * (sfgpu_bgzw_write_device) where it lies, chunk c + 1 formatted while chunk c is encoded, copied and sunk.  `z` copies and sinks
 * what it writes; its result (sfgpu_bgzw_close) holds the compressed bytes, the encode, copy and sink times.  format:
 * SFGPU_SAMW_TEXT, the alignment lines of sfgpu_sam_write_text (a "sam.gz" file when the caller has written the @HD / @SQ lines
 * through the same handle).  In `out`, n_bytes counts the uncompressed bytes, n_chunks the chunks handed to `z`; d2h_ms and sink_ms
 * stay 0.  A batch that cannot be written fails before anything reaches `z` (error_kind etc. as in sfgpu_sam_write_text); a failure
 * of `z` (SFGPU_ERR_IO: its sink refused) ends the call and leaves `z` broken.  n_reads == 0 writes nothing.
 * SFGPU_SAMW_BAM writes the same lines as BAM records (a BAM file when the caller has written the magic, the header text and the
 * reference list through the same handle): what samfile.sam_to_bam makes of the text, stated in csrc/bamwfmt.h -- mapq 255, the
 * specification's bin, CIGAR words S and M, SEQ 4-bit packed through =ACMGRSVTWYHKDBN after upper-casing (anything else 15), QUAL
 * 0xff, no SEQ given: l_seq 0; each group of the batch as sfgpu_samw_batch says.  A unit is then the one or two records of a hit
 * record or record-less read, n_lines counts records, and error kinds 3 .. 5 apply. */
enum { SFGPU_SAMW_TEXT = 0, SFGPU_SAMW_BAM = 1 };
SFGPU_API int sfgpu_sam_write_bgzf(const sfgpu_samw_batch* batch, uint64_t chunk_bytes, sfgpu_bgzw* z, int format,
                                   sfgpu_samwrite_result* out, sfgpu_stream stream);
/* Reads as a FASTA / FASTQ text, formatted on the device from the batch where it lies: the mirror of sfgpu_reads_parse_*.  What a
 * record says is csrc/readwfmt.h (the bytes of readfile.reads_text_host):
 *   d_bases / d_off[n_reads + 1]   the bases back to back and their int64 offsets (never decreasing, none negative)
 *   d_qual                         the qualities, sharing d_off: the text is then FASTQ, '@' name \n bases \n + \n qualities \n;
 *                                  NULL: FASTA, '>' name \n bases \n, never wrapped
 *   d_names / d_name_off[n_reads + 1]   the names back to back and their 64-bit offsets; both NULL: the name of record r is 'r' and
 *                                  the decimal of read_index_base + r (the default QNAME of sfgpu_sam_write_text)
 *   d_select                       one byte a record, nonzero = write it; NULL: every record.  The text is the selected records in
 *                                  input order; unselected records are neither written nor checked
 * All pointers are device pointers of any alignment; the inputs are not modified.  n_reads < 2^32 - 1 and records of less than
 * 2^32 bytes (else SFGPU_ERR_RANGE); an offset array that decreases, offsets that name bytes of a NULL array and names without
 * offsets are SFGPU_ERR_INVALID.  A selected record that cannot be written is SFGPU_ERR_FORMAT before any sink call, `out` naming
 * the lowest (record << 8 | kind): error_kind SFGPU_READW_NAME_NEWLINE a name holds '\n', _SEQ_NEWLINE the bases do, _QUAL_NEWLINE
 * the qualities do, _FASTA_SEQ_START the first base of a FASTA record is '>'.  A '\r' is written as given.
 * The text goes to `sink` in chunks of at most chunk_bytes (0 = 32 MiB; otherwise 16 .. 2^30, else SFGPU_ERR_INVALID), greedy, each
 * a whole number of records, through two pinned buffers owned by the call; a record longer than chunk_bytes is SFGPU_ERR_RANGE
 * before the first sink call (`out` holds the sizes), a nonzero return of the sink SFGPU_ERR_IO.  sink == NULL sizes and checks
 * only.  With nothing selected, or n_reads == 0, the call returns SFGPU_OK, reports 0 bytes and does not call the sink.
 * Synchronous, ordered behind the work already on `stream`, no CPU path.
 * sfgpu_reads_write_bgzf is the same call into a BGZF handle, as sfgpu_sam_write_bgzf: the chunks go to `z` on the device
 * (sfgpu_bgzw_write_device), d2h_ms and sink_ms stay 0, and a batch that cannot be written fails before anything reaches `z`. */
enum {
    SFGPU_READW_OK = 0,
    SFGPU_READW_NAME_NEWLINE = 1,
    SFGPU_READW_SEQ_NEWLINE = 2,
    SFGPU_READW_QUAL_NEWLINE = 3,
    SFGPU_READW_FASTA_SEQ_START = 4
};
typedef struct {
    uint64_t n_reads, n_selected, n_bytes, n_chunks, max_record_bytes;
    uint64_t error_record;   /* the record of the lowest (record << 8 | kind), valid when error_kind != 0 */
    int32_t  error_kind;     /* 0, or SFGPU_READW_NAME_NEWLINE 1, _SEQ_NEWLINE 2, _QUAL_NEWLINE 3, _FASTA_SEQ_START 4 */
    double   format_ms, d2h_ms, sink_ms;   /* device events around the kernels and the staged copies, host clock inside the sink */
} sfgpu_readwrite_result;
SFGPU_API int sfgpu_reads_write_text(const uint8_t* d_bases, const int64_t* d_off, uint64_t n_reads, const uint8_t* d_qual,
                                     const uint8_t* d_names, const uint64_t* d_name_off, uint64_t read_index_base,
                                     const uint8_t* d_select, uint64_t chunk_bytes, sfgpu_text_sink sink, void* user,
                                     sfgpu_readwrite_result* out, sfgpu_stream stream);
SFGPU_API int sfgpu_reads_write_bgzf(const uint8_t* d_bases, const int64_t* d_off, uint64_t n_reads, const uint8_t* d_qual,
                                     const uint8_t* d_names, const uint64_t* d_name_off, uint64_t read_index_base,
                                     const uint8_t* d_select, uint64_t chunk_bytes, sfgpu_bgzw* z, sfgpu_readwrite_result* out,
                                     sfgpu_stream stream);
/* The compressed size of every member a BGZF handle writes, kept on the device: what virtual file offsets are made of.
 *   track_members  from this call on every write also keeps its members' sizes (4 bytes a member of device memory, in file order).
 *                  The bytes written, the results and the other calls do not change.
 *   member_sizes   *d_sizes[0 .. *n_members): the sizes of the members written since, the EOF member not among them; the pointer
 *                  holds until the next write.  SFGPU_ERR_STATE on a handle that does not track. */
SFGPU_API int sfgpu_bgzw_track_members(sfgpu_bgzw* z);
SFGPU_API int sfgpu_bgzw_member_sizes(sfgpu_bgzw* z, const uint32_t** d_sizes, uint64_t* n_members);
/* A coordinate-sorted BAM file with its BAI index, from the device.  What the file and the index say -- the order, the member cut,
 * virtual offsets, chunks, the linear index -- is stated once in csrc/baifmt.h; the kernels are csrc/bamsort.hip; the Python
 * statements are samfile.write_bam(sort="coordinate") and samfile.build_bai.
 *   open     an empty record store on the current device.
 *   collect  the batch, checks, errors and `out` of sfgpu_sam_write_bgzf with SFGPU_SAMW_BAM, the handle in place of `z` (and no
 *            chunk_bytes): the batch's records are formatted into one device segment owned by the handle and listed (key, address,
 *            length); out->n_chunks stays 0.  A batch that breaks a rule stores nothing.  The store holds fewer than 2^32 records:
 *            the call that would reach that returns SFGPU_ERR_RANGE and stores nothing.  Device memory: the records' bytes and
 *            20 bytes a record; nothing is spilled to the host.  The sort key, the bin and the index are read from the records' own
 *            pos and CIGAR words: they follow the batch's alignment, and tags and posteriors change none of them.
 *   finish   `z` must track its members (sfgpu_bgzw_track_members, from its first write) and hold the file's header already.  The
 *            records are sorted stably by (uint32)refID << 32 | (uint32)(pos + 1), gathered into the sorted stream in pieces of
 *            piece_bytes (0 = 32 MiB, else 16 .. 2^30; rounded down to a multiple of 32 768, at least that) and written through `z`,
 *            piece i + 1 gathered while piece i is encoded: the file does not depend on piece_bytes.  With index_sink != NULL the
 *            BAI of n_refs references is then built on the device and handed to index_sink in pieces of at most 32 MiB (a nonzero
 *            return: SFGPU_ERR_IO).  The caller closes `z` afterwards (the EOF member, whose offset the index already names).  An
 *            index of 2^28 chunks or more is SFGPU_ERR_RANGE.  finish adds 28 bytes a record, two pieces and, for the index,
 *            40 bytes a record and 28 bytes a chunk of device memory.
 *   close    frees the store.
 * collect after finish and finish twice are SFGPU_ERR_STATE.  All calls are synchronous and ordered behind the work on `stream`. */
typedef struct sfgpu_bamsort sfgpu_bamsort;
typedef struct {
    uint64_t n_records;
    uint64_t n_no_coor;       /* records with refID < 0: they stand last */
    uint64_t n_bytes;         /* the sorted record stream, uncompressed */
    uint64_t state_bytes;     /* peak device bytes held by the handle and by finish */
    uint64_t index_bytes;     /* 0 without an index */
    uint64_t n_pieces;        /* writes made to `z` */
    uint64_t n_index_chunks;
    uint64_t n_index_bins;    /* the pseudo-bins not counted */
    double sort_ms;           /* device events: the sort */
    double gather_ms;         /* device events: the gather kernels of all pieces */
    double index_ms;          /* host clock: the index kernels, their copies and the sink */
} sfgpu_bamsort_result;
SFGPU_API int sfgpu_bamsort_open(sfgpu_bamsort** out);
SFGPU_API int sfgpu_bamsort_collect(sfgpu_bamsort* b, const sfgpu_samw_batch* batch, sfgpu_samwrite_result* out, sfgpu_stream stream);
SFGPU_API int sfgpu_bamsort_finish(sfgpu_bamsort* b, sfgpu_bgzw* z, uint32_t n_refs, uint64_t piece_bytes, sfgpu_text_sink index_sink,
                                   void* user, sfgpu_bamsort_result* res, sfgpu_stream stream);
SFGPU_API int sfgpu_bamsort_close(sfgpu_bamsort* b);
/* ---- the class-table exchange of a multi-GPU run (the reference has one table in one process) ----------
 * One process / thread per GPU builds the table of ITS reads; afterwards every rank must hold the table a single
 * builder would have produced from all reads.  The library does the device work on class tables in CSR form (the
 * sfgpu_eq_export_device arrays); the HOST moves the byte blocks (RCCL, MPI, ...):
 *   1. owner(class) = a function of its XXH64 mod N.  sfgpu_eqvec_owner_sizes -> classes / ids per owner;
 *      sfgpu_eqvec_pack_by_owner -> N blocks, block d = [counts u64[c_d] | lens u32[c_d] | ids u32[l_d] | pad to 8 B]
 *      at d_blocks + h_block_off[d] (SFGPU_BLOCK_BYTES(c_d, l_d) bytes; classes keep their canonical order).
 *   2. all-to-all: block d goes to rank d.  The owner folds what it received with sfgpu_eq_add_block_device (upsert:
 *      equal labels add their counts), finish()es and exports ITS partition of the merged table.
 *   3. sfgpu_eqvec_export_block -> the partition as one block [counts u64[C] | hashes u64[C] | lens u32[C] | ids u32[L]]
 *      (SFGPU_GATHER_BYTES(C, L) bytes); all-gather of the blocks: the partitions are DISJOINT.
 *   4. sfgpu_eqvec_merge_disjoint -> the union in the canonical order (first id, XXH64, length, label), as CSR: a sort
 *      of (first id, hash) keys and a gather, nothing is hashed again.  *same_key_twice = 1 (and no output) if two
 *      different labels share first id and XXH64: fold the blocks through a builder instead (never seen).
 * Integer work throughout: the result equals the single-builder table class for class, in order.  n_owners <= 256,
 * n_parts <= 64; the h_* arrays are host arrays; calls are synchronous on `stream`.  A call refused with SFGPU_ERR_INVALID has
 * written none of its outputs. */
#define SFGPU_BLOCK_BYTES(c, l) ((12ull * (uint64_t)(c) + 4ull * (uint64_t)(l) + 7ull) & ~7ull)
#define SFGPU_GATHER_BYTES(c, l) (20ull * (uint64_t)(c) + 4ull * (uint64_t)(l))
SFGPU_API int sfgpu_eqvec_owner_sizes(const uint32_t* d_rowptr, const uint64_t* d_hashes, uint64_t n_classes, uint32_t n_owners,
                                      uint64_t* h_classes, uint64_t* h_ids, sfgpu_stream stream);
SFGPU_API int sfgpu_eqvec_pack_by_owner(const uint32_t* d_rowptr, const uint32_t* d_ids, const uint64_t* d_counts, const uint64_t* d_hashes,
                                        uint64_t n_classes, uint32_t n_owners, const uint64_t* h_classes, const uint64_t* h_ids,
                                        void* d_blocks, uint64_t* h_block_off /* [n_owners + 1] */, sfgpu_stream stream);
SFGPU_API int sfgpu_eq_add_block_device(sfgpu_eq* eq, const void* d_block, uint64_t n_classes, uint64_t n_ids, sfgpu_stream stream);
SFGPU_API int sfgpu_eqvec_export_block(const uint32_t* d_rowptr, const uint32_t* d_ids, const uint64_t* d_counts, const uint64_t* d_hashes,
                                       uint64_t n_classes, uint64_t n_ids, void* d_block, sfgpu_stream stream);
SFGPU_API int sfgpu_eqvec_merge_disjoint(const void* const* d_blocks, const uint64_t* n_classes, const uint64_t* n_ids, uint32_t n_parts,
                                         uint32_t* d_rowptr, uint32_t* d_ids, uint64_t* d_counts, uint64_t* d_hashes,
                                         int* same_key_twice, sfgpu_stream stream);

/* Builder counters since the last start(): device time of the insert kernel (HIP events on the
 * builder's stream), launches, table growths, deferred-and-replayed reads, current table slots. */
typedef struct {
    double insert_ms;
    uint64_t insert_launches;
    uint64_t table_grows;
    uint64_t deferred_reads;
    uint64_t table_slots;
    uint64_t hot_reads;       /* reads whose class was already hot and that the route pass counted itself */
    uint64_t spilled_reads;   /* reads of the partitioned passes that went to the generic kernel (bin overflow, long labels) */
    uint64_t pipeline_drains; /* times the pipelined partition passes had to run dry (table growth, deferred reads, reallocation) */
} sfgpu_eq_stats;
SFGPU_API int sfgpu_eq_get_stats(sfgpu_eq* eq, sfgpu_eq_stats* out);
/* finish() :64-80: snapshot into the canonical class order (first id, XXH64, length, label --
 * the reference's order is hash-table order and run dependent).  Reports what the reference
 * logs: #classes and sum(count); nnz = sum of label lengths. Synchronous. */
SFGPU_API int sfgpu_eq_finish(sfgpu_eq* eq, uint64_t* n_classes, uint64_t* nnz, uint64_t* total_reads);
/* eqVec() :110-112 as CSR: rowptr[C+1], ids[nnz], counts[C] (uint64 like TGValue::count),
 * hashes[C] (TranscriptGroup::hash; may be NULL).  nnz must be < 2^32 (SFGPU_ERR_RANGE).
 * _device is asynchronous on the builder's stream; _host is synchronous. */
SFGPU_API int sfgpu_eq_export_device(sfgpu_eq* eq, uint32_t* d_rowptr, uint32_t* d_ids, uint64_t* d_counts, uint64_t* d_hashes);
SFGPU_API int sfgpu_eq_export_host(sfgpu_eq* eq, uint32_t* h_rowptr, uint32_t* h_ids, uint64_t* h_counts, uint64_t* h_hashes);

/* ---------------------------------------------------------------------------------------------
 * a14. fragment-length distribution -> effective lengths   src/SailfishQuantify.cpp
 * The 1000-entry correction tables are serial prefix sums and are built on the host in the
 * reference's evaluation order; the O(M) transform runs on the device.
 * ------------------------------------------------------------------------------------------- */
/* getNormalFragLengthDist :648-673 (mean/sd are integers in SailfishOpts.hpp:34-35) */
SFGPU_API int sfgpu_cf_gaussian(uint32_t max_frag_len, uint64_t mean, uint64_t sd, double* h_cf);
/* correctionFactorsFromCounts :769-807 */
SFGPU_API int sfgpu_cf_counts(const uint32_t* h_fl_counts, uint32_t max_frag_len, double* h_cf);
/* computeSmoothedEffectiveLengths :809-838 ; setEffectiveLengthsDirect :706-715 when h_cf == NULL.
 * Asynchronous on `stream`: the table h_cf is copied to the device by a stream-ordered copy, so a PINNED h_cf must stay valid and
 * unchanged until the stream has passed this call (pageable memory is staged by the runtime before the call returns). */
SFGPU_API int sfgpu_efflen_smoothed(const uint32_t* d_ref_len, uint64_t M, const double* h_cf, uint32_t max_frag_len,
                          double* d_eff_len, sfgpu_stream stream);
/* --unsmoothedFLD: computeEmpiricalEffectiveLengths :717-767 over EmpiricalDistribution
 * (src/EmpiricalDistribution.cpp:29-118; float pdf table, cut where the cumulative mass passes 1 - 1e-6,
 * two-ended median walk).  h_fl_counts[i] = observed fragments of length i, i in [0, max_frag_len).
 * eff = RefLength when RefLength <= median, else sum_l pdf(l) * (RefLength - l + 1).  Synchronous. */
SFGPU_API int sfgpu_efflen_empirical(const uint32_t* h_fl_counts, uint32_t max_frag_len, const uint32_t* d_ref_len, uint64_t M,
                           double* d_eff_len, sfgpu_stream stream);

/* ---------------------------------------------------------------------------------------------
 * a6-a12. CollapsedEMOptimizer   src/CollapsedEMOptimizer.cpp:711-893
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    uint64_t M;               /* transcripts() .size(); <= 2^31 */
    const double* d_len;      /* per transcript: RefLength if noEffectiveLengthCorrection else
                                 EffectiveLength (:736-737); clamped to >= 1 internally (:738) */
    uint64_t C;               /* eqVec().size() */
    const uint32_t* d_rowptr; /* C+1 */
    const uint32_t* d_ids;    /* rowptr[C] */
    const uint64_t* d_counts; /* C; every count must be < 2^31 (SFGPU_ERR_RANGE).  The builder's counts are >= 1.  A class with
                                 count 0 contributes nothing, under EM (the reference skips its 0 / 0 weights, :269) and under
                                 VBEM alike (where the reference itself returns NaN for such a class of two or more members:
                                 the kernels never form the stored weights); its members still count as active */
    uint64_t num_mapped;      /* ReadExperiment::numMappedFragments() (:792) */
} sfgpu_problem;

typedef struct {
    int use_vbem;             /* sopt.useVBOpt (:784) */
    double tol;               /* relDiffTolerance: 0.01 at the call site, src/SailfishQuantify.cpp:1343 */
    uint32_t min_iter;        /* 50 in optimize() (:716); 0 in doBootstrap (:486) */
    uint32_t max_iter;        /* 10000 at the call site */
    int check_mode;           /* 0: gate on alphasPrime > 1e-2 (:852); 1: on alphas > 1e-2 (:499) */
    uint32_t iters_per_launch;/* iterations enqueued between host polls of the device-side stop
                                 latch (the stop iteration is exact regardless). 0 = default (32) */
} sfgpu_em_opts;

typedef struct {
    uint32_t iters;           /* itNum when the loop stopped */
    uint32_t converged;
    double max_rel_diff;      /* as logged at :871-872 */
    double alpha_sum;         /* after truncateCountVector (:875) */
    uint64_t n_active;        /* activeTranscriptIDs.size() (:774-782) */
    double loop_ms;           /* device time of the iteration loop (HIP events on `stream`) */
    uint32_t fused;           /* 1: the loop ran as one kernel per iteration (update folded into the sweep), 0: sweep + update */
    uint32_t persistent;      /* 1: the whole loop ran as ONE launch (csrc/em_persist.h); implies fused */
} sfgpu_em_stats;

SFGPU_API int sfgpu_em_create(sfgpu_em** out, const sfgpu_problem* prob, sfgpu_stream stream);
SFGPU_API int sfgpu_em_destroy(sfgpu_em* em);
/* optimize() :711-893 without the bias branch: writes estCount (alpha after truncation) to
 * d_alpha_out[M] and, if non-NULL, mass = alpha/alphaSum to d_mass_out[M].  Synchronous.
 * Returns SFGPU_ERR_NO_ACTIVE / SFGPU_ERR_ALPHA_SUM where the reference returns false. */
SFGPU_API int sfgpu_em_optimize(sfgpu_em* em, const sfgpu_em_opts* opts, double* d_alpha_out, double* d_mass_out,
                      sfgpu_em_stats* stats);

/* The same loop in pieces, for callers that own the iteration (multi-GPU: classes sharded over
 * ranks, alphaOut all-reduced between sweep and update).  All asynchronous on the stream.
 *   begin : zero alphaOut, then alphaOut[t] = 1 for every transcript in a local class (:774-782)
 *           -> caller may SUM-all-reduce alphaOut across ranks
 *   init  : n_active = #(alphaOut > 0); alpha = active ? numMapped/n_active : 0 (:800-803); it = 0
 *   sweep : alphaOut += E-step contributions of the local classes (EMUpdate_ :224-281 /
 *           VBEMUpdate_ :322-367); no-op once the stop latch is set
 *           -> caller may SUM-all-reduce alphaOut across ranks
 *   update: [VBEM: alphaOut += prior] convergence test + alpha <- alphaOut, alphaOut <- 0
 *           (:849-861), ++it, evaluates the loop condition of :820 into the stop latch
 *   poll  : synchronous; reads the latch and counters
 *   finish: truncate (:875), alphaSum, write outputs; synchronous */
SFGPU_API int sfgpu_em_begin(sfgpu_em* em, const sfgpu_em_opts* opts);
SFGPU_API int sfgpu_em_init(sfgpu_em* em);
SFGPU_API int sfgpu_em_sweep(sfgpu_em* em);
SFGPU_API int sfgpu_em_update(sfgpu_em* em);
SFGPU_API int sfgpu_em_poll(sfgpu_em* em, int* done, sfgpu_em_stats* stats);
SFGPU_API int sfgpu_em_finish(sfgpu_em* em, double* d_alpha_out, double* d_mass_out, sfgpu_em_stats* stats);
/* device pointer of alphaOut (M doubles) for the caller's collective */
SFGPU_API double* sfgpu_em_alpha_out(sfgpu_em* em);
/* The piecewise loop with doBiasCorrect (src/CollapsedEMOptimizer.cpp:814-840): run to a recompute iteration by
 * lowering the stop bounds (set_bounds, between polls), hand the current abundances (sfgpu_em_alpha) and lengths
 * (sfgpu_em_lengths: effLens as the loop holds them, clamped at 1) to sfgpu_bias_update, then give the new lengths
 * back with rebase -- updateEqClassWeights (:527-555): the lengths are replaced (clamped at 1) and x is rebuilt from
 * the current alpha -- raise the bounds again and continue.  The next begin() restores the problem's own lengths. */
SFGPU_API double* sfgpu_em_alpha(sfgpu_em* em);
SFGPU_API double* sfgpu_em_lengths(sfgpu_em* em);
SFGPU_API int sfgpu_em_set_bounds(sfgpu_em* em, uint32_t min_iter, uint32_t max_iter);
/* Process-wide: may optimize() / the bootstrap run the EM loop as ONE persistent launch (csrc/em_persist.h; the loop of
 * src/CollapsedEMOptimizer.cpp:818-861)?  Default 1.  The launch needs every one of its blocks resident, i.e. the device to itself while
 * it starts: processes or ranks that share a device call this with 0 (one kernel per iteration then; the same results).  Takes effect
 * for runs that begin afterwards; handles planned while it was 0 have no tables for the loop and keep one kernel per iteration. */
SFGPU_API int sfgpu_em_allow_persistent(int on);
/* Diagnostic, like sfgpu_xxh64_labels: the device arithmetic of VBEM's x_t = exp(psi(alpha_t) - c) / effLen_t (csrc/vbmath.h; :300-320)
 * on its own, one lane per element, for the tests that hold every form to mpmath.  out[i] = form(d_a[i], d_c[i], d_len[i]); all pointers
 * are device memory (a form reads only the arrays it names; the others may be NULL), n = 0 is fine, asynchronous on `stream`.  An unknown
 * form returns SFGPU_ERR_INVALID and writes nothing.  The x forms are defined for a >= 0.01, len >= 1, c < 50 (what the loops hand them). */
enum {
    SFGPU_VB_DIGAMMA = 0,   /* digamma_pos(a) */
    SFGPU_VB_X_PREPARE = 1, /* exp(digamma_pos(a) - c) / len: k_vb_prepare, the first x of every run and the two-kernel loop */
    SFGPU_VB_X_LEAN = 2,    /* vb_x_lean: the fused sweep */
    SFGPU_VB_X_FAST = 3,    /* vb_x_fast: one division, its own exp, constants in constant memory */
    SFGPU_VB_X_HEAD = 4,    /* vb_x_head: the persistent loop (fast_rcp, literal constants) */
    SFGPU_VB_RCP = 5        /* fast_rcp(len) */
};
SFGPU_API int sfgpu_vb_eval(int form, const double* d_a, const double* d_c, const double* d_len, uint64_t n, double* d_out,
                            sfgpu_stream stream);
SFGPU_API int sfgpu_em_rebase(sfgpu_em* em, const double* d_len);
/* Diagnostic, like sfgpu_vb_eval: the PLAN of a handle (csrc/em.hip sfgpu_em_create, csrc/em_persist.h) in numbers, for the tests that
 * build a class table for one boundary of the plan and must know that the run took that path.  Read-only: it waits for the plan's own
 * stream, reads the plan's tables back and resolves the two lazy verdicts the way a run would; it changes no table, no launch and no
 * result.  Synchronous.  A problem without classes reports zeros and verdict 1.  (The struct is named by its tag: `struct
 * sfgpu_em_plan_info`.) */
struct sfgpu_em_plan_info {
    uint32_t n_tiles;          /* tiles of the plan */
    uint32_t tile_nnz;         /* nonzeros per tile: the cuts fall at its multiples */
    uint32_t redone;           /* times the plan was redone with one more round because a tile held more than 7800 classes */
    uint32_t most_classes;     /* the most classes in one tile (the persistent loop's den_cap, the null class of the gather form) */
    uint64_t P;                /* window slots over all tiles */
    uint64_t E;                /* escapes: members outside their tile's window */
    uint32_t renumbered;       /* 1: the plan runs in a transcript order of its own */
    uint32_t gather;           /* 1: the gather form of the sweep; 0: the scatter form (SFGPU_EM_GATHER=0, or every member an escape) */
    uint32_t cover_tiles;      /* tiles that more than six tiles overlap: they go by the cover list (gather form; 0 otherwise) */
    uint32_t most_far_slots;   /* the most distinct far transcripts of a tile */
    uint32_t longest_far_list; /* the most far members of a tile */
    uint32_t fused_ok;         /* 1: the plan can run one kernel per iteration */
    uint64_t n1, n2, n3, n4;   /* sums over the tiles of the persistent loop's class records: 4-, 8-, 16-byte, 16-byte + overflow */
    uint64_t n_ov;             /* ... and of their overflow chunks (all 0 when the plan has no tables for the persistent loop) */
    uint32_t persist_verdict;  /* 0: eligible for the persistent loop; else why not: 1 no tables (SFGPU_EM_PERSIST=0 when the plan was
                                  made, the scatter form, no classes), 2 plan event, 3 a far member's transcript lies in no window,
                                  4 a transcript fed by more than 16 far slots, 5 a tile that goes by the cover list, 6 LDS,
                                  7 device query, 8 function attribute, 9 occupancy query, 10 more tiles than resident blocks;
                                  11 the plan was eligible, but a persistent launch of this handle gave up waiting (a shared
                                  device): the handle keeps one kernel per iteration from then on */
    uint32_t pad_;
};
SFGPU_API int sfgpu_em_plan_info(sfgpu_em* em, struct sfgpu_em_plan_info* info);
/* The sharded loop as ONE call (classes partitioned over the GPUs, alpha replicated, one SUM all-reduce of
 * alphaOut per iteration): `em` holds THIS rank's slice of the classes; `allreduce` must leave the element-wise sum over
 * all ranks in d_buf on every rank (in place; it may enqueue on `stream`, the stream the loop runs on, or synchronise --
 * e.g. ncclAllReduce(d_buf, d_buf, n, ncclDouble, ncclSum, comm, stream)).  Runs begin -> all-reduce (union of the
 * active sets) -> init -> { sweep, all-reduce, update } with the stop latch polled every `poll_every` iterations ->
 * finish: every rank stops at the same iteration with the same alpha (the reference's stop iteration for the union of
 * the classes).  Same outputs and return codes as sfgpu_em_optimize.  Replaces the reference's
 * CollapsedEMOptimizer::optimize call (src/SailfishQuantify.cpp:1343) in a multi-GPU host. */
typedef int (*sfgpu_allreduce_fn)(double* d_buf, uint64_t n, void* user, sfgpu_stream stream);
SFGPU_API int sfgpu_em_optimize_sharded(sfgpu_em* em, const sfgpu_em_opts* opts, sfgpu_allreduce_fn allreduce, void* user,
                                        uint32_t poll_every, double* d_alpha_out, double* d_mass_out, sfgpu_em_stats* stats);
/* the stream the handle's kernels run on (what to pass to a collective that must be ordered with them) */
/* The sharded loop with ONE sweep kernel per iteration (the update folded into the head of the next sweep, as in optimize()): sweep +
 * fold + all-reduce per iteration instead of sweep + fold + all-reduce + update.  Every rank must run the same form: ask each rank
 * (sfgpu_em_sharded_fused_ok: 1 if its plan allows it), agree on the minimum, tell each rank (sfgpu_em_set_sharded_fused). */
SFGPU_API int sfgpu_em_sharded_fused_ok(sfgpu_em* em);
SFGPU_API int sfgpu_em_set_sharded_fused(sfgpu_em* em, int on);
SFGPU_API sfgpu_stream sfgpu_em_stream(sfgpu_em* em);

/* ---------------------------------------------------------------------------------------------
 * (e) multi-GPU transport: RCCL over xGMI, bound at run time (csrc/comm.hip).  No counterpart in the reference (a
 * shared-memory program: the atomic adds of src/CollapsedEMOptimizer.cpp:224-281 are what the all-reduce replaces).
 * libsfgpu.so does not link librccl: it is dlopen'ed on first use (the copy the process already holds, else /opt/rocm/lib).
 * A communicator is made the NCCL way: one rank calls sfgpu_comm_unique_id and hands the SFGPU_COMM_ID_BYTES bytes to the
 * others by any channel (MPI_Bcast, a torch.distributed broadcast, a file); every rank then calls sfgpu_comm_create with
 * its own device current.  sfgpu_comm_allreduce_fn() is the callback for sfgpu_em_optimize_sharded (user = the
 * communicator): ncclAllReduce(buf, buf, n, ncclDouble, ncclSum, comm, stream), enqueued on the loop's stream, so that
 * no host code runs between two EM iterations. */
#define SFGPU_COMM_ID_BYTES 128
typedef struct sfgpu_comm sfgpu_comm;
SFGPU_API int sfgpu_comm_available(void);                                   /* 1 if librccl.so could be loaded */
SFGPU_API int sfgpu_comm_unique_id(void* id_out /* SFGPU_COMM_ID_BYTES */);
SFGPU_API int sfgpu_comm_create(sfgpu_comm** out, const void* id /* SFGPU_COMM_ID_BYTES */, int world, int rank);
SFGPU_API int sfgpu_comm_count(sfgpu_comm* c, int* ranks);                     /* ncclCommCount: the ranks the communicator really spans */
SFGPU_API int sfgpu_comm_destroy(sfgpu_comm* c);
SFGPU_API int sfgpu_comm_allreduce_sum_f64(sfgpu_comm* c, double* d_buf, uint64_t n, sfgpu_stream stream);   /* in place, on `stream` */
SFGPU_API sfgpu_allreduce_fn sfgpu_comm_allreduce_fn(void);
/* average duration (us) of one such all-reduce, `reps` back to back on `stream` (HIP events): what a host's choice between
 * the replicated and the sharded EM rests on */
SFGPU_API int sfgpu_comm_time_allreduce(sfgpu_comm* c, double* d_buf, uint64_t n, uint32_t reps, sfgpu_stream stream, double* avg_us);
/* Launch the E-step sweep kernel `n` times back to back (state untouched afterwards) and
 * return its average duration from HIP events on the stream: the live roofline measurement. */
SFGPU_API int sfgpu_em_time_sweep(sfgpu_em* em, const sfgpu_em_opts* opts, uint32_t n, double* avg_ms);

/* ---------------------------------------------------------------------------------------------
 * a15/a17. Bootstrap   src/CollapsedEMOptimizer.cpp:438-525 (doBootstrap), :557-709 (gatherBootstraps),
 *                      include/MultinomialSampler.hpp:13-64
 * Each draw b: class counts ~ Multinomial(N = sum(count) [uint32, as in the reference], p = count/N)
 * (exact; tree of conditional binomials, Philox4x32-10 streams keyed by (seed, b)), alpha
 * re-initialised uniformly over the active transcripts, EM/VBEM to convergence with doBootstrap's
 * loop (no 50-iteration floor, gate on alphas > 1e-2), truncation.  The reference seeds from
 * std::random_device, so only the DISTRIBUTION of the outputs is comparable.
 *   d_out   : n_bootstraps x M doubles on the device, or NULL
 *   cb      : writeBootstrap (std::function<bool(const std::vector<double>&)>): called once per
 *             draw with a host copy of alpha; return 0 to abort.  May be NULL.
 *   h_iters : per-draw iteration counts (host), may be NULL
 * opts->use_vbem / tol / max_iter are honoured; min_iter and check_mode are forced to doBootstrap's.
 * Where a replicate's EM loop runs as one persistent launch the draws run one after the other; elsewhere up to three
 * run concurrently (the handle plus internal clones of it, each on its own stream and host thread);
 * SFGPU_BS_LANES=1..8 overrides; draw b is the same whichever lane computes it and
 * `cb` is still called one draw at a time, in draw order.
 * Synchronous.  The handle's counts are restored afterwards.
 * ------------------------------------------------------------------------------------------- */
typedef int (*sfgpu_sample_cb)(const double* h_alpha, uint64_t M, void* user);
SFGPU_API int sfgpu_bootstrap(sfgpu_em* em, const sfgpu_em_opts* opts, uint32_t n_bootstraps, uint64_t seed,
                    double* d_out, sfgpu_sample_cb cb, void* user, uint32_t* h_iters);
/* One multinomial resample of the class counts (the sampCounts of doBootstrap :468) into
 * d_counts_out[C] (uint32), for draw index `draw` of `seed`.  Synchronous. */
SFGPU_API int sfgpu_bootstrap_counts(sfgpu_em* em, uint64_t seed, uint64_t draw, uint32_t* d_counts_out);

/* ---------------------------------------------------------------------------------------------
 * a16. CollapsedGibbsSampler::sample<ReadExperiment>   src/CollapsedGibbsSampler.cpp:198-291
 * (initCountMap_ :35-94, sampleRound_ :96-186).  Requires Transcript::mass from a prior optimize().
 * Runs `n_chains` independent chains (0 = default: min(n_samples, 1024) rounded up to 64); every
 * chain is initialised like initCountMap_ and then yields one sample per sampleRound_, so sample s
 * comes from chain s % n_chains after s / n_chains + 1 rounds (the reference runs one chain per TBB
 * chunk of the sample range and one round per sample).  The reference seeds from std::random_device:
 * parity is distributional.  Unlike the reference this call does NOT overwrite Transcript::mass
 * (:219-221 mutate it in place); the same transformed values are used internally.
 *   d_mass : M doubles, mass = alpha / alphaSum as written by optimize()
 *   d_out  : n_samples x M int32 on the device, or NULL
 *   cb     : writeSample (std::function<bool(const std::vector<int>&)>), host copy per sample; may be NULL
 * Device memory: 4 * nnz * n_chains + 4 * M * n_chains bytes of chain state.  Synchronous.
 * Domain: every ratio of weights the sampler forms divides by a NORMAL, finite double whose reciprocal is normal too (2^-1022 <= b <=
 * 2^1022; csrc/rng.h, ratio_of: reciprocal instruction plus two Newton steps, NaN outside).  Effective lengths are clamped at 1 and
 * every weight carries the prior, so finite lengths and masses in [0, 1] stay ~300 binary orders inside it.
 * ------------------------------------------------------------------------------------------- */
typedef int (*sfgpu_gibbs_cb)(const int32_t* h_counts, uint64_t M, void* user);
SFGPU_API int sfgpu_gibbs_sample(const sfgpu_problem* prob, const double* d_mass, uint32_t n_samples, uint32_t n_chains,
                       uint64_t seed, int32_t* d_out, sfgpu_gibbs_cb cb, void* user, sfgpu_stream stream);
/* Diagnostics, like sfgpu_vb_eval: the samplers' device arithmetic (csrc/rng.h, csrc/gibbsfmt.h, csrc/sampling.hip) on its own, for the
 * tests that hold it to the host build of the same headers draw for draw (tests/test_gpu_rng.py).  Every draw is a function of (seed,
 * stream, substream, arguments) alone.  All pointers are device memory, a count of 0 is fine, asynchronous on `stream`; an unknown form
 * returns SFGPU_ERR_INVALID and writes nothing.
 * sfgpu_rng_eval: one lane per element i, Philox(seed, d_stream ? d_stream[i] : i, d_substream ? d_substream[i] : 0) -- the lanes of a
 * wavefront may hold different arguments.  A form reads only the arrays it names; the others may be NULL. */
enum {
    SFGPU_RNG_WORDS = 0,        /* d_out: uint32 [n][w], the first w words of next32() */
    SFGPU_RNG_UNIFORM = 1,      /* d_out: double [n][w], the first w values of uniform() */
    SFGPU_RNG_RATIO = 2,        /* d_out: double [n], ratio_of(d_a[i], d_b[i]) (no random numbers) */
    SFGPU_RNG_BINOMIAL = 3,     /* d_out: uint32 [n], binomial(d_n[i], p = d_a[i]) */
    SFGPU_RNG_BINOMIAL_INV = 4, /* d_out: uint32 [n], binomial_by_inversion(d_n[i], p = d_a[i]) */
    SFGPU_RNG_BLOCK = 5         /* d_out: uint32 [n][4], one raw Philox4x32-10 block: key = seed's low and high word, counter words 0, 1 =
                                 * d_stream[i]'s and 2, 3 = d_substream[i]'s (both required) -- the generator's published known answers */
};
SFGPU_API int sfgpu_rng_eval(int form, uint64_t seed, const uint64_t* d_stream, const uint64_t* d_substream, const uint32_t* d_n,
                             const double* d_a, const double* d_b, uint32_t w, uint64_t n, void* d_out, sfgpu_stream stream);
/* multinomial_chain over k weights d_w (their sum in member order is p_total): `count` draws of n reads with member `last` left out,
 * draw d from Philox(seed, d, 0), one lane per draw; d_out: uint32 [count][k].  light = 1: binomial_by_inversion (the phase kernel's
 * LIGHT form), 0: binomial; anything else is the unknown form. */
SFGPU_API int sfgpu_chain_eval(int light, const double* d_w, uint32_t k, uint32_t n, uint32_t last, uint64_t seed, uint64_t count,
                               uint32_t* d_out, sfgpu_stream stream);
/* The bootstrap's multinomial tree over the caller's own prefix sums (d_prefix[0 .. C], exclusive, of the class counts in the caller's
 * order -- sfgpu_bootstrap_counts works in the plan's): d_out[C] = draw `draw` of `seed` of n_total reads.  SFGPU_MN_TREE=levels as there. */
SFGPU_API int sfgpu_mn_tree_eval(const uint64_t* d_prefix, uint64_t C, uint32_t n_total, uint64_t seed, uint64_t draw, uint32_t* d_out,
                                 sfgpu_stream stream);

/* ---------------------------------------------------------------------------------------------
 * (next) A quasi-mapping front end: reads in, sfgpu_hit records out -- what the reference gets from RapMap's
 * SACollector inside processReadsQuasi (src/SailfishQuantify.cpp:141-142, 192-213 paired end, :487-488, 526-528 single
 * end), so that the hit lists the path consumes have a producer on the device.  RapMap (COMBINE-lab/RapMap @ sf-v0.10.1,
 * scripts/fetchRapMap.sh:20) is not in the reference tree; this is NOT its algorithm and parity with it is unpinned.
 * The contract (csrc/mapper.hip; oracle/mapper_oracle.py restates it): exact k-mer seeds at read offsets 0 and len - k,
 * forward strand then reverse complement; the first occurrence seen for a (transcript, strand) fixes the position;
 * hits sorted by (transcript, strand); mates on one transcript with opposite strands pair up (PAIRED_END_PAIRED,
 * fragment length = max end - min start), otherwise both mates' hits are kept as orphans (left run, right run).
 *   sfgpu_index_build : d_seq / d_seq_off / d_ref_len as for sfgpu_bias_create (transcript t = d_seq[d_seq_off[t] ..
 *                       + d_ref_len[t])); 8 <= k <= 31; max_occ = occurrences kept per lookup (0: 1000).
 *   sfgpu_map_reads   : reads of one batch, read r = d_seq1[d_off1[r] .. d_off1[r + 1]) (bytes; any case; other letters
 *                       than ACGT never match); d_seq2 / d_off2 = the mates or NULL.  Writes d_hit_offsets[n_reads + 1]
 *                       and, if they fit hit_capacity, the records (else SFGPU_ERR_RANGE with *n_hits set: size and
 *                       call again; d_hits = NULL with capacity 0 is the sizing call).  n_reads = 0: OK, d_hit_offsets[0] = 0, the
 *                       reads may be NULL.  A read with a mate of more than 65 535 bases gets no records (see sfgpu_index_set_scan).
 *                       The output feeds sfgpu_filter_hits directly.  Synchronous. */
typedef struct sfgpu_index sfgpu_index;
struct sfgpu_hit;
SFGPU_API int sfgpu_index_build(sfgpu_index** out, const char* d_seq, const uint64_t* d_seq_off, const uint32_t* d_ref_len, uint64_t M,
                                uint32_t k, uint32_t max_occ, sfgpu_stream stream);
SFGPU_API int sfgpu_index_destroy(sfgpu_index* idx);
/* Seeds per strand (default 2: offsets 0 and len - k, every (transcript, strand) either seed hits is kept).  With S > 2 the
 * seeds sit at offsets floor(j (len - k) / (S - 1)), j = 0 .. S-1, and a mate keeps only the (transcript, strand) pairs that the
 * most seeds hit: more sensitive on reads with errors (one clean k-mer is enough) without keeping what a single repeat k-mer
 * drags in.  2 <= S <= 8. */
SFGPU_API int sfgpu_index_set_seeds(sfgpu_index* x, uint32_t seeds_per_strand);
/* The mapping mode.  seed_len != 0 (the DEFAULT after sfgpu_index_build: min(19, k)): SCAN mode, modelled on RapMap's maximal
 * mappable prefixes -- the sorted k-mer table is used as a suffix array of depth k, a seed of seed_len <= k bases is a prefix
 * range of it.  A mate is walked on both strands in LOCKSTEP (one step on the forward strand, one on the reverse complement, and
 * so on; a match that covers the whole read ends both walks, and the 8 groups are shared by the two strands in the order they are
 * found).  A step: window at i -> prefix range; no occurrence or more than max_occ -> i += 1 (windows that hold a non-ACGT base are
 * skipped without a step);
 * otherwise every occurrence is extended base by base on the transcripts' text (the index keeps a copy), L = the longest
 * extension, the occurrences that reach L form a group, i += L - seed_len + 1 (at most 8 groups per mate).  A (transcript,
 * strand) is positioned by the first group that holds it and gets a vote per group; with several candidates only those with
 * the most votes are kept.  A read with substitutions maps as long as seed_len clean bases remain somewhere that an indexed
 * k-mer starts in: seeds are prefix ranges of WHOLE k-mers, so a seed that begins within the last k - 1 bases of a
 * transcript, or within k - 1 bases upstream of a non-ACGT base, is not in the index.
 * LENGTHS, both modes: read_len and mate_len are 16-bit fields.  A read with a mate of more than 65 535 bases gets NO records, single
 * end or paired and whichever mate it is (an orphan record carries the other mate's length too); at exactly 65 535 bases frag_len is
 * computed from the true lengths.  (This subsumes the scan mode's older limit of 2^24 - 1 bases.)
 * seed_len == 0: the END-SEED contract above (exact k-mers at offsets 0 and len - k, or sfgpu_index_set_seeds' S seeds) -- the
 * baseline of rounds 1-2.  8 <= seed_len <= k.  Parity with RapMap is unpinned in both modes. */
SFGPU_API int sfgpu_index_set_scan(sfgpu_index* x, uint32_t seed_len);
SFGPU_API int sfgpu_index_info(const sfgpu_index* idx, uint32_t* k, uint64_t* n_positions, uint64_t* n_kmers);
SFGPU_API int sfgpu_map_reads(const sfgpu_index* idx, const char* d_seq1, const uint64_t* d_off1, const char* d_seq2, const uint64_t* d_off2,
                              uint32_t n_reads, struct sfgpu_hit* d_hits, uint64_t hit_capacity, uint32_t* d_hit_offsets, uint64_t* n_hits,
                              sfgpu_stream stream);

/* ---------------------------------------------------------------------------------------------
 * (next) Per-read hit filtering: the loop bodies of processReadsQuasi
 * (src/SailfishQuantify.cpp:215-417 paired end, :530-626 single end) between "the mapper returned
 * jointHits for a read" and eqBuilder.addGroup -- maxReadOccs cut (:217, :532), orphan policy (:226),
 * orphan merge by transcript id (:231-246), library-type compatibility (sailfish::utils::compatibleHit /
 * hitType, src/SailfishUtils.cpp:157-289; pinned by the reference's tests/LibraryTypeTests.cpp), the
 * "compatible hits if any, else all hits unless enforceLibCompat" rule (:324-341, :355-368, :395-416) and
 * the fragment-length sampling of unique proper pairs (:419-434).  Bias / GC sampling: sfgpu_sample_bias below.
 * One record per hit, reads in CSR form; the output is the packed hit lists sfgpu_eq_add_batch_device
 * takes (reads that end up unmapped get an empty list), so labels never visit the host.
 * Enum values: mate_status 0 SINGLE_END, 1 PAIRED_END_LEFT, 2 PAIRED_END_RIGHT, 3 PAIRED_END_PAIRED (the
 * adaptor maps rapmap::utils::MateStatus); sfgpu_libfmt fields as include/LibraryFormat.hpp:7-9
 * (type 0 SE / 1 PE; orientation 0 SAME, 1 AWAY, 2 TOWARD, 3 NONE; strandedness 0 SA, 1 AS, 2 S, 3 A, 4 U).
 * ------------------------------------------------------------------------------------------- */
typedef struct sfgpu_hit {
    uint32_t tid;          /* QuasiAlignment::transcriptID() */
    int32_t  pos;          /* h.pos */
    int32_t  mate_pos;     /* h.matePos */
    uint32_t frag_len;     /* h.fragLen */
    uint16_t read_len;     /* h.readLen */
    uint16_t mate_len;     /* h.mateLen */
    uint8_t  fwd;          /* h.fwd */
    uint8_t  mate_fwd;     /* h.mateIsFwd */
    uint8_t  mate_status;  /* h.mateStatus */
    uint8_t  pad_;
} sfgpu_hit;               /* 24 bytes */
typedef struct sfgpu_libfmt { uint8_t type, orientation, strandedness, pad_; } sfgpu_libfmt;
typedef struct sfgpu_filter_opts {
    uint32_t max_read_occs;     /* sfOpts.maxReadOccs */
    uint32_t max_frag_len;      /* sfOpts.maxFragLen: size of the fragment-length histogram */
    int32_t  paired_library;    /* 1: the paired-end loop (:215-417), 0: the single-end loop (:530-626) */
    int32_t  discard_orphans;   /* !sfOpts.allowOrphans (:139) */
    int32_t  ignore_compat;     /* sfOpts.ignoreLibCompat (:156) */
    int32_t  enforce_compat;    /* sfOpts.enforceLibCompat (:160) */
    int32_t  can_dovetail;      /* sfOpts.allowDovetail (:165) */
    sfgpu_libfmt expected;      /* rl.format() (:163) */
} sfgpu_filter_opts;
typedef struct sfgpu_filter_stats {   /* all ACCUMULATED by the call */
    uint64_t n_observed;        /* numObservedFragments */
    uint64_t n_mapped;          /* validHits: reads handed to addGroup */
    uint64_t total_hits;        /* totalHits (after the maxReadOccs / orphan cuts) */
    uint64_t upper_bound_hits;  /* upperBoundHits: reads with at least one hit before the cuts */
    uint64_t n_fwd, n_rc;       /* readExp.addNumFwd / addNumRC */
    uint64_t fl_sampled;        /* fragment lengths added to the histogram by this call */
} sfgpu_filter_stats;
/* d_hits[d_hit_offsets[r] .. d_hit_offsets[r+1]) are read r's hits in the mapper's order (for orphans: left
 * mate's hits first, each run ascending in tid, as mergeLeftRightHits leaves them).
 * d_ids_out needs room for d_hit_offsets[n_reads] ids; d_offsets_out for n_reads + 1.
 * d_fl_counts (max_frag_len uint32, may be NULL) and *remaining_fl_ops (may be NULL) carry the
 * fragment-length histogram and its sample budget across calls: the first *remaining_fl_ops qualifying
 * reads in read order are counted, exactly what one mapping thread does.  Synchronous. */
SFGPU_API int sfgpu_filter_hits(const sfgpu_hit* d_hits, const uint32_t* d_hit_offsets, uint32_t n_reads,
                      const sfgpu_filter_opts* opts, uint32_t* d_ids_out, uint32_t* d_offsets_out,
                      uint32_t* d_fl_counts, int64_t* remaining_fl_ops, sfgpu_filter_stats* stats, sfgpu_stream stream);

/* ---------------------------------------------------------------------------------------------
 * Verification of the mapper's hit records against the transcripts' bases: an optional pass between sfgpu_map_reads and whatever
 * consumes its records.  The mapper places a mate on the strength of one exact match and never compares the rest; this pass scores
 * every record, ungapped, on the diagonal the mapper recorded, drops the records that fail and optionally all but the best of a
 * read.  What it means is stated once, serially, in csrc/verifyfmt.h (hits.verify_hits_host is the Python statement):
 *   job     one mate of one record.  mate_status 0 / 1: mate 1's bases on strand fwd at pos; 2: mate 2's bases on strand fwd at
 *           pos; 3: two jobs -- mate 1, fwd, pos and mate 2, mate_fwd, mate_pos.  len = the mate's length from d_off1 / d_off2
 *           (not the record's 16-bit read_len / mate_len).
 *   bases   oriented base j: forward code(r[j]), reverse 3 - code(r[len - 1 - j]) (A C G T in either case -> 0 .. 3, anything else
 *           4 on either strand).  Transcript position x = pos + j: x < 0 or x >= the transcript's length counts in `over`;
 *           otherwise a mismatch (`mism`) when either code is 4 or the codes differ (N against N is a mismatch).
 *   pass    a job passes iff 1000 * (len - over - mism) >= min_identity_permille * len; a record passes iff all its jobs do (a
 *           pair stands or falls as a whole).  keep_best != 0: of a read's passing records only those with the read's minimum
 *           cost (mism + over summed over the record's jobs) survive.
 *   output  the survivors in input order (d_hits_out, room for d_hit_offsets[n_reads] records), CSR offsets over the same reads
 *           (d_offsets_out, n_reads + 1), one score per survivor (d_scores_out, may be NULL; the fields saturate at 65 535, the
 *           decisions use the unsaturated counts), *n_out = the survivors.  The outputs must not overlap the inputs.
 *   errors  a record with tid >= the index's transcript count: SFGPU_ERR_RANGE, sfgpu_last_error names the lowest such record, the
 *           outputs are left untouched.  NULL idx / opts / n_out / stats, min_identity_permille > 1000, or NULL reads, records or
 *           outputs where n_reads > 0 needs them: SFGPU_ERR_INVALID.  d_seq2 / d_off2 = NULL: single end (a record that
 *           names mate 2 is then SFGPU_ERR_INVALID).
 * Ungapped: a read with an indel fails past the indel.  Synchronous.  The stats are SET by the call. */
typedef struct sfgpu_hit_score { uint16_t mism, over, mate_mism, mate_over; } sfgpu_hit_score;      /* 8 bytes */
typedef struct sfgpu_verify_opts {
    uint32_t min_identity_permille;   /* 0 .. 1000 */
    int32_t  keep_best;
} sfgpu_verify_opts;
typedef struct sfgpu_verify_stats {
    uint64_t records_in, records_out;
    uint64_t reads_in, reads_out;     /* reads with at least one record, before and after */
    uint64_t failed_identity;         /* records with a job below min_identity_permille */
    uint64_t dropped_not_best;        /* passing records dropped by keep_best */
    uint64_t sum_mism;                /* mism over the survivors' jobs, unsaturated */
} sfgpu_verify_stats;
SFGPU_API int sfgpu_hits_verify(const sfgpu_index* idx, const char* d_seq1, const uint64_t* d_off1, const char* d_seq2, const uint64_t* d_off2,
                                uint32_t n_reads, const sfgpu_hit* d_hits, const uint32_t* d_hit_offsets, const sfgpu_verify_opts* opts,
                                sfgpu_hit* d_hits_out, uint32_t* d_offsets_out, sfgpu_hit_score* d_scores_out, uint64_t* n_out,
                                sfgpu_verify_stats* stats, sfgpu_stream stream);

/* The same pass scored WITH GAPS: a job's banded edit distance in place of its ungapped count, so that a read with an indel against
 * the transcript keeps its true record.  Arguments, jobs, base codes, orientation, output layout and order are sfgpu_hits_verify's;
 * the rule is stated once in csrc/verifygfmt.h (hits.gapped_edits_host / hits.verify_hits_gapped_host are the Python statement).
 * For a job of len oriented bases a[] at pos on a transcript of tlen bases, with band k = max_indel (1 .. 15):
 *   cells   D[i][d], rows i = -1 .. len - 1, diagonals d = -k .. k; cell (i, d) aligns read base i to x = pos + i + d.  The column
 *           character is the transcript's base code for 0 <= x < tlen and OFF elsewhere; sub(i, x) = 0 iff a[i] is a base and equals
 *           it, else 1 (N matches nothing, OFF matches nothing).
 *   start   D[-1][d] = 0 for every d: the start diagonal is free, since the mapper's seed may lie behind an indel.
 *   row     V[d] = min(D[i-1][d] + sub(i, pos + i + d), D[i-1][d+1] + 1) (the second term for d < k), then
 *           D[i][d] = min over d' <= d of V[d'] + (d - d').
 *   edits   min over d of D[len-1][d]; 0 for len == 0.  edits <= mism + over of the ungapped pass (k = 0 would be equal).
 *   pass    a job passes iff 1000 * (len - edits) >= min_identity_permille * len; a record iff all its jobs do.  keep_best: of a
 *           read's passing records those of least cost (edits summed over the record's jobs, unsaturated).
 *   score   per survivor {edits, ungapped, mate_edits, mate_ungapped}: ungapped = mism + over on the recorded diagonal; the fields
 *           saturate at 65 535 (the decisions use the unsaturated values); the mate fields are 0 unless the status is 3.
 *   stats   as sfgpu_verify_stats with sum_edits for sum_mism, and `rescued`: the survivors with at least one job that the ungapped
 *           rule (1000 * (len - over - mism) >= min_identity_permille * len) fails.
 *   errors  as sfgpu_hits_verify (tid >= M: SFGPU_ERR_RANGE naming the lowest record, the outputs untouched; a record naming mate 2 of
 *           a single-end batch: SFGPU_ERR_INVALID); max_indel outside 1 .. 15: SFGPU_ERR_INVALID.
 * The records' pos, and so the CIGAR and POS a mappings writer derives from them, still describe the recorded diagonal.  Mates
 * shorter than 2^30 bases.  Synchronous.  The stats are SET by the call. */
typedef struct sfgpu_hit_gscore { uint16_t edits, ungapped, mate_edits, mate_ungapped; } sfgpu_hit_gscore;      /* 8 bytes */
typedef struct sfgpu_verify_gopts {
    uint32_t min_identity_permille;   /* 0 .. 1000 */
    int32_t  keep_best;
    uint32_t max_indel;               /* 1 .. 15: the band's half width */
} sfgpu_verify_gopts;
typedef struct sfgpu_verify_gstats {
    uint64_t records_in, records_out;
    uint64_t reads_in, reads_out;     /* reads with at least one record, before and after */
    uint64_t failed_identity;         /* records with a job below min_identity_permille */
    uint64_t dropped_not_best;        /* passing records dropped by keep_best */
    uint64_t sum_edits;               /* edits over the survivors' jobs, unsaturated */
    uint64_t rescued;                 /* survivors that the ungapped rule would have dropped */
} sfgpu_verify_gstats;
SFGPU_API int sfgpu_hits_verify_gapped(const sfgpu_index* idx, const char* d_seq1, const uint64_t* d_off1, const char* d_seq2, const uint64_t* d_off2,
                                       uint32_t n_reads, const sfgpu_hit* d_hits, const uint32_t* d_hit_offsets, const sfgpu_verify_gopts* opts,
                                       sfgpu_hit* d_hits_out, uint32_t* d_offsets_out, sfgpu_hit_gscore* d_scores_out, uint64_t* n_out,
                                       sfgpu_verify_gstats* stats, sfgpu_stream stream);

/* MATE RESCUE: an optional pass between sfgpu_map_reads and sfgpu_hits_verify.  The mapper places a mate on one exact seed; a pair
 * of which one mate found none leaves it as orphan records only.  This pass searches each such orphan's transcript for the missing
 * mate, ungapped and with sfgpu_hits_verify's base comparison, inside the window an inward-facing fragment allows, and turns the
 * orphan into a pair where it finds a placement.  Arguments, base codes and orientation are sfgpu_hits_verify's (paired batches
 * only); the rule is stated once in csrc/rescuefmt.h (hits.rescue_mates_host is the Python statement):
 *   reads       a read is eligible iff it has at least one record and every record has mate_status 1 or 2; every other read keeps
 *               its records unchanged and in order.
 *   job         one orphan record of an eligible read.  The anchor is the mate it places (mate 1 for status 1, mate 2 for status 2)
 *               at p = pos on strand f = fwd, la bases long (from d_off1 / d_off2, not the 16-bit fields); the missing mate is the
 *               other one, lb bases, oriented on strand 1 - f.
 *   candidates  x with 0 <= x <= tlen - lb and, W = opts->window: f == 1: x >= p and x + lb <= p + W; f == 0: x + lb <= p + la and
 *               x >= p + la - W (inward facing, no dovetail).  lb == 0, lb > tlen, lb > 65 535 and la > 65 535 give none.
 *   score       mism(x) = the columns j < lb where either code is 4 or the codes differ against transcript base x + j.  A candidate
 *               passes iff 1000 * (lb - mism) >= min_identity_permille * lb; the placement is the passing candidate of least mism,
 *               the lowest x on a tie.
 *   record      status 1 -> {tid, p, x, frag, len1, len2, f, 1 - f, 3, 0}; status 2 -> {tid, x, p, frag, len1, len2, 1 - f, f, 3, 0};
 *               frag = max(ends) - min(starts), as sfgpu_map_reads computes it.
 *   read        at least one job placed: the read's records become the placed records only, ordered by (tid, fwd) ascending and by
 *               input order on equal keys (the order sfgpu_map_reads leaves for pairs); none placed: the read keeps its orphans.
 *   output      d_hits_out (room for d_hit_offsets[n_reads] records: never more go out than came in), CSR offsets over the same
 *               reads (d_offsets_out, n_reads + 1), per output record the placed mate's mism saturated at 65 535 (d_mism_out, may
 *               be NULL; 0 for records that passed through), *n_out = the records.  The outputs must not overlap the inputs.
 *   errors      a record with tid >= the index's transcript count: SFGPU_ERR_RANGE, sfgpu_last_error names the lowest such record,
 *               the outputs are left untouched.  A single-end batch (d_seq2 == NULL), min_identity_permille > 1000, a window
 *               outside 1 .. 2^20, NULL idx / opts / n_out / stats, or NULL reads, records or outputs where n_reads > 0 needs
 *               them: SFGPU_ERR_INVALID.
 * Synchronous.  The stats are SET by the call. */
typedef struct sfgpu_rescue_opts {
    uint32_t min_identity_permille;   /* 0 .. 1000 */
    uint32_t window;                  /* 1 .. 2^20: the longest fragment searched for */
} sfgpu_rescue_opts;
typedef struct sfgpu_rescue_stats {
    uint64_t reads_eligible;          /* reads whose records are all orphans */
    uint64_t records_orphan;          /* their records: the jobs */
    uint64_t jobs_with_candidates;
    uint64_t candidates;              /* sum of the window sizes */
    uint64_t reads_rescued, records_rescued;
    uint64_t records_dropped;         /* orphans of rescued reads that found no mate */
    uint64_t sum_mism;                /* mism of the placed mates, unsaturated */
} sfgpu_rescue_stats;
SFGPU_API int sfgpu_hits_rescue_mates(const sfgpu_index* idx, const char* d_seq1, const uint64_t* d_off1, const char* d_seq2, const uint64_t* d_off2,
                                      uint32_t n_reads, const sfgpu_hit* d_hits, const uint32_t* d_hit_offsets, const sfgpu_rescue_opts* opts,
                                      sfgpu_hit* d_hits_out, uint32_t* d_offsets_out, uint16_t* d_mism_out, uint64_t* n_out,
                                      sfgpu_rescue_stats* stats, sfgpu_stream stream);

/* The gapped ALIGNMENT of the records that survive sfgpu_hits_verify_gapped: the path through the same band, as a position and
 * BAM CIGAR words per job.  Arguments, jobs, base codes and orientation are sfgpu_hits_verify_gapped's; the rule, with its tie
 * rules, is stated once in csrc/aligngfmt.h (hits.align_hits_host is the Python statement):
 *   walk    from the end cell (D[len-1][d] == edits with least |d|, the negative one on a tie) back to row -1, a gap once opened
 *           continued while it is a candidate, else the first candidate of diagonal, read base unaligned (I), transcript base
 *           skipped (D).
 *   trim    at either end columns are dropped until a base aligned to a transcript position 0 <= x < tlen remains: dropped read bases
 *           are that end's soft clip, dropped D columns vanish.  Nothing left: the job is unalignable and has no operations.
 *   slots   two per record: slot 2 h + j is job j of record h; the second slot of a record with one job is empty.
 *   output  d_pos[slot] (the transcript position of the first remaining column, 0-based; 0 where there are no operations),
 *           d_nm[slot] (mismatching aligned bases + I + D bases), d_op_off[2 n + 1] (CSR over the slots, n =
 *           d_hit_offsets[n_reads]), d_ops[] (len << 4 | op with M 0, I 1, D 2, S 4, in reference order; room for cap_ops words).
 *           *n_ops = the words needed.  They do not fit cap_ops: SFGPU_ERR_RANGE, *n_ops is still set and nothing is written.
 *   scratch 8 * width * ceil(len / 16) bytes per job whose ungapped count is not 0 (width 16 for max_indel <= 7, else 32).  The
 *           slots run in slices whose scratch stays within scratch_cap_bytes (0: 256 MiB); a single job above it runs alone.
 *           The cap bounds memory and never changes a result.
 *   errors  as sfgpu_hits_verify_gapped, the outputs untouched: tid >= M: SFGPU_ERR_RANGE naming the lowest record; NULL
 *           pointers, max_indel outside 1 .. 15, a record naming mate 2 of a single-end batch: SFGPU_ERR_INVALID.
 * Mates shorter than 2^28 bases.  Synchronous.  The stats are SET by the call. */
typedef struct sfgpu_align_gopts {
    uint32_t max_indel;               /* 1 .. 15 */
    uint32_t reserved;                /* 0 */
    uint64_t scratch_cap_bytes;       /* 0: 256 MiB */
} sfgpu_align_gopts;
typedef struct sfgpu_align_gstats {
    uint64_t jobs;                    /* slots that are a job */
    uint64_t jobs_traced;             /* ... whose ungapped count is not 0: the recurrence and the walk ran */
    uint64_t unalignable;             /* jobs without an operation */
    uint64_t sum_nm;
    uint64_t words;                   /* operations over all slots */
    uint64_t scratch_bytes;           /* the largest slice's scratch */
} sfgpu_align_gstats;
SFGPU_API int sfgpu_hits_align_gapped(const sfgpu_index* idx, const char* d_seq1, const uint64_t* d_off1, const char* d_seq2, const uint64_t* d_off2,
                                      uint32_t n_reads, const sfgpu_hit* d_hits, const uint32_t* d_hit_offsets, const sfgpu_align_gopts* opts,
                                      int32_t* d_pos, uint32_t* d_nm, uint64_t* d_op_off, uint32_t* d_ops, uint64_t cap_ops, uint64_t* n_ops,
                                      sfgpu_align_gstats* stats, sfgpu_stream stream);

/* The NM and MD tags of the lines a mappings file holds for these records (the rule is stated once in csrc/mdfmt.h;
 * hits.md_tags_host is the Python statement).  Records, reads, jobs, base codes and orientation are sfgpu_hits_align_gapped's.
 *   slots   two per record: slot 2 h + which is line `which` of record h; a record's missing second slot has nm 0 and no MD byte.
 *   cigar   d_aln_pos / d_aln_op_off / d_aln_ops (sfgpu_hits_align_gapped's d_pos, d_op_off, d_ops for the same records; all three
 *           or none, anything else: SFGPU_ERR_INVALID): the slot's words at POS - 1 = d_aln_pos[slot].  Without them the line's
 *           ungapped CIGAR, <clip>S<match>M from the record's pos and read_len (mate_pos and mate_len on the second line).  A line
 *           the writer refuses (no base on the transcript; a slot without an operation) has nm 0 and MD "0".
 *   walk    over the ORIENTED mate and the transcript from POS - 1.  An M / = / X column is a mismatch iff it lies off the
 *           transcript or past the mate's bases, or either base is not A C G T, or the bases differ: <run><reference character>,
 *           nm + 1; else the run of matches grows.  I n: nm + n.  D n / N n: <run>^<n reference characters>, nm + n.  At the end
 *           <run>.  The reference character is the transcript's byte upper-cased, N where that is no letter or off the transcript.
 *           For a slot sfgpu_hits_align_gapped produced, nm equals its d_nm.
 *   output  d_nm[2 n], d_md_off[2 n + 1] (CSR over the slots, n = d_hit_offsets[n_reads]), d_md[] (room for cap_md bytes; no
 *           terminator).  *n_md = the bytes needed.  They do not fit cap_md: SFGPU_ERR_RANGE, *n_md is still set and nothing is
 *           written.  NH is not an output: it is d_hit_offsets[r + 1] - d_hit_offsets[r], which the writer reads itself.
 *   errors  the outputs untouched: tid >= M: SFGPU_ERR_RANGE naming the lowest record; NULL pointers, a record naming mate 2 of a
 *           single-end batch: SFGPU_ERR_INVALID.
 * Mates and operations shorter than 2^28 bases.  Synchronous.  The stats are SET by the call. */
typedef struct sfgpu_mdtag_stats {
    uint64_t slots;                   /* slots that are a line */
    uint64_t sum_nm;
    uint64_t md_bytes;                /* over all slots */
    uint64_t max_md_bytes;            /* of the longest MD */
    uint64_t slots_plain;             /* lines whose CIGAR is one M operation and whose nm is 0: the MD is <len> */
} sfgpu_mdtag_stats;
SFGPU_API int sfgpu_hits_md_tags(const sfgpu_index* idx, const char* d_seq1, const uint64_t* d_off1, const char* d_seq2, const uint64_t* d_off2,
                                 uint32_t n_reads, const sfgpu_hit* d_hits, const uint32_t* d_hit_offsets, const int32_t* d_aln_pos,
                                 const uint64_t* d_aln_op_off, const uint32_t* d_aln_ops, uint32_t* d_nm, uint64_t* d_md_off, uint8_t* d_md,
                                 uint64_t cap_md, uint64_t* n_md, sfgpu_mdtag_stats* stats, sfgpu_stream stream);

/* The posterior probability of every record of a batch under a weight per transcript, and what a mappings file says of it in its
 * ZW:f: tag (the rule is stated once in csrc/postfmt.h; hits.posteriors_host is the Python statement).  Only tid is read of a
 * record; no index and no read bases are needed.
 *   weight  x_h = d_weights[tid_h], a weight below 2^-960 reading as 0.  Every record is a candidate of its own: a transcript that
 *           holds two records of a read has two terms.
 *   sum     S over the n records of a read, in a fixed order whatever way the work is laid out: 64 accumulators a_j = x_j +
 *           x_{j+64} + ... serially and ascending, then a_j += a_{j xor k} for k = 32, 16, 8, 4, 2, 1; S = a_0.
 *   value   p_h = x_h / S where S > 0, else 1 / n; a p_h below 2^-56 is written as 0.
 *   output  d_p[n] the values; d_rec[n] their six-digit records (csrc/gfmt.h: the token is printf("%g", p)); d_f32[n] the float a
 *           BAM reader gets from that token, (float)strtod(token); n = d_hit_offsets[n_reads].  n_reads == 0 is a valid call.
 *   errors  the outputs untouched, the weights checked first: a weight that is negative, NaN, infinite or above 2^960:
 *           SFGPU_ERR_INVALID naming the lowest transcript; tid >= n_refs: SFGPU_ERR_RANGE naming the lowest record; NULL pointers:
 *           SFGPU_ERR_INVALID.
 * Synchronous.  The stats are SET by the call. */
typedef struct sfgpu_posterior_stats {
    uint64_t reads;
    uint64_t reads_mapped;            /* reads with a record */
    uint64_t reads_multi;             /* ... with two or more */
    uint64_t records;
    uint64_t reads_flat;              /* reads with records whose S is 0: 1 / n each */
    uint64_t records_zero;            /* records whose p is written as 0 */
    uint64_t max_records;             /* of the read with the most */
} sfgpu_posterior_stats;
SFGPU_API int sfgpu_hits_posteriors(const sfgpu_hit* d_hits, const uint32_t* d_hit_offsets, uint32_t n_reads, const double* d_weights, uint64_t n_refs,
                                    double* d_p, uint32_t* d_rec, float* d_f32, sfgpu_posterior_stats* stats, sfgpu_stream stream);

/* What library format a batch's records show: the tally behind lib_format "A" and aux/lib_format_counts.json (the rule is stated
 * once in csrc/libdetfmt.h; hits.library_kinds_host is the Python statement).  No index and no read bases are needed.
 *   kind    of a record, SFGPU_LIBDET_KINDS of them: 0 .. 5 ISF ISR OSF OSR MSF MSR (mate_status 3, the reference's hitType on the
 *           s1, s2 that sfgpu_filter_hits computes; the dovetail stretch iff can_dovetail), 6 .. 9 LF LR RF RR (orphans: status 1 / 2,
 *           forward / reverse), 10 11 SF SR (status 0), 12 any other status byte.
 *   read    no record: counted in `reads` only.  More than max_read_occs records: reads_over_occs and nothing else (the filter drops
 *           it too).  Else reads_mapped; every record in records_kind; the read in reads_kind[k] where all its records are of kind k,
 *           else in reads_mixed; with has_expected, in reads_compatible iff one of its kinds is one that sfgpu_filter_hits accepts
 *           for `expected`.
 *   votes   a mapped read votes iff all its records are of one kind and that is 0 .. 5 (paired_library) or 10 / 11 (single end).
 *           The first *remaining_votes voters in read order are counted in votes_kind / votes and taken off *remaining_votes, which
 *           carries the budget across calls as remaining_fl_ops does: the tally does not depend on how the reads were cut into
 *           batches.  With *remaining_votes == 0 no vote is looked for.
 *   errors  NULL d_hit_offsets (with n_reads > 0), opts, remaining_votes or stats, NULL d_hits with records: SFGPU_ERR_INVALID;
 *           n_reads >= 2^31: SFGPU_ERR_RANGE.  Nothing is added then.  n_reads == 0 is a valid call.
 * Synchronous.  The stats are ACCUMULATED by the call.  There is no host path. */
#define SFGPU_LIBDET_KINDS 13
typedef struct sfgpu_libdet_opts {
    uint32_t max_read_occs;           /* sfOpts.maxReadOccs, as sfgpu_filter_opts */
    int32_t  paired_library;          /* which kinds vote */
    int32_t  can_dovetail;            /* sfOpts.allowDovetail */
    int32_t  has_expected;            /* 1: count reads_compatible against `expected` */
    sfgpu_libfmt expected;
} sfgpu_libdet_opts;
typedef struct sfgpu_libdet_stats {
    uint64_t reads;
    uint64_t reads_mapped;            /* 1 .. max_read_occs records */
    uint64_t reads_over_occs;
    uint64_t reads_mixed;             /* mapped, records of more than one kind */
    uint64_t reads_compatible;
    uint64_t votes;                   /* the sum of votes_kind */
    uint64_t records_kind[SFGPU_LIBDET_KINDS];
    uint64_t reads_kind[SFGPU_LIBDET_KINDS];
    uint64_t votes_kind[SFGPU_LIBDET_KINDS];
} sfgpu_libdet_stats;
SFGPU_API int sfgpu_hits_library_kinds(const sfgpu_hit* d_hits, const uint32_t* d_hit_offsets, uint32_t n_reads, const sfgpu_libdet_opts* opts,
                                       int64_t* remaining_votes, sfgpu_libdet_stats* stats, sfgpu_stream stream);

/* Posterior-weighted coverage of the transcripts by the mappings, accumulated over the batches of a run, and its bedGraph file (the
 * rule is stated once in csrc/coverfmt.h; hits.coverage_host is the Python statement).  Only a record's own fields and the transcript
 * lengths are read; no index and no read bases are needed.
 *   open     d_ref_len[M] is read once; the handle then holds ONE uint64 array of sum(len) + M slots (8 bytes each: about 3.6 GB for
 *            a transcriptome of 450 M bases), transcript t owning len_t + 1 of them.  M == 0 is valid.  A length of 2^32 - 1:
 *            SFGPU_ERR_RANGE.
 *   add      a record's line 0 is (pos, read_len), a mate_status == 3 record has line 1, (mate_pos, mate_len).  Without alignments a
 *            line is the interval [max(pos, 0), min(pos + len, len_t)).  With d_aln_pos / d_aln_op_off / d_aln_ops (all three or none:
 *            sfgpu_hits_align_gapped's outputs for the same records, slot 2 h + which) its words are walked from d_aln_pos[slot]: M, =
 *            and X cover [x, x + n) clipped to the transcript and advance x, D and N advance x, I, S, H and P do neither; a slot
 *            without operations has no interval.  An interval [a, b) adds q to slot a and takes it off slot b, q = trunc(p 2^32) of
 *            the record's d_p (both lines of a pair carry it), or floor(2^32 / n), n the read's record count, where d_p is NULL.
 *            Empty intervals add nothing and are counted.  64-bit integer atomics: the result does not depend on any order.
 *            errors, state and stats untouched: tid >= M: SFGPU_ERR_RANGE naming the lowest record; a p that is NaN, negative or above
 *            1: SFGPU_ERR_INVALID naming the lowest record; lines that would bring the handle's total to 2^32: SFGPU_ERR_RANGE; a call
 *            after finish: SFGPU_ERR_INVALID.  n_reads == 0 is a valid call.  The stats are ACCUMULATED by the call.
 *   finish   one inclusive scan turns the slots into sums (every transcript's last slot then reads 0: `residue` counts those that do
 *            not and must be 0); the runs -- maximal stretches of one transcript's bases with one nonzero sum, by transcript, then
 *            start -- are counted per block, placed by a scan and written as (tid, start, end, sum); a wavefront per transcript
 *            folds its bases into covered, the 128-bit sum and the maximum, and the three columns CoveredFraction = covered / len,
 *            MeanDepth = (double)floor(S / len) 2^-32, MaxDepth = (double)max 2^-32 (0 for len == 0).  A second finish returns the
 *            same result.
 *   runs / summary   copies of the results into the caller's device arrays (n_runs and M entries; a NULL pointer is skipped); before
 *            finish: SFGPU_ERR_STATE.
 *   write    the rows name \t start \t end \t %g(sum 2^-32) \n, 0-based and half open, without a header line, formatted in 4 KB tiles
 *            and handed over in chunks as sfgpu_quant_write_text's rows are (d_names / d_name_off[M + 1] and chunk_bytes as there; sink
 *            NULL: only sized); sfgpu_cov_write_bgzf hands the chunks to the BGZF encoder where they lie, as sfgpu_reads_write_bgzf
 *            does.  Before finish: SFGPU_ERR_STATE.
 * Synchronous. */
typedef struct sfgpu_cov sfgpu_cov;
typedef struct sfgpu_cov_stats {
    uint64_t reads;
    uint64_t records;
    uint64_t lines;
    uint64_t intervals;               /* added */
    uint64_t empty_intervals;         /* nothing left after the clip */
    uint64_t bases_added;             /* the bases of the added intervals */
} sfgpu_cov_stats;
typedef struct sfgpu_cov_result {
    uint64_t n_runs;
    uint64_t bases_covered, bases_total;
    uint64_t residue;                 /* transcripts whose last slot is not 0 after the scan: 0 */
    uint64_t state_bytes;             /* device memory the handle holds */
    uint64_t n_bytes, n_chunks, max_row_bytes;      /* of a write */
    double finish_ms, format_ms, d2h_ms, sink_ms;
} sfgpu_cov_result;
SFGPU_API int sfgpu_cov_open(sfgpu_cov** out, const uint32_t* d_ref_len, uint64_t M, sfgpu_stream stream);
SFGPU_API int sfgpu_cov_close(sfgpu_cov* c);
SFGPU_API int sfgpu_cov_add(sfgpu_cov* c, const sfgpu_hit* d_hits, const uint32_t* d_hit_offsets, uint32_t n_reads, const double* d_p,
                            const int32_t* d_aln_pos, const uint64_t* d_aln_op_off, const uint32_t* d_aln_ops, sfgpu_cov_stats* stats,
                            sfgpu_stream stream);
SFGPU_API int sfgpu_cov_finish(sfgpu_cov* c, sfgpu_cov_result* out, sfgpu_stream stream);
SFGPU_API int sfgpu_cov_runs(sfgpu_cov* c, uint32_t* d_tid, uint32_t* d_start, uint32_t* d_end, uint64_t* d_sum);
SFGPU_API int sfgpu_cov_summary(sfgpu_cov* c, double* d_covered_fraction, double* d_mean, double* d_max);
SFGPU_API int sfgpu_cov_write_text(sfgpu_cov* c, const char* d_names, const uint64_t* d_name_off, uint64_t chunk_bytes, sfgpu_text_sink sink,
                                   void* user, sfgpu_cov_result* out, sfgpu_stream stream);
SFGPU_API int sfgpu_cov_write_bgzf(sfgpu_cov* c, const char* d_names, const uint64_t* d_name_off, uint64_t chunk_bytes, sfgpu_bgzw* z,
                                   sfgpu_cov_result* out, sfgpu_stream stream);

/* The coverage of the chromosomes: a finished sfgpu_cov's runs projected through the transcripts' exon blocks, summed per genomic base,
 * and its bedGraph file (the rule is stated once in csrc/covgfmt.h; hits.coverage_genome_host is the Python statement).
 *   open     the model, read once and copied onto the handle: d_status[M] (0 = placed, anything else not), d_chrom[M] and d_strand[M]
 *            (+1 / -1; both read for placed transcripts only), d_exon_off[M + 1] and the blocks d_exon_start / d_exon_len
 *            [d_exon_off[M]] in TRANSCRIPT order, 0-based.  It is validated on the device: the offsets start at 0 and never decrease;
 *            every block has 1 <= len and start + len <= 2^32 - 1; a placed transcript has a chromosome below n_chrom, a strand of
 *            +1 or -1, and blocks that ascend on + and descend on - without overlapping (touching is fine).  A model that fails:
 *            SFGPU_ERR_INVALID with the lowest offending transcript in the error text.  2^32 - 1 blocks or more: SFGPU_ERR_RANGE.
 *            The handle also keeps the 64-bit prefix sums of the block lengths, which place a block in its transcript.
 *   project  `finished` is a handle after sfgpu_cov_finish (before: SFGPU_ERR_STATE; another M than the model's: SFGPU_ERR_INVALID).
 *            A lane per transcript run finds its first and last block by binary search and leaves the piece count; the counts are
 *            scanned; runs of up to 8 pieces write their events (key = chrom << 32 | position, +sum at a piece's start, -sum at its
 *            end) a lane each, longer ones a wavefront each in a second launch.  The keys are sorted with the event index as payload,
 *            the 64-bit deltas gathered and scanned inclusively: the sum after a key's LAST event is the sum that holds from it on
 *            (a key's delta is the difference of the scan across its events -- a segmented sum by subtraction, no atomics on the
 *            sums).  The last events of the keys are compacted; a key whose sum equals the key's before it has delta 0 and neither
 *            opens nor closes anything; the runs are counted, placed by a scan and written as (chrom, start, end, sum), by chromosome,
 *            then start.  2^32 - 1 events or more: SFGPU_ERR_RANGE, and the handle keeps what it had.  May be called again (for
 *            instance after a refusal); the last result is the one runs and write show.
 *   event_cap  for tests: projections of this handle refuse `cap` events or more (0, or anything above it: the 2^32 - 1 of the rule).
 *   runs     copies of the result into the caller's device arrays (n_runs entries; a NULL pointer is skipped); before project:
 *            SFGPU_ERR_STATE.
 *   write    the rows chrom \t start \t end \t %g(sum 2^-32) \n through the transcript file's formatter and chunk loop:
 *            d_chrom_names / d_chrom_name_off[n_chrom + 1], chunk_bytes, sink and z as in sfgpu_cov_write_text / _bgzf.  Before
 *            project: SFGPU_ERR_STATE.
 * Synchronous. */
typedef struct sfgpu_covg sfgpu_covg;
typedef struct sfgpu_covg_result {
    uint64_t n_pieces, n_events;
    uint64_t n_keys;                  /* distinct keys whose delta is not 0 */
    uint64_t n_runs, bases_covered;
    uint64_t runs_unplaced, bases_unplaced;         /* runs of transcripts that are not placed, dropped whole */
    uint64_t bases_off_model;         /* bases of placed transcripts' runs at or beyond the blocks' total length */
    uint64_t transcripts_placed;
    uint64_t transcripts_length_mismatch;           /* placed, and the blocks' total length is not the transcript's */
    uint64_t state_bytes;             /* device memory held at the projection's peak, scratch included */
    uint64_t n_bytes, n_chunks, max_row_bytes;      /* of a write */
    double project_ms, format_ms, d2h_ms, sink_ms;
    double emit_ms, sort_ms, sum_ms, runs_ms;       /* project_ms by stage: count, scan and emit; the sort; gather and scan; the runs */
} sfgpu_covg_result;
SFGPU_API int sfgpu_covg_open(sfgpu_covg** out, const uint8_t* d_status, const int32_t* d_chrom, const int8_t* d_strand, const uint64_t* d_exon_off,
                              const uint32_t* d_exon_start, const uint32_t* d_exon_len, uint64_t M, uint32_t n_chrom, sfgpu_stream stream);
SFGPU_API int sfgpu_covg_close(sfgpu_covg* g);
SFGPU_API int sfgpu_covg_event_cap(sfgpu_covg* g, uint64_t cap);
SFGPU_API int sfgpu_covg_project(sfgpu_covg* g, sfgpu_cov* finished, sfgpu_covg_result* out, sfgpu_stream stream);
SFGPU_API int sfgpu_covg_runs(sfgpu_covg* g, uint32_t* d_chrom, uint32_t* d_start, uint32_t* d_end, uint64_t* d_sum);
SFGPU_API int sfgpu_covg_write_text(sfgpu_covg* g, const char* d_chrom_names, const uint64_t* d_chrom_name_off, uint64_t chunk_bytes,
                                    sfgpu_text_sink sink, void* user, sfgpu_covg_result* out, sfgpu_stream stream);
SFGPU_API int sfgpu_covg_write_bgzf(sfgpu_covg* g, const char* d_chrom_names, const uint64_t* d_chrom_name_off, uint64_t chunk_bytes, sfgpu_bgzw* z,
                                    sfgpu_covg_result* out, sfgpu_stream stream);

/* A batch of hit records and their alignment slots rewritten from transcript into GENOME terms through the exon blocks, so that the
 * alignment writers above, opened over the chromosomes' names, write a genome-coordinate SAM / BAM with spliced CIGARs (the rule is
 * stated once in csrc/galnfmt.h; hits.project_alignments_host is the Python statement; csrc/genomealn.hip).  The writers are not told:
 * they take RNAME from tid, POS and CIGAR from the alignment group and count N in the reference span.
 *   open     the model sfgpu_covg_open takes, validated by the same rule with the same errors; the handle keeps a copy and the 64-bit
 *            prefix sums of the block lengths.
 *   project  batch: hits / hit_off[n_reads + 1] (the offsets start at 0 and never decrease, else SFGPU_ERR_INVALID; a tid that is no
 *            transcript of the model: SFGPU_ERR_RANGE naming the lowest record); aln_pos / aln_op_off / aln_ops: the transcript
 *            alignment (all three or none, SFGPU_ERR_INVALID otherwise; none: the writer's <clip>S<match>M); aln_nm: the slots' nm
 *            (optional; gathered); tag_nm / tag_md_off / tag_md: the NM / MD tags (all three or none).
 *            A lane per record sizes it: the start block by binary search of the prefix sums, the words walked, which gives the
 *            record's fate, each line's interval, its output words and MD bytes.  Three scans give the new record index (the new
 *            hit_off[r] is that index at the old hit_off[r]), the word offsets and the MD offsets.  A lane per slot of a kept record
 *            then writes the record (line 0's lane), the slot's position, nm and offsets, walks the words again to their places
 *            (back to front on a - transcript) and copies or reverses the MD.
 *            out: hits[n], hit_off[n_reads + 1], aln_pos[2 n], aln_nm[2 n], aln_op_off[2 n + 1], aln_ops[cap_ops], tag_nm[2 n],
 *            tag_md_off[2 n + 1], tag_md[cap_md], src_record[n], n = hit_off[n_reads] of the batch; the entries of the kept records
 *            are written (stats->records_out of them, two slots each, and one closing offset).  aln_nm may be NULL; the tag outputs
 *            are read only where the batch gives tags.  *n_ops / *n_md = the words / MD bytes needed; where they exceed cap_ops /
 *            cap_md: SFGPU_ERR_RANGE, both still set, nothing written.
 * Operations shorter than 2^28 bases.  Synchronous.  The stats are SET by the call. */
typedef struct sfgpu_galn sfgpu_galn;
typedef struct sfgpu_galn_batch {
    const struct sfgpu_hit* hits;
    const uint32_t* hit_off;         /* [n_reads + 1] */
    uint32_t n_reads;
    uint32_t pad_;
    const int32_t* aln_pos;          /* [2 records] */
    const uint64_t* aln_op_off;      /* [2 records + 1] */
    const uint32_t* aln_ops;
    const uint32_t* aln_nm;          /* [2 records] */
    const uint32_t* tag_nm;          /* [2 records] */
    const uint64_t* tag_md_off;      /* [2 records + 1] */
    const uint8_t* tag_md;
} sfgpu_galn_batch;
typedef struct sfgpu_galn_out {
    struct sfgpu_hit* hits;
    uint32_t* hit_off;
    int32_t* aln_pos;
    uint32_t* aln_nm;
    uint64_t* aln_op_off;
    uint32_t* aln_ops;
    uint64_t cap_ops;
    uint32_t* tag_nm;
    uint64_t* tag_md_off;
    uint8_t* tag_md;
    uint64_t cap_md;
    uint32_t* src_record;
} sfgpu_galn_out;
typedef struct sfgpu_galn_stats {
    uint64_t records_in, records_out;
    uint64_t records_unplaced;        /* the transcript is not placed, or has no block */
    uint64_t records_unalignable;     /* a line without a reference column */
    uint64_t records_off_range;       /* a line that starts below 0 on its transcript, leaves [0, 2^31 - 1] on the chromosome or needs an N of 2^28 or more */
    uint64_t reads_emptied;           /* reads that had records and keep none */
    uint64_t lines;                   /* of the kept records, as the following */
    uint64_t lines_spliced;           /* lines with an N */
    uint64_t n_operations;            /* N operations inserted */
    uint64_t lines_reversed;          /* lines of - transcripts */
    uint64_t columns_beyond_model;    /* reference columns at or beyond the blocks' total length */
    uint64_t words_in, words_out;
    double project_ms;                /* device events around the whole pass */
    double size_ms, scan_ms, emit_ms; /* ... by stage: the check and the size kernel; the three scans; the counts' way to the host, the reads and the emit kernel */
} sfgpu_galn_stats;
SFGPU_API int sfgpu_galn_open(sfgpu_galn** out, const uint8_t* d_status, const int32_t* d_chrom, const int8_t* d_strand, const uint64_t* d_exon_off,
                              const uint32_t* d_exon_start, const uint32_t* d_exon_len, uint64_t M, uint32_t n_chrom, sfgpu_stream stream);
SFGPU_API int sfgpu_galn_close(sfgpu_galn* g);
SFGPU_API int sfgpu_galn_project(sfgpu_galn* g, const sfgpu_galn_batch* batch, const sfgpu_galn_out* out, uint64_t* n_ops, uint64_t* n_md,
                                 sfgpu_galn_stats* stats, sfgpu_stream stream);

/* The samples the same loop collects when bias correction is on (one more pass over the hit records, for the
 * callers that need it): for every read, the 6-mer context of the FIRST hit that yields one (needBiasSample,
 * src/SailfishQuantify.cpp:270-287 / :559-581; ReadKmerDist<6>::update, include/ReadKmerDist.hpp:35-73), while
 * the budget sfOpts.numBiasSamples lasts -- "the first N successful reads in read order", what one mapping thread
 * does; and, in a paired library, the fragment-GC percentage of every properly paired hit (:375-389; no budget).
 * The reads and hits considered are those that survive the maxReadOccs / orphan cuts of sfgpu_filter_hits (same
 * opts).  Counters are ACCUMULATED into d_read_bias (4096 uint32) / d_observed_gc (101 uint32); either may be NULL.
 * d_gc_prefix: the per-transcript inclusive G/C counts laid out like d_seq (sfgpu_gc_prefix; 4 bytes per base),
 * required with d_observed_gc -- Transcript::GCCount_ for gcSampFactor 1 (include/Transcript.hpp:183-196).
 * Synchronous. */
typedef struct sfgpu_bias_sampler {
    const char* d_seq;                /* RapMapSAIndex::seq */
    const uint64_t* d_seq_off;        /* [M] txpOffsets */
    const uint32_t* d_ref_len;        /* [M] */
    uint32_t* d_read_bias;            /* [4096] ReadKmerDist<6>::counts, or NULL (biasCorrect off) */
    int64_t* remaining_bias_samples;  /* sfOpts.numBiasSamples (host), decremented */
    uint32_t* d_observed_gc;          /* [101] ReadExperiment::observedGC, or NULL (gcBiasCorrect off) */
    const uint32_t* d_gc_prefix;      /* see above */
    uint64_t n_bias_sampled, n_gc_sampled;   /* ACCUMULATED by the call */
    uint32_t gc_size_samp;            /* SailfishOpts::gcSampFactor: 0 or 1 = exact counts, > 1 = the reference's interpolation (bin clamped to [0,100]) */
    uint32_t pad_;
} sfgpu_bias_sampler;
SFGPU_API int sfgpu_gc_prefix(const char* d_seq, const uint64_t* d_seq_off, const uint32_t* d_ref_len, uint64_t M,
                      uint32_t* d_gc_prefix, sfgpu_stream stream);
SFGPU_API int sfgpu_sample_bias(const sfgpu_hit* d_hits, const uint32_t* d_hit_offsets, uint32_t n_reads,
                      const sfgpu_filter_opts* opts, sfgpu_bias_sampler* sampler, sfgpu_stream stream);

/* ---------------------------------------------------------------------------------------------
 * (next) Bias-aware effective lengths: sailfish::utils::updateEffectiveLengths
 * (src/SailfishUtils.cpp:611-926) -- the sequence-specific (--biasCorrect; 6-mer context model,
 * include/ReadKmerDist.hpp, include/UtilityFunctions.hpp:40-148) and fragment-GC (--gcBiasCorrect;
 * Transcript::gcFrac, include/Transcript.hpp:85-95) corrections -- and the optimize() variant that calls it
 * at iterations 50, 500 and 1000 (src/CollapsedEMOptimizer.cpp:814-840) and hands the corrected lengths back
 * (:888).  A handle holds what the function reads from ReadExperiment / SailfishOpts and is constant over the
 * run; sfgpu_bias_update is one call of updateEffectiveLengths.
 *   d_seq / d_seq_off : RapMapSAIndex::seq on the device and txpOffsets (Transcript::Sequence() =
 *                       seq + txpOffsets[i], include/ReadExperiment.hpp:115); bytes A C G T U in either case,
 *                       any other byte counts as 'A' in a k-mer (what nextKmerIndex does; a first k-mer
 *                       with such a byte is undefined behaviour in the reference)
 *   d_txp_eff_len     : Transcript::EffectiveLength as the FLD correction left it (:703, :821)
 *   h_fl_counts       : the vector ReadExperiment::setFragLengthDist received (counts of lengths
 *                       0..max_frag_len-1); the EmpiricalDistribution is rebuilt from it
 *   h_read_bias       : 4096 ReadKmerDist<6>::counts, pseudo-count included (may be NULL when !seq_bias)
 *   h_observed_gc     : 101 ReadExperiment::observedGC counts, pseudo-count included (may be NULL when !gc_bias)
 *   gc_speed_samp     : SailfishOpts::pdfSampFactor (--gcSpeedSamp)
 *   gc_size_samp      : SailfishOpts::gcSampFactor (--gcSizeSamp).  Above 1 the reference keeps the G/C count at every
 *                       gc_size_samp-th base only and interpolates (Transcript::gcCountInterp_, include/Transcript.hpp:
 *                       133-162, lambda on the LEFT sample as written); the same values are used here (slow path:
 *                       per-base table built for the duration of sfgpu_bias_create).  The interpolated difference
 *                       can leave [0, fragment length], where the reference indexes outside its 101 bins: the bin is
 *                       clamped to [0,100]
 * As in the reference, seq_bias and gc_bias together, or num_fwd + num_rc == 0, make every update a copy
 * of its input (status 2 / 1).  GC correction needs fld_low >= 1 (the reference divides by the fragment
 * length) and a 0.995 quantile below 16000 (SFGPU_ERR_RANGE).  Device memory: 808 bytes per transcript in
 * GC mode (the per-transcript GC-bin profile, built once at create), else O(1).
 * A handle carries the state of its last update (the expectation vectors): use one per optimize() that runs at a time.
 * Floating point: sums run in a different order than the reference's serial loops (and the 4096-bin
 * expectation is accumulated with atomics), so lengths agree to ~1e-12 relative, not bit for bit.
 * ------------------------------------------------------------------------------------------- */
typedef struct sfgpu_bias sfgpu_bias;
typedef struct sfgpu_bias_inputs {
    uint64_t M;
    const char* d_seq;
    const uint64_t* d_seq_off;      /* [M] */
    const uint32_t* d_ref_len;      /* [M] */
    const double* d_txp_eff_len;    /* [M] */
    const uint32_t* h_fl_counts;    /* [max_frag_len] */
    uint32_t max_frag_len;
    uint32_t gc_speed_samp;
    const uint32_t* h_read_bias;    /* [4096] */
    const uint32_t* h_observed_gc;  /* [101] */
    int64_t num_fwd, num_rc;        /* ReadExperiment::numFwd() / numRC() */
    int32_t seq_bias, gc_bias;      /* SailfishOpts::biasCorrect / gcBiasCorrect */
    uint32_t gc_size_samp;
    uint32_t pad_;
} sfgpu_bias_inputs;
typedef struct sfgpu_bias_stats {
    int32_t status;                 /* 0 recomputed, 1 no mappings (:625-630), 2 both models on (:633-638) */
    int32_t fld_low, fld_high;      /* the 0.005 / 0.995 quantiles of the FLD (:669-681), GC mode */
    int32_t pad_;
    uint64_t n_corrected, n_uncorrected;   /* numCorrected / numUncorrected (:806-807) of the last update */
} sfgpu_bias_stats;
SFGPU_API int sfgpu_bias_create(sfgpu_bias** out, const sfgpu_bias_inputs* in, sfgpu_stream stream);
SFGPU_API int sfgpu_bias_destroy(sfgpu_bias* b);
/* effLensOut = updateEffectiveLengths(sopt, readExp, effLensIn, alphas); d_eff_out may alias d_eff_in.
 * Asynchronous on `stream` when stats is NULL, else synchronises and fills *stats. */
SFGPU_API int sfgpu_bias_update(sfgpu_bias* b, const double* d_eff_in, const double* d_alpha, double* d_eff_out,
                      sfgpu_bias_stats* stats, sfgpu_stream stream);
/* ReadExperiment::expectedSeqBias() (4096) / expectedGCBias() (101) after the last update (the aux/
 * expected_bias, expected_gc files, src/GZipWriter.cpp:140-165); either pointer may be NULL.  Synchronous. */
SFGPU_API int sfgpu_bias_expected(sfgpu_bias* b, double* h_expected_seq, double* h_expected_gc);
/* CollapsedEMOptimizer::optimize with doBiasCorrect (:717): as sfgpu_em_optimize, plus the recompute hook
 * at iterations 50, 500, 1000 and d_eff_len_out [M] = the lengths to store back into
 * Transcript::EffectiveLength (:888; may be NULL).  n_recomputes (may be NULL) = hooks taken. */
SFGPU_API int sfgpu_em_optimize_bias(sfgpu_em* em, const sfgpu_em_opts* opts, sfgpu_bias* bias, double* d_alpha_out,
                      double* d_mass_out, double* d_eff_len_out, uint32_t* n_recomputes, sfgpu_em_stats* stats);

/* ---------------------------------------------------------------------------------------------
 * a13. quant.sf columns   src/GZipWriter.cpp:216-245
 *   TPM_t = ((estCount_t/numMapped)/len_t) / sum_u((estCount_u/numMapped)/len_u) * 1e6
 * d_len as in sfgpu_problem.  Asynchronous on `stream`.
 * ------------------------------------------------------------------------------------------- */
SFGPU_API int sfgpu_tpm(const double* d_est_count, const double* d_len, uint64_t M, double num_mapped,
              double* d_tpm, sfgpu_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* SFGPU_H */
