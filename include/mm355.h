/* mm355.h -- C-ABI of the MI355X-native mapping path (libmm355.so).
 *
 * Drop-in boundary for the ONE hot path of Adoni5/mappy-rs: the per-read minimap2
 * mapping call.  In the reference that call is `minimap2::Aligner::map` ->
 * `mm_map` of minimap2-sys (reference call sites /root/reference/src/lib.rs:482-488
 * for Aligner.map and :587-593 for the map_batch worker), surrounded by the
 * index/option FFI at lib.rs:333-416 and the sequence accessors at :716/:747.
 * Each entry point below names the reference FFI symbol it replaces.
 *
 * Plain pointers and sizes only; no torch / HIP types cross this boundary.
 * All functions return 0 on success or a negative MM355_E* code; mm355_strerror
 * gives the message.  The library refuses to run (MM355_ENODEV) when no gfx950
 * device is visible: there is no CPU fallback.
 */
#ifndef MM355_H
#define MM355_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MM355_OK        0
#define MM355_ENODEV   (-1)   /* no HIP device / kernel image not loadable */
#define MM355_EINVAL   (-2)
#define MM355_ENOMEM   (-3)
#define MM355_EIO      (-4)   /* cannot open / parse index or FASTA */
#define MM355_ENOIDX   (-5)   /* "No index" (L2 crate error string) */
#define MM355_EEMPTY   (-6)   /* "Sequence is empty" (L2 crate error string) */
#define MM355_EUNSUP   (-7)   /* option outside the long-read hot path (sr/splice presets, query-strand / heap-sort flags) */
#define MM355_EHIP     (-8)   /* a HIP runtime call failed */

typedef struct mm355_index mm355_index_t;     /* replaces mm_idx_t* (lib.rs:400-410) */
typedef struct mm355_ctx   mm355_ctx_t;       /* replaces mm_tbuf_t: one per host thread / GPU */

/* replaces mm_idxopt_t (lib.rs:332) */
typedef struct {
	int16_t k, w, flag, bucket_bits;
	int64_t mini_batch_size;
	uint64_t batch_size;
} mm355_idxopt_t;

/* replaces mm_mapopt_t (lib.rs:331); same field meaning as minimap2 2.26 */
typedef struct {
	int64_t flag;
	int32_t seed, sdust_thres, max_qlen;
	int32_t bw, bw_long, max_gap, max_gap_ref, max_frag_len;
	int32_t max_chain_skip, max_chain_iter, min_cnt, min_chain_score;
	float chain_gap_scale, chain_skip_scale;
	int32_t rmq_size_cap, rmq_inner_dist, rmq_rescue_size;
	float rmq_rescue_ratio, mask_level;
	int32_t mask_len;
	float pri_ratio;
	int32_t best_n;
	float alt_drop;
	int32_t a, b, q, e, q2, e2, sc_ambi;
	int32_t zdrop, zdrop_inv, end_bonus, min_dp_max, min_ksw_len;
	float max_clip_ratio;
	float mid_occ_frac, q_occ_frac;
	int32_t min_mid_occ, max_mid_occ, mid_occ, max_occ, max_max_occ, occ_dist;
	int64_t max_sw_mat;
} mm355_mapopt_t;

/* one alignment; mirrors mappy_rs::Mapping (lib.rs:109-154) filled from mm_reg1_t */
typedef struct {
	int32_t query_start, query_end;
	int32_t strand;                 /* +1 forward, -1 reverse */
	int32_t rid;                    /* index into mm355_index_info names */
	int32_t target_len, target_start, target_end;
	int32_t match_len, block_len;
	uint32_t mapq;
	int32_t is_primary;
	int32_t NM;
	int32_t n_cigar;
	int64_t cigar_off;              /* into mm355_hits_t::cigar, u32 = len<<4|op */
	int64_t cs_off, cs_len;         /* into mm355_hits_t::str; cs_len < 0 => None */
	int64_t md_off, md_len;
	int32_t score0, dp_max, dp_max2, dp_score, cnt, n_sub, subsc, reserved;
} mm355_hit_t;

/* what minimap2's PAF writer prints besides the columns, per hit (MM355_OUT_TAGS): the fields of mm_reg1_t / mm_extra_t behind
 * s1 / dv / de / rl / zd and the tp letter (cm, s2, ms, AS, nn come from mm355_hit_t: cnt, subsc, dp_max, dp_score, n_ambi below) */
#define MM355_TAG_INV      1u       /* flags bit 0: r->inv (an inversion record, tp:A:I / i) */
#define MM355_TAG_SAM_PRI  2u       /* flags bit 1: r->sam_pri (a primary without it is supplementary) */
#define MM355_TAG_SPLIT_SHIFT 2     /* flags bits 2-3: r->split (zd) */
typedef struct {
	int32_t score;                  /* r->score (s1; differs from score0 on split regions) */
	float div;                      /* r->div as mm_est_err left it; -1 = not estimated */
	int32_t rep_len;                /* of the read, repeated on each of its hits (rl) */
	int32_t n_ambi;
	int32_t n_gap, n_gapo;          /* summed lengths / number of the I and D operations of the final CIGAR; 0 without a CIGAR */
	uint32_t flags;
	int32_t reserved;
} mm355_tags_t;

/* result of one batch; owned by the library until mm355_free_hits */
typedef struct {
	int64_t n_reads;
	int64_t *hit_off;               /* n_reads+1 offsets into hits[] */
	int32_t *status;                /* per read: 0 ok, MM355_EEMPTY for an empty sequence */
	mm355_hit_t *hits;
	uint32_t *cigar;
	char *str;
	int64_t n_hits, n_cigar, n_str;
	mm355_tags_t *tags;             /* parallel to hits[]; NULL unless MM355_OUT_TAGS was asked for */
} mm355_hits_t;

/* --- options: replaces mm_set_opt (lib.rs:333,336) and mm_mapopt_update (lib.rs:414) --- */
int mm355_set_opt(const char *preset, mm355_idxopt_t *io, mm355_mapopt_t *mo);
int mm355_mapopt_update(mm355_mapopt_t *mo, const mm355_index_t *idx);

/* --- index: replaces mm_idx_reader_open/read/close + mm_idx_index_name (lib.rs:397-416) --- */
int mm355_index_load(const char *path, const mm355_idxopt_t *io, int n_threads, mm355_index_t **out);
int mm355_index_build(const mm355_idxopt_t *io, int n_seq, const char *const *seqs, const int64_t *lens,
                      const char *const *names, int n_threads, mm355_index_t **out);
/* same index, built on GPU `device` (sketch + radix sort + table fill in HBM; replaces the FASTA branch of
 * mm_idx_reader_read for large references).  The table stays resident on that device; other devices get peer copies (mm355_upload). */
int mm355_index_build_device(const mm355_idxopt_t *io, int n_seq, const uint8_t *const *seqs, const int64_t *lens,
                             const char *const *names, int device, mm355_index_t **out);
/* a FASTA / FASTQ path (plain or gzip: the reader of mm355_index_load) indexed on GPU `device` through mm355_index_build_device; a path
 * whose magic is MMI\2 is loaded as mm355_index_load loads it (a host image: there is nothing to build).  Same error codes as
 * mm355_index_load, plus MM355_ENODEV. */
int mm355_index_load_device(const char *path, const mm355_idxopt_t *io, int device, mm355_index_t **out);
/* an MMI\2 file loaded into the HBM of `device`: the result is device-resident exactly like an index from mm355_index_build_device
 * (table and pos[] only in HBM; the host keeps header, names and the 4-bit sequence image).  The host reads the bucket headers, the bucket
 * sections cross in pieces of 32 MB (MM355_IDXLOAD_PIECE=<bytes>) and are scattered into the table and pos[] on the device; no host table
 * is ever made.  Not an MMI\2 file: MM355_EINVAL (nothing is built: use mm355_index_load_device).  Unreadable, truncated or inconsistent
 * file: MM355_EIO.  MM355_ENODEV / ENOMEM / EHIP / EUNSUP (2^32 or more positions) as mm355_index_build_device.  Only the first part of a
 * multi-part file is read, as by mm355_index_load. */
int mm355_index_load_mmi_device(const char *path, int device, mm355_index_t **out);
/* writes the index as a minimap2 MMI\2 file: replaces mm_idx_dump, the reference's fn_idx_out (lib.rs:391-394).  Any index: loaded from
 * .mmi, built on the host, or built on a device (its table is converted in HBM and copied out in fixed-size pieces).  The file is the one
 * U:index.c::mm_idx_load reads:
 *   magic; w k b n_seq flag (5 x u32); per contig u8 name length, name, u32 length; for each of the 1<<b buckets i32 n, n position words,
 *   u32 size, size (key, value) pairs; unless flag & 2 (MM_I_NO_SEQ) the 4-bit sequence image, (sum_len+7)/8 words.
 *   bucket = minimizer & ((1<<b)-1); key = minimizer>>b<<1, | 1 for a singleton; value = the position word of a singleton, else
 *   start<<32 | count with start relative to the bucket's own p[].
 * minimap2 lists a bucket's pairs in khash slot order, which no loader depends on (they re-insert).  This writer's order is CANONICAL, so
 * that the file is a pure function of the index: within a bucket the pairs have ascending keys, and p[] holds the runs of the
 * multi-occurrence keys in that same order, each run ascending -- the p[] layout of U:index.c::worker_post, so the p[] sections and every
 * value equal minimap2's own dump.
 * MM355_ENOIDX for NULL; MM355_EINVAL when a contig name is longer than 255 bytes (the length field is one byte; checked before the file
 * is opened); MM355_EIO when the file cannot be created or written (a partly written file is removed); MM355_ENOMEM / MM355_EHIP from
 * the device conversion.  The index is unchanged. */
int mm355_index_dump(const mm355_index_t *idx, const char *path);
void mm355_index_free(mm355_index_t *idx);
/* header fields read at lib.rs:655-670 (k, w, n_seq) */
int mm355_index_info(const mm355_index_t *idx, int32_t *k, int32_t *w, int32_t *b, int32_t *flag, uint32_t *n_seq);
const char *mm355_index_seq_name(const mm355_index_t *idx, uint32_t rid);   /* lib.rs:447-455 */
int64_t mm355_index_seq_len(const mm355_index_t *idx, uint32_t rid);
int mm355_index_name2id(const mm355_index_t *idx, const char *name);        /* mm_idx_name2id, lib.rs:716 */
int mm355_index_getseq(const mm355_index_t *idx, uint32_t rid, uint32_t st, uint32_t en, uint8_t *seq); /* mm_idx_getseq, lib.rs:747 */
/* host-side diagnostic equivalent of mm_idx_get(): occurrences of one minimizer (returns the count) */
int mm355_index_get(const mm355_index_t *idx, uint64_t minier, uint64_t *vals, int cap);
int mm355_index_stat(const mm355_index_t *idx, int64_t *n_minimizers, int64_t *n_distinct, int64_t *table_bytes, int64_t *pos_bytes);

/* --- multi-GPU: the reference shares ONE read-only mm_idx_t between its N worker threads (lib.rs:541-546, `self.aligner.clone()`
 * per thread); the GPU analogue is one replica of the index in the HBM of every device, shared by all contexts of that device.
 * mm355_upload replicates the index to the listed devices (H2D from the host image; a device-built index is copied device-to-device);
 * idempotent.  mm355_ctx_create replicates lazily when its device has no replica yet.  No collective is involved. --- */
int mm355_upload(mm355_index_t *idx, const int *device_ids, int n);

/* --- device context (one per host thread / GPU): replaces mm_tbuf_init/destroy --- */
int mm355_ctx_create(const mm355_index_t *idx, int device_id, mm355_ctx_t **out);   /* uses (or creates) the replica of device_id */
void mm355_ctx_destroy(mm355_ctx_t *ctx);

/* --- the hot path: replaces mm_map (+ mm_gen_cs / mm_gen_MD) for a whole batch of reads.
 * seqs[i] need not be NUL-terminated.  flags: bit0 = cs (short form), bit1 = MD, bit2 = tags (mm355_hits_t::tags; legal in both modes),
 * bit3 = cs in the long form (alone or together with bit0: the long form).
 * cs, short form (minimap2 --cs, format.c::write_cs_core with no_iden): inside a match operation (CIGAR op 0, 7, 8) a maximal run of columns
 * with equal codes prints ':' and its length, a mismatch '*' + target + query in lower case; an insertion '+' and its query bases, a deletion
 * '-' and its target bases, lower case.  A run ends at a mismatch and at the end of its CIGAR operation.
 * cs, long form (minimap2 --cs=long, no_iden == 0): the same, except that a run prints '=' followed by its query bases in upper case from
 * "ACGTN" (code 4 against code 4 is equal and prints 'N').  Runs end where they end in the short form, so two adjacent match operations
 * ("5=" then "3=") print two '='.  The '+' / '-' text, mlen, blen, n_ambi, dp_max, the gap counts and MD are those of the short form.
 * Without MM_F_CIGAR in mo->flag the call maps chain-only (minimap2 without -c): seeds, chains, regions, MAPQ from the chains, no extension.
 * Its hits have n_cigar = 0, cs_len = md_len = -1, NM = dp_max = dp_max2 = dp_score = 0; cs / MD flags are MM355_EINVAL; an index without
 * sequence (MM_I_NO_SEQ) is mappable.  The region logic runs on the device (k_regs); MM355_REGS_HOST=1 runs it on the host for every read. --- */
#define MM355_OUT_CS 1
#define MM355_OUT_MD 2
#define MM355_OUT_TAGS 4
#define MM355_OUT_CS_LONG 8   /* every map call that takes MM355_OUT_CS takes it; chain-only calls refuse it alike */
int mm355_map_batch(mm355_ctx_t *ctx, const mm355_mapopt_t *mo, int64_t n_reads, const char *const *seqs,
                    const int32_t *lens, int flags, mm355_hits_t **out);
/* the same call split in two, for callers that keep a batch resident in HBM (bench.py times mm355_map_resident):
 * mm355_map_batch == mm355_batch_upload + mm355_map_resident */
int mm355_batch_upload(mm355_ctx_t *ctx, int64_t n_reads, const char *const *seqs, const int32_t *lens);
/* several resident batches per context: make batch `slot` (0..63) the current one; upload / map_resident act on the current batch */
int mm355_batch_select(mm355_ctx_t *ctx, int slot);
int mm355_map_resident(mm355_ctx_t *ctx, const mm355_mapopt_t *mo, int flags, mm355_hits_t **out);
/* The same calls with query names (minimap2's mm_map(..., qname); mappy's map(seq, name=...)).  names[i] is NUL-terminated; names == NULL
 * or names[i] == NULL: that read has no name and maps exactly as through the calls above.  A name does two things:
 *   - it enters the read hash that orders regions of equal score (X31 of the name, unless MM_F_NO_HASH_NAME 0x400000000 is set);
 *   - with MM_F_NO_DIAG (0x1) / MM_F_NO_DUAL (0x2), which the ava-ont / ava-pb presets set, seeds are filtered by the contig's name
 *     (U:map.c::skip_seed): NO_DIAG drops the diagonal of a read against its own copy (equal name and equal length), NO_DUAL drops every
 *     contig whose name sorts before the read's (strcmp order), so that an all-vs-all run reports each pair once.  On an index without
 *     names (MM_I_NO_NAME) only the hash applies.
 * A batch uploaded with names keeps them while it is resident: mm355_map_resident uses them. */
int mm355_map_batch_named(mm355_ctx_t *ctx, const mm355_mapopt_t *mo, int64_t n_reads, const char *const *seqs,
                          const int32_t *lens, const char *const *names, int flags, mm355_hits_t **out);
int mm355_batch_upload_named(mm355_ctx_t *ctx, int64_t n_reads, const char *const *seqs, const int32_t *lens, const char *const *names);
void mm355_free_hits(mm355_hits_t *hits);

/* --- PAF text: replaces the caller's own formatting loop over the hit records (one mappy_rs.paf_line per hit: minimap2's
 * format.c::mm_write_paf + write_tags).  One line per row of hits[], in row order, each ending in '\n': the twelve columns; with a CIGAR
 * NM ms AS nn; tp cm s1, and s2 on primaries; de with a CIGAR, otherwise dv when 0 <= div <= 1 ("0" when exactly zero, else C's %.4f of
 * the double); zd when the split bits are set; rl; with a CIGAR cg:Z:, then cs:Z: / MD:Z: when cs_len / md_len >= 0.  The query name is
 * the read's name up to its first space or tab; a read without a name prints "*" (minimap2 has no unnamed reads in a file).  A read
 * without hits, or with status MM355_EEMPTY, writes nothing.  The text is produced on the device (mm355_paf.hip: a length kernel, a scan,
 * a write kernel; query and contig names reach the GPU for this writer only) or on the host (mm355_paf.h, the same emitter run serially). */
typedef struct {
	int64_t n_reads, n_lines, n_text;
	int64_t *line_off;              /* n_reads+1; lines of read i = text[line_off[i] .. line_off[i+1]) */
	char *text;                     /* n_text bytes (and a NUL behind them) */
	double ms_format;               /* wall time of the formatting step: uploads, kernels and the copy back, or the host loops */
	int32_t on_device, reserved;    /* 1: the device formatter wrote the text */
} mm355_text_t;
#define MM355_PAF_AUTO 0            /* host below a hit count (128 with a CIGAR, 1024 chain-only: measured, see README; MM355_PAF_MIN_HITS=<n> overrides), device from there on */
#define MM355_PAF_HOST 1
#define MM355_PAF_DEVICE 2
/* formats an existing batch result; hits->tags must be there (MM355_EINVAL otherwise, as for a row that points outside its arena, names
 * no contig or, with a CIGAR, has block_len + n_ambi - n_gap + n_gapo == 0: de would divide by zero).  The %.4f of dv / de is exact for
 * magnitudes below 2^50, which these fields cannot reach; beyond that the text is "inf", unlike printf.
 * mo tells CIGAR mode from chain-only; qnames == NULL or qnames[i] == NULL: an unnamed read; qlens[i]: the read's length */
int mm355_paf_format(mm355_ctx_t *ctx, const mm355_mapopt_t *mo, const mm355_hits_t *hits, const char *const *qnames,
                     const int32_t *qlens, int where, mm355_text_t **out);
/* == mm355_map_batch_named with flags | MM355_OUT_TAGS, then mm355_paf_format, then mm355_free_hits: byte for byte */
int mm355_map_batch_paf(mm355_ctx_t *ctx, const mm355_mapopt_t *mo, int64_t n_reads, const char *const *seqs, const int32_t *lens,
                        const char *const *names, int flags, int where, mm355_text_t **out);
void mm355_free_text(mm355_text_t *t);

/* --- SAM text: minimap2 -a without a header (format.c::mm_write_sam3, write_sam_cigar, sam_write_sq, write_tags of 2.26), one line per row
 * of hits[] in row order, and one unmapped record for a read without rows.  Needs MM_F_CIGAR in mo->flag and hits->tags.  With qlen the
 * read's length, qs / qe / rev (strand < 0) of the row, tab-separated, each line ending in '\n':
 *   QNAME  the read's name up to its first space or tab; "*" for an unnamed read
 *   FLAG   0x10 if rev; 0x100 if !is_primary, otherwise 0x800 if the tags row lacks MM355_TAG_SAM_PRI
 *   RNAME, POS = target_start + 1, MAPQ (unsigned)
 *   CIGAR  clip5 = rev ? qlen - qe : qs, clip3 = rev ? qs : qlen - qe, each printed when non-zero around the CIGAR words, with the letter H
 *          when FLAG & 0x800 and soft clipping is off, otherwise S (a secondary too); "*" for a row with n_cigar == 0; no long-CIGAR handling
 *   RNEXT PNEXT TLEN   "*", 0, 0
 *   SEQ QUAL   FLAG & 0x900 == 0 or soft clipping on: the whole read, reversed and complemented if rev, and the whole quality, reversed if
 *          rev ("*" without one); otherwise a secondary: "*", "*"; otherwise (supplementary, hard-clipped) read[qs:qe] and qual[qs:qe]
 *          treated the same way.  Complement: bytes below 128, case kept, A<->T C<->G R<->Y K<->M B<->V D<->H, U->A, everything else
 *          unchanged.  The bytes are the caller's; nothing is upper-cased.
 *   tags   NM ms AS nn tp cm s1, s2 on primaries, de, zd when split (the block PAF prints); SA:Z: on a row with is_primary when the read has
 *          another row q with is_primary and n_cigar > 0: for each such q in row order "rname,pos,strand,cigar,mapq,nm;" with pos =
 *          q.target_start + 1, strand + or -, cigar = clip5 S, l_M M, l_I I, l_D D, clip3 S (zero parts left out; if qe - qs < te - ts then
 *          l_M = qe - qs, l_D = te - ts - l_M, else l_M = te - ts, l_I = qe - qs - l_M), nm = block_len - match_len + n_ambi; cs:Z: / MD:Z:
 *          when the row has them; rl:i: (the tags row's rep_len) last.
 * A read without rows (status 0, qlen > 0) writes "QNAME 4 * 0 0 * * 0 0 SEQ QUAL rl:i:<rep_len[i]>", SEQ and QUAL as given, unless
 * MM355_SAM_HIT_ONLY is set.  A read with status MM355_EEMPTY writes nothing.  n_lines counts the lines; line_off delimits a read's lines.
 * The text is formed on the device (mm355_sam.hip: a length kernel and a scan, a kernel for the short fields and the CIGAR, a tiled copy
 * kernel for SEQ and QUAL; reads and qualities are uploaded for this writer) or on the host (mm355_sam.h, the same emitter run serially).
 * MM355_EINVAL, before anything is allocated or launched: whatever the PAF formatter refuses; an option record without MM_F_CIGAR; a row
 * outside 0 <= qs <= qe <= qlen; rows on an MM355_EEMPTY read; seqs[i] == NULL where qlens[i] > 0; unknown sam_flags bits; rep_len == NULL
 * when an unmapped record would print it.  `where` as for the PAF formatter; AUTO picks the host below 48 hits (measured, see
 * README; MM355_SAM_MIN_HITS=<n> overrides it, read per call). */
#define MM355_SAM_SOFTCLIP 1        /* minimap2 -Y */
#define MM355_SAM_HIT_ONLY 2        /* minimap2 --sam-hit-only */
/* quals == NULL or quals[i] == NULL: no quality ("*"), otherwise qlens[i] bytes; rep_len[i] is read only for reads without rows */
int mm355_sam_format(mm355_ctx_t *ctx, const mm355_mapopt_t *mo, const mm355_hits_t *hits, const char *const *qnames, const char *const *seqs,
                     const int32_t *qlens, const char *const *quals, const int32_t *rep_len, int sam_flags, int where, mm355_text_t **out);
/* == mm355_map_batch_named with flags | MM355_OUT_TAGS, then mm355_sam_format with the call's per-read rep_len, then mm355_free_hits: byte
 * for byte.  flags: MM355_OUT_CS | MM355_OUT_MD | MM355_OUT_CS_LONG */
int mm355_map_batch_sam(mm355_ctx_t *ctx, const mm355_mapopt_t *mo, int64_t n_reads, const char *const *seqs, const int32_t *lens,
                        const char *const *names, const char *const *quals, int flags, int sam_flags, int where, mm355_text_t **out);

/* --- BAM records: uncompressed BAM, that is BGZF with stored deflate blocks (what `samtools view -u` writes and every htslib tool reads).
 * The rule: a record is the BAM encoding of the SAM line mm355_sam_format writes for the same row under the same sam_flags -- the SAM/BAM
 * specification's encoding, with htslib's choices where the specification leaves one.  Little-endian, field by field:
 *   block_size   the length of the rest of the record
 *   refID = rid, pos = target_start, l_read_name = printed name length + 1, mapq (one byte),
 *   bin = reg2bin(pos, pos + max(1, reflen)) & 0xffff, reflen = the summed lengths of the row's M D N = X words, in 64 bits,
 *   n_cigar_op, flag (the SAM line's), l_seq, next_refID = -1, next_pos = -1, tlen = 0, read_name and a NUL
 *   CIGAR  clip5 (H or S by the SAM line's rule), the row's words unchanged (len << 4 | op is BAM's word), clip3; a row with n_cigar == 0 has
 *          no words.  More than 65535 words: htslib's long-CIGAR form -- n_cigar_op = 2, the words (uint32)l_seq << 4 | S and
 *          (uint32)reflen << 4 | N, and the real words in a CG:B:I tag, the record's last
 *   SEQ    what the SAM line prints as SEQ (l_seq = 0 and no bytes where it prints "*": a secondary without soft clipping), two bases per
 *          byte, high nibble first, a final odd base padded with 0; code = index in "=ACMGRSVTWYHKDBN" in either case, every other byte (U
 *          and u among them) 15.  On the reverse strand the byte is complemented first, as the line's is: U -> A -> 1
 *   QUAL   l_seq bytes: the quality byte minus 33 mod 256, last byte first on the reverse strand; 0xFF each for a read without quality
 *   tags   in the SAM line's order: NM ms AS nn tp cm s1 [s2] de [zd] [SA] [cs] [MD] rl [CG], copied tags (mm355_bam_format_aux) between rl
 *          and CG.  An i tag takes htslib's smallest type: C up to 255, S up to 65535, else I; c down to -128, s down to -32768, else i.
 *          tp is A.  de is f: the float32 of the double N / 10000.0, N
 *          the integer behind the line's %.4f digits (0 for the printed "0", the sign kept) -- (float)strtod(text) without the text.  SA, cs
 *          and MD are Z with a NUL, SA's text the SAM line's
 * The unmapped record: refID -1, pos -1, mapq 0, bin 4680, flag 4, no CIGAR, SEQ and QUAL as given, rl.
 * One thing the text cannot say and the record can: a SEQ or QUAL of one byte that is `*` (a one-base read or hard-clipped slice) prints the
 * SAM marker of a missing field; the record holds what the read holds (l_seq 1, code 15; quality 9).
 * MM355_EINVAL, before anything is allocated or launched (the library's check is mm355_bam.h::mm355_bam_check): whatever the SAM formatter
 * refuses; a row with mapq > 255; a printed read name of more than 254 bytes on a read that writes a record; a clip of 2^28 bases or more
 * (a word's length has 28 bits).
 * BGZF: the stream of records is cut every 0xff00 bytes (htslib's block payload; records may straddle blocks).  A block is the 18-byte gzip
 * header with the BC extra field and BSIZE, one stored deflate block (01, LEN, NLEN), the payload, CRC-32 and ISIZE: payload + 31 bytes, so
 * block b starts at b * (0xff00 + 31).  One call's output is a whole number of blocks, and the outputs of consecutive calls, one behind
 * the other, are a valid stream of records; the header blocks and the empty 28-byte EOF block are the file writer's, once per file.
 * In the result `text` is the BGZF bytes, n_lines the number of records, and line_off[i] the offset of read i's first record IN THE UNFRAMED
 * STREAM of records (byte x of it is byte x + 23 + 31 * (x / 0xff00) of text).  Formed on the device (mm355_bam.hip: a length kernel and two
 * scans, a kernel for the fields, a tiled kernel that packs SEQ and QUAL, a framing kernel with a workgroup per block) or on the host
 * (mm355_bam.h: the same emitter run serially, zlib's crc32).  `where` as for the PAF formatter; AUTO picks the host below 24 hits
 * (measured, see README; MM355_BAM_MIN_HITS=<n> overrides it, read per call). */
int mm355_bam_format(mm355_ctx_t *ctx, const mm355_mapopt_t *mo, const mm355_hits_t *hits, const char *const *qnames, const char *const *seqs,
                     const int32_t *qlens, const char *const *quals, const int32_t *rep_len, int sam_flags, int where, mm355_text_t **out);
/* == mm355_map_batch_named with flags | MM355_OUT_TAGS, then mm355_bam_format with the call's per-read rep_len, then mm355_free_hits: byte
 * for byte.  flags: MM355_OUT_CS | MM355_OUT_MD | MM355_OUT_CS_LONG */
int mm355_map_batch_bam(mm355_ctx_t *ctx, const mm355_mapopt_t *mo, int64_t n_reads, const char *const *seqs, const int32_t *lens,
                        const char *const *names, const char *const *quals, int flags, int sam_flags, int where, mm355_text_t **out);
/* the framing stage by itself: n arbitrary bytes into stored BGZF blocks (n == 0: zero bytes), on the host (ctx may be NULL) or on the
 * device (an upload, the framing kernel, a copy back); AUTO is the host: the bytes are in host memory, and either transfer moves as much
 * as the host's crc32 reads.  n_lines counts the blocks, n_reads is 0.  The BAM header of a file goes through here. */
int mm355_bgzf_wrap(mm355_ctx_t *ctx, const void *data, int64_t n, int where, mm355_text_t **out);

/* --- compressed BAM: the three calls above with `int level` -- 0: the stored blocks, byte for byte what the call without it writes (which is
 * this one at level 0); 1: every BGZF payload as one dynamic-Huffman deflate block (RFC 1951: LZ77 matches inside the payload, one code set per
 * payload), or stored as at level 0 where that would not be shorter, so that no block is longer than at level 0 and BSIZE always fits; any
 * other level: MM355_EINVAL, before anything is allocated, mapped or launched.  The gzip header, CRC-32 and ISIZE are level 0's; BSIZE is the
 * block's real size.  What `samtools view -b` writes and htslib reads.  The coder is stated once (mm355_deflate.h) and runs as a kernel with
 * a workgroup per payload (mm355_bam.hip: k_bgzf_deflate, a scan of the block sizes, k_bgzf_compact) or serially on the host: the same bytes,
 * and the same bytes from call to call.  `text` is the blocks, n_lines the records (the blocks for mm355_bgzf_deflate), and line_off still
 * points into the UNFRAMED stream: the arithmetic block-offset formula above holds at level 0 only -- at level 1 walk the blocks by BSIZE.
 * `where` as for the level-0 calls, with the same thresholds.  MM355_BAM_TIMES=1: a level-1 call on the device prints a line of its own on
 * stderr (the kernels' time between two events, bytes in and out, stored blocks). */
int mm355_bam_format_deflate(mm355_ctx_t *ctx, const mm355_mapopt_t *mo, const mm355_hits_t *hits, const char *const *qnames, const char *const *seqs,
                             const int32_t *qlens, const char *const *quals, const int32_t *rep_len, int sam_flags, int where, int level, mm355_text_t **out);
int mm355_map_batch_bam_deflate(mm355_ctx_t *ctx, const mm355_mapopt_t *mo, int64_t n_reads, const char *const *seqs, const int32_t *lens,
                                const char *const *names, const char *const *quals, int flags, int sam_flags, int where, int level, mm355_text_t **out);
int mm355_bgzf_deflate(mm355_ctx_t *ctx, const void *data, int64_t n, int where, int level, mm355_text_t **out);

/* --- copied aux tags: the calls above with the tags a read brought along (MM / ML of a basecaller's BAM, RG, qs, ...), which the record
 * carries through.  aux == NULL: the calls above, byte for byte (they are these with aux == NULL; aux_len and aux_mod are not read).
 * Otherwise per read: aux[i] points to aux_len[i] bytes of BAM aux tags in the two groups mm355_bam_aux_split makes, the second -- the tags
 * that index the bases of the read as sequenced, MM ML MN Mm Ml -- beginning at aux_mod[i]; aux[i] == NULL or aux_len[i] == 0: none.
 * The rule, field by field behind the record's own tags: ... rl [copied tags] [CG], so CG stays the record's last, and
 *   aux[i][0 .. aux_len[i])   on a record whose SEQ is the whole read: a row with FLAG & 0x900 == 0, every row under MM355_SAM_SOFTCLIP, and
 *                             the unmapped record
 *   aux[i][0 .. aux_mod[i])   on every other record: a hard-clipped supplementary (its SEQ is a slice: MM / ML would count bases that are
 *                             not there) and a secondary with SEQ `*`
 * The bytes are copied as given (mm355_bam.hip: a third bulk run of k_bam_bulk, 16-byte pieces from shifted source dwords; on the host a
 * memcpy): their well-formedness is mm355_bam_aux_split's job -- the reader always runs it, the Python surface runs it on a caller's bytes.
 * A record must not hold a tag twice, which is why the split drops the tags the writer emits itself.  The SAM specification gives tag order
 * no meaning.  SAM and PAF text do not print copied tags: mm355_sam_format and mm355_paf_format have no such argument (a follow-up, as
 * bgzip-compressed text is).  `level` as for the _deflate calls.
 * MM355_EINVAL, before anything is allocated or launched, besides what mm355_bam_format refuses: aux != NULL with aux_len or aux_mod NULL;
 * a negative aux_len[i]; aux[i] == NULL with aux_len[i] > 0; aux_mod[i] outside [0, aux_len[i]]; a record that would be longer than
 * 2^32 + 3 bytes (block_size has 32 bits). */
int mm355_bam_format_aux(mm355_ctx_t *ctx, const mm355_mapopt_t *mo, const mm355_hits_t *hits, const char *const *qnames, const char *const *seqs,
                         const int32_t *qlens, const char *const *quals, const int32_t *rep_len, const uint8_t *const *aux, const int32_t *aux_len,
                         const int32_t *aux_mod, int sam_flags, int where, int level, mm355_text_t **out);
int mm355_map_batch_bam_aux(mm355_ctx_t *ctx, const mm355_mapopt_t *mo, int64_t n_reads, const char *const *seqs, const int32_t *lens,
                            const char *const *names, const char *const *quals, const uint8_t *const *aux, const int32_t *aux_len, const int32_t *aux_mod,
                            int flags, int sam_flags, int where, int level, mm355_text_t **out);
/* One bounded walk over a BAM aux block of n bytes (mm355_bamaux.h) and the split the calls above take.  A tag is two name bytes, a type
 * and a value: A c C one byte, s S two, i I f four, d eight, Z H up to a NUL inside the block, B a subtype out of cCsSiIf, a uint32 count
 * and count x size bytes inside the block (the product in 64 bits).  `keep` is "*" for every tag or two-letter names back to back
 * ("MMMLMN").  `out` (n bytes) receives the kept tags in two groups, each in input order: first every kept tag but MM ML MN Mm Ml, then,
 * from *mod_off, those; *n_out: the bytes written.  Always dropped, because the writer emits them itself: NM ms AS nn tp cm s1 s2 de dv
 * zd SA cs MD rl CG.  The block is untrusted input.  MM355_EINVAL: an unknown type or subtype, a value or NUL past the end, a trailing
 * partial tag, n < 0, a `keep` that is NULL, empty or of odd length (but "*"). */
int mm355_bam_aux_split(const uint8_t *aux, int32_t n, const char *keep, uint8_t *out, int32_t *n_out, int32_t *mod_off);

/* --- coordinate-sorted BAM: the records of a call in samtools' coordinate order, as a RUN a file writer merges with others.  The key of a
 * record (mm355_bamsort.h::bam_sort_key; refID, pos and flag are the record's own little-endian fields):
 *   (uint64)(uint32)refID << 32 | (uint32)(pos + 1) << 1 | (flag >> 4 & 1)
 * -- contigs in header order; inside a contig by position; at one position forward before reverse; records without a contig (refID -1; the
 * unmapped record has pos -1, so its low word is 0) last.  TIES KEEP INPUT ORDER: a run is the stable sort of its input, so the stable merge
 * of the runs of a file's calls, taken in call order, is the stable sort of the file the unsorted calls write, however the reads were cut
 * into calls.  `rec` is the records in key order, back to back and UNFRAMED (mm355_bgzf_deflate frames a stream of them), rec_off their
 * n_rec + 1 offsets, key their keys, ascending; ms_sort the sort step alone (keys, sort, permutation; on the device between two events);
 * on_device: 1 when the device sorted.
 * mm355_bam_sort is the stage by itself: n_rec records in the n_bytes at rec (host memory), record i at rec_off[i] .. rec_off[i + 1].
 * `where`: MM355_PAF_HOST (ctx may be NULL: keys, std::stable_sort of indices, memcpy), MM355_PAF_DEVICE (an upload; mm355_bam.hip: k_rec_key
 * a thread per record, rocPRIM's radix sort of (key, index) pairs, which is stable, a gather and two scans for the new offsets and tiles,
 * k_rec_permute a block per 4096 output bytes of a record with aligned 16-byte stores from shifted source dwords; a copy back), or
 * MM355_PAF_AUTO, which is the host as for mm355_bgzf_wrap.  n_rec == 0 (and n_bytes == 0) gives an empty run.
 * MM355_EINVAL, before anything is allocated or launched: offsets that do not ascend from 0 to n_bytes, a piece of fewer than 37 bytes
 * (block_size, the 32 fixed bytes, a one-byte name), a piece whose block_size + 4 is not its length, more than 2^31 - 1 records, an
 * unknown `where`, MM355_PAF_DEVICE without a context.
 * mm355_map_batch_bam_run is mm355_map_batch_bam_aux up to the finished records (aux == NULL allowed), then the sort where the records
 * were formed -- `where` and its threshold are the formatter's: on the device the records never leave HBM before they are sorted -- and
 * one copy of rec, key and rec_off to the host.  Nothing is framed.  It refuses what mm355_map_batch_bam_aux refuses.
 * mm355_bam_gather is the copy loop of the merge: piece i is len[i] bytes at base + src_off[i]; the pieces go back to back into out.
 * MM355_EINVAL before a byte is copied: a negative offset or length, a piece that passes base_len, a total that passes out_cap.
 * MM355_BAM_TIMES=1: a sorted call on the device prints a line of its own on stderr (records, bytes, the sort step between two events). */
typedef struct {
	int64_t n_rec, n_bytes;
	uint64_t *key;                  /* n_rec, ascending */
	int64_t *rec_off;               /* n_rec + 1 offsets into rec */
	char *rec;                      /* the records, sorted, UNFRAMED */
	double ms_sort;                 /* the sort step alone */
	int32_t on_device, packed;      /* packed: 1 only from mm355_map_batch_bam_run_packed (below): rec holds BGZF members */
	int64_t *span;                  /* n_rec spans in the order of rec, or NULL: only the _span calls below fill it */
	int64_t n_blk;                  /* a packed run: the BGZF members in rec; otherwise 0 */
	int64_t *blk_off;               /* a packed run: n_blk + 1 offsets of the members inside rec; otherwise NULL */
} mm355_run_t;
int mm355_bam_sort(mm355_ctx_t *ctx, const void *rec, int64_t n_bytes, const int64_t *rec_off, int64_t n_rec, int where, mm355_run_t **out);
int mm355_map_batch_bam_run(mm355_ctx_t *ctx, const mm355_mapopt_t *mo, int64_t n_reads, const char *const *seqs, const int32_t *lens,
                            const char *const *names, const char *const *quals, const uint8_t *const *aux, const int32_t *aux_len,
                            const int32_t *aux_mod, int flags, int sam_flags, int where, mm355_run_t **out);
int mm355_bam_gather(const void *base, int64_t base_len, const int64_t *src_off, const int64_t *len, int64_t n, void *out, int64_t out_cap);
void mm355_free_run(mm355_run_t *r);

/* --- the .bai index of a coordinate-sorted BAM file (mm355_bai.h states the rule once; SAM v1 sections 5.2 and 5.3).
 * THE SPAN of a record (`rec` with its block_size word, any address): l_read_name is the byte at 12, n_cigar_op the uint16 at 16, flag the
 * uint16 at 18, pos the int32 at 8, and the CIGAR words lie at 36 + l_read_name.  reflen is the 64-bit sum of the lengths (word >> 4) of
 * the words whose op (word & 15) is M, D, N, = or X (0, 2, 3, 7, 8); every other op code, 9 to 15 included, adds nothing; reflen is 0 when
 * flag & 4 or n_cigar_op == 0.  end = pos + max(1, reflen): the writer's own rule for `bin`, and htslib's bam_endpos.  The long-CIGAR
 * form needs no case: its two placeholder words `l_seq S, reflen N` sum to reflen, and the CG tag is not read.
 *   span = end << 1 | (flag >> 2 & 1)
 * The _span calls take the arguments of their siblings and also fill run->span, n_rec entries in the order of rec: on the host serially,
 * on the device by k_rec_span (mm355_bam.hip) on the sorted stream where it lies in HBM -- a wave per record, the words lane-strided from
 * aligned dwords shifted into place, a 64-bit wave sum -- so that 8 more bytes per record cross to the host.  MM355_EINVAL, before
 * anything is launched: a record whose 36 + l_read_name + 4 * n_cigar_op passes its length.  The calls without _span are these without the
 * span: they launch, copy and return what they always did, and their run->span is NULL.  MM355_BAM_TIMES=1: the bam_sort_times line of a
 * _span call on the device ends with k_rec_span_us.
 * THE BUILDER is host code and takes keys, spans, lengths and BGZF blocks -- never record bytes.
 *   mm355_bai_open     n_ref contigs; first_block_at: the file offset of the first block of records (the length of the header blocks)
 *   mm355_bai_records  n records in FILE ORDER, repeatable: record i has ref = key >> 32 (as int32), beg = pos = ((uint32)key >> 1) - 1,
 *                      end = span >> 1, the unmapped bit span & 1 and len[i] bytes; u_i, the running sum of the lengths, is its offset in
 *                      the unframed stream
 *   mm355_bai_blocks   n bytes of whole BGZF blocks as they were just written behind those before, repeatable: walked by BSIZE
 *                      (mm355_bgzfwalk.h); a block's size and ISIZE are noted.  No block is assumed to hold 0xff00 bytes.
 *   mm355_bai_finish   the bytes of the .bai as a text (free: mm355_free_text; n_reads / n_lines: the bins' chunks before / after the
 *                      finishing merges).  May be called again after more records or blocks.
 *   mm355_bai_close
 * Virtual offsets: V(u) = coffset(b) << 16 | (u - isum(b)), b the first block with isum(b + 1) > u -- blocks of ISIZE 0 are passed over;
 * for u the stream's length b is one past the last block, uoffset 0.  vb_i = V(u_i), ve_i = V(u_{i+1}).
 * Records with ref < 0 only count in n_no_coor.  bin = reg2bin(beg, end) of section 5.3, recomputed, not taken from the record.  Raw
 * chunks: the maximal runs of consecutive records of equal (ref, bin), [vb of the first, ve of the last) (hts_idx_push's rule).  Linear
 * index: for w in beg >> 14 .. (end - 1) >> 14, ioffset[ref][w] is the vb of the first record in file order that touches w; n_intv is one
 * past the largest touched w; an untouched window takes the value of the next touched one above it.  Pseudo-bin 37450 per ref with records:
 * the chunks (vb of its first record, ve of its last) and (n_mapped, n_unmapped) -- unmapped is the flag bit.  Finishing a ref, in the
 * spirit of htslib's compress_binning (no claim of byte equality with samtools): level 5 down to 1, bins ascending, a bin is emptied into
 * its parent (b - 1) >> 3 (created if absent) and removed when (max end >> 16) - (min beg >> 16) < 0x10000 over the chunks it then holds
 * -- so a merge can cascade; then every bin's chunks are sorted by (beg, end) and merged while next.beg >> 16 <= prev.end >> 16, end = max.
 * Bytes: "BAI\1", n_ref; per ref n_bin, the bins ASCENDING BY NUMBER with 37450 last (bin, n_chunk, the chunks), n_intv and the offsets;
 * n_no_coor as a trailing uint64.  A ref without records has n_bin = 0 and n_intv = 0.  The file is a pure function of the BAM file.
 * MM355_EINVAL: keys that do not ascend (an unsorted stream has no index; also across calls), ref >= n_ref, pos < 0 on a placed record,
 * end > 2^29 (or end <= pos), a length below 37 -- all n records of a call are checked before one is taken; bytes that are not whole BGZF
 * blocks; at finish, ISIZEs that do not sum to the records' lengths.  n_ref < 0 or first_block_at < 0 at open. */
int mm355_bam_sort_span(mm355_ctx_t *ctx, const void *rec, int64_t n_bytes, const int64_t *rec_off, int64_t n_rec, int where, mm355_run_t **out);
int mm355_map_batch_bam_run_span(mm355_ctx_t *ctx, const mm355_mapopt_t *mo, int64_t n_reads, const char *const *seqs, const int32_t *lens,
                                 const char *const *names, const char *const *quals, const uint8_t *const *aux, const int32_t *aux_len,
                                 const int32_t *aux_mod, int flags, int sam_flags, int where, mm355_run_t **out);
typedef struct mm355_bai mm355_bai_t;
int mm355_bai_open(int32_t n_ref, int64_t first_block_at, mm355_bai_t **out);
int mm355_bai_records(mm355_bai_t *h, const uint64_t *key, const int64_t *span, const int64_t *len, int64_t n);
int mm355_bai_blocks(mm355_bai_t *h, const void *bytes, int64_t n);
int mm355_bai_finish(mm355_bai_t *h, mm355_text_t **out);
void mm355_bai_close(mm355_bai_t *h);

/* --- compressed runs: a sorted file whose records never lie uncompressed outside HBM (mm355_bammerge.h states the step once).
 * A PACKED RUN is what mm355_map_batch_bam_run_packed returns: the arguments of mm355_map_batch_bam_run_span plus want_span (0: no spans,
 * as mm355_map_batch_bam_run; anything else: spans).  Everything up to the sorted stream (and the spans) is that call's; then the stream
 * is deflated where it lies (the device: k_bgzf_deflate / k_bgzf_compact on the sorted records in HBM, and only the members, keys,
 * offsets and spans cross to the host; the host formatter: the serial coder, the same bytes).  Field by field:
 *   n_rec, key, span, ms_sort, on_device   as in an unpacked run
 *   rec_off    still the n_rec + 1 offsets into the UNFRAMED stream: rec_off[n_rec] is the raw length
 *   rec        the BGZF members of that stream at level 1: byte for byte mm355_bgzf_deflate(level 1) of the unpacked run's rec
 *   n_bytes    the members' byte count (never more than raw + 31 * n_blk: a payload deflate would not shorten is stored)
 *   n_blk      the members: ceil(raw / 0xff00); member b holds raw bytes [b * 0xff00, min((b + 1) * 0xff00, raw))
 *   blk_off    n_blk + 1 offsets of the members inside rec; blk_off[n_blk] == n_bytes
 *   packed     1
 * The calls without _packed return what they always did, with packed == 0, n_blk == 0 and blk_off == NULL.
 * THE MERGE STEP takes records out of such members and writes the next BGZF blocks of the merged file.
 *   base, base_len        the spool: the members of all runs as they were written, memory-mapped
 *   slice_at[s], slice_bytes[s]   s < n_slice: a range of the spool that holds whole members of one run
 *   slice_raw_at[s]       the offset, in that run's unframed stream, of the first payload byte of the slice's first member
 *   rec_slice[i], rec_at[i], rec_len[i]   i < n_rec, in merged order: record i is rec_len[i] bytes at offset rec_at[i] of the unframed
 *                         stream of the run slice rec_slice[i] belongs to, i.e. at rec_at[i] - slice_raw_at[...] of the slice's payloads
 *   carry, n_carry        the raw bytes the previous step left over, fewer than 0xff00
 *   final                 not 0: the last step -- everything is written, a short last payload too
 *   where                 MM355_PAF_HOST (ctx may be NULL), MM355_PAF_DEVICE, or MM355_PAF_AUTO, which is the host as for mm355_bgzf_wrap
 *   level                 0: stored blocks, 1: deflated, as for mm355_bgzf_deflate
 *   out                   the BGZF blocks of every whole 0xff00-byte payload of `carry + records` (final: of all of it); n_lines counts
 *                         the blocks; a step smaller than one payload gives a text of zero bytes
 *   carry_out, n_carry_out   room for 0xff00 bytes (it may be `carry` itself): the raw bytes behind the last whole payload, and their count
 * The blocks of consecutive steps, one behind the other, are mm355_bgzf_deflate(level) of the merged stream, whatever the steps' sizes.
 * On the host: mm355_bgzfwalk.h walks the members, mm355_inflate.h inflates them, mm355_bam_gather's loop copies the records, the host
 * framer or coder writes the blocks.  On the device: one upload of the compressed slices through pinned staging; the host walks the
 * members of all slices into one table (every payload's place a prefix sum); k_bgzf_inflate inflates them into one buffer in HBM;
 * k_rec_gather (mm355_bam.hip) copies record i from its place in that buffer to n_carry + sum(rec_len[0 .. i)) of the output stream --
 * k_rec_permute's tile scheme and copy loop with a per-record source address: a block per 4096 output bytes of a record, a thread per
 * aligned 16-byte store from shifted source dwords, byte stores at the ragged ends, every byte one writer; the deflate or framing
 * kernels run on the whole payloads, and one copy brings the blocks down.
 * MM355_EINVAL, before anything is allocated on the device or launched: a slice that passes base_len; a negative length or offset; a
 * record whose [rec_at - slice_raw_at, + rec_len) passes the sum of the ISIZEs of its slice's members; rec_slice out of range;
 * n_carry >= 0xff00; an unknown `where` or `level`; MM355_PAF_DEVICE without a context.  MM355_EIO: a slice that is not whole BGZF
 * members, or a member the inflater refuses (it checks CRC-32 and ISIZE); nothing is returned then, and carry_out is untouched.
 * MM355_BAM_TIMES=1: a device step prints a line on stderr (members in, bytes in, records, bytes out; inflate, gather and deflate each
 * between two events). */
int mm355_map_batch_bam_run_packed(mm355_ctx_t *ctx, const mm355_mapopt_t *mo, int64_t n_reads, const char *const *seqs, const int32_t *lens,
                                   const char *const *names, const char *const *quals, const uint8_t *const *aux, const int32_t *aux_len,
                                   const int32_t *aux_mod, int flags, int sam_flags, int where, int want_span, mm355_run_t **out);
int mm355_bam_merge_step(mm355_ctx_t *ctx, const void *base, int64_t base_len, const int64_t *slice_at, const int64_t *slice_bytes,
                         const int64_t *slice_raw_at, int64_t n_slice, const int32_t *rec_slice, const int64_t *rec_at, const int64_t *rec_len,
                         int64_t n_rec, const void *carry, int64_t n_carry, int final, int where, int level, mm355_text_t **out,
                         void *carry_out, int64_t *n_carry_out);

/* --- BGZF input: the inverse of mm355_bgzf_deflate.  `data` is n bytes of BGZF members (what mm355_bgzf_wrap / _deflate, bgzip or any BAM
 * writer produced): gzip members with the BC extra subfield (other subfields may stand in front of it; MTIME, XFL and OS are ignored), cdata of
 * at most 64 KB holding any RFC 1951 stream -- several deflate blocks, stored, fixed and dynamic ones, run symbols 16 - 18, codes of 15 bits,
 * a single one-bit distance code or none, distances up to 32768, ISIZE 0 (the EOF block) to 65536.  The host walks the members by BSIZE
 * (mm355_bgzfwalk.h), which gives every payload its place; the members are inflated by the decoder of mm355_inflate.h, one after the other
 * on the host (ctx may be NULL) or a workgroup per member on the device (mm355_inflate.hip: k_bgzf_inflate; an upload, the kernel, a copy
 * back).  `where`: MM355_PAF_HOST, MM355_PAF_DEVICE, or MM355_PAF_AUTO, which is the host here as for mm355_bgzf_wrap.  `text` is the
 * payloads back to back, n_lines the number of members (the empty EOF member counts), n_reads 0; n == 0 gives zero bytes.
 * The input is untrusted: the decoder reads and writes inside the spans the walk gave and refuses a member for BTYPE 11, stored LEN != ~NLEN,
 * an over-subscribed code, an incomplete one (but a single code of one bit, and a distance set without any code), a missing end-of-block
 * code, a run symbol without a previous length or past HLIT + HDIST, literal/length symbols 286 / 287 and distance symbols 30 / 31, a
 * distance before the payload's first byte, output beyond or short of ISIZE, input that ends inside a symbol, and a CRC-32 that is not the
 * trailer's -- what zlib's inflate refuses.  Bytes between the last deflate block and the trailer are ignored.
 * MM355_EINVAL: the data's first bytes are no BGZF member (plain gzip, text).  MM355_EIO: a later member is malformed, the data ends inside a
 * member, or a member was refused.  Nothing is returned then.  A missing EOF member is no error.
 * MM355_INFLATE_TIMES=1: a device call prints a line on stderr (members, bytes in and out, the kernel's time between two events). */
int mm355_bgzf_inflate(mm355_ctx_t *ctx, const void *data, int64_t n, int where, mm355_text_t **out);

/* --- streaming FASTA / FASTQ reader, plain or gzip: the record rules of the index builder's parser (the name ends at the first blank,
 * multi-line sequences, a '+' line followed by quality as long as the sequence, CRLF).  A read set is cut into sub-batches without ever
 * being in memory as a whole.  mm355_fastx_next returns the next records: at least one, at most max_reads, and no record that would take
 * the sub-batch over max_bases unless it is its first (both limits >= 1); *out = NULL with return 0 at the end of the file.  MM355_EIO: the
 * file cannot be opened, or its gzip stream is truncated or corrupt (reported when the reader gets there); MM355_EINVAL: a record of 2^31
 * or more bases.  After an error every further call returns it again.  The reads own what they point to: names[i] is NUL-terminated,
 * seqs[i] has lens[i] bases. */
typedef struct mm355_fastx mm355_fastx_t;
typedef struct { int64_t n; const char *const *seqs; const int32_t *lens; const char *const *names; } mm355_reads_t;
int mm355_fastx_open(const char *path, mm355_fastx_t **out);
int mm355_fastx_next(mm355_fastx_t *fx, int64_t max_reads, int64_t max_bases, mm355_reads_t **out);
void mm355_reads_free(mm355_reads_t *r);
/* the same reader keeping FASTQ qualities: the quality strings of a sub-batch, parallel to seqs[] -- NULL for a reader opened without
 * quality; an entry is NULL for a FASTA record or a record whose quality length differs from its sequence length, otherwise lens[i] bytes */
int mm355_fastx_open_qual(const char *path, mm355_fastx_t **out);
const char *const *mm355_reads_quals(const mm355_reads_t *r);
void mm355_fastx_close(mm355_fastx_t *fx);
/* BAM as a reads file: when the (inflated) stream begins "BAM\1", mm355_fastx_next reads BAM records instead of text, whichever open made the
 * handle -- unaligned BAM as basecallers write it, or an aligned one.  The header is skipped; a record with flag & 0x900 (secondary,
 * supplementary) is skipped as `samtools fastq` skips it; the name is read_name, the bases come from the nibbles ("=ACMGRSVTWYHKDBN"), the
 * quality is qual + 33 (first byte 0xff: none); a record with flag 0x10 is reverse-complemented and its quality reversed, back to the read
 * as sequenced.  Aux tags are dropped unless mm355_fastx_keep_aux asks for them.  MM355_EIO: block_size below 32, l_read_name 0, name + CIGAR + SEQ + QUAL beyond block_size, or a
 * stream that ends inside the header or a record.  The index builders do not read BAM: a BAM is no reference.
 * mm355_fastx_open_device: the same reader over a BGZF file (bgzip FASTQ / FASTA, BAM) whose members GPU `device` inflates
 * (k_bgzf_inflate).  The file is read in pieces of 32 MB of compressed bytes (MM355_INFLATE_PIECE=<bytes> overrides it; a piece always
 * holds at least one whole member) into two pinned buffers; upload, kernel and the copy of the inflated bytes back run on a stream the
 * handle owns while the next piece is read and walked; the record loop on the host cuts the bytes.  keep_qual != 0: as mm355_fastx_open_qual.
 * MM355_EINVAL: the file's first bytes are no BGZF member (plain text, plain gzip) -- nothing is opened and no device is touched: open it with
 * mm355_fastx_open.  MM355_EIO: unreadable.  MM355_ENODEV / ENOMEM / EHIP.  A malformed or refused member surfaces as MM355_EIO from
 * mm355_fastx_next when the reader gets there.  MM355_INFLATE_TIMES=1: a line per piece on stderr. */
int mm355_fastx_open_device(const char *path, int keep_qual, int device, mm355_fastx_t **out);
/* Aux tags of a BAM reads file.  mm355_fastx_keep_aux: `tags` as mm355_bam_aux_split's `keep`, or NULL for none (the default); it must come
 * before the first mm355_fastx_next -- after it, and for a malformed `tags`, MM355_EINVAL.  On a stream that turns out not to be a BAM it has
 * no effect.  The reader then reads a record's aux block (in chunks, never allocating by a length the stream has not delivered) instead of
 * skipping it and runs it through mm355_bam_aux_split; a malformed block is MM355_EIO like every other malformed record.  A record with flag
 * 0x10 keeps its aux verbatim: MM / ML are defined on the read as sequenced, which is what the reader restores.  Either byte source
 * (mm355_fastx_open*, mm355_fastx_open_device) serves it.
 * mm355_reads_aux: the blocks of a sub-batch, parallel to seqs[] -- aux[i] has (*aux_len)[i] bytes, its second group from (*aux_mod)[i], as
 * mm355_bam_format_aux takes them; NULL (and NULL lengths) when nothing is kept or the stream is no BAM.  The reads own them.
 * mm355_fastx_bam_rg: the @RG lines of the BAM's header text, verbatim and newline-terminated, *len their bytes (an RG:Z tag without its
 * header line is no valid file: the writer of the output header needs them); NULL and 0 for a stream that is no BAM or a header without
 * @RG.  It may be called before the first mm355_fastx_next and reads the header then; once records have been read it answers only if
 * mm355_fastx_keep_aux was set (a reader that keeps nothing skips the header text as before).  The handle owns the string. */
int mm355_fastx_keep_aux(mm355_fastx_t *fx, const char *tags);
const uint8_t *const *mm355_reads_aux(const mm355_reads_t *r, const int32_t **aux_len, const int32_t **aux_mod);
const char *mm355_fastx_bam_rg(mm355_fastx_t *fx, int64_t *len);

/* --- per-stage entry points (same kernels as mm355_map_batch; used by the parity tests and
 * by bench.py to time one kernel with HIP events).  Outputs are caller-allocated host buffers. --- */
typedef struct {
	int64_t n_reads, n_bases;
	int64_t n_mz, n_hit, n_a, n_a_multi;       /* SURVEY 8(d) counters of the seed stage */
	int64_t chain_pairs, dp_cells, n_dp_jobs;
	double ms_sketch, ms_seed, ms_sort, ms_chain, ms_backtrack, ms_dp, ms_host, ms_total;
	double ms_seed_lookup, ms_seed_expand;
	int64_t n_launch_seed;
	int64_t n_launch_dp;                         /* extension launch groups (one per round and HBM-budget chunk) */
	/* per extension kernel of a launch group, timed with HIP events on the stream it is launched on; group = 2 * size class + exact,
	 * size classes: targets <= 128, 256, 512, 1024 (k_ksw_reg<1|2|4|8, exact>), <= 4096, <= 12288, larger (k_ksw_extd2<512>; one launch
	 * for groups 8-9, timed as 8, and one for 10-13, timed as 10); 14 / 15 / 16 = k_ksw_row<2|4|8> (full-band approximate gap fills), 17 k_ksw_rowl,
	 * 18 k_ksw_regw8, 19 / 20 / 21 = k_ksw_band<1|2|4> (the same fills on a band of 128 / 256 / 512 diagonals), 22 = k_ksw_band2 (64 diagonals, two problems per wave),
	 * 23 = second run of band problems */
	double ms_dp_group[24];
	int64_t dp_cells_group[24], n_launch_group[24];
	int64_t n_ext_rounds;                        /* extension rounds of the last call (the reference has no bound on them) */
	int64_t n_sort_fast_reads, n_sort_tie_reads; /* anchor sort: reads of anchor-rich batches (cull + per-read LDS sort) / of those, reads whose surviving
	                                                anchors contain equal keys and went through the literal radix_sort_128x emulation */
	/* mg_lchain_rmq on the device (row a9): kernel time, reads re-chained there, reads handed to the literal host implementation because the
	 * device could not prove its range-minimum answer unique (or ran out of LDS capacity), window elements looked at */
	double ms_rmq;
	int64_t n_rmq_reads, n_rmq_host, rmq_scanned;
	double host_cpu_ms;                          /* CPU time (not wall) the host tail of the last call spent, summed over the pool threads */
	int64_t n_a_kept;                            /* anchors left after the cull of the anchor-rich sort path (x-components too small to chain dropped);
	                                                0 when the batch took the literal path for every read */
	/* every kernel outside the extension rounds, timed alone with a HIP-event pair on the stream it is launched on (the extension kernels:
	 * ms_dp_group).  Slots: 0 sketch, 1 mz_flt, 2 seed lookup (tile list + probes), 3 seed select, 4 seed expand, 5 anchor cull, 6 anchor
	 * sort (LDS), 7 literal radix_sort_128x emulation (reads with equal keys), 8 chain segments, 9 chain (long segments, a wave each),
	 * 10 chain (short segments, a lane each), 11 chain backtrack, 12 / 13 / 14 mg_lchain_rmq sort / recurrence / backtrack, 15 extension
	 * gather, 16 extension backtrack (CIGAR), 17 mm_update_extra + cs walk, 18 read codes, 19 chain / anchor pack; the literal emulation by kernel:
	 * 7 k_sort_level_mw<1024> (all its levels), 20 k_sort_level_mw<256>, 21 k_sort_tasks, 22 its plain sort / copy / tcnt of the tie reads;
	 * 23 the chain-only region stage (k_regs) */
	double ms_kernel[24];
	int64_t chain_pairs_big;                     /* k_chain_big's share of chain_pairs */
	int64_t n_a_literal;                         /* anchors (all of them, culled ones included) of the reads that were sorted literally */
	int64_t n_v_rmq;                             /* anchors mg_lchain_rmq chained on the device */
	int64_t n_dp_band, n_dp_band_redo;           /* gap fills run on a diagonal band with a sufficiency proof / of those, run again on the full matrix */
	int64_t n_rounds_split;                      /* extension rounds whose direction matrices did not fit the HBM budget and were cut into several launches */
	/* chain-only calls (mo->flag without MM_F_CIGAR): reads whose region logic ran on the device (k_regs, kernel time in ms_kernel[23]) /
	   reads that took the host path (the RMQ stage left them to the host, an argument of logf beyond the device table, a strand_retained
	   comparison on a divergence that pow() rounding could move -- with MM355_OUT_TAGS any reported divergence that it could move --, or
	   MM355_REGS_HOST=1) */
	int64_t n_regs_dev, n_regs_host;
} mm355_stats_t;

/* sketch: minimizers of each read (mm_sketch). mz_off[n_reads+1] host array is filled; mz = (x,y) pairs */
int mm355_stage_sketch(mm355_ctx_t *ctx, int64_t n_reads, const char *const *seqs, const int32_t *lens,
                       int64_t *mz_off, uint64_t *mz, int64_t mz_cap);
/* seeds: sketch + mm_seed_mz_flt + mm_collect_matches + collect_seed_hits; anchors in generation order
 * (sorted = 0), after the radix_sort_128x emulation (sorted = 1: the reference's whole sorted array) or as the mapping path hands them
 * to the chainer (sorted = 2: anchor-rich batches drop the x-components that are too small to chain, see mm355_cullsort.hip; a_off
 * then describes the shorter arrays). */
int mm355_stage_anchors(mm355_ctx_t *ctx, const mm355_mapopt_t *mo, int64_t n_reads, const char *const *seqs,
                        const int32_t *lens, int sorted, int64_t *a_off, uint64_t *a, int64_t a_cap,
                        int32_t *rep_len, int32_t *n_mini_pos);
/* the same with query names (see mm355_map_batch_named); anchors a named read generates against its own copy off the diagonal carry
 * MM_SEED_SELF (bit 43 of y) */
int mm355_stage_anchors_named(mm355_ctx_t *ctx, const mm355_mapopt_t *mo, int64_t n_reads, const char *const *seqs,
                              const int32_t *lens, const char *const *names, int sorted, int64_t *a_off, uint64_t *a, int64_t a_cap,
                              int32_t *rep_len, int32_t *n_mini_pos);
/* chaining DP fill (mg_lchain_dp) on the sorted anchors: f, p, v per anchor (p as int32, -1 = none) */
int mm355_stage_chain(mm355_ctx_t *ctx, const mm355_mapopt_t *mo, int64_t n_reads, const char *const *seqs,
                      const int32_t *lens, int64_t *a_off, uint64_t *a, int32_t *f, int32_t *p, int32_t *v, int64_t a_cap);
/* chains after backtrack + compact_a: u (score<<32|cnt) and the compacted anchors */
int mm355_stage_chains(mm355_ctx_t *ctx, const mm355_mapopt_t *mo, int64_t n_reads, const char *const *seqs,
                       const int32_t *lens, int64_t *u_off, uint64_t *u, int64_t u_cap,
                       int64_t *a_off, uint64_t *a, int64_t a_cap);
/* chains after the long-join re-chain (mg_lchain_rmq on the chained anchors when U:map.c::mm_map_frag's rescue test fires) or, for MM_F_RMQ
 * presets, after mg_lchain_rmq as the primary chainer: u and the compacted anchors as mm355_stage_chains returns them, plus state[r]:
 * 0 = not re-chained, 1 = re-chained on the device, 2 = the long-join re-chain is left to the literal host implementation (equal range-minimum
 * priorities): a[] then holds the read's chained anchors sorted by x and u_off[r+1] == u_off[r]; 3 = every mg_lchain_rmq call of the read is
 * left to the host (MM_F_RMQ presets whose primary pass was handed back, or MM355_RMQ_ON_HOST=1): a[] = the read's sorted anchors */
int mm355_stage_rmq(mm355_ctx_t *ctx, const mm355_mapopt_t *mo, int64_t n_reads, const char *const *seqs,
                    const int32_t *lens, int64_t *u_off, uint64_t *u, int64_t u_cap,
                    int64_t *a_off, uint64_t *a, int64_t a_cap, int32_t *state);
/* one batch of banded extension problems (ksw_extd2_sse semantics); see mm355_dpjob_t */
typedef struct {
	int32_t qlen, tlen;
	int64_t qoff, toff;     /* offsets into the code arrays (0..4 per byte) */
	int32_t w, zdrop, end_bonus, flag;
} mm355_dpjob_t;
typedef struct {
	int32_t max, zdropped, max_q, max_t, mqe, mqe_t, mte, mte_q, score, reach_end, n_cigar;
	int64_t cigar_off;
} mm355_dpres_t;
int mm355_stage_dp(mm355_ctx_t *ctx, const mm355_mapopt_t *mo, int64_t n_jobs, const mm355_dpjob_t *jobs,
                   const uint8_t *qcodes, int64_t n_q, const uint8_t *tcodes, int64_t n_t,
                   mm355_dpres_t *res, uint32_t *cigar, int64_t cigar_cap);
/* the per-base walk of an aligned region (minimap2 align.c::mm_update_extra after mm_fix_cigar: mlen, blen, n_ambi, dp_max) and its cs
   string (format.c::write_cs_core, either form), as the mapping path runs them on the device for all regions of a batch (k_extra).
   Stage entry for parity tests: the query codes (0..4 per byte) come from the caller, the target from the index (contig rid, from t_st).
   want_cs: bit 0 = cs, bit 1 = MD (format.c::write_MD_core); both strings land in `cs` (cs_off / md_off); bit 2 = gap counts: `pad` returns
   the number of I / D operations of the CIGAR (n_gapo) and `pad2` their summed lengths (n_gap); both stay 0 without the bit; bit 3 = cs in
   the long form (implies bit 0's cs_off / cs_len; with bit 0 still the long form). */
typedef struct { int64_t q_off; int64_t cigar_off; int32_t rid, t_st, n_cigar, pad; } mm355_extrajob_t;
typedef struct { int32_t mlen, blen, n_ambi, dp_max; int64_t cs_off; int32_t cs_len, pad; int64_t md_off; int32_t md_len, pad2; } mm355_extrares_t;
int mm355_stage_extra(mm355_ctx_t *ctx, const mm355_mapopt_t *mo, int64_t n_regions, const mm355_extrajob_t *jobs,
                      const uint8_t *qcodes, int64_t n_q, const uint32_t *cigar, int64_t n_cigar, int want_cs,
                      mm355_extrares_t *res, char *cs, int64_t cs_cap);

int mm355_get_stats(mm355_ctx_t *ctx, mm355_stats_t *st);   /* counters/timers of the last call on ctx */
int mm355_device_count(void);
int mm355_device_synchronize(int device_id);                /* drains every stream of the device (hipDeviceSynchronize): bench.py brackets its timed region with it */
const char *mm355_strerror(int code);
const char *mm355_version(void);

#ifdef __cplusplus
}
#endif
#endif
