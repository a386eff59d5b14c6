// mm355_sam.h -- the SAM lines of one read, stated once: mappy_rs.sam_lines (format.c::mm_write_sam3, write_sam_cigar, sam_write_sq and
// write_tags of minimap2 2.26) byte for byte.  One emitter, templated on a sink, as mm355_paf.h: the counting sink and the writing sinks run
// the same code, and the host formatter below is that emitter run serially.  Plain C++ that also compiles as device code
// (tests/host_harness/sam_host.cpp builds it with g++ alone).
//
// A sink has what a PAF sink has -- ch(c), bytes(p, n), cigar(w, n) -- and seq(p, n, rev, comp): a run of n read or quality bytes that
// exists in memory, written forwards or (rev) from its last byte to its first, each byte complemented (comp) or not.  SEQ and QUAL are the
// bulk of the text: the device sinks only note them down, and a kernel of its own copies them (mm355_sam.hip::k_sam_copy).
#pragma once
#include "mm355_paf.h"

// minimap2's seq_comp_table: bytes below 128, case kept, A<->T C<->G R<->Y K<->M B<->V D<->H, U->A; everything else (S W N among them) stays
MM_HD unsigned char sam_comp(unsigned char c)
{
	const unsigned char u = c & 0xdf;     // the upper-case letter of a letter
	if (c >= 128 || u < 'A' || u > 'Z') return c;
	unsigned char d;
	switch (u) {
	case 'A': d = 'T'; break; case 'T': d = 'A'; break; case 'U': d = 'A'; break;
	case 'C': d = 'G'; break; case 'G': d = 'C'; break;
	case 'R': d = 'Y'; break; case 'Y': d = 'R'; break;
	case 'K': d = 'M'; break; case 'M': d = 'K'; break;
	case 'B': d = 'V'; break; case 'V': d = 'B'; break;
	case 'D': d = 'H'; break; case 'H': d = 'D'; break;
	default: return c;
	}
	return (unsigned char)(d | (c & 0x20));
}

// ---- what the lines of one read are made from.  Contig names as one byte string and n_seq + 1 offsets (the form the device has them in).
struct SamRead {
	const mm355_hit_t *rows; const mm355_tags_t *tags; int32_t n_rows;   // the read's rows, in row order (SA:Z: names the other primaries)
	const char *qname; int64_t qname_len; int32_t qlen;                  // the bytes to print (an unnamed read: "*", 1)
	const char *seq, *qual;                                              // qlen bytes each; qual == 0: the read has none
	const char *tn; const int64_t *tn_off;
	const uint32_t *cigar; const char *str;                              // the batch's CIGAR words and string arena
	int32_t rep_len; int sam_flags;                                      // rep_len: of an unmapped read (a row's comes from its tags row)
	const uint8_t *aux; int32_t aux_len, aux_mod;                        // copied aux tags (BAM records only; the text formats do not print them): [0, aux_mod) on
	                                                                     // every record, [aux_mod, aux_len) on records that hold the whole read; none: 0, 0, 0
};
// the copied aux tags of a batch, per read: aux == 0: none; aux[i] == 0: read i has none
struct RecAux { const uint8_t *const *aux = 0; const int32_t *len = 0, *mod = 0; };
struct SamLine { const SamRead *R; int32_t row; };                       // row < 0: the unmapped record

MM_HD uint32_t sam_flag_of(const mm355_hit_t &h, const mm355_tags_t &t)
{
	return (h.strand < 0? 0x10u : 0u) | (!h.is_primary? 0x100u : !(t.flags & MM355_TAG_SAM_PRI)? 0x800u : 0u);
}
template <typename S> MM_HD void sam_clip(S &s, uint32_t n, char letter) { if (n) { paf_u64(s, n); s.ch(letter); } }

// one entry of SA:Z: -- rname,pos,strand,cigar,mapq,nm; (the names go out byte by byte: they are short, and no run table bounds them)
template <typename S> MM_HD void sam_emit_sa(S &s, const SamRead &R, const mm355_hit_t &q, const mm355_tags_t &qt)
{
	const bool rev = q.strand < 0;
	const uint32_t ql = (uint32_t)(q.query_end - q.query_start), tl = (uint32_t)(q.target_end - q.target_start);
	const uint32_t clip5 = (uint32_t)(rev? R.qlen - q.query_end : q.query_start), clip3 = (uint32_t)(rev? q.query_start : R.qlen - q.query_end);
	for (int64_t i = R.tn_off[q.rid]; i < R.tn_off[q.rid + 1]; ++i) s.ch(R.tn[i]);
	s.ch(','); paf_i64(s, (int64_t)q.target_start + 1);
	s.ch(','); s.ch(rev? '-' : '+'); s.ch(',');
	uint32_t l_M, l_I = 0, l_D = 0;
	if ((int64_t)q.query_end - q.query_start < (int64_t)q.target_end - q.target_start) { l_M = ql; l_D = tl - ql; }
	else { l_M = tl; l_I = ql - tl; }
	sam_clip(s, clip5, 'S'); sam_clip(s, l_M, 'M'); sam_clip(s, l_I, 'I'); sam_clip(s, l_D, 'D'); sam_clip(s, clip3, 'S');
	s.ch(','); paf_u64(s, q.mapq);
	s.ch(','); paf_i64(s, (int64_t)q.block_len - q.match_len + qt.n_ambi);
	s.ch(';');
}

template <typename S> MM_HD void sam_emit_line(S &s, const SamLine &L)
{
	const SamRead &R = *L.R;
	s.bytes(R.qname, R.qname_len);
	if (L.row < 0) {   // a read without hits
		paf_lit(s, "\t4\t*\t0\t0\t*\t*\t0\t0\t");
		s.seq(R.seq, R.qlen, false, false);
		s.ch('\t');
		if (R.qual) s.seq(R.qual, R.qlen, false, false); else s.ch('*');
		paf_tag_i(s, "\trl:i:", R.rep_len);
		s.ch('\n');
		return;
	}
	const mm355_hit_t &h = R.rows[L.row]; const mm355_tags_t &t = R.tags[L.row];
	const bool rev = h.strand < 0, soft = (R.sam_flags & MM355_SAM_SOFTCLIP) != 0;
	const uint32_t flag = sam_flag_of(h, t);
	s.ch('\t'); paf_u64(s, flag);
	s.ch('\t'); s.bytes(R.tn + R.tn_off[h.rid], R.tn_off[h.rid + 1] - R.tn_off[h.rid]);
	s.ch('\t'); paf_i64(s, (int64_t)h.target_start + 1);
	s.ch('\t'); paf_u64(s, h.mapq);
	s.ch('\t');
	if (h.n_cigar > 0) {
		const char letter = (flag & 0x800) && !soft? 'H' : 'S';
		sam_clip(s, (uint32_t)(rev? R.qlen - h.query_end : h.query_start), letter);
		s.cigar(R.cigar + h.cigar_off, h.n_cigar);
		sam_clip(s, (uint32_t)(rev? h.query_start : R.qlen - h.query_end), letter);
	} else s.ch('*');
	paf_lit(s, "\t*\t0\t0\t");
	if ((flag & 0x900) == 0 || soft) {
		s.seq(R.seq, R.qlen, rev, rev);
		s.ch('\t');
		if (R.qual) s.seq(R.qual, R.qlen, rev, false); else s.ch('*');
	} else if (flag & 0x100) paf_lit(s, "*\t*");
	else {   // supplementary, hard-clipped: the aligned part of the read
		s.seq(R.seq + h.query_start, h.query_end - h.query_start, rev, rev);
		s.ch('\t');
		if (R.qual) s.seq(R.qual + h.query_start, h.query_end - h.query_start, rev, false); else s.ch('*');
	}
	paf_emit_tags(s, h, t, true);
	if (h.is_primary) {
		bool any = false;
		for (int32_t j = 0; j < R.n_rows; ++j) {
			const mm355_hit_t &q = R.rows[j];
			if (j == L.row || !q.is_primary || q.n_cigar <= 0) continue;
			if (!any) { paf_lit(s, "\tSA:Z:"); any = true; }
			sam_emit_sa(s, R, q, R.tags[j]);
		}
	}
	if (h.cs_len >= 0) { paf_lit(s, "\tcs:Z:"); s.bytes(R.str + h.cs_off, h.cs_len); }
	if (h.md_len >= 0) { paf_lit(s, "\tMD:Z:"); s.bytes(R.str + h.md_off, h.md_len); }
	paf_tag_i(s, "\trl:i:", t.rep_len);
	s.ch('\n');
}

// ---- the serial sinks
struct SamCountSink : PafCountSink {
	MM_HD void seq(const char *, int64_t l, bool, bool) { n += l; }
};
struct SamWriteSink : PafWriteSink {
	MM_HD explicit SamWriteSink(char *p_) : PafWriteSink(p_) {}
	MM_HD void seq(const char *b, int64_t l, bool rev, bool comp)
	{
		for (int64_t i = 0; i < l; ++i) { const unsigned char c = (unsigned char)(rev? b[l - 1 - i] : b[i]); p[n++] = (char)(comp? sam_comp(c) : c); }
	}
};

// ------------------------------------------------------------------ host side
// how many lines read i writes: its rows; one unmapped record for a read without rows (unless hit-only); nothing for an empty sequence
inline int64_t mm355_sam_n_lines(const mm355_hits_t *H, const int32_t *qlens, int sam_flags, int64_t i)
{
	const int64_t nh = H->hit_off[i + 1] - H->hit_off[i];
	if (H->status[i] == MM355_EEMPTY) return 0;
	return nh > 0? nh : qlens[i] > 0 && !(sam_flags & MM355_SAM_HIT_ONLY)? 1 : 0;
}

// everything mm355_paf_check asks, plus what a SAM line reads besides: MM_F_CIGAR (-a implies it), the status array, 0 <= qs <= qe <= qlen on
// every row, no rows on an empty read, the bytes of every read that has some, rep_len where an unmapped record prints it
inline int mm355_sam_check(const mm355_hits_t *H, uint32_t n_seq, bool has_cigar, const char *const *seqs, const int32_t *qlens, const int32_t *rep_len, int sam_flags)
{
	if (!has_cigar || (sam_flags & ~(MM355_SAM_SOFTCLIP | MM355_SAM_HIT_ONLY))) return MM355_EINVAL;
	if (int rc = mm355_paf_check(H, n_seq, true)) return rc;
	if (H->n_reads > 0 && (H->status == 0 || qlens == 0 || seqs == 0)) return MM355_EINVAL;
	for (int64_t i = 0; i < H->n_reads; ++i) {
		const int64_t nh = H->hit_off[i + 1] - H->hit_off[i];
		if (H->status[i] == MM355_EEMPTY) { if (nh) return MM355_EINVAL; continue; }
		if (qlens[i] > 0 && seqs[i] == 0) return MM355_EINVAL;
		if (nh == 0 && rep_len == 0 && mm355_sam_n_lines(H, qlens, sam_flags, i)) return MM355_EINVAL;
		for (int64_t k = H->hit_off[i]; k < H->hit_off[i + 1]; ++k) {
			const mm355_hit_t &h = H->hits[k];
			if (h.query_start < 0 || h.query_start > h.query_end || h.query_end > qlens[i]) return MM355_EINVAL;
		}
	}
	return 0;
}

// the contig names as the emitter reads them
struct SamNames {
	std::string bytes; std::vector<int64_t> off;
	explicit SamNames(const PafNames &nm) : off((size_t)nm.n_seq + 1) {
		for (uint32_t i = 0; i < nm.n_seq; ++i) { off[i] = (int64_t)bytes.size(); bytes += nm.names[i]; }
		off[nm.n_seq] = (int64_t)bytes.size();
	}
};

inline SamRead mm355_sam_read_of(const mm355_hits_t *H, int64_t i, const char *const *qnames, const char *const *seqs, const int32_t *qlens,
                                 const char *const *quals, const int32_t *rep_len, const SamNames &nm, int sam_flags, const RecAux &ax = RecAux())
{
	SamRead R;
	const int64_t k0 = H->hit_off[i];
	R.rows = H->hits + k0; R.tags = H->tags + k0; R.n_rows = (int32_t)(H->hit_off[i + 1] - k0);
	const char *qn = qnames? qnames[i] : 0;
	R.qname = qn? qn : "*"; R.qname_len = qn? paf_qname_len(qn) : 1; R.qlen = qlens[i];
	R.seq = seqs[i]; R.qual = quals? quals[i] : 0;
	R.tn = nm.bytes.data(); R.tn_off = nm.off.data();
	R.cigar = H->cigar; R.str = H->str;
	R.rep_len = R.n_rows == 0 && rep_len? rep_len[i] : 0; R.sam_flags = sam_flags;
	const bool has_aux = ax.aux && ax.aux[i] && ax.len[i] > 0;
	R.aux = has_aux? ax.aux[i] : 0; R.aux_len = has_aux? ax.len[i] : 0; R.aux_mod = has_aux? ax.mod[i] : 0;
	return R;
}

// ---- the format as the shared writers see it (the host walk below; the device record writer, mm355_recdev.h): compile-time facts only
struct SamFmt {
	typedef SamLine Line; typedef SamCountSink HostCount; typedef SamWriteSink HostWrite;
	enum { RUNS = 4, TILE_RUNS = 2 };                                  // runs of a line the wave copies: qname, rname, cs, MD; runs the bulk kernel writes in tiles: SEQ, QUAL
	static constexpr bool WAVE_CIGAR = true, TILED = true, FRAMED = false;   // the CIGAR is text, which the wave writes; SEQ and QUAL go in tiles; the text is the result
	// every line has its newline at least, and none is too long; lines the upload takes (the tile table has TILE_RUNS runs per line)
	static constexpr int64_t MIN_RECORD = 1, MAX_RECORD = INT64_MAX, MAX_LINES = INT32_MAX / TILE_RUNS;
	static MM_HD int64_t word_term(uint32_t w) { return paf_cigar_width(w); }   // summed over a row's CIGAR words: the length of the CIGAR text
	template <typename S> static MM_HD void emit(S &s, const SamLine &L, int64_t, uint32_t) { sam_emit_line(s, L); }
	static int64_t n_lines(const mm355_hits_t *H, const int32_t *qlens, int sam_flags, int64_t i) { return mm355_sam_n_lines(H, qlens, sam_flags, i); }
	static int64_t host_sum(const mm355_hits_t *, const mm355_hit_t &) { return 0; }   // (the serial sinks spell the CIGAR out)
	static int64_t out_size(int64_t n) { return n; }
};

// The host formatter of a format whose records carry the read (SamFmt; BamFmt of mm355_bam.h): the emitter run serially, once to count and
// once to write, then the format's framing if it has one.  The arguments must have passed the format's check.  line_off counts in the
// unframed text.
template <typename F> inline int mm355_rec_format_host(const mm355_hits_t *H, const char *const *qnames, const char *const *seqs, const int32_t *qlens,
                                                       const char *const *quals, const int32_t *rep_len, const PafNames &pn, int sam_flags, mm355_text_t **out,
                                                       const RecAux &ax = RecAux())
{
	*out = 0;
	const SamNames nm(pn);
	std::vector<int64_t> off, first((size_t)H->n_reads + 1);
	int64_t tot = 0;
	for (int64_t i = 0; i < H->n_reads; ++i) {
		first[i] = (int64_t)off.size();
		const int64_t nl = F::n_lines(H, qlens, sam_flags, i);
		if (nl == 0) continue;
		const SamRead R = mm355_sam_read_of(H, i, qnames, seqs, qlens, quals, rep_len, nm, sam_flags, ax);
		for (int64_t j = 0; j < nl; ++j) {
			typename F::HostCount cs;
			F::emit(cs, SamLine{ &R, R.n_rows? (int32_t)j : -1 }, R.n_rows? F::host_sum(H, R.rows[j]) : 0, 0);
			if (cs.n > F::MAX_RECORD) return MM355_EINVAL;
			off.push_back(tot); tot += cs.n;
		}
	}
	first[H->n_reads] = (int64_t)off.size();
	off.push_back(tot);
	std::vector<char> raw(F::FRAMED? (size_t)tot + 1 : 0);
	mm355_text_t *T = mm355_text_alloc(H->n_reads, (int64_t)off.size() - 1, F::out_size(tot));
	if (T == 0) return MM355_ENOMEM;
	char *dst = F::FRAMED? raw.data() : T->text;
	for (int64_t i = 0; i <= H->n_reads; ++i) T->line_off[i] = off[first[i]];
	for (int64_t i = 0; i < H->n_reads; ++i) {
		if (first[i + 1] == first[i]) continue;
		const SamRead R = mm355_sam_read_of(H, i, qnames, seqs, qlens, quals, rep_len, nm, sam_flags, ax);
		for (int64_t l = first[i]; l < first[i + 1]; ++l) {
			typename F::HostWrite ws(dst + off[l]);
			const int32_t j = (int32_t)(l - first[i]);
			F::emit(ws, SamLine{ &R, R.n_rows? j : -1 }, R.n_rows? F::host_sum(H, R.rows[j]) : 0, (uint32_t)(off[l + 1] - off[l] - 4));
			if (ws.n != off[l + 1] - off[l]) { mm355_free_text_host(T); return MM355_EINVAL; }   // the two passes disagree: a bug, never a short record
		}
	}
	if constexpr (F::FRAMED) { T->n_text = F::frame_host(raw.data(), tot, T->text); T->text[T->n_text] = 0; }   // (a deflating frame writes less than out_size(tot))
	*out = T;
	return 0;
}

inline int mm355_sam_format_host(const mm355_hits_t *H, const char *const *qnames, const char *const *seqs, const int32_t *qlens, const char *const *quals,
                                 const int32_t *rep_len, const PafNames &pn, int sam_flags, mm355_text_t **out)
{
	return mm355_rec_format_host<SamFmt>(H, qnames, seqs, qlens, quals, rep_len, pn, sam_flags, out);
}
