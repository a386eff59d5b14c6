// mm355_paf.h -- the PAF line of one hit, stated once: mappy_rs.paf_line (format.c::mm_write_paf + write_tags) byte for byte.
// One emitter, templated on a sink: a counting sink and a writing sink run the same code, so the length pass and the write pass of the
// device formatter (mm355_recdev.h, instantiated with PafFmt) cannot disagree, and the host formatter below is that emitter run serially --
// the readable statement.
// Plain C++ that also compiles as device code (tests/host_harness/paf_host.cpp builds it with g++ alone).
//
// A sink has: ch(c) one byte; bytes(p, n) a run of bytes that exists in memory already (names, cs, MD); cigar(w, n) the text of n packed
// CIGAR words (len<<4 | op).  The serial sinks spell the last two out; the device sinks note them down for the whole wave.
#pragma once
#include <stdint.h>
#include "../../include/mm355.h"
#include "mm355_core.h"

// ---- integers
MM_HD int paf_digits(uint32_t v)
{
	return v < 10u? 1 : v < 100u? 2 : v < 1000u? 3 : v < 10000u? 4 : v < 100000u? 5 : v < 1000000u? 6 : v < 10000000u? 7 : v < 100000000u? 8 : v < 1000000000u? 9 : 10;
}
template <typename S> MM_HD void paf_u64(S &s, uint64_t v)
{
	if (v <= 0xffffffffu) {           // every field but a string length: 32-bit arithmetic (a 64-bit division is a subroutine on the device)
		const uint32_t u = (uint32_t)v;
		uint32_t p = 1;
		for (int d = paf_digits(u); d > 1; --d) p *= 10;
		for (; p > 0; p /= 10) s.ch((char)('0' + u / p % 10));
		return;
	}
	uint64_t p = 1;
	while (v / p >= 10) p *= 10;      // (v / p, not p * 10 <= v: no overflow at 2^64 - 1)
	for (; p > 0; p /= 10) s.ch((char)('0' + v / p % 10));
}
template <typename S> MM_HD void paf_i64(S &s, int64_t v)
{
	if (v < 0) { s.ch('-'); paf_u64(s, (uint64_t)0 - (uint64_t)v); }
	else paf_u64(s, (uint64_t)v);
}
template <typename S> MM_HD void paf_lit(S &s, const char *z) { for (; *z; ++z) s.ch(*z); }

// ---- C's "%.4f" of a double, in integers ("0" for exactly zero, as mappy_rs._f4).  x = m * 2^-sh with the 53-bit mantissa m, so
// x * 10000 = (m * 10000) >> sh: the product is below 2^67 and exact in 128 bits, the quotient is rounded half to even on the exact
// remainder.  sh runs from 3 (just under 2^50) to 1074 (denormals).  From sh = 68 on the product is below half a unit and the result is 0;
// the code takes that branch from sh = 120 on, which is what keeps the 128-bit shift count in range, and computes the (zero) quotient in
// between.  NaN prints "nan"; values of 2^50 and more print "inf", which is not what printf does with a large finite value: the fields
// this serves are a divergence in [0, 1] and 1 - mlen / n with 32-bit integers, at most 2^31 + 1 in magnitude.
// The number behind the text: what x is (PAF_F4_ZERO: exactly zero, "0"; PAF_F4_NAN; PAF_F4_INF; PAF_F4_NUM), its sign bit, and for a
// number q = |x| * 10000 rounded half to even, so that the text is q / 10000 "." and four digits of q % 10000 (the BAM writer stores q / 10000.0)
enum { PAF_F4_ZERO, PAF_F4_NAN, PAF_F4_INF, PAF_F4_NUM };
MM_HD int paf_f4_scaled(double x, bool *neg, uint64_t *q_out)
{
	union { double d; uint64_t u; } z; z.d = x;
	const int e = (int)(z.u >> 52 & 0x7ff);
	const uint64_t frac = z.u & ((1ULL << 52) - 1);
	*neg = false; *q_out = 0;
	if (e == 0 && frac == 0) return PAF_F4_ZERO;
	if (e == 0x7ff && frac) return PAF_F4_NAN;
	*neg = z.u >> 63 != 0;
	if (e >= 1023 + 50) return PAF_F4_INF;
	const uint64_t m = e? frac | 1ULL << 52 : frac;
	const int sh = e? 1075 - e : 1074;                      // 3 .. 1074
	uint64_t q = 0;
	if (sh < 120) {
		const unsigned __int128 p = (unsigned __int128)m * 10000u, one = 1;
		const unsigned __int128 rem = p & ((one << sh) - 1), half = one << (sh - 1);
		q = (uint64_t)(p >> sh);
		if (rem > half || (rem == half && (q & 1))) ++q;
	}
	*q_out = q;
	return PAF_F4_NUM;
}
template <typename S> MM_HD void paf_f4(S &s, double x)
{
	bool neg; uint64_t q;
	const int kind = paf_f4_scaled(x, &neg, &q);
	if (kind == PAF_F4_ZERO) { s.ch('0'); return; }
	if (kind == PAF_F4_NAN) { paf_lit(s, "nan"); return; }
	if (neg) s.ch('-');
	if (kind == PAF_F4_INF) { paf_lit(s, "inf"); return; }
	paf_u64(s, q / 10000);
	s.ch('.');
	const uint32_t f = (uint32_t)(q % 10000);
	s.ch((char)('0' + f / 1000)); s.ch((char)('0' + f / 100 % 10)); s.ch((char)('0' + f / 10 % 10)); s.ch((char)('0' + f % 10));
}

// ---- CIGAR words
MM_HD char paf_cigar_op(uint32_t w) { return (w & 0xf) <= 8? "MIDNSHP=X"[w & 0xf] : '?'; }
MM_HD int paf_cigar_width(uint32_t w) { return paf_digits(w >> 4) + 1; }
// the query name as the line prints it: up to its first space or tab
MM_HD int64_t paf_qname_len(const char *nm) { int64_t l = 0; while (nm[l] && nm[l] != ' ' && nm[l] != '\t') ++l; return l; }

// ---- what one line is made from.  qname / tname: the bytes to print (an unnamed read: "*", 1)
struct PafLine {
	const mm355_hit_t *h; const mm355_tags_t *t;
	const char *qname; int64_t qname_len; int32_t qlen;
	const char *tname; int64_t tname_len;
	const uint32_t *cigar;   // the batch's CIGAR words (h->cigar_off counts from here)
	const char *str;         // the batch's string arena
	bool has_cigar;          // the batch was mapped with MM_F_CIGAR
};

template <typename S> MM_HD void paf_tag_i(S &s, const char *tag, int64_t v) { paf_lit(s, tag); paf_i64(s, v); }
// gap-compressed divergence (de): this order, in double
MM_HD double paf_de(const mm355_hit_t &h, const mm355_tags_t &t)
{
	const double den = (double)((int64_t)h.block_len + t.n_ambi - t.n_gap + t.n_gapo);
	const double r = (double)h.match_len / den;
	return 1.0 - r;
}

// the tag block PAF and SAM share (format.c::write_tags up to zd): with a CIGAR NM ms AS nn; tp cm s1, s2 on primaries; de with a CIGAR,
// otherwise dv when it was estimated; zd on split regions
template <typename S> MM_HD void paf_emit_tags(S &s, const mm355_hit_t &h, const mm355_tags_t &t, bool has_cigar)
{
	if (has_cigar) {
		paf_tag_i(s, "\tNM:i:", h.NM); paf_tag_i(s, "\tms:i:", h.dp_max); paf_tag_i(s, "\tAS:i:", h.dp_score); paf_tag_i(s, "\tnn:i:", t.n_ambi);
	}
	const bool inv = (t.flags & MM355_TAG_INV) != 0, pri = h.is_primary != 0;
	paf_lit(s, "\ttp:A:"); s.ch(pri? (inv? 'I' : 'P') : (inv? 'i' : 'S'));
	paf_tag_i(s, "\tcm:i:", h.cnt);
	paf_tag_i(s, "\ts1:i:", t.score);
	if (pri) paf_tag_i(s, "\ts2:i:", h.subsc);
	if (has_cigar) { paf_lit(s, "\tde:f:"); paf_f4(s, paf_de(h, t)); }
	else if (t.div >= 0.0f && t.div <= 1.0f) { paf_lit(s, "\tdv:f:"); paf_f4(s, (double)t.div); }
	const uint32_t zd = t.flags >> MM355_TAG_SPLIT_SHIFT & 3;
	if (zd) paf_tag_i(s, "\tzd:i:", zd);
}

template <typename S> MM_HD void paf_emit_line(S &s, const PafLine &L)
{
	const mm355_hit_t &h = *L.h; const mm355_tags_t &t = *L.t;
	s.bytes(L.qname, L.qname_len);
	s.ch('\t'); paf_i64(s, L.qlen);
	s.ch('\t'); paf_i64(s, h.query_start);
	s.ch('\t'); paf_i64(s, h.query_end);
	s.ch('\t'); s.ch(h.strand > 0? '+' : '-');
	s.ch('\t'); s.bytes(L.tname, L.tname_len);
	s.ch('\t'); paf_i64(s, h.target_len);
	s.ch('\t'); paf_i64(s, h.target_start);
	s.ch('\t'); paf_i64(s, h.target_end);
	s.ch('\t'); paf_i64(s, h.match_len);
	s.ch('\t'); paf_i64(s, h.block_len);
	s.ch('\t'); paf_u64(s, h.mapq);
	paf_emit_tags(s, h, t, L.has_cigar);
	paf_tag_i(s, "\trl:i:", t.rep_len);
	if (L.has_cigar) {
		paf_lit(s, "\tcg:Z:"); s.cigar(L.cigar + h.cigar_off, h.n_cigar);
		if (h.cs_len >= 0) { paf_lit(s, "\tcs:Z:"); s.bytes(L.str + h.cs_off, h.cs_len); }
		if (h.md_len >= 0) { paf_lit(s, "\tMD:Z:"); s.bytes(L.str + h.md_off, h.md_len); }
	}
	s.ch('\n');
}

// ---- the format as the shared record writer sees it (mm355_recdev.h): compile-time facts only
struct PafFmt {
	typedef PafLine Line;
	enum { RUNS = 4 };                                                 // runs of a line the wave copies: qname, tname, cs, MD
	static constexpr bool WAVE_CIGAR = true, TILED = false;            // the CIGAR is text, which the wave writes; a line has no SEQ and QUAL
	static constexpr int64_t MIN_RECORD = 1, MAX_LINES = INT32_MAX;    // every line has its newline at least; what the upload takes
	static MM_HD int64_t word_term(uint32_t w) { return paf_cigar_width(w); }   // summed over a row's CIGAR words: the length of the cg:Z: text
	template <typename S> static MM_HD void emit(S &s, const PafLine &L, int64_t, uint32_t) { paf_emit_line(s, L); }
	// how many lines read i writes: its hits (H->status may be absent)
	static int64_t n_lines(const mm355_hits_t *H, const int32_t *, int, int64_t i) { return H->hit_off[i + 1] - H->hit_off[i]; }
};

// ---- the serial sinks
struct PafCountSink {
	int64_t n = 0;
	MM_HD void ch(char) { ++n; }
	MM_HD void bytes(const char *, int64_t l) { n += l; }
	MM_HD void cigar(const uint32_t *w, int64_t k) { for (int64_t i = 0; i < k; ++i) n += paf_cigar_width(w[i]); }
};
struct PafWriteSink {
	char *p; int64_t n = 0;
	MM_HD explicit PafWriteSink(char *p_) : p(p_) {}
	MM_HD void ch(char c) { p[n++] = c; }
	MM_HD void bytes(const char *b, int64_t l) { for (int64_t i = 0; i < l; ++i) p[n++] = b[i]; }
	MM_HD void cigar(const uint32_t *w, int64_t k) { for (int64_t i = 0; i < k; ++i) { paf_u64(*this, w[i] >> 4); ch(paf_cigar_op(w[i])); } }
};

// ------------------------------------------------------------------ host side
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

// what a formatter needs of the index: the contig names
struct PafNames { const std::string *names; uint32_t n_seq; };

// every offset of every row lies inside its arena, every rid names a contig, hit_off ascends, de has a divisor: checked once, before either formatter reads a row
inline int mm355_paf_check(const mm355_hits_t *H, uint32_t n_seq, bool has_cigar)
{
	if (H == 0 || H->tags == 0 || H->n_reads < 0 || H->n_hits < 0 || H->hit_off == 0) return MM355_EINVAL;
	if (H->hit_off[0] != 0 || H->hit_off[H->n_reads] != H->n_hits) return MM355_EINVAL;
	for (int64_t i = 0; i < H->n_reads; ++i) if (H->hit_off[i] > H->hit_off[i + 1]) return MM355_EINVAL;
	for (int64_t k = 0; k < H->n_hits; ++k) {
		const mm355_hit_t &h = H->hits[k];
		if (h.rid < 0 || (uint32_t)h.rid >= n_seq) return MM355_EINVAL;
		if (!has_cigar) continue;
		if (h.n_cigar < 0 || h.cigar_off < 0 || h.cigar_off > H->n_cigar - h.n_cigar) return MM355_EINVAL;
		if ((int64_t)h.block_len + H->tags[k].n_ambi - H->tags[k].n_gap + H->tags[k].n_gapo == 0) return MM355_EINVAL;   // de = 1 - mlen / 0: paf_line raises there
		if (h.cs_len >= 0 && (h.cs_off < 0 || h.cs_off > H->n_str - h.cs_len)) return MM355_EINVAL;
		if (h.md_len >= 0 && (h.md_off < 0 || h.md_off > H->n_str - h.md_len)) return MM355_EINVAL;
	}
	return 0;
}

inline void mm355_free_text_host(mm355_text_t *t) { if (t) { free(t->line_off); free(t->text); free(t); } }

// the result record with line_off[] of n_reads + 1 words and n_text bytes of text (one spare byte, so that no size is zero)
inline mm355_text_t *mm355_text_alloc(int64_t n_reads, int64_t n_lines, int64_t n_text)
{
	mm355_text_t *T = (mm355_text_t*)calloc(1, sizeof(mm355_text_t));
	if (T == 0) return 0;
	T->n_reads = n_reads; T->n_lines = n_lines; T->n_text = n_text;
	T->line_off = (int64_t*)malloc((size_t)(n_reads + 1) * 8);
	T->text = (char*)malloc((size_t)n_text + 1);
	if (T->line_off == 0 || T->text == 0) { mm355_free_text_host(T); return 0; }
	T->text[n_text] = 0;
	return T;
}

inline PafLine mm355_paf_line_of(const mm355_hits_t *H, int64_t k, const char *qname, int32_t qlen, const PafNames &nm, bool has_cigar)
{
	PafLine L;
	L.h = H->hits + k; L.t = H->tags + k;
	L.qname = qname? qname : "*"; L.qname_len = qname? paf_qname_len(qname) : 1; L.qlen = qlen;
	const std::string &tn = nm.names[L.h->rid];
	L.tname = tn.data(); L.tname_len = (int64_t)tn.size();
	L.cigar = H->cigar; L.str = H->str; L.has_cigar = has_cigar;
	return L;
}

// The host formatter: the emitter run serially, once to count and once to write.  H must have passed mm355_paf_check.
inline int mm355_paf_format_host(const mm355_hits_t *H, const char *const *qnames, const int32_t *qlens, const PafNames &nm, bool has_cigar, mm355_text_t **out)
{
	*out = 0;
	std::vector<int64_t> off((size_t)H->n_hits + 1);
	int64_t tot = 0;
	for (int64_t i = 0; i < H->n_reads; ++i)
		for (int64_t k = H->hit_off[i]; k < H->hit_off[i + 1]; ++k) {
			PafCountSink cs;
			paf_emit_line(cs, mm355_paf_line_of(H, k, qnames? qnames[i] : 0, qlens[i], nm, has_cigar));
			off[k] = tot; tot += cs.n;
		}
	off[H->n_hits] = tot;
	mm355_text_t *T = mm355_text_alloc(H->n_reads, H->n_hits, tot);
	if (T == 0) return MM355_ENOMEM;
	for (int64_t i = 0; i <= H->n_reads; ++i) T->line_off[i] = off[H->hit_off[i]];
	for (int64_t i = 0; i < H->n_reads; ++i)
		for (int64_t k = H->hit_off[i]; k < H->hit_off[i + 1]; ++k) {
			PafWriteSink ws(T->text + off[k]);
			paf_emit_line(ws, mm355_paf_line_of(H, k, qnames? qnames[i] : 0, qlens[i], nm, has_cigar));
			if (ws.n != off[k + 1] - off[k]) { mm355_free_text_host(T); return MM355_EINVAL; }   // the two passes disagree: a bug, never a short line
		}
	*out = T;
	return 0;
}
