// mm355_bam.h -- the BAM records of one read and their BGZF framing, stated once (the rule is written out in include/mm355.h): a record is the
// BAM encoding of the SAM line sam_emit_line writes for the same row under the same sam_flags.  One emitter, templated on a sink, as
// mm355_sam.h: the counting sink and the writing sinks run the same code, and the host formatter (mm355_bam_format_host) is that emitter
// run serially plus host framing with zlib's crc32.  Plain C++ that also compiles as device code (tests/host_harness/bam_host.cpp builds it with g++ alone).
//
// A sink has binary primitives: ch(c) / u8(v) one byte, u16(v) and u32(v) little-endian, bytes(p, n) a run that exists in memory (names,
// cs, MD), cigar(w, n) n packed CIGAR words as they are (len<<4 | op is BAM's own word), seq4(p, n, rev) n bases packed two per byte,
// qual(p, n, rev) n quality bytes minus 33, fill(n) n bytes of 0xFF, aux(p, n) n bytes of copied aux tags as they are.  SEQ, QUAL and the
// copied tags are the bulk of a record: the device sinks only note them down, and a kernel of its own writes them (mm355_bam.hip::k_bam_bulk).
#pragma once
#include <zlib.h>
#include <algorithm>
#include "mm355_sam.h"

// ---- BGZF with stored deflate blocks: the stream is cut every BGZF_PAYLOAD bytes (htslib's block payload); a block is the 18-byte gzip
// header with the BC extra field, the 5-byte header of one stored deflate block, the payload, CRC-32 and ISIZE
#define BGZF_PAYLOAD 0xff00
#define BGZF_HEAD 23
#define BGZF_EXTRA 31
MM_HD int64_t bgzf_blocks(int64_t n) { return (n + BGZF_PAYLOAD - 1) / BGZF_PAYLOAD; }
MM_HD int64_t bgzf_size(int64_t n) { return n + bgzf_blocks(n) * BGZF_EXTRA; }
// byte i (0 .. 22) of the header of a block with len payload bytes
MM_HD unsigned char bgzf_head_byte(int i, uint32_t len)
{
	const uint32_t bsize = len + BGZF_EXTRA - 1, nlen = ~len & 0xffffu;
	switch (i) {
	case 0: return 0x1f; case 1: return 0x8b; case 2: return 8; case 3: return 4;               // magic, deflate, FEXTRA
	case 9: return 0xff; case 10: return 6; case 12: return 'B'; case 13: return 'C'; case 14: return 2;   // OS unknown, XLEN 6, BC, SLEN 2
	case 16: return (unsigned char)(bsize & 0xff); case 17: return (unsigned char)(bsize >> 8);
	case 18: return 1;                                                                         // BFINAL, BTYPE 00: stored
	case 19: return (unsigned char)(len & 0xff); case 20: return (unsigned char)(len >> 8);
	case 21: return (unsigned char)(nlen & 0xff); case 22: return (unsigned char)(nlen >> 8);
	default: return 0;                                                                         // MTIME, XFL, the high bytes of XLEN and SLEN
	}
}

// ---- CRC-32 of a block by BGZF_LANES lanes that never read each other's bytes (mm355_bam.hip::k_bgzf_frame; tests/host_harness/bam_host.cpp
// runs the same functions serially against zlib).  The register update is linear over GF(2), and zero bytes leave a zero register as it
// is.  So the whole BGZF_CHUNK-byte chunks of the payload are taken to stand at the END of a message of BGZF_LANES chunks, zeros in front:
// every lane has a chunk of the same length whatever the payload's, and a chunk begins at a multiple of BGZF_CHUNK in the payload, which
// 16-byte loads can read.  A lane starts from a zero register, except the lane of the payload's first chunk, which starts from 0xffffffff;
// lanes in front of it keep zero.  Two neighbouring groups of lanes combine as reg(left) * x^(8 * bytes of the right group) + reg(right)
// (mod the CRC polynomial): the right group's length is BGZF_CHUNK << level, so eight constants serve the eight levels and no "advance by
// n" for a general n is needed.  What is left of a short last block, fewer than BGZF_CHUNK bytes, one lane adds serially to the combined
// register (every block but a stream's last is BGZF_PAYLOAD bytes, a whole number of chunks).  The CRC is the complement of the result.
#define BGZF_CHUNK 256
#define BGZF_LANES 256         // BGZF_CHUNK * (BGZF_LANES - 1) >= BGZF_PAYLOAD: lane 0 never has a chunk
#define CRC32_POLY 0xedb88320u
MM_HD uint32_t crc32_tab_entry(uint32_t i) { for (int k = 0; k < 8; ++k) i = i & 1? CRC32_POLY ^ i >> 1 : i >> 1; return i; }
// a * b mod the polynomial, bit-reflected as the register is (bit 31 is x^0)
MM_HD uint32_t crc32_mulmod(uint32_t a, uint32_t b)
{
	uint32_t p = 0;
	for (uint32_t m = 1u << 31; m; m >>= 1) {
		if (a & m) p ^= b;
		b = b & 1? b >> 1 ^ CRC32_POLY : b >> 1;
	}
	return p;
}
// x^(2^k) mod the polynomial; level l of the combine multiplies by x^(8 * (BGZF_CHUNK << l)) = crc32_x2n(11 + l)
MM_HD uint32_t crc32_x2n(int k) { uint32_t p = 1u << 30; for (int i = 0; i < k; ++i) p = crc32_mulmod(p, p); return p; }
static_assert(BGZF_CHUNK == 1 << 8 && BGZF_CHUNK * (BGZF_LANES - 1) >= BGZF_PAYLOAD && BGZF_PAYLOAD % BGZF_CHUNK == 0, "crc32_x2n(11 + level) is x^(8 * 256 << level)");
// the register of one lane after its chunk; src: the payload, 16-byte aligned; tab: the 256 entries of crc32_tab_entry
MM_HD uint32_t bgzf_lane_crc(const unsigned char *src, uint32_t len, int lane, const uint32_t *tab)
{
	const int first = BGZF_LANES - (int)(len / BGZF_CHUNK);      // the lane of the payload's first chunk (BGZF_LANES: it has none)
	if (lane < first) return 0;
	const unsigned char *p = (const unsigned char*)__builtin_assume_aligned(src + (size_t)(lane - first) * BGZF_CHUNK, 16);
	uint32_t r = lane == first? 0xffffffffu : 0u;
	for (int i = 0; i < BGZF_CHUNK; i += 16) {
		uint32_t w[4];
		memcpy(w, p + i, 16);                                    // (one 16-byte load)
		for (int k = 0; k < 4; ++k) {
			r ^= w[k];                                           // little-endian: the dword's lowest byte is the message's next
			for (int j = 0; j < 4; ++j) r = tab[r & 0xff] ^ r >> 8;
		}
	}
	return r;
}
// one level of the combine, for the lane that owns a left group (lane % (2 << level) == 0): reg[] holds a register per lane
MM_HD uint32_t bgzf_crc_level(const uint32_t *reg, int lane, int level, uint32_t x_pow) { return crc32_mulmod(x_pow, reg[lane]) ^ reg[lane + (1 << level)]; }
// the block's register from the combined one: what is left behind the whole chunks, byte by byte (a payload without a whole chunk starts here)
MM_HD uint32_t bgzf_tail_crc(const unsigned char *src, uint32_t len, uint32_t combined, const uint32_t *tab)
{
	uint32_t r = len >= BGZF_CHUNK? combined : 0xffffffffu;
	for (uint32_t i = len & ~(uint32_t)(BGZF_CHUNK - 1); i < len; ++i) r = tab[(r ^ src[i]) & 0xff] ^ r >> 8;
	return r;
}

// ---- the pieces of a record
// index in "=ACMGRSVTWYHKDBN", either case; every other byte (U and u among them) is 15
MM_HD unsigned char bam_code(unsigned char c)
{
	if (c == '=') return 0;
	switch (c & 0xdf) {           // a letter's upper case; no other byte lands on a letter
	case 'A': return 1; case 'C': return 2; case 'M': return 3; case 'G': return 4; case 'R': return 5; case 'S': return 6; case 'V': return 7;
	case 'T': return 8; case 'W': return 9; case 'Y': return 10; case 'H': return 11; case 'K': return 12; case 'D': return 13; case 'B': return 14;
	default: return 15;
	}
}
// the base as the SAM line prints it on that strand, then its code
MM_HD unsigned char bam_code_on(unsigned char c, bool rev) { return bam_code(rev? sam_comp(c) : c); }
// the SAM specification's reg2bin, in 64 bits (pos + reflen may pass 2^31)
MM_HD uint32_t bam_reg2bin(int64_t beg, int64_t end)
{
	--end;
	if (beg >> 14 == end >> 14) return (uint32_t)(((1 << 15) - 1) / 7 + (beg >> 14));
	if (beg >> 17 == end >> 17) return (uint32_t)(((1 << 12) - 1) / 7 + (beg >> 17));
	if (beg >> 20 == end >> 20) return (uint32_t)(((1 << 9) - 1) / 7 + (beg >> 20));
	if (beg >> 23 == end >> 23) return (uint32_t)(((1 << 6) - 1) / 7 + (beg >> 23));
	if (beg >> 26 == end >> 26) return (uint32_t)(((1 << 3) - 1) / 7 + (beg >> 26));
	return 0;
}
// what a CIGAR word adds to the reference length: the length of M D N = X
MM_HD int64_t bam_ref_len(uint32_t w) { return (0x18du >> (w & 0xf) & 1)? (int64_t)(w >> 4) : 0; }
// an integer tag in htslib's smallest type
template <typename S> MM_HD void bam_tag_i(S &s, char a, char b, int64_t v)
{
	s.ch(a); s.ch(b);
	if (v >= 0) {
		if (v <= 255) { s.ch('C'); s.u8((uint32_t)v); } else if (v <= 65535) { s.ch('S'); s.u16((uint32_t)v); } else { s.ch('I'); s.u32((uint32_t)v); }
	} else {
		if (v >= -128) { s.ch('c'); s.u8((uint32_t)v & 0xff); } else if (v >= -32768) { s.ch('s'); s.u16((uint32_t)v & 0xffff); } else { s.ch('i'); s.u32((uint32_t)v); }
	}
}
template <typename S> MM_HD void bam_tag_z(S &s, char a, char b, const char *p, int64_t n) { s.ch(a); s.ch(b); s.ch('Z'); s.bytes(p, n); s.u8(0); }
// the float32 a reader of the SAM text would store for a field paf_f4 printed: (float)strtod(text), from the integer behind the text
MM_HD uint32_t bam_f4_bits(double x)
{
	bool neg; uint64_t q;
	const int kind = paf_f4_scaled(x, &neg, &q);
	union { float f; uint32_t u; } z;
	if (kind == PAF_F4_ZERO) return 0;
	if (kind == PAF_F4_NAN) return 0x7fc00000u;
	if (kind == PAF_F4_INF) return neg? 0xff800000u : 0x7f800000u;
	const double d = (double)q / 10000.0;
	z.f = (float)(neg? -d : d);
	return z.u;
}

// the tag block BAM shares with the SAM line (paf_emit_tags with a CIGAR): NM ms AS nn tp cm s1 [s2] de [zd]
template <typename S> MM_HD void bam_emit_tags(S &s, const mm355_hit_t &h, const mm355_tags_t &t)
{
	bam_tag_i(s, 'N', 'M', h.NM); bam_tag_i(s, 'm', 's', h.dp_max); bam_tag_i(s, 'A', 'S', h.dp_score); bam_tag_i(s, 'n', 'n', t.n_ambi);
	const bool inv = (t.flags & MM355_TAG_INV) != 0, pri = h.is_primary != 0;
	s.ch('t'); s.ch('p'); s.ch('A'); s.ch(pri? (inv? 'I' : 'P') : (inv? 'i' : 'S'));
	bam_tag_i(s, 'c', 'm', h.cnt);
	bam_tag_i(s, 's', '1', t.score);
	if (pri) bam_tag_i(s, 's', '2', h.subsc);
	s.ch('d'); s.ch('e'); s.ch('f'); s.u32(bam_f4_bits(paf_de(h, t)));
	const uint32_t zd = t.flags >> MM355_TAG_SPLIT_SHIFT & 3;
	if (zd) bam_tag_i(s, 'z', 'd', zd);
}

// One record, block_size included.  reflen: the summed bam_ref_len of the row's words (0 for the unmapped record); block_size: the record's
// length without this word, which the counting pass gives (the counting pass itself passes anything)
template <typename S> MM_HD void bam_emit_record(S &s, const SamLine &L, int64_t reflen, uint32_t block_size)
{
	const SamRead &R = *L.R;
	s.u32(block_size);
	if (L.row < 0) {   // a read without hits
		s.u32(0xffffffffu); s.u32(0xffffffffu);
		s.u8((uint32_t)R.qname_len + 1); s.u8(0); s.u16(4680); s.u16(0); s.u16(4); s.u32((uint32_t)R.qlen);
		s.u32(0xffffffffu); s.u32(0xffffffffu); s.u32(0);
		s.bytes(R.qname, R.qname_len); s.u8(0);
		s.seq4(R.seq, R.qlen, false);
		if (R.qual) s.qual(R.qual, R.qlen, false); else s.fill(R.qlen);
		bam_tag_i(s, 'r', 'l', R.rep_len);
		if (R.aux_len > 0) s.aux(R.aux, R.aux_len);
		return;
	}
	const mm355_hit_t &h = R.rows[L.row]; const mm355_tags_t &t = R.tags[L.row];
	const bool rev = h.strand < 0, soft = (R.sam_flags & MM355_SAM_SOFTCLIP) != 0;
	const uint32_t flag = sam_flag_of(h, t);
	const uint32_t clip_op = (flag & 0x800) && !soft? 5u : 4u;   // H or S, as the line
	const uint32_t clip5 = h.n_cigar > 0? (uint32_t)(rev? R.qlen - h.query_end : h.query_start) : 0u;
	const uint32_t clip3 = h.n_cigar > 0? (uint32_t)(rev? h.query_start : R.qlen - h.query_end) : 0u;
	const int64_t n_words = (int64_t)h.n_cigar + (clip5? 1 : 0) + (clip3? 1 : 0);
	const bool lng = n_words > 65535;                            // htslib's long-CIGAR form: two place-holder words, the real ones in CG:B:I
	const char *sq = 0, *ql = 0; int32_t l_seq = 0;
	if ((flag & 0x900) == 0 || soft) { sq = R.seq; ql = R.qual; l_seq = R.qlen; }
	else if (!(flag & 0x100)) { sq = R.seq + h.query_start; ql = R.qual? R.qual + h.query_start : 0; l_seq = h.query_end - h.query_start; }
	const int64_t pos = h.target_start;
	s.u32((uint32_t)h.rid); s.u32((uint32_t)h.target_start);
	s.u8((uint32_t)R.qname_len + 1); s.u8(h.mapq); s.u16(bam_reg2bin(pos, pos + (reflen > 1? reflen : 1)) & 0xffffu);
	s.u16(lng? 2u : (uint32_t)n_words); s.u16(flag); s.u32((uint32_t)l_seq);
	s.u32(0xffffffffu); s.u32(0xffffffffu); s.u32(0);
	s.bytes(R.qname, R.qname_len); s.u8(0);
	if (lng) { s.u32((uint32_t)l_seq << 4 | 4u); s.u32((uint32_t)reflen << 4 | 3u); }
	else {
		if (clip5) s.u32(clip5 << 4 | clip_op);
		s.cigar(R.cigar + h.cigar_off, h.n_cigar);
		if (clip3) s.u32(clip3 << 4 | clip_op);
	}
	if (sq) {
		s.seq4(sq, l_seq, rev);
		if (ql) s.qual(ql, l_seq, rev); else s.fill(l_seq);
	}
	bam_emit_tags(s, h, t);
	if (h.is_primary) {
		bool any = false;
		for (int32_t j = 0; j < R.n_rows; ++j) {
			const mm355_hit_t &q = R.rows[j];
			if (j == L.row || !q.is_primary || q.n_cigar <= 0) continue;
			if (!any) { s.ch('S'); s.ch('A'); s.ch('Z'); any = true; }
			sam_emit_sa(s, R, q, R.tags[j]);
		}
		if (any) s.u8(0);
	}
	if (h.cs_len >= 0) bam_tag_z(s, 'c', 's', R.str + h.cs_off, h.cs_len);
	if (h.md_len >= 0) bam_tag_z(s, 'M', 'D', R.str + h.md_off, h.md_len);
	bam_tag_i(s, 'r', 'l', t.rep_len);
	// the read's copied tags: all of them where SEQ is the whole read, otherwise those that do not index its bases (CG stays last)
	const int32_t n_aux = (flag & 0x900) == 0 || soft? R.aux_len : R.aux_mod;
	if (n_aux > 0) s.aux(R.aux, n_aux);
	if (lng) {
		s.ch('C'); s.ch('G'); s.ch('B'); s.ch('I'); s.u32((uint32_t)n_words);
		if (clip5) s.u32(clip5 << 4 | clip_op);
		s.cigar(R.cigar + h.cigar_off, h.n_cigar);
		if (clip3) s.u32(clip3 << 4 | clip_op);
	}
}

// ---- the serial sinks
struct BamCountSink {
	int64_t n = 0;
	MM_HD void ch(char) { ++n; }
	MM_HD void u8(uint32_t) { ++n; }
	MM_HD void u16(uint32_t) { n += 2; }
	MM_HD void u32(uint32_t) { n += 4; }
	MM_HD void bytes(const char *, int64_t l) { n += l; }
	MM_HD void cigar(const uint32_t *, int64_t k) { n += 4 * k; }
	MM_HD void seq4(const char *, int64_t l, bool) { n += (l + 1) / 2; }
	MM_HD void qual(const char *, int64_t l, bool) { n += l; }
	MM_HD void fill(int64_t l) { n += l; }
	MM_HD void aux(const uint8_t *, int64_t l) { n += l; }
};
struct BamWriteSink {
	unsigned char *p; int64_t n = 0;
	MM_HD explicit BamWriteSink(char *p_) : p((unsigned char*)p_) {}
	MM_HD void ch(char c) { p[n++] = (unsigned char)c; }
	MM_HD void u8(uint32_t v) { p[n++] = (unsigned char)v; }
	MM_HD void u16(uint32_t v) { u8(v & 0xff); u8(v >> 8 & 0xff); }
	MM_HD void u32(uint32_t v) { u16(v & 0xffff); u16(v >> 16); }
	MM_HD void bytes(const char *b, int64_t l) { for (int64_t i = 0; i < l; ++i) p[n++] = (unsigned char)b[i]; }
	MM_HD void cigar(const uint32_t *w, int64_t k) { for (int64_t i = 0; i < k; ++i) u32(w[i]); }
	MM_HD void seq4(const char *b, int64_t l, bool rev)
	{
		for (int64_t i = 0; i < l; i += 2) {
			const unsigned char hi = bam_code_on((unsigned char)(rev? b[l - 1 - i] : b[i]), rev);
			const unsigned char lo = i + 1 < l? bam_code_on((unsigned char)(rev? b[l - 2 - i] : b[i + 1]), rev) : 0;
			p[n++] = (unsigned char)(hi << 4 | lo);
		}
	}
	MM_HD void qual(const char *b, int64_t l, bool rev) { for (int64_t i = 0; i < l; ++i) p[n++] = (unsigned char)((unsigned char)(rev? b[l - 1 - i] : b[i]) - 33); }
	MM_HD void fill(int64_t l) { for (int64_t i = 0; i < l; ++i) p[n++] = 0xff; }
	MM_HD void aux(const uint8_t *b, int64_t l) { memcpy(p + n, b, (size_t)l); n += l; }
};

// ------------------------------------------------------------------ host side
inline int64_t mm355_bam_reflen(const mm355_hits_t *H, const mm355_hit_t &h)
{
	int64_t r = 0;
	for (int32_t i = 0; i < h.n_cigar; ++i) r += bam_ref_len(H->cigar[h.cigar_off + i]);
	return r;
}

// everything mm355_sam_check asks, plus what a BAM record cannot hold: a mapq above 255, a printed read name of more than 254 bytes on a
// read that writes a record, a clip of 2^28 bases or more (a CIGAR word has 28 bits of length: the row's own words cannot say more)
inline int mm355_bam_check(const mm355_hits_t *H, uint32_t n_seq, bool has_cigar, const char *const *qnames, const char *const *seqs, const int32_t *qlens,
                           const int32_t *rep_len, int sam_flags)
{
	if (int rc = mm355_sam_check(H, n_seq, has_cigar, seqs, qlens, rep_len, sam_flags)) return rc;
	for (int64_t i = 0; i < H->n_reads; ++i) {
		if (mm355_sam_n_lines(H, qlens, sam_flags, i) == 0) continue;
		if (qnames && qnames[i] && paf_qname_len(qnames[i]) > 254) return MM355_EINVAL;
		for (int64_t k = H->hit_off[i]; k < H->hit_off[i + 1]; ++k) {
			const mm355_hit_t &h = H->hits[k];
			if (h.mapq > 255) return MM355_EINVAL;
			if (h.n_cigar > 0 && (h.query_start >= 1 << 28 || qlens[i] - h.query_end >= 1 << 28)) return MM355_EINVAL;
		}
	}
	return 0;
}

// n bytes framed into bgzf_size(n) bytes of stored BGZF blocks
inline void mm355_bgzf_frame_host(const char *data, int64_t n, char *out)
{
	for (int64_t at = 0; at < n; at += BGZF_PAYLOAD) {
		const uint32_t len = (uint32_t)(n - at < BGZF_PAYLOAD? n - at : BGZF_PAYLOAD);
		unsigned char *o = (unsigned char*)out + at / BGZF_PAYLOAD * (BGZF_PAYLOAD + BGZF_EXTRA);
		for (int i = 0; i < BGZF_HEAD; ++i) o[i] = bgzf_head_byte(i, len);
		memcpy(o + BGZF_HEAD, data + at, len);
		const uint32_t crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), (const Bytef*)(data + at), len);
		unsigned char *t = o + BGZF_HEAD + len;
		for (int i = 0; i < 4; ++i) { t[i] = (unsigned char)(crc >> 8 * i); t[4 + i] = (unsigned char)(len >> 8 * i); }
	}
}

// ---- the format as the shared writers see it (the host walk of mm355_sam.h; the device record writer, mm355_recdev.h)
struct BamFmt {
	typedef SamLine Line; typedef BamCountSink HostCount; typedef BamWriteSink HostWrite;
	enum { RUNS = 5, TILE_RUNS = 3 };                                  // runs of a record the wave copies: qname, the CIGAR words, cs, MD, the CG words; runs in tiles: SEQ, QUAL, copied tags
	static constexpr bool WAVE_CIGAR = false, TILED = true, FRAMED = true;   // the CIGAR is a run of words; SEQ and QUAL go in tiles; the result is the stream in BGZF blocks
	// the fixed part of a record is 36 bytes, and block_size is 32 bits; records the upload takes (the tile table has TILE_RUNS runs per record)
	static constexpr int64_t MIN_RECORD = 36, MAX_RECORD = (int64_t)UINT32_MAX + 4, MAX_LINES = INT32_MAX / TILE_RUNS;
	static MM_HD int64_t word_term(uint32_t w) { return bam_ref_len(w); }   // summed over a row's CIGAR words: the reference length (the bin needs it)
	template <typename S> static MM_HD void emit(S &s, const SamLine &L, int64_t reflen, uint32_t block_size) { bam_emit_record(s, L, reflen, block_size); }
	static int64_t n_lines(const mm355_hits_t *H, const int32_t *qlens, int sam_flags, int64_t i) { return mm355_sam_n_lines(H, qlens, sam_flags, i); }
	static int64_t host_sum(const mm355_hits_t *H, const mm355_hit_t &h) { return mm355_bam_reflen(H, h); }
	static int64_t out_size(int64_t n) { return bgzf_size(n); }
	static int64_t frame_host(const char *raw, int64_t n, char *out) { mm355_bgzf_frame_host(raw, n, out); return bgzf_size(n); }   // the bytes written: out_size(n) at most
};

// line_off counts in the unframed stream of records
inline int mm355_bam_format_host(const mm355_hits_t *H, const char *const *qnames, const char *const *seqs, const int32_t *qlens, const char *const *quals,
                                 const int32_t *rep_len, const PafNames &pn, int sam_flags, mm355_text_t **out, const RecAux &ax = RecAux())
{
	return mm355_rec_format_host<BamFmt>(H, qnames, seqs, qlens, quals, rep_len, pn, sam_flags, out, ax);
}

// the same with copied aux tags, and what they add: a negative length, aux[i] == NULL with a positive length, aux_mod outside [0, aux_len],
// and a record that would pass MAX_RECORD with them.  A sum of the read's lengths that is above any of its records decides for every
// read a file will ever hold; only a read whose sum passes the limit is counted record by record (the counting sink reads lengths, never
// a byte of a read or a tag), so the formatter's own counting pass is not run twice
inline int mm355_bam_check_aux(const mm355_hits_t *H, const PafNames &pn, bool has_cigar, const char *const *qnames, const char *const *seqs, const int32_t *qlens,
                               const int32_t *rep_len, int sam_flags, const RecAux &ax)
{
	if (int rc = mm355_bam_check(H, pn.n_seq, has_cigar, qnames, seqs, qlens, rep_len, sam_flags)) return rc;
	if (ax.aux == 0) return 0;
	if (ax.len == 0 || ax.mod == 0) return MM355_EINVAL;
	bool any = false;
	for (int64_t i = 0; i < H->n_reads; ++i) {
		if (ax.len[i] < 0 || (ax.len[i] > 0 && ax.aux[i] == 0) || ax.mod[i] < 0 || ax.mod[i] > ax.len[i]) return MM355_EINVAL;
		any = any || ax.len[i] > 0;
	}
	if (!any) return 0;
	int64_t name_max = 0;
	for (uint32_t k = 0; k < pn.n_seq; ++k) name_max = std::max<int64_t>(name_max, (int64_t)pn.names[k].size());
	for (int64_t i = 0; i < H->n_reads; ++i) {
		const int64_t nl = ax.len[i] > 0? mm355_sam_n_lines(H, qlens, sam_flags, i) : 0;
		if (nl == 0) continue;
		// above every record of the read: the fixed part, name and scalar tags (1024), SEQ and QUAL, the tags, and per row its words
		// (twice: CG), its strings and its SA entry (a name and less than 128 bytes of numbers and letters)
		int64_t bound = 1024 + 2 * (int64_t)qlens[i] + ax.len[i];
		for (int64_t k = H->hit_off[i]; k < H->hit_off[i + 1]; ++k) {
			const mm355_hit_t &h = H->hits[k];
			bound += 8 * ((int64_t)h.n_cigar + 2) + (h.cs_len > 0? h.cs_len : 0) + (h.md_len > 0? h.md_len : 0) + name_max + 128;
		}
		if (bound <= BamFmt::MAX_RECORD) continue;
		const SamNames nm(pn);
		const SamRead R = mm355_sam_read_of(H, i, qnames, seqs, qlens, 0, rep_len, nm, sam_flags, ax);
		for (int64_t j = 0; j < nl; ++j) {
			BamCountSink cs;
			bam_emit_record(cs, SamLine{ &R, R.n_rows? (int32_t)j : -1 }, 0, 0);   // (the reference length decides the bin, not the size)
			if (cs.n > BamFmt::MAX_RECORD) return MM355_EINVAL;
		}
	}
	return 0;
}

// mm355_bgzf_wrap on the host
inline int mm355_bgzf_wrap_host(const void *data, int64_t n, mm355_text_t **out)
{
	mm355_text_t *T = mm355_text_alloc(0, bgzf_blocks(n), bgzf_size(n));
	if (T == 0) return MM355_ENOMEM;
	T->line_off[0] = 0;
	mm355_bgzf_frame_host((const char*)data, n, T->text);
	*out = T;
	return 0;
}
