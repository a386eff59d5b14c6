// mm355_deflate.h -- one BGZF payload (1 .. BGZF_PAYLOAD bytes) as one RFC 1951 dynamic-Huffman block, stated once: the functions the kernel
// calls with a lane number (mm355_bam.hip::k_bgzf_deflate, 256 lanes and barriers between the steps) are the functions the host runs in
// loops over the lanes (dfl_block_host below; tests/host_harness/deflate_host.cpp builds it with g++ alone), and both give the same bytes.
// The steps, each independent of the order in which the lanes run:
//   candidates  positions are taken in rounds of DFL_ROUND.  Position p reads table[hash of its 4 bytes], which holds (plus one) the largest
//               position of any EARLIER round with that hash, and notes it down in scr[p]; after a barrier every position of the round
//               raises its entry to itself (an atomic maximum).  A position with fewer than 4 bytes behind it has no candidate.
//   parse       the payload is DFL_SEGS segments of DFL_SEG bytes, a lane each.  Greedy: at p the candidate is extended byte by byte, to at
//               most 258 bytes and never past the segment's end; 4 bytes or more (3 within 4096) are a match, anything else a literal.  A
//               candidate lies anywhere in front of p within 32768 bytes, never before the payload's first byte.  The tokens go to
//               scr[segment start ...] (token k of a segment is written after scr[p], p >= start + k, was read) and into the histograms.
//   codes       the used symbols ranked by (count, symbol) -- a total order, so any sort gives the same -- then on one lane the in-place
//               two-queue merge of Moffat and Katajainen on the sorted counts, the lengths cut at 15 bits (7 for the code-length code) by
//               moving leaves down until the Kraft sum is one, lengths dealt out by rank, canonical codes bit-reversed for the stream.
//               The header spells every length out (no symbols 16 - 18).  No match at all: one distance code of length 0; one distance
//               symbol: one code of one bit (RFC 1951 3.2.7).
//   bits        per segment the bits of its tokens, an exclusive scan, and every lane ORs its codes into the block at its bit offset.
// A payload whose stream would not be shorter than its stored form (len + 5 bytes) is written stored, exactly as mm355_bgzf_frame_host and
// k_bgzf_frame write it.
#pragma once
#include <algorithm>
#include "mm355_bam.h"

#define DFL_ROUND 256
#define DFL_SEGS 256
#define DFL_SEG 255
#define DFL_HASH_BITS 14
#define DFL_MAX_MATCH 258
#define DFL_MAX_DIST 32768
#define DFL_TOO_FAR 4096            // a match of 3 bytes farther away costs more than its literals
#define DFL_N_LL 286
#define DFL_N_D 30
#define DFL_N_CL 19
#define DFL_EOB 256
#define DFL_TOK_MATCH 0x80000000u   // a token: a literal's byte, or this | (length - 3) << 16 | (distance - 1)
#define DFL_BUF_WORDS (1 << DFL_HASH_BITS)   // the hash table, and after the parse the block being built: 64 KB
#define DFL_GZ_HEAD 18              // the gzip header with the BC field; the deflate stream follows
static_assert(DFL_SEGS * DFL_SEG == BGZF_PAYLOAD && DFL_ROUND * 255 == BGZF_PAYLOAD, "a lane per segment, a lane per position of a round");
static_assert(DFL_BUF_WORDS * 4 >= BGZF_PAYLOAD + BGZF_EXTRA + 16, "a block no longer than its stored form fits, with the last 64-bit flush");

#if defined(__HIP_DEVICE_COMPILE__)
#define DFL_RAISE(p, v) atomicMax(p, v)
#define DFL_ADD(p, v) atomicAdd(p, v)
#define DFL_OR(p, v) atomicOr(p, v)
#else
#define DFL_RAISE(p, v) (void)(*(p) = *(p) > (v)? *(p) : (v))
#define DFL_ADD(p, v) (void)(*(p) += (v))
#define DFL_OR(p, v) (void)(*(p) |= (v))
#endif

// what a block's lanes share besides the 64-KB buffer: histograms, codes (code | length << 16), the sort, the segments' token and bit counts
struct DflWork {
	uint32_t ll_f[DFL_N_LL + 2], d_f[DFL_N_D + 2], cl_f[DFL_N_CL + 1];
	uint32_t ll_cw[DFL_N_LL + 2], d_cw[DFL_N_D + 2], cl_cw[DFL_N_CL + 1];
	uint32_t a[DFL_N_LL + 2];                      // the merge's work array
	uint16_t ll_sorted[DFL_N_LL + 2], d_sorted[DFL_N_D + 2], cl_sorted[DFL_N_CL + 1];
	uint32_t n_tok[DFL_SEGS], seg_bits[DFL_SEGS];  // seg_bits: the bits of a segment's tokens, then (scanned) the bit offset of its first
	uint32_t n_ll, n_d, n_cl, head_bits, n_bytes;  // HLIT, HDIST, HCLEN as counts; bits of the block header; bytes of the deflate stream
};

MM_HD uint32_t dfl_word(const unsigned char *s, uint32_t p) { return (uint32_t)s[p] | (uint32_t)s[p + 1] << 8 | (uint32_t)s[p + 2] << 16 | (uint32_t)s[p + 3] << 24; }
MM_HD uint32_t dfl_hash(uint32_t v) { return v * 2654435761u >> (32 - DFL_HASH_BITS); }

// ---- candidates: a round for the lane of position p -- its hash plus one (0: fewer than 4 bytes, nothing to look up or raise), which needs no
// table, then the two halves with a barrier between them
MM_HD uint32_t dfl_hash1(const unsigned char *src, uint32_t len, uint32_t p) { return p + 4 <= len? dfl_hash(dfl_word(src, p)) + 1 : 0; }
MM_HD void dfl_round_read(uint32_t p, uint32_t len, uint32_t h1, const uint32_t *table, uint32_t *scr) { if (p < len) scr[p] = h1? table[h1 - 1] : 0; }
MM_HD void dfl_round_raise(uint32_t p, uint32_t h1, uint32_t *table) { if (h1) DFL_RAISE(&table[h1 - 1], p + 1); }

// ---- symbols: length 3 .. 258 and distance 1 .. 32768 as symbol, count of extra bits and their value
MM_HD void dfl_len_sym(uint32_t l, uint32_t *sym, uint32_t *eb, uint32_t *ev)
{
	const uint32_t x = l - 3;
	if (l == DFL_MAX_MATCH) { *sym = 285; *eb = 0; *ev = 0; }
	else if (x < 8) { *sym = 257 + x; *eb = 0; *ev = 0; }
	else { const uint32_t e = 29 - (uint32_t)__builtin_clz(x); *eb = e; *sym = 261 + 4 * e + (x >> e & 3); *ev = x & ((1u << e) - 1); }
}
MM_HD void dfl_dist_sym(uint32_t d, uint32_t *sym, uint32_t *eb, uint32_t *ev)
{
	const uint32_t x = d - 1;
	if (x < 4) { *sym = x; *eb = 0; *ev = 0; }
	else { const uint32_t hb = 31 - (uint32_t)__builtin_clz(x), e = hb - 1; *eb = e; *sym = 2 * hb + (x >> e & 1); *ev = x & ((1u << e) - 1); }
}

// ---- parse: the tokens of segment `seg` into scr[seg * DFL_SEG ...] and the histograms; returns how many
MM_HD uint32_t dfl_parse(const unsigned char *src, uint32_t len, uint32_t seg, uint32_t *scr, uint32_t *ll_f, uint32_t *d_f)
{
	const uint32_t s0 = seg * DFL_SEG;
	if (s0 >= len) return 0;
	const uint32_t s1 = s0 + DFL_SEG < len? s0 + DFL_SEG : len;
	uint32_t k = 0;
	for (uint32_t p = s0; p < s1; ) {
		const uint32_t c = scr[p];
		uint32_t m = 0, dist = 0;
		if (c) {
			const uint32_t q = c - 1;
			dist = p - q;
			if (dist <= DFL_MAX_DIST) {
				const uint32_t lim = s1 - p < DFL_MAX_MATCH? s1 - p : DFL_MAX_MATCH;
				while (m < lim && src[q + m] == src[p + m]) ++m;
			}
		}
		if (m >= 4 || (m == 3 && dist <= DFL_TOO_FAR)) {
			uint32_t sym, eb, ev;
			dfl_len_sym(m, &sym, &eb, &ev); DFL_ADD(&ll_f[sym], 1u);
			dfl_dist_sym(dist, &sym, &eb, &ev); DFL_ADD(&d_f[sym], 1u);
			scr[s0 + k++] = DFL_TOK_MATCH | (m - 3) << 16 | (dist - 1);
			p += m;
		} else {
			DFL_ADD(&ll_f[src[p]], 1u);
			scr[s0 + k++] = src[p];
			++p;
		}
	}
	return k;
}

// ---- codes
// where symbol s stands among the used ones of f[0 .. n), by (count, symbol)
MM_HD void dfl_rank(const uint32_t *f, int n, int s, uint16_t *sorted)
{
	if (f[s] == 0) return;
	int r = 0;
	for (int t = 0; t < n; ++t) r += f[t] != 0 && (f[t] < f[s] || (f[t] == f[s] && t < s));
	sorted[r] = (uint16_t)s;
}
// the lengths of a code of at most max_bits for the used symbols (sorted[] from dfl_rank), and the canonical codes: cw[s] = the code, its
// first bit lowest, | length << 16; a[]: n words of work
MM_HD void dfl_make_code(const uint32_t *f, int n, int max_bits, const uint16_t *sorted, uint32_t *a, uint32_t *cw)
{
	int m = 0;
	for (int s = 0; s < n; ++s) { cw[s] = 0; m += f[s] != 0; }
	if (m == 0) return;
	if (m == 1) { cw[sorted[0]] = 1u << 16; return; }          // one code of one bit: 0
	for (int i = 0; i < m; ++i) a[i] = f[sorted[i]];
	// Moffat and Katajainen, "In-place calculation of minimum-redundancy codes": a[] ascending -> code lengths, descending
	a[0] += a[1];
	int root = 0, leaf = 2;
	for (int next = 1; next < m - 1; ++next) {
		if (leaf >= m || a[root] < a[leaf]) { a[next] = a[root]; a[root++] = (uint32_t)next; } else a[next] = a[leaf++];
		if (leaf >= m || (root < next && a[root] < a[leaf])) { a[next] += a[root]; a[root++] = (uint32_t)next; } else a[next] += a[leaf++];
	}
	a[m - 2] = 0;
	for (int next = m - 3; next >= 0; --next) a[next] = a[a[next]] + 1;
	int avbl = 1, used = 0, dpth = 0, next = m - 1;
	root = m - 2;
	while (avbl > 0) {
		while (root >= 0 && (int)a[root] == dpth) { ++used; --root; }
		while (avbl > used) { a[next--] = (uint32_t)dpth; --avbl; }
		avbl = 2 * used; ++dpth; used = 0;
	}
	// how many codes of each length; what is longer than max_bits is cut there, and leaves move down until the Kraft sum is one again
	uint32_t cnt[34];
	for (int i = 0; i < 34; ++i) cnt[i] = 0;
	for (int i = 0; i < m; ++i) ++cnt[a[i] < 33? a[i] : 33];
	for (int i = max_bits + 1; i < 34; ++i) { cnt[max_bits] += cnt[i]; cnt[i] = 0; }
	uint32_t total = 0;
	for (int i = max_bits; i > 0; --i) total += cnt[i] << (max_bits - i);
	while (total != 1u << max_bits) {
		--cnt[max_bits];
		for (int i = max_bits - 1; i > 0; --i)
			if (cnt[i]) { --cnt[i]; cnt[i + 1] += 2; break; }
		--total;
	}
	// the shortest codes to the last of the ranking; then the canonical codes in symbol order
	int j = m;
	for (int l = 1; l <= max_bits; ++l)
		for (uint32_t k = 0; k < cnt[l]; ++k) cw[sorted[--j]] = (uint32_t)l << 16;
	uint32_t nxt[17], code = 0;
	nxt[0] = 0;
	for (int l = 1; l <= max_bits; ++l) { code = (code + (l > 1? cnt[l - 1] : 0)) << 1; nxt[l] = code; }
	for (int s = 0; s < n; ++s) {
		const uint32_t l = cw[s] >> 16;
		if (l == 0) continue;
		uint32_t c = nxt[l]++, r = 0;
		for (uint32_t b = 0; b < l; ++b) { r = r << 1 | (c & 1); c >>= 1; }
		cw[s] = r | l << 16;
	}
}
// the order in which the header lists the code-length code's lengths
MM_HD int dfl_cl_order(int i)
{
	switch (i) {
	case 0: return 16; case 1: return 17; case 2: return 18; case 3: return 0; case 4: return 8; case 5: return 7; case 6: return 9; case 7: return 6; case 8: return 10;
	case 9: return 5; case 10: return 11; case 11: return 4; case 12: return 12; case 13: return 3; case 14: return 13; case 15: return 2; case 16: return 14;
	case 17: return 1; default: return 15;
	}
}
// one lane, after the ranking of ll_f and d_f: the three codes, the header's counts and its length in bits
MM_HD void dfl_build(DflWork &W)
{
	dfl_make_code(W.ll_f, DFL_N_LL, 15, W.ll_sorted, W.a, W.ll_cw);
	dfl_make_code(W.d_f, DFL_N_D, 15, W.d_sorted, W.a, W.d_cw);
	uint32_t n_ll = 257, n_d = 1;
	for (uint32_t s = 257; s < DFL_N_LL; ++s) if (W.ll_cw[s]) n_ll = s + 1;
	for (uint32_t s = 1; s < DFL_N_D; ++s) if (W.d_cw[s]) n_d = s + 1;
	for (int s = 0; s <= DFL_N_CL; ++s) W.cl_f[s] = 0;
	for (uint32_t s = 0; s < n_ll; ++s) ++W.cl_f[W.ll_cw[s] >> 16];
	for (uint32_t s = 0; s < n_d; ++s) ++W.cl_f[W.d_cw[s] >> 16];
	int used = 0;
	for (int s = 0; s < DFL_N_CL; ++s) used += W.cl_f[s] != 0;
	if (used == 1) ++W.cl_f[W.cl_f[0]? 1 : 0];                 // (a code-length code has to be complete: a second symbol that nothing uses)
	for (int s = 0; s < DFL_N_CL; ++s) dfl_rank(W.cl_f, DFL_N_CL, s, W.cl_sorted);
	dfl_make_code(W.cl_f, DFL_N_CL, 7, W.cl_sorted, W.a, W.cl_cw);
	uint32_t n_cl = 4;
	for (int i = 4; i < DFL_N_CL; ++i) if (W.cl_cw[dfl_cl_order(i)]) n_cl = (uint32_t)i + 1;
	uint32_t bits = 3 + 5 + 5 + 4 + 3 * n_cl;
	for (uint32_t s = 0; s < n_ll; ++s) bits += W.cl_cw[W.ll_cw[s] >> 16] >> 16;
	for (uint32_t s = 0; s < n_d; ++s) bits += W.cl_cw[W.d_cw[s] >> 16] >> 16;
	W.n_ll = n_ll; W.n_d = n_d; W.n_cl = n_cl; W.head_bits = bits;
}

// ---- bits
// the bits of segment seg's tokens
MM_HD uint32_t dfl_seg_bits(const DflWork &W, uint32_t seg, const uint32_t *scr)
{
	const uint32_t *t = scr + seg * DFL_SEG;
	uint32_t bits = 0;
	for (uint32_t k = 0; k < W.n_tok[seg]; ++k) {
		if (t[k] & DFL_TOK_MATCH) {
			uint32_t sym, eb, ev;
			dfl_len_sym((t[k] >> 16 & 0xff) + 3, &sym, &eb, &ev); bits += (W.ll_cw[sym] >> 16) + eb;
			dfl_dist_sym((t[k] & 0x7fff) + 1, &sym, &eb, &ev); bits += (W.d_cw[sym] >> 16) + eb;
		} else bits += W.ll_cw[t[k]] >> 16;
	}
	return bits;
}
// a run of bits from bit `at` of the words on: whole words leave as they fill, and every word is OR-ed, since neighbours share the ends
struct DflBits {
	uint32_t *w; uint64_t acc; uint32_t n, word;
	MM_HD DflBits(uint32_t *w_, uint32_t at) : w(w_), acc(0), n(at & 31), word(at >> 5) {}
	MM_HD void put(uint32_t v, uint32_t k)
	{
		acc |= (uint64_t)v << n; n += k;
		if (n >= 32) { DFL_OR(&w[word], (uint32_t)acc); ++word; acc >>= 32; n -= 32; }
	}
	MM_HD void cw(uint32_t c) { put(c & 0xffff, c >> 16); }
	MM_HD void flush() { if (n) DFL_OR(&w[word], (uint32_t)acc); }
};
MM_HD void dfl_put_byte(uint32_t *w, uint32_t at, uint32_t v) { DFL_OR(&w[at >> 2], (v & 0xff) << 8 * (at & 3)); }
// the gzip header (BSIZE: the block's real size), the block header and the codes' lengths: one lane.  The deflate stream begins at byte DFL_GZ_HEAD
MM_HD void dfl_emit_head(const DflWork &W, uint32_t *w)
{
	const uint32_t total = DFL_GZ_HEAD + W.n_bytes + 8;
	for (uint32_t i = 0; i < DFL_GZ_HEAD; ++i) dfl_put_byte(w, i, i == 16? (total - 1) & 0xff : i == 17? (total - 1) >> 8 : bgzf_head_byte((int)i, 0));
	DflBits b(w, DFL_GZ_HEAD * 8);
	b.put(1, 1); b.put(2, 2);                                  // BFINAL, BTYPE 10: dynamic Huffman
	b.put(W.n_ll - 257, 5); b.put(W.n_d - 1, 5); b.put(W.n_cl - 4, 4);
	for (uint32_t i = 0; i < W.n_cl; ++i) b.put(W.cl_cw[dfl_cl_order((int)i)] >> 16, 3);
	for (uint32_t s = 0; s < W.n_ll; ++s) b.cw(W.cl_cw[W.ll_cw[s] >> 16]);
	for (uint32_t s = 0; s < W.n_d; ++s) b.cw(W.cl_cw[W.d_cw[s] >> 16]);
	b.flush();
}
// segment seg's tokens, from the bit offset the scan gave it (W.seg_bits[seg], counted from the deflate stream's first bit)
MM_HD void dfl_emit_seg(const DflWork &W, uint32_t seg, const uint32_t *scr, uint32_t *w)
{
	const uint32_t *t = scr + seg * DFL_SEG;
	DflBits b(w, DFL_GZ_HEAD * 8 + W.seg_bits[seg]);
	for (uint32_t k = 0; k < W.n_tok[seg]; ++k) {
		if (t[k] & DFL_TOK_MATCH) {
			uint32_t sym, eb, ev;
			dfl_len_sym((t[k] >> 16 & 0xff) + 3, &sym, &eb, &ev); b.cw(W.ll_cw[sym]); b.put(ev, eb);
			dfl_dist_sym((t[k] & 0x7fff) + 1, &sym, &eb, &ev); b.cw(W.d_cw[sym]); b.put(ev, eb);
		} else b.cw(W.ll_cw[t[k]]);
	}
	b.flush();
}
// the end-of-block code at bit `at` of the stream, CRC-32 and ISIZE behind the stream's last byte: one lane
MM_HD void dfl_emit_tail(const DflWork &W, uint32_t at, uint32_t crc, uint32_t len, uint32_t *w)
{
	DflBits b(w, DFL_GZ_HEAD * 8 + at);
	b.cw(W.ll_cw[DFL_EOB]);
	b.flush();
	for (uint32_t i = 0; i < 4; ++i) { dfl_put_byte(w, DFL_GZ_HEAD + W.n_bytes + i, crc >> 8 * i); dfl_put_byte(w, DFL_GZ_HEAD + W.n_bytes + 4 + i, len >> 8 * i); }
}
// the stream's bytes from the header's bits, the tokens' and the end-of-block code's; shorter than the stored form's len + 5, or the block is stored
MM_HD uint32_t dfl_stream_bytes(const DflWork &W, uint32_t token_bits) { return (W.head_bits + token_bits + (W.ll_cw[DFL_EOB] >> 16) + 7) / 8; }

// ------------------------------------------------------------------ host side: the lanes in loops
struct DflHost {
	std::vector<uint32_t> buf, scr; DflWork W;
	DflHost() : buf(DFL_BUF_WORDS), scr(BGZF_PAYLOAD) {}
};
// one payload into o (room for len + BGZF_EXTRA bytes); returns the block's size; *stored: the stored form was written
inline uint32_t dfl_block_host(const unsigned char *src, uint32_t len, unsigned char *o, DflHost &S, bool *stored)
{
	DflWork &W = S.W;
	uint32_t *buf = S.buf.data(), *scr = S.scr.data();
	memset(&W, 0, sizeof(W));
	std::fill(S.buf.begin(), S.buf.end(), 0u);
	for (uint32_t r = 0; r * DFL_ROUND < len; ++r) {
		uint32_t h1[DFL_ROUND];
		for (uint32_t lane = 0; lane < DFL_ROUND; ++lane) { h1[lane] = dfl_hash1(src, len, r * DFL_ROUND + lane); dfl_round_read(r * DFL_ROUND + lane, len, h1[lane], buf, scr); }
		for (uint32_t lane = 0; lane < DFL_ROUND; ++lane) dfl_round_raise(r * DFL_ROUND + lane, h1[lane], buf);
	}
	for (uint32_t seg = 0; seg < DFL_SEGS; ++seg) W.n_tok[seg] = dfl_parse(src, len, seg, scr, W.ll_f, W.d_f);
	W.ll_f[DFL_EOB] = 1;
	for (int s = 0; s < DFL_N_LL; ++s) dfl_rank(W.ll_f, DFL_N_LL, s, W.ll_sorted);
	for (int s = 0; s < DFL_N_D; ++s) dfl_rank(W.d_f, DFL_N_D, s, W.d_sorted);
	dfl_build(W);
	uint32_t at = W.head_bits;
	for (uint32_t seg = 0; seg < DFL_SEGS; ++seg) { const uint32_t b = dfl_seg_bits(W, seg, scr); W.seg_bits[seg] = at; at += b; }
	W.n_bytes = dfl_stream_bytes(W, at - W.head_bits);
	*stored = W.n_bytes >= len + 5;
	if (*stored) { mm355_bgzf_frame_host((const char*)src, len, (char*)o); return len + BGZF_EXTRA; }
	std::fill(S.buf.begin(), S.buf.end(), 0u);
	dfl_emit_head(W, buf);
	for (uint32_t seg = 0; seg < DFL_SEGS; ++seg) dfl_emit_seg(W, seg, scr, buf);
	dfl_emit_tail(W, at, (uint32_t)crc32(crc32(0L, Z_NULL, 0), (const Bytef*)src, len), len, buf);
	const uint32_t total = DFL_GZ_HEAD + W.n_bytes + 8;
	for (uint32_t i = 0; i < total; ++i) o[i] = (unsigned char)(buf[i >> 2] >> 8 * (i & 3));
	return total;
}

// n bytes into BGZF blocks, deflated where that is shorter; out: room for bgzf_size(n) bytes; returns the bytes written
inline int64_t mm355_bgzf_deflate_host(const char *data, int64_t n, char *out, int64_t *n_stored = 0)
{
	DflHost S;
	int64_t at_out = 0, ns = 0;
	for (int64_t at = 0; at < n; at += BGZF_PAYLOAD) {
		bool stored;
		at_out += dfl_block_host((const unsigned char*)data + at, (uint32_t)(n - at < BGZF_PAYLOAD? n - at : BGZF_PAYLOAD), (unsigned char*)out + at_out, S, &stored);
		ns += stored;
	}
	if (n_stored) *n_stored = ns;
	return at_out;
}
