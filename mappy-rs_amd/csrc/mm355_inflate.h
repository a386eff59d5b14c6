// mm355_inflate.h -- the RFC 1951 decoder of ONE BGZF member, stated once (the inverse of mm355_deflate.h): the functions the kernel calls
// (mm355_inflate.hip::k_bgzf_inflate: 256 lanes, barriers between the steps) are the functions the host runs in loops over the lanes
// (inf_member_host below; tests/host_harness/inflate_host.cpp builds it with g++ alone).  The input is untrusted: every read of the compressed
// bytes and every write or back-reference in the output is bounded by the spans the caller gave, and a member is refused (a status, no payload)
// for anything zlib's inflate refuses -- tests/test_inflate_host.py holds the two to the same verdict over 20 000 mutated members.
// The steps of a member:
//   stage    the compressed bytes (cdata: BSIZE + 1 - header - 8 bytes) as little-endian dwords, zeros behind the last byte: a lane per dword.
//            The bit reader takes whole dwords and can never leave the staged words; what it took is counted, and a symbol that needed a bit
//            past cdata's end is "input ran out".
//   head     one lane, per deflate block (a member has as many as its producer liked): BFINAL, BTYPE; stored: LEN / NLEN and where the bytes lie;
//            fixed: the code lengths of RFC 1951 3.2.6; dynamic: the code-length code, the HLIT + HDIST lengths with the run symbols 16 - 18 (a
//            run may cross from the literal/length lengths into the distance lengths).  Then for both codes the counts per length, the Kraft
//            check (over-subscribed: refused; incomplete: refused unless the code is a single code of one bit, or -- distances only -- no code at
//            all), the symbols sorted by (length, symbol) and every symbol's canonical code, its first bit lowest.
//   tables   a lane per symbol: a code of at most INF_LL_BITS (INF_D_BITS) bits is replicated into a first-level table indexed by the stream's
//            next bits.  Longer codes are not in it: the decoding lane finds them by the canonical walk over the counts, bit by bit.
//   symbols  one lane: literals, matches (length 3 .. 258, distance 1 .. 32768, never before the payload's first byte, never past ISIZE; a
//            match may overlap its own output) into the window, up to the end-of-block code.
//   stored   all lanes copy LEN bytes from the staged words into the window.
// After the last block the window holds ISIZE bytes or the member is refused; CRC-32 and ISIZE are compared with the trailer (the kernel: the
// framing kernel's lanes, mm355_bam.h::bgzf_lane_crc; the host: zlib's crc32).  Bytes between the last block's end and the trailer are ignored.
#pragma once
#include <vector>
#include "mm355_bam.h"

#define INF_MAX_ISIZE 65536              // the BGZF specification's largest payload (this library writes BGZF_PAYLOAD = 0xff00)
#define INF_MAX_CDATA 65536              // BSIZE is 16 bits: a member is at most 65536 bytes, header and trailer included
#define INF_IN_WORDS (INF_MAX_CDATA / 4 + 2)
#define INF_LL_BITS 10
#define INF_D_BITS 8
#define INF_N_LL 288                     // HLIT is 5 bits: up to 288 lengths can be sent (286 and 287 never decode to anything legal)
#define INF_N_D 32
#define INF_N_CL 19
#define INF_STORED 0
#define INF_HUFFMAN 1

// a member's status: 0, or why it was refused
enum {
	INF_OK = 0, INF_E_BTYPE, INF_E_STORED, INF_E_HEADER, INF_E_OVER, INF_E_INCOMPLETE, INF_E_NO_EOB, INF_E_REPEAT, INF_E_SYMBOL, INF_E_DIST,
	INF_E_OUT_LONG, INF_E_OUT_SHORT, INF_E_INPUT, INF_E_CRC, INF_E_SPAN
};

// a Huffman code as the canonical walk reads it (count per length, symbols by (length, symbol)) and as the table fill reads it (code per symbol)
struct InfCode { uint16_t count[16], sym[INF_N_LL], code[INF_N_LL]; };

// what a member's lanes share besides the window
struct InfWork {
	uint32_t in[INF_IN_WORDS];                          // cdata, staged
	uint32_t ll_tab[1 << INF_LL_BITS], d_tab[1 << INF_D_BITS];   // symbol | length << 16; 0: not a code of at most that many bits
	InfCode ll, d;
	unsigned char lens[INF_N_LL + INF_N_D];            // the block's code lengths: literal/length, then distance
	uint32_t n_in, isize, out, status, last, kind, n_ll, n_d, st_at, st_len;   // out: bytes in the window; st_*: a stored block's bytes in cdata
};

// dword w of the n bytes at p, little-endian, zeros behind the last byte
MM_HD uint32_t inf_word(const unsigned char *p, uint32_t n, uint32_t w)
{
	uint32_t v = 0;
	for (uint32_t k = 0; k < 4; ++k) if (4 * w + k < n) v |= (uint32_t)p[4 * w + k] << 8 * k;
	return v;
}
MM_HD uint32_t inf_in_words(uint32_t n_in) { return (n_in + 3) / 4; }
MM_HD unsigned char inf_in_byte(const uint32_t *in, uint32_t at) { return (unsigned char)(in[at >> 2] >> 8 * (at & 3)); }

// the bit reader of the decoding lane: whole staged dwords into a 64-bit buffer, the stream's next bit lowest
struct InfBits {
	const uint32_t *in; uint32_t n_words, n_in; uint64_t buf; uint32_t cnt, wpos;
	MM_HD InfBits(const uint32_t *in_, uint32_t n_in_) : in(in_), n_words(inf_in_words(n_in_)), n_in(n_in_), buf(0), cnt(0), wpos(0) {}
	MM_HD void fill() { if (cnt <= 32) { buf |= (uint64_t)(wpos < n_words? in[wpos] : 0u) << cnt; ++wpos; cnt += 32; } }   // more than 32 bits after it
	MM_HD uint32_t peek(uint32_t k) const { return (uint32_t)buf & ((1u << k) - 1); }
	MM_HD void drop(uint32_t k) { buf >>= k; cnt -= k; }
	MM_HD uint32_t get(uint32_t k) { fill(); const uint32_t v = peek(k); drop(k); return v; }                               // k <= 16
	MM_HD uint64_t used() const { return (uint64_t)32 * wpos - cnt; }              // bits taken from the stream
	MM_HD bool overrun() const { return used() > (uint64_t)8 * n_in; }             // some of them were not cdata's
	MM_HD void seek(uint32_t byte) { wpos = byte >> 2; buf = 0; cnt = 0; fill(); drop(8 * (byte & 3)); }
};

MM_HD int inf_cl_order(int i)
{
	switch (i) {
	case 0: return 16; case 1: return 17; case 2: return 18; case 3: return 0; case 4: return 8; case 5: return 7; case 6: return 9; case 7: return 6; case 8: return 10;
	case 9: return 5; case 10: return 11; case 11: return 4; case 12: return 12; case 13: return 3; case 14: return 13; case 15: return 2; case 16: return 14;
	case 17: return 1; default: return 15;
	}
}

// counts, Kraft check, sorted symbols and canonical codes of n lengths.  cl: the code-length code, which may not be incomplete at all
MM_HD uint32_t inf_construct(const unsigned char *lens, int n, bool cl, InfCode &C)
{
	for (int l = 0; l < 16; ++l) C.count[l] = 0;
	for (int s = 0; s < n; ++s) ++C.count[lens[s]];
	int max = 15;
	while (max > 0 && C.count[max] == 0) --max;
	int left = 1;
	for (int l = 1; l < 16; ++l) {
		left = 2 * left - (int)C.count[l];
		if (left < 0) return INF_E_OVER;
	}
	if (max == 0) { C.count[0] = 0; return cl? INF_E_INCOMPLETE : INF_OK; }   // no code at all: every symbol of it is refused when it is met
	if (left > 0 && (cl || max != 1)) return INF_E_INCOMPLETE;
	uint16_t offs[16], nxt[16];
	uint32_t code = 0;
	offs[1] = 0; nxt[0] = 0;
	for (int l = 1; l < 15; ++l) offs[l + 1] = (uint16_t)(offs[l] + C.count[l]);
	for (int l = 1; l < 16; ++l) { code = (code + (l > 1? C.count[l - 1] : 0u)) << 1; nxt[l] = (uint16_t)code; }
	for (int s = 0; s < n; ++s) {
		const uint32_t l = lens[s];
		C.code[s] = 0;
		if (l == 0) continue;
		C.sym[offs[l]++] = (uint16_t)s;
		uint32_t c = nxt[l]++, r = 0;
		for (uint32_t b = 0; b < l; ++b) { r = r << 1 | (c & 1); c >>= 1; }
		C.code[s] = (uint16_t)r;
	}
	C.count[0] = 0;
	return INF_OK;
}

// the lane of symbol s: its code, if short enough, into every table entry whose low bits are the code
MM_HD void inf_fill(const InfCode &C, const unsigned char *lens, uint32_t s, uint32_t bits, uint32_t *tab)
{
	const uint32_t l = lens[s];
	if (l == 0 || l > bits) return;
	for (uint32_t i = C.code[s]; i < 1u << bits; i += 1u << l) tab[i] = s | l << 16;
}

// the next symbol (B holds more than 15 bits, zeros where the stream has ended), or -1: the bits are no code
MM_HD int inf_decode(InfBits &B, const uint32_t *tab, uint32_t bits, const InfCode &C)
{
	const uint32_t e = tab[B.peek(bits)];
	if (e) { B.drop(e >> 16); return (int)(e & 0xffff); }
	int code = 0, first = 0, index = 0;
	uint32_t b = (uint32_t)B.buf;
	for (uint32_t l = 1; l < 16; ++l) {
		code |= (int)(b & 1); b >>= 1;
		const int cnt = C.count[l];
		if (code - cnt < first) { B.drop(l); return C.sym[index + (code - first)]; }
		index += cnt; first += cnt; first <<= 1; code <<= 1;
	}
	return -1;
}
// the same through the walk alone (the code-length code: no table)
MM_HD int inf_decode_slow(InfBits &B, const InfCode &C)
{
	int code = 0, first = 0, index = 0;
	uint32_t b = (uint32_t)B.buf;
	for (uint32_t l = 1; l < 16; ++l) {
		code |= (int)(b & 1); b >>= 1;
		const int cnt = C.count[l];
		if (code - cnt < first) { B.drop(l); return C.sym[index + (code - first)]; }
		index += cnt; first += cnt; first <<= 1; code <<= 1;
	}
	return -1;
}

// ---- head: one lane.  Returns the status; W.kind says what follows, W.last that no block does
MM_HD uint32_t inf_block_head(InfWork &W, InfBits &B)
{
	W.last = B.get(1);
	const uint32_t type = B.get(2);
	if (B.overrun()) return INF_E_INPUT;
	if (type == 3) return INF_E_BTYPE;
	if (type == 0) {
		B.drop(B.cnt & 7);                                 // to the next byte of the stream
		const uint32_t len = B.get(16), nlen = B.get(16);
		if (B.overrun()) return INF_E_INPUT;
		if (len != (~nlen & 0xffffu)) return INF_E_STORED;
		const uint32_t at = (uint32_t)(B.used() / 8);
		if (len > W.n_in - at) return INF_E_INPUT;
		if (len > W.isize - W.out) return INF_E_OUT_LONG;
		W.kind = INF_STORED; W.st_at = at; W.st_len = len;
		return INF_OK;
	}
	W.kind = INF_HUFFMAN;
	if (type == 1) {
		W.n_ll = 288; W.n_d = 32;                          // (all 32 five-bit distance codes exist: 30 and 31 are refused when they are met)
		for (uint32_t s = 0; s < 288; ++s) W.lens[s] = (unsigned char)(s < 144? 8 : s < 256? 9 : s < 280? 7 : 8);
		for (uint32_t s = 0; s < 32; ++s) W.lens[288 + s] = 5;
	} else {
		const uint32_t n_ll = B.get(5) + 257, n_d = B.get(5) + 1, n_cl = B.get(4) + 4;
		if (B.overrun()) return INF_E_INPUT;
		if (n_ll > 286 || n_d > 30) return INF_E_HEADER;
		unsigned char cl[INF_N_CL];
		for (int i = 0; i < INF_N_CL; ++i) cl[i] = 0;
		for (uint32_t i = 0; i < n_cl; ++i) cl[inf_cl_order((int)i)] = (unsigned char)B.get(3);
		if (B.overrun()) return INF_E_INPUT;
		if (uint32_t e = inf_construct(cl, INF_N_CL, true, W.ll)) return e;      // (W.ll is free until the lengths are known)
		uint32_t have = 0;
		while (have < n_ll + n_d) {
			B.fill();
			const int s = inf_decode_slow(B, W.ll);
			if (s < 0) return B.overrun()? INF_E_INPUT : INF_E_SYMBOL;
			if (s < 16) { W.lens[have++] = (unsigned char)s; if (B.overrun()) return INF_E_INPUT; continue; }
			uint32_t rep, v = 0;
			if (s == 16) { if (have == 0) return INF_E_REPEAT; v = W.lens[have - 1]; rep = 3 + B.get(2); }
			else if (s == 17) rep = 3 + B.get(3);
			else rep = 11 + B.get(7);
			if (B.overrun()) return INF_E_INPUT;
			if (have + rep > n_ll + n_d) return INF_E_REPEAT;
			while (rep--) W.lens[have++] = (unsigned char)v;
		}
		if (W.lens[256] == 0) return INF_E_NO_EOB;
		for (uint32_t s = n_d; s-- > 0; ) W.lens[288 + s] = W.lens[n_ll + s];      // the distance lengths to their place (n_ll <= 288: upwards, from the top)
		for (uint32_t s = n_ll; s < 288; ++s) W.lens[s] = 0;
		W.n_ll = n_ll; W.n_d = n_d;
	}
	if (uint32_t e = inf_construct(W.lens, (int)W.n_ll, false, W.ll)) return e;
	if (uint32_t e = inf_construct(W.lens + 288, (int)W.n_d, false, W.d)) return e;
	return INF_OK;
}

// ---- symbols: one lane, from the block's first code to its end-of-block code; the window's bytes [W.out, ...) are written
MM_HD uint32_t inf_codes(InfWork &W, InfBits &B, unsigned char *win)
{
	uint32_t out = W.out;
	const uint32_t isize = W.isize;
	for (;;) {
		B.fill();
		int s = inf_decode(B, W.ll_tab, INF_LL_BITS, W.ll);
		if (s < 0) return B.overrun()? INF_E_INPUT : INF_E_SYMBOL;
		if (s < 256) {
			if (B.overrun()) return INF_E_INPUT;
			if (out >= isize) return INF_E_OUT_LONG;
			win[out++] = (unsigned char)s;
			continue;
		}
		if (s == 256) { if (B.overrun()) return INF_E_INPUT; W.out = out; return INF_OK; }
		if (s >= 286) return INF_E_SYMBOL;
		const uint32_t k = (uint32_t)s - 257;
		uint32_t len;
		if (k < 8) len = 3 + k;
		else if (k == 28) len = 258;
		else { const uint32_t e = (k - 4) >> 2; len = 3 + ((4 + (k & 3)) << e) + B.peek(e); B.drop(e); }
		B.fill();
		const int d = inf_decode(B, W.d_tab, INF_D_BITS, W.d);
		if (d < 0) return B.overrun()? INF_E_INPUT : INF_E_SYMBOL;
		if (d >= 30) return INF_E_SYMBOL;
		uint32_t dist;
		if (d < 4) dist = 1 + (uint32_t)d;
		else { const uint32_t e = ((uint32_t)d >> 1) - 1; dist = 1 + ((2 + ((uint32_t)d & 1)) << e) + B.peek(e); B.drop(e); }
		if (B.overrun()) return INF_E_INPUT;
		if (dist > out) return INF_E_DIST;
		if (len > isize - out) return INF_E_OUT_LONG;
		const unsigned char *from = win + (out - dist);
		uint32_t i = 0;
		if (dist >= 8)                                             // eight loads, then eight stores: none of them reads what the chunk writes
			for (; i + 8 <= len; i += 8) {
				unsigned char t[8];
				for (uint32_t k = 0; k < 8; ++k) t[k] = from[i + k];
				for (uint32_t k = 0; k < 8; ++k) win[out + i + k] = t[k];
			}
		for (; i < len; ++i) win[out + i] = from[i];               // (byte by byte: a match may overlap itself)
		out += len;
	}
}

// ---- stored: the lane's bytes of the block's LEN, then (one lane) the reader behind them
MM_HD void inf_stored_copy(const InfWork &W, uint32_t lane, uint32_t n_lanes, unsigned char *win)
{
	for (uint32_t i = lane; i < W.st_len; i += n_lanes) win[W.out + i] = inf_in_byte(W.in, W.st_at + i);
}
MM_HD void inf_stored_done(InfWork &W, InfBits &B) { W.out += W.st_len; B.seek(W.st_at + W.st_len); }

// ------------------------------------------------------------------ host side: the lanes in loops
struct InfHost { InfWork W; };
// one member: cdata[0 .. n_in) inflated into out[0 .. isize), the trailer's CRC-32 compared; returns the status
inline uint32_t inf_member_host(const unsigned char *cdata, uint32_t n_in, uint32_t isize, uint32_t crc, unsigned char *out, InfHost &S)
{
	InfWork &W = S.W;
	if (n_in > INF_MAX_CDATA || isize > INF_MAX_ISIZE) return INF_E_SPAN;
	for (uint32_t w = 0; w < inf_in_words(n_in) + 1; ++w) W.in[w] = inf_word(cdata, n_in, w);
	W.n_in = n_in; W.isize = isize; W.out = 0; W.status = 0; W.last = 0;
	InfBits B(W.in, n_in);
	for (;;) {
		if ((W.status = inf_block_head(W, B))) return W.status;
		if (W.kind == INF_STORED) {
			for (uint32_t lane = 0; lane < BGZF_LANES; ++lane) inf_stored_copy(W, lane, BGZF_LANES, out);
			inf_stored_done(W, B);
		} else {
			for (uint32_t i = 0; i < 1u << INF_LL_BITS; ++i) W.ll_tab[i] = 0;
			for (uint32_t i = 0; i < 1u << INF_D_BITS; ++i) W.d_tab[i] = 0;
			for (uint32_t s = 0; s < W.n_ll; ++s) inf_fill(W.ll, W.lens, s, INF_LL_BITS, W.ll_tab);
			for (uint32_t s = 0; s < W.n_d; ++s) inf_fill(W.d, W.lens + 288, s, INF_D_BITS, W.d_tab);
			if ((W.status = inf_codes(W, B, out))) return W.status;
		}
		if (W.last) break;
	}
	if (W.out != isize) return W.status = INF_E_OUT_SHORT;
	if ((uint32_t)crc32(crc32(0L, Z_NULL, 0), (const Bytef*)out, isize) != crc) return W.status = INF_E_CRC;
	return INF_OK;
}
