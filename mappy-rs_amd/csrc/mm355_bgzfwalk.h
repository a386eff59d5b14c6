// mm355_bgzfwalk.h -- the host's walk over a buffer of BGZF members, the only sequential part of reading a BGZF file: a member's place
// follows from the BSIZE of the members before it.  Plain C++: no HIP here, the CPU suite compiles this file with g++ alone.
//   member   1f 8b 08 FLG(FEXTRA set, no name / comment / header CRC) MTIME(4) XFL OS XLEN(2) -- 12 bytes; XLEN bytes of subfields
//            (SI1 SI2 SLEN(2) data), one of them 'B' 'C' with SLEN 2: BSIZE = the member's size - 1; cdata; CRC-32(4) ISIZE(4)
// MTIME, XFL and OS are ignored, and other subfields may stand in front of BC.  Per member the walk gives where cdata lies, its length, the
// trailer's CRC-32 and ISIZE and the exclusive prefix sum of ISIZE: the inflate kernel writes every payload straight to its place.
#pragma once
#include <stdint.h>
#include <vector>
#include "../../include/mm355.h"

#define BGZF_WALK_NOT_BGZF 1             // the buffer's first member is no BGZF member: not an error, the file is something else
#define BGZF_MAX_ISIZE 65536

struct BgzfMember { int64_t c_off, o_off; uint32_t c_len, isize, crc, pad; };   // cdata at c_off of the buffer, c_len bytes; the payload at o_off of the output

static inline uint32_t bgzf_le16(const unsigned char *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
static inline uint32_t bgzf_le32(const unsigned char *p) { return bgzf_le16(p) | bgzf_le16(p + 2) << 16; }

// The member at buf[at ...) of the n bytes.  Returns its size and fills *m (o_off apart); 0: the buffer ends inside it (more bytes are needed);
// -1: these bytes are no BGZF member
static inline int64_t bgzf_member(const unsigned char *buf, int64_t n, int64_t at, BgzfMember *m)
{
	const unsigned char *p = buf + at;
	const int64_t have = n - at;
	if (have >= 1 && p[0] != 0x1f) return -1;
	if (have >= 2 && p[1] != 0x8b) return -1;
	if (have >= 3 && p[2] != 8) return -1;
	if (have >= 4 && ((p[3] & 4) == 0 || (p[3] & 0x1a) != 0)) return -1;
	if (have < 12) return 0;
	const int64_t xlen = bgzf_le16(p + 10);
	if (have < 12 + xlen) return 0;
	int64_t bsize = -1;
	for (int64_t x = 12; x + 4 <= 12 + xlen; ) {
		const int64_t slen = bgzf_le16(p + x + 2);
		if (x + 4 + slen > 12 + xlen) return -1;          // a subfield that leaves the extra field
		if (p[x] == 'B' && p[x + 1] == 'C' && slen == 2) { bsize = bgzf_le16(p + x + 4); break; }
		x += 4 + slen;
	}
	if (bsize < 0) return -1;
	const int64_t total = bsize + 1;
	if (total < 12 + xlen + 8) return -1;                  // no room for the trailer
	if (have < total) return 0;
	m->c_off = at + 12 + xlen; m->c_len = (uint32_t)(total - 12 - xlen - 8);
	m->crc = bgzf_le32(p + total - 8); m->isize = bgzf_le32(p + total - 4); m->pad = 0; m->o_off = 0;
	if (m->isize > BGZF_MAX_ISIZE) return -1;
	return total;
}

// Walks the whole members of buf[0 .. n) and appends them to `out`, o_off counting on from *n_out (which is advanced).  first: buf begins at the
// file's first byte; at_eof: nothing follows buf.  max_out > 0: no more members than inflate to max_out bytes, but one at least (a reader
// bounds a piece's output by it: a few crafted bytes can claim 64 KB each).  *used: the bytes of the members taken -- the rest goes in front
// of the next piece.  Returns 0; BGZF_WALK_NOT_BGZF (first only); MM355_EIO for a malformed later member or a file that ends inside a member.
// A file need not end with the empty EOF member.
static inline int bgzf_walk(const unsigned char *buf, int64_t n, bool first, bool at_eof, std::vector<BgzfMember> &out, int64_t *used, int64_t *n_out, int64_t max_out = 0)
{
	int64_t at = 0;
	const int64_t base = *n_out;
	*used = 0;
	while (at < n) {
		BgzfMember m;
		const int64_t sz = bgzf_member(buf, n, at, &m);
		if (sz < 0) return first && at == 0? BGZF_WALK_NOT_BGZF : MM355_EIO;
		if (sz == 0) {
			if (!at_eof) break;
			return first && at == 0 && n < 18? BGZF_WALK_NOT_BGZF : MM355_EIO;   // (a file too short for any member's header is something else)
		}
		if (max_out > 0 && at > 0 && *n_out - base + (int64_t)m.isize > max_out) break;
		m.o_off = *n_out; *n_out += m.isize;
		out.push_back(m);
		at += sz;
	}
	*used = at;
	return 0;
}
