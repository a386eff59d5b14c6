// mm355_bamread.h -- what the streaming reader of read sets (mm355_index.cpp: mm355_fastx_next) reads through and, for a BAM, with:
//   ByteSource   where the inflated bytes of a reads file come from: zlib (plain and gzip files, and BGZF on the host), or the device
//                inflater's stream (mm355_inflate.hip)
//   the BAM loop a stream that begins "BAM\1" is a BAM file (unaligned, as basecallers write it, or aligned): the header is skipped, and every
//                record but the secondary and supplementary ones (flag & 0x900, as `samtools fastq`) gives a read -- the name, the bases from
//                the nibbles, the quality + 33 (first byte 0xff: none), a record with flag 0x10 turned back to the read as sequenced.  Aux
//                tags are dropped, or (mm355_fastx_keep_aux) read in chunks and filtered by mm355_bamaux.h::bam_aux_split; a 0x10 record keeps
//                its aux verbatim: MM / ML are defined on the read as sequenced, which is what the reader restores.  The @RG lines of the
//                header text are kept for the writer of the output header.
// The loop parses untrusted input: it takes a record's fields only as far as block_size allows, never allocates by a length the stream has
// not delivered, and answers MM355_EIO for a block_size below 32, an l_read_name of 0, fields that exceed block_size and a stream that ends
// inside the header or a record.  Plain C++ (tests/host_harness/inflate_host.cpp builds it with g++ alone).
#pragma once
#include <stdint.h>
#include <string>
#include "mm355_sam.h"
#include "mm355_bamaux.h"

struct ByteSource {
	virtual ~ByteSource() {}
	virtual int64_t read(void *buf, size_t cap) = 0;       // the next bytes, at most cap: > 0; 0 at the end; an MM355_E* code
};

// exactly n bytes through a buffer the reader owns; R has: int64_t take(void *dst, size_t n) -- the bytes it could give (fewer: the stream
// ended), dst == 0 to skip them; int err() -- the source's error, if that is why
template <typename R> static inline int bam_need(R &r, void *dst, size_t n) { return (size_t)r.take(dst, n) == n? 0 : MM355_EIO; }

static inline uint32_t bam_le32(const unsigned char *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// the @RG lines of a header text that arrives in pieces: a line is kept from its first byte on while it can still begin "@RG\t", the text
// ends at its first NUL, and a last line without a newline gets one
struct BamRgFilter {
	std::string *rg; std::string line; bool live = true, done = false;
	explicit BamRgFilter(std::string *rg_) : rg(rg_) {}
	void end_line() { if (live && line.size() >= 4) { *rg += line; *rg += '\n'; } line.clear(); live = true; }
	void feed(const unsigned char *p, size_t n)
	{
		for (size_t i = 0; i < n && !done; ++i) {
			if (p[i] == 0) { done = true; break; }
			if (p[i] == '\n') { end_line(); continue; }
			if (!live) continue;
			if (line.size() < 4 && (char)p[i] != "@RG\t"[line.size()]) { live = false; line.clear(); continue; }
			line += (char)p[i];
		}
	}
	void finish() { if (!line.empty()) end_line(); }
};

// the header, magic included: l_text, text, n_ref, per reference l_name, name, l_ref.  rg != 0: the text's @RG lines are appended to it
template <typename R> static inline int bam_read_header(R &r, std::string *rg)
{
	unsigned char w[8];
	if (bam_need(r, w, 8) || memcmp(w, "BAM\1", 4) != 0) return MM355_EIO;
	if (bam_le32(w + 4) > (uint32_t)INT32_MAX) return MM355_EIO;
	if (rg == 0) { if (bam_need(r, 0, bam_le32(w + 4))) return MM355_EIO; }
	else {
		BamRgFilter flt(rg);
		unsigned char chunk[4096];
		for (uint64_t left = bam_le32(w + 4); left > 0; ) {    // (in chunks: what is kept has been delivered)
			const size_t k = left < sizeof(chunk)? (size_t)left : sizeof(chunk);
			if (bam_need(r, chunk, k)) return MM355_EIO;
			flt.feed(chunk, k);
			left -= k;
		}
		flt.finish();
	}
	if (bam_need(r, w, 4)) return MM355_EIO;
	const uint32_t n_ref = bam_le32(w);
	if (n_ref > (uint32_t)INT32_MAX) return MM355_EIO;
	for (uint32_t i = 0; i < n_ref; ++i) {
		if (bam_need(r, w, 4) || bam_le32(w) > (uint32_t)INT32_MAX || bam_need(r, 0, (size_t)bam_le32(w) + 4)) return MM355_EIO;
	}
	return 0;
}
template <typename R> static inline int bam_read_header(R &r) { return bam_read_header(r, (std::string*)0); }

MM_HD char bam_base(uint32_t code)
{
	switch (code & 15) {
	case 0: return '='; case 1: return 'A'; case 2: return 'C'; case 3: return 'M'; case 4: return 'G'; case 5: return 'R'; case 6: return 'S'; case 7: return 'V';
	case 8: return 'T'; case 9: return 'W'; case 10: return 'Y'; case 11: return 'H'; case 12: return 'K'; case 13: return 'D'; case 14: return 'B'; default: return 'N';
	}
}

// The next read: 1, the name set, the bases APPENDED to seq, qual set (*has_qual: the record has one); 0 at the end of the stream; MM355_EIO.
// keep != 0 (a string bam_aux_keep_ok accepts): the record's aux block through bam_aux_split into aux, *aux_mod the offset of its second
// group; a malformed block is MM355_EIO like every other malformed record
template <typename R> static inline int bam_read_record(R &r, std::string &name, std::string &seq, std::string &qual, bool *has_qual, const char *keep, std::string &aux,
                                                        int32_t *aux_mod)
{
	for (;;) {
		unsigned char f[36];
		const int64_t got = r.take(f, 4);
		if (got == 0) return r.err()? MM355_EIO : 0;
		if (got != 4) return MM355_EIO;
		const uint64_t block_size = bam_le32(f);
		if (block_size < 32 || bam_need(r, f + 4, 32)) return MM355_EIO;
		const uint64_t l_name = f[12], n_cigar = (uint32_t)f[16] | (uint32_t)f[17] << 8, l_seq = bam_le32(f + 20);
		const uint32_t flag = (uint32_t)f[18] | (uint32_t)f[19] << 8;
		const uint64_t fields = l_name + 4 * n_cigar + (l_seq + 1) / 2 + l_seq;
		if (l_name == 0 || 32 + fields > block_size) return MM355_EIO;
		if (flag & 0x900) {                                    // not a read of its own
			if (bam_need(r, 0, (size_t)(block_size - 32))) return MM355_EIO;
			continue;
		}
		char nm[256];
		if (bam_need(r, nm, (size_t)l_name) || bam_need(r, 0, (size_t)(4 * n_cigar))) return MM355_EIO;
		name.assign(nm, strnlen(nm, (size_t)l_name - 1));
		const size_t start = seq.size();
		const bool rev = (flag & 0x10) != 0;
		unsigned char chunk[4096];
		for (uint64_t done = 0; done < l_seq; ) {              // (in chunks: what is appended has been delivered)
			const uint64_t bases = l_seq - done < 8192? l_seq - done : 8192;
			if (bam_need(r, chunk, (size_t)((bases + 1) / 2))) return MM355_EIO;
			for (uint64_t i = 0; i < bases; ++i) seq.push_back(bam_base(i & 1? chunk[i >> 1] : chunk[i >> 1] >> 4));
			done += bases;
		}
		qual.clear();
		*has_qual = false;
		for (uint64_t done = 0; done < l_seq; ) {
			const uint64_t k = l_seq - done < sizeof(chunk)? l_seq - done : sizeof(chunk);
			if (bam_need(r, chunk, (size_t)k)) return MM355_EIO;
			if (done == 0) *has_qual = chunk[0] != 0xff;
			if (*has_qual) for (uint64_t i = 0; i < k; ++i) qual.push_back((char)(chunk[i] + 33));
			done += k;
		}
		const uint64_t n_aux = block_size - 32 - fields;
		if (keep == 0) { if (bam_need(r, 0, (size_t)n_aux)) return MM355_EIO; }
		else {
			if (n_aux > (uint64_t)INT32_MAX) return MM355_EIO;
			std::string raw;
			for (uint64_t done = 0; done < n_aux; ) {          // (in chunks, as the bases)
				const uint64_t k = n_aux - done < sizeof(chunk)? n_aux - done : sizeof(chunk);
				if (bam_need(r, chunk, (size_t)k)) return MM355_EIO;
				raw.append((const char*)chunk, (size_t)k);
				done += k;
			}
			aux.resize(raw.size());
			int32_t n_out = 0;
			if (bam_aux_split((const uint8_t*)raw.data(), (int32_t)raw.size(), keep, (uint8_t*)&aux[0], &n_out, aux_mod)) return MM355_EIO;
			aux.resize((size_t)n_out);
		}
		if (rev) {
			for (size_t i = start, j = seq.size(); i < j; ) {
				--j;
				const char a = (char)sam_comp((unsigned char)seq[j]), b = (char)sam_comp((unsigned char)seq[i]);
				seq[i] = a; if (i != j) seq[j] = b;
				++i;
			}
			for (size_t i = 0, j = qual.size(); i + 1 < j; ++i) { --j; const char x = qual[i]; qual[i] = qual[j]; qual[j] = x; }
		}
		return 1;
	}
}

template <typename R> static inline int bam_read_record(R &r, std::string &name, std::string &seq, std::string &qual, bool *has_qual)
{
	std::string aux; int32_t mod = 0;
	return bam_read_record(r, name, seq, qual, has_qual, (const char*)0, aux, &mod);
}

// a streaming reader of read sets (mm355_fastx_t) over a source it takes over: mm355_fastx_next, mm355_fastx_close as for mm355_fastx_open
struct mm355_fastx;
mm355_fastx *mm355_fastx_from_source(ByteSource *src, bool keep_qual);
