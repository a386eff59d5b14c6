// mm355_bai.h -- the .bai index of a coordinate-sorted BAM file, stated once: the span of a record on the reference (the only part that
// reads record bytes: a sum over the CIGAR words), and the builder, which takes keys, spans, lengths and the BGZF blocks as they were written
// and never a record.  include/mm355.h repeats the rule field by field.
// The span's pieces (bam_span_words, bam_cigar_ref_len, bam_span_of) are what k_rec_span (mm355_bam.hip) calls with a wave per record, so the
// host and the device cannot disagree.  Plain C++ that also compiles as device code where marked (tests/host_harness/bai_host.cpp builds it
// with g++ alone).
#pragma once
#include <map>
#include <string>
#include "mm355_bamsort.h"
#include "mm355_bgzfwalk.h"

#define BAI_MAX_END ((int64_t)1 << 29)   // the last coordinate a .bai can hold: six levels, 16 kb windows at the lowest
#define BAI_PSEUDO_BIN 37450u            // samtools' bin of a contig's own numbers: its file range and its record counts
#define BAI_WINDOW 14                    // the linear index has a window per 2^14 bases

// ------------------------------------------------------------------ the span of a record
// the fixed fields the span needs: l_read_name at 12, n_cigar_op at 16, flag at 18 (byte loads: a record starts anywhere)
MM_HD uint32_t bam_rec_l_name(const uint8_t *rec) { return rec[12]; }
MM_HD uint32_t bam_rec_n_cigar(const uint8_t *rec) { return (uint32_t)rec[16] | (uint32_t)rec[17] << 8; }
MM_HD uint32_t bam_rec_flag(const uint8_t *rec) { return (uint32_t)rec[18] | (uint32_t)rec[19] << 8; }
// the reference bases of one CIGAR word: its length for M D N = X (0 2 3 7 8), nothing for every other op code, 9 to 15 included
MM_HD uint64_t bam_cigar_ref_len(uint32_t w) { return (0x18du >> (w & 15u) & 1u)? (uint64_t)(w >> 4) : 0; }
// the words that are summed: none for an unmapped record (flag & 4), whatever CIGAR it carries
MM_HD uint32_t bam_span_words(uint32_t flag, uint32_t n_cigar) { return (flag & 4u)? 0u : n_cigar; }
// end = pos + max(1, reflen) (the writer's rule for `bin`, htslib's bam_endpos), and the unmapped bit below it
MM_HD int64_t bam_span_of(int32_t pos, uint32_t flag, uint64_t reflen)
{
	const int64_t end = (int64_t)pos + (int64_t)(reflen > 0? reflen : 1);
	return (int64_t)((uint64_t)end << 1 | (flag >> 2 & 1u));
}
// what the host checks before anything is launched: the fixed part and the words lie inside the record's len bytes
MM_HD bool bam_span_fits(const uint8_t *rec, int64_t len)
{
	return len >= 36 && 36 + (int64_t)bam_rec_l_name(rec) + 4 * (int64_t)bam_rec_n_cigar(rec) <= len;
}
// rec: a record with its block_size word, at any address; reads nothing outside [rec, rec + len) (the caller has asked bam_span_fits).
// The long-CIGAR form needs no case: its two placeholder words `l_seq S, reflen N` sum to reflen, and the CG tag is not read.
MM_HD int64_t bam_rec_span(const uint8_t *rec, int64_t len)
{
	(void)len;
	const uint32_t flag = bam_rec_flag(rec), n = bam_span_words(flag, bam_rec_n_cigar(rec));
	const uint8_t *w = rec + 36 + bam_rec_l_name(rec);
	uint64_t reflen = 0;
	for (uint32_t i = 0; i < n; ++i) reflen += bam_cigar_ref_len(bam_rec_u32(w + 4 * (size_t)i));
	return bam_span_of((int32_t)bam_rec_u32(rec + 8), flag, reflen);
}
// every record of a checked stream (bam_sort_check) against bam_span_fits
inline int bam_span_check(const void *rec, const int64_t *rec_off, int64_t n_rec)
{
	for (int64_t i = 0; i < n_rec; ++i)
		if (!bam_span_fits((const uint8_t*)rec + rec_off[i], rec_off[i + 1] - rec_off[i])) return MM355_EINVAL;
	return 0;
}
inline void bam_span_host(const void *rec, const int64_t *rec_off, int64_t n_rec, int64_t *span)
{
	for (int64_t i = 0; i < n_rec; ++i) span[i] = bam_rec_span((const uint8_t*)rec + rec_off[i], rec_off[i + 1] - rec_off[i]);
}
// mm355_bam_sort_span on the host: the serial sort, then the spans of the sorted records.  The stream has passed bam_span_check.
inline int bam_sort_run_span_host(const void *rec, int64_t n_bytes, const int64_t *rec_off, int64_t n_rec, mm355_run_t **out)
{
	if (int rc = bam_sort_run_host(rec, n_bytes, rec_off, n_rec, out, true)) return rc;
	bam_span_host((*out)->rec, (*out)->rec_off, n_rec, (*out)->span);
	return 0;
}

// ------------------------------------------------------------------ the index
// SAM v1 section 5.3; beg < end <= 2^29
inline uint32_t bai_reg2bin(int64_t beg, int64_t end)
{
	--end;
	if (beg >> 14 == end >> 14) return (uint32_t)(4681 + (beg >> 14));
	if (beg >> 17 == end >> 17) return (uint32_t)(585 + (beg >> 17));
	if (beg >> 20 == end >> 20) return (uint32_t)(73 + (beg >> 20));
	if (beg >> 23 == end >> 23) return (uint32_t)(9 + (beg >> 23));
	if (beg >> 26 == end >> 26) return (uint32_t)(1 + (beg >> 26));
	return 0;
}

struct BaiChunk { uint64_t beg, end; };
struct BaiRec { int32_t ref, beg, end, unmapped; };

struct BaiBuilder {
	int32_t n_ref = 0;
	int64_t first_block_at = 0;
	bool any_key = false;
	uint64_t last_key = 0;
	int64_t n_no_coor = 0, n_bytes = 0;
	std::vector<BaiRec> rec;                 // the placed records, file order
	std::vector<int64_t> starts, ends;       // u_i and u_{i+1} of the placed records: their place in the unframed stream
	std::vector<int64_t> c_end, i_end;       // per block: the compressed bytes and the ISIZEs up to and including it
	int64_t n_raw_chunks = 0, n_chunks = 0;  // finish(): the chunks of the bins before and after the finishing merges

	// n records in file order: keys (mm355_bamsort.h), spans (bam_rec_span), lengths.  All n are checked before one is taken.
	int records(const uint64_t *key, const int64_t *span, const int64_t *len, int64_t n)
	{
		if (n < 0 || (n > 0 && (key == 0 || span == 0 || len == 0))) return MM355_EINVAL;
		uint64_t lk = last_key; bool ak = any_key;
		for (int64_t i = 0; i < n; ++i) {
			if (ak && key[i] < lk) return MM355_EINVAL;                  // an unsorted stream has no index
			lk = key[i]; ak = true;
			if (len[i] < BAM_SORT_MIN_RECORD) return MM355_EINVAL;
			const int32_t ref = (int32_t)(uint32_t)(key[i] >> 32);
			if (ref < 0) continue;
			const int64_t beg = (int64_t)((uint32_t)key[i] >> 1) - 1, end = span[i] >> 1;
			if (ref >= n_ref || beg < 0 || end <= beg || end > BAI_MAX_END) return MM355_EINVAL;
		}
		for (int64_t i = 0; i < n; ++i) {
			const int32_t ref = (int32_t)(uint32_t)(key[i] >> 32);
			if (ref < 0) ++n_no_coor;
			else {
				BaiRec r = { ref, (int32_t)(((uint32_t)key[i] >> 1) - 1), (int32_t)(span[i] >> 1), (int32_t)(span[i] & 1) };
				rec.push_back(r);
				starts.push_back(n_bytes); ends.push_back(n_bytes + len[i]);
			}
			n_bytes += len[i];
		}
		last_key = lk; any_key = ak;
		return 0;
	}

	// n bytes of whole BGZF blocks, as they were written behind the ones before
	int blocks(const void *bytes, int64_t n)
	{
		if (n < 0 || (n > 0 && bytes == 0)) return MM355_EINVAL;
		std::vector<int64_t> c, s;
		int64_t ce = c_end.empty()? 0 : c_end.back(), ie = i_end.empty()? 0 : i_end.back();
		for (int64_t at = 0; at < n; ) {
			BgzfMember m;
			const int64_t sz = bgzf_member((const unsigned char*)bytes, n, at, &m);
			if (sz <= 0) return MM355_EINVAL;                            // no member, or one the bytes end in
			ce += sz; ie += m.isize; at += sz;
			c.push_back(ce); s.push_back(ie);
		}
		c_end.insert(c_end.end(), c.begin(), c.end());
		i_end.insert(i_end.end(), s.begin(), s.end());
		return 0;
	}

	// V(u): the first block that holds byte u of the stream -- blocks of ISIZE 0 are passed over -- and the offset inside it; for u the
	// stream's length one past the last block, offset 0
	uint64_t voffset(int64_t at) const
	{
		const size_t b = (size_t)(std::upper_bound(i_end.begin(), i_end.end(), at) - i_end.begin());
		const int64_t c0 = first_block_at + (b? c_end[b - 1] : 0), i0 = b? i_end[b - 1] : 0;
		return (uint64_t)c0 << 16 | (uint64_t)(at - i0);
	}

	static void put32(std::string &o, uint32_t v) { for (int k = 0; k < 4; ++k) o.push_back((char)(v >> 8 * k)); }
	static void put64(std::string &o, uint64_t v) { for (int k = 0; k < 8; ++k) o.push_back((char)(v >> 8 * k)); }

	// one contig's records [a, b) of rec: bins, the finishing by level, the linear index
	void finish_ref(size_t a, size_t b, std::string &o)
	{
		if (a == b) { put32(o, 0); put32(o, 0); return; }
		std::map<uint32_t, std::vector<BaiChunk>> bins;
		std::vector<uint64_t> iv;
		const uint64_t none = ~(uint64_t)0;
		uint64_t n_map = 0, n_unmap = 0;
		uint32_t run_bin = 0; bool in_run = false;
		for (size_t i = a; i < b; ++i) {
			const BaiRec &r = rec[i];
			const uint64_t vb = voffset(starts[i]), ve = voffset(ends[i]);
			const uint32_t bin = bai_reg2bin(r.beg, r.end);
			if (in_run && bin == run_bin) bins[bin].back().end = ve;     // hts_idx_push's rule: a maximal run of records of one bin
			else { bins[bin].push_back(BaiChunk{ vb, ve }); run_bin = bin; in_run = true; ++n_raw_chunks; }
			const size_t w0 = (size_t)(r.beg >> BAI_WINDOW), w1 = (size_t)((r.end - 1) >> BAI_WINDOW);
			if (iv.size() <= w1) iv.resize(w1 + 1, none);
			for (size_t w = w0; w <= w1; ++w) if (iv[w] == none) iv[w] = vb;   // (file order: the first record that touches w)
			if (r.unmapped) ++n_unmap; else ++n_map;
		}
		for (size_t w = iv.size(); w-- > 0; ) if (iv[w] == none) iv[w] = iv[w + 1];   // (the last window is a touched one)
		// by level, 5 down to 1, bins ascending: a bin whose chunks lie within 64 KB of the file goes into its parent
		static const uint32_t first[7] = { 0, 1, 9, 73, 585, 4681, 37449 };
		for (int l = 5; l >= 1; --l)
			for (auto it = bins.lower_bound(first[l]); it != bins.end() && it->first < first[l + 1]; ) {
				uint64_t lo = none, hi = 0;
				for (const BaiChunk &c : it->second) { lo = std::min(lo, c.beg); hi = std::max(hi, c.end); }
				if ((int64_t)(hi >> 16) - (int64_t)(lo >> 16) < 0x10000) {
					std::vector<BaiChunk> &p = bins[(it->first - 1) >> 3];   // (a lower key: the iteration does not meet it on this level)
					p.insert(p.end(), it->second.begin(), it->second.end());
					it = bins.erase(it);
				} else ++it;
			}
		put32(o, (uint32_t)bins.size() + 1);
		for (auto &kv : bins) {
			std::vector<BaiChunk> &c = kv.second;
			std::sort(c.begin(), c.end(), [](const BaiChunk &x, const BaiChunk &y) { return x.beg != y.beg? x.beg < y.beg : x.end < y.end; });
			size_t m = 0;
			for (size_t i = 1; i < c.size(); ++i)
				if (c[i].beg >> 16 <= c[m].end >> 16) c[m].end = std::max(c[m].end, c[i].end);
				else c[++m] = c[i];
			c.resize(m + 1);
			n_chunks += (int64_t)c.size();
			put32(o, kv.first); put32(o, (uint32_t)c.size());
			for (const BaiChunk &x : c) { put64(o, x.beg); put64(o, x.end); }
		}
		put32(o, BAI_PSEUDO_BIN); put32(o, 2);
		put64(o, voffset(starts[a])); put64(o, voffset(ends[b - 1])); put64(o, n_map); put64(o, n_unmap);
		put32(o, (uint32_t)iv.size());
		for (uint64_t v : iv) put64(o, v);
	}

	// the file's bytes (SAM v1 section 5.2).  The blocks must hold exactly the records' bytes.
	int finish(std::string &o)
	{
		if ((i_end.empty()? 0 : i_end.back()) != n_bytes) return MM355_EINVAL;
		o.clear(); n_raw_chunks = n_chunks = 0;
		o.append("BAI\1", 4); put32(o, (uint32_t)n_ref);
		size_t a = 0;
		for (int32_t r = 0; r < n_ref; ++r) {
			size_t b = a;
			while (b < rec.size() && rec[b].ref == r) ++b;
			finish_ref(a, b, o);
			a = b;
		}
		put64(o, (uint64_t)n_no_coor);
		return 0;
	}
};
