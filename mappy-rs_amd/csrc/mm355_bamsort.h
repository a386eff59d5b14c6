// mm355_bamsort.h -- the coordinate order of BAM records, stated once: the key of a record, the serial sort of a stream of records, the check
// of a caller's stream and the copy loop of the file merge.  The device sort (mm355_bam.hip: k_rec_key, rocPRIM's radix sort, k_rec_permute)
// computes the same key with the same function and must give the same bytes as bam_sort_host.
// The order is samtools': contigs in header order, inside a contig by position, at one position forward before reverse, records without a
// contig (refID -1) last -- and records of equal key KEEP THEIR INPUT ORDER, so that the sorted stream is the stable sort of the unsorted
// one and does not depend on how the input was cut into calls.
// Plain C++ that also compiles as device code (tests/host_harness/bamsort_host.cpp builds it with g++ alone).
#pragma once
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "../../include/mm355.h"

#ifndef MM_HD
#if defined(__HIPCC__)
#define MM_HD __host__ __device__ inline
#else
#define MM_HD inline
#endif
#endif

#define BAM_SORT_MIN_RECORD 37      // block_size, the 32 fixed bytes and a read name of one NUL at least

MM_HD uint32_t bam_rec_u32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// rec: a record with its block_size word, at any address (byte loads).  refID at 4, pos at 8, flag at 18.
MM_HD uint64_t bam_sort_key(const uint8_t *rec)
{
	const uint32_t refid = bam_rec_u32(rec + 4), pos = bam_rec_u32(rec + 8), flag = (uint32_t)rec[18] | (uint32_t)rec[19] << 8;
	return (uint64_t)refid << 32 | (uint32_t)((pos + 1u) << 1) | (flag >> 4 & 1u);
}

// the stream of n_rec records in the n_bytes at rec: offsets ascend from 0 to n_bytes, every piece is a whole record
inline int bam_sort_check(const void *rec, int64_t n_bytes, const int64_t *rec_off, int64_t n_rec)
{
	if (n_rec < 0 || n_bytes < 0 || (n_rec > 0 && (rec == 0 || rec_off == 0)) || n_rec > (int64_t)INT32_MAX) return MM355_EINVAL;
	if (n_rec == 0) return n_bytes == 0? 0 : MM355_EINVAL;
	if (rec_off[0] != 0 || rec_off[n_rec] != n_bytes) return MM355_EINVAL;
	for (int64_t i = 0; i < n_rec; ++i) {
		const int64_t a = rec_off[i], b = rec_off[i + 1];
		if (a < 0 || b > n_bytes || b - a < BAM_SORT_MIN_RECORD) return MM355_EINVAL;       // (also b <= a)
		if ((int64_t)bam_rec_u32((const uint8_t*)rec + a) + 4 != b - a) return MM355_EINVAL;
	}
	return 0;
}

// the serial sort: key[] ascending, out_off[] the n_rec + 1 new offsets, out the records in that order.  The stream has passed bam_sort_check.
inline void bam_sort_host(const void *rec, const int64_t *rec_off, int64_t n_rec, uint64_t *key, int64_t *out_off, char *out)
{
	std::vector<uint64_t> k((size_t)n_rec);
	std::vector<int64_t> idx((size_t)n_rec);
	for (int64_t i = 0; i < n_rec; ++i) { k[(size_t)i] = bam_sort_key((const uint8_t*)rec + rec_off[i]); idx[(size_t)i] = i; }
	std::stable_sort(idx.begin(), idx.end(), [&](int64_t a, int64_t b) { return k[(size_t)a] < k[(size_t)b]; });
	int64_t at = 0;
	for (int64_t j = 0; j < n_rec; ++j) {
		const int64_t i = idx[(size_t)j], l = rec_off[i + 1] - rec_off[i];
		key[j] = k[(size_t)i]; out_off[j] = at;
		memcpy(out + at, (const char*)rec + rec_off[i], (size_t)l);
		at += l;
	}
	out_off[n_rec] = at;
}

// mm355_bam_gather (include/mm355.h): n pieces of base, back to back into out; every piece and the total are checked before a byte moves
inline int bam_gather(const void *base, int64_t base_len, const int64_t *src_off, const int64_t *len, int64_t n, void *out, int64_t out_cap)
{
	if (n < 0 || base_len < 0 || out_cap < 0 || (n > 0 && (src_off == 0 || len == 0))) return MM355_EINVAL;
	int64_t tot = 0;
	for (int64_t i = 0; i < n; ++i) {
		if (len[i] < 0 || src_off[i] < 0 || src_off[i] > base_len || len[i] > base_len - src_off[i]) return MM355_EINVAL;
		if (len[i] > out_cap - tot) return MM355_EINVAL;
		tot += len[i];
	}
	if (tot > 0 && (base == 0 || out == 0)) return MM355_EINVAL;
	char *o = (char*)out;
	for (int64_t i = 0; i < n; ++i) { if (len[i]) memcpy(o, (const char*)base + src_off[i], (size_t)len[i]); o += len[i]; }
	return 0;
}

// ---- the result record (mm355_run_t): three arrays of the host's, and the spans (mm355_bai.h) where a call asked for them
inline void mm355_free_run_host(mm355_run_t *r) { if (r) { free(r->key); free(r->rec_off); free(r->rec); free(r->span); free(r->blk_off); free(r); } }
inline mm355_run_t *mm355_run_alloc(int64_t n_rec, int64_t n_bytes, bool span = false)
{
	mm355_run_t *R = (mm355_run_t*)calloc(1, sizeof(mm355_run_t));
	if (R == 0) return 0;
	R->n_rec = n_rec; R->n_bytes = n_bytes;
	R->key = (uint64_t*)malloc((size_t)(n_rec > 0? n_rec : 1) * 8);
	R->rec_off = (int64_t*)malloc((size_t)(n_rec + 1) * 8);
	R->rec = (char*)malloc((size_t)n_bytes + 1);
	if (span) R->span = (int64_t*)malloc((size_t)(n_rec > 0? n_rec : 1) * 8);
	if (R->key == 0 || R->rec_off == 0 || R->rec == 0 || (span && R->span == 0)) { mm355_free_run_host(R); return 0; }
	R->rec_off[0] = 0; R->rec[n_bytes] = 0;
	return R;
}

// mm355_bam_sort on the host
inline int bam_sort_run_host(const void *rec, int64_t n_bytes, const int64_t *rec_off, int64_t n_rec, mm355_run_t **out, bool span = false)
{
	mm355_run_t *R = mm355_run_alloc(n_rec, n_bytes, span);
	if (R == 0) return MM355_ENOMEM;
	if (n_rec > 0) bam_sort_host(rec, rec_off, n_rec, R->key, R->rec_off, R->rec);
	*out = R;
	return 0;
}
