// mm355_samdev.h -- what the device writers of read-carrying records share (mm355_sam.hip: SAM text, mm355_bam.hip: BAM records): the batch
// result, the tables and the reads as the kernels see them, the host code that lays them out and uploads them, and the 16-byte piece of a
// copy whose source is not aligned with its destination.  Device code: included by the two .hip files only.
#pragma once
#include <stdio.h>
#include <algorithm>
#include "mm355_pipeline.h"
#include "mm355_sam.h"

struct SamDev {
	const mm355_hit_t *hits; const mm355_tags_t *tags; const uint32_t *cigar; const char *str;
	const int64_t *hit_off; const int32_t *qlen, *rep_len;            // per read
	const int64_t *qn_off; const char *qn;                            // per read: its name = qn[qn_off[r] .. qn_off[r + 1])
	const int64_t *seq_off, *qual_off; const char *bytes;             // per read: its bases and quality in bytes[]; qual_off < 0: none
	const char *tn; const int64_t *tn_off;                            // contig names
	const int32_t *l_read; const int64_t *l_first;                    // read of a line; first line of a read (n_reads + 1)
	int64_t n_lines; int sam_flags;
};

__device__ __forceinline__ SamRead sam_read_dev(const SamDev &D, int32_t r)
{
	SamRead R;
	const int64_t k0 = D.hit_off[r];
	R.rows = D.hits + k0; R.tags = D.tags + k0; R.n_rows = (int32_t)(D.hit_off[r + 1] - k0);
	R.qname = D.qn + D.qn_off[r]; R.qname_len = D.qn_off[r + 1] - D.qn_off[r]; R.qlen = D.qlen[r];
	R.seq = D.bytes + D.seq_off[r]; R.qual = D.qual_off[r] >= 0? D.bytes + D.qual_off[r] : 0;
	R.tn = D.tn; R.tn_off = D.tn_off; R.cigar = D.cigar; R.str = D.str;
	R.rep_len = D.rep_len[r]; R.sam_flags = D.sam_flags;
	return R;
}
__device__ __forceinline__ int32_t sam_row_of(const SamDev &D, int64_t l, int32_t r) { return D.hit_off[r + 1] > D.hit_off[r]? (int32_t)(l - D.l_first[r]) : -1; }

// 16 source bytes from src + s as four dwords, lowest address first: whole dwords around the span are read, at most 3 bytes before it and 4
// behind (the arenas are padded)
__device__ __forceinline__ void sam_load16(const char *src, int64_t s, uint32_t v[4])
{
	const uintptr_t ps = (uintptr_t)(src + s);
	const uint32_t *pa = (const uint32_t*)(ps & ~(uintptr_t)3);
	const int sh = (int)(ps & 3) * 8;
	uint32_t w[5];
	for (int k = 0; k < 5; ++k) w[k] = pa[k];
	for (int k = 0; k < 4; ++k) v[k] = (uint32_t)(((uint64_t)w[k + 1] << 32 | w[k]) >> sh);
}
// the same four dwords with the last byte first: mirrored dword order, bytes swapped within the dword
__device__ __forceinline__ void sam_mirror16(uint32_t v[4])
{
	const uint32_t a = __builtin_bswap32(v[3]), b = __builtin_bswap32(v[2]), c = __builtin_bswap32(v[1]), d = __builtin_bswap32(v[0]);
	v[0] = a; v[1] = b; v[2] = c; v[3] = d;
}

// 16 output bytes of a run from 16 source bytes: s = the source index of the lowest of them; mode bit 0: last byte first, bit 1: complemented
__device__ __forceinline__ uint4 sam_piece(const char *src, int64_t s, int mode, const unsigned char *comp)
{
	uint32_t v[4];
	sam_load16(src, s, v);
	if (mode & 1) sam_mirror16(v);
	if (mode & 2)
		for (int k = 0; k < 4; ++k)
			v[k] = (uint32_t)comp[v[k] & 0xff] | (uint32_t)comp[v[k] >> 8 & 0xff] << 8 | (uint32_t)comp[v[k] >> 16 & 0xff] << 16 | (uint32_t)comp[v[k] >> 24] << 24;
	return make_uint4(v[0], v[1], v[2], v[3]);
}

// ------------------------------------------------------------------ host side
static inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

// Lays out what the host makes (the lines, the query names as the record prints them, where every read's bases and quality go), uploads it
// with the batch result into c->sam_in and fills D.  D->n_lines == 0 on return: nothing was uploaded, there is nothing to launch.
// *t_packed: the host clock when the packing was done (MM355_SAM_TIMES).
static int sam_upload(mm355_ctx *c, const mm355_hits_t *H, const char *const *qnames, const char *const *seqs, const int32_t *qlens,
                      const char *const *quals, const int32_t *rep_len, int sam_flags, SamDev *Dp, double *t_packed)
{
	SamDev &D = *Dp;
	const int64_t nh = H->n_hits, nr = H->n_reads;
	std::vector<int64_t> n_line((size_t)nr), qn_len((size_t)nr);
	int64_t nl = 0, qn_tot = 0, by_tot = 0;
	for (int64_t i = 0; i < nr; ++i) {
		n_line[i] = mm355_sam_n_lines(H, qlens, sam_flags, i);
		nl += n_line[i];
		qn_len[i] = n_line[i] == 0? 0 : qnames && qnames[i]? paf_qname_len(qnames[i]) : 1;
		qn_tot += qn_len[i];
		if (n_line[i]) by_tot += (int64_t)qlens[i] * (quals && quals[i]? 2 : 1);
	}
	D.n_lines = nl; D.sam_flags = sam_flags;
	*t_packed = mm355_now_ms();
	if (nl == 0) return 0;
	if (nl > (int64_t)INT32_MAX / 2 || nr > (int64_t)INT32_MAX) return MM355_EINVAL;
	HIPCHK(hipSetDevice(c->dev));
	const char *d_tn = 0; const int64_t *d_tn_off = 0;
	if (int rc = mm355_replica_tnames(c->mi, c->dev, &d_tn, &d_tn_off)) return rc;
	const size_t nc = H->n_cigar > 0? (size_t)H->n_cigar : 0, ns = H->n_str > 0? (size_t)H->n_str : 0;
	// one device buffer; one pinned staging buffer for the parts made here (the tables, the names, the reads and qualities back to back)
	const size_t o_hits = 0, o_tags = o_hits + up256((size_t)nh * sizeof(mm355_hit_t) + 8), o_cig = o_tags + up256((size_t)nh * sizeof(mm355_tags_t) + 8),
	             o_str = o_cig + up256(nc * 4 + 4), o_qlen = o_str + up256(ns + 4), o_hoff = o_qlen + up256((size_t)nr * 4), o_made = o_hoff + up256((size_t)(nr + 1) * 8);
	const size_t m_lread = 0, m_lfirst = m_lread + up256((size_t)nl * 4), m_rep = m_lfirst + up256((size_t)(nr + 1) * 8), m_qoff = m_rep + up256((size_t)nr * 4),
	             m_soff = m_qoff + up256((size_t)(nr + 1) * 8), m_uoff = m_soff + up256((size_t)nr * 8), m_qn = m_uoff + up256((size_t)nr * 8),
	             m_by = m_qn + up256((size_t)qn_tot + 4), m_end = m_by + up256((size_t)by_tot + 64);   // (64: the copy kernels read whole dwords around a span)
	if (c->sam_in.ensure(o_made + m_end) || c->h_sam_in.ensure(m_end) || c->h_sam_out.ensure(64, 1 << 20)) return MM355_ENOMEM;
	char *hm = (char*)c->h_sam_in.p, *din = (char*)c->sam_in.p;
	int32_t *l_read = (int32_t*)(hm + m_lread), *rl = (int32_t*)(hm + m_rep);
	int64_t *l_first = (int64_t*)(hm + m_lfirst), *qoff = (int64_t*)(hm + m_qoff), *soff = (int64_t*)(hm + m_soff), *uoff = (int64_t*)(hm + m_uoff);
	char *qn = hm + m_qn, *by = hm + m_by;
	int64_t at = 0, bat = 0, lat = 0;
	for (int64_t i = 0; i < nr; ++i) {
		l_first[i] = lat;
		for (int64_t j = 0; j < n_line[i]; ++j) l_read[lat++] = (int32_t)i;
		rl[i] = rep_len && H->hit_off[i + 1] == H->hit_off[i]? rep_len[i] : 0;
		qoff[i] = at;
		if (qn_len[i] > 0) memcpy(qn + at, qnames && qnames[i]? qnames[i] : "*", (size_t)qn_len[i]);
		at += qn_len[i];
		soff[i] = 0; uoff[i] = -1;
		if (n_line[i]) {
			soff[i] = bat; memcpy(by + bat, seqs[i], (size_t)qlens[i]); bat += qlens[i];
			if (quals && quals[i]) { uoff[i] = bat; memcpy(by + bat, quals[i], (size_t)qlens[i]); bat += qlens[i]; }
		}
	}
	l_first[nr] = lat; qoff[nr] = at;
	memset(by + bat, 0, 64);
	*t_packed = mm355_now_ms();
	hipStream_t st = c->st;
	if (nh) {
		HIPCHK(hipMemcpyAsync(din + o_hits, H->hits, (size_t)nh * sizeof(mm355_hit_t), hipMemcpyHostToDevice, st));
		HIPCHK(hipMemcpyAsync(din + o_tags, H->tags, (size_t)nh * sizeof(mm355_tags_t), hipMemcpyHostToDevice, st));
	}
	if (nc) HIPCHK(hipMemcpyAsync(din + o_cig, H->cigar, nc * 4, hipMemcpyHostToDevice, st));
	if (ns) HIPCHK(hipMemcpyAsync(din + o_str, H->str, ns, hipMemcpyHostToDevice, st));
	HIPCHK(hipMemcpyAsync(din + o_qlen, qlens, (size_t)nr * 4, hipMemcpyHostToDevice, st));
	HIPCHK(hipMemcpyAsync(din + o_hoff, H->hit_off, (size_t)(nr + 1) * 8, hipMemcpyHostToDevice, st));
	HIPCHK(hipMemcpyAsync(din + o_made, hm, m_by + (size_t)bat + 64, hipMemcpyHostToDevice, st));
	D.hits = (const mm355_hit_t*)(din + o_hits); D.tags = (const mm355_tags_t*)(din + o_tags); D.cigar = (const uint32_t*)(din + o_cig); D.str = din + o_str;
	D.hit_off = (const int64_t*)(din + o_hoff); D.qlen = (const int32_t*)(din + o_qlen); D.rep_len = (const int32_t*)(din + o_made + m_rep);
	D.qn_off = (const int64_t*)(din + o_made + m_qoff); D.qn = din + o_made + m_qn;
	D.seq_off = (const int64_t*)(din + o_made + m_soff); D.qual_off = (const int64_t*)(din + o_made + m_uoff); D.bytes = din + o_made + m_by;
	D.tn = d_tn; D.tn_off = d_tn_off;
	D.l_read = (const int32_t*)(din + o_made + m_lread); D.l_first = (const int64_t*)(din + o_made + m_lfirst);
	return 0;
}

// the result of a call that writes nothing
static int sam_text_empty(int64_t nr, mm355_text_t **out)
{
	mm355_text_t *T = mm355_text_alloc(nr, 0, 0);
	if (T == 0) return MM355_ENOMEM;
	for (int64_t i = 0; i <= nr; ++i) T->line_off[i] = 0;
	*out = T;
	return 0;
}
