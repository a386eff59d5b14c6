// mm355_bammerge.h -- one step of the merge of COMPRESSED runs, stated once (include/mm355.h repeats it field by field): the records of a
// step lie in BGZF members of a memory-mapped spool; the step inflates the members it needs, copies the records in merged order behind the
// bytes the last step left over, and frames or deflates every whole payload of the result.  Here: the plan of a step (checks, the walk over
// the members, where every record lies in the inflated bytes), the step on the host, and the packing of a run the host formed.  The device
// step (mm355_bam.hip: k_bgzf_inflate, k_rec_gather, the deflate or framing kernels) runs the same plan and must give the same bytes.
// Plain C++ (tests/host_harness/bammerge_host.cpp builds it with g++ alone).
#pragma once
#include "mm355_bamsort.h"
#include "mm355_bgzfwalk.h"
#include "mm355_inflate.h"
#include "mm355_deflate.h"

// what a step was given (mm355_bam_merge_step's arguments)
struct BamMergeIn {
	const void *base; int64_t base_len;
	const int64_t *slice_at, *slice_bytes, *slice_raw_at; int64_t n_slice;
	const int32_t *rec_slice; const int64_t *rec_at, *rec_len; int64_t n_rec;
	const void *carry; int64_t n_carry;
	int final, level;
};

// what follows from it before a byte moves
struct BamMergePlan {
	std::vector<BgzfMember> mem;         // the members of all slices: c_off counts from `base`, o_off is the payload's place in the inflated bytes
	std::vector<int64_t> slice_base;     // n_slice + 1: where a slice's first payload byte lies in the inflated bytes
	std::vector<int64_t> slice_mem;      // n_slice + 1: a slice's first member in mem
	std::vector<int64_t> src;            // per record: its place in the inflated bytes
	int64_t n_in = 0, n_inflated = 0, n_rec_bytes = 0, n_stream = 0, n_now = 0, n_left = 0;
};

// MM355_EINVAL for arguments that cannot be a step, MM355_EIO for a slice that is not whole BGZF members; 0 and the plan
inline int bam_merge_plan(const BamMergeIn &a, BamMergePlan &p)
{
	if (a.base_len < 0 || a.n_slice < 0 || a.n_rec < 0 || a.n_carry < 0 || a.n_carry >= BGZF_PAYLOAD || a.level < 0 || a.level > 1) return MM355_EINVAL;
	if ((a.n_slice > 0 && (a.slice_at == 0 || a.slice_bytes == 0 || a.slice_raw_at == 0)) || (a.n_rec > 0 && (a.rec_slice == 0 || a.rec_at == 0 || a.rec_len == 0)) ||
	    (a.n_carry > 0 && a.carry == 0) || a.n_slice > (int64_t)INT32_MAX || a.n_rec > (int64_t)INT32_MAX) return MM355_EINVAL;
	for (int64_t s = 0; s < a.n_slice; ++s) {
		if (a.slice_at[s] < 0 || a.slice_bytes[s] < 0 || a.slice_raw_at[s] < 0 || a.slice_at[s] > a.base_len || a.slice_bytes[s] > a.base_len - a.slice_at[s]) return MM355_EINVAL;
		if (a.slice_bytes[s] > 0 && a.base == 0) return MM355_EINVAL;
	}
	for (int64_t i = 0; i < a.n_rec; ++i)
		if (a.rec_slice[i] < 0 || a.rec_slice[i] >= a.n_slice || a.rec_at[i] < 0 || a.rec_len[i] < 0) return MM355_EINVAL;
	p.mem.clear(); p.slice_base.assign((size_t)a.n_slice + 1, 0); p.slice_mem.assign((size_t)a.n_slice + 1, 0); p.src.assign((size_t)a.n_rec, 0);
	p.n_in = 0; p.n_inflated = 0;
	for (int64_t s = 0; s < a.n_slice; ++s) {
		p.slice_base[(size_t)s] = p.n_inflated;
		const size_t m0 = p.mem.size();
		p.slice_mem[(size_t)s] = (int64_t)m0;
		int64_t used = 0;
		if (a.slice_bytes[s] > 0) {
			if (bgzf_walk((const unsigned char*)a.base + a.slice_at[s], a.slice_bytes[s], false, true, p.mem, &used, &p.n_inflated)) return MM355_EIO;
			if (used != a.slice_bytes[s]) return MM355_EIO;
		}
		for (size_t m = m0; m < p.mem.size(); ++m) p.mem[m].c_off += a.slice_at[s];
		p.n_in += a.slice_bytes[s];
	}
	p.slice_base[(size_t)a.n_slice] = p.n_inflated; p.slice_mem[(size_t)a.n_slice] = (int64_t)p.mem.size();
	if (p.mem.size() > (size_t)INT32_MAX) return MM355_EINVAL;
	p.n_rec_bytes = 0;
	for (int64_t i = 0; i < a.n_rec; ++i) {
		const int64_t s = a.rec_slice[i], room = p.slice_base[(size_t)s + 1] - p.slice_base[(size_t)s], at = a.rec_at[i] - a.slice_raw_at[s];
		if (at < 0 || at > room || a.rec_len[i] > room - at) return MM355_EINVAL;
		p.src[(size_t)i] = p.slice_base[(size_t)s] + at;
		p.n_rec_bytes += a.rec_len[i];
	}
	p.n_stream = a.n_carry + p.n_rec_bytes;
	p.n_now = a.final? p.n_stream : p.n_stream / BGZF_PAYLOAD * BGZF_PAYLOAD;
	p.n_left = p.n_stream - p.n_now;
	return 0;
}

// the blocks of n bytes at `raw` as a text: stored (level 0) or deflated where that is shorter (level 1); n_lines counts the blocks
inline int bam_merge_blocks_host(const char *raw, int64_t n, int level, mm355_text_t **out)
{
	if (int rc = mm355_bgzf_wrap_host(raw, n, out)) return rc;
	if (level && n) {
		std::vector<char> z((size_t)bgzf_size(n) + 1);
		const int64_t n_out = mm355_bgzf_deflate_host(raw, n, z.data());
		memcpy((*out)->text, z.data(), (size_t)n_out);
		(*out)->n_text = n_out; (*out)->text[n_out] = 0;
	}
	return 0;
}

// the step on the host: the planned members inflated one after the other, the records copied (bam_gather's loop), the whole payloads framed
// or deflated, the rest to carry_out (room for BGZF_PAYLOAD bytes; it may be the buffer `carry` points to)
inline int bam_merge_step_host(const BamMergeIn &a, const BamMergePlan &p, mm355_text_t **out, void *carry_out, int64_t *n_carry_out)
{
	std::vector<unsigned char> inf((size_t)p.n_inflated + 1);
	std::vector<InfHost> S(1);
	for (const BgzfMember &m : p.mem)
		if (inf_member_host((const unsigned char*)a.base + m.c_off, m.c_len, m.isize, m.crc, inf.data() + m.o_off, S[0])) return MM355_EIO;
	std::vector<char> stream((size_t)p.n_stream + 1);
	if (a.n_carry) memcpy(stream.data(), a.carry, (size_t)a.n_carry);
	if (int rc = bam_gather(inf.data(), p.n_inflated, p.src.data(), a.rec_len, a.n_rec, stream.data() + a.n_carry, p.n_rec_bytes)) return rc;
	if (int rc = bam_merge_blocks_host(stream.data(), p.n_now, a.level, out)) return rc;
	if (p.n_left) memcpy(carry_out, stream.data() + p.n_now, (size_t)p.n_left);
	*n_carry_out = p.n_left;
	return 0;
}

// a run the host formed, packed as the device packs one: rec becomes the BGZF members of the unframed stream (the serial coder: the same
// bytes), n_bytes their count, blk_off their n_blk + 1 offsets; rec_off stays as it is
inline int bam_run_pack_host(mm355_run_t *R)
{
	const int64_t raw = R->n_bytes, nb = bgzf_blocks(raw);
	char *z = (char*)malloc((size_t)bgzf_size(raw) + 1);
	int64_t *bo = (int64_t*)malloc((size_t)(nb + 1) * 8);
	if (z == 0 || bo == 0) { free(z); free(bo); return MM355_ENOMEM; }
	const int64_t n_out = raw? mm355_bgzf_deflate_host(R->rec, raw, z) : 0;
	int64_t at = 0;
	for (int64_t b = 0; b < nb; ++b) { bo[b] = at; at += (int64_t)bgzf_le16((const unsigned char*)z + at + 16) + 1; }   // (the coder's own BSIZE)
	bo[nb] = at;
	if (at != n_out) { free(z); free(bo); return MM355_EINVAL; }
	z[n_out] = 0;
	free(R->rec);
	R->rec = z; R->n_bytes = n_out; R->n_blk = nb; R->blk_off = bo; R->packed = 1;
	return 0;
}
