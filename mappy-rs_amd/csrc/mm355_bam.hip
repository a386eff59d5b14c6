// mm355_bam.hip -- the BAM records of a batch result and their BGZF framing, written on the device.  The record is stated once, in
// mm355_bam.h (bam_emit_record); the device record writer of mm355_recdev.h runs it, a wave per record.  What is BAM's own: the lanes sum
// the reference length of the CIGAR (the bin needs it); the fixed fields and the tags go straight to the stream byte by byte; the CIGAR
// and the CG words are runs the wave copies as they lie; SEQ and QUAL are noted down as runs and packed by
//   k_bam_bulk    work item = (record, field, tile of BAM_TILE output bytes), one block each.  A thread owns an aligned 16-byte piece of
//                 the destination.  SEQ: 32 bases from nine aligned source dwords shifted into place (reversed: mirrored, which swaps the
//                 nibbles' order with the bytes'), each through the 256-entry code table in LDS (the reversed table is the code of the
//                 complement, so U and u need no special case), two codes per byte.  QUAL: 16 bytes minus 33, mirrored on the reverse
//                 strand; no quality: 0xFF.  Copied aux tags (mode 5): 16 bytes as they lie, from five aligned source dwords shifted into
//                 place -- the blocks lie back to back in the upload and records start anywhere, so source and destination are misaligned
//                 against each other in every way.  The ragged head and tail of a tile, and the padded last byte of an odd SEQ, are byte stores.
// and the records, written into an unframed buffer, are framed by a pass of their own (one more read and write of the stream in HBM):
//   k_bgzf_frame  one workgroup per BGZF block of the unframed stream: header, payload (aligned 16-byte stores from shifted source dwords),
//                 CRC-32 by lanes with fixed-length chunks read 16 bytes at a time and a table in LDS (mm355_bam.h: bgzf_lane_crc, the combine
//                 and the tail of a short last block), ISIZE.  Block b starts at b * (0xff00 + 31): the output offsets are arithmetic.
// or (level 1) deflated by a pass that takes k_bgzf_frame's place:
//   k_bgzf_deflate  a workgroup per payload, a grid of resident workgroups that loops over the blocks: the coder of mm355_deflate.h, its lanes
//                 the threads -- the hash table in LDS, candidates and tokens in the workgroup's 255 KB of global scratch, the histograms by LDS
//                 atomics, the ranking by all threads and the codes by one, a scan of the segments' bits, and the block (gzip header, stream,
//                 CRC-32 by the framing kernel's lanes, ISIZE) OR-ed together in the LDS the table had, then stored to the staging buffer in
//                 16-byte pieces at DFL_STRIDE * block.  A payload that deflate would not shorten is framed exactly as k_bgzf_frame does.
//   k_bgzf_compact  after an exclusive scan of the blocks' sizes: every block to its place, aligned 16-byte stores from shifted source dwords.
// A sorted call (mm355_map_batch_bam_run) frames nothing: its last step puts the records into coordinate order in a second buffer
// (k_rec_key, rocPRIM's radix sort, k_rec_sorted_len, k_rec_permute: further down) and returns them with their keys as a run.  A call that
// asked for spans (the .bai index: mm355_bai.h) runs k_rec_span on the sorted stream behind the permutation.  A packed run
// (mm355_map_batch_bam_run_packed) is deflated where the permutation left it, and the merge step of such runs (mm355_bammerge.h;
// mm355_bam_merge_step further down) is k_bgzf_inflate, k_rec_gather -- k_rec_permute's copy loop with a per-record source
// address -- and the deflate or framing kernels, all on buffers in HBM.
#include "mm355_bgzfdev.h"
#include "mm355_deflate.h"
#include "mm355_bai.h"
#include "mm355_bammerge.h"
#include <rocprim/device/device_radix_sort.hpp>

#define BAM_TILE 4096         // output bytes of one k_bam_bulk block: 256 threads x 16 bytes

MM_HD int64_t bam_tiles(int64_t n) { return (n + BAM_TILE - 1) / BAM_TILE; }
// a SEQ / QUAL / aux run of a record: len bases or bytes.  mode 0 / 1: bases packed two per byte, forwards / last base first and complemented;
// 2 / 3: quality bytes minus 33, forwards / last byte first; 4: len bytes of 0xFF; 5: len bytes copied as they are (aux tags)
MM_HD int64_t bam_bulk_bytes(const RecTileRun &r) { return r.mode < 2? ((int64_t)r.len + 1) / 2 : r.len; }
MM_HD int64_t bam_run_tiles(const RecTileRun &r) { return bam_tiles(bam_bulk_bytes(r)); }

// four bytes through the code table, two codes per byte: the 16 bits of two output bytes
__device__ __forceinline__ uint32_t bam_pack4(uint32_t x, const unsigned char *cd)
{
	return (uint32_t)cd[x & 0xff] << 4 | (uint32_t)cd[x >> 8 & 0xff] | (uint32_t)cd[x >> 16 & 0xff] << 12 | (uint32_t)cd[x >> 24] << 8;
}
__device__ __forceinline__ uint32_t bam_minus33(uint32_t x)
{
	return ((x & 0xff) - 33 & 0xff) | ((x >> 8 & 0xff) - 33 & 0xff) << 8 | ((x >> 16 & 0xff) - 33 & 0xff) << 16 | ((x >> 24) - 33 & 0xff) << 24;
}

__global__ __launch_bounds__(256) void k_bam_bulk(const RecTileRun *bulk, const int64_t *tile_off, int64_t n_lines, char *text)
{
	__shared__ unsigned char code[2][256];     // forwards; on the reverse strand: the code of the complement
	code[0][threadIdx.x] = bam_code((unsigned char)threadIdx.x);
	code[1][threadIdx.x] = bam_code(sam_comp((unsigned char)threadIdx.x));
	int64_t t;
	const RecTileRun r = rec_tile_run<BamFmt::TILE_RUNS>(bulk, tile_off, n_lines, blockIdx.x, bam_run_tiles, &t);
	__syncthreads();
	const int64_t nb = bam_bulk_bytes(r), n = r.len;
	const int64_t o0 = t * BAM_TILE, o1 = o0 + BAM_TILE < nb? o0 + BAM_TILE : nb;   // this tile: bytes [o0, o1) of the run
	if (t < 0 || o0 >= o1) return;
	const bool rev = r.mode < 4 && (r.mode & 1) != 0;
	const unsigned char *cd = code[rev? 1 : 0];
	const unsigned char *src = (const unsigned char*)r.src;
	char *dst = text + r.dst;
	const uintptr_t d0 = (uintptr_t)(dst + o0), d1 = (uintptr_t)(dst + o1);
	for (uintptr_t c = (d0 & ~(uintptr_t)15) + 16 * (uintptr_t)threadIdx.x; c < d1; c += 16 * 256) {
		const int64_t oc = (int64_t)c - (int64_t)(uintptr_t)dst;
		// a whole piece: inside the tile, and (SEQ) every one of its 32 bases exists -- the padded byte of an odd run goes the byte way
		if (c >= d0 && c + 16 <= d1 && (r.mode >= 2 || 2 * (oc + 16) <= n)) {
			uint32_t v[4];
			if (r.mode == 4) v[0] = v[1] = v[2] = v[3] = 0xffffffffu;
			else if (r.mode == 5) sam_load16(r.src, oc, v);
			else if (r.mode >= 2) {
				sam_load16(r.src, rev? n - 16 - oc : oc, v);
				if (rev) sam_mirror16(v);
				for (int k = 0; k < 4; ++k) v[k] = bam_minus33(v[k]);
			} else {
				uint32_t a[4], e[4];               // the 32 bases, lowest address first; mirrored: the halves swap too
				const int64_t s = rev? n - 32 - 2 * oc : 2 * oc;
				sam_load16(r.src, s, a); sam_load16(r.src, s + 16, e);
				if (rev) {
					for (int k = 0; k < 4; ++k) { const uint32_t x = a[k]; a[k] = e[k]; e[k] = x; }
					sam_mirror16(a); sam_mirror16(e);
				}
				v[0] = bam_pack4(a[0], cd) | bam_pack4(a[1], cd) << 16; v[1] = bam_pack4(a[2], cd) | bam_pack4(a[3], cd) << 16;
				v[2] = bam_pack4(e[0], cd) | bam_pack4(e[1], cd) << 16; v[3] = bam_pack4(e[2], cd) | bam_pack4(e[3], cd) << 16;
			}
			*(uint4*)c = make_uint4(v[0], v[1], v[2], v[3]);
		} else {
			const uintptr_t e = c + 16 < d1? c + 16 : d1;
			for (uintptr_t a = c > d0? c : d0; a < e; ++a) {
				const int64_t o = (int64_t)(a - (uintptr_t)dst);
				unsigned char x;
				if (r.mode == 4) x = 0xff;
				else if (r.mode == 5) x = src[o];
				else if (r.mode >= 2) x = (unsigned char)(src[rev? n - 1 - o : o] - 33);
				else {
					const int64_t i = 2 * o;
					const unsigned char hi4 = cd[src[rev? n - 1 - i : i]], lo4 = i + 1 < n? cd[src[rev? n - 2 - i : i + 1]] : 0;
					x = (unsigned char)(hi4 << 4 | lo4);
				}
				*(unsigned char*)a = x;
			}
		}
	}
}

// one stored block at o: header, payload, CRC-32, ISIZE
__device__ __forceinline__ void bgzf_stored_block(const char *src, uint32_t len, char *o, const uint32_t *tab, uint32_t *reg, const uint32_t *x_pow, int tid)
{
	if (tid < BGZF_HEAD) o[tid] = (char)bgzf_head_byte(tid, len);
	char *dst = o + BGZF_HEAD;
	bgzf_copy(src, dst, len, tid);
	__syncthreads();
	const uint32_t crc = bgzf_block_crc(src, len, tab, reg, x_pow, tid);
	if (tid == 0)
		for (int i = 0; i < 4; ++i) { dst[len + i] = (char)(crc >> 8 * i); dst[len + 4 + i] = (char)(len >> 8 * i); }
}

// in: n bytes, readable for 8 more (whole dwords are read around a span); out: bgzf_size(n) bytes; one workgroup per block
__global__ __launch_bounds__(BGZF_LANES) void k_bgzf_frame(const char *in, int64_t n, char *out)
{
	__shared__ uint32_t tab[256], reg[BGZF_LANES], x_pow[8];
	const int tid = threadIdx.x;
	tab[tid] = crc32_tab_entry((uint32_t)tid);
	if (tid < 8) x_pow[tid] = crc32_x2n(11 + tid);
	const int64_t b = blockIdx.x, at = b * BGZF_PAYLOAD;
	const uint32_t len = (uint32_t)(n - at < BGZF_PAYLOAD? n - at : BGZF_PAYLOAD);
	bgzf_stored_block(in + at, len, out + b * (BGZF_PAYLOAD + BGZF_EXTRA), tab, reg, x_pow, tid);
}

#define DFL_STRIDE 65312      // a block's place in the staging buffer: BGZF_PAYLOAD + BGZF_EXTRA up to a multiple of 16
#define DFL_MAX_GRID 512      // resident workgroups (two per CU: 71 KB of LDS each); the token scratch is sized by them, not by the blocks
static_assert(DFL_STRIDE % 16 == 0 && DFL_STRIDE >= BGZF_PAYLOAD + BGZF_EXTRA && BGZF_LANES == DFL_SEGS && BGZF_LANES == DFL_ROUND, "a thread is a CRC lane, a segment and a position of a round");

// in: n bytes in n_blocks payloads, readable for 8 more; scratch: BGZF_PAYLOAD words per workgroup of the grid; stage: n_blocks * DFL_STRIDE
// bytes, block b at b * DFL_STRIDE; size[b]: its bytes
__global__ __launch_bounds__(BGZF_LANES, 2) void k_bgzf_deflate(const char *in, int64_t n, int64_t n_blocks, uint32_t *scratch, char *stage, int64_t *size)
{
	__shared__ __attribute__((aligned(16))) uint32_t buf[DFL_BUF_WORDS];   // the hash table; from the emission on the block
	__shared__ DflWork W;
	__shared__ uint32_t tab[256], reg[BGZF_LANES], x_pow[8];
	const uint32_t tid = threadIdx.x;
	tab[tid] = crc32_tab_entry(tid);
	if (tid < 8) x_pow[tid] = crc32_x2n(11 + (int)tid);
	uint32_t *scr = scratch + (size_t)blockIdx.x * BGZF_PAYLOAD;
	for (int64_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
		const int64_t at = b * BGZF_PAYLOAD;
		const uint32_t len = (uint32_t)(n - at < BGZF_PAYLOAD? n - at : BGZF_PAYLOAD);
		const unsigned char *src = (const unsigned char*)in + at;
		char *o = stage + b * DFL_STRIDE;
		for (uint32_t i = tid; i < DFL_BUF_WORDS; i += BGZF_LANES) buf[i] = 0;
		for (uint32_t i = tid; i < sizeof(DflWork) / 4; i += BGZF_LANES) ((uint32_t*)&W)[i] = 0;
		__syncthreads();
		// candidates: the hashes of eight rounds are loaded ahead (they need no table), then a round is two LDS steps between barriers
		const uint32_t rounds = (len + DFL_ROUND - 1) / DFL_ROUND;
		for (uint32_t r0 = 0; r0 < rounds; r0 += 8) {
			uint32_t h1[8];
			for (uint32_t k = 0; k < 8; ++k) h1[k] = dfl_hash1(src, len, (r0 + k) * DFL_ROUND + tid);
			for (uint32_t k = 0; k < 8 && r0 + k < rounds; ++k) {
				const uint32_t p = (r0 + k) * DFL_ROUND + tid;
				dfl_round_read(p, len, h1[k], buf, scr);
				__syncthreads();
				dfl_round_raise(p, h1[k], buf);
				__syncthreads();
			}
		}
		W.n_tok[tid] = dfl_parse(src, len, tid, scr, W.ll_f, W.d_f);
		if (tid == 0) W.ll_f[DFL_EOB] = 1;
		__syncthreads();
		for (int s = (int)tid; s < DFL_N_LL; s += BGZF_LANES) dfl_rank(W.ll_f, DFL_N_LL, s, W.ll_sorted);
		if (tid < DFL_N_D) dfl_rank(W.d_f, DFL_N_D, (int)tid, W.d_sorted);
		__syncthreads();
		if (tid == 0) dfl_build(W);
		__syncthreads();
		// the segments' bits, their inclusive scan, and from it every segment's first bit in the stream
		const uint32_t mine = dfl_seg_bits(W, tid, scr);
		W.seg_bits[tid] = mine;
		__syncthreads();
		for (uint32_t d = 1; d < DFL_SEGS; d <<= 1) {
			const uint32_t v = tid >= d? W.seg_bits[tid - d] : 0u;
			__syncthreads();
			W.seg_bits[tid] += v;
			__syncthreads();
		}
		const uint32_t incl = W.seg_bits[tid], token_bits = W.seg_bits[DFL_SEGS - 1];
		__syncthreads();
		W.seg_bits[tid] = W.head_bits + incl - mine;
		if (tid == 0) W.n_bytes = dfl_stream_bytes(W, token_bits);
		__syncthreads();
		if (W.n_bytes >= len + 5) {                            // (the whole workgroup)
			bgzf_stored_block((const char*)src, len, o, tab, reg, x_pow, (int)tid);
			if (tid == 0) size[b] = (int64_t)len + BGZF_EXTRA;
		} else {
			for (uint32_t i = tid; i < DFL_BUF_WORDS; i += BGZF_LANES) buf[i] = 0;
			__syncthreads();
			if (tid == 0) dfl_emit_head(W, buf);
			dfl_emit_seg(W, tid, scr, buf);
			const uint32_t crc = bgzf_block_crc((const char*)src, len, tab, reg, x_pow, (int)tid);
			if (tid == 0) dfl_emit_tail(W, W.head_bits + token_bits, crc, len, buf);
			__syncthreads();
			const uint32_t total = DFL_GZ_HEAD + W.n_bytes + 8;    // (o is 16-byte aligned: whole pieces, then the last one's bytes)
			for (uint32_t i = 16 * tid; i < total; i += 16 * BGZF_LANES) {
				if (i + 16 <= total) *(uint4*)(o + i) = *(const uint4*)(buf + i / 4);
				else for (uint32_t j = i; j < total; ++j) o[j] = (char)(buf[j >> 2] >> 8 * (j & 3));
			}
			if (tid == 0) size[b] = total;
		}
		__syncthreads();
	}
}

// block b, size[b] bytes at stage + b * DFL_STRIDE (readable for 8 more), to out + off[b]; one workgroup per block
__global__ __launch_bounds__(BGZF_LANES) void k_bgzf_compact(const char *stage, const int64_t *size, const int64_t *off, char *out)
{
	const int64_t b = blockIdx.x;
	bgzf_copy(stage + b * DFL_STRIDE, out + off[b], (uint32_t)size[b], threadIdx.x);
}

// ---- the sort stage of a sorted call (mm355_bamsort.h states the order): keys, rocPRIM's radix sort of (key, index), the new offsets, and
//   k_rec_permute  work item = (sorted record j, tile of BAM_TILE output bytes), one block each, as k_bam_bulk's mode 5: a thread owns an
//                 aligned 16-byte piece of the destination, the source comes from shifted aligned dwords, the ragged head and tail of a tile
//                 are byte stores.  Every byte has one writer.
// record i of the stream at src + off[i]: its key, and its index as the sort's value
__global__ __launch_bounds__(256) void k_rec_key(const char *src, const int64_t *off, int64_t n, uint64_t *key, uint32_t *idx)
{
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	key[i] = bam_sort_key((const uint8_t*)src + off[i]);       // (byte loads: a record starts at any residue)
	idx[i] = (uint32_t)i;
}
// the lengths and tile counts in sorted order; entry n of each is 0, where the scans leave the totals
__global__ __launch_bounds__(256) void k_rec_sorted_len(const int64_t *off, const uint32_t *idx, int64_t n, int64_t *len, int64_t *ntile)
{
	const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (j > n) return;
	const int64_t l = j < n? off[idx[j] + 1] - off[idx[j]] : 0;
	len[j] = l; ntile[j] = bam_tiles(l);
}
// the two halves k_rec_permute and k_rec_gather share.  The work item of block b: the output record *rec and its bytes [*o0, *o1); false: none
__device__ __forceinline__ bool rec_tile_find(const int64_t *new_off, const int64_t *tile_off, int64_t n, int64_t b, int64_t *rec, int64_t *o0, int64_t *o1)
{
	if (b >= tile_off[n]) return false;        // (the whole block)
	int64_t lo = 0, hi = n;                    // the last record whose first tile is <= b (rec_tile_run's search; a record without bytes has no tile and is passed over)
	while (hi - lo > 1) { const int64_t mid = (lo + hi) >> 1; if (tile_off[mid] <= b) lo = mid; else hi = mid; }
	const int64_t t = b - tile_off[lo], len = new_off[lo + 1] - new_off[lo];
	*rec = lo;
	*o0 = t * BAM_TILE; *o1 = *o0 + BAM_TILE < len? *o0 + BAM_TILE : len;   // this tile: bytes [o0, o1) of the record
	return *o0 < *o1;
}
// The copy loop: bytes [o0, o1) of the record at s to dst, by the block's 256 threads
__device__ __forceinline__ void rec_tile_copy(const char *s, char *dst, int64_t o0, int64_t o1)
{
	const uintptr_t d0 = (uintptr_t)(dst + o0), d1 = (uintptr_t)(dst + o1);
	for (uintptr_t c = (d0 & ~(uintptr_t)15) + 16 * (uintptr_t)threadIdx.x; c < d1; c += 16 * 256) {
		if (c >= d0 && c + 16 <= d1) {
			uint32_t v[4];
			sam_load16(s, (int64_t)c - (int64_t)(uintptr_t)dst, v);
			*(uint4*)c = make_uint4(v[0], v[1], v[2], v[3]);
		} else {
			const uintptr_t e = c + 16 < d1? c + 16 : d1;
			for (uintptr_t a = c > d0? c : d0; a < e; ++a) *(char*)a = s[(int64_t)(a - (uintptr_t)dst)];
		}
	}
}
// src: readable for 8 bytes behind its last record (whole dwords are read around a span); new_off, tile_off: n + 1 entries; the grid may
// be larger than the tile total (it is sized on the host by a bound): the blocks behind it leave
__global__ __launch_bounds__(256) void k_rec_permute(const char *src, const int64_t *off, const uint32_t *idx, const int64_t *new_off, const int64_t *tile_off, int64_t n, char *out)
{
	int64_t lo, o0, o1;
	if (!rec_tile_find(new_off, tile_off, n, blockIdx.x, &lo, &o0, &o1)) return;
	rec_tile_copy(src + off[idx[lo]], out + new_off[lo], o0, o1);
}

// ---- the merge step of compressed runs (mm355_bammerge.h states it): the records of a step, in merged order, out of the inflated slices
//   k_rec_tiles   the tile count of every record from its length; entry n of both arrays is 0, where the scans leave the totals
//   k_rec_gather  k_rec_permute with a per-record source address: record i lies at src + at[i] (any residue) and goes to out + new_off[i].
//                 src is readable for 8 bytes behind its last byte; the grid is sized by the same bound, the blocks behind the tiles leave
__global__ __launch_bounds__(256) void k_rec_tiles(const int64_t *len, int64_t n, int64_t *ntile)
{
	const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (j <= n) ntile[j] = bam_tiles(len[j]);
}
__global__ __launch_bounds__(256) void k_rec_gather(const char *src, const int64_t *at, const int64_t *new_off, const int64_t *tile_off, int64_t n, char *out)
{
	int64_t lo, o0, o1;
	if (!rec_tile_find(new_off, tile_off, n, blockIdx.x, &lo, &o0, &o1)) return;
	rec_tile_copy(src + at[lo], out + new_off[lo], o0, o1);
}

// The span of every record of the sorted stream (mm355_bai.h states it; the pieces are its functions): a wave per record.  The fixed fields by
// byte loads; the CIGAR words, which start at any residue, lane-strided from aligned dwords shifted into place -- the dword below a word
// starts at most 3 bytes before it, inside the record's fixed part, the one above is read only where the word reaches into it; a 64-bit sum
// per lane and over the wave; lane 0 stores.  The word count is held to the record's length, so nothing outside the record is read.
__global__ __launch_bounds__(256) void k_rec_span(const char *src, const int64_t *off, int64_t n, int64_t *span)
{
	const int lane = threadIdx.x & 63;
	const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
	if (j >= n) return;                        // (the whole wave)
	const int64_t at = off[j], len = off[j + 1] - at;
	const uint8_t *rec = (const uint8_t*)src + at;
	const uint32_t flag = bam_rec_flag(rec), l_name = bam_rec_l_name(rec);
	const int64_t room = (len - 36 - (int64_t)l_name) / 4;
	uint32_t nw = bam_span_words(flag, bam_rec_n_cigar(rec));
	if ((int64_t)nw > room) nw = room > 0? (uint32_t)room : 0u;
	const uintptr_t w0 = (uintptr_t)(rec + 36 + l_name);
	const int sh = (int)(w0 & 3) * 8;
	const uint32_t *pa = (const uint32_t*)(w0 & ~(uintptr_t)3);
	uint64_t sum = 0;
	for (uint32_t i = (uint32_t)lane; i < nw; i += 64) {
		uint32_t w = pa[i];
		if (sh) w = w >> sh | pa[i + 1] << (32 - sh);
		sum += bam_cigar_ref_len(w);
	}
	sum = wave_reduce_add64(sum);
	if (lane == 0) span[j] = bam_span_of((int32_t)bam_rec_u32(rec + 8), flag, sum);
}

// ------------------------------------------------------------------ host side
// Sorts the n records of the stream at d_src (device memory, n_bytes, readable for 8 more; record i at d_off[i], n + 1 offsets on the device)
// into c->bam_sorted and copies the records, their keys and their new offsets into R's arrays (allocated for n and n_bytes).  The four
// launches and the library calls between them lie between the context's two events: microseconds in *k_us.  The permute grid is sized by a
// bound on the tiles, n_bytes / BAM_TILE + n, so that nothing crosses to the host before the one copy at the end.
// R->span (a call that asked for spans): k_rec_span on the sorted stream, before the second event, and 8 bytes more per record in the copy;
// span_us (MM355_BAM_TIMES=1): that kernel between two events of its own.  rec_down false (a packed run): the records stay in c->bam_sorted and
// R->rec is not written
static int bam_sort_device(mm355_ctx *c, const char *d_src, int64_t n_bytes, const int64_t *d_off, int64_t n, mm355_run_t *R, double *k_us, double *span_us = 0, bool rec_down = true)
{
	hipStream_t st = c->st;
	*k_us = 0;
	if (span_us) *span_us = 0;
	if (n == 0) return 0;
	const int64_t max_tiles = n_bytes / BAM_TILE + n;
	if (n > (int64_t)INT32_MAX || max_tiles > (int64_t)INT32_MAX) return MM355_EINVAL;
	size_t tb_sort = 0, tb_scan = 0;
	(void)rocprim::radix_sort_pairs(nullptr, tb_sort, (uint64_t*)0, (uint64_t*)0, (uint32_t*)0, (uint32_t*)0, (size_t)n, 0u, 64u, st);
	(void)rocprim::exclusive_scan(nullptr, tb_scan, (int64_t*)0, (int64_t*)0, (int64_t)0, (size_t)n + 1, rocprim::plus<int64_t>(), st);
	const size_t w8 = up256((size_t)(n + 1) * 8), w4 = up256((size_t)n * 4);
	const size_t w_key0 = 0, w_key1 = w_key0 + w8, w_idx0 = w_key1 + w8, w_idx1 = w_idx0 + w4, w_len = w_idx1 + w4, w_noff = w_len + w8, w_nt = w_noff + w8, w_to = w_nt + w8,
	             w_span = w_to + w8, w_tmp = w_span + (R->span? w8 : 0);
	if (c->bam_work.ensure(w_tmp + up256(std::max(tb_sort, tb_scan) + 256)) || c->bam_sorted.ensure((size_t)n_bytes + 64)) return MM355_ENOMEM;
	char *dw = (char*)c->bam_work.p;
	uint64_t *key0 = (uint64_t*)(dw + w_key0), *key1 = (uint64_t*)(dw + w_key1);
	uint32_t *idx0 = (uint32_t*)(dw + w_idx0), *idx1 = (uint32_t*)(dw + w_idx1);
	int64_t *d_len = (int64_t*)(dw + w_len), *d_noff = (int64_t*)(dw + w_noff), *d_nt = (int64_t*)(dw + w_nt), *d_to = (int64_t*)(dw + w_to);
	(void)hipEventRecord(c->ev0, st);
	hipLaunchKernelGGL(k_rec_key, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_src, d_off, n, key0, idx0);
	HIPCHK(hipGetLastError());
	HIPCHK(rocprim::radix_sort_pairs(dw + w_tmp, tb_sort, key0, key1, idx0, idx1, (size_t)n, 0u, 64u, st));   // (a radix sort is stable: equal keys in index order)
	hipLaunchKernelGGL(k_rec_sorted_len, dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, st, d_off, (const uint32_t*)idx1, n, d_len, d_nt);
	HIPCHK(hipGetLastError());
	HIPCHK(rocprim::exclusive_scan(dw + w_tmp, tb_scan, d_len, d_noff, (int64_t)0, (size_t)n + 1, rocprim::plus<int64_t>(), st));
	HIPCHK(rocprim::exclusive_scan(dw + w_tmp, tb_scan, d_nt, d_to, (int64_t)0, (size_t)n + 1, rocprim::plus<int64_t>(), st));
	hipLaunchKernelGGL(k_rec_permute, dim3((unsigned)max_tiles), dim3(256), 0, st, d_src, d_off, (const uint32_t*)idx1, (const int64_t*)d_noff, (const int64_t*)d_to, n, (char*)c->bam_sorted.p);
	HIPCHK(hipGetLastError());
	struct SpanEvents { hipEvent_t v[2] = { 0, 0 }; ~SpanEvents() { for (hipEvent_t e : v) if (e) (void)hipEventDestroy(e); } } sev;   // (span_us: the kernel timed alone)
	if (R->span) {
		const bool timed = span_us && hipEventCreate(&sev.v[0]) == hipSuccess && hipEventCreate(&sev.v[1]) == hipSuccess;
		if (timed) (void)hipEventRecord(sev.v[0], st);
		hipLaunchKernelGGL(k_rec_span, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, (const char*)c->bam_sorted.p, (const int64_t*)d_noff, n, (int64_t*)(dw + w_span));
		HIPCHK(hipGetLastError());
		if (timed) (void)hipEventRecord(sev.v[1], st);
	}
	(void)hipEventRecord(c->ev1, st);
	if (R->span) HIPCHK(hipMemcpyAsync(R->span, dw + w_span, (size_t)n * 8, hipMemcpyDeviceToHost, st));
	if (rec_down) HIPCHK(hipMemcpyAsync(R->rec, c->bam_sorted.p, (size_t)n_bytes, hipMemcpyDeviceToHost, st));
	HIPCHK(hipMemcpyAsync(R->key, key1, (size_t)n * 8, hipMemcpyDeviceToHost, st));
	HIPCHK(hipMemcpyAsync(R->rec_off, d_noff, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, st));
	HIPCHK(mm355_wait_stream(st));
	if (R->rec_off[n] != n_bytes) return MM355_EHIP;           // (the lengths are a permutation of the input's)
	float ms = 0; (void)hipEventElapsedTime(&ms, c->ev0, c->ev1); *k_us = (double)ms * 1e3;
	if (R->span && span_us && sev.v[1]) { (void)hipEventElapsedTime(&ms, sev.v[0], sev.v[1]); *span_us = (double)ms * 1e3; }
	return 0;
}

// frames the n bytes at src (device memory, readable for 8 more: c->rec_text.p, or the sorted stream) into c->bam_out and copies the blocks to
// `to`; timed: the kernel between the context's two events, microseconds in *k_us
static int bam_frame_device(mm355_ctx *c, const char *src, int64_t n, char *to, bool timed, double *k_us)
{
	hipStream_t st = c->st;
	if (n == 0) return 0;
	if (bgzf_blocks(n) > (int64_t)INT32_MAX) return MM355_EINVAL;
	if (c->bam_out.ensure((size_t)bgzf_size(n) + 64)) return MM355_ENOMEM;
	if (timed) (void)hipEventRecord(c->ev0, st);
	hipLaunchKernelGGL(k_bgzf_frame, dim3((unsigned)bgzf_blocks(n)), dim3(BGZF_LANES), 0, st, src, n, (char*)c->bam_out.p);
	HIPCHK(hipGetLastError());
	if (timed) (void)hipEventRecord(c->ev1, st);
	HIPCHK(hipMemcpyAsync(to, c->bam_out.p, (size_t)bgzf_size(n), hipMemcpyDeviceToHost, st));
	HIPCHK(mm355_wait_stream(st));
	if (timed) { float ms = 0; (void)hipEventElapsedTime(&ms, c->ev0, c->ev1); *k_us = (double)ms * 1e3; }
	return 0;
}

// deflates the n bytes at src (device memory, readable for 8 more) into c->bam_out: *n_out bytes of blocks, which the caller copies; timed: the two
// kernels and the scan between the context's two events, microseconds in *k_us, and the count of blocks that were written stored; h_blk_off (a
// packed run): the blocks' bgzf_blocks(n) + 1 offsets inside the result
static int bam_deflate_device(mm355_ctx *c, const char *src, int64_t n, int64_t *n_out, bool timed, double *k_us, int64_t *n_stored, int64_t *h_blk_off = 0)
{
	hipStream_t st = c->st;
	*n_out = 0; *n_stored = 0;
	if (n == 0) return 0;
	const int64_t nb = bgzf_blocks(n);
	if (nb > (int64_t)INT32_MAX) return MM355_EINVAL;
	const unsigned grid = (unsigned)(nb < DFL_MAX_GRID? nb : DFL_MAX_GRID);
	size_t tb = 0;
	(void)rocprim::exclusive_scan(nullptr, tb, (int64_t*)0, (int64_t*)0, (int64_t)0, (size_t)nb + 1, rocprim::plus<int64_t>(), st);
	const size_t w1 = up256((size_t)(nb + 1) * 8), w_size = 0, w_off = w1, w_tmp = 2 * w1, w_scr = w_tmp + up256(tb + 256);
	if (c->bam_work.ensure(w_scr + (size_t)grid * BGZF_PAYLOAD * 4) || c->bam_stage.ensure((size_t)nb * DFL_STRIDE + 64) || c->bam_out.ensure((size_t)bgzf_size(n) + 64) ||
	    c->h_rec_out.ensure(64, 1 << 20)) return MM355_ENOMEM;
	char *dw = (char*)c->bam_work.p;
	int64_t *d_size = (int64_t*)(dw + w_size), *d_off = (int64_t*)(dw + w_off);
	HIPCHK(hipMemsetAsync(d_size + nb, 0, 8, st));
	if (timed) (void)hipEventRecord(c->ev0, st);
	hipLaunchKernelGGL(k_bgzf_deflate, dim3(grid), dim3(BGZF_LANES), 0, st, src, n, nb, (uint32_t*)(dw + w_scr), (char*)c->bam_stage.p, d_size);
	HIPCHK(hipGetLastError());
	HIPCHK(rocprim::exclusive_scan(dw + w_tmp, tb, d_size, d_off, (int64_t)0, (size_t)nb + 1, rocprim::plus<int64_t>(), st));
	hipLaunchKernelGGL(k_bgzf_compact, dim3((unsigned)nb), dim3(BGZF_LANES), 0, st, (const char*)c->bam_stage.p, d_size, d_off, (char*)c->bam_out.p);
	HIPCHK(hipGetLastError());
	if (timed) (void)hipEventRecord(c->ev1, st);
	int64_t *h_tot = (int64_t*)c->h_rec_out.p;
	HIPCHK(hipMemcpyAsync(h_tot, d_off + nb, 8, hipMemcpyDeviceToHost, st));
	if (h_blk_off) HIPCHK(hipMemcpyAsync(h_blk_off, d_off, (size_t)(nb + 1) * 8, hipMemcpyDeviceToHost, st));
	HIPCHK(mm355_wait_stream(st));
	if (h_tot[0] < nb * (DFL_GZ_HEAD + 8) || h_tot[0] > bgzf_size(n)) return MM355_EHIP;   // (no block is longer than its stored form)
	*n_out = h_tot[0];
	if (timed) {
		float ms = 0; (void)hipEventElapsedTime(&ms, c->ev0, c->ev1); *k_us = (double)ms * 1e3;
		std::vector<int64_t> hs((size_t)nb);
		HIPCHK(hipMemcpy(hs.data(), d_size, (size_t)nb * 8, hipMemcpyDeviceToHost));
		for (int64_t b = 0; b < nb; ++b) *n_stored += hs[b] == (n - b * BGZF_PAYLOAD < BGZF_PAYLOAD? n - b * BGZF_PAYLOAD : BGZF_PAYLOAD) + BGZF_EXTRA;
	}
	return 0;
}
// the n_out bytes of blocks in c->bam_out to the host
static int bam_blocks_back(mm355_ctx *c, int64_t n_out, char *to)
{
	if (n_out) HIPCHK(hipMemcpyAsync(to, c->bam_out.p, (size_t)n_out, hipMemcpyDeviceToHost, c->st));
	HIPCHK(mm355_wait_stream(c->st));
	return 0;
}
// MM355_BAM_TIMES=1: the line of a deflate call
static void bam_deflate_times(const char *who, int64_t n, int64_t n_out, int64_t n_stored, double k_us, bool device)
{
	fprintf(stderr, "[mm355] bgzf_deflate_times %s %s blocks %lld bytes_in %lld bytes_out %lld stored_blocks %lld k_bgzf_deflate_compact_us %.1f\n", who, device? "device" : "host",
	        (long long)bgzf_blocks(n), (long long)n, (long long)n_out, (long long)n_stored, k_us);
}
static bool bam_times_on() { const char *te = getenv("MM355_BAM_TIMES"); return te && *te && *te != '0'; }

// A packed run: the n_raw bytes of the sorted stream in c->bam_sorted (bam_sort_device has left them there, and R's other arrays are filled)
// deflated where they lie; R->rec becomes the members, R->blk_off their offsets.  Only the members cross to the host.
static int bam_run_pack_device(mm355_ctx *c, int64_t n_raw, mm355_run_t *R, bool times)
{
	const int64_t nb = bgzf_blocks(n_raw);
	int64_t n_out = 0, n_stored = 0;
	double d_us = 0;
	R->blk_off = (int64_t*)calloc((size_t)nb + 1, 8);
	if (R->blk_off == 0) return MM355_ENOMEM;
	if (int rc = bam_deflate_device(c, (const char*)c->bam_sorted.p, n_raw, &n_out, times, &d_us, &n_stored, R->blk_off)) return rc;
	char *z = (char*)malloc((size_t)n_out + 1);
	if (z == 0) return MM355_ENOMEM;
	free(R->rec);
	R->rec = z; z[n_out] = 0;
	if (int rc = bam_blocks_back(c, n_out, z)) return rc;
	if (R->blk_off[nb] != n_out) return MM355_EHIP;
	R->n_bytes = n_out; R->n_blk = nb; R->packed = 1;
	if (times) bam_deflate_times("run", n_raw, n_out, n_stored, d_us, true);
	return 0;
}

// BamFmt as the device writes it
struct BamDevFmt : BamFmt {
	typedef RecDev Dev;
	struct Count : BamCountSink {
		int64_t tiles = 0;
		__device__ explicit Count(int64_t) {}
		__device__ void seq4(const char *, int64_t l, bool) { n += (l + 1) / 2; tiles += bam_tiles((l + 1) / 2); }
		__device__ void qual(const char *, int64_t l, bool) { n += l; tiles += bam_tiles(l); }
		__device__ void fill(int64_t l) { n += l; tiles += bam_tiles(l); }
		__device__ void aux(const uint8_t *, int64_t l) { n += l; tiles += bam_tiles(l); }
	};
	struct Write : RecWrite<RUNS, TILE_RUNS> {
		using RecWrite<RUNS, TILE_RUNS>::RecWrite;
		__device__ void u8(uint32_t v) { p[n++] = (char)v; }
		__device__ void u16(uint32_t v) { u8(v & 0xff); u8(v >> 8 & 0xff); }
		__device__ void u32(uint32_t v) { u16(v & 0xffff); u16(v >> 16); }
		__device__ void cigar(const uint32_t *w, int64_t k) { bytes((const char*)w, 4 * k); }      // (the device is little-endian: the words as they lie)
		__device__ void seq4(const char *b, int64_t l, bool rev) { note(b, l, rev? 1 : 0); n += (l + 1) / 2; }
		__device__ void qual(const char *b, int64_t l, bool rev) { note(b, l, rev? 3 : 2); n += l; }
		__device__ void fill(int64_t l) { note(0, l, 4); n += l; }
		__device__ void aux(const uint8_t *b, int64_t l) { note((const char*)b, l, 5); n += l; }
	};
	// MM355_BAM_TIMES=1 (tools/bam_bench.py, tools/aux_bench.py): one line on stderr with the framing kernel's time between two events and, at its end, k_bam_bulk's
	static constexpr const char *TIMES_ENV = "MM355_BAM_TIMES";
	static int bulk(mm355_ctx *c, RecCall &k, const RecTileRun *runs, const int64_t *tile_off)
	{
		// timed: a pair of events of the call's own around the kernel (the framing step uses the context's two); finish() reads and frees them
		const bool timed = k.times && hipEventCreate(&k.bulk_ev[0]) == hipSuccess && hipEventCreate(&k.bulk_ev[1]) == hipSuccess;
		if (timed) (void)hipEventRecord(k.bulk_ev[0], c->st);
		if (k.n_tiles > 0) {
			hipLaunchKernelGGL(k_bam_bulk, dim3((unsigned)k.n_tiles), dim3(256), 0, c->st, runs, tile_off, k.n_lines, (char*)c->rec_text.p);
			HIPCHK(hipGetLastError());
		}
		if (timed) (void)hipEventRecord(k.bulk_ev[1], c->st);
		return 0;
	}
	static int finish(mm355_ctx *c, RecCall &k, const int64_t *d_lo, mm355_text_t **out)
	{
		double b_us = 0;
		const int rc = finish_1(c, k, d_lo, out, &b_us);
		for (hipEvent_t &e : k.bulk_ev) if (e) { (void)hipEventDestroy(e); e = 0; }
		return rc;
	}
	static int finish_1(mm355_ctx *c, RecCall &k, const int64_t *d_lo, mm355_text_t **out, double *b_us)
	{
		double k_us = 0, d_us = 0;
		int64_t n_out = bgzf_size(k.n_text), n_stored = 0;
		if (k.last.level)
			if (int rc = bam_deflate_device(c, (const char*)c->rec_text.p, k.n_text, &n_out, k.times, &d_us, &n_stored)) return rc;
		mm355_text_t *T = mm355_text_alloc(k.n_reads, k.n_lines, n_out);
		if (T == 0) return MM355_ENOMEM;
		hipError_t e = hipMemcpyAsync(T->line_off, d_lo, (size_t)(k.n_reads + 1) * 8, hipMemcpyDeviceToHost, c->st);
		int rc = e != hipSuccess? MM355_EHIP : k.last.level? bam_blocks_back(c, n_out, T->text) : bam_frame_device(c, (const char*)c->rec_text.p, k.n_text, T->text, k.times, &k_us);
		if (rc) { fprintf(stderr, "[mm355] error %d in the BAM writer (%s)\n", rc, hipGetErrorString(e)); mm355_free_text_host(T); return rc; }
		if (k.times && k.bulk_ev[1]) { float ms = 0; (void)hipEventElapsedTime(&ms, k.bulk_ev[0], k.bulk_ev[1]); *b_us = (double)ms * 1e3; }   // (the stream has been waited for)
		if (k.times && k.last.level) bam_deflate_times("records", k.n_text, n_out, n_stored, d_us, true);
		else if (k.times)
			fprintf(stderr, "[mm355] bam_times records %lld stream_bytes %lld blocks %lld tiles %lld pack_ms %.3f k_bgzf_frame_us %.1f total_ms %.3f k_bam_bulk_us %.1f\n", (long long)k.n_lines,
			        (long long)k.n_text, (long long)bgzf_blocks(k.n_text), (long long)k.n_tiles, k.t_packed - k.t_begin, k_us, mm355_now_ms() - k.t_begin, *b_us);
		*out = T;
		return 0;
	}
};

// BamDevFmt for a call with copied tags: the kernels' argument carries them
struct BamAuxDevFmt : BamDevFmt { typedef RecDevAux Dev; };

// The sorted call (mm355_map_batch_bam_run): the kernels, sinks and bulk step are B's -- the same instantiations an unsorted call launches --
// and the last step sorts the records where they lie instead of framing them: the result is a run.
// MM355_BAM_TIMES=1 (tools/sort_bench.py): a line of its own with the sort step's time between two events and k_bam_bulk's
// k.last.span (mm355_map_batch_bam_run_span): the run carries the records' spans, from k_rec_span behind the permutation; the line ends with its time
// k.last.packed (mm355_map_batch_bam_run_packed): the records stay in HBM and are deflated there; the run carries their BGZF members
template <typename B> struct BamRunFmtOf : B {
	typedef B Kern;
	static int finish(mm355_ctx *c, RecCall &k, const int64_t *, mm355_run_t **out)
	{
		double s_us = 0, b_us = 0, sp_us = 0;
		const bool span = k.last.span, packed = k.last.packed;
		mm355_run_t *R = mm355_run_alloc(k.n_lines, packed? 0 : k.n_text, span);
		int rc = R? bam_sort_device(c, (const char*)c->rec_text.p, k.n_text, k.d_off, k.n_lines, R, &s_us, span && k.times? &sp_us : 0, !packed) : MM355_ENOMEM;
		if (rc == 0 && packed) rc = bam_run_pack_device(c, k.n_text, R, k.times);
		if (rc == 0 && k.times && k.bulk_ev[1]) { float ms = 0; (void)hipEventElapsedTime(&ms, k.bulk_ev[0], k.bulk_ev[1]); b_us = (double)ms * 1e3; }   // (the stream has been waited for)
		for (hipEvent_t &e : k.bulk_ev) if (e) { (void)hipEventDestroy(e); e = 0; }
		if (rc) {                                  // (a copy into R's arrays may be queued: the stream first, then the free)
			(void)mm355_wait_stream(c->st);
			fprintf(stderr, "[mm355] error %d in the BAM sort stage\n", rc);
			mm355_free_run_host(R);
			return rc;
		}
		if (k.times) {
			fprintf(stderr, "[mm355] bam_sort_times records %lld stream_bytes %lld tiles %lld k_rec_key_sort_permute_us %.1f k_bam_bulk_us %.1f total_ms %.3f", (long long)k.n_lines,
			        (long long)k.n_text, (long long)k.n_tiles, s_us, b_us, mm355_now_ms() - k.t_begin);
			if (span) fprintf(stderr, " k_rec_span_us %.1f", sp_us);
			fprintf(stderr, "\n");
		}
		R->ms_sort = s_us / 1e3;
		*out = R;
		return 0;
	}
};

// MM355_PAF_AUTO for BAM: the device formatter from this many hits on.  Measured with tools/bam_bench.py (profiles/bam_file.json, format_sweep:
// ms_format of the two formatters on the hits of 16 .. 9216 reads, map-ont with cs, reads of N50 8 kb with qualities): the host is ahead at 16
// hits (0.22 against 0.25 ms), the device at 24 (0.25 against 0.32 ms) and at every point above, 14 times at 9234 (14.8 against 203 ms).  The host formatter packs bases one by one, so the device pays off
// earlier than for SAM.  MM355_BAM_MIN_HITS=<n> overrides (read per call: the tests switch it).
#define MM355_BAM_MIN_HITS_DEFAULT 24

// the host formatter at level 1: BamFmt with the deflating frame
struct BamDeflateFmt : BamFmt {
	static int64_t frame_host(const char *raw, int64_t n, char *out) { return mm355_bgzf_deflate_host(raw, n, out); }
};

// the host formatter's records as they are: BamFmt without the framing (a sorted call sorts them)
struct BamRawFmt : BamFmt {
	static constexpr bool FRAMED = false;
	static int64_t out_size(int64_t n) { return n; }
};

// ---- one BAM call.  Every entry point below states its call as a plan and forwards, after its own argument checks, to bam_format (a batch
// result in hand) or bam_map_format (reads in hand).  level, span and packed (RecLast) reach the device formatter's last step in the RecCall;
// ax: the copied tags; the result goes to *text as BGZF blocks or, a sorted call, to *run as a run
struct BamPlan : RecLast {
	RecAux ax;
	mm355_text_t **text = 0; mm355_run_t **run = 0;
	BamPlan(const uint8_t *const *aux, const int32_t *aux_len, const int32_t *aux_mod) { if (aux) { ax.aux = aux; ax.len = aux_len; ax.mod = aux_mod; } }
	bool sorted() const { return run != 0; }
};
static BamPlan bam_plan_blocks(const uint8_t *const *aux, const int32_t *aux_len, const int32_t *aux_mod, int level, mm355_text_t **out)
{ BamPlan p(aux, aux_len, aux_mod); p.level = level; p.text = out; return p; }
static BamPlan bam_plan_run(const uint8_t *const *aux, const int32_t *aux_len, const int32_t *aux_mod, bool span, bool packed, mm355_run_t **out)
{ BamPlan p(aux, aux_len, aux_mod); p.span = span; p.packed = packed; p.run = out; return p; }
// false: the caller gave no place for the result; otherwise that place is cleared
static bool bam_plan_open(const BamPlan &p)
{
	if (p.text == 0 && p.run == 0) return false;
	if (p.sorted()) *p.run = 0; else *p.text = 0;
	return true;
}

// a run from the device formatter: the kernels an unsorted call launches, then the sort where the records were formed
static int bam_run_device(mm355_ctx_t *c, const mm355_hits_t *H, const char *const *qnames, const char *const *seqs, const int32_t *qlens, const char *const *quals,
                          const int32_t *rep_len, int sam_flags, const BamPlan &p)
{
	const int rc = p.ax.aux? rec_format_device_to<BamRunFmtOf<BamAuxDevFmt>, mm355_run_t>(c, H, qnames, seqs, qlens, quals, rep_len, sam_flags, true, p.run, p.ax, p)
	                       : rec_format_device_to<BamRunFmtOf<BamDevFmt>, mm355_run_t>(c, H, qnames, seqs, qlens, quals, rep_len, sam_flags, true, p.run, p.ax, p);
	if (rc) return rc;
	mm355_run_t *R = *p.run;
	R->on_device = 1;
	// the empty run comes from rec_text_empty, which knows no plan: the arrays a run with spans and a packed run always have (no member)
	if ((p.span && R->span == 0 && (R->span = (int64_t*)malloc(8)) == 0) || (p.packed && !R->packed && (R->blk_off = (int64_t*)calloc(1, 8)) == 0)) {
		mm355_free_run_host(R); *p.run = 0;
		return MM355_ENOMEM;
	}
	if (p.packed) R->packed = 1;
	return 0;
}
// a run from the host formatter: its unframed records, the host sort and, packed, the serial coder (the device's bytes)
static int bam_run_host(const mm355_hits_t *H, const char *const *qnames, const char *const *seqs, const int32_t *qlens, const char *const *quals, const int32_t *rep_len,
                        const PafNames &nm, int sam_flags, const BamPlan &p)
{
	mm355_text_t *T = 0;
	if (int rc = mm355_rec_format_host<BamRawFmt>(H, qnames, seqs, qlens, quals, rep_len, nm, sam_flags, &T, p.ax)) return rc;
	std::vector<int64_t> off((size_t)T->n_lines + 1);
	int64_t at = 0;
	for (int64_t i = 0; i < T->n_lines; ++i) { off[(size_t)i] = at; at += (int64_t)bam_rec_u32((const uint8_t*)T->text + at) + 4; }   // (the writer's own block_size words)
	off[(size_t)T->n_lines] = at;
	const double t0 = mm355_now_ms();
	int rc = at != T->n_text? MM355_EINVAL : p.span? bam_span_check(T->text, off.data(), T->n_lines) : 0;
	if (rc == 0) rc = p.span? bam_sort_run_span_host(T->text, T->n_text, off.data(), T->n_lines, p.run) : bam_sort_run_host(T->text, T->n_text, off.data(), T->n_lines, p.run);
	if (rc == 0) (*p.run)->ms_sort = mm355_now_ms() - t0;
	if (rc == 0 && p.packed && (rc = bam_run_pack_host(*p.run)) != 0) { mm355_free_run_host(*p.run); *p.run = 0; }
	mm355_free_text_host(T);
	return rc;
}

// format: the records of a batch result as the plan says -- the input check, the choice of formatter, blocks or a run
static int bam_format(mm355_ctx_t *c, const mm355_mapopt_t *mo, const mm355_hits_t *H, const char *const *qnames, const char *const *seqs, const int32_t *qlens,
                      const char *const *quals, const int32_t *rep_len, int sam_flags, int where, const BamPlan &p)
{
	if (!bam_plan_open(p)) return MM355_EINVAL;
	if (c == 0 || mo == 0 || H == 0 || where < MM355_PAF_AUTO || where > MM355_PAF_DEVICE || p.level < 0 || p.level > 1) return MM355_EINVAL;
	if (c->mi == 0) return MM355_ENOIDX;
	const PafNames nm = { c->mi->names.data(), c->mi->n_seq };
	if (int rc = mm355_bam_check_aux(H, nm, (mo->flag & MMF_CIGAR) != 0, qnames, seqs, qlens, rep_len, sam_flags, p.ax)) return rc;
	if (p.sorted())
		return rec_where(where, H->n_hits, "MM355_BAM_MIN_HITS", MM355_BAM_MIN_HITS_DEFAULT) == MM355_PAF_DEVICE? bam_run_device(c, H, qnames, seqs, qlens, quals, rep_len, sam_flags, p)
		                                                                                                   : bam_run_host(H, qnames, seqs, qlens, quals, rep_len, nm, sam_flags, p);
	return rec_format_where(where, H->n_hits, "MM355_BAM_MIN_HITS", MM355_BAM_MIN_HITS_DEFAULT,
	                        [&] { return p.level? mm355_rec_format_host<BamDeflateFmt>(H, qnames, seqs, qlens, quals, rep_len, nm, sam_flags, p.text, p.ax)
	                                            : mm355_bam_format_host(H, qnames, seqs, qlens, quals, rep_len, nm, sam_flags, p.text, p.ax); },
	                        [&] { return p.ax.aux? rec_format_device_to<BamAuxDevFmt, mm355_text_t>(c, H, qnames, seqs, qlens, quals, rep_len, sam_flags, true, p.text, p.ax, p)
	                                             : rec_format_device_to<BamDevFmt, mm355_text_t>(c, H, qnames, seqs, qlens, quals, rep_len, sam_flags, true, p.text, p.ax, p); }, p.text);
}

// map, then format: the reads mapped with rep_len kept, then bam_format on the result
static int bam_map_format(mm355_ctx_t *c, const mm355_mapopt_t *mo, int64_t n_reads, const char *const *seqs, const int32_t *lens, const char *const *names,
                          const char *const *quals, int flags, int sam_flags, int where, const BamPlan &p)
{
	if (!bam_plan_open(p)) return MM355_EINVAL;
	if (p.level < 0 || p.level > 1 || (p.ax.aux && (p.ax.len == 0 || p.ax.mod == 0))) return MM355_EINVAL;   // (before anything is mapped)
	if (mo && !(mo->flag & MMF_CIGAR)) return MM355_EINVAL;
	mm355_hits_t *H = 0; const int32_t *rep_len = 0;
	int rc = mm355_map_batch_rl(c, mo, n_reads, seqs, lens, names, flags | MM355_OUT_TAGS, &H, &rep_len);
	if (rc) return rc;
	rc = bam_format(c, mo, H, names, seqs, lens, quals, rep_len, sam_flags, where, p);
	mm355_free_hits(H);
	return rc;
}

extern "C" int mm355_bam_format_aux(mm355_ctx_t *c, const mm355_mapopt_t *mo, const mm355_hits_t *H, const char *const *qnames, const char *const *seqs,
                                    const int32_t *qlens, const char *const *quals, const int32_t *rep_len, const uint8_t *const *aux, const int32_t *aux_len,
                                    const int32_t *aux_mod, int sam_flags, int where, int level, mm355_text_t **out)
{
	return bam_format(c, mo, H, qnames, seqs, qlens, quals, rep_len, sam_flags, where, bam_plan_blocks(aux, aux_len, aux_mod, level, out));
}

extern "C" int mm355_bam_format_deflate(mm355_ctx_t *c, const mm355_mapopt_t *mo, const mm355_hits_t *H, const char *const *qnames, const char *const *seqs,
                                        const int32_t *qlens, const char *const *quals, const int32_t *rep_len, int sam_flags, int where, int level, mm355_text_t **out)
{
	return mm355_bam_format_aux(c, mo, H, qnames, seqs, qlens, quals, rep_len, 0, 0, 0, sam_flags, where, level, out);
}

extern "C" int mm355_bam_format(mm355_ctx_t *c, const mm355_mapopt_t *mo, const mm355_hits_t *H, const char *const *qnames, const char *const *seqs,
                                const int32_t *qlens, const char *const *quals, const int32_t *rep_len, int sam_flags, int where, mm355_text_t **out)
{
	return mm355_bam_format_aux(c, mo, H, qnames, seqs, qlens, quals, rep_len, 0, 0, 0, sam_flags, where, 0, out);
}

extern "C" int mm355_map_batch_bam_aux(mm355_ctx_t *c, const mm355_mapopt_t *mo, int64_t n_reads, const char *const *seqs, const int32_t *lens,
                                       const char *const *names, const char *const *quals, const uint8_t *const *aux, const int32_t *aux_len, const int32_t *aux_mod,
                                       int flags, int sam_flags, int where, int level, mm355_text_t **out)
{
	return bam_map_format(c, mo, n_reads, seqs, lens, names, quals, flags, sam_flags, where, bam_plan_blocks(aux, aux_len, aux_mod, level, out));
}

extern "C" int mm355_map_batch_bam_deflate(mm355_ctx_t *c, const mm355_mapopt_t *mo, int64_t n_reads, const char *const *seqs, const int32_t *lens,
                                           const char *const *names, const char *const *quals, int flags, int sam_flags, int where, int level, mm355_text_t **out)
{
	return mm355_map_batch_bam_aux(c, mo, n_reads, seqs, lens, names, quals, 0, 0, 0, flags, sam_flags, where, level, out);
}

extern "C" int mm355_map_batch_bam(mm355_ctx_t *c, const mm355_mapopt_t *mo, int64_t n_reads, const char *const *seqs, const int32_t *lens,
                                   const char *const *names, const char *const *quals, int flags, int sam_flags, int where, mm355_text_t **out)
{
	return mm355_map_batch_bam_aux(c, mo, n_reads, seqs, lens, names, quals, 0, 0, 0, flags, sam_flags, where, 0, out);
}

// ---- sorted calls
extern "C" void mm355_free_run(mm355_run_t *r) { mm355_free_run_host(r); }

extern "C" int mm355_bam_gather(const void *base, int64_t base_len, const int64_t *src_off, const int64_t *len, int64_t n, void *out, int64_t out_cap)
{
	return bam_gather(base, base_len, src_off, len, n, out, out_cap);
}

// mm355_bam_sort and, with span, mm355_bam_sort_span
static int bam_sort_stage(mm355_ctx_t *c, const void *rec, int64_t n_bytes, const int64_t *rec_off, int64_t n_rec, int where, bool span, mm355_run_t **out)
{
	if (out == 0) return MM355_EINVAL;
	*out = 0;
	if (where < MM355_PAF_AUTO || where > MM355_PAF_DEVICE || (where == MM355_PAF_DEVICE && c == 0)) return MM355_EINVAL;
	if (int rc = bam_sort_check(rec, n_bytes, rec_off, n_rec)) return rc;
	if (span)
		if (int rc = bam_span_check(rec, rec_off, n_rec)) return rc;
	const double t0 = mm355_now_ms();
	// AUTO: the host, as for the bare wrap -- the bytes are the caller's, in host memory
	if (where != MM355_PAF_DEVICE || n_rec == 0) {
		if (int rc = span? bam_sort_run_span_host(rec, n_bytes, rec_off, n_rec, out) : bam_sort_run_host(rec, n_bytes, rec_off, n_rec, out)) return rc;
		(*out)->ms_sort = mm355_now_ms() - t0;
		return 0;
	}
	HIPCHK(hipSetDevice(c->dev));
	if (c->rec_text.ensure((size_t)n_bytes + 64) || c->rec_work.ensure((size_t)(n_rec + 1) * 8)) return MM355_ENOMEM;
	HIPCHK(hipMemcpyAsync(c->rec_text.p, rec, (size_t)n_bytes, hipMemcpyHostToDevice, c->st));
	HIPCHK(hipMemcpyAsync(c->rec_work.p, rec_off, (size_t)(n_rec + 1) * 8, hipMemcpyHostToDevice, c->st));
	mm355_run_t *R = mm355_run_alloc(n_rec, n_bytes, span);
	if (R == 0) { (void)mm355_wait_stream(c->st); return MM355_ENOMEM; }     // (the uploads read the caller's memory)
	double k_us = 0, sp_us = 0;
	const bool times = bam_times_on();
	const int rc = bam_sort_device(c, (const char*)c->rec_text.p, n_bytes, (const int64_t*)c->rec_work.p, n_rec, R, &k_us, span && times? &sp_us : 0);
	if (rc) { (void)mm355_wait_stream(c->st); mm355_free_run_host(R); return rc; }
	if (times) {
		fprintf(stderr, "[mm355] bam_sort_times stage records %lld stream_bytes %lld k_rec_key_sort_permute_us %.1f total_ms %.3f", (long long)n_rec, (long long)n_bytes, k_us, mm355_now_ms() - t0);
		if (span) fprintf(stderr, " k_rec_span_us %.1f", sp_us);
		fprintf(stderr, "\n");
	}
	R->ms_sort = k_us / 1e3; R->on_device = 1;
	*out = R;
	return 0;
}
extern "C" int mm355_bam_sort(mm355_ctx_t *c, const void *rec, int64_t n_bytes, const int64_t *rec_off, int64_t n_rec, int where, mm355_run_t **out)
{
	return bam_sort_stage(c, rec, n_bytes, rec_off, n_rec, where, false, out);
}
extern "C" int mm355_bam_sort_span(mm355_ctx_t *c, const void *rec, int64_t n_bytes, const int64_t *rec_off, int64_t n_rec, int where, mm355_run_t **out)
{
	return bam_sort_stage(c, rec, n_bytes, rec_off, n_rec, where, true, out);
}

// ---- the sorted calls that map: bam_map_format with a run plan
extern "C" int mm355_map_batch_bam_run(mm355_ctx_t *c, const mm355_mapopt_t *mo, int64_t n_reads, const char *const *seqs, const int32_t *lens,
                                       const char *const *names, const char *const *quals, const uint8_t *const *aux, const int32_t *aux_len, const int32_t *aux_mod,
                                       int flags, int sam_flags, int where, mm355_run_t **out)
{
	return bam_map_format(c, mo, n_reads, seqs, lens, names, quals, flags, sam_flags, where, bam_plan_run(aux, aux_len, aux_mod, false, false, out));
}
extern "C" int mm355_map_batch_bam_run_span(mm355_ctx_t *c, const mm355_mapopt_t *mo, int64_t n_reads, const char *const *seqs, const int32_t *lens,
                                            const char *const *names, const char *const *quals, const uint8_t *const *aux, const int32_t *aux_len, const int32_t *aux_mod,
                                            int flags, int sam_flags, int where, mm355_run_t **out)
{
	return bam_map_format(c, mo, n_reads, seqs, lens, names, quals, flags, sam_flags, where, bam_plan_run(aux, aux_len, aux_mod, true, false, out));
}
extern "C" int mm355_map_batch_bam_run_packed(mm355_ctx_t *c, const mm355_mapopt_t *mo, int64_t n_reads, const char *const *seqs, const int32_t *lens,
                                              const char *const *names, const char *const *quals, const uint8_t *const *aux, const int32_t *aux_len, const int32_t *aux_mod,
                                              int flags, int sam_flags, int where, int want_span, mm355_run_t **out)
{
	return bam_map_format(c, mo, n_reads, seqs, lens, names, quals, flags, sam_flags, where, bam_plan_run(aux, aux_len, aux_mod, want_span != 0, true, out));
}

// ---- the merge step of compressed runs (mm355_bammerge.h: the plan and the host step)
// The step on the device.  One upload through the context's pinned staging: the compressed slices back to back, the member table (cdata
// offsets rebased to the upload), every record's place in the inflated bytes, the lengths, the carry.  Then k_bgzf_inflate into
// c->bam_sorted, the lengths' and tile counts' scans and k_rec_gather into c->rec_text behind the carry, the deflate or framing kernels on the
// whole payloads, and the blocks, the members' status words and the leftover bytes down.  A refused member: MM355_EIO, nothing returned.
static int bam_merge_step_device(mm355_ctx *c, const BamMergeIn &a, const BamMergePlan &p, mm355_text_t **out, void *carry_out, int64_t *n_carry_out)
{
	hipStream_t st = c->st;
	const int64_t n = a.n_rec, n_mem = (int64_t)p.mem.size();
	const int64_t max_tiles = p.n_rec_bytes / BAM_TILE + n;
	if (max_tiles > (int64_t)INT32_MAX || bgzf_blocks(p.n_now) > (int64_t)INT32_MAX) return MM355_EINVAL;
	const bool times = bam_times_on();
	HIPCHK(hipSetDevice(c->dev));
	// the upload's layout
	const size_t u_mem = up256((size_t)p.n_in + 64), u_src = u_mem + up256((size_t)n_mem * sizeof(BgzfMember)), u_len = u_src + up256((size_t)n * 8),
	             u_carry = u_len + up256((size_t)(n + 1) * 8), u_end = u_carry + up256((size_t)a.n_carry);
	size_t tb_scan = 0;
	(void)rocprim::exclusive_scan(nullptr, tb_scan, (int64_t*)0, (int64_t*)0, (int64_t)0, (size_t)n + 1, rocprim::plus<int64_t>(), st);
	const size_t w8 = up256((size_t)(n + 1) * 8), w_nt = 0, w_noff = w8, w_to = 2 * w8, w_status = 3 * w8, w_tmp = w_status + up256((size_t)n_mem * 4 + 4);
	const size_t h_status = 64;                // (the first bytes of h_rec_out are the deflate stage's total)
	if (c->h_rec_in.ensure(u_end) || c->rec_in.ensure(u_end) || c->rec_work.ensure(w_tmp + up256(tb_scan + 256)) || c->bam_sorted.ensure((size_t)p.n_inflated + 64) ||
	    c->rec_text.ensure((size_t)p.n_stream + 64) || c->h_rec_out.ensure(h_status + (size_t)n_mem * 4 + 64)) return MM355_ENOMEM;
	char *h = (char*)c->h_rec_in.p, *d = (char*)c->rec_in.p, *dw = (char*)c->rec_work.p;
	{
		int64_t at = 0;                        // the slices back to back; a member's cdata moves with its slice
		BgzfMember *hm = (BgzfMember*)(h + u_mem);
		size_t m = 0;
		for (int64_t s = 0; s < a.n_slice; ++s) {
			if (a.slice_bytes[s]) memcpy(h + at, (const char*)a.base + a.slice_at[s], (size_t)a.slice_bytes[s]);
			for (; m < (size_t)p.slice_mem[(size_t)s + 1]; ++m) { hm[m] = p.mem[m]; hm[m].c_off += at - a.slice_at[s]; }
			at += a.slice_bytes[s];
		}
		if (n) { memcpy(h + u_src, p.src.data(), (size_t)n * 8); memcpy(h + u_len, a.rec_len, (size_t)n * 8); }
		*(int64_t*)(h + u_len + (size_t)n * 8) = 0;
		if (a.n_carry) memcpy(h + u_carry, a.carry, (size_t)a.n_carry);
	}
	struct StepEvents { hipEvent_t v[4] = { 0, 0, 0, 0 }; ~StepEvents() { for (hipEvent_t e : v) if (e) (void)hipEventDestroy(e); } } ev;   // (inflate and gather, each timed alone)
	bool timed = times;
	for (int i = 0; i < 4 && timed; ++i) timed = hipEventCreate(&ev.v[i]) == hipSuccess;
	HIPCHK(hipMemcpyAsync(d, h, u_end, hipMemcpyHostToDevice, st));
	int32_t *d_status = (int32_t*)(dw + w_status), *h_st = (int32_t*)((char*)c->h_rec_out.p + h_status);
	if (timed) (void)hipEventRecord(ev.v[0], st);
	if (n_mem) {
		if (int rc = bgzf_inflate_launch(c->dev, st, (const unsigned char*)d, (const BgzfMember*)(d + u_mem), n_mem, (char*)c->bam_sorted.p, d_status)) return rc;
	}
	if (timed) (void)hipEventRecord(ev.v[1], st);      // (the kernel alone: the status words' copy comes behind the event)
	if (n_mem) HIPCHK(hipMemcpyAsync(h_st, d_status, (size_t)n_mem * 4, hipMemcpyDeviceToHost, st));
	char *stream = (char*)c->rec_text.p;
	if (a.n_carry) HIPCHK(hipMemcpyAsync(stream, d + u_carry, (size_t)a.n_carry, hipMemcpyDeviceToDevice, st));
	if (n) {
		const int64_t *d_len = (const int64_t*)(d + u_len);
		int64_t *d_nt = (int64_t*)(dw + w_nt), *d_noff = (int64_t*)(dw + w_noff), *d_to = (int64_t*)(dw + w_to);
		hipLaunchKernelGGL(k_rec_tiles, dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, st, d_len, n, d_nt);
		HIPCHK(hipGetLastError());
		HIPCHK(rocprim::exclusive_scan(dw + w_tmp, tb_scan, d_len, d_noff, (int64_t)0, (size_t)n + 1, rocprim::plus<int64_t>(), st));
		HIPCHK(rocprim::exclusive_scan(dw + w_tmp, tb_scan, d_nt, d_to, (int64_t)0, (size_t)n + 1, rocprim::plus<int64_t>(), st));
		if (timed) (void)hipEventRecord(ev.v[2], st);  // (k_rec_gather alone: the carry's copy, k_rec_tiles and the scans lie in front of the event)
		if (max_tiles > 0) {
			hipLaunchKernelGGL(k_rec_gather, dim3((unsigned)max_tiles), dim3(256), 0, st, (const char*)c->bam_sorted.p, (const int64_t*)(d + u_src), (const int64_t*)d_noff,
			                   (const int64_t*)d_to, n, stream + a.n_carry);
			HIPCHK(hipGetLastError());
		}
	}
	if (timed) { if (n == 0) (void)hipEventRecord(ev.v[2], st); (void)hipEventRecord(ev.v[3], st); }
	// the blocks of the whole payloads
	int64_t n_out = bgzf_size(p.n_now), n_stored = 0;
	double f_us = 0;
	if (a.level && p.n_now)
		if (int rc = bam_deflate_device(c, stream, p.n_now, &n_out, timed, &f_us, &n_stored)) return rc;
	mm355_text_t *T = mm355_text_alloc(0, bgzf_blocks(p.n_now), n_out);
	if (T == 0) { (void)mm355_wait_stream(st); return MM355_ENOMEM; }
	T->line_off[0] = 0;
	int rc = a.level? bam_blocks_back(c, p.n_now? n_out : 0, T->text) : bam_frame_device(c, stream, p.n_now, T->text, timed, &f_us);
	if (rc == 0 && p.n_now == 0 && mm355_wait_stream(st) != hipSuccess) rc = MM355_EHIP;     // (bam_frame_device has nothing to wait for then)
	if (rc == 0)
		for (int64_t b = 0; b < n_mem; ++b)
			if (h_st[b]) { rc = MM355_EIO; break; }
	if (rc == 0 && p.n_left) {                 // (carry_out may be `carry`: the upload that read it has long been waited for)
		hipError_t e = hipMemcpyAsync(carry_out, stream + p.n_now, (size_t)p.n_left, hipMemcpyDeviceToHost, st);
		if (e == hipSuccess) e = mm355_wait_stream(st);
		if (e != hipSuccess) rc = MM355_EHIP;
	}
	if (rc) { (void)mm355_wait_stream(st); mm355_free_text_host(T); return rc; }
	*n_carry_out = p.n_left;
	if (timed) {
		float ms_i = 0, ms_g = 0;
		(void)hipEventElapsedTime(&ms_i, ev.v[0], ev.v[1]); (void)hipEventElapsedTime(&ms_g, ev.v[2], ev.v[3]);
		fprintf(stderr, "[mm355] bam_merge_times members %lld bytes_in %lld records %lld bytes_out %lld k_bgzf_inflate_us %.1f k_rec_gather_us %.1f %s %.1f\n", (long long)n_mem,
		        (long long)p.n_in, (long long)n, (long long)n_out, (double)ms_i * 1e3, (double)ms_g * 1e3, a.level? "k_bgzf_deflate_compact_us" : "k_bgzf_frame_us", f_us);
	}
	T->on_device = 1;
	*out = T;
	return 0;
}

extern "C" int mm355_bam_merge_step(mm355_ctx_t *c, const void *base, int64_t base_len, const int64_t *slice_at, const int64_t *slice_bytes,
                                    const int64_t *slice_raw_at, int64_t n_slice, const int32_t *rec_slice, const int64_t *rec_at, const int64_t *rec_len,
                                    int64_t n_rec, const void *carry, int64_t n_carry, int final, int where, int level, mm355_text_t **out,
                                    void *carry_out, int64_t *n_carry_out)
{
	if (out == 0) return MM355_EINVAL;
	*out = 0;
	if (carry_out == 0 || n_carry_out == 0 || where < MM355_PAF_AUTO || where > MM355_PAF_DEVICE || (where == MM355_PAF_DEVICE && c == 0)) return MM355_EINVAL;
	const BamMergeIn a = { base, base_len, slice_at, slice_bytes, slice_raw_at, n_slice, rec_slice, rec_at, rec_len, n_rec, carry, n_carry, final, level };
	try {
		BamMergePlan p;
		if (int rc = bam_merge_plan(a, p)) return rc;
		const double t0 = mm355_now_ms();
		// AUTO: the host, as for the bare wrap
		const int rc = where == MM355_PAF_DEVICE? bam_merge_step_device(c, a, p, out, carry_out, n_carry_out) : bam_merge_step_host(a, p, out, carry_out, n_carry_out);
		if (rc) { if (*out) { mm355_free_text_host(*out); *out = 0; } return rc; }
		(*out)->ms_format = mm355_now_ms() - t0;
		return 0;
	} catch (const std::bad_alloc&) { return MM355_ENOMEM; }
}

// ---- the .bai builder (mm355_bai.h): host code, keys, spans, lengths and blocks
struct mm355_bai { BaiBuilder b; };
extern "C" int mm355_bai_open(int32_t n_ref, int64_t first_block_at, mm355_bai_t **out)
{
	if (out == 0) return MM355_EINVAL;
	*out = 0;
	if (n_ref < 0 || first_block_at < 0) return MM355_EINVAL;
	mm355_bai *h = new (std::nothrow) mm355_bai;
	if (h == 0) return MM355_ENOMEM;
	h->b.n_ref = n_ref; h->b.first_block_at = first_block_at;
	*out = h;
	return 0;
}
extern "C" int mm355_bai_records(mm355_bai_t *h, const uint64_t *key, const int64_t *span, const int64_t *len, int64_t n)
{
	if (h == 0) return MM355_EINVAL;
	try { return h->b.records(key, span, len, n); } catch (const std::bad_alloc&) { return MM355_ENOMEM; }
}
extern "C" int mm355_bai_blocks(mm355_bai_t *h, const void *bytes, int64_t n)
{
	if (h == 0) return MM355_EINVAL;
	try { return h->b.blocks(bytes, n); } catch (const std::bad_alloc&) { return MM355_ENOMEM; }
}
extern "C" int mm355_bai_finish(mm355_bai_t *h, mm355_text_t **out)
{
	if (out == 0) return MM355_EINVAL;
	*out = 0;
	if (h == 0) return MM355_EINVAL;
	try {
		std::string o;
		if (int rc = h->b.finish(o)) return rc;
		mm355_text_t *T = mm355_text_alloc(0, 0, (int64_t)o.size());
		if (T == 0) return MM355_ENOMEM;
		memcpy(T->text, o.data(), o.size());
		T->n_reads = h->b.n_raw_chunks; T->n_lines = h->b.n_chunks;
		*out = T;
		return 0;
	} catch (const std::bad_alloc&) { return MM355_ENOMEM; }
}
extern "C" void mm355_bai_close(mm355_bai_t *h) { delete h; }

extern "C" int mm355_bgzf_deflate(mm355_ctx_t *c, const void *data, int64_t n, int where, int level, mm355_text_t **out)
{
	if (out == 0) return MM355_EINVAL;
	*out = 0;
	if (n < 0 || (n > 0 && data == 0) || where < MM355_PAF_AUTO || where > MM355_PAF_DEVICE || (where == MM355_PAF_DEVICE && c == 0) || level < 0 || level > 1) return MM355_EINVAL;
	const double t0 = mm355_now_ms();
	const bool times = level && bam_times_on();
	int64_t n_out = bgzf_size(n), n_stored = 0;
	double k_us = 0;
	// AUTO: the host.  The bytes are the caller's, in host memory: the device would frame them between an upload and a copy back that each
	// move as much as the host's crc32 reads
	if (where != MM355_PAF_DEVICE) {
		if (int rc = mm355_bgzf_wrap_host(data, n, out)) return rc;               // (stored blocks: the largest a level-1 result can be)
		if (level) {
			std::vector<char> z((size_t)n_out + 1);
			n_out = mm355_bgzf_deflate_host((const char*)data, n, z.data(), &n_stored);
			memcpy((*out)->text, z.data(), (size_t)n_out);
			(*out)->n_text = n_out; (*out)->text[n_out] = 0;
		}
	} else {
		HIPCHK(hipSetDevice(c->dev));
		if (c->rec_text.ensure((size_t)n + 64)) return MM355_ENOMEM;
		if (n) HIPCHK(hipMemcpyAsync(c->rec_text.p, data, (size_t)n, hipMemcpyHostToDevice, c->st));
		if (level)
			if (int rc = bam_deflate_device(c, (const char*)c->rec_text.p, n, &n_out, times, &k_us, &n_stored)) return rc;
		mm355_text_t *T = mm355_text_alloc(0, bgzf_blocks(n), n_out);
		if (T == 0) return MM355_ENOMEM;
		T->line_off[0] = 0;
		const int rc = level? bam_blocks_back(c, n_out, T->text) : bam_frame_device(c, (const char*)c->rec_text.p, n, T->text, false, &k_us);
		if (rc) { mm355_free_text_host(T); return rc; }
		*out = T;
	}
	if (times) bam_deflate_times("wrap", n, n_out, n_stored, k_us, where == MM355_PAF_DEVICE);
	(*out)->on_device = where == MM355_PAF_DEVICE;
	(*out)->ms_format = mm355_now_ms() - t0;
	return 0;
}

extern "C" int mm355_bgzf_wrap(mm355_ctx_t *c, const void *data, int64_t n, int where, mm355_text_t **out) { return mm355_bgzf_deflate(c, data, n, where, 0, out); }
