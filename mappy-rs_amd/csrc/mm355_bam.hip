// mm355_bam.hip -- the BAM records of a batch result and their BGZF framing, written on the device.  The record is stated once, in
// mm355_bam.h (bam_emit_record, templated on a sink); here the same emitter runs with two device sinks, a wave per RECORD, as the SAM
// writer runs its lines (mm355_sam.hip; the upload and the tables are that writer's, mm355_samdev.h):
//   k_bam_len     the lanes add up the reference length of the CIGAR (wave reduction: the bin needs it); lane 0 runs the emitter with the
//                 counting sink and counts the record's SEQ / QUAL tiles.  Two exclusive scans give every record's offset in the unframed
//                 stream and its first tile; both totals cross to the host with the call's one synchronisation.
//   k_bam_fields  lane 0 runs the emitter with the writing sink: the fixed fields and the tags go straight to the stream byte by byte;
//                 qname, the CIGAR words, cs, MD and the CG words are noted down and copied by the wave (a full table falls back to lane 0);
//                 SEQ and QUAL are only noted down, two runs per record.
//   k_bam_bulk    the bulk of a record.  Work item = (record, field, tile of BAM_TILE output bytes), one block each.  A thread owns an
//                 aligned 16-byte piece of the destination.  SEQ: 32 bases from nine aligned source dwords shifted into place (reversed:
//                 mirrored, which swaps the nibbles' order with the bytes'), each through the 256-entry code table in LDS (the reversed
//                 table is the code of the complement, so U and u need no special case), two codes per byte.  QUAL: 16 bytes minus 33,
//                 mirrored on the reverse strand; no quality: 0xFF.  The ragged head and tail of a tile, and the padded last byte of an
//                 odd SEQ, are byte stores.
//   k_bgzf_frame  one workgroup per BGZF block of the unframed stream: header, payload (aligned 16-byte stores from shifted source dwords),
//                 CRC-32 by lanes with fixed-length chunks read 16 bytes at a time and a table in LDS (mm355_bam.h: bgzf_lane_crc, the combine
//                 and the tail of a short last block), ISIZE.  Block b
//                 starts at b * (0xff00 + 31): the output offsets are arithmetic.
// Records are written into an unframed buffer and framed by a pass of their own: one more read and write of the stream in HBM.
// Every byte has one writer: plain vector stores, no atomics.
#include <rocprim/device/device_scan.hpp>
#include "mm355_wave.h"
#include "mm355_samdev.h"
#include "mm355_bam.h"

#define BAM_TILE 4096         // output bytes of one k_bam_bulk block: 256 threads x 16 bytes
#define BAM_RUNS 5            // qname, CIGAR, cs, MD, CG

MM_HD int64_t bam_tiles(int64_t n) { return (n + BAM_TILE - 1) / BAM_TILE; }

// a run the wave copies after lane 0 has laid the record out: len bytes from src to byte `at` of the record
struct BamRun { const char *src; int64_t at, len; };
// a SEQ / QUAL run of a record: n bases or bytes from src to byte `dst` of the stream.  mode 0 / 1: bases packed two per byte, forwards /
// last base first and complemented; 2 / 3: quality bytes minus 33, forwards / last byte first; 4: n bytes of 0xFF
struct BamBulkRun { const char *src; int64_t dst; int32_t n, mode; };
MM_HD int64_t bam_bulk_bytes(const BamBulkRun &r) { return r.mode < 2? ((int64_t)r.n + 1) / 2 : r.n; }

struct BamDevCount : BamCountSink {
	int64_t tiles = 0;
	__device__ void seq4(const char *, int64_t l, bool) { n += (l + 1) / 2; tiles += bam_tiles((l + 1) / 2); }
	__device__ void qual(const char *, int64_t l, bool) { n += l; tiles += bam_tiles(l); }
	__device__ void fill(int64_t l) { n += l; tiles += bam_tiles(l); }
};
struct BamDevWrite {
	unsigned char *p; int64_t n = 0, rec_at; BamRun *runs; BamBulkRun *bulk; int n_runs = 0, n_bulk = 0;
	__device__ void ch(char c) { p[n++] = (unsigned char)c; }
	__device__ void u8(uint32_t v) { p[n++] = (unsigned char)v; }
	__device__ void u16(uint32_t v) { u8(v & 0xff); u8(v >> 8 & 0xff); }
	__device__ void u32(uint32_t v) { u16(v & 0xffff); u16(v >> 16); }
	__device__ void bytes(const char *b, int64_t l)
	{
		if (n_runs < BAM_RUNS) { runs[n_runs++] = BamRun{ b, n, l }; n += l; }
		else for (int64_t i = 0; i < l; ++i) p[n++] = (unsigned char)b[i];
	}
	__device__ void cigar(const uint32_t *w, int64_t k) { bytes((const char*)w, 4 * k); }      // (the device is little-endian: the words as they lie)
	__device__ void note(const char *b, int64_t l, int mode) { if (n_bulk < 2) bulk[n_bulk++] = BamBulkRun{ b, rec_at + n, (int32_t)l, mode }; }   // (a record has SEQ and QUAL, no third run)
	__device__ void seq4(const char *b, int64_t l, bool rev) { note(b, l, rev? 1 : 0); n += (l + 1) / 2; }
	__device__ void qual(const char *b, int64_t l, bool rev) { note(b, l, rev? 3 : 2); n += l; }
	__device__ void fill(int64_t l) { note(0, l, 4); n += l; }
};

__global__ __launch_bounds__(256) void k_bam_len(SamDev D, int64_t *len, int64_t *reflen, int64_t *ntile)
{
	const int lane = threadIdx.x & 63;
	const int64_t l = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
	if (l >= D.n_lines) return;                // (the whole wave)
	const int32_t r = D.l_read[l], row = sam_row_of(D, l, r);
	long long rl = 0;
	if (row >= 0) {
		const mm355_hit_t &h = D.hits[D.hit_off[r] + row];
		const uint32_t *w = D.cigar + h.cigar_off;
		for (int32_t i = lane; i < h.n_cigar; i += 64) rl += bam_ref_len(w[i]);
		for (int d = 32; d > 0; d >>= 1) rl += __shfl_xor(rl, d);
	}
	if (lane == 0) {
		const SamRead R = sam_read_dev(D, r);
		BamDevCount s;
		bam_emit_record(s, SamLine{ &R, row }, rl, 0);
		len[l] = s.n; reflen[l] = rl; ntile[l] = s.tiles;
	}
}

__global__ void k_bam_line_off(const int64_t *off, const int64_t *l_first, int64_t n_reads, int64_t *line_off)
{
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i <= n_reads) line_off[i] = off[l_first[i]];
}

__global__ __launch_bounds__(256) void k_bam_fields(SamDev D, const int64_t *off, const int64_t *reflen, char *text, BamBulkRun *bulk)
{
	__shared__ BamRun runs[4][BAM_RUNS];       // per wave
	__shared__ int n_runs[4];
	const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
	const int64_t l = (int64_t)blockIdx.x * 4 + wv;
	const bool on = l < D.n_lines;
	char *rec = on? text + off[l] : text;
	if (on && lane == 0) {
		const int32_t r = D.l_read[l];
		const SamRead R = sam_read_dev(D, r);
		bulk[2 * l] = bulk[2 * l + 1] = BamBulkRun{ 0, 0, 0, 4 };
		BamDevWrite s; s.p = (unsigned char*)rec; s.rec_at = off[l]; s.runs = runs[wv]; s.bulk = bulk + 2 * l;
		bam_emit_record(s, SamLine{ &R, sam_row_of(D, l, r) }, reflen[l], (uint32_t)(off[l + 1] - off[l] - 4));
		n_runs[wv] = s.n_runs;
	}
	__syncthreads();
	if (!on) return;
	const int nr = n_runs[wv];
	for (int r = 0; r < nr; ++r) {
		const char *src = runs[wv][r].src; char *dst = rec + runs[wv][r].at;
		const int64_t n = runs[wv][r].len;
		for (int64_t i = lane; i < n; i += 64) dst[i] = src[i];
	}
}

// four bytes through the code table, two codes per byte: the 16 bits of two output bytes
__device__ __forceinline__ uint32_t bam_pack4(uint32_t x, const unsigned char *cd)
{
	return (uint32_t)cd[x & 0xff] << 4 | (uint32_t)cd[x >> 8 & 0xff] | (uint32_t)cd[x >> 16 & 0xff] << 12 | (uint32_t)cd[x >> 24] << 8;
}
__device__ __forceinline__ uint32_t bam_minus33(uint32_t x)
{
	return ((x & 0xff) - 33 & 0xff) | ((x >> 8 & 0xff) - 33 & 0xff) << 8 | ((x >> 16 & 0xff) - 33 & 0xff) << 16 | ((x >> 24) - 33 & 0xff) << 24;
}

__global__ __launch_bounds__(256) void k_bam_bulk(const BamBulkRun *bulk, const int64_t *tile_off, int64_t n_lines, char *text)
{
	__shared__ unsigned char code[2][256];     // forwards; on the reverse strand: the code of the complement
	code[0][threadIdx.x] = bam_code((unsigned char)threadIdx.x);
	code[1][threadIdx.x] = bam_code(sam_comp((unsigned char)threadIdx.x));
	const int64_t b = blockIdx.x;
	int64_t lo = 0, hi = n_lines;              // the last record whose first tile is <= b (records without tiles in front of it share that number)
	while (hi - lo > 1) { const int64_t mid = (lo + hi) >> 1; if (tile_off[mid] <= b) lo = mid; else hi = mid; }
	int64_t t = b - tile_off[lo];
	BamBulkRun r = bulk[2 * lo];
	if (t >= bam_tiles(bam_bulk_bytes(r))) { t -= bam_tiles(bam_bulk_bytes(r)); r = bulk[2 * lo + 1]; }
	__syncthreads();
	const int64_t nb = bam_bulk_bytes(r), n = r.n;
	const int64_t o0 = t * BAM_TILE, o1 = o0 + BAM_TILE < nb? o0 + BAM_TILE : nb;   // this tile: bytes [o0, o1) of the run
	if (t < 0 || o0 >= o1) return;
	const bool rev = (r.mode & 1) != 0;
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

// in: n bytes, readable for 8 more (whole dwords are read around a span); out: bgzf_size(n) bytes; one workgroup per block
__global__ __launch_bounds__(BGZF_LANES) void k_bgzf_frame(const char *in, int64_t n, char *out)
{
	__shared__ uint32_t tab[256], reg[BGZF_LANES], x_pow[8];
	const int tid = threadIdx.x;
	tab[tid] = crc32_tab_entry((uint32_t)tid);
	if (tid < 8) x_pow[tid] = crc32_x2n(11 + tid);
	const int64_t b = blockIdx.x, at = b * BGZF_PAYLOAD;
	const uint32_t len = (uint32_t)(n - at < BGZF_PAYLOAD? n - at : BGZF_PAYLOAD);
	const char *src = in + at;
	char *o = out + b * (BGZF_PAYLOAD + BGZF_EXTRA);
	if (tid < BGZF_HEAD) o[tid] = (char)bgzf_head_byte(tid, len);
	// the payload: a thread owns an aligned 16-byte piece of the destination, the ragged ends are byte stores
	char *dst = o + BGZF_HEAD;
	const uintptr_t d0 = (uintptr_t)dst, d1 = d0 + len;
	for (uintptr_t c = (d0 & ~(uintptr_t)15) + 16 * (uintptr_t)tid; c < d1; c += 16 * BGZF_LANES) {
		if (c >= d0 && c + 16 <= d1) {
			uint32_t v[4];
			sam_load16(src, (int64_t)(c - d0), v);
			*(uint4*)c = make_uint4(v[0], v[1], v[2], v[3]);
		} else {
			const uintptr_t e = c + 16 < d1? c + 16 : d1;
			for (uintptr_t a = c > d0? c : d0; a < e; ++a) *(char*)a = src[a - d0];
		}
	}
	__syncthreads();
	reg[tid] = bgzf_lane_crc((const unsigned char*)src, len, tid, tab);
	__syncthreads();
	for (int level = 0; level < 8; ++level) {
		uint32_t x = 0;
		const bool mine = (tid & ((2 << level) - 1)) == 0;
		if (mine) x = bgzf_crc_level(reg, tid, level, x_pow[level]);
		__syncthreads();
		if (mine) reg[tid] = x;
		__syncthreads();
	}
	if (tid == 0) {
		const uint32_t crc = ~bgzf_tail_crc((const unsigned char*)src, len, reg[0], tab);
		for (int i = 0; i < 4; ++i) { dst[len + i] = (char)(crc >> 8 * i); dst[len + 4 + i] = (char)(len >> 8 * i); }
	}
}

// ------------------------------------------------------------------ host side
// frames the n bytes at c->sam_text.p (readable for 8 more) into c->bam_out and copies the blocks to `to`; timed: the kernel between the
// context's two events, microseconds in *k_us
static int bam_frame_device(mm355_ctx *c, int64_t n, char *to, bool timed, double *k_us)
{
	hipStream_t st = c->st;
	if (n == 0) return 0;
	if (bgzf_blocks(n) > (int64_t)INT32_MAX) return MM355_EINVAL;
	if (c->bam_out.ensure((size_t)bgzf_size(n) + 64)) return MM355_ENOMEM;
	if (timed) (void)hipEventRecord(c->ev0, st);
	hipLaunchKernelGGL(k_bgzf_frame, dim3((unsigned)bgzf_blocks(n)), dim3(BGZF_LANES), 0, st, (const char*)c->sam_text.p, n, (char*)c->bam_out.p);
	HIPCHK(hipGetLastError());
	if (timed) (void)hipEventRecord(c->ev1, st);
	HIPCHK(hipMemcpyAsync(to, c->bam_out.p, (size_t)bgzf_size(n), hipMemcpyDeviceToHost, st));
	HIPCHK(mm355_wait_stream(st));
	if (timed) { float ms = 0; (void)hipEventElapsedTime(&ms, c->ev0, c->ev1); *k_us = (double)ms * 1e3; }
	return 0;
}

static int bam_format_device(mm355_ctx *c, const mm355_hits_t *H, const char *const *qnames, const char *const *seqs, const int32_t *qlens,
                             const char *const *quals, const int32_t *rep_len, int sam_flags, mm355_text_t **out)
{
	const int64_t nr = H->n_reads;
	// MM355_BAM_TIMES=1 (read per call; tools/bam_bench.py): one line on stderr with the framing kernel's time between two events
	const char *te = getenv("MM355_BAM_TIMES"); const bool times = te && *te && *te != '0';
	const double t_begin = mm355_now_ms();
	SamDev D; double t_packed;
	if (int rc = sam_upload(c, H, qnames, seqs, qlens, quals, rep_len, sam_flags, &D, &t_packed)) return rc;
	const int64_t nl = D.n_lines;
	if (nl == 0) return sam_text_empty(nr, out);   // nothing to launch
	hipStream_t st = c->st;
	// lengths and tile counts (one word more each: the scans leave the totals there), their offsets, reference lengths, line_off, the runs, scan space
	size_t tb = 0;
	(void)rocprim::exclusive_scan(nullptr, tb, (int64_t*)0, (int64_t*)0, (int64_t)0, (size_t)nl + 1, rocprim::plus<int64_t>(), st);
	const size_t w1 = up256((size_t)(nl + 1) * 8);
	const size_t w_len = 0, w_off = w_len + w1, w_nt = w_off + w1, w_to = w_nt + w1, w_rl = w_to + w1, w_lo = w_rl + w1, w_run = w_lo + up256((size_t)(nr + 1) * 8),
	             w_tmp = w_run + up256((size_t)nl * 2 * sizeof(BamBulkRun));
	if (c->sam_work.ensure(w_tmp + tb + 256)) return MM355_ENOMEM;
	char *dw = (char*)c->sam_work.p;
	int64_t *d_len = (int64_t*)(dw + w_len), *d_off = (int64_t*)(dw + w_off), *d_nt = (int64_t*)(dw + w_nt), *d_to = (int64_t*)(dw + w_to),
	        *d_rl = (int64_t*)(dw + w_rl), *d_lo = (int64_t*)(dw + w_lo);
	BamBulkRun *d_run = (BamBulkRun*)(dw + w_run);
	HIPCHK(hipMemsetAsync(d_len + nl, 0, 8, st));
	HIPCHK(hipMemsetAsync(d_nt + nl, 0, 8, st));
	const unsigned grid = (unsigned)((nl + 3) / 4);
	hipLaunchKernelGGL(k_bam_len, dim3(grid), dim3(256), 0, st, D, d_len, d_rl, d_nt);
	HIPCHK(hipGetLastError());
	HIPCHK(rocprim::exclusive_scan(dw + w_tmp, tb, d_len, d_off, (int64_t)0, (size_t)nl + 1, rocprim::plus<int64_t>(), st));
	HIPCHK(rocprim::exclusive_scan(dw + w_tmp, tb, d_nt, d_to, (int64_t)0, (size_t)nl + 1, rocprim::plus<int64_t>(), st));
	hipLaunchKernelGGL(k_bam_line_off, dim3((unsigned)((nr + 1 + 255) / 256)), dim3(256), 0, st, d_off, D.l_first, nr, d_lo);
	HIPCHK(hipGetLastError());
	int64_t *h_tot = (int64_t*)c->h_sam_out.p;
	HIPCHK(hipMemcpyAsync(h_tot, d_off + nl, 8, hipMemcpyDeviceToHost, st));
	HIPCHK(hipMemcpyAsync(h_tot + 1, d_to + nl, 8, hipMemcpyDeviceToHost, st));
	HIPCHK(mm355_wait_stream(st));
	const int64_t tot = h_tot[0], n_tiles = h_tot[1];
	// (the fixed part of a record is 36 bytes, and a tile holds at least one byte of the stream)
	if (tot < 36 * nl || n_tiles < 0 || n_tiles > tot || n_tiles > (int64_t)INT32_MAX) return MM355_EHIP;
	if (c->sam_text.ensure((size_t)tot + 64)) return MM355_ENOMEM;
	hipLaunchKernelGGL(k_bam_fields, dim3(grid), dim3(256), 0, st, D, d_off, d_rl, (char*)c->sam_text.p, d_run);
	HIPCHK(hipGetLastError());
	if (n_tiles > 0) {
		hipLaunchKernelGGL(k_bam_bulk, dim3((unsigned)n_tiles), dim3(256), 0, st, d_run, d_to, nl, (char*)c->sam_text.p);
		HIPCHK(hipGetLastError());
	}
	mm355_text_t *T = mm355_text_alloc(nr, nl, bgzf_size(tot));
	if (T == 0) return MM355_ENOMEM;
	double k_us = 0;
	hipError_t e = hipMemcpyAsync(T->line_off, d_lo, (size_t)(nr + 1) * 8, hipMemcpyDeviceToHost, st);
	int rc = e == hipSuccess? bam_frame_device(c, tot, T->text, times, &k_us) : MM355_EHIP;
	if (rc) { fprintf(stderr, "[mm355] error %d in the BAM writer (%s)\n", rc, hipGetErrorString(e)); mm355_free_text_host(T); return rc; }
	if (times)
		fprintf(stderr, "[mm355] bam_times records %lld stream_bytes %lld blocks %lld tiles %lld pack_ms %.3f k_bgzf_frame_us %.1f total_ms %.3f\n", (long long)nl,
		        (long long)tot, (long long)bgzf_blocks(tot), (long long)n_tiles, t_packed - t_begin, k_us, mm355_now_ms() - t_begin);
	*out = T;
	return 0;
}

// MM355_PAF_AUTO for BAM: the device formatter from this many hits on.  Measured with tools/bam_bench.py (profiles/bam_file.json, format_sweep:
// ms_format of the two formatters on the hits of 16 .. 9216 reads, map-ont with cs, reads of N50 8 kb with qualities): the host is ahead at 16
// hits (0.22 against 0.25 ms), the device at 24 (0.25 against 0.32 ms) and at every point above, 14 times at 9234 (14.8 against 203 ms).  The host formatter packs bases one by one, so the device pays off
// earlier than for SAM.  MM355_BAM_MIN_HITS=<n> overrides (read per call: the tests switch it).
#define MM355_BAM_MIN_HITS_DEFAULT 24

extern "C" int mm355_bam_format(mm355_ctx_t *c, const mm355_mapopt_t *mo, const mm355_hits_t *H, const char *const *qnames, const char *const *seqs,
                                const int32_t *qlens, const char *const *quals, const int32_t *rep_len, int sam_flags, int where, mm355_text_t **out)
{
	if (out == 0) return MM355_EINVAL;
	*out = 0;
	if (c == 0 || mo == 0 || H == 0 || where < MM355_PAF_AUTO || where > MM355_PAF_DEVICE) return MM355_EINVAL;
	if (c->mi == 0) return MM355_ENOIDX;
	if (int rc = mm355_bam_check(H, c->mi->n_seq, (mo->flag & MMF_CIGAR) != 0, qnames, seqs, qlens, rep_len, sam_flags)) return rc;
	const double t0 = mm355_now_ms();
	if (where == MM355_PAF_AUTO) {
		const char *e = getenv("MM355_BAM_MIN_HITS");
		const int64_t min_hits = e && *e? atoll(e) : MM355_BAM_MIN_HITS_DEFAULT;
		where = H->n_hits >= min_hits? MM355_PAF_DEVICE : MM355_PAF_HOST;
	}
	const PafNames nm = { c->mi->names.data(), c->mi->n_seq };
	const int rc = where == MM355_PAF_DEVICE? bam_format_device(c, H, qnames, seqs, qlens, quals, rep_len, sam_flags, out)
	                                        : mm355_bam_format_host(H, qnames, seqs, qlens, quals, rep_len, nm, sam_flags, out);
	if (rc) return rc;
	(*out)->on_device = where == MM355_PAF_DEVICE;
	(*out)->ms_format = mm355_now_ms() - t0;
	return 0;
}

extern "C" int mm355_map_batch_bam(mm355_ctx_t *c, const mm355_mapopt_t *mo, int64_t n_reads, const char *const *seqs, const int32_t *lens,
                                   const char *const *names, const char *const *quals, int flags, int sam_flags, int where, mm355_text_t **out)
{
	if (out == 0) return MM355_EINVAL;
	*out = 0;
	if (mo && !(mo->flag & MMF_CIGAR)) return MM355_EINVAL;    // (before anything is mapped)
	mm355_hits_t *H = 0; const int32_t *rep_len = 0;
	int rc = mm355_map_batch_rl(c, mo, n_reads, seqs, lens, names, flags | MM355_OUT_TAGS, &H, &rep_len);
	if (rc) return rc;
	rc = mm355_bam_format(c, mo, H, names, seqs, lens, quals, rep_len, sam_flags, where, out);
	mm355_free_hits(H);
	return rc;
}

extern "C" int mm355_bgzf_wrap(mm355_ctx_t *c, const void *data, int64_t n, int where, mm355_text_t **out)
{
	if (out == 0) return MM355_EINVAL;
	*out = 0;
	if (n < 0 || (n > 0 && data == 0) || where < MM355_PAF_AUTO || where > MM355_PAF_DEVICE || (where == MM355_PAF_DEVICE && c == 0)) return MM355_EINVAL;
	const double t0 = mm355_now_ms();
	// AUTO: the host.  The bytes are the caller's, in host memory: the device would frame them between an upload and a copy back that each
	// move as much as the host's crc32 reads
	if (where != MM355_PAF_DEVICE) {
		if (int rc = mm355_bgzf_wrap_host(data, n, out)) return rc;
	} else {
		HIPCHK(hipSetDevice(c->dev));
		if (c->sam_text.ensure((size_t)n + 64)) return MM355_ENOMEM;
		mm355_text_t *T = mm355_text_alloc(0, bgzf_blocks(n), bgzf_size(n));
		if (T == 0) return MM355_ENOMEM;
		T->line_off[0] = 0;
		double k_us = 0;
		hipError_t e = n? hipMemcpyAsync(c->sam_text.p, data, (size_t)n, hipMemcpyHostToDevice, c->st) : hipSuccess;
		const int rc = e == hipSuccess? bam_frame_device(c, n, T->text, false, &k_us) : MM355_EHIP;
		if (rc) { mm355_free_text_host(T); return rc; }
		*out = T;
	}
	(*out)->on_device = where == MM355_PAF_DEVICE;
	(*out)->ms_format = mm355_now_ms() - t0;
	return 0;
}
