// mm355_bam.hip -- the BAM records of a batch result and their BGZF framing, written on the device.  The record is stated once, in
// mm355_bam.h (bam_emit_record); the device record writer of mm355_recdev.h runs it, a wave per record.  What is BAM's own: the lanes sum
// the reference length of the CIGAR (the bin needs it); the fixed fields and the tags go straight to the stream byte by byte; the CIGAR
// and the CG words are runs the wave copies as they lie; SEQ and QUAL are noted down as runs and packed by
//   k_bam_bulk    work item = (record, field, tile of BAM_TILE output bytes), one block each.  A thread owns an aligned 16-byte piece of
//                 the destination.  SEQ: 32 bases from nine aligned source dwords shifted into place (reversed: mirrored, which swaps the
//                 nibbles' order with the bytes'), each through the 256-entry code table in LDS (the reversed table is the code of the
//                 complement, so U and u need no special case), two codes per byte.  QUAL: 16 bytes minus 33, mirrored on the reverse
//                 strand; no quality: 0xFF.  The ragged head and tail of a tile, and the padded last byte of an odd SEQ, are byte stores.
// and the records, written into an unframed buffer, are framed by a pass of their own (one more read and write of the stream in HBM):
//   k_bgzf_frame  one workgroup per BGZF block of the unframed stream: header, payload (aligned 16-byte stores from shifted source dwords),
//                 CRC-32 by lanes with fixed-length chunks read 16 bytes at a time and a table in LDS (mm355_bam.h: bgzf_lane_crc, the combine
//                 and the tail of a short last block), ISIZE.  Block b starts at b * (0xff00 + 31): the output offsets are arithmetic.
#include "mm355_recdev.h"
#include "mm355_bam.h"

#define BAM_TILE 4096         // output bytes of one k_bam_bulk block: 256 threads x 16 bytes

MM_HD int64_t bam_tiles(int64_t n) { return (n + BAM_TILE - 1) / BAM_TILE; }
// a SEQ / QUAL run of a record: len bases or bytes.  mode 0 / 1: bases packed two per byte, forwards / last base first and complemented;
// 2 / 3: quality bytes minus 33, forwards / last byte first; 4: len bytes of 0xFF
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
	const RecTileRun r = rec_tile_run(bulk, tile_off, n_lines, blockIdx.x, bam_run_tiles, &t);
	__syncthreads();
	const int64_t nb = bam_bulk_bytes(r), n = r.len;
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
// frames the n bytes at c->rec_text.p (readable for 8 more) into c->bam_out and copies the blocks to `to`; timed: the kernel between the
// context's two events, microseconds in *k_us
static int bam_frame_device(mm355_ctx *c, int64_t n, char *to, bool timed, double *k_us)
{
	hipStream_t st = c->st;
	if (n == 0) return 0;
	if (bgzf_blocks(n) > (int64_t)INT32_MAX) return MM355_EINVAL;
	if (c->bam_out.ensure((size_t)bgzf_size(n) + 64)) return MM355_ENOMEM;
	if (timed) (void)hipEventRecord(c->ev0, st);
	hipLaunchKernelGGL(k_bgzf_frame, dim3((unsigned)bgzf_blocks(n)), dim3(BGZF_LANES), 0, st, (const char*)c->rec_text.p, n, (char*)c->bam_out.p);
	HIPCHK(hipGetLastError());
	if (timed) (void)hipEventRecord(c->ev1, st);
	HIPCHK(hipMemcpyAsync(to, c->bam_out.p, (size_t)bgzf_size(n), hipMemcpyDeviceToHost, st));
	HIPCHK(mm355_wait_stream(st));
	if (timed) { float ms = 0; (void)hipEventElapsedTime(&ms, c->ev0, c->ev1); *k_us = (double)ms * 1e3; }
	return 0;
}

// BamFmt as the device writes it
struct BamDevFmt : BamFmt {
	struct Count : BamCountSink {
		int64_t tiles = 0;
		__device__ explicit Count(int64_t) {}
		__device__ void seq4(const char *, int64_t l, bool) { n += (l + 1) / 2; tiles += bam_tiles((l + 1) / 2); }
		__device__ void qual(const char *, int64_t l, bool) { n += l; tiles += bam_tiles(l); }
		__device__ void fill(int64_t l) { n += l; tiles += bam_tiles(l); }
	};
	struct Write : RecWrite<RUNS> {
		using RecWrite<RUNS>::RecWrite;
		__device__ void u8(uint32_t v) { p[n++] = (char)v; }
		__device__ void u16(uint32_t v) { u8(v & 0xff); u8(v >> 8 & 0xff); }
		__device__ void u32(uint32_t v) { u16(v & 0xffff); u16(v >> 16); }
		__device__ void cigar(const uint32_t *w, int64_t k) { bytes((const char*)w, 4 * k); }      // (the device is little-endian: the words as they lie)
		__device__ void seq4(const char *b, int64_t l, bool rev) { note(b, l, rev? 1 : 0); n += (l + 1) / 2; }
		__device__ void qual(const char *b, int64_t l, bool rev) { note(b, l, rev? 3 : 2); n += l; }
		__device__ void fill(int64_t l) { note(0, l, 4); n += l; }
	};
	// MM355_BAM_TIMES=1 (tools/bam_bench.py): one line on stderr with the framing kernel's time between two events
	static constexpr const char *TIMES_ENV = "MM355_BAM_TIMES";
	static int bulk(mm355_ctx *c, const RecCall &k, const RecTileRun *runs, const int64_t *tile_off)
	{
		if (k.n_tiles > 0) {
			hipLaunchKernelGGL(k_bam_bulk, dim3((unsigned)k.n_tiles), dim3(256), 0, c->st, runs, tile_off, k.n_lines, (char*)c->rec_text.p);
			HIPCHK(hipGetLastError());
		}
		return 0;
	}
	static int finish(mm355_ctx *c, RecCall &k, const int64_t *d_lo, mm355_text_t **out)
	{
		mm355_text_t *T = mm355_text_alloc(k.n_reads, k.n_lines, bgzf_size(k.n_text));
		if (T == 0) return MM355_ENOMEM;
		double k_us = 0;
		hipError_t e = hipMemcpyAsync(T->line_off, d_lo, (size_t)(k.n_reads + 1) * 8, hipMemcpyDeviceToHost, c->st);
		int rc = e == hipSuccess? bam_frame_device(c, k.n_text, T->text, k.times, &k_us) : MM355_EHIP;
		if (rc) { fprintf(stderr, "[mm355] error %d in the BAM writer (%s)\n", rc, hipGetErrorString(e)); mm355_free_text_host(T); return rc; }
		if (k.times)
			fprintf(stderr, "[mm355] bam_times records %lld stream_bytes %lld blocks %lld tiles %lld pack_ms %.3f k_bgzf_frame_us %.1f total_ms %.3f\n", (long long)k.n_lines,
			        (long long)k.n_text, (long long)bgzf_blocks(k.n_text), (long long)k.n_tiles, k.t_packed - k.t_begin, k_us, mm355_now_ms() - k.t_begin);
		*out = T;
		return 0;
	}
};

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
	const PafNames nm = { c->mi->names.data(), c->mi->n_seq };
	return rec_format_where(where, H->n_hits, "MM355_BAM_MIN_HITS", MM355_BAM_MIN_HITS_DEFAULT,
	                        [&] { return mm355_bam_format_host(H, qnames, seqs, qlens, quals, rep_len, nm, sam_flags, out); },
	                        [&] { return rec_format_device<BamDevFmt>(c, H, qnames, seqs, qlens, quals, rep_len, sam_flags, true, out); }, out);
}

extern "C" int mm355_map_batch_bam(mm355_ctx_t *c, const mm355_mapopt_t *mo, int64_t n_reads, const char *const *seqs, const int32_t *lens,
                                   const char *const *names, const char *const *quals, int flags, int sam_flags, int where, mm355_text_t **out)
{
	return rec_map_batch(mm355_bam_format, c, mo, n_reads, seqs, lens, names, quals, flags, sam_flags, where, out);
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
		if (c->rec_text.ensure((size_t)n + 64)) return MM355_ENOMEM;
		mm355_text_t *T = mm355_text_alloc(0, bgzf_blocks(n), bgzf_size(n));
		if (T == 0) return MM355_ENOMEM;
		T->line_off[0] = 0;
		double k_us = 0;
		hipError_t e = n? hipMemcpyAsync(c->rec_text.p, data, (size_t)n, hipMemcpyHostToDevice, c->st) : hipSuccess;
		const int rc = e == hipSuccess? bam_frame_device(c, n, T->text, false, &k_us) : MM355_EHIP;
		if (rc) { mm355_free_text_host(T); return rc; }
		*out = T;
	}
	(*out)->on_device = where == MM355_PAF_DEVICE;
	(*out)->ms_format = mm355_now_ms() - t0;
	return 0;
}
