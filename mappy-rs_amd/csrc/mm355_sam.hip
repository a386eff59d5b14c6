// mm355_sam.hip -- the SAM text of a batch result, written on the device.  The line is stated once, in mm355_sam.h (sam_emit_line, templated
// on a sink); here the same emitter runs with two device sinks, a wave per LINE -- a line is a row of hits[], or the unmapped record of a read
// without rows; the host lays out line -> read and read -> first line next to the uploads:
//   k_sam_len     the lanes add up the CIGAR text width (wave reduction); lane 0 runs the emitter with the counting sink (SEQ and QUAL widths
//                 are arithmetic) and also counts the line's SEQ / QUAL tiles.  rocPRIM's exclusive scan over the lengths gives every line's
//                 offset and the total, a second one over the tile counts the first tile of every line and the tile total; both totals cross
//                 to the host with the call's one synchronisation and size the text and the copy grid.
//   k_sam_fields  lane 0 runs the emitter with the writing sink: single bytes (the short fields, the SA tag with its contig names) go
//                 straight to the text; qname, rname, cs, MD are noted down and copied by the wave (a full table falls back to lane 0: the
//                 table never decides what is written); the CIGAR is written by the wave in tiles of 64 operations; SEQ and QUAL are only
//                 noted down, in a table of two runs per line.
//   k_sam_copy    the bulk of the text.  Work item = (line, field, tile of SAM_TILE output bytes), one block each, so a 200-kb read is 49
//                 blocks and not one wave.  A thread owns an aligned 16-byte piece of the destination: the interior is one 16-byte store, made
//                 of five aligned source dwords shifted into place (reversed: byte-swapped dwords in mirrored order), complemented through
//                 the 256-entry table in LDS; the ragged head and tail of the tile are byte stores.
// Every byte of the text has one writer: plain vector stores, no atomics.  Uploaded per call: what the PAF writer uploads, plus the reads
// and qualities of the reads that print them (the caller's bytes: the mapping path's resident copy is packed and not guaranteed to be them).
#include <rocprim/device/device_scan.hpp>
#include "mm355_wave.h"
#include "mm355_samdev.h"

#define SAM_TILE 4096         // output bytes of one k_sam_copy block: 256 threads x 16 bytes
#define SAM_RUNS 4            // qname, rname, cs, MD

MM_HD int64_t sam_tiles(int64_t n) { return (n + SAM_TILE - 1) / SAM_TILE; }

// a run the wave copies after lane 0 has laid the line out: len bytes (CIGAR: words) from src to byte `at` of the line
struct SamRun { const void *src; int64_t at, len; };
// a SEQ / QUAL run of a line: len bytes from src (mode bit 0: last byte first, bit 1: complemented) to byte `dst` of the text
struct SamCopyRun { const char *src; int64_t dst; int32_t len, mode; };

struct SamDevCount {
	int64_t n = 0, cg, tiles = 0;
	__device__ void ch(char) { ++n; }
	__device__ void bytes(const char *, int64_t l) { n += l; }
	__device__ void cigar(const uint32_t *, int64_t) { n += cg; }
	__device__ void seq(const char *, int64_t l, bool, bool) { n += l; tiles += sam_tiles(l); }
};
struct SamDevWrite {
	char *p; int64_t n = 0, cg, line_at; SamRun *runs, *cig; SamCopyRun *copy; int n_runs = 0, n_copy = 0;
	__device__ void ch(char c) { p[n++] = c; }
	__device__ void bytes(const char *b, int64_t l)
	{
		if (n_runs < SAM_RUNS) { runs[n_runs++] = SamRun{ b, n, l }; n += l; }
		else for (int64_t i = 0; i < l; ++i) p[n++] = b[i];
	}
	__device__ void cigar(const uint32_t *w, int64_t k) { *cig = SamRun{ w, n, k }; n += cg; }
	__device__ void seq(const char *b, int64_t l, bool rev, bool comp)
	{
		if (n_copy < 2) copy[n_copy++] = SamCopyRun{ b, line_at + n, (int32_t)l, (rev? 1 : 0) | (comp? 2 : 0) };   // (a line has SEQ and QUAL, no third run)
		n += l;
	}
};

__global__ __launch_bounds__(256) void k_sam_len(SamDev D, int64_t *len, int64_t *cglen, int64_t *ntile)
{
	const int lane = threadIdx.x & 63;
	const int64_t l = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
	if (l >= D.n_lines) return;                // (the whole wave)
	const int32_t r = D.l_read[l], row = sam_row_of(D, l, r);
	long long cg = 0;
	if (row >= 0) {
		const mm355_hit_t &h = D.hits[D.hit_off[r] + row];
		const uint32_t *w = D.cigar + h.cigar_off;
		for (int32_t i = lane; i < h.n_cigar; i += 64) cg += paf_cigar_width(w[i]);
		for (int d = 32; d > 0; d >>= 1) cg += __shfl_xor(cg, d);
	}
	if (lane == 0) {
		const SamRead R = sam_read_dev(D, r);
		SamDevCount s; s.cg = cg;
		sam_emit_line(s, SamLine{ &R, row });
		len[l] = s.n; cglen[l] = cg; ntile[l] = s.tiles;
	}
}

__global__ void k_sam_line_off(const int64_t *off, const int64_t *l_first, int64_t n_reads, int64_t *line_off)
{
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i <= n_reads) line_off[i] = off[l_first[i]];
}

__global__ __launch_bounds__(256) void k_sam_fields(SamDev D, const int64_t *off, const int64_t *cglen, char *text, SamCopyRun *copy)
{
	__shared__ SamRun runs[4][SAM_RUNS + 1];   // per wave; the last one is the CIGAR
	__shared__ int n_runs[4];
	const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
	const int64_t l = (int64_t)blockIdx.x * 4 + wv;
	const bool on = l < D.n_lines;
	char *line = on? text + off[l] : text;
	if (on && lane == 0) {
		const int32_t r = D.l_read[l];
		const SamRead R = sam_read_dev(D, r);
		runs[wv][SAM_RUNS] = SamRun{ 0, 0, 0 };
		copy[2 * l] = copy[2 * l + 1] = SamCopyRun{ 0, 0, 0, 0 };
		SamDevWrite s; s.p = line; s.cg = cglen[l]; s.line_at = off[l]; s.runs = runs[wv]; s.cig = &runs[wv][SAM_RUNS]; s.copy = copy + 2 * l;
		sam_emit_line(s, SamLine{ &R, sam_row_of(D, l, r) });
		n_runs[wv] = s.n_runs;
	}
	__syncthreads();
	if (!on) return;
	const int nr = n_runs[wv];
	for (int r = 0; r < nr; ++r) {
		const char *src = (const char*)runs[wv][r].src; char *dst = line + runs[wv][r].at;
		const int64_t n = runs[wv][r].len;
		for (int64_t i = lane; i < n; i += 64) dst[i] = src[i];
	}
	paf_wave_cigar(line + runs[wv][SAM_RUNS].at, (const uint32_t*)runs[wv][SAM_RUNS].src, runs[wv][SAM_RUNS].len, lane);
}

__global__ __launch_bounds__(256) void k_sam_copy(const SamCopyRun *copy, const int64_t *tile_off, int64_t n_lines, char *text)
{
	__shared__ unsigned char comp[256];
	comp[threadIdx.x] = sam_comp((unsigned char)threadIdx.x);
	const int64_t b = blockIdx.x;
	int64_t lo = 0, hi = n_lines;              // the last line whose first tile is <= b (lines without tiles in front of it share that number)
	while (hi - lo > 1) { const int64_t mid = (lo + hi) >> 1; if (tile_off[mid] <= b) lo = mid; else hi = mid; }
	int64_t t = b - tile_off[lo];
	SamCopyRun r = copy[2 * lo];
	if (t >= sam_tiles(r.len)) { t -= sam_tiles(r.len); r = copy[2 * lo + 1]; }
	__syncthreads();
	const int64_t o0 = t * SAM_TILE, o1 = o0 + SAM_TILE < (int64_t)r.len? o0 + SAM_TILE : (int64_t)r.len;   // this tile: bytes [o0, o1) of the run
	if (t < 0 || o0 >= o1) return;
	char *dst = text + r.dst;
	const uintptr_t d0 = (uintptr_t)(dst + o0), d1 = (uintptr_t)(dst + o1);
	for (uintptr_t c = (d0 & ~(uintptr_t)15) + 16 * (uintptr_t)threadIdx.x; c < d1; c += 16 * 256) {
		if (c >= d0 && c + 16 <= d1) {
			const int64_t o = (int64_t)(c - (uintptr_t)dst);
			*(uint4*)c = sam_piece(r.src, (r.mode & 1)? r.len - 16 - o : o, r.mode, comp);
		} else {
			const uintptr_t e = c + 16 < d1? c + 16 : d1;
			for (uintptr_t a = c > d0? c : d0; a < e; ++a) {
				const int64_t o = (int64_t)(a - (uintptr_t)dst);
				const unsigned char x = (unsigned char)r.src[(r.mode & 1)? r.len - 1 - o : o];
				*(char*)a = (char)((r.mode & 2)? comp[x] : x);
			}
		}
	}
}

// ------------------------------------------------------------------ host side

static int sam_format_device(mm355_ctx *c, const mm355_hits_t *H, const char *const *qnames, const char *const *seqs, const int32_t *qlens,
                             const char *const *quals, const int32_t *rep_len, int sam_flags, mm355_text_t **out)
{
	const int64_t nr = H->n_reads;
	// MM355_SAM_TIMES=1 (read per call; tools/sam_bench.py): one line on stderr with where the call's time went -- k_sam_copy between two events,
	// the host's packing and the copy of the text into the pageable result with the host clock
	const char *te = getenv("MM355_SAM_TIMES"); const bool times = te && *te && *te != '0';
	const double t_begin = mm355_now_ms();
	SamDev D; double t_packed;
	if (int rc = sam_upload(c, H, qnames, seqs, qlens, quals, rep_len, sam_flags, &D, &t_packed)) return rc;
	const int64_t nl = D.n_lines;
	if (nl == 0) return sam_text_empty(nr, out);   // nothing to launch
	hipStream_t st = c->st;
	// lengths and tile counts (one word more each: the scans leave the totals there), their offsets, CIGAR text lengths, line_off, the runs, scan space
	size_t tb = 0;
	(void)rocprim::exclusive_scan(nullptr, tb, (int64_t*)0, (int64_t*)0, (int64_t)0, (size_t)nl + 1, rocprim::plus<int64_t>(), st);
	const size_t w1 = up256((size_t)(nl + 1) * 8);
	const size_t w_len = 0, w_off = w_len + w1, w_nt = w_off + w1, w_to = w_nt + w1, w_cg = w_to + w1, w_lo = w_cg + w1, w_run = w_lo + up256((size_t)(nr + 1) * 8),
	             w_tmp = w_run + up256((size_t)nl * 2 * sizeof(SamCopyRun));
	if (c->sam_work.ensure(w_tmp + tb + 256)) return MM355_ENOMEM;
	char *dw = (char*)c->sam_work.p;
	int64_t *d_len = (int64_t*)(dw + w_len), *d_off = (int64_t*)(dw + w_off), *d_nt = (int64_t*)(dw + w_nt), *d_to = (int64_t*)(dw + w_to),
	        *d_cg = (int64_t*)(dw + w_cg), *d_lo = (int64_t*)(dw + w_lo);
	SamCopyRun *d_run = (SamCopyRun*)(dw + w_run);
	HIPCHK(hipMemsetAsync(d_len + nl, 0, 8, st));
	HIPCHK(hipMemsetAsync(d_nt + nl, 0, 8, st));
	const unsigned grid = (unsigned)((nl + 3) / 4);
	hipLaunchKernelGGL(k_sam_len, dim3(grid), dim3(256), 0, st, D, d_len, d_cg, d_nt);
	HIPCHK(hipGetLastError());
	HIPCHK(rocprim::exclusive_scan(dw + w_tmp, tb, d_len, d_off, (int64_t)0, (size_t)nl + 1, rocprim::plus<int64_t>(), st));
	HIPCHK(rocprim::exclusive_scan(dw + w_tmp, tb, d_nt, d_to, (int64_t)0, (size_t)nl + 1, rocprim::plus<int64_t>(), st));
	hipLaunchKernelGGL(k_sam_line_off, dim3((unsigned)((nr + 1 + 255) / 256)), dim3(256), 0, st, d_off, D.l_first, nr, d_lo);
	HIPCHK(hipGetLastError());
	int64_t *h_tot = (int64_t*)c->h_sam_out.p;
	HIPCHK(hipMemcpyAsync(h_tot, d_off + nl, 8, hipMemcpyDeviceToHost, st));
	HIPCHK(hipMemcpyAsync(h_tot + 1, d_to + nl, 8, hipMemcpyDeviceToHost, st));
	HIPCHK(mm355_wait_stream(st));
	const int64_t tot = h_tot[0], n_tiles = h_tot[1];
	// (every line has its newline at least, and a tile holds at least one byte of the text)
	if (tot < nl || n_tiles < 0 || n_tiles > tot || n_tiles > (int64_t)INT32_MAX) return MM355_EHIP;
	if (c->sam_text.ensure((size_t)tot + 64)) return MM355_ENOMEM;
	hipLaunchKernelGGL(k_sam_fields, dim3(grid), dim3(256), 0, st, D, d_off, d_cg, (char*)c->sam_text.p, d_run);
	HIPCHK(hipGetLastError());
	if (times) (void)hipEventRecord(c->ev0, st);
	if (n_tiles > 0) {
		hipLaunchKernelGGL(k_sam_copy, dim3((unsigned)n_tiles), dim3(256), 0, st, d_run, d_to, nl, (char*)c->sam_text.p);
		HIPCHK(hipGetLastError());
	}
	if (times) { (void)hipEventRecord(c->ev1, st); HIPCHK(mm355_wait_stream(st)); }   // (so that the copy below is timed alone)
	mm355_text_t *T = mm355_text_alloc(nr, nl, tot);
	if (T == 0) return MM355_ENOMEM;
	const double t_copy = mm355_now_ms();
	hipError_t e = hipMemcpyAsync(T->text, c->sam_text.p, (size_t)tot, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess) e = hipMemcpyAsync(T->line_off, d_lo, (size_t)(nr + 1) * 8, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess) e = mm355_wait_stream(st);
	if (e != hipSuccess) { fprintf(stderr, "[mm355] HIP error %s in the SAM writer\n", hipGetErrorString(e)); mm355_free_text_host(T); return MM355_EHIP; }
	if (times) {
		float k_ms = 0; (void)hipEventElapsedTime(&k_ms, c->ev0, c->ev1);
		const double t_end = mm355_now_ms();
		fprintf(stderr, "[mm355] sam_times lines %lld text_bytes %lld tiles %lld pack_ms %.3f k_sam_copy_us %.1f text_copy_ms %.3f total_ms %.3f\n", (long long)nl, (long long)tot,
		        (long long)n_tiles, t_packed - t_begin, (double)k_ms * 1e3, t_end - t_copy, t_end - t_begin);
	}
	*out = T;
	return 0;
}

// MM355_PAF_AUTO for SAM: the device formatter from this many hits on.  Measured with tools/sam_bench.py (profiles/sam_file.json, format_sweep:
// ms_format of the two formatters on the hits of 16 .. 9216 reads, map-ont with cs, reads of N50 8 kb with qualities): the host is ahead at 32
// hits (0.21 against 0.24 ms), the device at 48 (0.26 against 0.33 ms) and from there on, 6.5 times at 9234 (17.5 against 113.6 ms).  A SAM line
// carries the read, so the device pays off earlier than for PAF.  MM355_SAM_MIN_HITS=<n> overrides (read per call: the tests switch it).
#define MM355_SAM_MIN_HITS_DEFAULT 48

extern "C" int mm355_sam_format(mm355_ctx_t *c, const mm355_mapopt_t *mo, const mm355_hits_t *H, const char *const *qnames, const char *const *seqs,
                                const int32_t *qlens, const char *const *quals, const int32_t *rep_len, int sam_flags, int where, mm355_text_t **out)
{
	if (out == 0) return MM355_EINVAL;
	*out = 0;
	if (c == 0 || mo == 0 || H == 0 || where < MM355_PAF_AUTO || where > MM355_PAF_DEVICE) return MM355_EINVAL;
	if (c->mi == 0) return MM355_ENOIDX;
	if (int rc = mm355_sam_check(H, c->mi->n_seq, (mo->flag & MMF_CIGAR) != 0, seqs, qlens, rep_len, sam_flags)) return rc;
	const double t0 = mm355_now_ms();
	if (where == MM355_PAF_AUTO) {
		const char *e = getenv("MM355_SAM_MIN_HITS");
		const int64_t min_hits = e && *e? atoll(e) : MM355_SAM_MIN_HITS_DEFAULT;
		where = H->n_hits >= min_hits? MM355_PAF_DEVICE : MM355_PAF_HOST;
	}
	const PafNames nm = { c->mi->names.data(), c->mi->n_seq };
	const int rc = where == MM355_PAF_DEVICE? sam_format_device(c, H, qnames, seqs, qlens, quals, rep_len, sam_flags, out)
	                                        : mm355_sam_format_host(H, qnames, seqs, qlens, quals, rep_len, nm, sam_flags, out);
	if (rc) return rc;
	(*out)->on_device = where == MM355_PAF_DEVICE;
	(*out)->ms_format = mm355_now_ms() - t0;
	return 0;
}

extern "C" int mm355_map_batch_sam(mm355_ctx_t *c, const mm355_mapopt_t *mo, int64_t n_reads, const char *const *seqs, const int32_t *lens,
                                   const char *const *names, const char *const *quals, int flags, int sam_flags, int where, mm355_text_t **out)
{
	if (out == 0) return MM355_EINVAL;
	*out = 0;
	if (mo && !(mo->flag & MMF_CIGAR)) return MM355_EINVAL;    // (before anything is mapped)
	mm355_hits_t *H = 0; const int32_t *rep_len = 0;
	int rc = mm355_map_batch_rl(c, mo, n_reads, seqs, lens, names, flags | MM355_OUT_TAGS, &H, &rep_len);
	if (rc) return rc;
	rc = mm355_sam_format(c, mo, H, names, seqs, lens, quals, rep_len, sam_flags, where, out);
	mm355_free_hits(H);
	return rc;
}
