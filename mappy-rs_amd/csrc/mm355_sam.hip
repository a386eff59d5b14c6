// mm355_sam.hip -- the SAM text of a batch result, written on the device.  The line is stated once, in mm355_sam.h (sam_emit_line); the
// device record writer of mm355_recdev.h runs it, a wave per line.  What is SAM's own: the CIGAR is text; the SA tag with its contig names
// goes out byte by byte; SEQ and QUAL, the bulk of the text, are noted down as runs (mode bit 0: last byte first, bit 1: complemented) and
// copied by
//   k_sam_copy    work item = (line, field, tile of SAM_TILE output bytes), one block each.  A thread owns an aligned 16-byte piece of the
//                 destination: the interior is one 16-byte store, made of five aligned source dwords shifted into place (reversed:
//                 byte-swapped dwords in mirrored order), complemented through the 256-entry table in LDS; the ragged head and tail of the
//                 tile are byte stores.
#include "mm355_recdev.h"

#define SAM_TILE 4096         // output bytes of one k_sam_copy block: 256 threads x 16 bytes

MM_HD int64_t sam_tiles(int64_t n) { return (n + SAM_TILE - 1) / SAM_TILE; }
MM_HD int64_t sam_run_tiles(const RecTileRun &r) { return sam_tiles(r.len); }

__global__ __launch_bounds__(256) void k_sam_copy(const RecTileRun *copy, const int64_t *tile_off, int64_t n_lines, char *text)
{
	__shared__ unsigned char comp[256];
	comp[threadIdx.x] = sam_comp((unsigned char)threadIdx.x);
	int64_t t;
	const RecTileRun r = rec_tile_run<SamFmt::TILE_RUNS>(copy, tile_off, n_lines, blockIdx.x, sam_run_tiles, &t);
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

// SamFmt as the device writes it
struct SamDevFmt : SamFmt {
	typedef RecDev Dev;
	struct Count : RecCount {
		using RecCount::RecCount;
		__device__ void seq(const char *, int64_t l, bool, bool) { n += l; tiles += sam_tiles(l); }
	};
	struct Write : RecWrite<RUNS> {
		using RecWrite<RUNS>::RecWrite;
		__device__ void seq(const char *b, int64_t l, bool rev, bool comp) { note(b, l, (rev? 1 : 0) | (comp? 2 : 0)); n += l; }
	};
	// MM355_SAM_TIMES=1 (tools/sam_bench.py): one line on stderr with where the call's time went -- k_sam_copy between two events, the host's
	// packing and the copy of the text into the pageable result with the host clock
	static constexpr const char *TIMES_ENV = "MM355_SAM_TIMES";
	static int bulk(mm355_ctx *c, const RecCall &k, const RecTileRun *runs, const int64_t *tile_off)
	{
		if (k.times) (void)hipEventRecord(c->ev0, c->st);
		if (k.n_tiles > 0) {
			hipLaunchKernelGGL(k_sam_copy, dim3((unsigned)k.n_tiles), dim3(256), 0, c->st, runs, tile_off, k.n_lines, (char*)c->rec_text.p);
			HIPCHK(hipGetLastError());
		}
		if (k.times) { (void)hipEventRecord(c->ev1, c->st); HIPCHK(mm355_wait_stream(c->st)); }   // (so that the copy back is timed alone)
		return 0;
	}
	static int finish(mm355_ctx *c, RecCall &k, const int64_t *d_lo, mm355_text_t **out)
	{
		if (int rc = rec_text_back(c, k, d_lo, "SAM", out)) return rc;
		if (k.times) {
			float k_ms = 0; (void)hipEventElapsedTime(&k_ms, c->ev0, c->ev1);
			const double t_end = mm355_now_ms();
			fprintf(stderr, "[mm355] sam_times lines %lld text_bytes %lld tiles %lld pack_ms %.3f k_sam_copy_us %.1f text_copy_ms %.3f total_ms %.3f\n", (long long)k.n_lines,
			        (long long)k.n_text, (long long)k.n_tiles, k.t_packed - k.t_begin, (double)k_ms * 1e3, t_end - k.t_copy, t_end - k.t_begin);
		}
		return 0;
	}
};

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
	const PafNames nm = { c->mi->names.data(), c->mi->n_seq };
	return rec_format_where(where, H->n_hits, "MM355_SAM_MIN_HITS", MM355_SAM_MIN_HITS_DEFAULT,
	                        [&] { return mm355_sam_format_host(H, qnames, seqs, qlens, quals, rep_len, nm, sam_flags, out); },
	                        [&] { return rec_format_device<SamDevFmt>(c, H, qnames, seqs, qlens, quals, rep_len, sam_flags, true, out); }, out);
}

extern "C" int mm355_map_batch_sam(mm355_ctx_t *c, const mm355_mapopt_t *mo, int64_t n_reads, const char *const *seqs, const int32_t *lens,
                                   const char *const *names, const char *const *quals, int flags, int sam_flags, int where, mm355_text_t **out)
{
	return rec_map_batch(mm355_sam_format, c, mo, n_reads, seqs, lens, names, quals, flags, sam_flags, where, out);
}
