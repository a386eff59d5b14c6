// mm355_recdev.h -- the device record writer behind the PAF, SAM and BAM formatters (mm355_paf.hip, mm355_sam.hip, mm355_bam.hip).  A record
// is a PAF line, a SAM line or a BAM record: a row of hits[], or (SAM, BAM) the unmapped record of a read without rows.  Each format
// states its record once, as an emitter templated on a sink (mm355_paf.h, mm355_sam.h, mm355_bam.h), and describes itself in a traits
// struct (PafFmt, SamFmt, BamFmt: compile-time facts only); its .hip file adds the device half -- the two device sinks, the bulk kernel
// and the last step -- and everything here is instantiated with that.  The same emitter runs with both sinks, a wave per record, so
// the length pass and the write pass cannot disagree:
//   upload        the hit and tags rows, the CIGAR words and the string arena (a result of mm355_map_batch lives on the host), the read
//                 lengths, and what the host lays out: record -> read, read -> first record, the query names cut at their first blank and
//                 (formats that print them) the reads and qualities -- the caller's bytes: the mapping path's resident copy is packed and
//                 not guaranteed to be them.  The contig names are uploaded once per index replica, on first use, and belong to the replica.
//   k_rec_len     the lanes stride over the row's CIGAR words and add up the format's term (wave reduction): the width of the CIGAR text,
//                 or the reference length BAM's bin needs.  Lane 0 runs the emitter with the counting sink, which takes that sum, and
//                 counts the record's SEQ / QUAL tiles where the format has them.
//   scan          rocPRIM's exclusive scan over the lengths: the offset of every record, the total behind the last; with tiles a second
//                 one over the tile counts: the first tile of every record and the tile total.  line_off[read] is a gather through the
//                 read's first record.  The totals cross to the host with the call's one synchronisation before the write and size the
//                 text buffer and the bulk grid.
//   k_rec_fields  lane 0 runs the emitter with the writing sink: single bytes go straight to the text; runs that exist in memory already
//                 (names, cs, MD, BAM's CIGAR words) are noted down with their place in the record and copied by the whole wave,
//                 lane-strided (a full table falls back to lane 0: the table never decides what is written); the text formats' CIGAR is
//                 written by the wave in tiles of 64 operations; SEQ and QUAL (BAM: and the copied aux tags) are only noted down, in a
//                 table of F::TILE_RUNS runs per record.
//   bulk          the format's own kernel over that table (k_sam_copy, k_bam_bulk): work item = (record, field, tile of output bytes), one
//                 block each, so a 200-kb read is 49 blocks and not one wave.
//   last step     the text formats copy the text back; BAM frames the stream first (k_bgzf_frame).
// Every byte of the text has one writer: plain vector stores, no atomics.  Device code: included by the three .hip files only.
#pragma once
#include <stdio.h>
#include <algorithm>
#include <type_traits>
#include <rocprim/device/device_scan.hpp>
#include "mm355_pipeline.h"
#include "mm355_wave.h"
#include "mm355_sam.h"
#include "mm355_bamsort.h"

// the batch result, the tables and the reads as the kernels see them
struct RecDev {
	const mm355_hit_t *hits; const mm355_tags_t *tags; const uint32_t *cigar; const char *str;
	const int64_t *hit_off; const int32_t *qlen, *rep_len;            // per read (rep_len, seq_off, qual_off, bytes: null where records carry no read)
	const int64_t *qn_off; const char *qn;                            // per read: its name = qn[qn_off[r] .. qn_off[r + 1])
	const int64_t *seq_off, *qual_off; const char *bytes;             // per read: its bases and quality in bytes[]; qual_off < 0: none
	const char *tn; const int64_t *tn_off;                            // contig names
	const int32_t *l_read; const int64_t *l_first;                    // read of a record; first record of a read (n_reads + 1)
	int64_t n_lines; int sam_flags, has_cigar;
};

// the same with the copied aux tags of a call that has some (BamAuxDevFmt): a format's kernels take F::Dev, so only that format's argument grows
struct RecDevAux : RecDev {
	const int64_t *aux_off; const int32_t *aux_len, *aux_mod;         // per read: its tags in bytes[]
};

__device__ __forceinline__ int32_t rec_row_of(const RecDev &D, int64_t l, int32_t r) { return D.hit_off[r + 1] > D.hit_off[r]? (int32_t)(l - D.l_first[r]) : -1; }

// what record l (of read r, its row `row`) is made from, as the format's emitter takes it.  A PAF line is a row: l counts hits[].
__device__ __forceinline__ void rec_line_dev(const RecDev &D, int64_t l, int32_t r, int32_t, SamRead &, PafLine &L)
{
	L.h = D.hits + l; L.t = D.tags + l;
	const int32_t rid = L.h->rid;
	L.qname = D.qn + D.qn_off[r]; L.qname_len = D.qn_off[r + 1] - D.qn_off[r]; L.qlen = D.qlen[r];
	L.tname = D.tn + D.tn_off[rid]; L.tname_len = D.tn_off[rid + 1] - D.tn_off[rid];
	L.cigar = D.cigar; L.str = D.str; L.has_cigar = D.has_cigar != 0;
}
__device__ __forceinline__ void rec_line_dev(const RecDev &D, int64_t, int32_t r, int32_t row, SamRead &R, SamLine &L)
{
	const int64_t k0 = D.hit_off[r];
	R.rows = D.hits + k0; R.tags = D.tags + k0; R.n_rows = (int32_t)(D.hit_off[r + 1] - k0);
	R.qname = D.qn + D.qn_off[r]; R.qname_len = D.qn_off[r + 1] - D.qn_off[r]; R.qlen = D.qlen[r];
	R.seq = D.bytes + D.seq_off[r]; R.qual = D.qual_off[r] >= 0? D.bytes + D.qual_off[r] : 0;
	R.tn = D.tn; R.tn_off = D.tn_off; R.cigar = D.cigar; R.str = D.str;
	R.rep_len = D.rep_len[r]; R.sam_flags = D.sam_flags;
	R.aux = 0; R.aux_len = R.aux_mod = 0;
	L.R = &R; L.row = row;
}
__device__ __forceinline__ void rec_line_dev(const RecDevAux &D, int64_t l, int32_t r, int32_t row, SamRead &R, SamLine &L)
{
	rec_line_dev((const RecDev&)D, l, r, row, R, L);
	R.aux = (const uint8_t*)D.bytes + D.aux_off[r]; R.aux_len = D.aux_len[r]; R.aux_mod = D.aux_mod[r];
}

// a run the wave copies after lane 0 has laid the record out: len bytes (the text formats' CIGAR: words) from src to byte `at` of the record
struct RecRun { const void *src; int64_t at, len; };
// a SEQ / QUAL / aux run of a record, which the format's bulk kernel writes in tiles: len bytes or bases from src to byte `dst` of the text; mode
// is the bulk kernel's to read
struct RecTileRun { const char *src; int64_t dst; int32_t len, mode; };

// ---- the device sinks of a wave's lane 0: what every format's have.  aux is the wave's sum over the CIGAR words.
struct RecCount {
	int64_t n = 0, aux, tiles = 0;
	__device__ explicit RecCount(int64_t aux_) : aux(aux_) {}
	__device__ void ch(char) { ++n; }
	__device__ void bytes(const char *, int64_t l) { n += l; }
	__device__ void cigar(const uint32_t *, int64_t) { n += aux; }            // (text: the wave has added up the widths)
};
// RUNS entries of runs[] are the table; a text format has one more behind them, for the CIGAR.  at0: where the record begins in the text.
// TILE_RUNS entries of tile[] are the record's bulk runs
template <int RUNS, int TILE_RUNS = 2> struct RecWrite {
	char *p; int64_t n = 0, aux, at0; RecRun *runs; RecTileRun *tile; int n_runs = 0, n_tile = 0;
	__device__ RecWrite(char *p_, int64_t aux_, int64_t at0_, RecRun *runs_, RecTileRun *tile_) : p(p_), aux(aux_), at0(at0_), runs(runs_), tile(tile_) {}
	__device__ void ch(char c) { p[n++] = c; }
	__device__ void bytes(const char *b, int64_t l)
	{
		if (n_runs < RUNS) { runs[n_runs++] = RecRun{ b, n, l }; n += l; }
		else for (int64_t i = 0; i < l; ++i) p[n++] = b[i];
	}
	__device__ void cigar(const uint32_t *w, int64_t k) { runs[RUNS] = RecRun{ w, n, k }; n += aux; }   // (text: the wave writes it)
	__device__ void note(const char *b, int64_t l, int mode) { if (n_tile < TILE_RUNS) tile[n_tile++] = RecTileRun{ b, at0 + n, (int32_t)l, mode }; }   // (a record has no more bulk runs than its format says)
};

// the text of nc CIGAR words, written by a whole wave in tiles of 64 operations: a prefix sum of the operations' widths, every lane its own
// digits and letter, the running offset carried from tile to tile (uniform trip count: the scan needs every lane)
__device__ __forceinline__ void rec_wave_cigar(char *dst, const uint32_t *w, int64_t nc, int lane)
{
	for (int64_t base = 0; base < nc; base += 64) {
		const bool have = base + lane < nc;
		const uint32_t x = have? w[base + lane] : 0u;
		const int32_t wid = have? paf_cigar_width(x) : 0;
		const int32_t incl = wave_incl_scan_add(wid);
		if (have) {
			char *q = dst + (incl - wid);
			uint32_t v = x >> 4;
			for (int i = wid - 2; i >= 0; --i) { q[i] = (char)('0' + v % 10); v /= 10; }
			q[wid - 1] = paf_cigar_op(x);
		}
		dst += __builtin_amdgcn_readlane(incl, 63);
	}
}

// ---- the kernels of the shared stages: a wave per record, four records per block
template <typename F> __global__ __launch_bounds__(256) void k_rec_len(typename F::Dev D, int64_t *len, int64_t *aux, int64_t *ntile)
{
	const int lane = threadIdx.x & 63;
	const int64_t l = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
	if (l >= D.n_lines) return;                // (the whole wave)
	const int32_t r = D.l_read[l], row = rec_row_of(D, l, r);
	long long sum = 0;
	if (row >= 0 && D.has_cigar) {
		const mm355_hit_t &h = D.hits[D.hit_off[r] + row];
		const uint32_t *w = D.cigar + h.cigar_off;
		for (int32_t i = lane; i < h.n_cigar; i += 64) sum += F::word_term(w[i]);
		for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d);
	}
	if (lane == 0) {
		SamRead R; typename F::Line L;
		rec_line_dev(D, l, r, row, R, L);
		typename F::Count s(sum);
		F::emit(s, L, sum, 0);
		len[l] = s.n; aux[l] = sum;
		if constexpr (F::TILED) ntile[l] = s.tiles;
	}
}

static __global__ void k_rec_line_off(const int64_t *off, const int64_t *l_first, int64_t n_reads, int64_t *line_off)
{
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i <= n_reads) line_off[i] = off[l_first[i]];
}

template <typename F> __global__ __launch_bounds__(256) void k_rec_fields(typename F::Dev D, const int64_t *off, const int64_t *aux, char *text, RecTileRun *tile)
{
	__shared__ RecRun runs[4][F::RUNS + (F::WAVE_CIGAR? 1 : 0)];   // per wave; a text format's last one is the CIGAR
	__shared__ int n_runs[4];
	const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
	const int64_t l = (int64_t)blockIdx.x * 4 + wv;
	const bool on = l < D.n_lines;
	char *rec = on? text + off[l] : text;
	if (on && lane == 0) {
		const int32_t r = D.l_read[l];
		SamRead R; typename F::Line L;
		rec_line_dev(D, l, r, rec_row_of(D, l, r), R, L);
		if constexpr (F::WAVE_CIGAR) runs[wv][F::RUNS] = RecRun{ 0, 0, 0 };
		RecTileRun *mine = 0;
		if constexpr (F::TILED) {
			mine = tile + F::TILE_RUNS * l;
			for (int k = 0; k < F::TILE_RUNS; ++k) mine[k] = RecTileRun{ 0, 0, 0, 0 };
		}
		typename F::Write s(rec, aux[l], off[l], runs[wv], mine);
		F::emit(s, L, aux[l], (uint32_t)(off[l + 1] - off[l] - 4));
		n_runs[wv] = s.n_runs;
	}
	__syncthreads();
	if (!on) return;
	const int nr = n_runs[wv];
	for (int r = 0; r < nr; ++r) {
		const char *src = (const char*)runs[wv][r].src; char *dst = rec + runs[wv][r].at;
		const int64_t n = runs[wv][r].len;
		for (int64_t i = lane; i < n; i += 64) dst[i] = src[i];
	}
	if constexpr (F::WAVE_CIGAR) rec_wave_cigar(rec + runs[wv][F::RUNS].at, (const uint32_t*)runs[wv][F::RUNS].src, runs[wv][F::RUNS].len, lane);
}

// the head of a bulk kernel: the run that block b of the tile grid works on and, in *t, which of the run's tiles it has.  tiles(run): how
// many tiles the format cuts a run into; NR: the runs of a record (F::TILE_RUNS)
template <int NR, typename Tiles> __device__ __forceinline__ RecTileRun rec_tile_run(const RecTileRun *runs, const int64_t *tile_off, int64_t n_lines, int64_t b, Tiles tiles, int64_t *t)
{
	int64_t lo = 0, hi = n_lines;              // the last record whose first tile is <= b (records without tiles in front of it share that number)
	while (hi - lo > 1) { const int64_t mid = (lo + hi) >> 1; if (tile_off[mid] <= b) lo = mid; else hi = mid; }
	*t = b - tile_off[lo];
	RecTileRun r = runs[NR * lo];
	for (int k = 1; k < NR && *t >= tiles(r); ++k) { *t -= tiles(r); r = runs[NR * lo + k]; }
	return r;
}

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

// Lays out what the host makes (the records, the query names as the record prints them, where every read's bases and quality go), uploads it
// with the batch result into c->rec_in and fills D.  D->n_lines == 0 on return: nothing was uploaded, there is nothing to launch.
// A format without SEQ and QUAL carries no read bytes: seqs, quals and rep_len are not read, and D's pointers to them are null.
// *t_packed: the host clock when the packing was done (MM355_SAM_TIMES).
template <typename F> static int rec_upload(mm355_ctx *c, const mm355_hits_t *H, const char *const *qnames, const char *const *seqs, const int32_t *qlens,
                                            const char *const *quals, const int32_t *rep_len, const RecAux &ax, int sam_flags, bool has_cigar, typename F::Dev *Dp, double *t_packed)
{
	typename F::Dev &D = *Dp;
	const int64_t nh = H->n_hits, nr = H->n_reads;
	std::vector<int64_t> n_line((size_t)nr), qn_len((size_t)nr);
	int64_t nl = 0, qn_tot = 0, by_tot = 0;
	const bool with_aux = std::is_same<typename F::Dev, RecDevAux>::value && ax.aux != 0;   // (the caller picks that format for a call with tags)
	for (int64_t i = 0; i < nr; ++i) {
		n_line[i] = F::n_lines(H, qlens, sam_flags, i);
		nl += n_line[i];
		qn_len[i] = n_line[i] == 0? 0 : qnames && qnames[i]? paf_qname_len(qnames[i]) : 1;   // (a read without records prints nothing)
		qn_tot += qn_len[i];
		if constexpr (F::TILED) if (n_line[i]) by_tot += (int64_t)qlens[i] * (quals && quals[i]? 2 : 1) + (with_aux && ax.aux[i] && ax.len[i] > 0? ax.len[i] : 0);
	}
	D.n_lines = nl; D.sam_flags = sam_flags; D.has_cigar = has_cigar;
	*t_packed = mm355_now_ms();
	if (nl == 0) return 0;
	if (nl > F::MAX_LINES || nr > (int64_t)INT32_MAX) return MM355_EINVAL;
	HIPCHK(hipSetDevice(c->dev));
	const char *d_tn = 0; const int64_t *d_tn_off = 0;
	if (int rc = mm355_replica_tnames(c->mi, c->dev, &d_tn, &d_tn_off)) return rc;
	// (a chain-only batch has no CIGAR words and no strings: H->cigar and H->str are not touched)
	const size_t nc = has_cigar && H->n_cigar > 0? (size_t)H->n_cigar : 0, ns = has_cigar && H->n_str > 0? (size_t)H->n_str : 0;
	const size_t per_read4 = F::TILED? up256((size_t)nr * 4) : 0, per_read8 = F::TILED? up256((size_t)nr * 8) : 0;   // rep_len; seq_off, qual_off
	const size_t aux4 = with_aux? per_read4 : 0, aux8 = with_aux? per_read8 : 0;                                     // aux_len, aux_mod; aux_off: only a call with aux has them
	// one device buffer; one pinned staging buffer for the parts made here (the tables, the names, the reads and qualities back to back)
	const size_t o_hits = 0, o_tags = o_hits + up256((size_t)nh * sizeof(mm355_hit_t) + 8), o_cig = o_tags + up256((size_t)nh * sizeof(mm355_tags_t) + 8),
	             o_str = o_cig + up256(nc * 4 + 4), o_qlen = o_str + up256(ns + 4), o_hoff = o_qlen + up256((size_t)nr * 4), o_made = o_hoff + up256((size_t)(nr + 1) * 8);
	const size_t m_lread = 0, m_lfirst = m_lread + up256((size_t)nl * 4), m_rep = m_lfirst + up256((size_t)(nr + 1) * 8), m_qoff = m_rep + per_read4,
	             m_soff = m_qoff + up256((size_t)(nr + 1) * 8), m_uoff = m_soff + per_read8, m_aoff = m_uoff + per_read8, m_alen = m_aoff + aux8, m_amod = m_alen + aux4, m_qn = m_amod + aux4,
	             m_by = m_qn + up256((size_t)qn_tot + 4), m_end = m_by + up256((size_t)by_tot + 64);   // (64: the copy kernels read whole dwords around a span)
	if (c->rec_in.ensure(o_made + m_end) || c->h_rec_in.ensure(m_end) || c->h_rec_out.ensure(64, 1 << 20)) return MM355_ENOMEM;
	char *hm = (char*)c->h_rec_in.p, *din = (char*)c->rec_in.p;
	int32_t *l_read = (int32_t*)(hm + m_lread), *rl = (int32_t*)(hm + m_rep);
	int64_t *l_first = (int64_t*)(hm + m_lfirst), *qoff = (int64_t*)(hm + m_qoff), *soff = (int64_t*)(hm + m_soff), *uoff = (int64_t*)(hm + m_uoff);
	int64_t *aoff = (int64_t*)(hm + m_aoff); int32_t *alen = (int32_t*)(hm + m_alen), *amod = (int32_t*)(hm + m_amod);
	char *qn = hm + m_qn, *by = hm + m_by;
	int64_t at = 0, bat = 0, lat = 0;
	for (int64_t i = 0; i < nr; ++i) {
		l_first[i] = lat;
		for (int64_t j = 0; j < n_line[i]; ++j) l_read[lat++] = (int32_t)i;
		qoff[i] = at;
		if (qn_len[i] > 0) memcpy(qn + at, qnames && qnames[i]? qnames[i] : "*", (size_t)qn_len[i]);
		at += qn_len[i];
		if constexpr (F::TILED) {
			rl[i] = rep_len && H->hit_off[i + 1] == H->hit_off[i]? rep_len[i] : 0;
			soff[i] = 0; uoff[i] = -1;
			if (n_line[i]) {
				soff[i] = bat; memcpy(by + bat, seqs[i], (size_t)qlens[i]); bat += qlens[i];
				if (quals && quals[i]) { uoff[i] = bat; memcpy(by + bat, quals[i], (size_t)qlens[i]); bat += qlens[i]; }
			}
			if (aux8) {
				const bool has = n_line[i] && ax.aux[i] && ax.len[i] > 0;
				aoff[i] = bat; alen[i] = has? ax.len[i] : 0; amod[i] = has? ax.mod[i] : 0;
				if (has) { memcpy(by + bat, ax.aux[i], (size_t)ax.len[i]); bat += ax.len[i]; }
			}
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
	const char *made = din + o_made;
	D.hits = (const mm355_hit_t*)(din + o_hits); D.tags = (const mm355_tags_t*)(din + o_tags); D.cigar = (const uint32_t*)(din + o_cig); D.str = din + o_str;
	D.hit_off = (const int64_t*)(din + o_hoff); D.qlen = (const int32_t*)(din + o_qlen); D.rep_len = F::TILED? (const int32_t*)(made + m_rep) : 0;
	D.qn_off = (const int64_t*)(made + m_qoff); D.qn = made + m_qn;
	D.seq_off = F::TILED? (const int64_t*)(made + m_soff) : 0; D.qual_off = F::TILED? (const int64_t*)(made + m_uoff) : 0; D.bytes = F::TILED? made + m_by : 0;
	if constexpr (std::is_same<typename F::Dev, RecDevAux>::value) {
		if (!with_aux) return MM355_EINVAL;
		D.aux_off = (const int64_t*)(made + m_aoff); D.aux_len = (const int32_t*)(made + m_alen); D.aux_mod = (const int32_t*)(made + m_amod);
	}
	D.tn = d_tn; D.tn_off = d_tn_off;
	D.l_read = (const int32_t*)(made + m_lread); D.l_first = (const int64_t*)(made + m_lfirst);
	return 0;
}

// the result of a call that writes nothing
static int rec_text_empty(int64_t nr, mm355_text_t **out)
{
	mm355_text_t *T = mm355_text_alloc(nr, 0, 0);
	if (T == 0) return MM355_ENOMEM;
	for (int64_t i = 0; i <= nr; ++i) T->line_off[i] = 0;
	*out = T;
	return 0;
}

// what a call's format-specific steps are told: the records, the bytes of the unframed text in c->rec_text, the tiles, the host clock at the
// call's begin and after the packing; times: the format's *_TIMES variable is set
// last: what the caller asks of the format's last step (BAM: the deflate level of the blocks; a sorted call: whether the run carries spans, and
// whether it is packed).  Run-time values: the kernels and the steps before the last one do not depend on them
struct RecLast { int level = 0; bool span = false, packed = false; };
struct RecCall { int64_t n_reads, n_lines, n_text, n_tiles; double t_begin, t_packed, t_copy; bool times; hipEvent_t bulk_ev[2] = { 0, 0 }; const int64_t *d_off = 0; RecLast last; };   // bulk_ev: a format's own, around its bulk kernel; d_off: the n_lines + 1 record offsets on the device

// the result of a sorted call that writes nothing (mm355_bam.hip: BamRunFmtOf)
static int rec_text_empty(int64_t, mm355_run_t **out)
{
	*out = mm355_run_alloc(0, 0);
	return *out? 0 : MM355_ENOMEM;
}

// the format whose kernels a format launches: its own, unless it only replaces the last step of another (typedef ... Kern)
template <typename F, typename = void> struct rec_kern { typedef F type; };
template <typename F> struct rec_kern<F, std::void_t<typename F::Kern>> { typedef typename F::Kern type; };

// The driver.  F is the format's device half: its traits struct plus Count and Write (the device sinks), TIMES_ENV (the variable that
// asks for a line of timings on stderr, or null), bulk() (with tiles: launches the bulk kernel on the run table) and finish() (the last
// step: the result record from the text in c->rec_text and line_off[] on the device).
// Out: the result record F::finish makes (mm355_text_t; mm355_run_t for a sorted BAM call); last: handed to F::finish in the RecCall
template <typename F, typename Out> static int rec_format_device_to(mm355_ctx *c, const mm355_hits_t *H, const char *const *qnames, const char *const *seqs, const int32_t *qlens,
                                                                    const char *const *quals, const int32_t *rep_len, int sam_flags, bool has_cigar, Out **out, const RecAux &ax = RecAux(),
                                                                    const RecLast &last = RecLast())
{
	typedef typename rec_kern<F>::type K;
	RecCall k; k.n_reads = H->n_reads; k.n_tiles = 0; k.last = last;
	const char *te = F::TIMES_ENV? getenv(F::TIMES_ENV) : 0; k.times = te && *te && *te != '0';   // (read per call)
	k.t_begin = mm355_now_ms();
	typename F::Dev D;
	if (int rc = rec_upload<K>(c, H, qnames, seqs, qlens, quals, rep_len, ax, sam_flags, has_cigar, &D, &k.t_packed)) return rc;
	const int64_t nr = k.n_reads, nl = k.n_lines = D.n_lines;
	if (nl == 0) return rec_text_empty(nr, out);   // nothing to launch
	hipStream_t st = c->st;
	// lengths and tile counts (one word more each: the scans leave the totals there), their offsets, the CIGAR sums, line_off, the runs, scan
	// space; a format without tiles has neither their counts nor the runs
	size_t tb = 0;
	(void)rocprim::exclusive_scan(nullptr, tb, (int64_t*)0, (int64_t*)0, (int64_t)0, (size_t)nl + 1, rocprim::plus<int64_t>(), st);
	size_t tile_runs = 0;                              // (a format without tiles says nothing about their runs)
	if constexpr (F::TILED) tile_runs = F::TILE_RUNS;
	const size_t w1 = up256((size_t)(nl + 1) * 8), wt = F::TILED? w1 : 0;
	const size_t w_len = 0, w_off = w_len + w1, w_nt = w_off + w1, w_to = w_nt + wt, w_aux = w_to + wt, w_lo = w_aux + w1, w_run = w_lo + up256((size_t)(nr + 1) * 8),
	             w_tmp = w_run + up256((size_t)nl * tile_runs * sizeof(RecTileRun));
	if (c->rec_work.ensure(w_tmp + tb + 256)) return MM355_ENOMEM;
	char *dw = (char*)c->rec_work.p;
	int64_t *d_len = (int64_t*)(dw + w_len), *d_off = (int64_t*)(dw + w_off), *d_nt = (int64_t*)(dw + w_nt), *d_to = (int64_t*)(dw + w_to),
	        *d_aux = (int64_t*)(dw + w_aux), *d_lo = (int64_t*)(dw + w_lo);
	RecTileRun *d_run = (RecTileRun*)(dw + w_run);
	HIPCHK(hipMemsetAsync(d_len + nl, 0, 8, st));
	if constexpr (F::TILED) HIPCHK(hipMemsetAsync(d_nt + nl, 0, 8, st));
	const unsigned grid = (unsigned)((nl + 3) / 4);
	hipLaunchKernelGGL(k_rec_len<K>, dim3(grid), dim3(256), 0, st, D, d_len, d_aux, d_nt);
	HIPCHK(hipGetLastError());
	HIPCHK(rocprim::exclusive_scan(dw + w_tmp, tb, d_len, d_off, (int64_t)0, (size_t)nl + 1, rocprim::plus<int64_t>(), st));
	if constexpr (F::TILED) HIPCHK(rocprim::exclusive_scan(dw + w_tmp, tb, d_nt, d_to, (int64_t)0, (size_t)nl + 1, rocprim::plus<int64_t>(), st));
	hipLaunchKernelGGL(k_rec_line_off, dim3((unsigned)((nr + 1 + 255) / 256)), dim3(256), 0, st, d_off, D.l_first, nr, d_lo);
	HIPCHK(hipGetLastError());
	int64_t *h_tot = (int64_t*)c->h_rec_out.p;
	HIPCHK(hipMemcpyAsync(h_tot, d_off + nl, 8, hipMemcpyDeviceToHost, st));
	if constexpr (F::TILED) HIPCHK(hipMemcpyAsync(h_tot + 1, d_to + nl, 8, hipMemcpyDeviceToHost, st));
	HIPCHK(mm355_wait_stream(st));
	const int64_t tot = k.n_text = h_tot[0];
	if (tot < F::MIN_RECORD * nl) return MM355_EHIP;   // (no record is shorter than its format's fixed part)
	if constexpr (F::TILED) {
		k.n_tiles = h_tot[1];                          // (a tile holds at least one byte of the text)
		if (k.n_tiles < 0 || k.n_tiles > tot || k.n_tiles > (int64_t)INT32_MAX) return MM355_EHIP;
	}
	if (c->rec_text.ensure((size_t)tot + 64)) return MM355_ENOMEM;
	hipLaunchKernelGGL(k_rec_fields<K>, dim3(grid), dim3(256), 0, st, D, d_off, d_aux, (char*)c->rec_text.p, d_run);
	HIPCHK(hipGetLastError());
	if constexpr (F::TILED) if (int rc = F::bulk(c, k, d_run, d_to)) return rc;
	k.d_off = d_off;
	return F::finish(c, k, d_lo, out);
}
template <typename F> static int rec_format_device(mm355_ctx *c, const mm355_hits_t *H, const char *const *qnames, const char *const *seqs, const int32_t *qlens,
                                                   const char *const *quals, const int32_t *rep_len, int sam_flags, bool has_cigar, mm355_text_t **out, const RecAux &ax = RecAux())
{
	return rec_format_device_to<F, mm355_text_t>(c, H, qnames, seqs, qlens, quals, rep_len, sam_flags, has_cigar, out, ax);
}

// the last step of a text format: the text and line_off[] copied into the result record.  k.t_copy: the host clock before the copies
static int rec_text_back(mm355_ctx *c, RecCall &k, const int64_t *d_lo, const char *name, mm355_text_t **out)
{
	mm355_text_t *T = mm355_text_alloc(k.n_reads, k.n_lines, k.n_text);
	if (T == 0) return MM355_ENOMEM;
	k.t_copy = mm355_now_ms();
	hipError_t e = hipMemcpyAsync(T->text, c->rec_text.p, (size_t)k.n_text, hipMemcpyDeviceToHost, c->st);
	if (e == hipSuccess) e = hipMemcpyAsync(T->line_off, d_lo, (size_t)(k.n_reads + 1) * 8, hipMemcpyDeviceToHost, c->st);
	if (e == hipSuccess) e = mm355_wait_stream(c->st);
	if (e != hipSuccess) { fprintf(stderr, "[mm355] HIP error %s in the %s writer\n", hipGetErrorString(e), name); mm355_free_text_host(T); return MM355_EHIP; }
	*out = T;
	return 0;
}

// ---- the front: what follows a format's input check in mm355_{paf,sam,bam}_format.  MM355_PAF_AUTO is resolved against the format's
// variable (read per call: the tests switch it) and its default, one of the two formatters runs, the result is stamped
static int rec_where(int where, int64_t n_hits, const char *min_hits_env, int64_t min_hits_default)
{
	if (where != MM355_PAF_AUTO) return where;
	const char *e = getenv(min_hits_env);
	const int64_t min_hits = e && *e? atoll(e) : min_hits_default;
	return n_hits >= min_hits? MM355_PAF_DEVICE : MM355_PAF_HOST;
}
template <typename Host, typename Dev> static int rec_format_where(int where, int64_t n_hits, const char *min_hits_env, int64_t min_hits_default, Host on_host, Dev on_device,
                                                                   mm355_text_t **out)
{
	const double t0 = mm355_now_ms();
	where = rec_where(where, n_hits, min_hits_env, min_hits_default);
	const int rc = where == MM355_PAF_DEVICE? on_device() : on_host();
	if (rc) return rc;
	(*out)->on_device = where == MM355_PAF_DEVICE;
	(*out)->ms_format = mm355_now_ms() - t0;
	return 0;
}

// mm355_map_batch_sam / _bam: map with rep_len kept, then the format's entry point on the result
typedef int (*rec_format_fn)(mm355_ctx_t*, const mm355_mapopt_t*, const mm355_hits_t*, const char *const*, const char *const*, const int32_t*, const char *const*,
                             const int32_t*, int, int, mm355_text_t**);
static int rec_map_batch(rec_format_fn format, mm355_ctx_t *c, const mm355_mapopt_t *mo, int64_t n_reads, const char *const *seqs, const int32_t *lens,
                         const char *const *names, const char *const *quals, int flags, int sam_flags, int where, mm355_text_t **out)
{
	if (out == 0) return MM355_EINVAL;
	*out = 0;
	if (mo && !(mo->flag & MMF_CIGAR)) return MM355_EINVAL;    // (before anything is mapped)
	mm355_hits_t *H = 0; const int32_t *rep_len = 0;
	int rc = mm355_map_batch_rl(c, mo, n_reads, seqs, lens, names, flags | MM355_OUT_TAGS, &H, &rep_len);
	if (rc) return rc;
	rc = format(c, mo, H, names, seqs, lens, quals, rep_len, sam_flags, where, out);
	mm355_free_hits(H);
	return rc;
}
