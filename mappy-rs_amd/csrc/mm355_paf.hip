// mm355_paf.hip -- the PAF text of a batch result, written on the device: the end of the run that mm355_idxbuild.hip / mm355_idxload.hip begin.
// The line is stated once, in mm355_paf.h (paf_emit_line, templated on a sink); here the same emitter runs with two device sinks, a wave per hit:
//   k_paf_len    the lanes stride over the hit's CIGAR words and add up digits(len) + 1 (wave reduction); lane 0 runs the emitter with the
//                counting sink, which takes that sum for the cg:Z: text.  One int64 length per hit, and the CIGAR text length beside it.
//   scan         rocPRIM's exclusive scan over the lengths: the offset of every line, the total behind the last; line_off[read] is a gather
//                through hit_off.  The total crosses to the host with the call's one synchronisation before the write; the text buffer is sized from it.
//   k_paf_write  lane 0 runs the emitter with the writing sink: single bytes go straight to the text, runs that exist in memory already
//                (the two names, cs, MD) and the CIGAR are noted down with their place in the line.  Then the whole wave copies the runs,
//                lane-strided, and writes the CIGAR in tiles of 64 operations (paf_wave_cigar, shared with the SAM writer).
// Every byte of the text has one writer: plain vector stores, no atomics.  What is uploaded per call: the hit and tags rows, the CIGAR words
// and the string arena (a result of mm355_map_batch lives on the host), the hit-to-read map, the read lengths, the query names cut at their
// first blank.  The contig names are uploaded once per index replica, on first use, and belong to the replica.
#include <stdio.h>
#include <algorithm>
#include <rocprim/device/device_scan.hpp>
#include "mm355_pipeline.h"
#include "mm355_wave.h"
#include "mm355_paf.h"

struct PafDev {
	const mm355_hit_t *hits; const mm355_tags_t *tags; const uint32_t *cigar; const char *str;
	const int32_t *h2r, *qlen; const int64_t *qn_off; const char *qn;   // read of a hit; per read: length, its name = qn[qn_off[r] .. qn_off[r + 1])
	const char *tn; const int64_t *tn_off;                               // contig names, the same way
	int64_t n_hits; int has_cigar;
};

__device__ __forceinline__ PafLine paf_line_dev(const PafDev &D, int64_t k)
{
	PafLine L;
	L.h = D.hits + k; L.t = D.tags + k;
	const int32_t r = D.h2r[k], rid = L.h->rid;
	L.qname = D.qn + D.qn_off[r]; L.qname_len = D.qn_off[r + 1] - D.qn_off[r]; L.qlen = D.qlen[r];
	L.tname = D.tn + D.tn_off[rid]; L.tname_len = D.tn_off[rid + 1] - D.tn_off[rid];
	L.cigar = D.cigar; L.str = D.str; L.has_cigar = D.has_cigar != 0;
	return L;
}

// the counting sink of a wave's lane 0: the CIGAR text length comes from the wave
struct PafDevCount {
	int64_t n = 0, cg;
	__device__ void ch(char) { ++n; }
	__device__ void bytes(const char *, int64_t l) { n += l; }
	__device__ void cigar(const uint32_t *, int64_t) { n += cg; }
};
// a run the wave copies after lane 0 has laid the line out: len bytes (CIGAR: words) from src to byte `at` of the line
struct PafRun { const void *src; int64_t at, len; };
#define PAF_RUNS 4            // qname, tname, cs, MD
struct PafDevWrite {
	char *p; int64_t n = 0, cg; PafRun *runs, *cig; int n_runs = 0;
	__device__ void ch(char c) { p[n++] = c; }
	__device__ void bytes(const char *b, int64_t l) { if (n_runs < PAF_RUNS) runs[n_runs++] = PafRun{ b, n, l }; n += l; }
	__device__ void cigar(const uint32_t *w, int64_t k) { *cig = PafRun{ w, n, k }; n += cg; }
};

__global__ __launch_bounds__(256) void k_paf_len(PafDev D, int64_t *len, int64_t *cglen)
{
	const int lane = threadIdx.x & 63;
	const int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
	if (k >= D.n_hits) return;                 // (the whole wave)
	long long cg = 0;
	if (D.has_cigar) {
		const uint32_t *w = D.cigar + D.hits[k].cigar_off;
		const int32_t nc = D.hits[k].n_cigar;
		for (int32_t i = lane; i < nc; i += 64) cg += paf_cigar_width(w[i]);
		for (int d = 32; d > 0; d >>= 1) cg += __shfl_xor(cg, d);
	}
	if (lane == 0) {
		PafDevCount s; s.cg = cg;
		paf_emit_line(s, paf_line_dev(D, k));
		len[k] = s.n; cglen[k] = cg;
	}
}

__global__ void k_paf_line_off(const int64_t *off, const int64_t *hit_off, int64_t n_reads, int64_t *line_off)
{
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i <= n_reads) line_off[i] = off[hit_off[i]];
}

__global__ __launch_bounds__(256) void k_paf_write(PafDev D, const int64_t *off, const int64_t *cglen, char *text)
{
	__shared__ PafRun runs[4][PAF_RUNS + 1];   // per wave; the last one is the CIGAR
	__shared__ int n_runs[4];
	const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
	const int64_t k = (int64_t)blockIdx.x * 4 + wv;
	const bool on = k < D.n_hits;
	char *line = on? text + off[k] : text;
	if (on && lane == 0) {
		runs[wv][PAF_RUNS] = PafRun{ 0, 0, 0 };
		PafDevWrite s; s.p = line; s.cg = cglen[k]; s.runs = runs[wv]; s.cig = &runs[wv][PAF_RUNS];
		paf_emit_line(s, paf_line_dev(D, k));
		n_runs[wv] = s.n_runs;
	}
	__syncthreads();
	if (!on) return;
	const int nr = n_runs[wv];
	for (int r = 0; r < nr; ++r) {
		const char *src = (const char*)runs[wv][r].src; char *dst = line + runs[wv][r].at;
		const int64_t l = runs[wv][r].len;
		for (int64_t i = lane; i < l; i += 64) dst[i] = src[i];
	}
	paf_wave_cigar(line + runs[wv][PAF_RUNS].at, (const uint32_t*)runs[wv][PAF_RUNS].src, runs[wv][PAF_RUNS].len, lane);
}

// ------------------------------------------------------------------ host side
int mm355_replica_tnames(const mm355_index *mi, int dev, const char **bytes, const int64_t **off)
{
	std::lock_guard<std::mutex> lk(mi->rep_mu);
	for (mm355_replica &r : mi->replicas) if (r.dev == dev) {
		if (r.tname == 0) {
			std::vector<int64_t> o((size_t)mi->n_seq + 1);
			std::string all;
			for (uint32_t i = 0; i < mi->n_seq; ++i) { o[i] = (int64_t)all.size(); all += mi->names[i]; }
			o[mi->n_seq] = (int64_t)all.size();
			void *db = 0, *dof = 0;
			if (hipMalloc(&db, all.size() + 8) != hipSuccess || hipMalloc(&dof, o.size() * 8) != hipSuccess) { if (db) (void)hipFree(db); return MM355_ENOMEM; }
			if ((!all.empty() && hipMemcpy(db, all.data(), all.size(), hipMemcpyHostToDevice) != hipSuccess) ||
			    hipMemcpy(dof, o.data(), o.size() * 8, hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(db); (void)hipFree(dof); return MM355_EHIP; }
			r.tname = db; r.tname_off = dof;
		}
		*bytes = (const char*)r.tname; *off = (const int64_t*)r.tname_off;
		return 0;
	}
	return MM355_EINVAL;
}

static inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

static int paf_format_device(mm355_ctx *c, const mm355_hits_t *H, const char *const *qnames, const int32_t *qlens, bool has_cigar, mm355_text_t **out)
{
	const int64_t nh = H->n_hits, nr = H->n_reads;
	if (nh == 0) {   // nothing to launch
		mm355_text_t *T = mm355_text_alloc(nr, 0, 0);
		if (T == 0) return MM355_ENOMEM;
		for (int64_t i = 0; i <= nr; ++i) T->line_off[i] = 0;
		*out = T;
		return 0;
	}
	if (nh > (int64_t)INT32_MAX || nr > (int64_t)INT32_MAX) return MM355_EINVAL;
	HIPCHK(hipSetDevice(c->dev));
	const char *d_tn = 0; const int64_t *d_tn_off = 0;
	if (int rc = mm355_replica_tnames(c->mi, c->dev, &d_tn, &d_tn_off)) return rc;
	// what the host lays out: hit -> read, and the query names as the line prints them
	std::vector<int64_t> qn_len((size_t)nr);
	int64_t qn_tot = 0;
	for (int64_t i = 0; i < nr; ++i) { qn_len[i] = H->hit_off[i + 1] == H->hit_off[i]? 0 : qnames && qnames[i]? paf_qname_len(qnames[i]) : 1; qn_tot += qn_len[i]; }   // (a read without hits prints nothing)
	const size_t nc = has_cigar && H->n_cigar > 0? (size_t)H->n_cigar : 0, ns = has_cigar && H->n_str > 0? (size_t)H->n_str : 0;
	// one device buffer, one pinned staging buffer for the parts made here (h2r, qn_off, qn)
	const size_t o_hits = 0, o_tags = o_hits + up256((size_t)nh * sizeof(mm355_hit_t)), o_cig = o_tags + up256((size_t)nh * sizeof(mm355_tags_t)),
	             o_str = o_cig + up256(nc * 4 + 4), o_qlen = o_str + up256(ns + 4), o_hoff = o_qlen + up256((size_t)nr * 4), o_made = o_hoff + up256((size_t)(nr + 1) * 8);
	const size_t m_h2r = 0, m_qoff = m_h2r + up256((size_t)nh * 4), m_qn = m_qoff + up256((size_t)(nr + 1) * 8), m_end = m_qn + up256((size_t)qn_tot + 4);
	if (c->paf_in.ensure(o_made + m_end) || c->h_paf_in.ensure(m_end) || c->h_paf_out.ensure(64, 1 << 20)) return MM355_ENOMEM;
	char *hm = (char*)c->h_paf_in.p, *din = (char*)c->paf_in.p;
	int32_t *h2r = (int32_t*)(hm + m_h2r); int64_t *qoff = (int64_t*)(hm + m_qoff); char *qn = hm + m_qn;
	int64_t at = 0;
	for (int64_t i = 0; i < nr; ++i) {
		for (int64_t k = H->hit_off[i]; k < H->hit_off[i + 1]; ++k) h2r[k] = (int32_t)i;
		qoff[i] = at;
		if (qn_len[i] > 0) memcpy(qn + at, qnames && qnames[i]? qnames[i] : "*", (size_t)qn_len[i]);
		at += qn_len[i];
	}
	qoff[nr] = at;
	hipStream_t st = c->st;
	HIPCHK(hipMemcpyAsync(din + o_hits, H->hits, (size_t)nh * sizeof(mm355_hit_t), hipMemcpyHostToDevice, st));
	HIPCHK(hipMemcpyAsync(din + o_tags, H->tags, (size_t)nh * sizeof(mm355_tags_t), hipMemcpyHostToDevice, st));
	if (nc) HIPCHK(hipMemcpyAsync(din + o_cig, H->cigar, nc * 4, hipMemcpyHostToDevice, st));
	if (ns) HIPCHK(hipMemcpyAsync(din + o_str, H->str, ns, hipMemcpyHostToDevice, st));
	HIPCHK(hipMemcpyAsync(din + o_qlen, qlens, (size_t)nr * 4, hipMemcpyHostToDevice, st));
	HIPCHK(hipMemcpyAsync(din + o_hoff, H->hit_off, (size_t)(nr + 1) * 8, hipMemcpyHostToDevice, st));
	HIPCHK(hipMemcpyAsync(din + o_made, hm, m_end, hipMemcpyHostToDevice, st));
	PafDev D;
	D.hits = (const mm355_hit_t*)(din + o_hits); D.tags = (const mm355_tags_t*)(din + o_tags); D.cigar = (const uint32_t*)(din + o_cig); D.str = din + o_str;
	D.h2r = (const int32_t*)(din + o_made + m_h2r); D.qlen = (const int32_t*)(din + o_qlen); D.qn_off = (const int64_t*)(din + o_made + m_qoff); D.qn = din + o_made + m_qn;
	D.tn = d_tn; D.tn_off = d_tn_off; D.n_hits = nh; D.has_cigar = has_cigar;
	// lengths (one word more: the scan leaves the total there), offsets, CIGAR text lengths, line_off, scan space
	size_t tb = 0;
	(void)rocprim::exclusive_scan(nullptr, tb, (int64_t*)0, (int64_t*)0, (int64_t)0, (size_t)nh + 1, rocprim::plus<int64_t>(), st);
	const size_t w_len = 0, w_off = w_len + up256((size_t)(nh + 1) * 8), w_cg = w_off + up256((size_t)(nh + 1) * 8), w_lo = w_cg + up256((size_t)nh * 8),
	             w_tmp = w_lo + up256((size_t)(nr + 1) * 8);
	if (c->paf_work.ensure(w_tmp + tb + 256)) return MM355_ENOMEM;
	char *dw = (char*)c->paf_work.p;
	int64_t *d_len = (int64_t*)(dw + w_len), *d_off = (int64_t*)(dw + w_off), *d_cg = (int64_t*)(dw + w_cg), *d_lo = (int64_t*)(dw + w_lo);
	HIPCHK(hipMemsetAsync(d_len + nh, 0, 8, st));
	const unsigned grid = (unsigned)((nh + 3) / 4);
	hipLaunchKernelGGL(k_paf_len, dim3(grid), dim3(256), 0, st, D, d_len, d_cg);
	HIPCHK(hipGetLastError());
	HIPCHK(rocprim::exclusive_scan(dw + w_tmp, tb, d_len, d_off, (int64_t)0, (size_t)nh + 1, rocprim::plus<int64_t>(), st));
	hipLaunchKernelGGL(k_paf_line_off, dim3((unsigned)((nr + 1 + 255) / 256)), dim3(256), 0, st, d_off, (const int64_t*)(din + o_hoff), nr, d_lo);
	HIPCHK(hipGetLastError());
	int64_t *h_tot = (int64_t*)c->h_paf_out.p;
	HIPCHK(hipMemcpyAsync(h_tot, d_off + nh, 8, hipMemcpyDeviceToHost, st));
	HIPCHK(mm355_wait_stream(st));
	const int64_t tot = *h_tot;
	if (tot < nh) return MM355_EHIP;           // (every line has its newline at least)
	if (c->paf_text.ensure((size_t)tot + 64)) return MM355_ENOMEM;
	hipLaunchKernelGGL(k_paf_write, dim3(grid), dim3(256), 0, st, D, d_off, d_cg, (char*)c->paf_text.p);
	HIPCHK(hipGetLastError());
	mm355_text_t *T = mm355_text_alloc(nr, nh, tot);
	if (T == 0) return MM355_ENOMEM;
	hipError_t e = hipMemcpyAsync(T->text, c->paf_text.p, (size_t)tot, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess) e = hipMemcpyAsync(T->line_off, d_lo, (size_t)(nr + 1) * 8, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess) e = mm355_wait_stream(st);
	if (e != hipSuccess) { fprintf(stderr, "[mm355] HIP error %s in the PAF writer\n", hipGetErrorString(e)); mm355_free_text_host(T); return MM355_EHIP; }
	*out = T;
	return 0;
}

// MM355_PAF_AUTO: the device formatter from this many hits on.  Measured with tools/paf_bench.py (profiles/paf_file.json, format_sweep: ms_format
// of the two formatters on the hits of 16 .. 9216 reads).  CIGAR mode with cs: the host is ahead at 64 hits (0.14 against 0.21 ms), the device at
// 256 (0.32 against 0.57 ms) and 14 times at 9234; the lines cross near 110 hits.  Chain-only (ava-ont): host ahead at 320 hits (0.07 against
// 0.13 ms), device at 1324 (0.14 against 0.18 ms) and 12 times at 62 775; they cross near 1000.  MM355_PAF_MIN_HITS=<n> overrides both (read per
// call: the tests switch it).
#define MM355_PAF_MIN_HITS_CIGAR 128
#define MM355_PAF_MIN_HITS_CHAIN 1024

extern "C" int mm355_paf_format(mm355_ctx_t *c, const mm355_mapopt_t *mo, const mm355_hits_t *H, const char *const *qnames, const int32_t *qlens, int where,
                                mm355_text_t **out)
{
	if (out == 0) return MM355_EINVAL;
	*out = 0;
	if (c == 0 || mo == 0 || H == 0 || (qlens == 0 && H->n_reads > 0) || where < MM355_PAF_AUTO || where > MM355_PAF_DEVICE) return MM355_EINVAL;
	if (c->mi == 0) return MM355_ENOIDX;
	const bool has_cigar = (mo->flag & MMF_CIGAR) != 0;
	if (int rc = mm355_paf_check(H, c->mi->n_seq, has_cigar)) return rc;
	const double t0 = mm355_now_ms();
	if (where == MM355_PAF_AUTO) {
		const char *e = getenv("MM355_PAF_MIN_HITS");
		const int64_t min_hits = e && *e? atoll(e) : has_cigar? MM355_PAF_MIN_HITS_CIGAR : MM355_PAF_MIN_HITS_CHAIN;
		where = H->n_hits >= min_hits? MM355_PAF_DEVICE : MM355_PAF_HOST;
	}
	const PafNames nm = { c->mi->names.data(), c->mi->n_seq };
	const int rc = where == MM355_PAF_DEVICE? paf_format_device(c, H, qnames, qlens, has_cigar, out) : mm355_paf_format_host(H, qnames, qlens, nm, has_cigar, out);
	if (rc) return rc;
	(*out)->on_device = where == MM355_PAF_DEVICE;
	(*out)->ms_format = mm355_now_ms() - t0;
	return 0;
}

extern "C" int mm355_map_batch_paf(mm355_ctx_t *c, const mm355_mapopt_t *mo, int64_t n_reads, const char *const *seqs, const int32_t *lens,
                                   const char *const *names, int flags, int where, mm355_text_t **out)
{
	if (out == 0) return MM355_EINVAL;
	*out = 0;
	mm355_hits_t *H = 0;
	int rc = mm355_map_batch_named(c, mo, n_reads, seqs, lens, names, flags | MM355_OUT_TAGS, &H);
	if (rc) return rc;
	rc = mm355_paf_format(c, mo, H, names, lens, where, out);
	mm355_free_hits(H);
	return rc;
}

extern "C" void mm355_free_text(mm355_text_t *t) { mm355_free_text_host(t); }
