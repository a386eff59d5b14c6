// mm355_paf.hip -- the PAF text of a batch result, written on the device: the end of the run that mm355_idxbuild.hip / mm355_idxload.hip begin.
// The line is stated once, in mm355_paf.h (paf_emit_line); the device record writer of mm355_recdev.h runs it, a wave per hit.  What is
// PAF's own: a record is a hit, so a read without hits writes nothing and H->status is not needed; the CIGAR is text (cg:Z:); a line
// carries no read, so there are no tiles, no second scan and no bulk kernel.  The contig names every format prints are uploaded here.
#include "mm355_recdev.h"

// PafFmt as the device writes it
struct PafDevFmt : PafFmt {
	typedef RecDev Dev;
	typedef RecCount Count;
	typedef RecWrite<RUNS> Write;
	static constexpr const char *TIMES_ENV = 0;
	static int finish(mm355_ctx *c, RecCall &k, const int64_t *d_lo, mm355_text_t **out) { return rec_text_back(c, k, d_lo, "PAF", out); }
};

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
	const PafNames nm = { c->mi->names.data(), c->mi->n_seq };
	return rec_format_where(where, H->n_hits, "MM355_PAF_MIN_HITS", has_cigar? MM355_PAF_MIN_HITS_CIGAR : MM355_PAF_MIN_HITS_CHAIN,
	                        [&] { return mm355_paf_format_host(H, qnames, qlens, nm, has_cigar, out); },
	                        [&] { return rec_format_device<PafDevFmt>(c, H, qnames, 0, qlens, 0, 0, 0, has_cigar, out); }, out);
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
