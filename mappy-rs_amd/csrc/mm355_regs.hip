// mm355_regs.hip -- the chain-only tail of a batch (mapping without MM_F_CIGAR, minimap2's default output mode): after the chainers
// (mm355_run_rmq) the chains of every read are still in HBM (u / a at aoff, mini_pos at roff).  k_regs turns them into regions, selects
// primaries and secondaries, estimates the divergence, computes MAPQ and writes the hit rows on the device (mm355_regs.h, a lane per read);
// only the rows and one count per read come back.  Reads the device does not decide -- those the RMQ stage left to the host, and those
// mm355_regs.h defers (logf argument beyond the table, a strand_retained comparison on an unsure divergence, with MM355_OUT_TAGS any
// reported divergence that is unsure) -- are packed alone and run through mm355_glue_regions + mm355_glue_chain_finish on the host pool.
// MM355_REGS_HOST=1 sends every read that way.  With MM355_OUT_TAGS a tags row (mm355_tags_t) goes with every hit row on both paths.
#include <stdio.h>
#include <string.h>
#include <mutex>
#include "mm355_pipeline.h"
#include "mm355_rmq.h"
#include "mm355_glue.h"
#include "mm355_regs.h"
#include "mm355_hits.h"

#define REGS_LOGT_N (1 << 22)     // logf(1 .. 2^22 - 1): chain scores of reads up to a few Mb (a chain scores at most about its query span)

struct RegsRead {                 // per read of the batch
	int64_t hoff;                 // first scratch / row slot (exclusive scan of n_u over the reads the device takes)
	int32_t qlen, rep_len, n_u, n_mini;
	int32_t run;                  // 1 = the device takes the read
	uint32_t name_hash;           // X31 of the query name as U:map.c::mm_map_frag hashes it; 0 for an unnamed read (the word was padding before)
};

#define K_REGS_ARGS int n_reads, const RegsRead *rr, const int64_t *aoff, const int64_t *roff, const uint64_t *u,                     \
                    const mm128 *a, const uint64_t *mini_pos, const uint32_t *seq_len, Mm355RegsOpt o,                           \
                    const float *logt, int32_t n_logt, Mm355Reg *sr, mm128 *sz, uint64_t *scov, int32_t *sw,                     \
                    int32_t *stmp, uint32_t *smq, mm355_hit_t *hits, int32_t *cnt
__device__ __forceinline__ void regs_lane(K_REGS_ARGS, mm355_tags_t *tags)
{
	const int r = blockIdx.x * 64 + threadIdx.x;
	if (r >= n_reads) return;
	const RegsRead q = rr[r];
	if (!q.run) { cnt[r] = 0; return; }
	const int64_t h = q.hoff;     // every write of the read stays in [h, h + n_u) of each scratch array, of hits and of tags
	Mm355RegsScratch s;
	s.r = sr + h; s.z = sz + h; s.cov = scov + h; s.w = sw + h; s.tmp = stmp + h;
	const int64_t ao = aoff[r];
	cnt[r] = mm355_regs_read(o, seq_len, q.qlen, q.rep_len, q.n_u, u + ao, a + ao, q.n_mini, mini_pos + roff[r], logt, n_logt, s, smq + h, hits + h,
	                         tags? tags + h : nullptr, q.name_hash);
}
// two entry points over one body: without MM355_OUT_TAGS the kernel takes the arguments and runs the code it always did
__global__ __launch_bounds__(64) void k_regs(K_REGS_ARGS)
{
	regs_lane(n_reads, rr, aoff, roff, u, a, mini_pos, seq_len, o, logt, n_logt, sr, sz, scov, sw, stmp, smq, hits, cnt, nullptr);
}
__global__ __launch_bounds__(64) void k_regs_tags(K_REGS_ARGS, mm355_tags_t *tags)
{
	regs_lane(n_reads, rr, aoff, roff, u, a, mini_pos, seq_len, o, logt, n_logt, sr, sz, scov, sw, stmp, smq, hits, cnt, tags);
}
#undef K_REGS_ARGS

static const std::vector<float> &host_logt()
{   // the host's logf of every table index, once per process (the values mm_set_mapq computes on the host)
	static std::vector<float> t;
	static std::once_flag once;
	std::call_once(once, [] { t.resize(REGS_LOGT_N); t[0] = 0.0f; for (int32_t i = 1; i < REGS_LOGT_N; ++i) t[i] = logf((float)i); });
	return t;
}

static inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

int mm355_map_chain_only(mm355_ctx *c, const mm355_mapopt_t *mo, const std::vector<int32_t> &qlen, int flags, mm355_hits_t **out)
{
	*out = 0;
	const bool want_tags = (flags & MM355_OUT_TAGS) != 0;
	const mm355_index *mi = c->mi;
	HostBatch &hb = c->hb;
	const int64_t n_reads = hb.n_reads;
	const bool all_host = [] { const char *e = getenv("MM355_REGS_HOST"); return e && atoi(e) != 0; }();   // (read per call: the tests switch it)
	// test hook: only the first n entries of the logf table count, so that reads with larger chain scores take the defer path
	const int32_t n_logt = [] { const char *e = getenv("MM355_REGS_LOGT_N"); const long v = e? atol(e) : 0; return v > 1 && v < REGS_LOGT_N? (int32_t)v : (int32_t)REGS_LOGT_N; }();
	// which reads the device takes, and their row slots
	if (c->h_regs_in.ensure((size_t)(n_reads + 1) * sizeof(RegsRead))) return MM355_ENOMEM;
	RegsRead *rr = (RegsRead*)c->h_regs_in.p;
	int64_t tot = 0, n_run = 0;
	for (int64_t i = 0; i < n_reads; ++i) {
		RegsRead &q = rr[i];
		memset(&q, 0, sizeof(q));
		const int rst = hb.rmq_state.empty()? MM355_RMQ_HOST_ALL : (int)hb.rmq_state[i];
		q.qlen = qlen[i]; q.rep_len = hb.rep_len[i]; q.n_u = hb.n_u[i]; q.n_mini = hb.n_mini[i]; q.name_hash = mm355_read_name_hash(hb, mo->flag, i);
		q.run = !all_host && q.qlen > 0 && (rst == MM355_RMQ_KEEP || rst == MM355_RMQ_DONE);
		q.hoff = tot;
		if (q.run) { tot += q.n_u; ++n_run; }
	}
	const size_t nt = (size_t)(tot > 0? tot : 1);
	const size_t o_z = al256(nt * sizeof(Mm355Reg)), o_cov = o_z + al256(nt * 16), o_w = o_cov + al256(nt * 8), o_tmp = o_w + al256(nt * 4),
	             o_mq = o_tmp + al256(nt * 4), o_hit = o_mq + al256(nt * 4), o_cnt = o_hit + al256(nt * sizeof(mm355_hit_t)),
	             o_tag = o_cnt + al256((size_t)(n_reads + 1) * 4), scr_b = o_tag + (want_tags? al256(nt * sizeof(mm355_tags_t)) : 0);
	const size_t ho_tag = al256(nt * sizeof(mm355_hit_t)) + al256((size_t)(n_reads + 1) * 4);
	const size_t out_b = ho_tag + (want_tags? nt * sizeof(mm355_tags_t) : 0);
	if (c->regs_scr.ensure(scr_b) || c->regs_in.ensure((size_t)(n_reads + 1) * sizeof(RegsRead)) || c->h_regs_out.ensure(out_b)) return MM355_ENOMEM;
	char *scr = c->regs_scr.as<char>();
	mm355_hit_t *h_rows = (mm355_hit_t*)c->h_regs_out.p;
	int32_t *h_cnt = (int32_t*)((char*)c->h_regs_out.p + al256(nt * sizeof(mm355_hit_t)));
	mm355_tags_t *h_tags = want_tags? (mm355_tags_t*)((char*)c->h_regs_out.p + ho_tag) : 0;
	if (n_run > 0) {
		if (!c->logt_ok) {
			const std::vector<float> &t = host_logt();
			if (c->logt.ensure(t.size() * 4, 1 << 30)) return MM355_ENOMEM;
			HIPCHK(hipMemcpy(c->logt.p, t.data(), t.size() * 4, hipMemcpyHostToDevice));
			c->logt_ok = true;
		}
		const Mm355RegsOpt o = mm355_regs_opt(mo, mi->k);
		HIPCHK(hipMemcpyAsync(c->regs_in.p, rr, (size_t)n_reads * sizeof(RegsRead), hipMemcpyHostToDevice, c->st));
		mm355_kt(c, KT_REGS, 0, c->st);
#define K_REGS_ACTUALS (int)n_reads, c->regs_in.as<RegsRead>(), c->aoff.as<int64_t>(), c->roff.as<int64_t>(), c->u.as<uint64_t>(), c->a.as<mm128>(),    \
		               c->mini_pos.as<uint64_t>(), c->dix.seq_len, o, c->logt.as<float>(), n_logt, (Mm355Reg*)scr, (mm128*)(scr + o_z),                    \
		               (uint64_t*)(scr + o_cov), (int32_t*)(scr + o_w), (int32_t*)(scr + o_tmp), (uint32_t*)(scr + o_mq), (mm355_hit_t*)(scr + o_hit),      \
		               (int32_t*)(scr + o_cnt)
		if (want_tags) hipLaunchKernelGGL(k_regs_tags, dim3((unsigned)((n_reads + 63) / 64)), dim3(64), 0, c->st, K_REGS_ACTUALS, (mm355_tags_t*)(scr + o_tag));
		else hipLaunchKernelGGL(k_regs, dim3((unsigned)((n_reads + 63) / 64)), dim3(64), 0, c->st, K_REGS_ACTUALS);
#undef K_REGS_ACTUALS
		mm355_kt(c, KT_REGS, 1, c->st);
		HIPCHK(hipGetLastError());
		HIPCHK(hipMemcpyAsync(h_cnt, scr + o_cnt, (size_t)n_reads * 4, hipMemcpyDeviceToHost, c->st));
		if (tot > 0) HIPCHK(hipMemcpyAsync(h_rows, scr + o_hit, (size_t)tot * sizeof(mm355_hit_t), hipMemcpyDeviceToHost, c->st));
		if (tot > 0 && want_tags) HIPCHK(hipMemcpyAsync(h_tags, scr + o_tag, (size_t)tot * sizeof(mm355_tags_t), hipMemcpyDeviceToHost, c->st));
		HIPCHK(mm355_wait_stream(c->st));
	}
	// the host path: reads the device did not take or deferred
	std::vector<int32_t> sel;
	for (int64_t i = 0; i < n_reads; ++i) if (qlen[i] > 0 && (!rr[i].run || h_cnt[i] < 0)) sel.push_back((int32_t)i);
	const int64_t n_sel = (int64_t)sel.size();
	std::vector<std::vector<mm355_hit_t>> hh((size_t)n_sel);
	std::vector<std::vector<mm355_tags_t>> ht(want_tags? (size_t)n_sel : 0);
	if (n_sel > 0) {
		PackedChains pk;
		const int rc = mm355_fetch_chains(c, sel.data(), n_sel, &pk);
		if (rc) return rc;
		auto one = [&](int64_t j) {
			ReadState rs;
			const int rst = mm355_seed_read(c, mo, pk, j, qlen[sel[j]], rs);
			mm355_glue_regions(mi, mo, rs, rst);
			mm355_glue_chain_finish(mi, mo, rs, hh[j], want_tags? &ht[j] : 0);
		};
		if (mm355_parallel_hook) mm355_parallel_hook(n_sel, one);
		else for (int64_t j = 0; j < n_sel; ++j) one(j);
	}
	// the batch result, in read order: a read's rows are its host vector, or its span of the device's row buffer
	std::vector<Mm355ReadRows> rows((size_t)n_reads);
	int64_t n_dev = 0;
	for (int64_t i = 0, j = 0; i < n_reads; ++i) {
		Mm355ReadRows &w = rows[i];
		if (j < n_sel && sel[j] == i) { w.hits = hh[j].data(); w.n = (int64_t)hh[j].size(); if (want_tags) w.tags = ht[j].data(); ++j; }
		else if (rr[i].run) { w.hits = h_rows + rr[i].hoff; w.n = h_cnt[i]; if (want_tags) w.tags = h_tags + rr[i].hoff; ++n_dev; }
	}
	const int rc = mm355_hits_assemble(n_reads, hb.status.data(), rows.data(), want_tags, out);
	if (rc) return rc;
	c->stats.n_regs_dev = n_dev; c->stats.n_regs_host = n_sel;
	return 0;
}
