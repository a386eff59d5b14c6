// Test harness (not product): mm355_regs.h compiled for the HOST with g++, like regs_host.cpp, but through the entry that also writes the
// tags rows (mm355_tags_t, MM355_OUT_TAGS).  tests/test_tags_host.py holds the rows against the oracle's mm_reg1_t records.
// force_unsure >= 0: the region with that index after est_err is marked div_unsure before the second half of the tail runs -- the mark
// est_err itself sets about once in 10^6 regions -- to show the pow rule of a tags request (the read is deferred) against the rule without
// tags (deferred only when a strand_retained comparison reads the mark).
#include <vector>
#include <stdlib.h>
#include "../../mappy-rs_amd/csrc/mm355_regs.h"

static const int32_t N_LOGT = 1 << 22;

static const float *logt()
{
	static std::vector<float> t;
	if (t.empty()) {
		t.resize(N_LOGT);
		t[0] = 0.0f;
		for (int32_t i = 1; i < N_LOGT; ++i) t[i] = logf((float)i);
	}
	return t.data();
}

extern "C" int regs_tags_size(void) { return (int)sizeof(mm355_tags_t); }
extern "C" int regs_reg_size(void) { return (int)sizeof(Mm355Reg); }

// opt_i: flag, mask_len, best_n, min_diff, min_strand_sc, min_chain_score, seed; opt_f: mask_level, pri_ratio.  out / tags: n_u rows each;
// tags may be NULL (no tags requested)
extern "C" int regs_tags_host(const int64_t *opt_i, const float *opt_f, const uint32_t *seq_len, int32_t qlen, int32_t rep_len,
                              int n_u, const uint64_t *u, const uint64_t *a, int32_t n_mini, const uint64_t *mini_pos, mm355_hit_t *out,
                              mm355_tags_t *tags, int force_unsure)
{
	Mm355RegsOpt o;
	o.flag = opt_i[0]; o.mask_len = (int32_t)opt_i[1]; o.best_n = (int32_t)opt_i[2]; o.min_diff = (int32_t)opt_i[3];
	o.min_strand_sc = (int32_t)opt_i[4]; o.min_chain_score = (int32_t)opt_i[5]; o.seed = (int32_t)opt_i[6];
	o.mask_level = opt_f[0]; o.pri_ratio = opt_f[1];
	const size_t m = n_u > 0? (size_t)n_u : 1;
	std::vector<Mm355Reg> r(m); std::vector<mm128> z(m); std::vector<uint64_t> cov(m); std::vector<int32_t> w(m), tmp(m); std::vector<uint32_t> mapq(m);
	Mm355RegsScratch s; s.r = r.data(); s.z = z.data(); s.cov = cov.data(); s.w = w.data(); s.tmp = tmp.data();
	const mm128 *aa = (const mm128*)a;
	if (force_unsure < 0)
		return mm355_regs_read(o, seq_len, qlen, rep_len, n_u, u, aa, n_mini, mini_pos, logt(), N_LOGT, s, mapq.data(), out, tags);
	// the steps of mm355_regs_read, with the mark set between its two halves
	if (n_u <= 0 || qlen <= 0) return 0;
	int n = mm355r_gen_regs(mm355r_read_hash(qlen, o.seed), qlen, n_u, u, aa, s.z, s.r);
	if (!(o.flag & MMF_ALL_CHAINS)) {
		mm355r_set_parent(o.mask_level, o.mask_len, n, s.r, (int)(o.flag & MMF_HARD_MLEVEL), s.cov, s.w);
		n = mm355r_select_sub(o.pri_ratio, o.min_diff, o.best_n, o.min_strand_sc, n, s.r, s.tmp);
	}
	mm355r_est_err(seq_len, qlen, n, s.r, aa, n_mini, mini_pos);
	if (force_unsure < n) s.r[force_unsure].div_unsure = 1;
	return mm355r_finish(o, seq_len, rep_len, n, s.r, logt(), N_LOGT, mapq.data(), out, tags);
}
