// Test harness (not product): the chain-only tail of a read -- mm355_regs.h, the header k_regs compiles for the device -- compiled for the
// HOST with g++, so that the CPU suite holds it against the oracle: tests/test_chain_only_host.py feeds it the oracle's anchors and final
// chains of a read and compares its hit rows with the oracle's mapping without MM_F_CIGAR.  The logf table is filled here the way the
// library fills the device's (glibc logf of every index).
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

extern "C" int regs_hit_size(void) { return (int)sizeof(mm355_hit_t); }

// opt_i: flag, mask_len, best_n, min_diff, min_strand_sc, min_chain_score, seed; opt_f: mask_level, pri_ratio.  out: n_u hit rows.
extern "C" int regs_host(const int64_t *opt_i, const float *opt_f, const uint32_t *seq_len, int32_t qlen, int32_t rep_len,
                         int n_u, const uint64_t *u, const uint64_t *a, int32_t n_mini, const uint64_t *mini_pos, mm355_hit_t *out)
{
	Mm355RegsOpt o;
	o.flag = opt_i[0]; o.mask_len = (int32_t)opt_i[1]; o.best_n = (int32_t)opt_i[2]; o.min_diff = (int32_t)opt_i[3];
	o.min_strand_sc = (int32_t)opt_i[4]; o.min_chain_score = (int32_t)opt_i[5]; o.seed = (int32_t)opt_i[6];
	o.mask_level = opt_f[0]; o.pri_ratio = opt_f[1];
	const size_t m = n_u > 0? (size_t)n_u : 1;
	std::vector<Mm355Reg> r(m); std::vector<mm128> z(m); std::vector<uint64_t> cov(m); std::vector<int32_t> w(m), tmp(m); std::vector<uint32_t> mapq(m);
	Mm355RegsScratch s; s.r = r.data(); s.z = z.data(); s.cov = cov.data(); s.w = w.data(); s.tmp = tmp.data();
	return mm355_regs_read(o, seq_len, qlen, rep_len, n_u, u, (const mm128*)a, n_mini, mini_pos, logt(), N_LOGT, s, mapq.data(), out);
}
