// Test harness (not product): the host-side pieces of query-name support compiled with g++ alone -- mm355_regs.h's tail with a name hash,
// the MM_SEED_SELF clamp of mm355_selfclamp.h and the name ranking of mm355_names.h.  tests/test_named_host.py holds them against the
// oracle, a hand-worked table and Python's bytes comparison.
#include <vector>
#include <string>
#include <stdlib.h>
#include "../../mappy-rs_amd/csrc/mm355_regs.h"
#include "../../mappy-rs_amd/csrc/mm355_selfclamp.h"
#include "../../mappy-rs_amd/csrc/mm355_names.h"

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

// as regs_tags_host (regs_tags_host.cpp), plus the name hash; with_hash = 0 calls the form without the argument
extern "C" int named_regs_host(const int64_t *opt_i, const float *opt_f, const uint32_t *seq_len, int32_t qlen, int32_t rep_len,
                               int n_u, const uint64_t *u, const uint64_t *a, int32_t n_mini, const uint64_t *mini_pos, mm355_hit_t *out,
                               mm355_tags_t *tags, int with_hash, uint32_t name_hash)
{
	Mm355RegsOpt o;
	o.flag = opt_i[0]; o.mask_len = (int32_t)opt_i[1]; o.best_n = (int32_t)opt_i[2]; o.min_diff = (int32_t)opt_i[3];
	o.min_strand_sc = (int32_t)opt_i[4]; o.min_chain_score = (int32_t)opt_i[5]; o.seed = (int32_t)opt_i[6];
	o.mask_level = opt_f[0]; o.pri_ratio = opt_f[1];
	const size_t m = n_u > 0? (size_t)n_u : 1;
	std::vector<Mm355Reg> r(m); std::vector<mm128> z(m); std::vector<uint64_t> cov(m); std::vector<int32_t> w(m), tmp(m); std::vector<uint32_t> mapq(m);
	Mm355RegsScratch s; s.r = r.data(); s.z = z.data(); s.cov = cov.data(); s.w = w.data(); s.tmp = tmp.data();
	if (!with_hash) return mm355_regs_read(o, seq_len, qlen, rep_len, n_u, u, (const mm128*)a, n_mini, mini_pos, logt(), N_LOGT, s, mapq.data(), out, tags);
	return mm355_regs_read(o, seq_len, qlen, rep_len, n_u, u, (const mm128*)a, n_mini, mini_pos, logt(), N_LOGT, s, mapq.data(), out, tags, name_hash);
}

extern "C" uint32_t named_read_hash(int32_t qlen, int32_t seed, uint32_t name_hash) { return mm355r_read_hash(qlen, seed, name_hash); }
extern "C" uint32_t named_read_hash0(int32_t qlen, int32_t seed) { return mm355r_read_hash(qlen, seed); }
extern "C" uint32_t named_x31(const char *s) { return mm355_x31(s); }

// c[8] = rs, qs, re, qe, rs0, qs0, re0, qe0 -> c[4..7] clamped in place
extern "C" void named_clamp(int32_t *c) { mm355_self_clamp(c[0], c[1], c[2], c[3], &c[4], &c[5], &c[6], &c[7]); }

// rank[n_names] of the contig names; key[n_q] of the query names (a null query = an unnamed read)
extern "C" void named_prepare(int n_names, const char *const *names, uint32_t *rank, int n_q, const char *const *qnames, uint64_t *key)
{
	std::vector<std::string> v, sorted; std::vector<uint32_t> r;
	for (int i = 0; i < n_names; ++i) v.emplace_back(names[i]);
	mm355_name_ranks(v, sorted, r);
	for (int i = 0; i < n_names; ++i) rank[i] = r[i];
	for (int i = 0; i < n_q; ++i) key[i] = mm355_name_key(sorted, qnames[i]);
}

extern "C" int named_filter_applies(int any_named, int64_t map_flag, int32_t idx_flag) { return mm355_name_filter_applies(any_named != 0, map_flag, idx_flag)? 1 : 0; }
