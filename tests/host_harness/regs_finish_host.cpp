// Test harness (not product): the HOST instantiation of mm355_regs.h -- the region type Reg / Extra of mm355_glue.h, glibc's logf and pow
// (Mm355Libm), caller-provided scratch -- as a stand-alone program for g++ -fsanitize=address,undefined.  tests/test_regs_finish_host.py
// writes the cases to stdin and holds the printed regions against the oracle's mmo_* functions.  The input is a stream of int64 words (a
// float travels as its bit pattern); a case starts with its kind, 1 = post, 2 = pre.
//   post  flag mask_level mask_len sub_diff pri_ratio min_diff best_n min_strand_sc min_chain_sc match_sc rep_len n
//         then per region: id parent cnt rid score score0 qs qe rs re mlen blen subsc n_sub hash rev inv has_p dp_max dp_max2
//         -> what mm355_glue_finish runs after hit_sort: set_parent(sub_diff), select_sub(check_strand = 0), set_sam_pri (none of the three
//            under MM_F_ALL_CHAINS), set_mapq(match_sc), the inversion pass
//   pre   flag mask_level mask_len pri_ratio min_diff best_n min_strand_sc seed qlen n_u n_a n_mini n_seq
//         then u[n_u], a[n_a] as x y pairs, mini_pos[n_mini], seq_len[n_seq]
//         -> what mm355_glue_pre_align runs: gen_regs, set_parent, select_sub(check_strand = 1), est_err (mm355r_regions), then
//            filter_strand_retained with EVERY region marked div_unsure: the host's pow decides, so the mark must not defer the read
// Output per case: the number of regions, then one line per region.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../mappy-rs_amd/csrc/mm355_glue.h"
#include "../../mappy-rs_amd/csrc/mm355_regs.h"

static void rd_n(void *p, size_t n_words)
{
	if (fread(p, 8, n_words, stdin) != n_words) { fprintf(stderr, "short input\n"); exit(2); }
}
static int64_t rd() { int64_t v; rd_n(&v, 1); return v; }
static float rdf() { const uint32_t b = (uint32_t)rd(); float f; memcpy(&f, &b, 4); return f; }

// scratch of exactly n entries each, fresh per case: a step that walks past what the caller provides is the sanitizer's to find
struct Scratch {
	std::vector<mm128> z; std::vector<uint64_t> cov; std::vector<int32_t> w, tmp; std::vector<uint32_t> mapq;
	explicit Scratch(int n) : z(n), cov(n), w(n), tmp(n), mapq(n) {}
	Mm355RegsScratch s() { return Mm355RegsScratch{ 0, z.data(), cov.data(), w.data(), tmp.data() }; }
};

static void post()
{
	Mm355RegsOpt o;
	memset(&o, 0, sizeof(o));
	o.flag = rd(); o.mask_level = rdf(); o.mask_len = (int32_t)rd();
	const int sub_diff = (int)rd();
	o.pri_ratio = rdf(); o.min_diff = (int32_t)rd(); o.best_n = (int32_t)rd(); o.min_strand_sc = (int32_t)rd(); o.min_chain_score = (int32_t)rd();
	const int match_sc = (int)rd(), rep_len = (int)rd();
	int n = (int)rd();
	std::vector<Reg> regs(n);
	for (Reg &r : regs) {
		r.id = (int32_t)rd(); r.parent = (int32_t)rd(); r.cnt = (int32_t)rd(); r.rid = (int32_t)rd(); r.score = (int32_t)rd(); r.score0 = (int32_t)rd();
		r.qs = (int32_t)rd(); r.qe = (int32_t)rd(); r.rs = (int32_t)rd(); r.re = (int32_t)rd(); r.mlen = (int32_t)rd(); r.blen = (int32_t)rd();
		r.subsc = (int32_t)rd(); r.n_sub = (int32_t)rd(); r.hash = (uint32_t)rd(); r.rev = (uint32_t)rd(); r.inv = (uint32_t)rd();
		const int has_p = (int)rd(), dp_max = (int)rd(), dp_max2 = (int)rd();
		if (has_p) { r.p = new Extra(); r.p->dp_max = dp_max; r.p->dp_max2 = dp_max2; }
	}
	Scratch sc(n);
	const Mm355RegsScratch s = sc.s();
	if (!(o.flag & MMF_ALL_CHAINS)) {
		mm355r_set_parent(o.mask_level, o.mask_len, n, regs.data(), (int)(o.flag & MMF_HARD_MLEVEL), s.cov, s.w, sub_diff);
		n = mm355r_select_sub(o.pri_ratio, o.min_diff, o.best_n, o.min_strand_sc, n, regs.data(), s.tmp, 0);
		mm355r_set_sam_pri(n, regs.data());
	}
	if (!mm355r_set_mapq(n, regs.data(), o.min_chain_score, match_sc, rep_len, Mm355Libm(), sc.mapq.data())) { fprintf(stderr, "the host deferred a read\n"); exit(3); }
	for (int i = 0; i < n; ++i) regs[i].mapq = sc.mapq[i];
	mm355_set_inv_mapq(n, regs.data());
	printf("%d\n", n);
	for (int i = 0; i < n; ++i) {
		const Reg &r = regs[i];
		printf("%d %d %d %d %u %u %u %u %d %d\n", r.id, r.parent, r.subsc, r.n_sub, r.mapq, r.sam_pri, r.strand_retained, r.inv, r.score, r.p? r.p->dp_max2 : -1);
		delete r.p;
	}
}

static void pre()
{
	Mm355RegsOpt o;
	memset(&o, 0, sizeof(o));
	o.flag = rd(); o.mask_level = rdf(); o.mask_len = (int32_t)rd(); o.pri_ratio = rdf(); o.min_diff = (int32_t)rd(); o.best_n = (int32_t)rd();
	o.min_strand_sc = (int32_t)rd(); o.seed = (int32_t)rd();
	const int32_t qlen = (int32_t)rd();
	const int n_u = (int)rd(), n_a = (int)rd(), n_mini = (int)rd(), n_seq = (int)rd();
	std::vector<uint64_t> u(n_u), mini(n_mini);
	std::vector<mm128> a(n_a);
	std::vector<uint32_t> seq_len(n_seq);
	rd_n(u.data(), u.size()); rd_n(a.data(), a.size() * 2); rd_n(mini.data(), mini.size());
	for (uint32_t &x : seq_len) x = (uint32_t)rd();
	std::vector<Reg> regs(n_u);
	Scratch sc(n_u);
	int n = mm355r_regions(o, seq_len.data(), qlen, n_u, u.data(), a.data(), n_mini, mini.data(), 0, sc.s(), regs.data());
	for (int i = 0; i < n; ++i) regs[i].div_unsure = 1;
	n = mm355r_filter_strand_retained(n, regs.data(), mm355r_pow_decides(Mm355Libm()));
	printf("%d\n", n);
	for (int i = 0; i < n; ++i) {
		const Reg &r = regs[i];
		uint32_t div; memcpy(&div, &r.div, 4);
		printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %u %u %u %u %u\n", r.id, r.parent, r.cnt, r.rid, r.score, r.score0, r.qs, r.qe, r.rs, r.re, r.as, r.mlen,
		       r.blen, r.subsc, r.n_sub, r.hash, r.rev, r.strand_retained, r.sam_pri, div);
	}
}

int main()
{
	int64_t kind;
	while (fread(&kind, 8, 1, stdin) == 1) {
		if (kind == 1) post();
		else if (kind == 2) pre();
		else { fprintf(stderr, "unknown case kind %lld\n", (long long)kind); return 2; }
	}
	return 0;
}
