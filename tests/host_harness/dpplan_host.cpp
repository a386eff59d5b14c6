// Test harness (not product): mm355_dpplan.h -- the plan of one extension problem, the one statement behind mm355_dp_run's layout and the HBM
// budget of a round -- compiled for the HOST with g++ as a stand-alone program (tests/test_dp_plan_host.py).
//   dpplan_host <use_band> <band_force> [time]
// stdin: one problem per line, "a b sc_ambi q e q2 e2 max_sw_mat qlen tlen w flag"; stdout: one line per problem,
// "skip group pad dlo lmin bw matrix_bytes line cigar_words state_words regw_lds budget_bytes".  `time`: a million plans over the problems
// read, nanoseconds per plan (the budget loop of a round calls the plan once per request, serially).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <chrono>
#include <vector>
#include "../../mappy-rs_amd/csrc/mm355_dpplan.h"

struct Problem { mm355_mapopt_t mo; int qlen, tlen, w, flag; };

int main(int argc, char **argv)
{
	if (argc < 3) { fprintf(stderr, "usage: dpplan_host <use_band> <band_force> [time]\n"); return 2; }
	DpKnobs kn;
	kn.use_band = atoi(argv[1]) != 0; kn.band_force = atoi(argv[2]);
	std::vector<Problem> in;
	long long v[12];
	while (scanf("%lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld", v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6, v + 7, v + 8, v + 9, v + 10, v + 11) == 12) {
		Problem x; memset(&x, 0, sizeof(x));
		x.mo.a = (int)v[0]; x.mo.b = (int)v[1]; x.mo.sc_ambi = (int)v[2]; x.mo.q = (int)v[3]; x.mo.e = (int)v[4]; x.mo.q2 = (int)v[5]; x.mo.e2 = (int)v[6];
		x.mo.max_sw_mat = v[7]; x.qlen = (int)v[8]; x.tlen = (int)v[9]; x.w = (int)v[10]; x.flag = (int)v[11];
		in.push_back(x);
	}
	if (argc > 3 && !strcmp(argv[3], "time")) {
		const size_t total = 1000000; size_t done = 0; unsigned long long sink = 0;
		const auto t0 = std::chrono::steady_clock::now();
		while (done < total && !in.empty()) for (size_t i = 0; i < in.size() && done < total; ++i, ++done) {
			const DpConst dc = mm355_dp_const(&in[i].mo);
			sink += mm355_dp_plan_budget(mm355_dp_plan(dc, kn, in[i].mo.max_sw_mat, in[i].qlen, in[i].tlen, in[i].w, in[i].flag));
		}
		const double ns = std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count();
		printf("ns_per_plan %.2f sink %llu\n", ns / (double)total, sink);
		return 0;
	}
	for (const Problem &x : in) {
		const DpConst dc = mm355_dp_const(&x.mo);
		const DpPlan p = mm355_dp_plan(dc, kn, x.mo.max_sw_mat, x.qlen, x.tlen, x.w, x.flag);
		printf("%d %d %d %d %d %d %zu %d %zu %zu %zu %zu\n", p.skip, p.group, p.pad, p.dlo, p.lmin, p.bw, p.bt_bytes, p.line? 1 : 0, p.cig_words, p.st_words, p.regw_lds,
		       mm355_dp_plan_budget(p));
	}
	return 0;
}
