// bamaux_host.cpp -- the copied aux tags on the host as a stand-alone program (g++ alone, AddressSanitizer + UBSan; tests/test_bamaux_host.py):
//   split <in> <out>              cases written by the test -- int32 n, int32 keep length (-1: NULL), the keep bytes, the n aux bytes -- through
//                                 bam_aux_split (mm355_bamaux.h), every block and every output buffer a heap block of its exact size:
//                                 per case int32 rc, n_out, mod_off and the n_out bytes
//   sets <in> <aux> <out> <level> result sets (tests/_sam_sets.py::serialize) and their tags (tests/_bamaux.py::serialize_aux) through
//                                 mm355_bam_check_aux and the host formatter: per set n_text, n_lines, line_off and the BGZF bytes
//   check <in> <aux>              mm355_bam_check_aux on every set: one "rc <code>" line each
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <memory>
#include <string>
#include <vector>
#include "../../mappy-rs_amd/csrc/mm355_bam.h"
#include "../../mappy-rs_amd/csrc/mm355_bamaux.h"
#include "../../mappy-rs_amd/csrc/mm355_deflate.h"

static bool rd(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

static int run_split(const char *in, const char *outp)
{
	FILE *f = fopen(in, "rb"), *o = fopen(outp, "wb");
	if (!f || !o) return 2;
	long n_cases = 0;
	for (;; ++n_cases) {
		int32_t hd[2];
		if (fread(hd, 4, 2, f) != 2) break;
		const int32_t n = hd[0], lk = hd[1];
		std::unique_ptr<char[]> keep(lk >= 0? new char[(size_t)lk + 1] : 0);
		if (lk >= 0) { if (!rd(f, keep.get(), (size_t)lk)) return 3; keep[(size_t)lk] = 0; }
		const size_t nb = n > 0? (size_t)n : 0;
		std::unique_ptr<uint8_t[]> aux(new uint8_t[nb]), out(new uint8_t[nb]);   // exact sizes: a byte read or written past the end is a report
		if (!rd(f, aux.get(), nb)) return 3;
		int32_t res[3] = { 0, -7, -7 };
		res[0] = bam_aux_split(aux.get(), n, keep.get(), out.get(), &res[1], &res[2]);
		if (res[0] == 0 && (res[1] < 0 || res[1] > n || res[2] < 0 || res[2] > res[1])) return 4;
		fwrite(res, 4, 3, o);
		if (res[0] == 0) fwrite(out.get(), 1, (size_t)res[1], o);
	}
	fclose(f); fclose(o);
	printf("split %ld\n", n_cases);
	return 0;
}

// the host formatter at level 1, as mm355_bam.hip has it
struct DeflateFmt : BamFmt {
	static int64_t frame_host(const char *raw, int64_t n, char *out) { return mm355_bgzf_deflate_host(raw, n, out); }
};

// the stream layout of sam_host.cpp's sets, and beside it the tags of every read
static int run_sets(const char *in, const char *auxp, const char *outp, int level, bool check_only)
{
	FILE *f = fopen(in, "rb"), *fa = fopen(auxp, "rb"), *o = outp? fopen(outp, "wb") : 0;
	if (!f || !fa || (outp && !o)) return 2;
	long n_sets = 0;
	for (;;) {
		int64_t hd[11];
		if (fread(hd, 8, 11, f) != 11) break;
		const int64_t nr = hd[0], nh = hd[1], nc = hd[2], ns = hd[3];
		const bool has_cigar = hd[4] != 0;
		const int sam_flags = (int)hd[10];
		std::vector<int64_t> hit_off((size_t)nr + 1); std::vector<int32_t> status((size_t)nr), qlens((size_t)nr), rep((size_t)nr);
		std::vector<uint8_t> has_name((size_t)nr), has_qual((size_t)nr), has_seq((size_t)nr);
		std::vector<mm355_hit_t> hits((size_t)nh); std::vector<mm355_tags_t> tags((size_t)nh); std::vector<uint32_t> cig((size_t)nc); std::vector<char> str((size_t)ns);
		std::vector<char> cb((size_t)hd[6]), qb((size_t)hd[7]), sq((size_t)hd[8]), ql((size_t)hd[9]);
		if (!rd(f, hit_off.data(), hit_off.size() * 8) || !rd(f, status.data(), (size_t)nr * 4) || !rd(f, qlens.data(), (size_t)nr * 4) || !rd(f, rep.data(), (size_t)nr * 4) ||
		    !rd(f, has_name.data(), (size_t)nr) || !rd(f, has_qual.data(), (size_t)nr) || !rd(f, has_seq.data(), (size_t)nr) ||
		    !rd(f, hits.data(), (size_t)nh * sizeof(mm355_hit_t)) || !rd(f, tags.data(), (size_t)nh * sizeof(mm355_tags_t)) || !rd(f, cig.data(), (size_t)nc * 4) ||
		    !rd(f, str.data(), (size_t)ns) || !rd(f, cb.data(), cb.size()) || !rd(f, qb.data(), qb.size()) || !rd(f, sq.data(), sq.size()) || !rd(f, ql.data(), ql.size())) return 3;
		std::vector<std::string> contigs;
		for (size_t a = 0; a < cb.size(); a += strlen(&cb[a]) + 1) contigs.emplace_back(&cb[a]);
		if ((int64_t)contigs.size() != hd[5]) return 4;
		std::vector<const char*> qn((size_t)nr, (const char*)0), sp((size_t)nr, (const char*)0), qp((size_t)nr, (const char*)0);
		std::vector<std::vector<char>> own;      // every read, quality string and aux block in a heap block of its own size
		std::vector<std::unique_ptr<uint8_t[]>> aux_own;
		std::vector<const uint8_t*> ap((size_t)nr, (const uint8_t*)0); std::vector<int32_t> alen((size_t)nr), amod((size_t)nr);
		size_t a = 0, sa = 0, qa = 0;
		for (int64_t i = 0; i < nr; ++i) {
			if (has_name[i]) { qn[i] = &qb[a]; a += strlen(&qb[a]) + 1; }
			size_t l = qlens[i] > 0? (size_t)qlens[i] : 0;
			if (check_only && l > sq.size() - sa) l = sq.size() - sa;   // (a set for the check may claim a longer read than it brings)
			own.emplace_back(sq.begin() + (long)sa, sq.begin() + (long)(sa + l)); sa += l;
			if (has_seq[i]) sp[i] = own.back().empty()? "" : own.back().data();
			if (has_qual[i]) { const size_t m = l < ql.size() - qa? l : ql.size() - qa; own.emplace_back(ql.begin() + (long)qa, ql.begin() + (long)(qa + m)); qa += m; qp[i] = own.back().empty()? "" : own.back().data(); }
			int32_t ah[4];
			if (fread(ah, 4, 4, fa) != 4 || ah[2] < 0) return 3;
			alen[i] = ah[0]; amod[i] = ah[1];
			aux_own.emplace_back(new uint8_t[(size_t)ah[2]]);
			if (!rd(fa, aux_own.back().get(), (size_t)ah[2])) return 3;
			if (!ah[3]) ap[i] = aux_own.back().get();
		}
		mm355_hits_t H; memset(&H, 0, sizeof(H));
		H.n_reads = nr; H.hit_off = hit_off.data(); H.status = status.data(); H.hits = hits.data(); H.cigar = cig.data(); H.str = str.data();
		H.n_hits = nh; H.n_cigar = nc; H.n_str = ns; H.tags = tags.data();
		static mm355_tags_t no_tags;
		if (nh == 0) H.tags = &no_tags;
		const PafNames nm = { contigs.data(), (uint32_t)contigs.size() };
		RecAux ax; ax.aux = ap.data(); ax.len = alen.data(); ax.mod = amod.data();
		int rc = mm355_bam_check_aux(&H, nm, has_cigar, qn.data(), sp.data(), qlens.data(), rep.data(), sam_flags, ax);
		if (check_only) { printf("rc %d\n", rc); ++n_sets; continue; }
		if (rc) { printf("set %ld: check %d\n", n_sets, rc); return 5; }
		mm355_text_t *T = 0;
		rc = level? mm355_rec_format_host<DeflateFmt>(&H, qn.data(), sp.data(), qlens.data(), qp.data(), rep.data(), nm, sam_flags, &T, ax)
		          : mm355_bam_format_host(&H, qn.data(), sp.data(), qlens.data(), qp.data(), rep.data(), nm, sam_flags, &T, ax);
		if (rc) { printf("set %ld: format %d\n", n_sets, rc); return 6; }
		fwrite(&T->n_text, 8, 1, o); fwrite(&T->n_lines, 8, 1, o); fwrite(T->line_off, 8, (size_t)nr + 1, o); fwrite(T->text, 1, (size_t)T->n_text, o);
		mm355_free_text_host(T);
		++n_sets;
	}
	fclose(f); fclose(fa); if (o) fclose(o);
	printf("sets %ld\n", n_sets);
	return 0;
}

int main(int argc, char **argv)
{
	if (argc == 4 && !strcmp(argv[1], "split")) return run_split(argv[2], argv[3]);
	if (argc == 6 && !strcmp(argv[1], "sets")) return run_sets(argv[2], argv[3], argv[4], atoi(argv[5]), false);
	if (argc == 4 && !strcmp(argv[1], "check")) return run_sets(argv[2], argv[3], 0, 0, true);
	fprintf(stderr, "usage: bamaux_host split <in> <out> | sets <in> <aux> <out> <level> | check <in> <aux>\n");
	return 64;
}
