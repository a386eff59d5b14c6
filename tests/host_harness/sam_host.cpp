// sam_host.cpp -- the host side of the SAM writer as a stand-alone program (g++ alone, AddressSanitizer + UBSan; tests/test_sam_host.py):
//   comp                     sam_comp of all 256 byte values, as 512 hex digits
//   sets <in> <out>          result sets written by the test (tests/_sam_sets.py::serialize) -> the host formatter's text and line_off per set;
//                            checks on every set that the counting sink equals the written length line by line and that line_off delimits whole lines
//   check <in>               mm355_sam_check on every set: one "rc <code>" line each
//   fastx <path> <max_reads> <max_bases> <qual>    the streaming reader, opened with quality (1) or without (0): one "batch <n> <quals>" line per
//                            mm355_fastx_next (quals: whether mm355_reads_quals returned an array), one "rec <name> <len> <seq> <quality or ->" line
//                            per record, "rc <code>"
// The reader lives in mm355_index.cpp, which is compiled into this program; what that file calls on the device side is stubbed below.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../mappy-rs_amd/csrc/mm355_index.cpp"
#include "../../mappy-rs_amd/csrc/mm355_sam.h"

// ---- device-side entry points mm355_index.cpp refers to (never reached from here)
void mm355_runtime_init(void) {}
extern "C" int mm355_index_build_device(const mm355_idxopt_t *, int, const uint8_t *const *, const int64_t *, const char *const *, int, mm355_index_t **) { return MM355_ENODEV; }
int mm355_index_dump_buckets_device(const mm355_index *, FILE *) { return MM355_ENODEV; }
void mm355_index_free_replicas(mm355_index *) {}

static int run_comp()
{
	for (int c = 0; c < 256; ++c) printf("%02x", sam_comp((unsigned char)c));
	printf("\n");
	return 0;
}

// ---- result sets.  Per set, little-endian: int64 n_reads, n_hits, n_cigar, n_str, has_cigar, n_contigs, contig_bytes, qname_bytes, seq_bytes,
// qual_bytes, sam_flags; hit_off (n_reads + 1 int64), status, qlens, rep_len (int32 each), has_name, has_qual, has_seq (n_reads bytes each), hit
// rows, tags rows, CIGAR words, string arena, contig names and query names (each NUL-terminated, back to back; an unnamed read has no entry),
// the reads back to back, the quality strings back to back (a read without one has no entry)
static bool rd(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

static int run_sets(const char *in, const char *outp, bool check_only)
{
	FILE *f = fopen(in, "rb"), *o = outp? fopen(outp, "wb") : 0;
	if (!f || (outp && !o)) return 2;
	long n_sets = 0;
	for (;;) {
		int64_t hd[11];
		if (fread(hd, 8, 11, f) != 11) break;
		const int64_t nr = hd[0], nh = hd[1], nc = hd[2], ns = hd[3];
		const bool has_cigar = hd[4] != 0;
		const int sam_flags = (int)hd[10];
		std::vector<int64_t> hit_off((size_t)nr + 1); std::vector<int32_t> status((size_t)nr), qlens((size_t)nr), rep((size_t)nr);
		std::vector<uint8_t> has_name((size_t)nr), has_qual((size_t)nr), has_seq((size_t)nr);
		// exact-size heap blocks: a read past the end of an arena is an AddressSanitizer report
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
		// every read and quality string in a heap block of its own size, for the same reason
		std::vector<std::vector<char>> own;
		size_t a = 0, sa = 0, qa = 0;
		for (int64_t i = 0; i < nr; ++i) {
			if (has_name[i]) { qn[i] = &qb[a]; a += strlen(&qb[a]) + 1; }
			const size_t l = qlens[i] > 0? (size_t)qlens[i] : 0;
			own.emplace_back(sq.begin() + (long)sa, sq.begin() + (long)(sa + l)); sa += l;
			if (has_seq[i]) sp[i] = own.back().empty()? "" : own.back().data();
			if (has_qual[i]) { own.emplace_back(ql.begin() + (long)qa, ql.begin() + (long)(qa + l)); qa += l; qp[i] = own.back().empty()? "" : own.back().data(); }
		}
		mm355_hits_t H; memset(&H, 0, sizeof(H));
		H.n_reads = nr; H.hit_off = hit_off.data(); H.status = status.data(); H.hits = hits.data(); H.cigar = cig.data(); H.str = str.data();
		H.n_hits = nh; H.n_cigar = nc; H.n_str = ns; H.tags = tags.data();
		static mm355_tags_t no_tags;
		if (nh == 0) H.tags = &no_tags;   // (an empty vector has no address, and a result without the tags array is refused)
		const PafNames nm = { contigs.data(), (uint32_t)contigs.size() };
		int rc = mm355_sam_check(&H, nm.n_seq, has_cigar, sp.data(), qlens.data(), rep.data(), sam_flags);
		if (check_only) { printf("rc %d\n", rc); ++n_sets; continue; }
		if (rc) { printf("set %ld: check %d\n", n_sets, rc); return 5; }
		mm355_text_t *T = 0;
		rc = mm355_sam_format_host(&H, qn.data(), sp.data(), qlens.data(), qp.data(), rep.data(), nm, sam_flags, &T);
		if (rc) { printf("set %ld: format %d\n", n_sets, rc); return 6; }
		// the counting sink against the written text, line by line; line_off against whole lines
		const SamNames snm(nm);
		int64_t at = 0, n_lines = 0;
		for (int64_t i = 0; i < nr; ++i) {
			if (T->line_off[i] != at) { printf("set %ld: line_off[%lld]\n", n_sets, (long long)i); return 7; }
			const int64_t nl = mm355_sam_n_lines(&H, qlens.data(), sam_flags, i);
			if (nl == 0) continue;
			const SamRead R = mm355_sam_read_of(&H, i, qn.data(), sp.data(), qlens.data(), qp.data(), rep.data(), snm, sam_flags);
			for (int64_t j = 0; j < nl; ++j, ++n_lines) {
				SamCountSink c;
				sam_emit_line(c, SamLine{ &R, R.n_rows? (int32_t)j : -1 });
				const char *e = (const char*)memchr(T->text + at, '\n', (size_t)(T->n_text - at));
				if (e == 0 || e - (T->text + at) + 1 != c.n) { printf("set %ld: read %lld line %lld counts %lld\n", n_sets, (long long)i, (long long)j, (long long)c.n); return 8; }
				at += c.n;
			}
		}
		if (T->line_off[nr] != at || at != T->n_text || T->n_lines != n_lines || T->n_reads != nr) { printf("set %ld: totals\n", n_sets); return 9; }
		fwrite(&T->n_text, 8, 1, o); fwrite(&T->n_lines, 8, 1, o); fwrite(T->line_off, 8, (size_t)nr + 1, o); fwrite(T->text, 1, (size_t)T->n_text, o);
		mm355_free_text_host(T);
		++n_sets;
	}
	fclose(f); if (o) fclose(o);
	printf("sets %ld\n", n_sets);
	return 0;
}

static int run_fastx(const char *path, int64_t max_reads, int64_t max_bases, bool qual)
{
	mm355_fastx_t *fx = 0;
	int rc = qual? mm355_fastx_open_qual(path, &fx) : mm355_fastx_open(path, &fx);
	if (rc) { printf("rc %d\n", rc); return 0; }
	for (;;) {
		mm355_reads_t *r = 0;
		rc = mm355_fastx_next(fx, max_reads, max_bases, &r);
		if (rc || r == 0) break;
		const char *const *q = mm355_reads_quals(r);
		printf("batch %lld %d\n", (long long)r->n, q != 0);
		for (int64_t i = 0; i < r->n; ++i) {
			printf("rec %s %d %.*s ", r->names[i], r->lens[i], r->lens[i], r->seqs[i]);
			if (q && q[i]) printf("%.*s\n", r->lens[i], q[i]); else printf("-\n");
		}
		mm355_reads_free(r);
	}
	if (rc) { mm355_reads_t *r = 0; if (mm355_fastx_next(fx, max_reads, max_bases, &r) != rc || r) { printf("error not sticky\n"); return 1; } }
	mm355_fastx_close(fx);
	printf("rc %d\n", rc);
	return 0;
}

int main(int argc, char **argv)
{
	if (argc == 2 && !strcmp(argv[1], "comp")) return run_comp();
	if (argc == 4 && !strcmp(argv[1], "sets")) return run_sets(argv[2], argv[3], false);
	if (argc == 3 && !strcmp(argv[1], "check")) return run_sets(argv[2], 0, true);
	if (argc == 6 && !strcmp(argv[1], "fastx")) return run_fastx(argv[2], atoll(argv[3]), atoll(argv[4]), atoi(argv[5]) != 0);
	fprintf(stderr, "usage: sam_host comp | sets <in> <out> | check <in> | fastx <path> <max_reads> <max_bases> <qual>\n");
	return 64;
}
