// paf_host.cpp -- the host side of the PAF writer as a stand-alone program (g++ alone, AddressSanitizer + UBSan; tests/test_paf_host.py):
//   f4                       paf_f4 against snprintf("%.4f") on grids, exact ties, denormals and random values; prints "f4 <checked> <wrong>"
//   ints                     paf_i64 / paf_u64 against snprintf; prints "ints <checked> <wrong>"
//   sets <in> <out>          result sets written by the test -> the host formatter's text and line_off per set; checks on every set that the
//                            counting sink equals the written length line by line and that line_off delimits whole lines
//   fastx <path> <max_reads> <max_bases>    the streaming reader: one "batch" line per mm355_fastx_next, one "rec" line per record, "rc <code>"
// The reader lives in mm355_index.cpp, which is compiled into this program; what that file calls on the device side is stubbed below.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include <random>
#include <string>
#include <vector>
#include "../../mappy-rs_amd/csrc/mm355_index.cpp"
#include "../../mappy-rs_amd/csrc/mm355_paf.h"

// ---- device-side entry points mm355_index.cpp refers to (never reached from here)
void mm355_runtime_init(void) {}
extern "C" int mm355_index_build_device(const mm355_idxopt_t *, int, const uint8_t *const *, const int64_t *, const char *const *, int, mm355_index_t **) { return MM355_ENODEV; }
int mm355_index_dump_buckets_device(const mm355_index *, FILE *) { return MM355_ENODEV; }
void mm355_index_free_replicas(mm355_index *) {}

struct StrSink { std::string s; void ch(char c) { s.push_back(c); } void bytes(const char *b, int64_t l) { s.append(b, (size_t)l); } void cigar(const uint32_t *, int64_t) {} };

static long g_checked = 0, g_wrong = 0;
static void f4_one(double x)
{
	char want[512];
	if (x == 0.0) strcpy(want, "0"); else snprintf(want, sizeof(want), "%.4f", x);
	StrSink s; paf_f4(s, x);
	PafCountSink c; paf_f4(c, x);
	++g_checked;
	if (s.s != want || c.n != (int64_t)s.s.size()) { if (++g_wrong <= 10) printf("f4 mismatch %a: got %s want %s\n", x, s.s.c_str(), want); }
}

static int run_f4()
{
	for (int k = 0; k <= 20000; ++k) { f4_one((double)k / 20000); f4_one((double)(float)((double)k / 20000)); f4_one((double)((float)k / 20000.0f)); }
	const double ties[] = { 1.0 / 32, 3.0 / 32, 5.0 / 32, 1.0 / 16, 0.0, 1.0, 4.9e-324, 1 - 630.0 / 653, 0.00005, 0.00015, 0.99995, 0.999949999, 2.2250738585072014e-308, 1e-30, 0.5 };
	for (double t : ties) f4_one(t);
	std::mt19937_64 rng(12345);
	std::uniform_real_distribution<float> U(0.0f, 1.0f);
	for (int i = 0; i < 1000000; ++i) f4_one((double)U(rng));
	for (int i = 0; i < 200000; ++i) {   // 1 - a / b, and float32 values next to a 5th-decimal midpoint
		const int64_t b = 1 + (int64_t)(rng() % 2000000), a = (int64_t)(rng() % (uint64_t)(b + 1));
		f4_one(1.0 - (double)a / (double)b);
		const float m = (float)((double)(rng() % 10000) / 10000 + 0.00005);
		f4_one((double)m); f4_one((double)nextafterf(m, 0.0f)); f4_one((double)nextafterf(m, 1.0f));
	}
	printf("f4 %ld %ld\n", g_checked, g_wrong);
	return g_wrong != 0;
}

static void int_one(int64_t v, bool as_unsigned)
{
	char want[64];
	if (as_unsigned) snprintf(want, sizeof(want), "%llu", (unsigned long long)v); else snprintf(want, sizeof(want), "%lld", (long long)v);
	StrSink s; PafCountSink c;
	if (as_unsigned) { paf_u64(s, (uint64_t)v); paf_u64(c, (uint64_t)v); } else { paf_i64(s, v); paf_i64(c, v); }
	++g_checked;
	if (s.s != want || c.n != (int64_t)s.s.size()) { if (++g_wrong <= 10) printf("int mismatch: got %s want %s\n", s.s.c_str(), want); }
}

static int run_ints()
{
	int64_t p = 1;
	int_one(0, false);
	for (int d = 0; d < 18; ++d, p *= 10) for (int64_t v : { p - 1, p, p + 1, 9 * p, -p, -(p - 1) }) { int_one(v, false); if (v >= 0) int_one(v, true); }
	for (int64_t v : { (int64_t)INT32_MAX, (int64_t)INT32_MIN, (int64_t)-1, (int64_t)UINT32_MAX, ((int64_t)1 << 28) - 1, (int64_t)1 << 32, INT64_MAX, INT64_MIN }) int_one(v, false);
	int_one((int64_t)UINT32_MAX, true); int_one(-1, true);   // 2^64 - 1
	for (uint32_t v : { 0u, 9u, 10u, 99u, 100u, 999999999u, 1000000000u, 4294967295u, (1u << 28) - 1 }) {
		char want[16]; snprintf(want, sizeof(want), "%u", v);
		++g_checked;
		if (paf_digits(v) != (int)strlen(want)) { ++g_wrong; printf("digits mismatch %u\n", v); }
	}
	printf("ints %ld %ld\n", g_checked, g_wrong);
	return g_wrong != 0;
}

// ---- result sets.  Per set, little-endian: int64 n_reads, n_hits, n_cigar, n_str, has_cigar, n_contigs, contig_bytes, qname_bytes; hit_off
// (n_reads + 1 int64), status, qlens (int32 each), has_name (n_reads bytes), hit rows, tags rows, CIGAR words, string arena, contig names and
// query names (each NUL-terminated, back to back; an unnamed read has no entry)
static bool rd(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

static int run_sets(const char *in, const char *outp)
{
	FILE *f = fopen(in, "rb"), *o = fopen(outp, "wb");
	if (!f || !o) return 2;
	long n_sets = 0;
	for (;;) {
		int64_t hd[8];
		if (fread(hd, 8, 8, f) != 8) break;
		const int64_t nr = hd[0], nh = hd[1], nc = hd[2], ns = hd[3];
		const bool has_cigar = hd[4] != 0;
		std::vector<int64_t> hit_off((size_t)nr + 1); std::vector<int32_t> status((size_t)nr), qlens((size_t)nr); std::vector<uint8_t> has_name((size_t)nr);
		// exact-size heap blocks: a read past the end of an arena is an AddressSanitizer report
		std::vector<mm355_hit_t> hits((size_t)nh); std::vector<mm355_tags_t> tags((size_t)nh); std::vector<uint32_t> cig((size_t)nc); std::vector<char> str((size_t)ns);
		std::vector<char> cb((size_t)hd[6]), qb((size_t)hd[7]);
		if (!rd(f, hit_off.data(), hit_off.size() * 8) || !rd(f, status.data(), (size_t)nr * 4) || !rd(f, qlens.data(), (size_t)nr * 4) || !rd(f, has_name.data(), (size_t)nr) ||
		    !rd(f, hits.data(), (size_t)nh * sizeof(mm355_hit_t)) || !rd(f, tags.data(), (size_t)nh * sizeof(mm355_tags_t)) || !rd(f, cig.data(), (size_t)nc * 4) ||
		    !rd(f, str.data(), (size_t)ns) || !rd(f, cb.data(), cb.size()) || !rd(f, qb.data(), qb.size())) return 3;
		std::vector<std::string> contigs;
		for (size_t a = 0; a < cb.size(); a += strlen(&cb[a]) + 1) contigs.emplace_back(&cb[a]);
		if ((int64_t)contigs.size() != hd[5]) return 4;
		std::vector<const char*> qn((size_t)nr, (const char*)0);
		size_t a = 0;
		for (int64_t i = 0; i < nr; ++i) if (has_name[i]) { qn[i] = &qb[a]; a += strlen(&qb[a]) + 1; }
		mm355_hits_t H; memset(&H, 0, sizeof(H));
		H.n_reads = nr; H.hit_off = hit_off.data(); H.status = status.data(); H.hits = hits.data(); H.cigar = cig.data(); H.str = str.data();
		H.n_hits = nh; H.n_cigar = nc; H.n_str = ns; H.tags = tags.data();
		static mm355_tags_t no_tags;
		if (nh == 0) H.tags = &no_tags;   // (an empty vector has no address, and a result without the tags array is refused)
		const PafNames nm = { contigs.data(), (uint32_t)contigs.size() };
		int rc = mm355_paf_check(&H, nm.n_seq, has_cigar);
		if (rc) { printf("set %ld: check %d\n", n_sets, rc); return 5; }
		mm355_text_t *T = 0;
		rc = mm355_paf_format_host(&H, qn.data(), qlens.data(), nm, has_cigar, &T);
		if (rc) { printf("set %ld: format %d\n", n_sets, rc); return 6; }
		// the counting sink against the written text, line by line; line_off against whole lines
		int64_t at = 0;
		for (int64_t i = 0; i < nr; ++i) {
			if (T->line_off[i] != at) { printf("set %ld: line_off[%lld]\n", n_sets, (long long)i); return 7; }
			for (int64_t k = hit_off[i]; k < hit_off[i + 1]; ++k) {
				PafCountSink c;
				paf_emit_line(c, mm355_paf_line_of(&H, k, qn[i], qlens[i], nm, has_cigar));
				const char *nl = (const char*)memchr(T->text + at, '\n', (size_t)(T->n_text - at));
				if (nl == 0 || nl - (T->text + at) + 1 != c.n) { printf("set %ld: hit %lld counts %lld\n", n_sets, (long long)k, (long long)c.n); return 8; }
				at += c.n;
			}
		}
		if (T->line_off[nr] != at || at != T->n_text || T->n_lines != nh || T->n_reads != nr) { printf("set %ld: totals\n", n_sets); return 9; }
		fwrite(&T->n_text, 8, 1, o); fwrite(T->line_off, 8, (size_t)nr + 1, o); fwrite(T->text, 1, (size_t)T->n_text, o);
		mm355_free_text_host(T);
		++n_sets;
	}
	fclose(f); fclose(o);
	printf("sets %ld\n", n_sets);
	return 0;
}

static int run_fastx(const char *path, int64_t max_reads, int64_t max_bases)
{
	mm355_fastx_t *fx = 0;
	int rc = mm355_fastx_open(path, &fx);
	if (rc) { printf("rc %d\n", rc); return 0; }
	for (;;) {
		mm355_reads_t *r = 0;
		rc = mm355_fastx_next(fx, max_reads, max_bases, &r);
		if (rc || r == 0) break;
		printf("batch %lld\n", (long long)r->n);
		for (int64_t i = 0; i < r->n; ++i) printf("rec %s %d %.*s\n", r->names[i], r->lens[i], r->lens[i], r->seqs[i]);
		mm355_reads_free(r);
	}
	if (rc) { mm355_reads_t *r = 0; if (mm355_fastx_next(fx, max_reads, max_bases, &r) != rc || r) { printf("error not sticky\n"); return 1; } }
	mm355_fastx_close(fx);
	printf("rc %d\n", rc);
	return 0;
}

int main(int argc, char **argv)
{
	if (argc >= 2 && !strcmp(argv[1], "f4")) return run_f4();
	if (argc >= 2 && !strcmp(argv[1], "ints")) return run_ints();
	if (argc == 4 && !strcmp(argv[1], "sets")) return run_sets(argv[2], argv[3]);
	if (argc == 5 && !strcmp(argv[1], "fastx")) return run_fastx(argv[2], atoll(argv[3]), atoll(argv[4]));
	fprintf(stderr, "usage: paf_host f4 | ints | sets <in> <out> | fastx <path> <max_reads> <max_bases>\n");
	return 64;
}
