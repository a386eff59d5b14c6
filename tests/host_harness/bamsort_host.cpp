// bamsort_host.cpp -- the coordinate order of BAM records on the host as a stand-alone program (g++ alone, AddressSanitizer + UBSan;
// tests/test_bamsort_host.py).  Every input array and every output buffer is a heap block of its exact size: a byte read or written past
// an end is a report.
//   key <in> <out>      cases written by the test -- int32 n and the n bytes of a record -- through bam_sort_key (mm355_bamsort.h): a uint64 each
//   sort <in> <out>     streams -- int64 n_rec, n_bytes, n_off, then n_off offsets and the n_bytes -- through bam_sort_check and, where it
//                       passes, bam_sort_host: per stream int32 rc, then key[n_rec], off[n_rec + 1] and the n_bytes sorted
//   gather <in> <out>   cases -- int64 base_len, out_cap, n, then src_off[n], len[n] and the base_len bytes -- through bam_gather: per case
//                       int32 rc, int64 total and the total bytes; after a refusal the output buffer must be untouched
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <memory>
#include <vector>
#include "../../mappy-rs_amd/csrc/mm355_bamsort.h"

static bool rd(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

static int run_key(FILE *f, FILE *o)
{
	long n_cases = 0;
	for (;; ++n_cases) {
		int32_t n;
		if (fread(&n, 4, 1, f) != 1) break;
		std::unique_ptr<uint8_t[]> rec(new uint8_t[(size_t)n]);
		if (!rd(f, rec.get(), (size_t)n)) return 3;
		const uint64_t k = bam_sort_key(rec.get());
		fwrite(&k, 8, 1, o);
	}
	printf("key %ld\n", n_cases);
	return 0;
}

static int run_sort(FILE *f, FILE *o)
{
	long n_cases = 0;
	for (;; ++n_cases) {
		int64_t hd[3];
		if (fread(hd, 8, 3, f) != 3) break;
		const int64_t n_rec = hd[0], n_bytes = hd[1], n_off = hd[2];
		std::unique_ptr<int64_t[]> off(new int64_t[(size_t)n_off]);
		std::unique_ptr<char[]> rec(new char[(size_t)(n_bytes > 0? n_bytes : 0)]);
		if (!rd(f, off.get(), (size_t)n_off * 8) || !rd(f, rec.get(), (size_t)(n_bytes > 0? n_bytes : 0))) return 3;
		const int32_t rc = bam_sort_check(rec.get(), n_bytes, off.get(), n_rec);
		fwrite(&rc, 4, 1, o);
		if (rc) continue;
		std::unique_ptr<uint64_t[]> key(new uint64_t[(size_t)n_rec]);
		std::unique_ptr<int64_t[]> noff(new int64_t[(size_t)n_rec + 1]);
		std::unique_ptr<char[]> out(new char[(size_t)n_bytes]);
		noff[0] = 0;
		if (n_rec) bam_sort_host(rec.get(), off.get(), n_rec, key.get(), noff.get(), out.get());
		fwrite(key.get(), 8, (size_t)n_rec, o); fwrite(noff.get(), 8, (size_t)n_rec + 1, o); fwrite(out.get(), 1, (size_t)n_bytes, o);
	}
	printf("sort %ld\n", n_cases);
	return 0;
}

static int run_gather(FILE *f, FILE *o)
{
	long n_cases = 0;
	for (;; ++n_cases) {
		int64_t hd[3];
		if (fread(hd, 8, 3, f) != 3) break;
		const int64_t base_len = hd[0], out_cap = hd[1], n = hd[2];
		std::unique_ptr<int64_t[]> src(new int64_t[(size_t)n]), len(new int64_t[(size_t)n]);
		std::unique_ptr<char[]> base(new char[(size_t)base_len]), out(new char[(size_t)(out_cap > 0? out_cap : 0)]);
		if (!rd(f, src.get(), (size_t)n * 8) || !rd(f, len.get(), (size_t)n * 8) || !rd(f, base.get(), (size_t)base_len)) return 3;
		if (out_cap > 0) memset(out.get(), 0x5a, (size_t)out_cap);
		const int32_t rc = bam_gather(base.get(), base_len, src.get(), len.get(), n, out.get(), out_cap);
		int64_t tot = 0;
		if (rc == 0) for (int64_t i = 0; i < n; ++i) tot += len[i];
		else for (int64_t i = 0; i < out_cap; ++i) if (out[(size_t)i] != 0x5a) return 4;      // a refusal has copied nothing
		fwrite(&rc, 4, 1, o); fwrite(&tot, 8, 1, o); fwrite(out.get(), 1, (size_t)tot, o);
	}
	printf("gather %ld\n", n_cases);
	return 0;
}

int main(int argc, char **argv)
{
	if (argc != 4) return 2;
	FILE *f = fopen(argv[2], "rb"), *o = fopen(argv[3], "wb");
	if (!f || !o) return 2;
	int rc = 2;
	if (!strcmp(argv[1], "key")) rc = run_key(f, o);
	else if (!strcmp(argv[1], "sort")) rc = run_sort(f, o);
	else if (!strcmp(argv[1], "gather")) rc = run_gather(f, o);
	fclose(f); fclose(o);
	return rc;
}
