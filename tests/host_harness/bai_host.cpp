// bai_host.cpp -- the .bai index on the host as a stand-alone program (g++ alone, AddressSanitizer + UBSan; tests/test_bai_host.py).
// Every input array is a heap block of its exact size: a byte read past an end is a report.
//   span <in> <out>     cases written by the test -- int32 n and the n bytes of a record -- through bam_span_fits and, where it passes,
//                       bam_rec_span (mm355_bai.h): per case int32 fits and the int64 span (0 after a refusal)
//   build <in> <out>    cases -- int32 n_ref, int32 piece, int64 first_block_at, n_rec, n_calls; key[n_rec], span[n_rec], len[n_rec]; then per
//                       call int64 n and n bytes of BGZF blocks -- through BaiBuilder: the records in pieces of `piece`, each call's blocks,
//                       finish.  Per case int32 rc of the first step that refused, int64 chunks before and after the finishing merges, int64
//                       size and the index's bytes
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <memory>
#include <vector>
#include "../../mappy-rs_amd/csrc/mm355_bai.h"

static bool rd(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

static int run_span(FILE *f, FILE *o)
{
	long n_cases = 0;
	for (;; ++n_cases) {
		int32_t n;
		if (fread(&n, 4, 1, f) != 1) break;
		std::unique_ptr<uint8_t[]> rec(new uint8_t[(size_t)n]);
		if (!rd(f, rec.get(), (size_t)n)) return 3;
		const int32_t fits = bam_span_fits(rec.get(), n)? 1 : 0;
		const int64_t s = fits? bam_rec_span(rec.get(), n) : 0;
		fwrite(&fits, 4, 1, o); fwrite(&s, 8, 1, o);
	}
	printf("span %ld\n", n_cases);
	return 0;
}

static int run_build(FILE *f, FILE *o)
{
	long n_cases = 0;
	for (;; ++n_cases) {
		int32_t h4[2]; int64_t h8[3];
		if (fread(h4, 4, 2, f) != 2) break;
		if (fread(h8, 8, 3, f) != 3) return 3;
		const int64_t n_rec = h8[1], n_calls = h8[2], piece = h4[1] > 0? h4[1] : 1;
		std::unique_ptr<uint64_t[]> key(new uint64_t[(size_t)n_rec]);
		std::unique_ptr<int64_t[]> span(new int64_t[(size_t)n_rec]), len(new int64_t[(size_t)n_rec]);
		if (!rd(f, key.get(), (size_t)n_rec * 8) || !rd(f, span.get(), (size_t)n_rec * 8) || !rd(f, len.get(), (size_t)n_rec * 8)) return 3;
		BaiBuilder b;
		b.n_ref = h4[0]; b.first_block_at = h8[0];
		int32_t rc = 0;
		for (int64_t i = 0; i < n_rec && rc == 0; i += piece) {
			const int64_t k = n_rec - i < piece? n_rec - i : piece;
			// (a piece of its own exact size, so that a read past a piece is a report too)
			std::unique_ptr<uint64_t[]> pk(new uint64_t[(size_t)k]);
			std::unique_ptr<int64_t[]> ps(new int64_t[(size_t)k]), pl(new int64_t[(size_t)k]);
			memcpy(pk.get(), key.get() + i, (size_t)k * 8); memcpy(ps.get(), span.get() + i, (size_t)k * 8); memcpy(pl.get(), len.get() + i, (size_t)k * 8);
			rc = b.records(pk.get(), ps.get(), pl.get(), k);
		}
		for (int64_t c = 0; c < n_calls; ++c) {
			int64_t n;
			if (fread(&n, 8, 1, f) != 1) return 3;
			std::unique_ptr<char[]> bytes(new char[(size_t)n]);
			if (!rd(f, bytes.get(), (size_t)n)) return 3;
			if (rc == 0) rc = b.blocks(bytes.get(), n);
		}
		std::string out;
		if (rc == 0) rc = b.finish(out);
		if (rc) out.clear();
		const int64_t sz = (int64_t)out.size(), raw = rc? 0 : b.n_raw_chunks, fin = rc? 0 : b.n_chunks;
		fwrite(&rc, 4, 1, o); fwrite(&raw, 8, 1, o); fwrite(&fin, 8, 1, o); fwrite(&sz, 8, 1, o); fwrite(out.data(), 1, out.size(), o);
	}
	printf("build %ld\n", n_cases);
	return 0;
}

int main(int argc, char **argv)
{
	if (argc != 4) return 2;
	FILE *f = fopen(argv[2], "rb"), *o = fopen(argv[3], "wb");
	if (!f || !o) return 2;
	int rc = 2;
	if (!strcmp(argv[1], "span")) rc = run_span(f, o);
	else if (!strcmp(argv[1], "build")) rc = run_build(f, o);
	fclose(f); fclose(o);
	return rc;
}
