// deflate_host.cpp -- the host side of the BGZF deflate stage as a stand-alone program (g++ alone, AddressSanitizer + UBSan;
// tests/test_deflate_host.py):
//   wrap <level> <in> <out>  the file's bytes through the serial coder of mm355_deflate.h (level 1: mm355_bgzf_deflate_host) or the stored
//                            framing (level 0: mm355_bgzf_wrap_host); prints "blocks <n> stored <k> bytes <m>"
//   code <max_bits> <counts> the code dfl_make_code builds for the counts (symbol 0 first) after dfl_rank: one "<length> <code, first bit lowest>" line per symbol
//   syms                     dfl_len_sym of every length and dfl_dist_sym of every distance as "<symbol> <extra bits> <value>" lines: 256, then 32768
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../mappy-rs_amd/csrc/mm355_deflate.h"

static int run_wrap(int level, const char *in, const char *outp)
{
	FILE *f = fopen(in, "rb"), *o = fopen(outp, "wb");
	if (!f || !o) return 2;
	std::vector<char> v; char buf[1 << 16]; size_t k;
	while ((k = fread(buf, 1, sizeof(buf), f)) > 0) v.insert(v.end(), buf, buf + k);
	fclose(f);
	const std::vector<char> exact(v);                     // (a heap block of the input's size: a read past a payload's end is a report)
	const int64_t n = (int64_t)exact.size();
	int64_t n_out = 0, n_stored = bgzf_blocks(n);
	if (level == 0) {
		mm355_text_t *T = 0;
		if (mm355_bgzf_wrap_host(exact.empty()? 0 : exact.data(), n, &T)) return 3;
		n_out = T->n_text;
		fwrite(T->text, 1, (size_t)n_out, o);
		mm355_free_text_host(T);
	} else {
		std::vector<char> out((size_t)bgzf_size(n));      // (and one of the largest result's: a write past it is a report)
		n_out = n? mm355_bgzf_deflate_host(exact.data(), n, out.data(), &n_stored) : 0;
		if (n_out > bgzf_size(n)) return 4;
		if (n_out) fwrite(out.data(), 1, (size_t)n_out, o);
	}
	fclose(o);
	printf("blocks %lld stored %lld bytes %lld\n", (long long)bgzf_blocks(n), (long long)n_stored, (long long)n_out);
	return 0;
}

static int run_code(int max_bits, int n, char **counts)
{
	if (n < 1 || n > DFL_N_LL || max_bits < 1 || max_bits > 15) return 2;
	std::vector<uint32_t> f((size_t)n), a((size_t)n), cw((size_t)n);
	std::vector<uint16_t> sorted((size_t)n);
	for (int s = 0; s < n; ++s) f[(size_t)s] = (uint32_t)strtoul(counts[s], 0, 10);
	for (int s = 0; s < n; ++s) dfl_rank(f.data(), n, s, sorted.data());
	dfl_make_code(f.data(), n, max_bits, sorted.data(), a.data(), cw.data());
	for (int s = 0; s < n; ++s) printf("%u %u\n", cw[(size_t)s] >> 16, cw[(size_t)s] & 0xffff);
	return 0;
}

static int run_syms()
{
	uint32_t s, eb, ev;
	for (uint32_t l = 3; l <= DFL_MAX_MATCH; ++l) { dfl_len_sym(l, &s, &eb, &ev); printf("%u %u %u\n", s, eb, ev); }
	for (uint32_t d = 1; d <= DFL_MAX_DIST; ++d) { dfl_dist_sym(d, &s, &eb, &ev); printf("%u %u %u\n", s, eb, ev); }
	return 0;
}

int main(int argc, char **argv)
{
	if (argc == 5 && !strcmp(argv[1], "wrap")) return run_wrap(atoi(argv[2]), argv[3], argv[4]);
	if (argc >= 4 && !strcmp(argv[1], "code")) return run_code(atoi(argv[2]), argc - 3, argv + 3);
	if (argc == 2 && !strcmp(argv[1], "syms")) return run_syms();
	fprintf(stderr, "usage: deflate_host wrap <level> <in> <out> | code <max_bits> <count> ... | syms\n");
	return 64;
}
