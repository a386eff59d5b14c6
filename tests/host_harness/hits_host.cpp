// hits_host.cpp -- mappy-rs_amd/csrc/mm355_hits.h compiled with g++ alone: the assembler of mm355_hits_t behind a flat C interface
// (tests/test_hits_assemble_host.py feeds it hand-made spans and compares every array with a layout computed in numpy).
// -DHITS_HOST_MAIN: a stand-alone program over the same cases in small, for a run under -fsanitize=address,undefined.
#include <vector>
#include "../../mappy-rs_amd/csrc/mm355_hits.h"

// per read i: n[i] rows at hits[i] (and tags[i]), n_cigar[i] words at cigar[i], n_str[i] bytes at str[i]; tags may be null without want_tags
extern "C" int hits_assemble_host(int64_t n_reads, const int32_t *status, const int64_t *n, const mm355_hit_t *const *hits, const mm355_tags_t *const *tags,
                                  const int64_t *n_cigar, const uint32_t *const *cigar, const int64_t *n_str, const char *const *str, int want_tags,
                                  mm355_hits_t **out)
{
	std::vector<Mm355ReadRows> rows((size_t)n_reads);
	for (int64_t i = 0; i < n_reads; ++i) {
		Mm355ReadRows &w = rows[i];
		w.hits = hits[i]; w.tags = tags? tags[i] : 0; w.n = n[i];
		w.cigar = cigar[i]; w.n_cigar = n_cigar[i]; w.str = str[i]; w.n_str = n_str[i];
	}
	return mm355_hits_assemble(n_reads, status, rows.data(), want_tags != 0, out);
}

#ifdef HITS_HOST_MAIN
#include <stdio.h>
#define CHECK(x) do { if (!(x)) { fprintf(stderr, "hits_host: %s failed at line %d\n", #x, __LINE__); return 1; } } while (0)
int main()
{
	// a "device" buffer whose reads sit at non-contiguous hoff, and per-read vectors between them
	std::vector<mm355_hit_t> dev(16); std::vector<mm355_tags_t> dtag(16);
	for (int k = 0; k < 16; ++k) { memset(&dev[k], 0, sizeof(mm355_hit_t)); memset(&dtag[k], 0, sizeof(mm355_tags_t)); dev[k].NM = 100 + k; dev[k].cs_len = dev[k].md_len = -1; dtag[k].score = 200 + k; }
	std::vector<mm355_hit_t> v1(2), v2(1); std::vector<mm355_tags_t> t1(2), t2(1);
	memset(v1.data(), 0, 2 * sizeof(mm355_hit_t)); memset(v2.data(), 0, sizeof(mm355_hit_t)); memset(t1.data(), 0, 2 * sizeof(mm355_tags_t)); memset(t2.data(), 0, sizeof(mm355_tags_t));
	const uint32_t c1[5] = {0x10, 0x21, 0x30, 0x42, 0x50}, c2[2] = {0x60, 0x71};
	const char s1[] = ":5\0" "7A\0", s2[] = "\0";                 // v1[0]: cs ":5" + MD "7A"; v2[0]: an empty cs (length 0)
	v1[0].NM = 1; v1[0].n_cigar = 3; v1[0].cigar_off = 0; v1[0].cs_off = 0; v1[0].cs_len = 2; v1[0].md_off = 3; v1[0].md_len = 2;
	v1[1].NM = 2; v1[1].n_cigar = 2; v1[1].cigar_off = 3; v1[1].cs_off = 5; v1[1].cs_len = -1; v1[1].md_off = 0; v1[1].md_len = -1;
	v2[0].NM = 3; v2[0].n_cigar = 2; v2[0].cigar_off = 0; v2[0].cs_off = 0; v2[0].cs_len = 0; v2[0].md_off = 9; v2[0].md_len = -1;
	t1[0].score = 11; t1[1].score = 12; t2[0].score = 13;
	// reads: empty | dev[8..10) | v1 | empty | empty | dev[2..3) | v2 | empty
	const int32_t status[8] = {MM355_EEMPTY, 0, 0, 0, 0, 0, 0, 0};
	const int64_t n[8] = {0, 2, 2, 0, 0, 1, 1, 0}, nc[8] = {0, 0, 5, 0, 0, 0, 2, 0}, ns[8] = {0, 0, 6, 0, 0, 0, 1, 0};
	const mm355_hit_t *hp[8] = {0, &dev[8], v1.data(), 0, 0, &dev[2], v2.data(), 0};
	const mm355_tags_t *tp[8] = {0, &dtag[8], t1.data(), 0, 0, &dtag[2], t2.data(), 0};
	const uint32_t *cp[8] = {0, 0, c1, 0, 0, 0, c2, 0};
	const char *sp[8] = {0, 0, s1, 0, 0, 0, s2, 0};
	for (int want_tags = 0; want_tags < 2; ++want_tags) {
		mm355_hits_t *H = 0;
		CHECK(hits_assemble_host(8, status, n, hp, tp, nc, cp, ns, sp, want_tags, &H) == 0 && H);
		const int64_t off[9] = {0, 0, 2, 4, 4, 4, 5, 6, 6};
		CHECK(H->n_reads == 8 && H->n_hits == 6 && H->n_cigar == 7 && H->n_str == 7 && memcmp(H->hit_off, off, sizeof(off)) == 0);
		CHECK(H->status[0] == MM355_EEMPTY && H->status[7] == 0 && (H->tags != 0) == (want_tags != 0));
		const int nm[6] = {108, 109, 1, 2, 102, 3};
		for (int k = 0; k < 6; ++k) CHECK(H->hits[k].NM == nm[k]);
		CHECK(H->hits[2].cigar_off == 0 && H->hits[3].cigar_off == 3 && H->hits[5].cigar_off == 5 && H->cigar[5] == 0x60 && H->cigar[4] == 0x50);
		CHECK(H->hits[2].cs_off == 0 && H->hits[2].md_off == 3 && H->hits[3].cs_off == 5 && H->hits[3].md_off == 0);   // lengths of -1: offsets stay
		CHECK(H->hits[5].cs_off == 6 && H->hits[5].cs_len == 0 && H->hits[5].md_off == 9 && memcmp(H->str, ":5\0" "7A\0\0", 7) == 0);
		if (want_tags) CHECK(H->tags[0].score == 208 && H->tags[2].score == 11 && H->tags[4].score == 202 && H->tags[5].score == 13);
		mm355_free_hits(H);
	}
	{   // chain-only form: no CIGAR words, no strings, arenas of one element
		const int64_t z[8] = {0, 0, 0, 0, 0, 0, 0, 0}, n2[8] = {0, 2, 0, 0, 0, 1, 0, 0};
		const uint32_t *cz[8] = {0, 0, 0, 0, 0, 0, 0, 0}; const char *sz[8] = {0, 0, 0, 0, 0, 0, 0, 0};
		mm355_hits_t *H = 0;
		CHECK(hits_assemble_host(8, status, n2, hp, tp, z, cz, z, sz, 1, &H) == 0);
		CHECK(H->n_hits == 3 && H->n_cigar == 0 && H->n_str == 0 && H->cigar && H->str && H->tags && memcmp(&H->hits[2], &dev[2], sizeof(mm355_hit_t)) == 0);
		H->cigar[0] = 0; H->str[0] = 0;
		mm355_free_hits(H);
	}
	{   // no reads
		mm355_hits_t *H = 0;
		CHECK(hits_assemble_host(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, &H) == 0 && H->n_reads == 0 && H->n_hits == 0 && H->hit_off[0] == 0 && H->hits && !H->tags);
		mm355_free_hits(H);
	}
	mm355_free_hits(0);
	printf("hits_host ok\n");
	return 0;
}
#endif
