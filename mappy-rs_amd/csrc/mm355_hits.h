// mm355_hits.h -- the one writer of a batch result (mm355_hits_t of include/mm355.h) and its release.  Both producers -- the CIGAR path
// of mm355_map_resident and the chain-only tail of mm355_regs.hip -- describe, per read, where the read's rows lie; the assembler lays
// them out in read order: hit_off / status, the hit rows (and the tags rows beside them), one CIGAR arena and one string arena.
// Plain C++ (tests/host_harness/hits_host.cpp compiles it with g++ alone).
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/mm355.h"

// The rows of one read: a span of the device's row buffer (k_regs) and a per-read vector of the host path are both just this.  tags is
// parallel to hits (read only when tags rows are asked for); a row's cigar_off counts from `cigar`, its cs_off / md_off from `str`.
struct Mm355ReadRows {
	const mm355_hit_t *hits = 0; const mm355_tags_t *tags = 0; int64_t n = 0;
	const uint32_t *cigar = 0; int64_t n_cigar = 0;
	const char *str = 0; int64_t n_str = 0;
};

extern "C" __attribute__((used)) inline void mm355_free_hits(mm355_hits_t *h)   // (used: exported although every call in here may be inlined)
{
	if (h == 0) return;
	free(h->hit_off); free(h->status); free(h->hits); free(h->cigar); free(h->str); free(h->tags); free(h);
}

// status: n_reads words.  Chain-only results are the same thing with no CIGAR words and no strings: n_cigar = n_str = 0 and arenas of one
// element.  tags stays null unless want_tags.
inline int mm355_hits_assemble(int64_t n_reads, const int32_t *status, const Mm355ReadRows *rows, bool want_tags, mm355_hits_t **out)
{
	*out = 0;
	int64_t nh = 0, nc = 0, ns = 0;
	for (int64_t i = 0; i < n_reads; ++i) { nh += rows[i].n; nc += rows[i].n_cigar; ns += rows[i].n_str; }
	mm355_hits_t *H = (mm355_hits_t*)calloc(1, sizeof(mm355_hits_t));
	if (H == 0) return MM355_ENOMEM;
	H->n_reads = n_reads; H->n_hits = nh; H->n_cigar = nc; H->n_str = ns;
	H->hit_off = (int64_t*)malloc((size_t)(n_reads + 1) * 8);
	H->status = (int32_t*)malloc((size_t)(n_reads > 0? n_reads : 1) * 4);
	H->hits = (mm355_hit_t*)malloc((size_t)(nh > 0? nh : 1) * sizeof(mm355_hit_t));
	H->cigar = (uint32_t*)malloc((size_t)(nc > 0? nc : 1) * 4);
	H->str = (char*)malloc((size_t)(ns > 0? ns : 1));
	if (want_tags) H->tags = (mm355_tags_t*)malloc((size_t)(nh > 0? nh : 1) * sizeof(mm355_tags_t));
	if (!H->hit_off || !H->status || !H->hits || !H->cigar || !H->str || (want_tags && !H->tags)) { mm355_free_hits(H); return MM355_ENOMEM; }
	nh = nc = ns = 0;
	for (int64_t i = 0; i < n_reads; ++i) {
		const Mm355ReadRows &r = rows[i];
		H->hit_off[i] = nh; H->status[i] = status[i];
		mm355_hit_t *h = H->hits + nh;
		if (r.n > 0) memcpy(h, r.hits, (size_t)r.n * sizeof(mm355_hit_t));
		if (r.n > 0 && want_tags) memcpy(H->tags + nh, r.tags, (size_t)r.n * sizeof(mm355_tags_t));
		for (int64_t k = 0; k < r.n && (nc || ns); ++k) {   // rebase into the batch's arenas
			h[k].cigar_off += nc;
			if (h[k].cs_len >= 0) h[k].cs_off += ns;
			if (h[k].md_len >= 0) h[k].md_off += ns;
		}
		if (r.n_cigar > 0) memcpy(H->cigar + nc, r.cigar, (size_t)r.n_cigar * 4);
		if (r.n_str > 0) memcpy(H->str + ns, r.str, (size_t)r.n_str);
		nh += r.n; nc += r.n_cigar; ns += r.n_str;
	}
	H->hit_off[n_reads] = nh;
	*out = H;
	return 0;
}
