// mm355_selfclamp.h -- U:align.c::mm_align1's clamp of the extension windows of a region whose first anchor carries MM_SEED_SELF (a named
// read against its own copy in the index, same strand, off the diagonal: MM_F_NO_DIAG).  Such a chain runs parallel to the diagonal at a
// distance of |qs - rs|; an end extension longer than that distance would reach the diagonal, where the trivial self-alignment beats
// everything.  rs / qs / re / qe: the region's chain coordinates; rs0 / qs0 / re0 / qe0: the extension limits, final except for this clamp.
// Written from recollection of minimap2 2.26: neither the oracle nor any fixture of this repository pins it.
// Plain C++ (tests/host_harness/selfclamp_host.cpp compiles it with g++ alone).
#pragma once
#include <stdint.h>

inline void mm355_self_clamp(int32_t rs, int32_t qs, int32_t re, int32_t qe, int32_t *rs0, int32_t *qs0, int32_t *re0, int32_t *qe0)
{
	int32_t max_ext = qs > rs? qs - rs : rs - qs;
	if (rs - *rs0 > max_ext) *rs0 = rs - max_ext;
	if (qs - *qs0 > max_ext) *qs0 = qs - max_ext;
	max_ext = qe > re? qe - re : re - qe;
	if (*re0 - re > max_ext) *re0 = re + max_ext;
	if (*qe0 - qe > max_ext) *qe0 = qe + max_ext;
}
