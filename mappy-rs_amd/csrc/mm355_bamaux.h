// mm355_bamaux.h -- the aux block of a BAM record, walked once: what the reader (mm355_bamread.h) and the Python surface run over aux bytes
// before the BAM writer copies them (the writer copies bytes as given: their well-formedness is decided here).  A block is tags back to
// back: two name bytes, a type byte, the value --
//   A c C    1 byte          s S    2 bytes          i I f    4 bytes          d    8 bytes (htslib reads it)
//   Z H      bytes up to a NUL that lies inside the block
//   B        a subtype out of cCsSiIf, a uint32 count, count x element size bytes (the product in 64 bits)
// and anything else is refused: an unknown type or subtype, a value or NUL past the end, a trailing partial tag.  The block is UNTRUSTED
// input: every length is compared with what is left of the block before a byte behind it is looked at.
// Plain C++ (tests/host_harness/bamaux_host.cpp builds it with g++ alone).
#pragma once
#include <stdint.h>
#include <string.h>
#include "../../include/mm355.h"

// the size of a value of scalar type t; 0: t is no scalar type
static inline int bam_aux_scalar(uint8_t t)
{
	switch (t) {
	case 'A': case 'c': case 'C': return 1;
	case 's': case 'S': return 2;
	case 'i': case 'I': case 'f': return 4;
	case 'd': return 8;
	default: return 0;
	}
}

// the length of the tag that begins at aux[at] (name, type and value), or -1: it does not fit into the n bytes or its type is unknown
static inline int64_t bam_aux_tag_len(const uint8_t *aux, int64_t n, int64_t at)
{
	const int64_t left = n - at;
	if (left < 3) return -1;
	const uint8_t t = aux[at + 2];
	if (const int w = bam_aux_scalar(t)) return left >= 3 + w? 3 + w : -1;
	if (t == 'Z' || t == 'H') {
		const void *nul = memchr(aux + at + 3, 0, (size_t)(left - 3));
		return nul? (const uint8_t*)nul - (aux + at) + 1 : -1;
	}
	if (t == 'B') {
		if (left < 8) return -1;
		const int w = aux[at + 3] == 'd'? 0 : bam_aux_scalar(aux[at + 3]);   // (no B:d, and A is no subtype)
		if (w == 0 || aux[at + 3] == 'A') return -1;
		const uint64_t count = (uint32_t)aux[at + 4] | (uint32_t)aux[at + 5] << 8 | (uint32_t)aux[at + 6] << 16 | (uint32_t)aux[at + 7] << 24;
		const uint64_t bytes = count * (uint64_t)w;                          // < 2^34
		return bytes <= (uint64_t)(left - 8)? 8 + (int64_t)bytes : -1;
	}
	return -1;
}

// the tags that index the bases of the read as sequenced: they are valid only on a record that holds the whole read
static inline bool bam_aux_is_mod(const uint8_t *t)
{
	return t[0] == 'M'? t[1] == 'M' || t[1] == 'L' || t[1] == 'N' || t[1] == 'm' || t[1] == 'l' : false;
}
// the tags the BAM writer emits itself (mm355_bam.h::bam_emit_record): a record must not hold a tag twice
static inline bool bam_aux_is_own(const uint8_t *t)
{
	static const char own[] = "NMmsASnntpcms1s2dedvzdSAcsMDrlCG";
	for (const char *o = own; *o; o += 2) if (t[0] == (uint8_t)o[0] && t[1] == (uint8_t)o[1]) return true;
	return false;
}
// keep: "*", or two-letter names back to back; 0 for anything else
static inline bool bam_aux_keep_ok(const char *keep)
{
	if (keep == 0) return false;
	const size_t l = strlen(keep);
	return (l == 1 && keep[0] == '*') || (l > 0 && l % 2 == 0);
}
static inline bool bam_aux_kept(const uint8_t *t, const char *keep)
{
	if (bam_aux_is_own(t)) return false;
	if (keep[0] == '*' && keep[1] == 0) return true;
	for (const char *k = keep; *k; k += 2) if (t[0] == (uint8_t)k[0] && t[1] == (uint8_t)k[1]) return true;
	return false;
}

// mm355_bam_aux_split (include/mm355.h): the library exports it from mm355_index.cpp
static inline int bam_aux_split(const uint8_t *aux, int32_t n, const char *keep, uint8_t *out, int32_t *n_out, int32_t *mod_off)
{
	if (n < 0 || (n > 0 && (aux == 0 || out == 0)) || n_out == 0 || mod_off == 0 || !bam_aux_keep_ok(keep)) return MM355_EINVAL;
	*n_out = *mod_off = 0;
	for (int64_t at = 0; at < n; ) {                       // the whole block is walked before a byte is written
		const int64_t l = bam_aux_tag_len(aux, n, at);
		if (l < 0) return MM355_EINVAL;
		at += l;
	}
	int32_t w = 0;
	for (int group = 0; group < 2; ++group) {
		if (group == 1) *mod_off = w;
		for (int64_t at = 0; at < n; ) {
			const int64_t l = bam_aux_tag_len(aux, n, at);
			if (bam_aux_kept(aux + at, keep) && (int)bam_aux_is_mod(aux + at) == group) { memcpy(out + w, aux + at, (size_t)l); w += (int32_t)l; }
			at += l;
		}
	}
	*n_out = w;
	return 0;
}
