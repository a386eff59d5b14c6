// mm355_names.h -- host preparation of the query-name rules of U:map.c (mm_map_frag's read hash, skip_seed's NO_DIAG / NO_DUAL branch).
// No string reaches a kernel: the distinct contig names are ranked once per index in strcmp order (unsigned bytes), a named read is
// reduced to three integers, and the device compares ranks:
//   strcmp(qname, contig) > 0   <=>  name_rank[rid] <  lb
//   strcmp(qname, contig) == 0  <=>  eq && name_rank[rid] == lb
// Plain C++ (tests/host_harness/names_host.cpp compiles it with g++ alone).
#pragma once
#include <stdint.h>
#include <string.h>
#include <string>
#include <vector>
#include <algorithm>

// U:map.c::mm_map_frag's hash of the query name (X31 over the bytes as C chars: a byte >= 0x80 is sign-extended, as `char` is on the
// platforms minimap2 is built for and as the oracle computes it)
inline uint32_t mm355_x31(const char *s)
{
	uint32_t h = (uint32_t)*s;
	if (h) for (++s; *s; ++s) h = (h << 5) - h + (uint32_t)*s;
	return h;
}

// strcmp order on whole strings (names hold no NUL)
inline int mm355_name_cmp(const char *a, size_t la, const char *b, size_t lb)
{
	const int c = memcmp(a, b, la < lb? la : lb);
	return c? c : la < lb? -1 : la > lb? 1 : 0;
}

// sorted = the distinct names in strcmp order; rank[rid] = index of names[rid] in it (equal names share a rank)
inline void mm355_name_ranks(const std::vector<std::string> &names, std::vector<std::string> &sorted, std::vector<uint32_t> &rank)
{
	auto lt = [](const std::string &a, const std::string &b) { return mm355_name_cmp(a.data(), a.size(), b.data(), b.size()) < 0; };
	sorted = names;
	std::sort(sorted.begin(), sorted.end(), lt);
	sorted.erase(std::unique(sorted.begin(), sorted.end()), sorted.end());
	rank.resize(names.size());
	for (size_t i = 0; i < names.size(); ++i) rank[i] = (uint32_t)(std::lower_bound(sorted.begin(), sorted.end(), names[i], lt) - sorted.begin());
}

// lb = number of distinct contig names < qname; eq = one of them equals qname (then it has rank lb)
inline void mm355_name_query(const std::vector<std::string> &sorted, const char *qname, uint32_t *lb, bool *eq)
{
	const size_t lq = strlen(qname);
	size_t lo = 0, hi = sorted.size();
	while (lo < hi) {
		const size_t mid = (lo + hi) >> 1;
		if (mm355_name_cmp(sorted[mid].data(), sorted[mid].size(), qname, lq) < 0) lo = mid + 1; else hi = mid;
	}
	*lb = (uint32_t)lo;
	*eq = lo < sorted.size() && mm355_name_cmp(sorted[lo].data(), sorted[lo].size(), qname, lq) == 0;
}

// the per-read word the named seed kernels read: lb | eq << 32 | named << 33 (0 = an unnamed read: the name rules do not apply to it)
#define MM355_NAME_EQ    (1ULL << 32)
#define MM355_NAME_NAMED (1ULL << 33)
inline uint64_t mm355_name_key(const std::vector<std::string> &sorted, const char *qname)
{
	if (qname == 0) return 0;
	uint32_t lb; bool eq;
	mm355_name_query(sorted, qname, &lb, &eq);
	return (uint64_t)lb | (eq? MM355_NAME_EQ : 0) | MM355_NAME_NAMED;
}

// skip_seed's name branch applies to a batch when a read has a name, MM_F_NO_DIAG (0x1) or MM_F_NO_DUAL (0x2) is set and the index kept
// its contig names (no MM_I_NO_NAME, index flag 4: then only the hash applies)
inline bool mm355_name_filter_applies(bool any_named, int64_t map_flag, int32_t idx_flag)
{
	return any_named && (map_flag & 3) != 0 && !(idx_flag & 4);
}
