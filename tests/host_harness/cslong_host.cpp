// The carry rule of the cs string across k_extra's segment cuts (mappy-rs_amd/csrc/mm355_extra.h), replayed serially on the CPU: mm355_extra_split,
// then for every segment in order the walk a lane makes (the string part of it, through the header's mm355_cs_long_match / mm355_cs_flush /
// mm355_cs_seg_close), then the composer (mm355_cs_compose) and the placement (mm355_cs_ins_bytes / mm355_cs_put_ins / mm355_cs_place) -- in
// both forms.  Every segment's slot is a heap block of exactly the size mm355_extra_split gives it, so AddressSanitizer sees a byte past it.
//
// usage: cslong_host FILE.  FILE: the number of regions, then per region a line "n_cigar q_len t_len", a line of CIGAR words (len << 4 | op), the
// query codes and the target codes as digit strings ("-" = empty).  Output per region, tab separated: the long form, the short form, the number
// of segments, a mask of the cases the region reached (below) and the fullest slot of the long form in per mille.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include <fstream>
#include <iostream>
#include "../../mappy-rs_amd/csrc/mm355_extra.h"

enum {
	CASE_NOFLUSH = 1,     // a segment with columns that never flushed (it only adds to the carry)
	CASE_MULTI = 2,       // ... entered with a run pending: the run crosses two cuts or more
	CASE_END_AT_CUT = 4,  // a later segment of a cut operation gets its own '=' (the run before ended at the cut)
	CASE_LEAD0 = 8,       // a run pending at a cut, and the first column behind the cut is a mismatch (lead 0)
	CASE_PRE = 16,        // the composer's byte stands behind text of leading gaps (cs_pre > 0)
	CASE_ALL_MISS = 32    // a piece of a cut operation that is all mismatches
};

#define DIE(...) do { fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); exit(2); } while (0)

struct Seg { Mm355ExtraSegOut o; std::vector<char> slot; int64_t cols; bool partial; };

// what one lane of k_extra / k_extra_long writes and leaves for the strings (the counts and the score walk are not the subject here)
template<bool LONG> static void walk(const Mm355ExtraJob &jb, const uint32_t *cig, const uint8_t *q, const uint8_t *t, Seg &s)
{
	const uint32_t *cg = cig + jb.cig_off;
	q += jb.q_src; t += jb.t_st;
	char *o = s.slot.data();
	int32_t n_out = 0, qoff = 0, toff = 0, cs_lead = 0, cs_pre = 0, flushed = 0;
	unsigned run = 0;
	const char *nt = "acgtn";
	for (int c = 0; c < jb.n_cigar; ++c) {
		const uint32_t op = cg[c] & 0xf, full = cg[c] >> 4;
		const uint32_t l0 = c == 0? (uint32_t)jb.skip0 : 0u, l1 = c == jb.n_cigar - 1 && jb.end_last > 0? (uint32_t)jb.end_last : full;
		const uint32_t len = l1 - l0;
		if (op == 0 || op == 7 || op == 8) {
			for (uint32_t l = 0; l < len; ++l) {
				const uint32_t cq = q[qoff + l], ct = t[toff + l];
				if (cq == ct) { if (LONG) mm355_cs_long_match(o, n_out, run, flushed, cq); ++run; }
				else { mm355_cs_flush<LONG>(o, n_out, run, flushed, cs_lead, cs_pre); o[n_out++] = '*'; o[n_out++] = nt[ct]; o[n_out++] = nt[cq]; }
			}
			if (l1 == full) mm355_cs_flush<LONG>(o, n_out, run, flushed, cs_lead, cs_pre);
			toff += (int32_t)len; qoff += (int32_t)len;
		} else if (op == 1) {
			o[n_out++] = '+';
			for (uint32_t l = 0; l < len; ++l) o[n_out++] = nt[q[qoff + l]];
			qoff += (int32_t)len;
		} else if (op == 2) {
			o[n_out++] = '-';
			for (uint32_t l = 0; l < len; ++l) o[n_out++] = nt[t[toff + l]];
			toff += (int32_t)len;
		} else if (op == 3) toff += (int32_t)len;
	}
	if ((size_t)n_out > s.slot.size()) DIE("a segment wrote %d bytes into a slot of %zu", n_out, s.slot.size());
	memset(&s.o, 0, sizeof(s.o));
	s.o.cs_len = n_out; s.o.flushed = flushed;
	mm355_cs_seg_close<LONG>(n_out, run, flushed, cs_lead, cs_pre, &s.o.cs_lead, &s.o.cs_tail, &s.o.cs_pre);
}

template<bool LONG> static std::string region(const std::vector<uint32_t> &cig, const std::vector<uint8_t> &q, const std::vector<uint8_t> &t, int *n_segs, int *cases, int *fill)
{
	const int n = (int)cig.size();
	const int ns = mm355_extra_split(cig.data(), n, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0);
	std::vector<Mm355ExtraJob> jobs((size_t)ns + 1);
	int64_t cs_cap = 0, md_cap = 0;
	if (mm355_extra_split(cig.data(), n, 0, 0, 0, 0, 0, 0, 0, jobs.data(), &cs_cap, &md_cap) != ns) DIE("the two passes of the split disagree");
	std::vector<Seg> segs((size_t)ns);
	int64_t q_seen = 0, t_seen = 0;
	for (int g = 0; g < ns; ++g) {
		const Mm355ExtraJob &jb = jobs[g];
		int64_t cols = 0; bool partial = false;
		if (jb.q_src != q_seen || jb.t_st != t_seen) DIE("segment %d starts at (%lld, %d), the segments before it end at (%lld, %lld)", g, (long long)jb.q_src, jb.t_st, (long long)q_seen, (long long)t_seen);
		for (int c = 0; c < jb.n_cigar; ++c) {
			const uint32_t w = cig[(size_t)jb.cig_off + c], op = w & 0xf, full = w >> 4;
			const uint32_t l0 = c == 0? (uint32_t)jb.skip0 : 0u, l1 = c == jb.n_cigar - 1 && jb.end_last > 0? (uint32_t)jb.end_last : full;
			cols += l1 - l0; partial |= l1 - l0 < full;
			if (op == 0 || op == 7 || op == 8) q_seen += l1 - l0, t_seen += l1 - l0; else if (op == 1) q_seen += l1 - l0; else if (op == 2 || op == 3) t_seen += l1 - l0;
		}
		const int64_t slot = 3 * cols + 12 * (int64_t)jb.n_cigar + 16;
		if (g + 1 < ns && jobs[g + 1].cs_off - jb.cs_off != slot) DIE("segment %d: a slot of %lld bytes, expected %lld", g, (long long)(jobs[g + 1].cs_off - jb.cs_off), (long long)slot);
		if (g + 1 == ns && (jb.cs_off + slot > cs_cap || cs_cap - (jb.cs_off + slot) > 15)) DIE("the last slot does not end at cs_cap");
		segs[g].slot.resize((size_t)slot); segs[g].cols = cols; segs[g].partial = partial;
		walk<LONG>(jb, cig.data(), q.data(), t.data(), segs[g]);
		if (LONG && cols > 0 && (int)(1000 * (int64_t)segs[g].o.cs_len / slot) > *fill) *fill = (int)(1000 * (int64_t)segs[g].o.cs_len / slot);
	}
	if (q_seen != (int64_t)q.size()) DIE("the segments cover %lld of %zu query bases", (long long)q_seen, q.size());
	// the composer: the segments of the region in order
	unsigned carry = 0; int64_t total = 0;
	for (int g = 0; g < ns; ++g) {
		Mm355ExtraSegOut &e = segs[g].o;
		if (LONG) {
			if (!(e.flushed & 1) && segs[g].cols > 0 && e.cs_lead > 0) *cases |= CASE_NOFLUSH | (carry > 0? CASE_MULTI : 0);
			if (g > 0 && jobs[g].skip0 > 0 && carry == 0 && e.cs_lead > 0) *cases |= CASE_END_AT_CUT;
			if (carry > 0 && (e.flushed & 1) && e.cs_lead == 0) *cases |= CASE_LEAD0;
			if (segs[g].partial && jobs[g].n_cigar == 1 && e.cs_len == 3 * segs[g].cols) *cases |= CASE_ALL_MISS;
		}
		e.cs_num = mm355_cs_compose<LONG>(e.flushed, e.cs_lead, e.cs_tail, carry);
		if (LONG && e.cs_num >= 0 && e.cs_pre > 0) *cases |= CASE_PRE;
		e.cs_dense = total;
		total += mm355_cs_ins_bytes<LONG>(e.cs_num) + e.cs_len;
	}
	// the placement: [pre][number or '='][body] of every segment
	std::string out((size_t)total, '\0');
	for (int g = 0; g < ns; ++g) {
		const Mm355ExtraSegOut &e = segs[g].o;
		char *dst = &out[0] + e.cs_dense;
		const int nn = mm355_cs_ins_bytes<LONG>(e.cs_num);
		mm355_cs_put_ins<LONG>(dst + e.cs_pre, e.cs_num);
		for (int i = 0; i < e.cs_len; ++i) dst[mm355_cs_place(i, e.cs_pre, nn)] = segs[g].slot[(size_t)i];
	}
	if (out.find('\0') != std::string::npos) DIE("a byte of the region's string was left unwritten");
	*n_segs = ns;
	return out;
}

static std::vector<uint8_t> codes(const std::string &s)
{
	std::vector<uint8_t> v;
	if (s == "-") return v;
	v.reserve(s.size() + 8);
	for (char ch : s) { if (ch < '0' || ch > '4') DIE("a code outside 0..4"); v.push_back((uint8_t)(ch - '0')); }
	return v;
}

int main(int argc, char **argv)
{
	if (argc != 2) DIE("usage: cslong_host FILE");
	std::ifstream in(argv[1]);
	if (!in) DIE("cannot read %s", argv[1]);
	long n_regions = 0;
	in >> n_regions;
	for (long r = 0; r < n_regions; ++r) {
		long n_cigar = 0, q_len = 0, tl = 0;
		in >> n_cigar >> q_len >> tl;
		std::vector<uint32_t> cig((size_t)n_cigar);
		for (long k = 0; k < n_cigar; ++k) in >> cig[(size_t)k];
		std::string qs, ts;
		in >> qs >> ts;
		if (!in) DIE("region %ld: short input", r);
		const std::vector<uint8_t> q = codes(qs), t = codes(ts);
		if ((long)q.size() != q_len || (long)t.size() != tl) DIE("region %ld: %zu / %zu codes, expected %ld / %ld", r, q.size(), t.size(), q_len, tl);
		int ns = 0, ns_short = 0, cases = 0, fill = 0, unused = 0;
		const std::string lg = region<true>(cig, q, t, &ns, &cases, &fill);
		const std::string sh = region<false>(cig, q, t, &ns_short, &unused, &unused);
		printf("%s\t%s\t%d\t%d\t%d\n", lg.c_str(), sh.c_str(), ns, cases, fill);
	}
	return 0;
}
