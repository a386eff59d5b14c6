// mm355_extra.h -- descriptors shared by the host tail (mm355_glue.cpp) and k_extra / k_extra_long (mm355_dp.hip), the cut of a region into segments,
// and the carry rule of the cs string across the cuts as plain inline functions (the kernels call them; g++ compiles them for the host harness)
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#define MM355_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define MM355_HD static inline
#endif
// ---- row f2: U:align.c::mm_update_extra's per-base walk, U:format.c::write_cs_core and write_MD_core on the device (k_extra)
#define MM355_EXTRA_SEG 64          // CIGAR operations per segment (at most)
#define MM355_EXTRA_SEG_COLS 2048   // ... and columns per segment: a lane's walk is a chain of dependent loads.  A match operation longer than
                                    // that is CUT (HiFi: 500-base and longer matches); insertions and deletions stay whole (<= max_gap columns)
#define MM355_EXTRA_MIN_PIECE 256   // a match operation is not cut to fill less than this much of a segment
struct Mm355ExtraJob {      // one SEGMENT of an aligned region: one lane of k_extra
	int64_t q_src;          // offset of its first query base in the per-read code buffer (strand-adjusted, like DpGather::q_src)
	int64_t cig_off;        // first CIGAR operation in the uploaded array
	int64_t cs_off, md_off; // where its pieces of the cs / MD strings may be written (worst-case sized slots)
	uint32_t rid; int32_t t_st;   // first target base
	int32_t n_cigar, region;      // operations of the segment (the first and the last may be partial); index of the region it belongs to
	int32_t skip0, end_last;      // columns of the first operation that earlier segments walked; column where this segment leaves its last
	                              // operation (0 = at its end).  Only match operations are ever partial
};
// What a segment leaves.  Counts add up.  The score walk s <- max(0, s + d) is a max-plus transform: with A_i the sum of the first i score
// steps, s after step i is A_i + max(s_in, -m_i) (m_i = min of A_1..A_i), so A = A_n, m = m_n give s_out and C = max A_i, P = max (A_i - m_i)
// give the largest s inside the segment: max(s_in + C, P).  The strings: a run of matches may begin before the segment and end behind it, so
// the FIRST number a segment would print is left to the composer (lead = matches counted up to the first flush; the number printed there is
// the carry of the earlier segments + lead), and the matches pending at its end go on as the next segment's carry (tail); a segment that
// never flushes only adds to the carry.  cs flushes at a mismatch and at the end of every match operation (only a number > 0 is printed); MD
// flushes at a mismatch and at a deletion (the number is always printed) and carries its count across operations.
//
// The LONG form of cs (want bit 3, MM355_OUT_CS_LONG; write_cs_core with no_iden == 0) prints '=' and the run's query bases where the short form
// prints ':' and the run's length.  Its carry rule, stated by the inline functions at the end of this file (k_extra, k_extra_compose and
// k_extra_compact call them; g++ compiles them, so tests/host_harness/cslong_host.cpp replays the segments of a region serially):
//   * a segment writes every matched base into its slot as it meets it (mm355_cs_long_match): the bases of a run that began in an earlier segment
//     are written by their own segments, not by the one that flushes;
//   * a segment writes the '=' of every run that begins behind its first flush, never the '=' of its LEAD run (the matched bases before its
//     first flush, or all of them if it never flushes).  cs_pre is where the lead run's bases begin: behind the text of leading gaps;
//   * the composer decides that '=' (mm355_cs_compose): one byte at cs_pre iff no run is pending from the earlier segments of the region
//     (carry == 0) and lead > 0.  The carry goes on as in the short form: tail, or carry + lead for a segment that never flushed.  A run that
//     crosses any number of cuts so gets exactly one '=', a run that ends at a cut (mismatch on the last column before it: tail == 0) leaves
//     the next segment's lead its own;
//   * the compactor places [pre][=?][body] as it places [pre][:number][body] (mm355_cs_ins_bytes / mm355_cs_put_ins / mm355_cs_place).
// The slot of a segment (3 * cols + 12 * ops + 16 bytes, mm355_extra_split) holds the long form too: a mismatch column costs 3 bytes, a gap
// column 1 and its sign 1 per operation; a matched column costs 1 byte plus one '=' per run, and every run has at least one matched column, so
// a run of k columns costs at most k + 1 <= 2 k <= 3 k bytes (runs <= mismatches + operations, and each has a column of its own to pay for its
// '=').  The worst case is a segment of mismatches only, 3 bytes per column, as in the short form; the long form's fullest is alternating
// match / mismatch, 5 bytes per 2 columns.  The '=' the composer inserts is not in the slot: it goes straight into the dense string, whose
// size is the sum of the real lengths.  The harness asserts that no segment passes its slot.
struct Mm355ExtraSegOut {
	double A, m, C, P;
	int32_t mlen, blen, n_ambi;
	int32_t cs_len, cs_lead, cs_tail, md_len, md_lead, md_tail, flushed;   // *_len: body bytes in the slot; flushed: bit 0 cs, bit 1 MD
	int32_t cs_pre, n_gapo;        // cs bytes written BEFORE the first flush (the text of leading insertions / deletions): they stand in front of the number (long form: in front of the lead run's bases);
	                               // n_gapo: I / D operations of the segment (a gap is never cut, so the counts of the segments add up)
	int32_t cs_num, md_num;        // filled by k_extra_compose: the number in front of the body (-1: none; long cs: 0 = one '=', -1: none)
	int32_t n_gap, pad;            // summed lengths of those operations
	int64_t cs_dense, md_dense;    // ... and where [number][body] goes inside the region's string
};
struct Mm355ExtraOut { int32_t mlen, blen, n_ambi, dp_max; int64_t cs_dense; int32_t cs_len, md_len, md_end_num, n_gapo, n_gap, pad; };   // cs at cs_dense, MD right behind it;
                                                                                          // n_gapo / n_gap: number / summed lengths of the region's I and D operations
struct Mm355ExtraScore { int8_t mat[25]; int8_t q, e; };

// Cuts one region into segments (at most MM355_EXTRA_SEG operations and MM355_EXTRA_SEG_COLS columns; a longer match operation is cut,
// a longer gap gets a segment of its own).  segs == 0: count only.  Returns the number of segments; *cs_cap / *md_cap: bytes of string slots used
static inline int mm355_extra_split(const uint32_t *cg, int n, int64_t q_src, uint32_t rid, int64_t t_st, int64_t cig_off, int64_t cs_off, int64_t md_off, int32_t region,
                                    Mm355ExtraJob *segs, int64_t *cs_cap, int64_t *md_cap)
{
	int g = 0;
	int64_t qoff = 0, toff = 0, cso = 0, mdo = 0;
	int c = 0; int64_t done = 0;     // next operation and the columns of it already assigned
	while (c < n) {
		Mm355ExtraJob j;
		j.q_src = q_src + qoff; j.cig_off = cig_off + c; j.cs_off = cs_off + cso; j.md_off = md_off + mdo; j.rid = rid; j.t_st = (int32_t)(t_st + toff);
		j.region = region; j.skip0 = (int32_t)done; j.end_last = 0;
		int ops = 0; int64_t cols = 0;
		while (c < n && ops < MM355_EXTRA_SEG) {
			const uint32_t op = cg[c] & 0xf; const int64_t len = (int64_t)(cg[c] >> 4), rest = len - done;
			const bool is_m = op == 0 || op == 7 || op == 8;
			int64_t take = rest;
			if (cols + rest > MM355_EXTRA_SEG_COLS) {
				if (is_m) { take = MM355_EXTRA_SEG_COLS - cols; if (take < MM355_EXTRA_MIN_PIECE && ops > 0) break; if (take < MM355_EXTRA_MIN_PIECE) take = rest < MM355_EXTRA_SEG_COLS? rest : MM355_EXTRA_SEG_COLS; }
				else if (ops > 0) break;
			}
			++ops; cols += take;
			if (is_m) qoff += take, toff += take; else if (op == 1) qoff += take; else if (op == 2 || op == 3) toff += take;
			if (take < rest) { done += take; j.end_last = (int32_t)done; break; }
			done = 0; ++c;
		}
		j.n_cigar = ops;
		if (segs) segs[g] = j;
		++g;
		cso += 3 * cols + 12 * (int64_t)ops + 16; mdo += 2 * cols + 12 * (int64_t)ops + 16;
	}
	if (cs_cap) *cs_cap = (cso + 15) & ~(int64_t)15;
	if (md_cap) *md_cap = (mdo + 15) & ~(int64_t)15;
	return g;
}

// ---- the cs carry rule (both forms): what a segment leaves, what the composer inserts, where the compactor puts it
MM355_HD int mm355_ex_digits(unsigned v) { int n = 1; while (v >= 10) { v /= 10; ++n; } return n; }
MM355_HD int mm355_ex_put_num(char *dst, char lead, unsigned v)
{
	char bf[12]; int nb = 0, n = 0;
	do { bf[nb++] = (char)('0' + v % 10); v /= 10; } while (v);
	if (lead) dst[n++] = lead;
	while (nb > 0) dst[n++] = bf[--nb];
	return n;
}
// long form, a matched column inside a segment's walk (the caller counts it into `run` afterwards): the '=' of a run that begins behind the
// segment's first flush, then the base.  The lead run gets no '=' here
MM355_HD void mm355_cs_long_match(char *o, int32_t &n_out, unsigned run, int32_t flushed, uint32_t cq)
{
	if (run == 0 && (flushed & 1)) o[n_out++] = '=';
	o[n_out++] = "ACGTN"[cq];
}
// a flush (mismatch, end of a match operation): the first one of a segment closes its lead run and fixes cs_pre; a later one prints the short
// form's number (the long form has written the run already)
// (k_extra keeps the text of the <false> case in its own macro, so that the short form's registers are the ones it had; the harness holds the two equal)
template<bool LONG> MM355_HD void mm355_cs_flush(char *o, int32_t &n_out, unsigned &run, int32_t &flushed, int32_t &cs_lead, int32_t &cs_pre)
{
	if (!(flushed & 1)) { cs_lead = (int32_t)run; cs_pre = LONG? n_out - (int32_t)run : n_out; flushed |= 1; }
	else if (!LONG && run) n_out += mm355_ex_put_num(o + n_out, ':', run);
	run = 0;
}
// the end of a segment's walk.  A segment that never flushed only adds to the carry; in the long form its matched bases (all of them: its lead
// run) stand at the end of what it wrote, behind the text of its gaps
template<bool LONG> MM355_HD void mm355_cs_seg_close(int32_t n_out, unsigned run, int32_t flushed, int32_t lead_seen, int32_t pre_seen, int32_t *cs_lead, int32_t *cs_tail, int32_t *cs_pre)
{
	if (flushed & 1) { *cs_lead = lead_seen; *cs_tail = (int32_t)run; *cs_pre = pre_seen; }
	else { *cs_lead = (int32_t)run; *cs_tail = 0; *cs_pre = LONG? n_out - (int32_t)run : 0; }
}
// the composer, one segment: returns cs_num (what stands at cs_pre; -1: nothing) and moves the carry on
template<bool LONG> MM355_HD int32_t mm355_cs_compose(int32_t flushed, int32_t lead, int32_t tail, unsigned &carry)
{
	int32_t num = -1;
	if (LONG) { if (carry == 0 && lead > 0) num = 0; }
	else if (flushed & 1) { const unsigned nn = carry + (unsigned)lead; if (nn) num = (int32_t)nn; }
	if (flushed & 1) carry = (unsigned)tail; else carry += (unsigned)lead;
	return num;
}
template<bool LONG> MM355_HD int mm355_cs_ins_bytes(int32_t cs_num) { return cs_num < 0? 0 : LONG? 1 : 1 + mm355_ex_digits((unsigned)cs_num); }
template<bool LONG> MM355_HD void mm355_cs_put_ins(char *dst, int32_t cs_num) { if (cs_num < 0) return; if (LONG) dst[0] = '='; else mm355_ex_put_num(dst, ':', (unsigned)cs_num); }
// byte i of a segment's slot goes to dst[mm355_cs_place(i, cs_pre, inserted bytes)] of its piece of the region's string
MM355_HD int mm355_cs_place(int i, int cs_pre, int nn) { return i < cs_pre? i : nn + i; }
