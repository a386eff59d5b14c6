// mm355_dpplan.h -- the plan of ONE extension problem: which launch group (kernel) takes it and what it needs laid out (direction matrix,
// CIGAR scratch, HBM state, LDS).  Stated once: mm355_dp_run lays a round out from it, and the HBM budget of a round (mm355_dp_matrix_bytes,
// asked by run_dp_round in mm355_map.hip) is the same plan's byte count.  No HIP and no environment in here: the switches arrive as DpKnobs,
// and the CPU suite compiles this header with g++ (tests/host_harness/dpplan_host.cpp, tests/test_dp_plan_host.py).  The kernel headers take
// the limits the plan reads from here.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include "../../include/mm355.h"
#include "mm355_dpdomain.h"

// U:ksw2.h KSW_EZ_*
#define EZ_SCORE_ONLY  0x01
#define EZ_RIGHT       0x02
#define EZ_APPROX_MAX  0x08
#define EZ_APPROX_DROP 0x10
#define EZ_EXTZ_ONLY   0x40
#define EZ_REV_CIGAR   0x80

// ---- limits of the kernels (each explained beside its kernel)
#define ROW_NEG (-16384)            // mm355_dprow.h: below every real value of the int16 row sweep
#define ROW_TILE_ROWS 4             // direction bytes in tiles of 4 query rows x 16 target cells
#define ROW_MAX_T 1024              // k_ksw_row: eight register sets
#define ROW_MAX_QT 6000             // qlen + tlen: keeps every value inside int16
#define ROWL_MAX_T 8192             // k_ksw_rowl: ROWL_PANEL * ROWL_MAX_PANELS
#define ROWL_MAX_Q 5120             // ... and its LDS column buffers
#define BAND_MIN_MARGIN 8           // mm355_dpband.h
#define DP_WIN_MAX_W 832            // mm355_dpreg.h: the widest band k_ksw_regw's window follows
#define MW_SEQ_MAX 98304            // mm355_dpmw.h: query + target bytes k_ksw_regw8 stages in LDS (padded to 16 each)
// bytes of the tiled direction matrix of a qlen x tlen problem (T = tlen rounded up to 16; the matrix starts on a 64-byte boundary)
static inline size_t row_matrix_bytes(int qlen, int T) { return (size_t)((qlen + ROW_TILE_ROWS - 1) & ~(ROW_TILE_ROWS - 1)) * ((size_t)T + 16) + 64; }
static inline size_t band_matrix_bytes(int qlen, int W) { return (size_t)((qlen + ROW_TILE_ROWS - 1) & ~(ROW_TILE_ROWS - 1)) * (size_t)W + 64; }

struct DpConst {            // scoring constants after ksw_extd2_sse's (q,e)/(q2,e2) ordering
	int32_t q, e, q2, e2, qe_preswap;
	int8_t sc_mch, sc_mis, sc_N;
	int32_t long_thres, long_diff, valid;
	int32_t int8_ok;         // no int8 lane of ksw_extd2_sse wraps on a cell of the matrix (mm355_dpdomain.h): the row / band kernels' premise
};

static inline DpConst mm355_dp_const(const mm355_mapopt_t *mo)
{
	DpConst c;
	int q = mo->q, e = mo->e, q2 = mo->q2, e2 = mo->e2, t;
	int a = mo->a < 0? -mo->a : mo->a, b = mo->b > 0? -mo->b : mo->b, amb = mo->sc_ambi > 0? -mo->sc_ambi : mo->sc_ambi;
	c.qe_preswap = (int8_t)q + (int8_t)e;
	if (q2 + e2 < q + e) t = q, q = q2, q2 = t, t = e, e = e2, e2 = t;
	c.q = q; c.e = e; c.q2 = q2; c.e2 = e2;
	c.sc_mch = (int8_t)a; c.sc_mis = (int8_t)b; c.sc_N = amb == 0? (int8_t)(-e2) : (int8_t)amb;
	c.long_thres = e != e2? (q2 - q) / (e - e2) - 1 : 0;
	if (q2 + e2 + c.long_thres * e2 > q + e + c.long_thres * e) ++c.long_thres;
	c.long_diff = c.long_thres * (e - e2) - (q2 - q) - e2;
	int min_sc = b < amb? b : amb;
	c.valid = !(-min_sc > 2 * (q + e));
	c.int8_ok = mm355_dp_int8_domain(mo->a, mo->b, mo->sc_ambi, mo->q, mo->e, mo->q2, mo->e2);
	return c;
}

// Launch groups.  A problem's group names its kernel; the number is also its slot in mm355_stats_t::ms_dp_group / dp_cells_group /
// n_launch_group, which bench.py, _ffi.py and the tests index: the numbers are ABI.
// Size classes: targets up to 1024 bases run register-resident (k_ksw_reg, 2 * NP cells per lane), split by score tracking mode
// (KSW_EZ_APPROX_MAX or exact); longer ones keep their per-target state in LDS (12 B per position) or, beyond 12288 positions, in HBM, with
// eight waves per alignment.
enum {
	DP_G_REG = 0,       //  0..7   k_ksw_reg<1 | 2 | 4 | 8>: 2 * size class + exact
	DP_G_LDS = 8,       //  8..11  k_ksw_extd2<512>, state in LDS: targets <= 4096 (8 approx, 9 exact), <= 12288 (10, 11)
	DP_G_HBM = 12,      // 12, 13  ... state in HBM
	DP_G_ROW2 = 14,     // 14..16  k_ksw_row<2 | 4 | 8>: full-band approximate fills (mm355_dprow.h)
	DP_G_ROW4 = 15,
	DP_G_ROW8 = 16,
	DP_G_ROWL = 17,     // k_ksw_rowl: the same, targets 1025..8192
	DP_G_REGW = 18,     // k_ksw_regw8 / k_ksw_regw: exact, narrow band (w <= DP_WIN_MAX_W), targets > 1024 -- the register kernel with a moving window
	DP_G_BAND1 = 19,    // 19..21  k_ksw_band<1 | 2 | 4>: the row sweep on a band of 128 / 256 / 512 diagonals with a sufficiency proof (mm355_dpband.h)
	DP_G_BAND2 = 20,
	DP_G_BAND4 = 21,
	DP_G_BANDH = 22,    // k_ksw_band2: two problems per wave, 64 diagonals each
	DP_G_REDO = 23      // (not a class: the second, full-matrix run of band problems whose proof failed -- timer / counter slot)
};
#define DP_N_GROUP 23            // groups a problem can plan into
#define MM355_DP_GROUPS 24       // slots of the per-group statistics, events and counters
#define DP_N_CLASS 7
static const int DP_CLASS_CAP[DP_N_CLASS - 1] = { 128, 256, 512, 1024, 4096, 12288 };   // targets (rounded up to 16) a size class takes; the last class has no cap

struct DpKnobs {            // the A/B switches of the plan (mm355_dp.hip reads them from the environment, once per process)
	bool use_row = true;          // MM355_DP_ROW=0: anti-diagonal kernels only
	bool use_rowl = true;         // MM355_DP_ROWL=0: no eight-wave row sweep
	bool use_regw = true;         // MM355_DP_REGW=0: no windowed register kernel
	bool regw8 = true;            // MM355_DP_REGW8=0: its single-wave form (same results)
	bool use_band = true;         // MM355_DP_BAND=0: full-matrix kernels only
	double band_thr = 0.65;       // MM355_DP_BAND_THR: a band is tried when a score of thr x (all matches) would prove it
	double band_thr_half = 0.72;  // MM355_DP_BAND_THR_HALF: ... for the 64-diagonal band (0 = never)
	int band_force = 0;           // MM355_DP_BAND_FORCE (test hook): this many register sets (64: half a set) whenever the geometry allows
};

// value range of the row sweep on a qlen x tlen problem (int16 halves; ROW_NEG must stay below every real value, differences of two real
// values and the shifted prefix terms G + t e must not wrap)
static inline bool rowl_range_ok(const DpConst &dc, int qlen, int tlen)
{
	const int tl = (tlen + 127) & ~127;       // the lanes beyond the target compute cells of a wider matrix
	auto cost = [&](int k) { const int c1 = dc.q + k * dc.e, c2 = dc.q2 + k * dc.e2; return c1 < c2? c1 : c2; };
	const int emax = dc.e > dc.e2? dc.e : dc.e2;
	const int hi = dc.sc_mch * (qlen < tl? qlen : tl);
	int step = dc.q + dc.e > dc.q2 + dc.e2? dc.q + dc.e : dc.q2 + dc.e2;
	if (-dc.sc_mis > step) step = -dc.sc_mis;
	if (-dc.sc_N > step) step = -dc.sc_N;
	const int lo = cost(qlen + 1) + cost(tl + 1) + step + emax + 64;
	return hi + emax * (tl + 1) <= 32000 && lo <= -ROW_NEG - 64 && hi + lo <= 32000;
}

// which full-matrix row-sweep kernel takes a problem: 0 none (the anti-diagonal kernels), 1 k_ksw_row, 2 k_ksw_rowl
static inline int row_class(const DpConst &dc, const DpKnobs &kn, int qlen, int tlen, int w_in, int flag)
{
	const int w = w_in < 0? (qlen > tlen? qlen : tlen) : w_in;
	// ... only for a regular two-piece cost (after ksw2's ordering: e > e2, or two identical pieces).  Otherwise the boundary row and
	// column of U:ksw2_extd2_sse.c follow the dearer piece (long_thres <= 1), H(t,q) - H(t-1,q-1) can exceed the match score next to
	// them, the kernel's clamp `z = min(z, sc_mch)` becomes active and the result is no longer the plain recurrence the row sweep
	// computes (found by the option fuzzer: scoring=(4,10,3,3,12,3)); those options keep the literal anti-diagonal kernels.
	const bool regular = dc.e > dc.e2 || (dc.e == dc.e2 && dc.q == dc.q2);
	// ... and only inside the int8 domain of the SSE kernel (mm355_dpdomain.h): beyond it, e.g. a gap sum (q + e) + (q2 + e2) above 128
	// or a + q + 2e above 128, its lanes wrap on true cells and its result is no longer the plain recurrence either
	const bool row_kind = dc.valid && dc.int8_ok && kn.use_row && regular && (flag & EZ_APPROX_MAX) && !(flag & (EZ_APPROX_DROP | EZ_EXTZ_ONLY | EZ_SCORE_ONLY)) && w >= qlen + tlen;
	if (!row_kind) return 0;
	// (the int16 value range is checked per problem: a user scoring such as e2 >= 7 or a large match score would wrap the packed halves)
	if (tlen <= ROW_MAX_T) return qlen + tlen <= ROW_MAX_QT && rowl_range_ok(dc, qlen, tlen <= 256? 256 : tlen <= 512? 512 : 1024)? 1 : 0;
	return kn.use_rowl && tlen <= ROWL_MAX_T && qlen <= ROWL_MAX_Q && rowl_range_ok(dc, qlen, tlen)? 2 : 0;
}

// ---- band kernels (mm355_dpband.h): which problems take them, with which band
struct BandPlan { int nsb, dlo, lmin, bw; };   // nsb = 0: the full-matrix kernels; bw = 64 (two problems per wave, nsb = 1), 128, 256, 512
static inline int band_ubound(const DpConst &dc, int qlen, int tlen, int d)   // no path through diagonal d (outside [min(0, D0), max(0, D0)]) scores more
{
	const int D0 = tlen - qlen, g1 = d < 0? -d : d, g2 = D0 - d < 0? d - D0 : D0 - d;
	auto cost = [&](int g) { if (g <= 0) return 0; const int c1 = dc.q + g * dc.e, c2 = dc.q2 + g * dc.e2; return c1 < c2? c1 : c2; };
	int a = dc.sc_mch; if (dc.sc_mis > a) a = dc.sc_mis; if (dc.sc_N > a) a = dc.sc_N; if (a < 0) a = 0;
	int m = (qlen + tlen - g1 - g2) / 2; if (m < 0) m = 0;
	return a * m - cost(g1) - cost(g2);
}
static inline BandPlan band_plan(const DpConst &dc, const DpKnobs &kn, int qlen, int tlen, int full_sets)
{
	BandPlan bp; bp.nsb = 0; bp.dlo = 0; bp.lmin = 0; bp.bw = 0;
	const int force = kn.band_force;
	if (!kn.use_band) return bp;
	const int D0 = tlen - qlen, lo = D0 < 0? D0 : 0, hi = D0 > 0? D0 : 0, span = hi - lo + 1;
	const int emax = dc.e > dc.e2? dc.e : dc.e2;
	auto cost = [&](int g) { const int c1 = dc.q + g * dc.e, c2 = dc.q2 + g * dc.e2; return c1 < c2? c1 : c2; };
	int a = dc.sc_mch > 0? dc.sc_mch : 0;
	const int n = qlen < tlen? qlen : tlen;
	for (int nsb = 0; nsb <= 4; nsb = nsb? nsb * 2 : 1) {   // nsb = 0: half a register set (64 diagonals, k_ksw_band2)
		const int W = nsb? 128 * nsb : 64;
		if (force && (nsb? nsb : 64) != force) continue;
		if (nsb && nsb >= full_sets && !force) break;                   // no narrower than the full matrix
		if (W < span + 2 * BAND_MIN_MARGIN) continue;
		// int16 range: real values stay above -(cost(qlen + 1) + cost(tlen + 1)) - ..., the cells left of the border column start at ROW_NEG and
		// drift by at most a per row for W rows; prefix terms G + d e with |d| <= W + span
		if (cost(qlen + 1) + cost(tlen + 1) + 256 > 7000 || a * (W + 8) > 4000 || (W + span + 8) * emax > 4000 || a * n + (W + span + 8) * emax > 30000) continue;
		const int dlo = lo - (W - span) / 2;
		int u1 = band_ubound(dc, qlen, tlen, dlo - 1), u2 = band_ubound(dc, qlen, tlen, dlo + W);
		const int lmin = (u1 > u2? u1 : u2) + 1;
		if (!force && (double)lmin > (nsb? kn.band_thr : kn.band_thr_half) * (double)(a * n)) continue;   // not worth a try: only a nearly perfect alignment would prove this band
		bp.nsb = nsb? nsb : 1; bp.dlo = dlo; bp.lmin = lmin; bp.bw = W;
		return bp;
	}
	return bp;
}

struct DpPlan {
	int skip;             // tlen * qlen beyond max_sw_mat (mm_align_pair treats it as z-dropped), or a scoring ksw_extd2_sse refuses: not aligned
	int group;            // launch group; skipped and empty problems are counted into group 0 and ride in its list (its kernel writes their result)
	int pad;              // DpJobDev::pad: 0 the reference's anti-diagonal rows, 1 the row sweep's tiles, 2 the band's tiles
	int dlo, lmin, bw;    // band kernels: first diagonal, least end score that proves the band, width in diagonals
	bool line;            // the direction matrix starts on a 64-byte line (tiles are 64-byte lines)
	size_t bt_bytes;      // direction matrix
	size_t cig_words;     // CIGAR scratch of k_ksw_backtrack
	size_t st_words;      // per-target state in HBM (DP_G_HBM only)
	size_t regw_lds;      // LDS bytes of the two sequences in k_ksw_regw8 (DP_G_REGW only)
};

static inline DpPlan mm355_dp_plan(const DpConst &dc, const DpKnobs &kn, int64_t max_sw_mat, int qlen, int tlen, int w_in, int flag)
{
	DpPlan p = {};
	p.skip = (max_sw_mat > 0 && (int64_t)tlen * qlen > max_sw_mat) || !dc.valid;
	if (qlen <= 0 || tlen <= 0 || p.skip) return p;
	const int w = w_in < 0? (qlen > tlen? qlen : tlen) : w_in;
	const int T = (tlen + 15) / 16 * 16;
	p.cig_words = (size_t)qlen + tlen + 2;
	// gap fills whose band never binds, without z-drop on the approximate score: the row sweep (mm355_dprow.h), on a band where one can be proven
	if (const int rk = row_class(dc, kn, qlen, tlen, w_in, flag)) {
		const BandPlan bp = band_plan(dc, kn, qlen, tlen, rk == 2? 64 : tlen <= 256? 2 : tlen <= 512? 4 : 8);
		p.line = true;
		if (bp.nsb) {
			p.pad = 2; p.dlo = bp.dlo; p.lmin = bp.lmin; p.bw = bp.bw;
			p.bt_bytes = band_matrix_bytes(qlen, bp.bw);
			p.group = bp.bw == 64? DP_G_BANDH : bp.nsb == 1? DP_G_BAND1 : bp.nsb == 2? DP_G_BAND2 : DP_G_BAND4;
		} else {
			p.pad = 1;
			p.bt_bytes = row_matrix_bytes(qlen, T);
			p.group = rk == 2? DP_G_ROWL : tlen <= 256? DP_G_ROW2 : tlen <= 512? DP_G_ROW4 : DP_G_ROW8;
		}
		return p;
	}
	int n_col_ = qlen < tlen? qlen : tlen;
	n_col_ = ((n_col_ < w + 1? n_col_ : w + 1) + 15) / 16 + 1;
	p.bt_bytes = ((size_t)(qlen + tlen - 1) * n_col_ + 1) * 16;
	const size_t seq = (size_t)((qlen + 15) & ~15) + (size_t)T;
	if (kn.use_regw && T > ROW_MAX_T && !(flag & EZ_APPROX_MAX) && w <= DP_WIN_MAX_W && (!kn.regw8 || seq <= MW_SEQ_MAX)) {
		p.group = DP_G_REGW; p.regw_lds = seq;
		return p;
	}
	int cls = 0;
	while (cls < DP_N_CLASS - 1 && T > DP_CLASS_CAP[cls]) ++cls;
	if (cls == DP_N_CLASS - 1) p.st_words = (size_t)T;
	p.group = cls * 2 + ((flag & EZ_APPROX_MAX)? 0 : 1);
	return p;
}

// bytes mm355_dp_run sets aside for the direction matrix of one problem, the alignment of its first tile included: what the caller adds up
// to cut a round so that a launch fits its HBM budget
static inline size_t mm355_dp_plan_budget(const DpPlan &p) { return p.bt_bytes + (p.line? 64 : 0); }
