// mm355_dpdomain.h -- the scorings for which U:ksw2_extd2_sse.c::ksw_extd2_sse's int8 lanes never wrap on a cell of the matrix.
// No HIP: mm355_dp.hip includes it (mm355_dp_const stores the answer in DpConst::int8_ok) and the CPU suite compiles it with g++
// (tests/host_harness/dp_domain_host.cpp, tests/test_ksw_domain_model.py).
//
// Why it matters.  The literal kernels (k_ksw_reg, k_ksw_regw, k_ksw_extd2) copy the SSE kernel's int8 difference recurrence and its
// wrap-around, whatever the scoring.  The row sweep and the band kernels (mm355_dprow.h, mm355_dpband.h) compute the TRUE two-piece affine
// recurrence in int16: they give the SSE kernel's result only where no int8 value of it wraps.  row_class sends a problem to them only
// inside this domain.
//
// The ranges.  Take the scoring after ksw2's ordering (q + e <= q2 + e2: the pieces are swapped otherwise), A = |a| the match score,
// m = min(-|b|, sc_N) the lowest substitution score, sc_N = sc_ambi == 0? -e2 : -|sc_ambi|, lo = min(-(q + e), long_diff) the lowest
// difference of two neighbouring cells (long_diff: the boundary's step where the second piece takes over).  On a cell that holds the true
// recurrence (every cell of the matrix when the band never binds) -- H(i,j) - H(i-1,j-1) <= A for a regular cost, H(i,j) >= H(i-1,j) - (q + e):
//     s, z           in [m, A]                           (z is also clamped to A)
//     u, v           in [lo, A - lo]                     (H(i,j) - H(i-1,j) = (H(i,j) - H(i-1,j-1)) + (H(i-1,j-1) - H(i-1,j)))
//     x, y           in [-(q + e), -e]                   x2, y2 in [-(q2 + e2), -e2]
//     x + v, y + u   in [lo - (q + e), A - lo - e]       x2 + v, y2 + u in [lo - (q2 + e2), A - lo - e2]
//     gate terms     (x + v) - z + q  in [lo - e - A, q]     (x2 + v) - z + q2 in [lo - e2 - A, q2]      (compared with 0: bits 0x08..0x40)
// plus the constants: sc_N, long_diff, -(q + e), -(q2 + e2) and q + e, q2 + e2 themselves (qe8, qe28).  The predicate asks all of these to
// lie in [-128, 127].  z - q and z - q2 may wrap: they only feed subtractions whose results are in range, exact modulo 256.  With lo = -(q + e)
// the binding conditions are (q + e) + (q2 + e2) <= 128 (x2 + v) and A + q + 2e <= 128 (the first gate term); A + q + e + e2 <= 128 (the second
// gate) and A + q + e <= 127 (u, v) follow from them when e >= e2 -- the regular costs, the only ones the row kernels take.
// The shipping presets sit well inside (asm5: gap sum 124, A + q + 2e = 46; map-ont: 31, 10).
#pragma once

static inline bool mm355_dp_i8(int x) { return x >= -128 && x <= 127; }

// a, b, sc_ambi, q, e, q2, e2 as the mapping options hold them (ksw_gen_simple_mat takes |a|, -|b|, -|sc_ambi|)
static inline bool mm355_dp_int8_domain(int a, int b, int sc_ambi, int q, int e, int q2, int e2)
{
	if (q < 0 || e < 0 || q2 < 0 || e2 < 0) return false;
	if (q2 + e2 < q + e) { int t = q; q = q2; q2 = t; t = e; e = e2; e2 = t; }   // ksw_extd2_sse: make sure q + e is no larger than q2 + e2
	const int A = a < 0? -a : a, mis = b > 0? -b : b, amb = sc_ambi > 0? -sc_ambi : sc_ambi;
	const int sc_N = amb == 0? -e2 : amb;
	const int m = mis < sc_N? mis : sc_N;
	int long_thres = e != e2? (q2 - q) / (e - e2) - 1 : 0;
	if (q2 + e2 + long_thres * e2 > q + e + long_thres * e) ++long_thres;
	const int long_diff = long_thres * (e - e2) - (q2 - q) - e2;
	const int qe = q + e, qe2 = q2 + e2;
	const int lo = long_diff < -qe? long_diff : -qe;
	const int hi = A - lo;
	return mm355_dp_i8(A) && mm355_dp_i8(m) && mm355_dp_i8(sc_N) && mm355_dp_i8(long_diff) && mm355_dp_i8(qe) && mm355_dp_i8(qe2) && mm355_dp_i8(-qe2)
	    && mm355_dp_i8(lo) && mm355_dp_i8(hi)                                  // u, v
	    && mm355_dp_i8(lo - qe) && mm355_dp_i8(hi - e)                         // x + v, y + u
	    && mm355_dp_i8(lo - qe2) && mm355_dp_i8(hi - e2)                       // x2 + v, y2 + u
	    && mm355_dp_i8(lo - e - A) && mm355_dp_i8(lo - e2 - A);                // the gate terms
}
