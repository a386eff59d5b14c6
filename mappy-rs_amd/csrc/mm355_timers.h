// mm355_timers.h -- the book of a context's lazy timers: event pairs recorded around launches and turned into milliseconds later
#pragma once
#include <hip/hip_runtime.h>
#include <string.h>
#include <vector>
#include "mm355_dev.h"

// A pair is two events, begin and end, and the accumulator its milliseconds are added to.  begin() and end() only record: resolve() reads
// the pairs once the caller has synchronised its stream anyway.  Pair k keeps its two events from one call to the next; a resolve or a
// reset hands the slots out again from 0.
struct mm355_timer_book {
	enum { RESOLVE_AT = 120 };             // pending pairs at which begin() resolves first -- unless a pair is open: its end event must land in its own slot, so the book grows
	std::vector<hipEvent_t> ev;            // pair k: ev[2k] begin, ev[2k + 1] end
	std::vector<double*> acc;
	int n_pend = 0, n_open = 0;            // pairs handed out since the last resolve / reset; those of them whose end is not recorded yet
	int kt_open[KT_N] = {};                // open mm355_kt pair of a kernel slot: its pair index + 1
	mm355_timer_book() = default;
	mm355_timer_book(const mm355_timer_book&) = delete; mm355_timer_book &operator=(const mm355_timer_book&) = delete;
	~mm355_timer_book() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); }
	int begin(double *a, hipStream_t st)   // -> the pair, or -1 (no event to be had: not timed)
	{
		if (n_pend >= RESOLVE_AT && n_open == 0) resolve();
		const int k = n_pend;
		while ((int)ev.size() < 2 * (k + 1)) { hipEvent_t e = 0; if (hipEventCreate(&e) != hipSuccess) return -1; ev.push_back(e); }
		if ((int)acc.size() <= k) acc.resize(k + 1);
		acc[k] = a; ++n_pend; ++n_open;
		(void)hipEventRecord(ev[2 * k], st);
		return k;
	}
	void end(int k, hipStream_t st) { if (k < 0) return; (void)hipEventRecord(ev[2 * k + 1], st); --n_open; }
	// every pending pair into its accumulator.  For the points where no pair is open: with one left open (a call that failed between a begin
	// and its end) no slot can be told from a stale one, and all pending pairs are dropped
	void resolve()
	{
		for (int k = 0; k < n_pend && n_open == 0; ++k) {
			float ms = 0;
			if (hipEventSynchronize(ev[2 * k + 1]) == hipSuccess && hipEventElapsedTime(&ms, ev[2 * k], ev[2 * k + 1]) == hipSuccess) *acc[k] += ms;
		}
		reset();
	}
	void reset() { n_pend = n_open = 0; memset(kt_open, 0, sizeof(kt_open)); }   // drops the pending pairs
};
