// mm355_ctx.cpp -- life cycle of a context: its streams and events, the per-device stream pools, its timers.  Host code only (no kernel):
// built like mm355_glue.cpp, and with g++ alone by tests/host_harness/ctx_life_host.cpp, which supplies the HIP entry points.
#include <stdio.h>
#include <stdlib.h>
#include <mutex>
#include "mm355_pipeline.h"

// ------------------------------------------------------------------ streams
// Streams of the extension rounds.  The runtime multiplexes the HIP streams of a priority level over GPU_MAX_HW_QUEUES hardware queues (8: set by
// mm355_runtime_init below, whatever the process inherited),
// handed out round-robin at stream creation; a kernel waits for everything in front of it on its QUEUE, whatever stream that came from.
// With eight extension streams per context (round 2) the long latency chains of one context (k_ksw_regw8 / k_ksw_rowl: a few dozen
// alignments for 10-20 ms) sat on the queue of another context's k_ksw_row<2> -- a kernel of the TURN, which every other context's round is
// waiting for (rocprofv3 trace of round 3: a turn kernel started 17 ms late behind such a chain; the turn kernels covered 56 % of the time).
// The rounds take turns anyway, so the classes need no stream per context: one pool of eight per device, each class on a queue of its own
//   0 row<2> + approximate targets <= 256    2 row<8> + approximate 1024    3 row<4> + approximate 512        (the turn)
//   1 exact register classes   4 eight-wave LDS kernel (all long targets)   6 k_ksw_rowl   5 / 7 k_ksw_regw8 (contexts alternate)
// Measured (round 3, default bench, alternating runs on one box): shared pool 853 / 795 Mbases/s against 876 / 865 with eight streams per
// context -- the exact classes and the long chains of different contexts then wait for one another on their one stream, which costs more
// than the occasional held turn.  Kept as an experiment switch (MM355_DP_SHARED_STREAMS=1); the default is a set of streams per context.
// Priority of an extension stream (experiment, off by default).  The runtime keeps a pool of hardware queues PER PRIORITY LEVEL: with the wide
// grids of the turn (classes 0, 2, 3) and the latency chains (1 exact register classes, 4 / 5 long targets, 6 k_ksw_rowl, 7 k_ksw_regw8) on
// one level, a turn kernel of one context sometimes sits on the hardware queue of another context's k_ksw_rowl / k_ksw_regw8 and starts when
// that chain ends, 6-19 ms late, with every other context's round waiting for the turn (rocprofv3 trace of the round-4 default bench: 12 such
// starts in 96 turns).  A level of their own for the chains (MM355_DP_PRIO3=1: chains normal, turn least; =2: turn normal, chains least)
// removes that -- and costs more than it saves: 1276 1279 1336 (=1) and 1320 1319 (=2) against 1380 1435 1428 / 1406 1422 Mbases/s with one
// level for every extension stream (alternating runs on one box): a third level is eight more hardware queues, and more than sixteen in
// use were slower in every sweep of the queue count as well (profiles/r04_knob_sweeps.txt; MM355_HW_QUEUES is the knob now).
int mm355_streams::dp_prio(int sidx) const
{
	static const int three = [] { const char *e = getenv("MM355_DP_PRIO3"); return e? atoi(e) : 0; }();   // 1: chains normal, turn least; 2: turn normal, chains least
	const bool chain = sidx == 1 || sidx >= 4;
	return three && (three == 1? chain : !chain) && prio_low - prio_high >= 2? (prio_low + prio_high) / 2 : prio_low;
}
static bool mm355_dp_shared_streams() { static const bool on = [] { const char *e = getenv("MM355_DP_SHARED_STREAMS"); return e && atoi(e) != 0; }(); return on; }

// What the contexts of one device share: the main + sort stream of up to eight of them, and the eight extension streams of
// MM355_DP_SHARED_STREAMS=1.  One object per device, indexed by the device id; everything here is read and written under g_streams_mu,
// which also makes the stream creations of a context one uninterrupted run.
struct DevicePool { hipStream_t front[16] = {}, dp[8] = {}; bool ready = false, dp_ready = false; uint8_t used = 0; };   // front: main stream of slot k at [k], its sort stream at [8 + k]
static std::vector<DevicePool> g_pools;
static std::mutex g_streams_mu;
static int g_n_ctx = 0;

static hipError_t make_stream(hipStream_t *s, unsigned flags, bool with_prio, int prio) { return with_prio? hipStreamCreateWithPriority(s, flags, prio) : hipStreamCreateWithFlags(s, flags); }
static void drop_streams(hipStream_t *s, int n) { for (int i = 0; i < n; ++i) if (s[i]) { (void)hipStreamDestroy(s[i]); s[i] = 0; } }
// the n streams of a pool in one go, make(i, &s[i]) in index order -- all of them or none: a partial failure destroys what it created
template <typename F> static hipError_t fill_pool(hipStream_t *s, int n, bool *ready, F make)
{
	if (*ready) return hipSuccess;
	hipError_t e = hipSuccess;
	for (int i = 0; i < n && e == hipSuccess; ++i) e = make(i, &s[i]);
	if (e != hipSuccess) drop_streams(s, n);
	*ready = e == hipSuccess;
	return e;
}

int mm355_streams::acquire(int device)
{
	int n = 0, lo = 0, hi = 0;
	if (hipGetDeviceCount(&n) != hipSuccess || n == 0 || device < 0 || device >= n) return MM355_ENODEV;
	HIPCHK(hipSetDevice(device));
	dev = device;
	// the per-read front kernels are latency chains of single waves: their stream outranks the extension streams, whose wide
	// grids would otherwise occupy every CU slot and stretch the front of the other contexts (MM355_STREAM_PRIO=0 disables)
	static const bool prio_on = [] { const char *e = getenv("MM355_STREAM_PRIO"); return !(e && atoi(e) == 0); }();
	HIPCHK(hipDeviceGetStreamPriorityRange(&lo, &hi));   // lo = least, hi = greatest (numerically lower)
	use_prio = prio_on && hi < lo; prio_low = use_prio? lo : 0; prio_high = use_prio? hi : 0;
	std::lock_guard<std::mutex> lk(g_streams_mu);
	if ((int)g_pools.size() < n) g_pools.resize(n);
	DevicePool &P = g_pools[dev];
	// The main and the sort stream of the first eight contexts of a device come from a pool that is created in one go -- eight main streams, then
	// eight sort streams: the runtime multiplexes the streams of a priority level over eight hardware queues, handed out in turn at stream
	// creation, and a kernel waits for everything in front of it on its QUEUE.  Created context by context (main, sort, main, sort ...) the main
	// streams of contexts i and i + 4 shared a queue, and so did their sort streams: the front of one context waited for the other's kernels.
	// From the pool, the two streams of a context share a queue with each other and with no other context (1401 against 1350 Mbases/s, six and
	// four alternating runs; MM355_STREAM_POOL=0: streams of its own for every context, as before).
	static const bool pool_on = [] { const char *e = getenv("MM355_STREAM_POOL"); return !(e && atoi(e) == 0); }();
	if (pool_on && use_prio) {
		HIPCHK(fill_pool(P.front, 16, &P.ready, [&](int i, hipStream_t *s) { return make_stream(s, i < 8? hipStreamDefault : hipStreamNonBlocking, true, hi); }));
		for (int k = 0; k < 8; ++k) if (!(P.used >> k & 1)) { P.used |= (uint8_t)(1u << k); pool_slot = k; st = P.front[k]; aux_st = P.front[8 + k]; break; }
	}
	if (st == 0) HIPCHK(make_stream(&st, hipStreamDefault, use_prio, hi));
	// The streams of the extension classes are created here, back to back under the lock: the runtime hands out hardware queues round-robin at
	// stream creation, and the classes of one context must not share a queue (MM355_DP_SHARED_STREAMS=1: the device's eight, made by its first context).
	ord = g_n_ctx++;
	if (!mm355_dp_shared_streams()) {
		// MM355_DP_QALIGN=1 (experiment): all eight extension streams at once, the four of the turn first (0, 2, 3 and the exact classes 1), then the
		// four chains (4 / 5 long targets, 6 k_ksw_rowl, 7 k_ksw_regw8) rotated by the context's ordinal: with eight queues handed out in turn, every
		// context's turn streams sit on queues 0-3 -- shared only with other contexts' turn streams, and turns exclude one another -- and a chain
		// of context j on queue 4 + (class + j) mod 4.
		static const bool qalign = [] { const char *e = getenv("MM355_DP_QALIGN"); return e && atoi(e) != 0; }();
		static const int turn_first[4] = { 0, 2, 3, 1 };
		for (int t = 0; t < (qalign? 8 : 6); ++t) {   // 0..3 the register classes, 4 and 5 the eight-wave kernel (mm355_dp_run): with the main and the sort stream, 8 per context
			const int i = !qalign? t : t < 4? turn_first[t] : 4 + ((t - ord) & 3);
			HIPCHK(make_stream(&dp_st[i], hipStreamNonBlocking, use_prio, dp_prio(i)));
		}
	} else {
		HIPCHK(fill_pool(P.dp, 8, &P.dp_ready, [&](int i, hipStream_t *s) { return make_stream(s, hipStreamNonBlocking, use_prio, dp_prio(i)); }));
		for (int i = 0; i < 8; ++i) dp_st[i] = P.dp[i];
		dp_shared = true;
	}
	// the stream of the block-level sort of anchor-rich reads: same consideration (7 streams per context, 8 hardware queues)
	if (aux_st == 0) HIPCHK(make_stream(&aux_st, hipStreamNonBlocking, use_prio, prio_high));
	HIPCHK(hipEventCreateWithFlags(&aux_ev, hipEventDisableTiming)); HIPCHK(hipEventCreateWithFlags(&aux_ev2, hipEventDisableTiming));
	HIPCHK(hipEventCreate(&ev0)); HIPCHK(hipEventCreate(&ev1));
	return 0;
}

void mm355_streams::release()
{
	if (!dp_shared) drop_streams(dp_st, 16);
	hipEvent_t *one[] = { &dp_up_ev, &aux_ev, &aux_ev2, &ev0, &ev1 };
	for (hipEvent_t *e : one) if (*e) { (void)hipEventDestroy(*e); *e = 0; }
	for (hipEvent_t *set : { dp_ev, dp_ev0, dp_ev1 }) for (int i = 0; i < MM355_DP_GROUPS; ++i) if (set[i]) { (void)hipEventDestroy(set[i]); set[i] = 0; }
	if (pool_slot < 0) { drop_streams(&aux_st, 1); drop_streams(&st, 1); }
	else { std::lock_guard<std::mutex> lk(g_streams_mu); g_pools[dev].used &= (uint8_t)~(1u << pool_slot); }   // (the streams stay with the device's pool)
	for (hipStream_t &s : dp_st) s = 0;
	st = aux_st = 0; pool_slot = -1; dp_shared = false;
}

int mm355_streams::dp_stream(int sidx, hipStream_t *out)
{
	if (dp_shared) {
		if (sidx == 5) sidx = 4;                         // one stream for every long-target launch
		if (sidx == 7 && (ord & 1)) sidx = 5;            // k_ksw_regw8: two streams, the contexts alternate
	} else if (dp_st[sidx] == 0) HIPCHK(make_stream(&dp_st[sidx], hipStreamNonBlocking, use_prio, dp_prio(sidx)));   // (6 and 7: on first use)
	*out = dp_st[sidx];
	return 0;
}

// ------------------------------------------------------------------ hardware queues
// The stream layout above is tuned for eight hardware queues per priority level (profiles/r04_knob_sweeps.txt: 1244 Mbases/s with 8, 1047 with
// 4, 921 with 16), and the runtime reads GPU_MAX_HW_QUEUES once, when it starts.  So the library sets it itself, before its first HIP call:
// MM355_HW_QUEUES (a number, clamped to 1..32) if given, else 8 -- over whatever the process inherited; a value that is no number counts as
// not given (atoi's 0 would mean ONE queue).  Every entry point that can be the first to reach the runtime calls this.  Where something else
// in the process started HIP earlier the call comes too late and changes nothing.  setenv() must not run beside another thread's getenv():
// the library's own threads (host pool, context threads) start after this call, and an embedder makes its first call into the library
// before it starts threads that read the environment.
void mm355_runtime_init(void)
{
	static std::once_flag once;
	std::call_once(once, [] {
		const char *seen = getenv("GPU_MAX_HW_QUEUES"), *want = getenv("MM355_HW_QUEUES");
		int q = 8;
		char *end = 0;
		const long w = want? strtol(want, &end, 10) : 0;
		const bool given = want && end != want && *end == 0;
		if (given) q = w < 1? 1 : w > 32? 32 : (int)w;
		char buf[16];
		snprintf(buf, sizeof(buf), "%d", q);
		if (getenv("MM355_VERBOSE")) fprintf(stderr, "[mm355] hardware queues: GPU_MAX_HW_QUEUES was %s, now %s (%s)\n", seen? seen : "not set", buf, given? "MM355_HW_QUEUES" : "the tuned default");
		setenv("GPU_MAX_HW_QUEUES", buf, 1);
	});
}

// ------------------------------------------------------------------ context
extern "C" int mm355_ctx_create(const mm355_index_t *mi, int device_id, mm355_ctx_t **out)
{
	mm355_runtime_init();
	*out = 0;
	if (mi == 0) return MM355_ENOIDX;
	mm355_ctx *c = new mm355_ctx();   // from here on every failure leaves through fail(): the destructor gives back whatever was acquired
	auto fail = [&](int rc) { mm355_ctx_destroy(c); return rc; };
	c->mi = mi;
	if (int rc = c->acquire(device_id)) return fail(rc);
	// the index replica of this device (shared by all its contexts; created on first use: H2D from the host image or a peer copy)
	mm355_replica rp;
	if (int rc = mm355_index_replica(mi, device_id, &rp)) return fail(rc);
	c->dix.slots = (const mm355_slot*)rp.slots; c->dix.line_mask = mi->n_lines - 1;
	c->dix.pos = (const uint64_t*)rp.pos; c->dix.S2 = (const uint32_t*)rp.S2; c->dix.nr = (const uint64_t*)rp.nr; c->dix.n_nr = rp.n_nr;
	c->dix.seq_off = (const uint64_t*)rp.seq_off; c->dix.seq_len = (const uint32_t*)rp.seq_len;
	c->dix.k = mi->k; c->dix.w = mi->w; c->dix.b = mi->b; c->dix.flag = mi->flag; c->dix.n_seq = mi->n_seq;
	c->d_name_rank = (const uint32_t*)rp.name_rank;
	if (c->counters.ensure(CTR_BYTES) || c->err.ensure(16)) return fail(MM355_ENOMEM);
	if (getenv("MM355_KPROF")) {
		if (c->kprof.ensure(512)) return fail(MM355_ENOMEM);
		if (hipMemset(c->kprof.p, 0, 512) != hipSuccess) return fail(MM355_EHIP);
	}
	mm355_stats_reset(c);
	*out = c;
	return 0;
}

extern "C" void mm355_ctx_destroy(mm355_ctx_t *c) { if (c) delete c; }

// ------------------------------------------------------------------ timers
void mm355_timers_resolve(mm355_ctx *c) { c->timers.resolve(); }

// per-kernel timer (mm355_dev.h): the pair comes from the book of EvTimer
void mm355_kt(void *kt, int slot, int end, hipStream_t st)
{
	mm355_ctx *c = (mm355_ctx*)kt;
	if (c == 0 || slot < 0 || slot >= KT_N || !c->timers_on) return;
	int &open = c->timers.kt_open[slot];
	if (!end) open = c->timers.begin(&c->stats.ms_kernel[slot], st) + 1;
	else if (open > 0) { c->timers.end(open - 1, st); open = 0; }
}
