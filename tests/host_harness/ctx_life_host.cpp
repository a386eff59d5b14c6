// Life cycle of a context on the CPU: mappy-rs_amd/csrc/mm355_ctx.cpp and its headers compiled with g++ against the HIP entry points
// defined here.  The stubs count live objects per kind, remember the device that was current when a stream was made, log stream creations
// in order, stamp every event record with a sequence number (hipEventElapsedTime = the difference of two stamps) and can fail the N-th
// call from now.  One scenario per run (argv[1]): the statics of the code under test start fresh.  tests/test_ctx_lifecycle_host.py
// builds this with -fsanitize=address,undefined and runs it as a child process.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <set>
#include <string>
#include <utility>
#include <vector>
#include "../../mappy-rs_amd/csrc/mm355_pipeline.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "CHECK failed at %s:%d: %s\n", __FILE__, __LINE__, #x); exit(1); } } while (0)

// ------------------------------------------------------------------ the stubs
struct Stream { int dev; unsigned flags; bool has_prio; int prio; };
struct Event { long stamp = -1; int n_rec = 0; };
static std::set<void*> g_dev, g_pin;
static std::set<Stream*> g_streams;
static std::set<Event*> g_events;
static std::vector<Stream*> g_log;      // stream creations, in order
static int g_n_dev = 1, g_cur = 0, g_fail_in = 0;
static long g_calls = 0, g_stamp = 0, g_frees = 0;
static const int PRIO_LO = 0, PRIO_HI = -1;

static bool fails() { ++g_calls; return g_fail_in > 0 && --g_fail_in == 0; }   // every stub counts as a call
static void fail_nth(int n) { g_fail_in = n; }

static hipError_t new_block(std::set<void*> &live, void **p, size_t n)
{
	if (fails()) { *p = 0; return hipErrorOutOfMemory; }
	*p = malloc(n? n : 1); live.insert(*p);
	return hipSuccess;
}
static hipError_t free_block(std::set<void*> &live, void *p)
{
	if (fails()) return hipErrorUnknown;
	if (p == 0) return hipSuccess;
	CHECK(live.erase(p) == 1);   // a block is freed once, by the kind that made it
	free(p); ++g_frees;
	return hipSuccess;
}
static hipError_t new_stream(hipStream_t *s, unsigned flags, bool has_prio, int prio)
{
	if (fails()) { *s = 0; return hipErrorUnknown; }
	Stream *x = new Stream{ g_cur, flags, has_prio, prio };
	g_streams.insert(x); g_log.push_back(x);
	*s = (hipStream_t)x;
	return hipSuccess;
}
static hipError_t new_event(hipEvent_t *e)
{
	if (fails()) { *e = 0; return hipErrorUnknown; }
	Event *x = new Event(); g_events.insert(x); *e = (hipEvent_t)x;
	return hipSuccess;
}

hipError_t hipMalloc(void **p, size_t n) { return new_block(g_dev, p, n); }
hipError_t hipFree(void *p) { return free_block(g_dev, p); }
hipError_t hipHostMalloc(void **p, size_t n, unsigned int) { return new_block(g_pin, p, n); }
hipError_t hipHostFree(void *p) { return free_block(g_pin, p); }
hipError_t hipMemset(void *p, int v, size_t n) { if (fails()) return hipErrorUnknown; CHECK(g_dev.count(p)); memset(p, v, n); return hipSuccess; }
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned int flags) { return new_stream(s, flags, false, 0); }
hipError_t hipStreamCreateWithPriority(hipStream_t *s, unsigned int flags, int prio) { return new_stream(s, flags, true, prio); }
hipError_t hipStreamDestroy(hipStream_t s)
{
	if (fails()) return hipErrorUnknown;
	CHECK(g_streams.erase((Stream*)s) == 1);
	for (Stream *&x : g_log) if (x == (Stream*)s) x = 0;
	delete (Stream*)s;
	return hipSuccess;
}
hipError_t hipEventCreate(hipEvent_t *e) { return new_event(e); }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { return new_event(e); }
hipError_t hipEventDestroy(hipEvent_t e) { if (fails()) return hipErrorUnknown; CHECK(g_events.erase((Event*)e) == 1); delete (Event*)e; return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s)
{
	if (fails()) return hipErrorUnknown;
	CHECK(g_events.count((Event*)e) && g_streams.count((Stream*)s));
	((Event*)e)->stamp = g_stamp++; ++((Event*)e)->n_rec;
	return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t e) { if (fails()) return hipErrorUnknown; CHECK(g_events.count((Event*)e)); return hipSuccess; }
hipError_t hipEventElapsedTime(float *ms, hipEvent_t a, hipEvent_t b)
{
	if (fails()) return hipErrorUnknown;
	CHECK(g_events.count((Event*)a) && g_events.count((Event*)b));
	if (((Event*)a)->stamp < 0 || ((Event*)b)->stamp < 0) return hipErrorInvalidHandle;
	*ms = (float)(((Event*)b)->stamp - ((Event*)a)->stamp);
	return hipSuccess;
}
hipError_t hipSetDevice(int d) { if (fails() || d < 0 || d >= g_n_dev) return hipErrorInvalidDevice; g_cur = d; return hipSuccess; }
hipError_t hipGetDeviceCount(int *n) { if (fails()) return hipErrorUnknown; *n = g_n_dev; return hipSuccess; }
hipError_t hipDeviceGetStreamPriorityRange(int *lo, int *hi) { if (fails()) return hipErrorUnknown; *lo = PRIO_LO; *hi = PRIO_HI; return hipSuccess; }
const char *hipGetErrorString(hipError_t) { return "injected"; }
int mm355_index_replica(const mm355_index *, int dev, mm355_replica *out) { if (fails()) return MM355_EHIP; *out = mm355_replica(); out->dev = dev; return 0; }

// ------------------------------------------------------------------ helpers
struct Live { size_t dev, pin, events, streams; bool operator==(const Live &o) const { return dev == o.dev && pin == o.pin && events == o.events && streams == o.streams; } };
static Live live() { return Live{ g_dev.size(), g_pin.size(), g_events.size(), g_streams.size() }; }
static int streams_of(int dev) { int n = 0; for (Stream *s : g_streams) n += s->dev == dev; return n; }
static mm355_index g_mi;
static void make_index() { g_mi.b = 14; g_mi.w = 10; g_mi.k = 15; g_mi.flag = 0; g_mi.n_seq = 1; g_mi.n_lines = 1; g_mi.n_minimizers = g_mi.n_distinct = 0; }
static mm355_ctx *create(int dev) { mm355_ctx_t *c = 0; CHECK(mm355_ctx_create(&g_mi, dev, &c) == 0 && c != 0); return c; }
static bool is_stream(hipStream_t s, unsigned flags, int prio, int dev) { const Stream *x = (const Stream*)s; return g_streams.count((Stream*)s) && x->flags == flags && x->has_prio && x->prio == prio && x->dev == dev; }
// the device's pool as the log shows it from entry `at` on: eight main streams, then eight sort streams, of the greatest priority
static void check_pool_at(size_t at, int dev)
{
	CHECK(g_log.size() >= at + 16);
	for (int i = 0; i < 16; ++i) CHECK(is_stream((hipStream_t)g_log[at + i], i < 8? hipStreamDefault : hipStreamNonBlocking, PRIO_HI, dev));
}

// ------------------------------------------------------------------ scenarios
static void sc_cycle()
{
	const Live z = live();
	CHECK(z.dev == 0 && z.pin == 0 && z.events == 0 && z.streams == 0);
	mm355_ctx *c = create(0);
	CHECK(live().streams == 16 + 6 && c->pool_slot == 0);
	// what a mapping call does to it: working buffers, pinned staging, a parked batch, arenas, timers, the two late extension streams
	CHECK(c->seq.ensure(1000) == 0 && c->dp_bt.ensure(1 << 20) == 0 && c->h_res.ensure(100) == 0 && c->h_arena[3].ensure(64) == 0);
	c->slots.resize(2); CHECK(c->slots[1].roff.ensure(80) == 0);
	hipStream_t s6 = 0, s7 = 0; CHECK(c->dp_stream(6, &s6) == 0 && c->dp_stream(7, &s7) == 0 && s6 && s7 && s6 != s7);
	CHECK(hipEventCreate(&c->dp_up_ev) == hipSuccess && hipEventCreate(&c->dp_ev[23]) == hipSuccess && hipEventCreate(&c->dp_ev0[0]) == hipSuccess && hipEventCreate(&c->dp_ev1[5]) == hipSuccess);
	{ EvTimer t(c, &c->stats.ms_sort); mm355_kt(c, KT_CULL, 0, c->st); mm355_kt(c, KT_CULL, 1, c->st); }
	CHECK(live().streams == 16 + 8 && live().events == 4 + 4 + 4 && live().dev == 2 + 3 && live().pin == 2);
	mm355_ctx_destroy(c);
	const Live e = live();
	CHECK(e.dev == 0 && e.pin == 0 && e.events == 0 && e.streams == 16);   // the pool's streams stay with the device
	check_pool_at(0, 0);
	mm355_ctx_destroy(0);
}

// every call of a create fails once: nothing is left behind but a completed pool, and the next create is as good as the first
static void inject(int dev0, int *n_calls)
{
	long K = 0;   // the calls of a create that succeeds (its own: the destroy's are not among them)
	{ const long a = g_calls; mm355_ctx *c = create(dev0); K = g_calls - a; mm355_ctx_destroy(c); }
	CHECK(K >= 3 + 16 + 6 + 4 + 1 + 2);
	for (int N = 1; N <= K; ++N) {
		const int dev = dev0 + N;
		CHECK(dev < g_n_dev && streams_of(dev) == 0);
		const Live before = live();
		const size_t log0 = g_log.size();
		mm355_ctx_t *c = (mm355_ctx_t*)&g_mi;   // (anything but null)
		fail_nth(N);
		const int rc = mm355_ctx_create(&g_mi, dev, &c);
		CHECK(g_fail_in == 0);                  // the N-th call was reached
		CHECK(rc != 0 && c == 0);
		Live after = live();
		const int left = streams_of(dev);
		CHECK(left == 0 || left == 16);         // a pool is whole or absent
		if (left) { check_pool_at(log0, dev); after.streams -= 16; }
		CHECK(after == before);
		mm355_ctx *d = create(dev);
		CHECK(d->pool_slot == 0 && streams_of(dev) == 16 + 6);
		mm355_ctx_destroy(d);
		after = live(); after.streams -= 16;
		CHECK(after == before && streams_of(dev) == 16);
	}
	*n_calls = (int)K;
}
// the same for a ninth context, which owns its main and its sort stream
static void inject_ninth(int dev)
{
	mm355_ctx *c[8];
	for (int i = 0; i < 8; ++i) { c[i] = create(dev); CHECK(c[i]->pool_slot == i); }
	long K = 0;
	{ const long a = g_calls; mm355_ctx *n = create(dev); K = g_calls - a; CHECK(n->pool_slot == -1); mm355_ctx_destroy(n); }
	CHECK(K >= 3 + 1 + 6 + 1 + 4 + 1 + 2);
	for (int N = 1; N <= K; ++N) {
		const Live before = live();
		mm355_ctx_t *x = (mm355_ctx_t*)&g_mi;
		fail_nth(N);
		const int rc = mm355_ctx_create(&g_mi, dev, &x);
		CHECK(g_fail_in == 0 && rc != 0 && x == 0 && live() == before);
		mm355_ctx *n = create(dev);
		CHECK(n->pool_slot == -1 && live().streams == before.streams + 8);
		mm355_ctx_destroy(n);
		CHECK(live() == before);
	}
	for (int i = 0; i < 8; ++i) mm355_ctx_destroy(c[i]);
}
static void sc_inject()
{
	g_n_dev = 200;
	int k0 = 0, k1 = 0;
	inject(0, &k0);
	inject_ninth(90);
	CHECK(setenv("MM355_KPROF", "1", 1) == 0);   // one more buffer and a hipMemset
	inject(100, &k1);
	CHECK(k1 == k0 + 2);
	printf("calls of a create on a fresh device: %d, with MM355_KPROF: %d\n", k0, k1);
}

static void sc_devices()
{
	g_n_dev = 20;
	mm355_ctx_t *none = 0;
	CHECK(mm355_ctx_create(&g_mi, 20, &none) == MM355_ENODEV && none == 0 && mm355_ctx_create(&g_mi, -1, &none) == MM355_ENODEV && none == 0);
	CHECK(mm355_ctx_create(0, 0, &none) == MM355_ENOIDX && live().streams == 0);
	const int devs[3] = { 3, 16, 19 };
	mm355_ctx *c[3];
	for (int i = 0; i < 3; ++i) {
		c[i] = create(devs[i]);
		CHECK(g_cur == devs[i] && c[i]->dev == devs[i] && c[i]->pool_slot == 0);
		hipStream_t late = 0; CHECK(c[i]->dp_stream(6, &late) == 0);
		std::vector<hipStream_t> all = { c[i]->st, c[i]->aux_st, late };
		for (int k = 0; k < 6; ++k) all.push_back(c[i]->dp_st[k]);
		for (hipStream_t s : all) CHECK(s && g_streams.count((Stream*)s) && ((Stream*)s)->dev == devs[i]);
		CHECK(streams_of(devs[i]) == 16 + 7);
	}
	for (int i = 0; i < 3; ++i) for (int j = 0; j < i; ++j) CHECK(c[i]->st != c[j]->st && c[i]->aux_st != c[j]->aux_st);
	CHECK((int)live().streams == 3 * (16 + 7));   // no stream on any other device
	for (int i = 0; i < 3; ++i) mm355_ctx_destroy(c[i]);
	CHECK(live().streams == 3 * 16 && live().events == 0);
	// nine contexts on one device
	mm355_ctx *n[9];
	std::set<hipStream_t> seen;
	for (int i = 0; i < 9; ++i) {
		n[i] = create(5);
		CHECK(n[i]->pool_slot == (i < 8? i : -1) && n[i]->ord == 3 + i);
		CHECK(seen.insert(n[i]->st).second && seen.insert(n[i]->aux_st).second);
	}
	const size_t with_nine = live().streams;
	CHECK(with_nine == 3 * 16 + 16 + 9 * 6 + 2);
	mm355_ctx_destroy(n[8]);
	CHECK(live().streams == with_nine - 8);            // the ninth owned its two
	const hipStream_t st2 = n[2]->st, aux2 = n[2]->aux_st;
	mm355_ctx_destroy(n[2]);
	CHECK(live().streams == with_nine - 8 - 6);        // the third only its extension streams
	mm355_ctx *again = create(5);
	CHECK(again->pool_slot == 2 && again->st == st2 && again->aux_st == aux2);
	mm355_ctx *tenth = create(5);
	CHECK(tenth->pool_slot == -1);
	mm355_ctx_destroy(again); mm355_ctx_destroy(tenth);
	for (int i = 0; i < 8; ++i) if (i != 2) mm355_ctx_destroy(n[i]);
	CHECK(live().streams == 4 * 16 && live().events == 0 && live().dev == 0 && live().pin == 0);
}

// Stream creation order decides the hardware queue of a stream.  Fresh device: eight main streams, eight sort streams, then the extension
// streams of the first context; a later context of the pool: its extension streams alone; a ninth: main stream, extension streams, sort stream.
static void sc_order(bool qalign)
{
	static const int plain[6] = { 0, 1, 2, 3, 4, 5 };
	static const int q_even[8] = { 0, 2, 3, 1, 4, 5, 6, 7 }, q_odd[8] = { 0, 2, 3, 1, 7, 4, 5, 6 };   // MM355_DP_QALIGN=1: the turn first, the chains rotated by the ordinal
	const int nd = qalign? 8 : 6;
	g_n_dev = 2;
	auto dp_at = [&](const mm355_ctx *c, size_t at, const int *order) {
		for (int t = 0; t < nd; ++t) {
			CHECK(g_log.size() > at + t && g_log[at + t] == (Stream*)c->dp_st[order[t]]);
			CHECK(is_stream(c->dp_st[order[t]], hipStreamNonBlocking, PRIO_LO, c->dev));
		}
		for (int i = nd; i < 16; ++i) CHECK(c->dp_st[i] == 0);
	};
	mm355_ctx *c[9];
	c[0] = create(1);
	CHECK(g_log.size() == (size_t)16 + nd);
	check_pool_at(0, 1);
	CHECK(c[0]->st == (hipStream_t)g_log[0] && c[0]->aux_st == (hipStream_t)g_log[8] && c[0]->ord == 0);
	dp_at(c[0], 16, qalign? q_even : plain);
	c[1] = create(1);
	CHECK(g_log.size() == (size_t)16 + 2 * nd && c[1]->st == (hipStream_t)g_log[1] && c[1]->aux_st == (hipStream_t)g_log[9] && c[1]->ord == 1);
	dp_at(c[1], 16 + nd, qalign? q_odd : plain);
	for (int i = 2; i < 8; ++i) c[i] = create(1);
	const size_t at = g_log.size();
	CHECK(at == (size_t)16 + 8 * nd);
	c[8] = create(1);   // ordinal 8
	CHECK(g_log.size() == at + 1 + nd + 1 && c[8]->pool_slot == -1);
	CHECK(g_log[at] == (Stream*)c[8]->st && is_stream(c[8]->st, hipStreamDefault, PRIO_HI, 1));
	dp_at(c[8], at + 1, qalign? q_even : plain);
	CHECK(g_log[at + 1 + nd] == (Stream*)c[8]->aux_st && is_stream(c[8]->aux_st, hipStreamNonBlocking, PRIO_HI, 1));
	if (!qalign) {   // 6 and 7 on first use, once
		const size_t n0 = g_log.size();
		hipStream_t a = 0, b = 0, a2 = 0;
		CHECK(c[0]->dp_stream(7, &a) == 0 && g_log.size() == n0 + 1 && g_log[n0] == (Stream*)a && a == c[0]->dp_st[7] && c[0]->dp_st[6] == 0);
		CHECK(c[0]->dp_stream(6, &b) == 0 && g_log.size() == n0 + 2 && g_log[n0 + 1] == (Stream*)b && b == c[0]->dp_st[6]);
		CHECK(c[0]->dp_stream(7, &a2) == 0 && a2 == a && g_log.size() == n0 + 2);
		CHECK(is_stream(a, hipStreamNonBlocking, PRIO_LO, 1) && is_stream(b, hipStreamNonBlocking, PRIO_LO, 1));
	}
	for (int i = 0; i < 9; ++i) mm355_ctx_destroy(c[i]);
	CHECK(live().streams == 16 && live().events == 0);
}

// MM355_DP_SHARED_STREAMS=1: the extension streams are the device's, made once after the pool, and stay with it
static void sc_shared()
{
	g_n_dev = 18;
	mm355_ctx *a = create(17), *b = create(17);
	CHECK(g_log.size() == 16 + 8 && a->ord == 0 && b->ord == 1);
	check_pool_at(0, 17);
	for (int i = 0; i < 8; ++i) CHECK(a->dp_st[i] == (hipStream_t)g_log[16 + i] && b->dp_st[i] == a->dp_st[i] && is_stream(a->dp_st[i], hipStreamNonBlocking, PRIO_LO, 17));
	hipStream_t s = 0;
	CHECK(a->dp_stream(5, &s) == 0 && s == a->dp_st[4] && a->dp_stream(7, &s) == 0 && s == a->dp_st[7]);   // one stream for the long targets; k_ksw_regw8: the contexts alternate
	CHECK(b->dp_stream(7, &s) == 0 && s == b->dp_st[5] && b->dp_stream(2, &s) == 0 && s == b->dp_st[2]);
	mm355_ctx_destroy(a); mm355_ctx_destroy(b);
	CHECK(live().streams == 24 && live().events == 0);
	for (int N = 3 + 16 + 1; N <= 3 + 16 + 8; ++N) {   // a failure among the eight on a fresh device (three calls and the pool's sixteen come first): none of them stays
		const int dev = N - 20;
		mm355_ctx_t *c = 0;
		fail_nth(N);
		CHECK(mm355_ctx_create(&g_mi, dev, &c) != 0 && c == 0 && g_fail_in == 0 && streams_of(dev) == 16);
		mm355_ctx *d = create(dev);
		CHECK(d->pool_slot == 0 && streams_of(dev) == 24);
		mm355_ctx_destroy(d);
	}
}

static void sc_buffers()
{
	{   // a buffer that grows frees the old block
		DBuf d; HBuf h;
		CHECK(d.ensure(100) == 0 && h.ensure(100) == 0 && live().dev == 1 && live().pin == 1);
		void *p0 = d.p, *q0 = h.p; const size_t cap0 = d.cap;
		CHECK(d.ensure(cap0) == 0 && d.p == p0 && g_frees == 0);                          // (fits: nothing happens)
		CHECK(d.ensure(cap0 + 1) == 0 && h.ensure(1 << 20) == 0);
		CHECK(live().dev == 1 && live().pin == 1 && g_frees == 2 && !g_dev.count(p0) && !g_pin.count(q0));
		d.release(); CHECK(d.p == 0 && d.cap == 0 && live().dev == 0 && g_frees == 3);
		d.release(); CHECK(g_frees == 3);
	}
	CHECK(live().dev == 0 && live().pin == 0 && g_frees == 4);
	{   // a moved-from buffer frees nothing; assignment frees what the target held
		DBuf a, b; HBuf ha;
		CHECK(a.ensure(10) == 0 && b.ensure(20) == 0 && ha.ensure(10) == 0);
		void *pa = a.p, *pb = b.p; const size_t ca = a.cap, cb = b.cap;
		const long f0 = g_frees;
		{ DBuf m(std::move(a)); CHECK(a.p == 0 && a.cap == 0 && m.p == pa && m.cap == ca && g_frees == f0); a = std::move(m); CHECK(m.p == 0 && a.p == pa && g_frees == f0); }
		CHECK(g_frees == f0 && live().dev == 2);      // m died empty
		std::swap(a, b);
		CHECK(a.p == pb && a.cap == cb && b.p == pa && b.cap == ca && g_frees == f0 && live().dev == 2);
		a = std::move(b);
		CHECK(g_frees == f0 + 1 && !g_dev.count(pb) && a.p == pa && b.p == 0 && live().dev == 1);
		{ HBuf hm(std::move(ha)); CHECK(ha.p == 0 && live().pin == 1); }
		CHECK(live().pin == 0);
	}
	CHECK(live().dev == 0 && live().pin == 0);
	{   // parked batches: the vector grows through the moves
		std::vector<ResidentBatch> v(1);
		DBuf *b0[7] = { &v[0].seq, &v[0].roff, &v[0].rlen, &v[0].order, &v[0].ck_read, &v[0].ck_start, &v[0].ck_r0 };
		void *p[7];
		for (int i = 0; i < 7; ++i) { CHECK(b0[i]->ensure(100 + i) == 0); p[i] = b0[i]->p; }
		v[0].hb.seq.assign(5, 1); v[0].n_chunks = 9;
		const long f0 = g_frees;
		v.resize(40);
		CHECK(g_frees == f0 && live().dev == 7 && v[0].seq.p == p[0] && v[0].ck_r0.p == p[6] && v[0].hb.seq.size() == 5 && v[0].n_chunks == 9);
		CHECK(v[39].seq.ensure(64) == 0 && v[17].order.ensure(64) == 0 && live().dev == 9);
		ResidentBatch cur; CHECK(cur.seq.ensure(8) == 0);
		std::swap(cur.seq, v[39].seq); std::swap(cur.hb, v[0].hb);   // (mm355_batch_select)
		CHECK(live().dev == 10 && g_frees == f0);
	}
	CHECK(live().dev == 0 && live().pin == 0);
}

struct Kt { mm355_ctx *c; int slot; Kt(mm355_ctx *c_, int s) : c(c_), slot(s) { mm355_kt(c, slot, 0, c->st); } ~Kt() { mm355_kt(c, slot, 1, c->st); } };   // (KtScope of mm355_dev.h)
static void clear_records() { for (Event *e : g_events) e->n_rec = 0; }
static void once_at_most() { for (Event *e : g_events) CHECK(e->n_rec <= 1); }
static void sc_timers()
{
	hipStream_t st = 0; CHECK(hipStreamCreateWithFlags(&st, 0) == hipSuccess);
	{   // an open pair keeps its slot however many pairs begin and end inside it
		mm355_timer_book tb;
		double outer = 0; std::vector<double> in(300, 0.0);
		const long s0 = g_stamp;
		const int o = tb.begin(&outer, st);
		for (int i = 0; i < 300; ++i) { const int k = tb.begin(&in[i], st); CHECK(k == i + 1 && tb.n_open == 2); tb.end(k, st); }
		tb.end(o, st);
		CHECK(o == 0 && g_stamp == s0 + 602 && tb.n_open == 0 && tb.n_pend == 301 && tb.ev.size() == 602);
		once_at_most();
		tb.resolve();
		CHECK(outer == 601.0 && tb.n_pend == 0);        // its own begin to its own end
		for (double x : in) CHECK(x == 1.0);
		clear_records();
		// with no pair open the 121st begin resolves and takes slot 0 again
		std::vector<double> acc(121, 0.0);
		for (int i = 0; i < 120; ++i) { const int k = tb.begin(&acc[i], st); CHECK(k == i); tb.end(k, st); }
		once_at_most();
		CHECK(tb.n_pend == 120 && acc[0] == 0.0);
		const int k = tb.begin(&acc[120], st);
		CHECK(k == 0 && tb.n_pend == 1 && tb.n_open == 1 && tb.ev.size() == 602);
		for (int i = 0; i < 120; ++i) CHECK(acc[i] == 1.0);
		tb.end(k, st); tb.resolve();
		CHECK(acc[120] == 1.0 && acc[0] == 1.0);
		// reset drops what is pending
		double dropped = 0;
		tb.end(tb.begin(&dropped, st), st); tb.reset(); tb.resolve();
		CHECK(dropped == 0.0 && tb.n_pend == 0 && live().events == 602);
	}
	CHECK(live().events == 0);
	// the same through a context: a stage timer around 300 kernel timers
	mm355_ctx *c = create(0);
	const size_t ev0 = live().events;
	c->timers_on = false;
	{
		const long s0 = g_stamp;
		{ EvTimer t(c, &c->stats.ms_sort); Kt ks(c, KT_SKETCH); mm355_kt(c, KT_CULL, 0, c->st); mm355_kt(c, KT_CULL, 1, c->st); }
		CHECK(g_stamp == s0 && live().events == ev0 && c->timers.n_pend == 0);   // nothing created, nothing recorded
	}
	c->timers_on = true;
	clear_records();
	{
		EvTimer t(c, &c->stats.ms_sort);
		for (int i = 0; i < 300; ++i) { Kt ks(c, i & 1? KT_CULL : KT_ASORT); }
		{ Kt a(c, KT_LITERAL); Kt b(c, KT_LIT_MED); }   // (two kernel slots open at once)
	}
	once_at_most();
	mm355_timers_resolve(c);
	const mm355_stats_t &s = c->stats;
	CHECK(s.ms_sort == 605.0 && s.ms_kernel[KT_CULL] == 150.0 && s.ms_kernel[KT_ASORT] == 150.0 && s.ms_kernel[KT_LITERAL] == 3.0 && s.ms_kernel[KT_LIT_MED] == 1.0);
	CHECK(s.ms_kernel[KT_SKETCH] == 0.0 && c->timers.n_pend == 0);
	{ EvTimer t(c, &c->stats.ms_chain); }
	mm355_stats_reset(c);
	mm355_timers_resolve(c);
	CHECK(c->stats.ms_chain == 0.0 && c->stats.ms_sort == 0.0 && c->timers.n_pend == 0);
	mm355_ctx_destroy(c);
	CHECK(hipStreamDestroy(st) == hipSuccess && live().events == 0 && live().streams == 16);
}

int main(int argc, char **argv)
{
	const std::string sc = argc > 1? argv[1] : "";
	make_index();
	if (sc == "cycle") sc_cycle();
	else if (sc == "inject") sc_inject();
	else if (sc == "devices") sc_devices();
	else if (sc == "order") sc_order(getenv("MM355_DP_QALIGN") != 0);
	else if (sc == "shared") sc_shared();
	else if (sc == "buffers") sc_buffers();
	else if (sc == "timers") sc_timers();
	else { fprintf(stderr, "usage: %s cycle|inject|devices|order|shared|buffers|timers\n", argv[0]); return 2; }
	for (Stream *s : g_streams) delete s;   // (the pools' streams live as long as the process: every scenario has counted them)
	printf("ok %s\n", sc.c_str());
	return 0;
}
