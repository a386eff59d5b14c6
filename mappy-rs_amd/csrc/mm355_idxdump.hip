// mm355_idxdump.hip -- the bucket sections of an MMI\2 file from a device-resident index (mm355_index_build_device), for mm355_index_dump
// (replaces U:index.c::mm_idx_dump, the reference's fn_idx_out at lib.rs:391-394; layout and canonical order: include/mm355.h).
// The table (128-B lines, filled in CAS order) and pos[] (runs in ascending-minimizer order) exist only in HBM, so the conversion runs there:
//   1. k_compact        occupied slots -> (sort key, value); sort key = (bucket << (2k-b) | minimizer >> b) << 1 | singleton
//   2. rocprim radix sort on bits 1..2k of the key (keys are distinct, so the result does not depend on the order the table was filled in)
//   3. a scan of the multi-occurrence counts = every run's place in the new p[]; k_bucket_bounds = every bucket's slice of the pairs and of p[]
//   4. k_gather_runs / k_gather_long   pos[] -> the new p[];   k_file_pairs   (key, value) as the file holds them, start relative to the bucket
//   5. the pair array and p[] cross to the host in fixed-size pieces and are interleaved into the file bucket by bucket.
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <chrono>
#include <vector>
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include "mm355_pipeline.h"
#include "mm355_wave.h"

#define ID_BLOCK 256
#define ID_LONG_RUN 4096u          // runs above this are copied by whole blocks (k_gather_long), the rest by the wave that owns their key
#define ID_LONG_CHUNK 2048u        // positions one block copies per step of a long run
#define ID_PIECE (4u << 20)        // 8-byte words per device-to-host piece (32 MB)
#define ID_EXACT 1024             // DBuf::ensure headroom divisor: these buffers live for one call and never grow

// One wave per 256 consecutive slots (four coalesced 16-B loads per lane), one atomic per wave: the order of the output is whatever the
// atomics give, the sort that follows makes it irrelevant.
__global__ __launch_bounds__(ID_BLOCK) void k_compact(const mm355_slot *slots, uint64_t n_slots, int k, int b, uint64_t *keys, uint64_t *vals, uint64_t cap,
                                                       unsigned long long *n_out, int *err)
{
	const int lane = threadIdx.x & 63;
	const uint64_t n_tiles = (n_slots + 255) / 256;
	const uint64_t bmask = (1ULL << b) - 1;
	for (uint64_t tile = (uint64_t)blockIdx.x * (ID_BLOCK / 64) + (threadIdx.x >> 6); tile < n_tiles; tile += (uint64_t)gridDim.x * (ID_BLOCK / 64)) {
		mm355_slot s[4]; int before[4], total = 0;
		for (int j = 0; j < 4; ++j) {
			const uint64_t i = tile * 256 + (uint64_t)j * 64 + lane;
			s[j].key = ~0ULL; s[j].val = 0;
			if (i < n_slots) s[j] = slots[i];
			const unsigned long long m = __ballot(s[j].key != ~0ULL);
			before[j] = total + __popcll(m & LANE_LT_MASK(lane));
			total += __popcll(m);
		}
		if (total == 0) continue;   // (wave-uniform)
		unsigned long long base = 0;
		if (lane == 0) base = atomicAdd(n_out, (unsigned long long)total);
		base = __shfl(base, 0);
		if (base + total > cap) { if (lane == 0) *err = 1; continue; }   // more keys than the index counted: never write past the arrays
		for (int j = 0; j < 4; ++j) {
			if (s[j].key == ~0ULL) continue;
			const uint64_t minier = s[j].key >> 1;
			keys[base + before[j]] = ((minier & bmask) << (2 * k - b) | minier >> b) << 1 | (s[j].key & 1);
			vals[base + before[j]] = s[j].val;
		}
	}
}

__global__ __launch_bounds__(ID_BLOCK) void k_multi_counts(const uint64_t *keys, const uint64_t *vals, uint64_t n, uint64_t *cnt)
{
	const uint64_t i = (uint64_t)blockIdx.x * ID_BLOCK + threadIdx.x;
	if (i <= n) cnt[i] = i < n && !(keys[i] & 1)? (uint32_t)vals[i] : 0;   // (entry n: the scan's total)
}

// pair_off[bkt] = first sorted pair whose bucket is >= bkt (binary search: parallel whatever the ratio of buckets to keys);
// p_off[bkt] = where that bucket's runs begin in the new p[]
__global__ __launch_bounds__(ID_BLOCK) void k_bucket_bounds(const uint64_t *keys, uint64_t n, const uint64_t *moff, int shift, uint64_t n_buckets, uint64_t *pair_off, uint64_t *p_off)
{
	const uint64_t bkt = (uint64_t)blockIdx.x * ID_BLOCK + threadIdx.x;
	if (bkt > n_buckets) return;
	uint64_t lo = 0, hi = n;
	while (lo < hi) {
		const uint64_t mid = lo + ((hi - lo) >> 1);
		if ((keys[mid] >> shift) < bkt) lo = mid + 1; else hi = mid;
	}
	pair_off[bkt] = lo; p_off[bkt] = moff[lo];
}

// The runs of 64 consecutive keys, copied by the wave that owns them.  Run lengths are skewed (most are 2-3, a few 10^4-10^6), so neither a
// lane nor a wave per run: the wave flattens its runs (prefix sum of the 64 counts) and every lane copies ONE position per step, finding the
// run it belongs to by a binary search over the 64 prefix sums in LDS -- all lanes busy for any mix of lengths up to ID_LONG_RUN.  Longer
// runs are only listed here; k_gather_long spreads each of them over the whole grid.
__global__ __launch_bounds__(ID_BLOCK) void k_gather_runs(const uint64_t *keys, const uint64_t *vals, const uint64_t *moff, uint64_t n, const uint64_t *pos, uint64_t n_pos,
                                                           uint64_t *p_new, uint64_t *long_list, uint32_t long_cap, uint32_t *n_long, int *err)
{
	__shared__ uint32_t s_ex[ID_BLOCK / 64][64];
	__shared__ uint64_t s_src[ID_BLOCK / 64][64], s_dst[ID_BLOCK / 64][64];
	const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
	const uint64_t i = ((uint64_t)blockIdx.x * (ID_BLOCK / 64) + wv) * 64 + lane;
	uint32_t cnt = 0; uint64_t src = 0, dst = 0;
	if (i < n && !(keys[i] & 1)) {
		const uint64_t v = vals[i];
		cnt = (uint32_t)v; src = v >> 32; dst = moff[i];
		if (src + cnt > n_pos || dst + cnt > n_pos) { *err = 1; cnt = 0; }   // an inconsistent table: refuse, never read or write outside pos[]
		else if (cnt > ID_LONG_RUN) {
			const uint32_t q = atomicAdd(n_long, 1u);
			if (q < long_cap) long_list[q] = i; else *err = 1;
			cnt = 0;
		}
	}
	const uint32_t incl = (uint32_t)wave_incl_scan_add((int32_t)cnt);
	const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
	s_ex[wv][lane] = incl - cnt; s_src[wv][lane] = src; s_dst[wv][lane] = dst;
	__syncthreads();
	for (uint32_t t = lane; t < total; t += 64) {
		int lo = 0, hi = 63;   // the last key whose exclusive prefix is <= t (a key without positions shares its prefix with its successor)
		while (lo < hi) {
			const int mid = (lo + hi + 1) >> 1;
			if (s_ex[wv][mid] <= t) lo = mid; else hi = mid - 1;
		}
		const uint32_t o = t - s_ex[wv][lo];
		p_new[s_dst[wv][lo] + o] = pos[s_src[wv][lo] + o];
	}
}

// every block takes its share of ID_LONG_CHUNK-sized pieces of every listed run (the list is short: at most n_pos / ID_LONG_RUN runs)
__global__ __launch_bounds__(ID_BLOCK) void k_gather_long(const uint64_t *vals, const uint64_t *moff, const uint64_t *pos, uint64_t *p_new, const uint64_t *long_list,
                                                           const uint32_t *n_long, uint32_t long_cap)
{
	const uint32_t nl = *n_long < long_cap? *n_long : long_cap;
	for (uint32_t r = 0; r < nl; ++r) {
		const uint64_t i = long_list[r], v = vals[i];
		const uint32_t cnt = (uint32_t)v;   // (bounds against n_pos were checked when the run was listed)
		const uint64_t src = v >> 32, dst = moff[i];
		for (uint64_t c = (uint64_t)blockIdx.x * ID_LONG_CHUNK; c < cnt; c += (uint64_t)gridDim.x * ID_LONG_CHUNK) {
			const uint64_t e = c + ID_LONG_CHUNK < cnt? c + ID_LONG_CHUNK : cnt;
			for (uint64_t o = c + threadIdx.x; o < e; o += ID_BLOCK) p_new[dst + o] = pos[src + o];
		}
	}
}

// the pairs as the file holds them: key = minimizer>>b<<1 | singleton; a multi-occurrence value = start<<32 | count, start relative to its bucket
__global__ __launch_bounds__(ID_BLOCK) void k_file_pairs(const uint64_t *keys, const uint64_t *vals, const uint64_t *moff, const uint64_t *p_off, uint64_t n, int shift, uint64_t n_buckets,
                                                          mm128 *kv, int *err)
{
	const uint64_t i = (uint64_t)blockIdx.x * ID_BLOCK + threadIdx.x;
	if (i >= n) return;
	const uint64_t key = keys[i], bkt = key >> shift;   // (shift = 2k-b+1: below the bucket sit minimizer>>b and the singleton bit)
	if (bkt >= n_buckets) { *err = 1; return; }         // a minimizer of more than 2k bits: not a table of this index
	mm128 o;
	o.x = key & ((1ULL << shift) - 1);
	o.y = (key & 1)? vals[i] : ((moff[i] - p_off[bkt]) << 32 | (uint32_t)vals[i]);
	kv[i] = o;
}

// a device array read front to back through one fixed-size host buffer
struct DevFeed {
	const uint64_t *d; uint64_t n, fetched = 0; std::vector<uint64_t> h; size_t at = 0, have = 0; double *t_write;
	DevFeed(const void *d_, uint64_t n_, double *tw) : d((const uint64_t*)d_), n(n_), h(std::min<uint64_t>(n_, ID_PIECE)), t_write(tw) {}
	int write(uint64_t want, FILE *fp) {   // the next `want` words -> fp
		while (want) {
			if (at == have) {
				if (fetched >= n) return MM355_EHIP;   // (the bucket tables asked for more than the arrays hold)
				have = (size_t)std::min<uint64_t>(n - fetched, ID_PIECE); at = 0;
				if (hipMemcpy(h.data(), d + fetched, have * 8, hipMemcpyDeviceToHost) != hipSuccess) return MM355_EHIP;
				fetched += have;
			}
			const size_t m = (size_t)std::min<uint64_t>(want, have - at);
			const auto t0 = std::chrono::steady_clock::now();
			if (fwrite(h.data() + at, 8, m, fp) != m) return MM355_EIO;
			*t_write += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
			at += m; want -= m;
		}
		return 0;
	}
};

#define ID_GRID(n) dim3((unsigned)(((n) + ID_BLOCK - 1) / ID_BLOCK))

int mm355_index_dump_buckets_device(const mm355_index *mi, FILE *fp)
{
	if (!mi->dev_resident || mi->d_slots == 0) return MM355_EINVAL;
	mm355_runtime_init();
	const bool verbose = getenv("MM355_VERBOSE") != 0;
	const auto t_begin = std::chrono::steady_clock::now();
	auto since = [&]() { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count(); };
	int prev_dev = 0;
	(void)hipGetDevice(&prev_dev);
	HIPCHK(hipSetDevice(mi->dev_id));
	hipStream_t st; HIPCHK(hipStreamCreate(&st));
	const uint64_t n = (uint64_t)mi->n_distinct, n_pos = mi->n_pos, n_slots = mi->n_lines * MM355_SLOTS_PER_LINE, n_buckets = 1ULL << mi->b;
	const int shift = 2 * mi->k - mi->b + 1;
	const uint32_t long_cap = (uint32_t)(n_pos / ID_LONG_RUN + 1);
	// every temporary is a DBuf of this scope: freed at each return below
	DBuf d_keys, d_vals, d_keys2, d_vals2, d_tmp, d_moff, d_pair_off, d_p_off, d_p, d_kv, d_long, d_ctr;
	std::vector<uint64_t> pair_off, p_off;
	double t_write = 0, t_dev = 0;
	int rc = 0;
#define ID_FAIL(code) do { rc = (code); goto done; } while (0)
	{
		if (d_keys.ensure((n + 1) * 8, ID_EXACT) || d_vals.ensure((n + 1) * 8, ID_EXACT) || d_keys2.ensure((n + 1) * 8, ID_EXACT) || d_vals2.ensure((n + 1) * 8, ID_EXACT) || d_ctr.ensure(64, ID_EXACT)) ID_FAIL(MM355_ENOMEM);
		unsigned long long *c_n = d_ctr.as<unsigned long long>(); uint32_t *c_long = d_ctr.as<uint32_t>() + 4; int *c_err = d_ctr.as<int>() + 8;
		if (hipMemsetAsync(d_ctr.p, 0, 64, st) != hipSuccess) ID_FAIL(MM355_EHIP);
		// 1. compact (n_slots >= 8: the grid is never empty; capped, the kernel strides)
		const uint64_t n_wave_tiles = (n_slots + 255) / 256;
		hipLaunchKernelGGL(k_compact, dim3((unsigned)std::min<uint64_t>((n_wave_tiles + 3) / 4, 8192)), dim3(ID_BLOCK), 0, st, (const mm355_slot*)mi->d_slots, n_slots, mi->k, mi->b,
		                   d_keys.as<uint64_t>(), d_vals.as<uint64_t>(), n, c_n, c_err);
		if (hipGetLastError() != hipSuccess) ID_FAIL(MM355_EHIP);
		struct { unsigned long long n; uint32_t pad[2]; uint32_t n_long, pad2[3]; int err; } ctr;
		if (hipMemcpyAsync(&ctr, d_ctr.p, sizeof(ctr), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) ID_FAIL(MM355_EHIP);
		if (ctr.err || ctr.n != n) ID_FAIL(MM355_EINVAL);   // the table does not hold the keys the index counted
		if (n > 0) {
			// 2. sort by (bucket, key); bit 0 carries the singleton flag along
			size_t tb = 0;
			(void)rocprim::radix_sort_pairs(nullptr, tb, d_keys.as<uint64_t>(), d_keys2.as<uint64_t>(), d_vals.as<uint64_t>(), d_vals2.as<uint64_t>(), (size_t)n, 1u, (unsigned)(2 * mi->k + 1), st);
			if (d_tmp.ensure(tb + 256, ID_EXACT)) ID_FAIL(MM355_ENOMEM);
			if (rocprim::radix_sort_pairs(d_tmp.p, tb, d_keys.as<uint64_t>(), d_keys2.as<uint64_t>(), d_vals.as<uint64_t>(), d_vals2.as<uint64_t>(), (size_t)n, 1u, (unsigned)(2 * mi->k + 1), st) != hipSuccess)
				ID_FAIL(MM355_EHIP);
			if (hipStreamSynchronize(st) != hipSuccess) ID_FAIL(MM355_EHIP);
		}
		d_keys.release(); d_vals.release();
		const uint64_t *keys = d_keys2.as<uint64_t>(), *vals = d_vals2.as<uint64_t>();
		// 3. places in the new p[] (n + 1 >= 1 entries: never an empty scan), bucket bounds
		if (d_moff.ensure((n + 1) * 8, ID_EXACT) || d_kv.ensure((n + 1) * 16, ID_EXACT) || d_pair_off.ensure((n_buckets + 1) * 8, ID_EXACT) || d_p_off.ensure((n_buckets + 1) * 8, ID_EXACT)) ID_FAIL(MM355_ENOMEM);
		uint64_t *cnt = d_kv.as<uint64_t>();   // (the pair array is written last: until then its buffer holds the counts)
		hipLaunchKernelGGL(k_multi_counts, ID_GRID(n + 1), dim3(ID_BLOCK), 0, st, keys, vals, n, cnt);
		{
			size_t tb = 0;
			(void)rocprim::exclusive_scan(nullptr, tb, cnt, d_moff.as<uint64_t>(), (uint64_t)0, (size_t)n + 1, rocprim::plus<uint64_t>(), st);
			if (d_tmp.ensure(tb + 256, ID_EXACT)) ID_FAIL(MM355_ENOMEM);
			if (rocprim::exclusive_scan(d_tmp.p, tb, cnt, d_moff.as<uint64_t>(), (uint64_t)0, (size_t)n + 1, rocprim::plus<uint64_t>(), st) != hipSuccess) ID_FAIL(MM355_EHIP);
		}
		uint64_t tot_p = 0;
		if (hipMemcpyAsync(&tot_p, d_moff.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) ID_FAIL(MM355_EHIP);
		if (tot_p != n_pos) ID_FAIL(MM355_EINVAL);
		hipLaunchKernelGGL(k_bucket_bounds, ID_GRID(n_buckets + 1), dim3(ID_BLOCK), 0, st, keys, n, d_moff.as<uint64_t>(), shift, n_buckets, d_pair_off.as<uint64_t>(), d_p_off.as<uint64_t>());
		// 4. the new p[] (nothing to gather in an index without a multi-occurrence key), then the file's pairs
		if (n_pos > 0) {
			if (d_p.ensure(n_pos * 8, ID_EXACT) || d_long.ensure((size_t)long_cap * 8, ID_EXACT)) ID_FAIL(MM355_ENOMEM);
			hipLaunchKernelGGL(k_gather_runs, ID_GRID(n), dim3(ID_BLOCK), 0, st, keys, vals, d_moff.as<uint64_t>(), n, (const uint64_t*)mi->d_pos, n_pos, d_p.as<uint64_t>(),
			                   d_long.as<uint64_t>(), long_cap, c_long, c_err);
			hipLaunchKernelGGL(k_gather_long, dim3(1024), dim3(ID_BLOCK), 0, st, vals, d_moff.as<uint64_t>(), (const uint64_t*)mi->d_pos, d_p.as<uint64_t>(), d_long.as<uint64_t>(), c_long, long_cap);
		}
		// (the scan has consumed k_multi_counts' output by now in stream order: its buffer becomes the pair array)
		if (n > 0) hipLaunchKernelGGL(k_file_pairs, ID_GRID(n), dim3(ID_BLOCK), 0, st, keys, vals, d_moff.as<uint64_t>(), d_p_off.as<uint64_t>(), n, shift, n_buckets, d_kv.as<mm128>(), c_err);
		if (hipGetLastError() != hipSuccess) ID_FAIL(MM355_EHIP);
		if (hipMemcpyAsync(&ctr, d_ctr.p, sizeof(ctr), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) ID_FAIL(MM355_EHIP);
		if (ctr.err) ID_FAIL(MM355_EINVAL);
		d_keys2.release(); d_vals2.release(); d_moff.release(); d_tmp.release(); d_long.release();
		t_dev = since();
		// 5. to the file: the bucket tables in pieces of ID_PIECE buckets, the two arrays through one ID_PIECE buffer each
		DevFeed f_p(d_p.p, n_pos, &t_write), f_kv(d_kv.p, 2 * n, &t_write);
		pair_off.resize((size_t)std::min<uint64_t>(n_buckets, ID_PIECE) + 1); p_off.resize(pair_off.size());
		for (uint64_t b0 = 0; b0 < n_buckets && rc == 0; b0 += ID_PIECE) {
			const uint64_t nb = std::min<uint64_t>(n_buckets - b0, ID_PIECE);
			if (hipMemcpy(pair_off.data(), d_pair_off.as<uint64_t>() + b0, (nb + 1) * 8, hipMemcpyDeviceToHost) != hipSuccess ||
			    hipMemcpy(p_off.data(), d_p_off.as<uint64_t>() + b0, (nb + 1) * 8, hipMemcpyDeviceToHost) != hipSuccess) ID_FAIL(MM355_EHIP);
			for (uint64_t j = 0; j < nb && rc == 0; ++j) {
				const uint64_t np = p_off[j + 1] - p_off[j], size = pair_off[j + 1] - pair_off[j];
				if (np > (uint64_t)INT32_MAX || size > UINT32_MAX) ID_FAIL(MM355_EUNSUP);   // the file's n is an int32, as minimap2's
				const int32_t n32 = (int32_t)np; const uint32_t size32 = (uint32_t)size;
				if (fwrite(&n32, 4, 1, fp) != 1) ID_FAIL(MM355_EIO);
				if ((rc = f_p.write(np, fp)) != 0) break;
				if (fwrite(&size32, 4, 1, fp) != 1) ID_FAIL(MM355_EIO);
				rc = f_kv.write(2 * size, fp);
			}
		}
	}
done:   // (ID_FAIL leaves the scope of every DBuf it jumps out of; the remaining ones are freed at the return)
	(void)hipStreamDestroy(st);
	(void)hipSetDevice(prev_dev);
	if (verbose) fprintf(stderr, "[mm355] index dump: %llu keys, %llu positions; device %.3f s, copies + file %.3f s (fwrite %.3f s), rc %d\n",
	                     (unsigned long long)n, (unsigned long long)n_pos, t_dev, since() - t_dev, t_write, rc);
	return rc;
}
