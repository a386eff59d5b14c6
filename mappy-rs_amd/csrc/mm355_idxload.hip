// mm355_idxload.hip -- an MMI\2 file straight into HBM (mm355_index_load_mmi_device): the inverse of mm355_idxdump.hip, and the device
// counterpart of the host loader of mm355_index.cpp (U:index.c::mm_idx_load, reached in the reference through mm_idx_reader_read at
// lib.rs:407-410 when the input is an index file).
//   1. the host walks the 2 << b bucket headers and plans the pieces (mm355_mmiwalk.h): every size is known before anything is allocated;
//   2. the bucket sections cross to the device in pieces of at most P bytes through two pinned buffers on one stream, so that reading piece
//      i + 1 from the file overlaps the copy and the kernel of piece i;
//   3. k_load_piece, one thread per item: a position word goes to its place in pos[], a pair is re-keyed from (bucket, key) to the
//      minimizer, its start made global, and inserted into the flat table with the probe the build uses; its count goes to a count array;
//   4. the counts are sorted descending for mm_idx_cal_max_occ and summed, the sequence section is copied, and the index is finished as a
//      device-built one is (mm355_index_finish_device).
// The result has no host table: like an index from mm355_index_build_device it is device-resident.
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <chrono>
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_reduce.hpp>
#include <rocprim/iterator/transform_iterator.hpp>
#include "mm355_pipeline.h"
#include "mm355_mmiwalk.h"

#define IL_BLOCK 256
#define IL_EXACT 1024              // DBuf::ensure headroom divisor: these buffers live for one call and never grow

struct IlCountTo64 { __device__ uint64_t operator()(uint32_t c) const { return c; } };

// stage: the piece as it lies in the file (every item 4-byte aligned: read as dwords); segs: its segments, item0 ascending
__global__ __launch_bounds__(IL_BLOCK) void k_load_piece(const uint32_t *stage, const MmiSeg *segs, uint32_t n_seg, uint32_t n_items, int b,
                                                          mm355_slot *slots, uint64_t line_mask, uint64_t *pos, uint64_t n_pos, uint32_t *counts, uint64_t n_distinct, int *err)
{
	const uint32_t t = blockIdx.x * IL_BLOCK + threadIdx.x;
	if (t >= n_items) return;
	uint32_t lo = 0, hi = n_seg - 1;   // the last segment whose first item is <= t
	while (lo < hi) {
		const uint32_t mid = (lo + hi + 1) >> 1;
		if (segs[mid].item0 <= t) lo = mid; else hi = mid - 1;
	}
	const MmiSeg s = segs[lo];
	const uint32_t j = t - s.item0;
	if (j >= s.count) { *err = 1; return; }   // (a plan whose segments do not tile the items: never read outside the piece)
	if (s.kind == MMI_SEG_POS) {
		const uint32_t *w = stage + ((s.off >> 2) + 2 * (size_t)j);
		const uint64_t gi = s.gidx + j;
		if (gi >= n_pos) { *err = 1; return; }
		pos[gi] = (uint64_t)w[1] << 32 | w[0];
		return;
	}
	const uint32_t *w = stage + ((s.off >> 2) + 4 * (size_t)j);
	const uint64_t key = (uint64_t)w[1] << 32 | w[0], gi = s.gidx + j;
	uint64_t val = (uint64_t)w[3] << 32 | w[2];
	if (gi >= n_distinct) { *err = 1; return; }
	uint32_t cnt = 1;
	if (!(key & 1)) {   // start << 32 | count, start relative to the bucket's own p[]
		const uint64_t start = val >> 32;
		cnt = (uint32_t)val;
		if (cnt < 1 || start + cnt > s.n) { *err = 1; return; }   // a run outside its bucket: the file is refused, nothing is inserted
		val = (s.p_base + start) << 32 | cnt;
	}
	const uint64_t minier = (key >> 1) << b | s.bucket;
	table_insert_dev(slots, line_mask, minier, minier << 1 | (key & 1), val);
	counts[gi] = cnt;
}

#define IL_ALIGN16(x) (((size_t)(x) + 15) & ~(size_t)15)

extern "C" int mm355_index_load_mmi_device(const char *path, int device, mm355_index_t **out)
{
	*out = 0;
	if (path == 0) return MM355_EINVAL;
	const bool verbose = getenv("MM355_VERBOSE") != 0;
	const auto t_begin = std::chrono::steady_clock::now();
	auto since = [&]() { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count(); };
	// ---- host: walk and plan; a file that is not an index, or a bad one, ends here, before the device is touched
	FILE *fp = fopen(path, "rb");
	if (fp == 0) return MM355_EIO;
	MmiWalk wk; MmiPlan plan;
	int rc = mmi_walk(fp, &wk);
	if (rc == 0 && wk.h.n_seq == 0) rc = MM355_EIO;
	if (rc) { fclose(fp); return rc; }
	mmi_plan(wk, mmi_piece_bytes(getenv("MM355_IDXLOAD_PIECE")), &plan);
	const int fd = fileno(fp);
	const double t_walk = since();
	mm355_runtime_init();
	int ndev = 0;
	if (device < 0 || hipGetDeviceCount(&ndev) != hipSuccess || device >= ndev) { fclose(fp); return MM355_ENODEV; }
	int prev_dev = 0;
	(void)hipGetDevice(&prev_dev);
	if (hipSetDevice(device) != hipSuccess) { fclose(fp); return MM355_EHIP; }
	mm355_index *mi = new mm355_index();
	mm355_index_set_header(mi, wk.h);
	mm355_index_finish_names(mi);
	mi->dev_id = device;
	mi->n_distinct = (int64_t)wk.n_distinct; mi->n_pos = wk.n_pos;
	const uint64_t n = wk.n_distinct, n_pos = wk.n_pos, sum_len = wk.h.sum_len;
	const size_t Sw = (sum_len + 7) / 8 + 2, n_S = (size_t)(wk.S_bytes / 4);
	uint64_t want = (uint64_t)(n / 0.55) + MM355_SLOTS_PER_LINE, n_lines = 1;   // the sizing rule of the build and of the host's table_alloc
	while (n_lines * MM355_SLOTS_PER_LINE < want) n_lines <<= 1;
	mi->n_lines = n_lines;
	size_t stage_bytes = 16;
	for (const MmiPiece &p : plan.pieces) stage_bytes = std::max(stage_bytes, IL_ALIGN16(p.bytes) + (size_t)p.n_seg * sizeof(MmiSeg));
	// every temporary is an object of this scope: freed at the return, whatever the path
	hipStream_t st = 0; hipEvent_t ev[2] = { 0, 0 };
	HBuf h_stage[2]; DBuf d_stage[2], d_cnt, d_cnt2, d_tmp, d_ctr;
	void *dS = 0;
	double t_pieces = 0, t_read = 0;
#define IL_FAIL(code) do { rc = (code); if (verbose) fprintf(stderr, "[mm355] index load failed at %s:%d (%s)\n", __FILE__, __LINE__, hipGetErrorString(hipGetLastError())); goto done; } while (0)
	if (hipStreamCreate(&st) != hipSuccess) { st = 0; IL_FAIL(MM355_EHIP); }
	for (int i = 0; i < 2; ++i) if (hipEventCreateWithFlags(&ev[i], hipEventDisableTiming) != hipSuccess) { ev[i] = 0; IL_FAIL(MM355_EHIP); }
	// ---- 1. allocate from the walk's totals
	if (hipMalloc(&mi->d_slots, n_lines * MM355_SLOTS_PER_LINE * sizeof(mm355_slot)) != hipSuccess) { mi->d_slots = 0; IL_FAIL(MM355_ENOMEM); }
	if (hipMalloc(&mi->d_pos, (n_pos + 2) * 8) != hipSuccess) { mi->d_pos = 0; IL_FAIL(MM355_ENOMEM); }
	if (hipMalloc(&dS, Sw * 4) != hipSuccess) { dS = 0; IL_FAIL(MM355_ENOMEM); }
	if (d_cnt.ensure((n + 1) * 4, IL_EXACT) || d_ctr.ensure(64, IL_EXACT)) IL_FAIL(MM355_ENOMEM);
	for (size_t i = 0; i < 2 && i < plan.pieces.size(); ++i)   // (a file of one piece has nothing to overlap: one buffer)
		if (h_stage[i].ensure(stage_bytes, IL_EXACT) || d_stage[i].ensure(stage_bytes, IL_EXACT)) IL_FAIL(MM355_ENOMEM);
	if (hipMemsetAsync(mi->d_slots, 0xff, n_lines * MM355_SLOTS_PER_LINE * sizeof(mm355_slot), st) != hipSuccess ||
	    hipMemsetAsync(mi->d_pos, 0, (n_pos + 2) * 8, st) != hipSuccess || hipMemsetAsync(dS, 0, Sw * 4, st) != hipSuccess ||
	    hipMemsetAsync(d_cnt.p, 0, (n + 1) * 4, st) != hipSuccess || hipMemsetAsync(d_ctr.p, 0, 64, st) != hipSuccess) IL_FAIL(MM355_EHIP);
	// ---- 2. the pieces
	for (size_t i = 0; i < plan.pieces.size(); ++i) {
		const MmiPiece &p = plan.pieces[i];
		const int q = (int)(i & 1);
		if (i >= 2 && hipEventSynchronize(ev[q]) != hipSuccess) IL_FAIL(MM355_EHIP);   // the copy of piece i - 2 has left this buffer
		uint8_t *h = (uint8_t*)h_stage[q].p;
		const size_t seg_at = IL_ALIGN16(p.bytes), total = seg_at + (size_t)p.n_seg * sizeof(MmiSeg);
		const auto t0 = std::chrono::steady_clock::now();
		if (!mmi_pread(fd, h, p.bytes, p.file_off)) IL_FAIL(MM355_EIO);   // (the file shrank after the walk)
		t_read += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
		if (p.n_seg) memcpy(h + seg_at, &plan.segs[p.seg0], (size_t)p.n_seg * sizeof(MmiSeg));
		if (hipMemcpyAsync(d_stage[q].p, h, total, hipMemcpyHostToDevice, st) != hipSuccess || hipEventRecord(ev[q], st) != hipSuccess) IL_FAIL(MM355_EHIP);
		if (p.n_items == 0) continue;   // headers only (empty buckets)
		hipLaunchKernelGGL(k_load_piece, dim3((p.n_items + IL_BLOCK - 1) / IL_BLOCK), dim3(IL_BLOCK), 0, st, (const uint32_t*)d_stage[q].p,
		                   (const MmiSeg*)((const uint8_t*)d_stage[q].p + seg_at), p.n_seg, p.n_items, mi->b, (mm355_slot*)mi->d_slots, n_lines - 1,
		                   (uint64_t*)mi->d_pos, n_pos, d_cnt.as<uint32_t>(), n, d_ctr.as<int>());
		if (hipGetLastError() != hipSuccess) IL_FAIL(MM355_EHIP);
	}
	{
		int e = 0;
		if (hipMemcpyAsync(&e, d_ctr.p, 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) IL_FAIL(MM355_EHIP);
		if (e) IL_FAIL(MM355_EIO);   // a value that points outside its bucket's p[]
	}
	t_pieces = since();
	for (int i = 0; i < 2; ++i) { h_stage[i].release(); d_stage[i].release(); }
	// ---- 3. counts: their sum is n_minimizers, their descending head answers mm_idx_cal_max_occ (as the build leaves it)
	mi->n_minimizers = 0;
	if (n > 0) {
		uint64_t *d_sum = d_ctr.as<uint64_t>() + 1;
		auto in64 = rocprim::make_transform_iterator(d_cnt.as<uint32_t>(), IlCountTo64());
		if (d_cnt2.ensure((n + 1) * 4, IL_EXACT)) IL_FAIL(MM355_ENOMEM);
		size_t tb_sum = 0, tb_sort = 0;
		(void)rocprim::reduce(nullptr, tb_sum, in64, d_sum, (uint64_t)0, (size_t)n, rocprim::plus<uint64_t>(), st);
		(void)rocprim::radix_sort_keys_desc(nullptr, tb_sort, d_cnt.as<uint32_t>(), d_cnt2.as<uint32_t>(), (size_t)n, 0u, 32u, st);
		if (d_tmp.ensure(std::max(tb_sum, tb_sort) + 256, IL_EXACT)) IL_FAIL(MM355_ENOMEM);
		if (rocprim::reduce(d_tmp.p, tb_sum, in64, d_sum, (uint64_t)0, (size_t)n, rocprim::plus<uint64_t>(), st) != hipSuccess) IL_FAIL(MM355_EHIP);
		uint64_t sum = 0;
		if (hipMemcpyAsync(&sum, d_sum, 8, hipMemcpyDeviceToHost, st) != hipSuccess) IL_FAIL(MM355_EHIP);
		if (rocprim::radix_sort_keys_desc(d_tmp.p, tb_sort, d_cnt.as<uint32_t>(), d_cnt2.as<uint32_t>(), (size_t)n, 0u, 32u, st) != hipSuccess) IL_FAIL(MM355_EHIP);
		const size_t keep = (size_t)std::min<uint64_t>(n, 2u << 20);
		mi->top_counts.resize(keep);
		if (hipMemcpyAsync(mi->top_counts.data(), d_cnt2.p, keep * 4, hipMemcpyDeviceToHost, st) != hipSuccess) IL_FAIL(MM355_EHIP);
		if (hipStreamSynchronize(st) != hipSuccess) IL_FAIL(MM355_EHIP);
		mi->n_minimizers = (int64_t)sum;
	}
	d_cnt.release(); d_cnt2.release(); d_tmp.release();
	// ---- 4. the sequence: the host keeps the 4-bit image (mm_idx_getseq, the .mmi), the device gets it for the 2-bit pack
	if (n_S) {
		mi->S.resize(n_S);
		if (!mmi_pread(fd, mi->S.data(), n_S * 4, wk.off_S)) IL_FAIL(MM355_EIO);
		if (hipMemcpy(dS, mi->S.data(), n_S * 4, hipMemcpyHostToDevice) != hipSuccess) IL_FAIL(MM355_EHIP);
	} else if (!(mi->flag & 2)) mi->S.resize(1);   // (contigs without a base: the host loader leaves one word)
	if (hipStreamSynchronize(st) != hipSuccess) IL_FAIL(MM355_EHIP);
	rc = mm355_index_finish_device(mi, device, dS); dS = 0;
done:   // (IL_FAIL jumps here from the function's own scope: the buffers above are freed at the return)
	if (dS) (void)hipFree(dS);
	for (int i = 0; i < 2; ++i) if (ev[i]) (void)hipEventDestroy(ev[i]);
	if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
	fclose(fp);
	if (verbose) fprintf(stderr, "[mm355] index load: %llu keys, %llu positions, %zu pieces of <= %llu bytes; walk %.3f s, pieces %.3f s (file reads %.3f s), total %.3f s, rc %d\n",
	                     (unsigned long long)n, (unsigned long long)n_pos, plan.pieces.size(), (unsigned long long)plan.P, t_walk, t_pieces - t_walk, t_read, since(), rc);
	if (rc) { mm355_index_free_build_buffers(mi); delete mi; (void)hipSetDevice(prev_dev); return rc; }
	(void)hipSetDevice(prev_dev);
	*out = mi;
	return 0;
}
