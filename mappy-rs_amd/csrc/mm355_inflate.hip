// mm355_inflate.hip -- BGZF members inflated on the device: the inverse of the deflate stage of mm355_bam.hip, as mm355_idxload.hip is the
// inverse of mm355_idxdump.hip.  The decoder is stated once, in mm355_inflate.h; the host walks the members (mm355_bgzfwalk.h: the only
// sequential part -- where cdata lies, ISIZE, and its prefix sum, so every payload has its place before anything runs).
//   k_bgzf_inflate  a workgroup per member, a grid of resident workgroups that loops over the members.  Huffman decoding of a member is serial:
//                 one lane walks a chain of dependent look-ups per symbol, so everything it touches is in LDS -- the compressed bytes staged
//                 as dwords (64 KB), the first-level tables (5 KB), the window the payload grows in (64 KB): 141 KB, one workgroup per CU.
//                 The other lanes stage the input, zero and fill the tables (a lane per symbol), copy stored blocks, compute the CRC-32 (the
//                 framing kernel's lanes: bgzf_block_crc) and store the finished window to its place in aligned 16-byte pieces (bgzf_copy).
//                 A refused member writes its status and nothing else; every byte of the output has one writer.
//   mm355_bgzf_inflate        the stage by itself: an upload, the kernel, a copy back (or the same functions serially on the host)
//   mm355_fastx_open_device   a reads file (bgzip FASTQ / FASTA, or BAM) through the kernel: pieces of the file through two pinned buffers on
//                 a stream the handle owns, the next piece read and walked while the device works on this one; the inflated bytes come back
//                 to the host, where the record loop of mm355_index.cpp cuts them.
#include <cstdio>
#include <cstdlib>
#include <fcntl.h>
#include <unistd.h>
#include <hip/hip_runtime.h>
#include "mm355_bgzfdev.h"
#include "mm355_inflate.h"
#include "mm355_bgzfwalk.h"
#include "mm355_bamread.h"

static_assert(sizeof(BgzfMember) == 32, "the member table is uploaded as it lies");

// data: the piece; mem[b]: member b's cdata in it (the walk has checked that it lies inside), its ISIZE, CRC-32 and place in out; status[b]: 0 or
// why the member was refused
__global__ __launch_bounds__(BGZF_LANES, 1) void k_bgzf_inflate(const unsigned char *data, const BgzfMember *mem, int64_t n_mem, char *out, int32_t *status)
{
	__shared__ __attribute__((aligned(16))) unsigned char win[INF_MAX_ISIZE + 16];   // (16: bgzf_copy reads whole dwords around a span)
	__shared__ InfWork W;
	__shared__ uint32_t tab[256], reg[BGZF_LANES], x_pow[8];
	const uint32_t tid = threadIdx.x;
	tab[tid] = crc32_tab_entry(tid);
	if (tid < 8) x_pow[tid] = crc32_x2n(11 + (int)tid);
	for (int64_t b = blockIdx.x; b < n_mem; b += gridDim.x) {
		const BgzfMember m = mem[b];
		if (m.c_len > INF_MAX_CDATA || m.isize > INF_MAX_ISIZE) {      // (the whole workgroup; the walk lets no such member through)
			if (tid == 0) status[b] = INF_E_SPAN;
			continue;
		}
		const unsigned char *cdata = data + m.c_off;
		for (uint32_t w = tid; w <= inf_in_words(m.c_len); w += BGZF_LANES) W.in[w] = inf_word(cdata, m.c_len, w);
		if (tid == 0) { W.n_in = m.c_len; W.isize = m.isize; W.out = 0; W.status = 0; W.last = 0; }
		InfBits B(W.in, m.c_len);                                     // (the decoding lane's)
		__syncthreads();
		for (;;) {
			if (tid == 0) W.status = inf_block_head(W, B);
			__syncthreads();
			if (W.status) break;                                       // (the whole workgroup)
			if (W.kind == INF_STORED) {
				inf_stored_copy(W, tid, BGZF_LANES, win);
				__syncthreads();
				if (tid == 0) inf_stored_done(W, B);
			} else {
				for (uint32_t i = tid; i < 1u << INF_LL_BITS; i += BGZF_LANES) W.ll_tab[i] = 0;
				if (tid < 1u << INF_D_BITS) W.d_tab[tid] = 0;
				__syncthreads();
				for (uint32_t s = tid; s < W.n_ll; s += BGZF_LANES) inf_fill(W.ll, W.lens, s, INF_LL_BITS, W.ll_tab);
				if (tid < W.n_d) inf_fill(W.d, W.lens + 288, tid, INF_D_BITS, W.d_tab);
				__syncthreads();
				if (tid == 0) W.status = inf_codes(W, B, win);
			}
			__syncthreads();
			const uint32_t stop = W.status | W.last;
			__syncthreads();                                           // (the next head writes both)
			if (stop) break;
		}
		__syncthreads();
		if (tid == 0 && W.status == 0 && W.out != m.isize) W.status = INF_E_OUT_SHORT;
		__syncthreads();
		if (W.status == 0) {
			const uint32_t crc = bgzf_block_crc((const char*)win, m.isize, tab, reg, x_pow, (int)tid);
			if (tid == 0 && crc != m.crc) W.status = INF_E_CRC;
			__syncthreads();
		}
		if (W.status == 0) bgzf_copy((const char*)win, out + m.o_off, m.isize, (int)tid);
		if (tid == 0) status[b] = (int32_t)W.status;
		__syncthreads();
	}
}
static_assert((1u << INF_D_BITS) <= BGZF_LANES && INF_N_D <= BGZF_LANES, "a lane per distance table entry and per distance symbol");

// ------------------------------------------------------------------ host side
static bool inflate_times_on() { const char *te = getenv("MM355_INFLATE_TIMES"); return te && *te && *te != '0'; }
static void inflate_times(const char *who, int64_t piece, int64_t n_mem, int64_t n_in, int64_t n_out, double k_us)
{
	fprintf(stderr, "[mm355] bgzf_inflate_times %s piece %lld blocks %lld bytes_in %lld bytes_out %lld k_bgzf_inflate_us %.1f\n", who, (long long)piece, (long long)n_mem,
	        (long long)n_in, (long long)n_out, k_us);
}
// the grid: a workgroup per CU (141 KB of LDS each), no more than there are members
static int inflate_grid(int dev, int64_t n_mem, unsigned *grid)
{
	int n_cu = 0;
	HIPCHK(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev));
	if (n_cu < 1) n_cu = 1;
	*grid = (unsigned)(n_mem < n_cu? n_mem : n_cu);
	return 0;
}
// k_bgzf_inflate on a caller's stream, for the merge step of mm355_bam.hip: the n_mem members of the table d_mem, cdata in d_in, into d_out
int bgzf_inflate_launch(int dev, hipStream_t st, const unsigned char *d_in, const BgzfMember *d_mem, int64_t n_mem, char *d_out, int32_t *d_status)
{
	unsigned grid = 1;
	if (int rc = inflate_grid(dev, n_mem, &grid)) return rc;
	hipLaunchKernelGGL(k_bgzf_inflate, dim3(grid), dim3(BGZF_LANES), 0, st, d_in, d_mem, n_mem, d_out, d_status);
	HIPCHK(hipGetLastError());
	return 0;
}
// a refused member among status[0 .. n)?
static bool inflate_refused(const int32_t *status, int64_t n, bool say)
{
	for (int64_t b = 0; b < n; ++b)
		if (status[b]) { if (say) fprintf(stderr, "[mm355] BGZF member %lld refused (status %d)\n", (long long)b, status[b]); return true; }
	return false;
}

// mm355_bgzf_inflate on the host: the walked members one after the other
static int bgzf_inflate_host(const unsigned char *data, const std::vector<BgzfMember> &mem, int64_t n_out, mm355_text_t **out)
{
	mm355_text_t *T = mm355_text_alloc(0, (int64_t)mem.size(), n_out);
	if (T == 0) return MM355_ENOMEM;
	T->line_off[0] = 0;
	std::vector<InfHost> S(1);
	for (const BgzfMember &m : mem)
		if (inf_member_host(data + m.c_off, m.c_len, m.isize, m.crc, (unsigned char*)T->text + m.o_off, S[0])) { mm355_free_text_host(T); return MM355_EIO; }
	*out = T;
	return 0;
}

extern "C" int mm355_bgzf_inflate(mm355_ctx_t *c, const void *data, int64_t n, int where, mm355_text_t **out)
{
	if (out == 0) return MM355_EINVAL;
	*out = 0;
	if (n < 0 || (n > 0 && data == 0) || where < MM355_PAF_AUTO || where > MM355_PAF_DEVICE || (where == MM355_PAF_DEVICE && c == 0)) return MM355_EINVAL;
	const double t0 = mm355_now_ms();
	std::vector<BgzfMember> mem;
	int64_t used = 0, n_out = 0;
	const int wrc = bgzf_walk((const unsigned char*)data, n, true, true, mem, &used, &n_out);
	if (wrc) return wrc == BGZF_WALK_NOT_BGZF? MM355_EINVAL : wrc;
	const int64_t n_mem = (int64_t)mem.size();
	// AUTO: the host, as for the bare wrap -- the bytes are the caller's, in host memory
	if (where != MM355_PAF_DEVICE || n_mem == 0) {
		if (int rc = bgzf_inflate_host((const unsigned char*)data, mem, n_out, out)) return rc;
	} else {
		HIPCHK(hipSetDevice(c->dev));
		const size_t w_status = up256((size_t)n_mem * sizeof(BgzfMember));
		if (c->rec_text.ensure((size_t)n + 64) || c->bam_out.ensure((size_t)n_out + 64) || c->bam_work.ensure(w_status + (size_t)n_mem * 4)) return MM355_ENOMEM;
		unsigned grid = 1;
		if (int rc = inflate_grid(c->dev, n_mem, &grid)) return rc;
		BgzfMember *d_mem = (BgzfMember*)c->bam_work.p;
		int32_t *d_status = (int32_t*)((char*)c->bam_work.p + w_status);
		HIPCHK(hipMemcpyAsync(c->rec_text.p, data, (size_t)n, hipMemcpyHostToDevice, c->st));
		HIPCHK(hipMemcpyAsync(d_mem, mem.data(), (size_t)n_mem * sizeof(BgzfMember), hipMemcpyHostToDevice, c->st));
		const bool times = inflate_times_on();
		if (times) (void)hipEventRecord(c->ev0, c->st);
		hipLaunchKernelGGL(k_bgzf_inflate, dim3(grid), dim3(BGZF_LANES), 0, c->st, (const unsigned char*)c->rec_text.p, (const BgzfMember*)d_mem, n_mem, (char*)c->bam_out.p, d_status);
		HIPCHK(hipGetLastError());
		if (times) (void)hipEventRecord(c->ev1, c->st);
		std::vector<int32_t> status((size_t)n_mem);
		HIPCHK(hipMemcpyAsync(status.data(), d_status, (size_t)n_mem * 4, hipMemcpyDeviceToHost, c->st));
		HIPCHK(mm355_wait_stream(c->st));
		if (times) { float ms = 0; (void)hipEventElapsedTime(&ms, c->ev0, c->ev1); inflate_times("unwrap", 0, n_mem, n, n_out, (double)ms * 1e3); }
		if (inflate_refused(status.data(), n_mem, false)) return MM355_EIO;   // (nothing has been copied back)
		mm355_text_t *T = mm355_text_alloc(0, n_mem, n_out);
		if (T == 0) return MM355_ENOMEM;
		T->line_off[0] = 0;
		hipError_t e = n_out? hipMemcpyAsync(T->text, c->bam_out.p, (size_t)n_out, hipMemcpyDeviceToHost, c->st) : hipSuccess;
		if (e == hipSuccess) e = mm355_wait_stream(c->st);
		if (e != hipSuccess) { mm355_free_text_host(T); return MM355_EHIP; }
		*out = T;
	}
	(*out)->on_device = where == MM355_PAF_DEVICE && n_mem > 0;
	(*out)->ms_format = mm355_now_ms() - t0;
	return 0;
}

// ------------------------------------------------------------------ the reader's byte source
#define INF_PIECE_DEFAULT ((size_t)32 << 20)
#define INF_MEMBER_MAX ((size_t)65536)                 // BSIZE + 1 at most

struct DevInflateSource : ByteSource {
	int fd = -1, dev = 0;
	hipStream_t st = 0; hipEvent_t k0 = 0, k1 = 0;
	size_t piece = INF_PIECE_DEFAULT, cap_in = 0;
	HBuf h_in[2], h_out[2], h_status[2]; DBuf d_in, d_mem, d_status, d_out;
	std::vector<BgzfMember> mem[2];
	size_t n_in[2] = { 0, 0 }; int64_t n_out[2] = { 0, 0 };
	std::vector<unsigned char> tail;                   // the head of the member that the next piece completes
	int64_t file_off = 0, n_pieces = 0; bool file_eof = false, first = true, in_flight = false, times = false;
	int cur = 0, err = 0;
	size_t out_pos = 0, out_end = 0; const char *out_buf = 0;
	~DevInflateSource()
	{
		(void)hipSetDevice(dev);
		if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
		if (k0) (void)hipEventDestroy(k0);
		if (k1) (void)hipEventDestroy(k1);
		if (fd >= 0) close(fd);
	}
	// the next piece into buffer q: the tail, then the file until a whole member is there; 0 (mem[q] may be empty: the file has ended),
	// BGZF_WALK_NOT_BGZF, or an MM355_E* code
	int prepare(int q)
	{
		unsigned char *h = (unsigned char*)h_in[q].p;
		size_t have = tail.size();
		if (have) memcpy(h, tail.data(), have);
		tail.clear();
		mem[q].clear(); n_in[q] = 0; n_out[q] = 0;
		for (;;) {
			size_t want = piece < cap_in - have? piece : cap_in - have;
			while (want > 0 && !file_eof) {
				const ssize_t r = pread(fd, h + have, want, (off_t)file_off);
				if (r < 0) return MM355_EIO;
				if (r == 0) { file_eof = true; break; }
				have += (size_t)r; want -= (size_t)r; file_off += r;
			}
			int64_t used = 0;
			const int rc = bgzf_walk(h, (int64_t)have, first, file_eof, mem[q], &used, &n_out[q], (int64_t)(8 * piece + INF_MAX_ISIZE));
			if (rc) return rc;
			if (mem[q].empty() && !file_eof && have < cap_in) continue;   // (a piece smaller than its first member: more of the file)
			if (mem[q].empty() && have > 0 && !file_eof) return MM355_EIO;
			first = false;
			n_in[q] = (size_t)used;
			tail.assign(h + used, h + have);
			return 0;
		}
	}
	// upload, kernel and copies back of buffer q, all on the stream
	int launch(int q)
	{
		const int64_t n_mem = (int64_t)mem[q].size();
		if (d_in.ensure(n_in[q] + 64) || d_out.ensure((size_t)n_out[q] + 64) || d_mem.ensure((size_t)n_mem * sizeof(BgzfMember)) || d_status.ensure((size_t)n_mem * 4) ||
		    h_out[q].ensure((size_t)n_out[q] + 64) || h_status[q].ensure((size_t)n_mem * 4 + 64)) return MM355_ENOMEM;
		unsigned grid = 1;
		if (int rc = inflate_grid(dev, n_mem, &grid)) return rc;
		HIPCHK(hipMemcpyAsync(d_in.p, h_in[q].p, n_in[q], hipMemcpyHostToDevice, st));
		HIPCHK(hipMemcpyAsync(d_mem.p, mem[q].data(), (size_t)n_mem * sizeof(BgzfMember), hipMemcpyHostToDevice, st));
		if (times) (void)hipEventRecord(k0, st);
		hipLaunchKernelGGL(k_bgzf_inflate, dim3(grid), dim3(BGZF_LANES), 0, st, (const unsigned char*)d_in.p, (const BgzfMember*)d_mem.p, n_mem, (char*)d_out.p, (int32_t*)d_status.p);
		HIPCHK(hipGetLastError());
		if (times) (void)hipEventRecord(k1, st);
		HIPCHK(hipMemcpyAsync(h_status[q].p, d_status.p, (size_t)n_mem * 4, hipMemcpyDeviceToHost, st));
		if (n_out[q]) HIPCHK(hipMemcpyAsync(h_out[q].p, d_out.p, (size_t)n_out[q], hipMemcpyDeviceToHost, st));
		in_flight = true; cur = q;
		return 0;
	}
	// the piece in flight has arrived: its bytes are the output; the next piece, read and walked meanwhile, is launched
	int advance()
	{
		HIPCHK(hipSetDevice(dev));
		const int q = cur, nx = 1 - cur;
		int prc = 0;
		mem[nx].clear();
		if (!file_eof || !tail.empty()) {              // (a file of one piece has nothing to overlap: one buffer)
			if (h_in[nx].ensure(cap_in, 1024)) return MM355_ENOMEM;
			prc = prepare(nx);                         // (the file read overlaps the device's work on piece q)
		}
		HIPCHK(mm355_wait_stream(st));
		in_flight = false;
		if (times) { float ms = 0; (void)hipEventElapsedTime(&ms, k0, k1); inflate_times("reader", n_pieces, (int64_t)mem[q].size(), (int64_t)n_in[q], n_out[q], (double)ms * 1e3); }
		++n_pieces;
		if (inflate_refused((const int32_t*)h_status[q].p, (int64_t)mem[q].size(), true)) return MM355_EIO;
		out_buf = (const char*)h_out[q].p; out_pos = 0; out_end = (size_t)n_out[q];
		if (prc) { next_err = prc < 0? prc : MM355_EIO; return 0; }   // (this piece's bytes first; the error when the reader gets there)
		if (!mem[nx].empty()) return launch(nx);
		return 0;
	}
	int next_err = 0;
	int64_t read(void *buf, size_t cap)
	{
		while (out_pos == out_end) {
			if (err) return err;
			if (!in_flight) { if (next_err) err = next_err; return err; }
			if (int rc = advance()) { err = rc; return rc; }
		}
		const size_t k = cap < out_end - out_pos? cap : out_end - out_pos;
		memcpy(buf, out_buf + out_pos, k);
		out_pos += k;
		return (int64_t)k;
	}
};

extern "C" int mm355_fastx_open_device(const char *path, int keep_qual, int device, mm355_fastx_t **out)
{
	if (out == 0) return MM355_EINVAL;
	*out = 0;
	if (path == 0) return MM355_EINVAL;
	const int fd = open(path, O_RDONLY);
	if (fd < 0) return MM355_EIO;
	// a file that is not BGZF ends here, before the device is touched: the caller opens it as it does today
	unsigned char head[INF_MEMBER_MAX];
	const ssize_t nh = pread(fd, head, sizeof(head), 0);
	BgzfMember m0;
	if (nh < 0) { close(fd); return MM355_EIO; }
	if (bgzf_member(head, nh, 0, &m0) < 0 || nh < 18) { close(fd); return MM355_EINVAL; }
	mm355_runtime_init();
	int ndev = 0;
	if (device < 0 || hipGetDeviceCount(&ndev) != hipSuccess || device >= ndev) { close(fd); return MM355_ENODEV; }
	DevInflateSource *S = new DevInflateSource();
	S->fd = fd; S->dev = device; S->times = inflate_times_on();
	if (const char *e = getenv("MM355_INFLATE_PIECE")) { const long long v = atoll(e); if (v > 0) S->piece = (size_t)v; }
	const off_t file_size = lseek(fd, 0, SEEK_END);
	if (file_size > 0 && (size_t)file_size < S->piece) S->piece = (size_t)file_size;   // (a small file: one piece, and no more pinned memory than it needs)
	S->cap_in = (S->piece > INF_MEMBER_MAX? S->piece : INF_MEMBER_MAX) + 2 * INF_MEMBER_MAX;
	int prev_dev = 0;
	(void)hipGetDevice(&prev_dev);
	int rc = 0;
	if (hipSetDevice(device) != hipSuccess || hipStreamCreate(&S->st) != hipSuccess) { S->st = 0; rc = MM355_EHIP; }
	if (rc == 0 && (hipEventCreate(&S->k0) != hipSuccess || hipEventCreate(&S->k1) != hipSuccess)) rc = MM355_EHIP;
	if (rc == 0 && S->h_in[0].ensure(S->cap_in, 1024)) rc = MM355_ENOMEM;
	if (rc == 0) rc = S->prepare(0);
	if (rc == BGZF_WALK_NOT_BGZF) rc = MM355_EINVAL;
	if (rc == 0 && !S->mem[0].empty()) rc = S->launch(0);
	(void)hipSetDevice(prev_dev);
	if (rc) { delete S; return rc; }
	*out = mm355_fastx_from_source(S, keep_qual != 0);
	return 0;
}
