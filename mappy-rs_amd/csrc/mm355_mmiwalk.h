// mm355_mmiwalk.h -- the host's view of an MMI\2 file (U:index.c::mm_idx_load): header and contigs (shared by the host loader of
// mm355_index.cpp and the device loader of mm355_idxload.hip), the walk over the bucket sections, and the plan that cuts them into
// pieces for the device.  Plain C++: no HIP here, the CPU suite compiles this file with g++ alone.
//   header   "MMI\2", w k b n_seq flag (uint32 each); per contig: uint8 l, l name bytes, uint32 len
//   bucket   int32 n, n x uint64 p[];  uint32 size, size x (uint64 key, uint64 value)        -- 1<<b of them
//   S        (sum_len + 7) / 8 x uint32, absent with MM_I_NO_SEQ (flag & 2)
// The only sequential part of the format is that a bucket's place follows from the sizes of the buckets before it: the walk reads the
// 2 << b headers and skips the payload.  Everything after that is known before a byte of payload is read.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <unistd.h>
#include <sys/types.h>
#include <sys/stat.h>
#include <string>
#include <vector>
#include "../../include/mm355.h"

struct MmiHeader {
	int32_t w = 0, k = 0, b = 0, flag = 0;
	uint32_t n_seq = 0;
	std::vector<std::string> names;
	std::vector<uint64_t> seq_off;
	std::vector<uint32_t> seq_len;
	uint64_t sum_len = 0;
};

// The header and the contig table from the start of fp, which is left at the first bucket.  MM355_EINVAL: not an MMI\2 file.  MM355_EIO:
// truncated, or a header no index can have.  A corrupt header must not drive the 1<<b bucket loop or the sketch kernels: U:sketch.c asserts
// 0 < w < 256, 0 < k <= 28; b <= 2k.
inline int mmi_read_header(FILE *fp, MmiHeader *h)
{
	char magic[4]; uint32_t x[5];
	if (fread(magic, 1, 4, fp) != 4 || memcmp(magic, "MMI\2", 4) != 0) return MM355_EINVAL;
	if (fread(x, 4, 5, fp) != 5) return MM355_EIO;
	if (x[0] < 1 || x[0] > 255 || x[1] < 1 || x[1] > 28 || x[2] > 28 || x[2] > 2 * x[1]) return MM355_EIO;
	h->w = (int32_t)x[0], h->k = (int32_t)x[1], h->b = (int32_t)x[2], h->n_seq = x[3], h->flag = (int32_t)x[4];
	h->names.clear(); h->seq_off.clear(); h->seq_len.clear(); h->sum_len = 0;
	for (uint32_t i = 0; i < h->n_seq; ++i) {
		uint8_t l; uint32_t len; char nm[256];
		if (fread(&l, 1, 1, fp) != 1) return MM355_EIO;
		if (l && fread(nm, 1, l, fp) != l) return MM355_EIO;
		if (fread(&len, 4, 1, fp) != 1) return MM355_EIO;
		h->names.emplace_back(nm, l); h->seq_off.push_back(h->sum_len); h->seq_len.push_back(len);
		h->sum_len += len;
	}
	return 0;
}

// ------------------------------------------------------------------ the walk
struct MmiBucket { uint64_t off; uint32_t n, size; };   // off: file offset of the bucket's int32 n; p[] at off + 4, size at off + 4 + 8n, pairs 4 further

struct MmiWalk {
	MmiHeader h;
	uint64_t off_buckets = 0, off_S = 0, file_size = 0, S_bytes = 0;
	std::vector<MmiBucket> bk;                // 1 << b
	std::vector<uint64_t> p_base, pair_base;  // exclusive prefix sums of n and of size, (1 << b) + 1 entries
	uint64_t n_pos = 0, n_distinct = 0;
};

inline bool mmi_pread(int fd, void *dst, size_t n, uint64_t off)
{
	uint8_t *d = (uint8_t*)dst;
	while (n) {
		const ssize_t r = pread(fd, d, n, (off_t)off);
		if (r <= 0) return false;
		d += r; n -= (size_t)r; off += (uint64_t)r;
	}
	return true;
}

// fp at offset 0.  0, or MM355_EINVAL (not an MMI\2 file), MM355_EIO (truncated or inconsistent: a negative n, a bucket that ends beyond
// the file, a short S section), MM355_EUNSUP (2^32 or more positions: a table value packs offset << 32 | count).  Only the first part of
// a multi-part file is walked, as the host loader reads only the first.
inline int mmi_walk(FILE *fp, MmiWalk *w)
{
	if (int rc = mmi_read_header(fp, &w->h)) return rc;
	const off_t at = ftello(fp);
	struct stat sb;
	const int fd = fileno(fp);
	if (at < 0 || fd < 0 || fstat(fd, &sb) != 0) return MM355_EIO;
	w->off_buckets = (uint64_t)at; w->file_size = (uint64_t)sb.st_size;
	const uint64_t nb = 1ULL << w->h.b;
	if (w->off_buckets > w->file_size || nb > (w->file_size - w->off_buckets) / 8) return MM355_EIO;   // (a bucket is at least its two headers: nothing is sized by a b the file cannot hold)
	w->bk.resize(nb); w->p_base.resize(nb + 1); w->pair_base.resize(nb + 1);
	uint64_t off = w->off_buckets, np = 0, nd = 0;
	for (uint64_t i = 0; i < nb; ++i) {
		int32_t n; uint32_t size;
		if (off + 4 > w->file_size || !mmi_pread(fd, &n, 4, off)) return MM355_EIO;
		if (n < 0) return MM355_EIO;
		const uint64_t off_size = off + 4 + 8ULL * (uint32_t)n;
		if (off_size + 4 > w->file_size || !mmi_pread(fd, &size, 4, off_size)) return MM355_EIO;
		const uint64_t end = off_size + 4 + 16ULL * size;
		if (end > w->file_size) return MM355_EIO;
		w->bk[i].off = off; w->bk[i].n = (uint32_t)n; w->bk[i].size = size;
		w->p_base[i] = np; w->pair_base[i] = nd;
		np += (uint32_t)n; nd += size; off = end;
	}
	w->p_base[nb] = np; w->pair_base[nb] = nd;
	w->n_pos = np; w->n_distinct = nd; w->off_S = off;
	w->S_bytes = (w->h.flag & 2)? 0 : (w->h.sum_len + 7) / 8 * 4;
	if (w->off_S + w->S_bytes > w->file_size) return MM355_EIO;
	if (np >= (1ULL << 32)) return MM355_EUNSUP;
	return 0;
}

// ------------------------------------------------------------------ the piece plan
// The bucket section is cut into consecutive file ranges of at most P bytes, each read with one call into a staging buffer and copied to the
// device whole.  A cut falls only between items: a 4-byte header (n or size), an 8-byte position word, a 16-byte pair.  Every item sits a
// multiple of 4 bytes after the first bucket, and the 4-byte size header between a bucket's p[] and its pairs puts the two 4 bytes apart
// modulo 8: no placement aligns both to their own size.  A piece therefore goes to the base of the (16-byte aligned) staging buffer, where all
// its items are 4-byte aligned whatever the section's offset in the file, and the kernel reads dwords.
#define MMI_SEG_POS  0u
#define MMI_SEG_PAIR 1u
struct MmiSeg {              // a run of items of one kind and one bucket inside a piece (empty runs are not listed; headers are not items)
	uint64_t gidx;           // the first item's global index: into pos[] (MMI_SEG_POS) or into the file's pair sequence (MMI_SEG_PAIR)
	uint64_t p_base;         // pairs: where the bucket's p[] begins in pos[]
	uint32_t item0;          // the first item's index among the piece's items (ascending over the list: a thread finds its segment by binary search)
	uint32_t count;          // items
	uint32_t off;            // byte offset of the first item inside the piece
	uint32_t bucket;
	uint32_t n;              // pairs: the bucket's n (start + count of a value must stay inside it)
	uint32_t kind;
};
struct MmiPiece { uint64_t file_off; uint32_t bytes, seg0, n_seg, n_items; };
struct MmiPlan { uint64_t P = 0; std::vector<MmiPiece> pieces; std::vector<MmiSeg> segs; };

#define MMI_PIECE_DEFAULT (32u << 20)
#define MMI_PIECE_MIN 64u
#define MMI_PIECE_MAX (1u << 30)   // offsets inside a piece and its item count are uint32

inline uint64_t mmi_piece_bytes(const char *env)   // MM355_IDXLOAD_PIECE
{
	uint64_t P = MMI_PIECE_DEFAULT;
	if (env && *env) { P = strtoull(env, 0, 10); if (P < MMI_PIECE_MIN) P = MMI_PIECE_MIN; if (P > MMI_PIECE_MAX) P = MMI_PIECE_MAX; }
	return P;
}

inline void mmi_plan(const MmiWalk &w, uint64_t P, MmiPlan *pl)
{
	if (P < MMI_PIECE_MIN) P = MMI_PIECE_MIN;
	if (P > MMI_PIECE_MAX) P = MMI_PIECE_MAX;
	pl->P = P; pl->pieces.clear(); pl->segs.clear();
	MmiPiece cur = { w.off_buckets, 0, 0, 0, 0 };
	auto close = [&]() {
		if (cur.bytes) { cur.n_seg = (uint32_t)pl->segs.size() - cur.seg0; pl->pieces.push_back(cur); }
		cur.file_off += cur.bytes; cur.bytes = 0; cur.seg0 = (uint32_t)pl->segs.size(); cur.n_seg = 0; cur.n_items = 0;
	};
	auto header = [&]() { if (cur.bytes + 4 > P) close(); cur.bytes += 4; };
	auto items = [&](uint32_t kind, uint32_t bucket, uint64_t total, uint32_t width, uint64_t gidx) {
		for (uint64_t done = 0; done < total;) {
			const uint64_t room = (P - cur.bytes) / width;
			if (room == 0) { close(); continue; }
			const uint64_t take = total - done < room? total - done : room;
			MmiSeg s;
			s.gidx = gidx + done; s.p_base = w.p_base[bucket]; s.item0 = cur.n_items; s.count = (uint32_t)take; s.off = cur.bytes;
			s.bucket = bucket; s.n = w.bk[bucket].n; s.kind = kind;
			pl->segs.push_back(s);
			cur.n_items += (uint32_t)take; cur.bytes += (uint32_t)(take * width); done += take;
		}
	};
	for (uint64_t i = 0; i < w.bk.size(); ++i) {
		header(); items(MMI_SEG_POS, (uint32_t)i, w.bk[i].n, 8, w.p_base[i]);
		header(); items(MMI_SEG_PAIR, (uint32_t)i, w.bk[i].size, 16, w.pair_base[i]);
	}
	close();
}
