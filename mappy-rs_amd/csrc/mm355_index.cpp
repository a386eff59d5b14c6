// mm355_index.cpp -- host side of the index: MMI\2 reader and writer, FASTA/FASTQ builder, the flat
// 128-B-line hash table that is uploaded to HBM, sequence accessors and option presets.
// Replaces, behind the C-ABI of include/mm355.h, the reference's FFI calls
//   mm_set_opt (lib.rs:333,336), mm_idx_reader_open/read/close (lib.rs:397-412),
//   mm_mapopt_update (lib.rs:414), mm_idx_index_name (lib.rs:416),
//   mm_idx_name2id (lib.rs:716), mm_idx_getseq (lib.rs:747), mm_idx_dump (fn_idx_out, lib.rs:391-394).
// minimap2 2.26 units whose observable behaviour is kept: U:index.c (file format, key/value
// encoding, positions ascending inside a run, mm_idx_cal_max_occ), U:options.c (presets).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <limits.h>
#include <algorithm>
#include <thread>
#include <atomic>
#include <zlib.h>
#include "mm355_host.h"
#include "mm355_mmiwalk.h"
#include "mm355_bamread.h"

#define mm_seq4_set(s, i, c) ((s)[(i)>>3] |= (uint32_t)(c) << (((i)&7)<<2))
#define mm_seq4_get(s, i)    ((s)[(i)>>3] >> (((i)&7)<<2) & 0xf)

// ------------------------------------------------------------------ options (U:options.c)
static void idxopt_init(mm355_idxopt_t *o)
{
	memset(o, 0, sizeof(*o));
	o->k = 15, o->w = 10, o->flag = 0, o->bucket_bits = 14;
	o->mini_batch_size = 50000000; o->batch_size = 4000000000ULL;
}

static void mapopt_init(mm355_mapopt_t *o)
{
	memset(o, 0, sizeof(*o));
	o->seed = 11;
	o->mid_occ_frac = 2e-4f; o->min_mid_occ = 10; o->max_mid_occ = 1000000;
	o->sdust_thres = 0; o->q_occ_frac = 0.01f;
	o->min_cnt = 3; o->min_chain_score = 40;
	o->bw = 500; o->bw_long = 20000;
	o->max_gap = 5000; o->max_gap_ref = -1;
	o->max_chain_skip = 25; o->max_chain_iter = 5000;
	o->rmq_inner_dist = 1000; o->rmq_size_cap = 100000; o->rmq_rescue_size = 1000; o->rmq_rescue_ratio = 0.1f;
	o->chain_gap_scale = 0.8f; o->chain_skip_scale = 0.0f;
	o->max_max_occ = 4095; o->occ_dist = 500;
	o->mask_level = 0.5f; o->mask_len = INT_MAX; o->pri_ratio = 0.8f; o->best_n = 5;
	o->alt_drop = 0.15f;
	o->a = 2; o->b = 4; o->q = 4; o->e = 2; o->q2 = 24; o->e2 = 1; o->sc_ambi = 1;
	o->zdrop = 400; o->zdrop_inv = 200; o->end_bonus = -1;
	o->min_dp_max = o->min_chain_score * o->a;
	o->min_ksw_len = 200; o->max_clip_ratio = 1.0f;
	o->max_sw_mat = 100000000;
}

extern "C" int mm355_set_opt(const char *preset, mm355_idxopt_t *io, mm355_mapopt_t *mo)
{
	if (preset == 0) { idxopt_init(io); mapopt_init(mo); return 0; }
	std::string p(preset);
	if (p == "map-ont") return 0;
	if (p == "map-hifi" || p == "map-ccs") {
		io->flag = 0; io->k = 19; io->w = 19;
		mo->max_gap = 10000;
		mo->a = 1; mo->b = 4; mo->q = 6; mo->q2 = 26; mo->e = 2; mo->e2 = 1;
		mo->min_mid_occ = 50; mo->max_mid_occ = 500;
		mo->min_dp_max = 200;
		return 0;
	}
	if (p == "ava-ont") {
		io->flag = 0; io->k = 15; io->w = 5;
		mo->flag |= 0x800000LL | 0x001LL | 0x002LL | 0x400LL;
		mo->min_chain_score = 100; mo->pri_ratio = 0.0f; mo->max_chain_skip = 25;
		mo->bw = mo->bw_long = 2000; mo->occ_dist = 0;
		return 0;
	}
	if (p == "asm5" || p == "asm10" || p == "asm20") {
		io->flag = 0; io->k = 19; io->w = 19;
		mo->bw = 1000; mo->bw_long = 100000; mo->max_gap = 10000;
		mo->flag |= MMF_RMQ;
		mo->min_mid_occ = 50; mo->max_mid_occ = 500; mo->min_dp_max = 200; mo->best_n = 50;
		if (p == "asm5") { mo->a = 1; mo->b = 19; mo->q = 39; mo->q2 = 81; mo->e = 3; mo->e2 = 1; mo->zdrop = mo->zdrop_inv = 200; }
		else if (p == "asm10") { mo->a = 1; mo->b = 9; mo->q = 16; mo->q2 = 41; mo->e = 2; mo->e2 = 1; mo->zdrop = mo->zdrop_inv = 200; }
		else if (p == "asm20") { mo->a = 1; mo->b = 4; mo->q = 6; mo->q2 = 26; mo->e = 2; mo->e2 = 1; mo->zdrop = mo->zdrop_inv = 200; io->w = 10; }
		else return MM355_EINVAL;
		return 0;
	}
	if (p == "map-pb" || p == "map10k") {   // homopolymer-compressed minimizers (MM_I_HPC = 1), U:options.c::mm_set_opt
		io->flag |= 1; io->k = 19;
		return 0;
	}
	if (p == "ava-pb") {
		io->flag |= 1; io->k = 19; io->w = 5;
		mo->flag |= 0x800000LL | 0x001LL | 0x002LL | 0x400LL;   // ALL_CHAINS | NO_DIAG | NO_DUAL | NO_LJOIN, as ava-ont
		mo->min_chain_score = 100; mo->pri_ratio = 0.0f; mo->max_chain_skip = 25;
		mo->bw_long = mo->bw; mo->occ_dist = 0;
		return 0;
	}
	// known minimap2 2.26 presets that are outside the long-read hot path (short reads, spliced): nothing is modified, the
	// caller gets MM355_EUNSUP and must refuse (mappy_rs.Aligner raises)
	static const char *const unsup[] = { "sr", "short", "splice", "splice:hq", "cdna", 0 };
	for (int i = 0; unsup[i]; ++i) if (p == unsup[i]) return MM355_EUNSUP;
	return MM355_EINVAL;   // unknown name: options untouched, as U:options.c::mm_set_opt's -1 (the reference ignores it, lib.rs:336)
}

int32_t mm355_index_cal_max_occ(const mm355_index *mi, float f)
{
	if (f <= 0.) return INT32_MAX;
	size_t n = (size_t)mi->n_distinct;
	if (n == 0) return INT32_MAX;
	if (mi->dev_resident) {   // k-th smallest == (n-1-k)-th largest of the saved descending tail
		size_t kk = (uint32_t)((1. - f) * n);
		if (kk >= n) kk = n - 1;
		size_t from_top = n - 1 - kk;
		if (from_top >= mi->top_counts.size()) return mi->top_counts.empty()? INT32_MAX : (int32_t)(mi->top_counts.back() + 1);
		return (int32_t)(mi->top_counts[from_top] + 1);
	}
	std::vector<uint32_t> a; a.reserve(n);
	for (const mm355_slot &s : mi->slots)
		if (s.key != UINT64_MAX) a.push_back(s.key & 1? 1u : (uint32_t)s.val);
	size_t kk = (uint32_t)((1. - f) * n);
	if (kk >= a.size()) kk = a.size() - 1;
	std::nth_element(a.begin(), a.begin() + kk, a.end());
	return (int32_t)(a[kk] + 1);
}

extern "C" int mm355_mapopt_update(mm355_mapopt_t *opt, const mm355_index_t *mi)
{
	if (mi == 0) return MM355_ENOIDX;
	if (opt->mid_occ <= 0) {
		opt->mid_occ = mm355_index_cal_max_occ(mi, opt->mid_occ_frac);
		if (opt->mid_occ < opt->min_mid_occ) opt->mid_occ = opt->min_mid_occ;
		if (opt->max_mid_occ > opt->min_mid_occ && opt->mid_occ > opt->max_mid_occ) opt->mid_occ = opt->max_mid_occ;
	}
	if (opt->bw_long < opt->bw) opt->bw_long = opt->bw;
	return 0;
}

// ------------------------------------------------------------------ flat table
static void table_insert(mm355_index *mi, uint64_t minier, bool single, uint64_t val)
{
	uint64_t mask = mi->n_lines - 1, line = mm_table_hash(minier) & mask;
	for (;;) {
		mm355_slot *ln = &mi->slots[line * MM355_SLOTS_PER_LINE];
		for (int q = 0; q < MM355_SLOTS_PER_LINE; ++q)
			if (ln[q].key == UINT64_MAX) { ln[q].key = minier << 1 | (single? 1 : 0); ln[q].val = val; return; }
		line = (line + 1) & mask;
	}
}

static void table_alloc(mm355_index *mi, uint64_t n_keys)
{
	uint64_t want = (uint64_t)(n_keys / 0.55) + MM355_SLOTS_PER_LINE, n_lines = 1;
	while (n_lines * MM355_SLOTS_PER_LINE < want) n_lines <<= 1;
	mi->n_lines = n_lines;
	mm355_slot empty = { UINT64_MAX, 0 };
	mi->slots.assign(n_lines * MM355_SLOTS_PER_LINE, empty);
}

// pairs: x = minimizer value (hash, 2k bits), y = rid<<32|pos<<1|strand.  Sorted here by (x, y): positions of
// one minimizer end up ascending, which is the order U:index.c::worker_post leaves in p[] (radix_sort_64).
int mm355_index_from_pairs(mm355_index *mi, std::vector<mm128> &a)
{
	std::sort(a.begin(), a.end(), [](const mm128 &p, const mm128 &q) { return p.x < q.x || (p.x == q.x && p.y < q.y); });
	uint64_t n_keys = 0, n_multi = 0;
	for (size_t i = 0; i < a.size();) {
		size_t j = i + 1;
		while (j < a.size() && a[j].x == a[i].x) ++j;
		++n_keys; if (j - i > 1) n_multi += j - i;
		i = j;
	}
	table_alloc(mi, n_keys);
	mi->pos.clear(); mi->pos.reserve(n_multi);
	for (size_t i = 0; i < a.size();) {
		size_t j = i + 1;
		while (j < a.size() && a[j].x == a[i].x) ++j;
		if (j - i == 1) table_insert(mi, a[i].x, true, a[i].y);
		else {
			uint64_t off = mi->pos.size();
			for (size_t k = i; k < j; ++k) mi->pos.push_back(a[k].y);
			table_insert(mi, a[i].x, false, off << 32 | (uint64_t)(j - i));
		}
		i = j;
	}
	mi->n_minimizers = (int64_t)a.size(); mi->n_distinct = (int64_t)n_keys;
	return 0;
}

// ------------------------------------------------------------------ MMI\2 reader (U:index.c::mm_idx_load)
void mm355_index_set_header(mm355_index *mi, MmiHeader &hd)
{
	mi->w = hd.w, mi->k = hd.k, mi->b = hd.b, mi->n_seq = hd.n_seq, mi->flag = hd.flag;
	mi->names.swap(hd.names); mi->seq_off.swap(hd.seq_off); mi->seq_len.swap(hd.seq_len);
}

static mm355_index *load_mmi(FILE *fp)
{
	MmiHeader hd;
	if (mmi_read_header(fp, &hd) != 0) return 0;   // (magic, the ranges of w, k and b, the contig table: mm355_mmiwalk.h)
	mm355_index *mi = new mm355_index();
	mm355_index_set_header(mi, hd);
	const uint64_t sum_len = hd.sum_len;
	// buckets -> (minimizer, positions); collected first to size the flat table
	struct Ent { uint64_t minier, val; uint32_t n; };
	std::vector<Ent> ents;
	std::vector<uint64_t> pos;
	for (uint64_t i = 0; i < 1ULL << mi->b; ++i) {
		int32_t n; uint32_t size;
		if (fread(&n, 4, 1, fp) != 1) { delete mi; return 0; }
		uint64_t base = pos.size();
		pos.resize(base + (n > 0? n : 0));
		if (n > 0 && fread(&pos[base], 8, n, fp) != (size_t)n) { delete mi; return 0; }
		if (fread(&size, 4, 1, fp) != 1) { delete mi; return 0; }
		for (uint32_t j = 0; j < size; ++j) {
			uint64_t kv[2];
			if (fread(kv, 8, 2, fp) != 2) { delete mi; return 0; }
			Ent e; e.minier = (kv[0] >> 1) << mi->b | i;
			if (kv[0] & 1) e.n = 1, e.val = kv[1];
			else e.n = (uint32_t)kv[1], e.val = base + (kv[1] >> 32);
			ents.push_back(e);
		}
	}
	table_alloc(mi, ents.size());
	mi->pos.swap(pos);
	int64_t tot = 0;
	for (const Ent &e : ents) {
		if (e.n == 1) table_insert(mi, e.minier, true, e.val);
		else table_insert(mi, e.minier, false, e.val << 32 | e.n);
		tot += e.n;
	}
	mi->n_minimizers = tot; mi->n_distinct = (int64_t)ents.size();
	if (!(mi->flag & 2)) {
		size_t n = (sum_len + 7) / 8;
		mi->S.resize(n? n : 1);
		if (fread(mi->S.data(), 4, n, fp) != n) { delete mi; return 0; }
	}
	return mi;
}

// ------------------------------------------------------------------ builder (U:index.c::mm_idx_gen)
struct HostBase { const char *s; int operator()(int i) const { return mm_nt4((uint8_t)s[i]); } };

static void sketch_contig(const char *s, int64_t len, int w, int k, uint32_t rid, bool is_hpc, std::vector<mm128> &out)
{
	if (len <= 0) return;
	std::vector<mm128> ring(w);
	std::vector<mm128> tmp((size_t)len);
	HostBase hb = { s };
	int64_t n = mm_sketch_seq(hb, (int)len, w, k, rid, tmp.data(), len, ring.data(), 1, is_hpc);
	for (int64_t i = 0; i < n; ++i) { mm128 m; m.x = tmp[i].x >> 8; m.y = tmp[i].y; out.push_back(m); }
}

static mm355_index *build_from_seqs(const mm355_idxopt_t *io, int n_seq, const char *const *seqs, const int64_t *lens, const char *const *names, int n_threads)
{
	mm355_index *mi = new mm355_index();
	mi->w = io->w < 1? 1 : io->w; mi->k = io->k; mi->b = io->bucket_bits; mi->flag = io->flag; mi->n_seq = n_seq;
	if (mi->k * 2 < mi->b) mi->b = mi->k * 2;
	uint64_t sum_len = 0;
	for (int i = 0; i < n_seq; ++i) {
		mi->names.emplace_back(names && names[i]? names[i] : "");
		mi->seq_off.push_back(sum_len); mi->seq_len.push_back((uint32_t)lens[i]);
		sum_len += lens[i];
	}
	mi->S.assign((sum_len + 7) / 8 + 1, 0);
	for (int i = 0; i < n_seq; ++i)
		for (int64_t j = 0; j < lens[i]; ++j) { uint64_t o = mi->seq_off[i] + j; int c = mm_nt4((uint8_t)seqs[i][j]); mm_seq4_set(mi->S.data(), o, c); }
	// sketch contigs on host threads (a contig is sequential; contigs are independent)
	if (n_threads < 1) n_threads = 1;
	std::vector<std::vector<mm128>> parts(n_seq);
	std::atomic<int> next(0);
	auto work = [&]() { for (;;) { int i = next.fetch_add(1); if (i >= n_seq) break; sketch_contig(seqs[i], lens[i], mi->w, mi->k, (uint32_t)i, (mi->flag & 1) != 0, parts[i]); } };
	std::vector<std::thread> th;
	for (int t = 1; t < n_threads && t < n_seq; ++t) th.emplace_back(work);
	work();
	for (auto &t : th) t.join();
	std::vector<mm128> all;
	size_t tot = 0; for (auto &p : parts) tot += p.size();
	all.reserve(tot);
	for (auto &p : parts) { all.insert(all.end(), p.begin(), p.end()); std::vector<mm128>().swap(p); }
	mm355_index_from_pairs(mi, all);
	return mi;
}

// FASTA/FASTQ, plain or gzip-compressed (U:bseq.c reads through zlib's gzFile, which passes plain files through unchanged).  One record
// loop serves the index builders (parse_fastx: the whole file) and the streaming reader of read sets (mm355_fastx_next).  The bytes come
// through a ByteSource (mm355_bamread.h): zlib here, or the device inflater's stream (mm355_inflate.hip: mm355_fastx_open_device).
struct GzSource : ByteSource {
	gzFile gz;
	explicit GzSource(gzFile g) : gz(g) { (void)gzbuffer(gz, 1 << 20); }
	~GzSource() { gzclose(gz); }
	int64_t read(void *buf, size_t cap)
	{
		const int r = gzread(gz, buf, (unsigned)cap);
		if (r > 0) return r;
		int zerr = 0; (void)gzerror(gz, &zerr);
		return r < 0 || (zerr != Z_OK && zerr != Z_STREAM_END)? MM355_EIO : 0;   // truncated / corrupt gzip stream
	}
};

struct mm355_fastx {
	ByteSource *src = 0;
	int io_err = 0;                       // the source's error: the stream ended there
	// mm355_fastx_next only: the stream's first four bytes have been looked at; "BAM\1": the BAM loop of mm355_bamread.h reads it (header_done: its header is behind)
	bool sniffed = false, is_bam = false, header_done = false;
	std::string line, next_name;          // line: a line that straddles two blocks; next_name: the header line that ended the previous record
	std::vector<char> buf = std::vector<char>(1 << 20);   // the file is read in blocks and cut into lines here (gzgets costs a call and a strlen per line)
	size_t pos = 0, end = 0;
	bool in_qual = false, is_fq = false, eof = false, have_next = false;
	size_t l_qual = 0; int64_t n_rec = 0;
	// mm355_fastx_next only: the record that did not fit the previous sub-batch, and the error the reader stopped at
	std::string held_name, held_seq; bool held = false; int err = 0;
	// mm355_fastx_open_qual: the quality of the record fastx_record has just returned (has_qual: a FASTQ record with a '+' line), and the held record's
	bool keep_qual = false, has_qual = false, held_has_qual = false; std::string qual, held_qual;
	// mm355_fastx_keep_aux: the tags to keep from a BAM's records (empty: none), the aux of the record reads_record has just returned as
	// bam_aux_split left it, and the held record's; started: mm355_fastx_next has been called.  rg: the @RG lines of a BAM's header text
	std::string keep_aux, aux, held_aux, rg; int32_t aux_mod = 0, held_aux_mod = 0; bool started = false;
	~mm355_fastx() { delete src; }
};

// the next block of the stream into the (used up) buffer; false at the end, or at the source's error
static bool fastx_refill(mm355_fastx *fx)
{
	fx->pos = fx->end = 0;
	int64_t r = fx->eof? 0 : fx->src->read(fx->buf.data(), fx->buf.size());
	if (r < 0) { fx->io_err = (int)r; r = 0; }
	if (r == 0) { fx->eof = true; return false; }
	fx->end = (size_t)r;
	return true;
}

// the next line of any length, without its line end (LF or CRLF): *p / *n point into the block, or into fx->line when the line straddles blocks.
// false at the end of the file (a last line without a newline is returned first)
static bool fastx_line(mm355_fastx *fx, const char **p, size_t *n)
{
	bool joined = false;
	for (;;) {
		const char *beg = fx->buf.data() + fx->pos;
		const char *nl = fx->end > fx->pos? (const char*)memchr(beg, '\n', fx->end - fx->pos) : 0;
		if (nl) {
			if (joined) { fx->line.append(beg, (size_t)(nl - beg)); *p = fx->line.data(); *n = fx->line.size(); }
			else { *p = beg; *n = (size_t)(nl - beg); }
			fx->pos = (size_t)(nl + 1 - fx->buf.data());
			break;
		}
		if (!joined) { fx->line.clear(); joined = true; }
		fx->line.append(beg, fx->end - fx->pos);
		if (!fastx_refill(fx)) {
			if (fx->line.empty()) return false;
			*p = fx->line.data(); *n = fx->line.size();
			break;
		}
	}
	while (*n > 0 && ((*p)[*n - 1] == '\n' || (*p)[*n - 1] == '\r')) --*n;
	return true;
}

// the next record: 1, name filled and the bases APPENDED to seq (a sub-batch collects its reads back to back without a copy); 0 at the end of the
// file; MM355_EIO when the gzip stream is truncated or corrupt (the records before that point have been handed out by then: a caller that must
// not use them checks the last return value)
static int fastx_record(mm355_fastx *fx, std::string &name, std::string &seq)
{
	const size_t start = seq.size();
	bool have = false;
	if (fx->keep_qual) { fx->qual.clear(); fx->has_qual = false; }
	if (fx->have_next) { name.swap(fx->next_name); fx->have_next = false; have = true; }
	const char *line; size_t n;
	while (fastx_line(fx, &line, &n)) {
		if (fx->in_qual) { if (fx->keep_qual) fx->qual.append(line, n); fx->l_qual += n; if (fx->l_qual >= seq.size() - start) fx->in_qual = false; continue; }
		if (n > 0 && (line[0] == '>' || (line[0] == '@' && (fx->n_rec == 0 || fx->is_fq)))) {
			fx->is_fq = line[0] == '@';
			size_t e = 1; while (e < n && line[e] != ' ' && line[e] != '\t') ++e;
			++fx->n_rec;
			if (have) { fx->next_name.assign(line + 1, e - 1); fx->have_next = true; return 1; }
			name.assign(line + 1, e - 1); have = true;
		} else if (n > 0 && line[0] == '+' && fx->is_fq) { fx->in_qual = have && seq.size() > start; fx->l_qual = 0; if (have) fx->has_qual = true; }
		else if (have) {
			size_t n_blank = 0;
			for (size_t i = 0; i < n; ++i) n_blank += line[i] <= ' ';
			if (n_blank == 0) seq.append(line, n);      // (the usual line: one copy)
			else for (size_t i = 0; i < n; ++i) if (line[i] > ' ') seq.push_back(line[i]);
		}
	}
	if (fx->io_err) return MM355_EIO;   // truncated / corrupt stream: no garbage index, no half a read set
	return have? 1 : 0;
}

// the stream as the BAM loop takes it: n bytes to dst (0: skipped), fewer at the end
struct FastxTake {
	mm355_fastx *fx;
	int64_t take(void *dst, size_t n)
	{
		size_t got = 0;
		while (got < n) {
			if (fx->pos == fx->end && !fastx_refill(fx)) break;
			const size_t k = std::min(n - got, fx->end - fx->pos);
			if (dst) memcpy((char*)dst + got, fx->buf.data() + fx->pos, k);
			fx->pos += k; got += k;
		}
		return (int64_t)got;
	}
	int err() const { return fx->io_err; }
};

// fastx_record for the streaming reader: a stream that begins "BAM\1" gives its records as reads (fx->qual, fx->has_qual: the record's quality)
// the stream's first bytes looked at and, for a BAM, its header read: 0, or MM355_EIO (fx->is_bam says which loop reads the records)
// (want_rg: the header text goes through the @RG filter; otherwise it is skipped as before)
static int reads_begin(mm355_fastx *fx, bool want_rg)
{
	if (!fx->sniffed) {
		fx->sniffed = true;
		while (fx->end < 4 && !fx->eof) {                        // (the buffer is empty: nothing has been read)
			int64_t r = fx->src->read(fx->buf.data() + fx->end, fx->buf.size() - fx->end);
			if (r < 0) { fx->io_err = (int)r; r = 0; }
			if (r == 0) fx->eof = true;
			fx->end += (size_t)r;
		}
		fx->is_bam = fx->end >= 4 && memcmp(fx->buf.data(), "BAM\1", 4) == 0;
	}
	if (fx->is_bam && !fx->header_done) {
		FastxTake t = { fx };
		if (bam_read_header(t, want_rg? &fx->rg : (std::string*)0)) return MM355_EIO;
		fx->header_done = true;
	}
	return 0;
}

static int reads_record(mm355_fastx *fx, std::string &name, std::string &seq)
{
	if (reads_begin(fx, !fx->keep_aux.empty())) return MM355_EIO;
	if (!fx->is_bam) return fastx_record(fx, name, seq);
	FastxTake t = { fx };
	return bam_read_record(t, name, seq, fx->qual, &fx->has_qual, fx->keep_aux.empty()? (const char*)0 : fx->keep_aux.c_str(), fx->aux, &fx->aux_mod);
}

static bool parse_fastx(const char *path, std::vector<std::string> &names, std::vector<std::string> &seqs)
{
	mm355_fastx fx;
	gzFile gz = gzopen(path, "rb");
	if (gz == 0) return false;
	fx.src = new GzSource(gz);
	std::string name, seq;
	int rc;
	while ((rc = fastx_record(&fx, name, seq)) == 1) { names.push_back(name); seqs.emplace_back(); seqs.back().swap(seq); }
	return rc == 0 && !names.empty();
}

extern "C" int mm355_fastx_open(const char *path, mm355_fastx_t **out)
{
	*out = 0;
	if (path == 0) return MM355_EINVAL;
	gzFile gz = gzopen(path, "rb");
	if (gz == 0) return MM355_EIO;
	*out = mm355_fastx_from_source(new GzSource(gz), false);
	return 0;
}

mm355_fastx *mm355_fastx_from_source(ByteSource *src, bool keep_qual)
{
	mm355_fastx *fx = new mm355_fastx();
	fx->src = src; fx->keep_qual = keep_qual;
	return fx;
}

extern "C" int mm355_fastx_open_qual(const char *path, mm355_fastx_t **out)
{
	const int rc = mm355_fastx_open(path, out);
	if (rc == 0) (*out)->keep_qual = true;
	return rc;
}

extern "C" void mm355_fastx_close(mm355_fastx_t *fx) { delete fx; }

extern "C" int mm355_fastx_keep_aux(mm355_fastx_t *fx, const char *tags)
{
	if (fx == 0 || fx->started || (tags && !bam_aux_keep_ok(tags))) return MM355_EINVAL;
	fx->keep_aux = tags? tags : "";
	return 0;
}

extern "C" const char *mm355_fastx_bam_rg(mm355_fastx_t *fx, int64_t *len)
{
	if (len) *len = 0;
	if (fx == 0 || fx->err) return 0;
	if (reads_begin(fx, true)) { fx->err = MM355_EIO; return 0; }    // (mm355_fastx_next reports it)
	if (!fx->is_bam || fx->rg.empty()) return 0;
	if (len) *len = (int64_t)fx->rg.size();
	return fx->rg.c_str();
}

extern "C" int mm355_bam_aux_split(const uint8_t *aux, int32_t n, const char *keep, uint8_t *out, int32_t *n_out, int32_t *mod_off)
{
	return bam_aux_split(aux, n, keep, out, n_out, mod_off);
}

// a sub-batch of reads and everything its pointers point to (mm355_reads_t is its first member: mm355_reads_free gets the box back)
struct ReadsBox {
	mm355_reads_t r;
	std::string seq_bytes, name_bytes;       // sequences back to back; names, each with its NUL
	std::vector<size_t> seq_at, name_at;
	std::vector<const char*> sp, np; std::vector<int32_t> ln;
	// a reader that keeps quality: the strings back to back, qual_at[i] < 0 for a record without one (FASTA, or a length other than the sequence's)
	bool keep_qual = false; std::string qual_bytes; std::vector<int64_t> qual_at; std::vector<const char*> qp;
	// a BAM reader that keeps aux: the filtered blocks back to back, every read has one (of length 0 where nothing was kept)
	bool keep_aux = false; std::string aux_bytes; std::vector<size_t> aux_at; std::vector<int32_t> aux_len, aux_mod; std::vector<const uint8_t*> ap;
};

extern "C" void mm355_reads_free(mm355_reads_t *r) { delete (ReadsBox*)r; }
extern "C" const char *const *mm355_reads_quals(const mm355_reads_t *r) { const ReadsBox *B = (const ReadsBox*)r; return B && B->keep_qual? B->qp.data() : 0; }

extern "C" const uint8_t *const *mm355_reads_aux(const mm355_reads_t *r, const int32_t **aux_len, const int32_t **aux_mod)
{
	const ReadsBox *B = (const ReadsBox*)r;
	const bool on = B && B->keep_aux;
	if (aux_len) *aux_len = on? B->aux_len.data() : 0;
	if (aux_mod) *aux_mod = on? B->aux_mod.data() : 0;
	return on? B->ap.data() : 0;
}

extern "C" int mm355_fastx_next(mm355_fastx_t *fx, int64_t max_reads, int64_t max_bases, mm355_reads_t **out)
{
	*out = 0;
	if (fx == 0 || max_reads < 1 || max_bases < 1) return MM355_EINVAL;
	fx->started = true;
	if (fx->err) return fx->err;
	ReadsBox *B = new ReadsBox();
	B->keep_qual = fx->keep_qual;
	std::string name, qual, aux; bool has_qual = false; int32_t aux_mod = 0;
	while ((int64_t)B->ln.size() < max_reads) {
		const size_t at = B->seq_bytes.size();
		if (fx->held) { name.swap(fx->held_name); B->seq_bytes += fx->held_seq; fx->held_seq.clear(); fx->held = false; qual.swap(fx->held_qual); has_qual = fx->held_has_qual;
			aux.swap(fx->held_aux); aux_mod = fx->held_aux_mod; }
		else {
			const int rc = reads_record(fx, name, B->seq_bytes);      // (the bases land behind the sub-batch's other reads)
			if (rc == 0) break;
			if (rc < 0) { fx->err = rc; break; }
			if (B->seq_bytes.size() - at >= (size_t)1 << 31) { fx->err = MM355_EINVAL; break; }
			if (fx->keep_qual) { qual.swap(fx->qual); has_qual = fx->has_qual; }
			if (!fx->keep_aux.empty() && fx->is_bam) { aux.swap(fx->aux); aux_mod = fx->aux_mod; }
		}
		if (!B->ln.empty() && (int64_t)B->seq_bytes.size() > max_bases) {   // over the base limit and not the first: it opens the next sub-batch
			fx->held_name.swap(name); fx->held_seq.assign(B->seq_bytes, at, std::string::npos); fx->held = true;
			fx->held_qual.swap(qual); fx->held_has_qual = has_qual;
			fx->held_aux.swap(aux); fx->held_aux_mod = aux_mod;
			B->seq_bytes.resize(at);
			break;
		}
		B->seq_at.push_back(at);
		B->name_at.push_back(B->name_bytes.size()); B->name_bytes.append(name.c_str(), name.size() + 1);
		B->ln.push_back((int32_t)(B->seq_bytes.size() - at));
		if (fx->keep_qual) {
			const bool ok = has_qual && qual.size() == B->seq_bytes.size() - at;
			B->qual_at.push_back(ok? (int64_t)B->qual_bytes.size() : -1);
			if (ok) B->qual_bytes += qual;
		}
		if (!fx->keep_aux.empty() && fx->is_bam) {
			B->keep_aux = true;
			B->aux_at.push_back(B->aux_bytes.size()); B->aux_len.push_back((int32_t)aux.size()); B->aux_mod.push_back(aux_mod);
			B->aux_bytes += aux;
		}
	}
	if (fx->err || B->ln.empty()) { delete B; return fx->err; }
	for (size_t i = 0; i < B->ln.size(); ++i) { B->sp.push_back(B->seq_bytes.data() + B->seq_at[i]); B->np.push_back(B->name_bytes.data() + B->name_at[i]); }
	for (size_t i = 0; i < B->qual_at.size(); ++i) B->qp.push_back(B->qual_at[i] < 0? (const char*)0 : B->qual_bytes.data() + B->qual_at[i]);
	for (size_t i = 0; i < B->aux_at.size(); ++i) B->ap.push_back((const uint8_t*)B->aux_bytes.data() + B->aux_at[i]);
	B->r.n = (int64_t)B->ln.size(); B->r.seqs = B->sp.data(); B->r.lens = B->ln.data(); B->r.names = B->np.data();
	*out = &B->r;
	return 0;
}

// the parsed records as the pointer arrays the builders take (they point into names / seqs)
struct FastxView {
	std::vector<const char*> sp, np; std::vector<int64_t> ln;
	FastxView(const std::vector<std::string> &names, const std::vector<std::string> &seqs) {
		for (size_t i = 0; i < names.size(); ++i) { sp.push_back(seqs[i].data()); np.push_back(names[i].c_str()); ln.push_back((int64_t)seqs[i].size()); }
	}
};

static mm355_index *build_from_fastx(const char *path, const mm355_idxopt_t *io, int n_threads)
{
	std::vector<std::string> names, seqs;
	if (!parse_fastx(path, names, seqs)) return 0;
	FastxView v(names, seqs);
	return build_from_seqs(io, (int)names.size(), v.sp.data(), v.ln.data(), v.np.data(), n_threads);
}

void mm355_index_finish_names(mm355_index *mi)
{
	for (uint32_t i = 0; i < mi->n_seq; ++i) mi->name2id.emplace(mi->names[i], (int)i);   // first wins, as a hash put would report a duplicate
	mm355_name_ranks(mi->names, mi->names_sorted, mi->name_rank);
}

extern "C" int mm355_index_load(const char *path, const mm355_idxopt_t *io, int n_threads, mm355_index_t **out)
{
	*out = 0;
	FILE *fp = fopen(path, "rb");
	if (fp == 0) return MM355_EIO;
	char magic[4]; size_t n = fread(magic, 1, 4, fp);
	rewind(fp);
	mm355_index *mi = 0;
	if (n == 4 && strncmp(magic, "MMI\2", 4) == 0) mi = load_mmi(fp);
	else if (n > 0) {
		fclose(fp); fp = 0;
		if (io->k <= 0 || io->k > 28 || io->w <= 0 || io->w >= 256) return MM355_EINVAL;
		mi = build_from_fastx(path, io, n_threads);
	}
	if (fp) fclose(fp);
	if (mi == 0 || mi->n_seq == 0) { delete mi; return MM355_EIO; }
	mm355_index_finish_names(mi);
	*out = mi;
	return 0;
}

void mm355_runtime_init(void);   // mm355_ctx.cpp

// the FASTA / FASTQ branch of mm355_index_load with the build on GPU `device` (mm355_idxbuild.hip); an .mmi has nothing to build
extern "C" int mm355_index_load_device(const char *path, const mm355_idxopt_t *io, int device, mm355_index_t **out)
{
	*out = 0;
	mm355_runtime_init();   // (this entry can be the first HIP user of the process)
	FILE *fp = fopen(path, "rb");
	if (fp == 0) return MM355_EIO;
	char magic[4]; size_t n = fread(magic, 1, 4, fp);
	fclose(fp);
	if (n == 4 && strncmp(magic, "MMI\2", 4) == 0) return mm355_index_load(path, io, 1, out);
	if (n == 0) return MM355_EIO;
	if (io->k <= 0 || io->k > 28 || io->w <= 0 || io->w >= 256) return MM355_EINVAL;
	if (device < 0) return MM355_ENODEV;
	std::vector<std::string> names, seqs;
	if (!parse_fastx(path, names, seqs)) return MM355_EIO;
	FastxView v(names, seqs);
	return mm355_index_build_device(io, (int)names.size(), (const uint8_t *const *)v.sp.data(), v.ln.data(), v.np.data(), device, out);
}

// ------------------------------------------------------------------ MMI\2 writer (U:index.c::mm_idx_dump; the layout and the canonical
// order are stated in include/mm355.h)
// The bucket sections of an index with a host image: the occupied slots ordered by (bucket, key), p[] re-laid in that order.
static int dump_buckets_host(const mm355_index *mi, FILE *fp)
{
	struct Ent { uint64_t bucket, key, val; };   // key as in the file: minimizer>>b<<1 | singleton
	const uint64_t mask = (1ULL << mi->b) - 1;
	std::vector<Ent> ents; ents.reserve((size_t)mi->n_distinct);
	for (const mm355_slot &s : mi->slots)
		if (s.key != UINT64_MAX) { const uint64_t minier = s.key >> 1; ents.push_back(Ent{ minier & mask, minier >> mi->b << 1 | (s.key & 1), s.val }); }
	std::sort(ents.begin(), ents.end(), [](const Ent &p, const Ent &q) { return p.bucket < q.bucket || (p.bucket == q.bucket && p.key < q.key); });
	std::vector<uint64_t> p, kv;
	size_t i = 0;
	for (uint64_t bkt = 0; bkt <= mask; ++bkt) {
		p.clear(); kv.clear();
		for (; i < ents.size() && ents[i].bucket == bkt; ++i) {
			const Ent &e = ents[i];
			kv.push_back(e.key);
			if (e.key & 1) { kv.push_back(e.val); continue; }
			const uint64_t start = e.val >> 32, cnt = (uint32_t)e.val;
			kv.push_back((uint64_t)p.size() << 32 | cnt);
			p.insert(p.end(), mi->pos.begin() + start, mi->pos.begin() + start + cnt);
		}
		if (p.size() > (size_t)INT32_MAX) return MM355_EUNSUP;   // the file's n is an int32, as minimap2's
		const int32_t n = (int32_t)p.size(); const uint32_t size = (uint32_t)(kv.size() / 2);
		fwrite(&n, 4, 1, fp); fwrite(p.data(), 8, p.size(), fp);
		fwrite(&size, 4, 1, fp); fwrite(kv.data(), 8, kv.size(), fp);
	}
	return 0;
}

extern "C" int mm355_index_dump(const mm355_index_t *mi, const char *path)
{
	if (mi == 0) return MM355_ENOIDX;
	if (path == 0) return MM355_EINVAL;
	for (const std::string &nm : mi->names) if (nm.size() > 255) return MM355_EINVAL;   // minimap2 would truncate the name silently
	FILE *fp = fopen(path, "wb");
	if (fp == 0) return MM355_EIO;
	(void)setvbuf(fp, 0, _IOFBF, 1 << 20);
	const uint32_t x[5] = { (uint32_t)mi->w, (uint32_t)mi->k, (uint32_t)mi->b, mi->n_seq, (uint32_t)mi->flag };
	fwrite("MMI\2", 1, 4, fp); fwrite(x, 4, 5, fp);
	uint64_t sum_len = 0;
	for (uint32_t i = 0; i < mi->n_seq; ++i) {
		const uint8_t l = (uint8_t)mi->names[i].size();
		fwrite(&l, 1, 1, fp); fwrite(mi->names[i].data(), 1, l, fp); fwrite(&mi->seq_len[i], 4, 1, fp);
		sum_len += mi->seq_len[i];
	}
	int rc = mi->dev_resident? mm355_index_dump_buckets_device(mi, fp) : dump_buckets_host(mi, fp);
	if (rc == 0 && !(mi->flag & 2)) {
		const size_t n = (sum_len + 7) / 8;
		if (mi->S.size() < n) rc = MM355_EINVAL; else fwrite(mi->S.data(), 4, n, fp);
	}
	if (rc == 0 && (fflush(fp) != 0 || ferror(fp))) rc = MM355_EIO;   // (a failed fwrite leaves the stream's error flag set)
	if (fclose(fp) != 0 && rc == 0) rc = MM355_EIO;
	if (rc) remove(path);
	return rc;
}

extern "C" int mm355_index_build(const mm355_idxopt_t *io, int n_seq, const char *const *seqs, const int64_t *lens, const char *const *names, int n_threads, mm355_index_t **out)
{
	*out = 0;
	if (n_seq <= 0) return MM355_EINVAL;
	if (io->k <= 0 || io->k > 28 || io->w <= 0 || io->w >= 256) return MM355_EINVAL;   // U:sketch.c::mm_sketch asserts the same ranges
	mm355_index *mi = build_from_seqs(io, n_seq, seqs, lens, names, n_threads);
	if (mi == 0) return MM355_EINVAL;
	mm355_index_finish_names(mi);
	*out = mi;
	return 0;
}

extern "C" void mm355_index_free(mm355_index_t *mi) { if (mi) mm355_index_free_replicas(mi); delete mi; }

extern "C" int mm355_index_info(const mm355_index_t *mi, int32_t *k, int32_t *w, int32_t *b, int32_t *flag, uint32_t *n_seq)
{
	if (mi == 0) return MM355_ENOIDX;
	if (k) *k = mi->k; if (w) *w = mi->w; if (b) *b = mi->b; if (flag) *flag = mi->flag; if (n_seq) *n_seq = mi->n_seq;
	return 0;
}
extern "C" const char *mm355_index_seq_name(const mm355_index_t *mi, uint32_t rid) { return mi && rid < mi->n_seq? mi->names[rid].c_str() : 0; }
extern "C" int64_t mm355_index_seq_len(const mm355_index_t *mi, uint32_t rid) { return mi && rid < mi->n_seq? (int64_t)mi->seq_len[rid] : -1; }
extern "C" int mm355_index_name2id(const mm355_index_t *mi, const char *name)
{
	if (mi == 0) return -2;
	auto it = mi->name2id.find(name);
	return it == mi->name2id.end()? -1 : it->second;
}
// U:index.c::mm_idx_getseq
extern "C" int mm355_index_getseq(const mm355_index_t *mi, uint32_t rid, uint32_t st, uint32_t en, uint8_t *seq)
{
	if (mi == 0 || (mi->flag & 2)) return -1;
	if (rid >= mi->n_seq || st >= mi->seq_len[rid]) return -1;
	if (en > mi->seq_len[rid]) en = mi->seq_len[rid];
	uint64_t st1 = mi->seq_off[rid] + st, en1 = mi->seq_off[rid] + en;
	for (uint64_t i = st1; i < en1; ++i) seq[i - st1] = mm_seq4_get(mi->S.data(), i);
	return (int)(en - st);
}
extern "C" int mm355_index_stat(const mm355_index_t *mi, int64_t *n_minimizers, int64_t *n_distinct, int64_t *table_bytes, int64_t *pos_bytes)
{
	if (mi == 0) return MM355_ENOIDX;
	if (n_minimizers) *n_minimizers = mi->n_minimizers;
	if (n_distinct) *n_distinct = mi->n_distinct;
	if (table_bytes) *table_bytes = (int64_t)(mi->dev_resident? mi->n_lines * MM355_SLOTS_PER_LINE : mi->slots.size()) * 16;
	if (pos_bytes) *pos_bytes = (int64_t)(mi->dev_resident? mi->n_pos : mi->pos.size()) * 8;
	return 0;
}

// host-side diagnostic view of mm_idx_get on the flat table (the product path looks up on the device: k_seed_lookup)
extern "C" int mm355_index_get(const mm355_index_t *mi, uint64_t minier, uint64_t *vals, int cap)
{
	if (mi == 0) return MM355_ENOIDX;
	if (mi->dev_resident) return MM355_EUNSUP;   // the table of a device-built index exists only in HBM
	uint64_t v = 0;
	uint32_t n = mm355_host_get(mi, minier, &v);
	if (n == 1) { if (cap > 0) vals[0] = v; }
	else for (uint32_t i = 0; i < n && (int)i < cap; ++i) vals[i] = mi->pos[v + i];
	return (int)n;
}
