// bam_host.cpp -- the host side of the BAM writer as a stand-alone program (g++ alone, AddressSanitizer + UBSan; tests/test_bam_host.py):
//   codes                    bam_code of all 256 byte values forwards, then on the reverse strand, as 2 x 512 hex digits
//   sets <in> <out>          result sets written by the test (tests/_sam_sets.py::serialize) -> per set n_text, n_lines, line_off and the BGZF
//                            bytes of the host formatter; checks on every set that the counting sink equals the written length record by record
//   check <in>               mm355_bam_check on every set: one "rc <code>" line each
//   wrap <in> <out>          the file's bytes through mm355_bgzf_wrap_host
//   crc <in>                 the CRC-32 the framing kernel computes, its lanes, combine levels and tail run serially (bgzf_lane_crc,
//                            bgzf_crc_level, bgzf_tail_crc), against zlib on every BGZF_PAYLOAD piece of the file: "crc <pieces>"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../mappy-rs_amd/csrc/mm355_bam.h"

static int run_codes()
{
	for (int rev = 0; rev < 2; ++rev) { for (int c = 0; c < 256; ++c) printf("%02x", bam_code_on((unsigned char)c, rev != 0)); printf("\n"); }
	return 0;
}

static bool rd(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
static std::vector<char> slurp(const char *path, bool *ok)
{
	std::vector<char> v; FILE *f = fopen(path, "rb");
	*ok = f != 0;
	if (!f) return v;
	char buf[1 << 16]; size_t k;
	while ((k = fread(buf, 1, sizeof(buf), f)) > 0) v.insert(v.end(), buf, buf + k);
	fclose(f);
	return v;
}

// the stream layout of sam_host.cpp's sets
static int run_sets(const char *in, const char *outp, bool check_only)
{
	FILE *f = fopen(in, "rb"), *o = outp? fopen(outp, "wb") : 0;
	if (!f || (outp && !o)) return 2;
	long n_sets = 0;
	for (;;) {
		int64_t hd[11];
		if (fread(hd, 8, 11, f) != 11) break;
		const int64_t nr = hd[0], nh = hd[1], nc = hd[2], ns = hd[3];
		const bool has_cigar = hd[4] != 0;
		const int sam_flags = (int)hd[10];
		std::vector<int64_t> hit_off((size_t)nr + 1); std::vector<int32_t> status((size_t)nr), qlens((size_t)nr), rep((size_t)nr);
		std::vector<uint8_t> has_name((size_t)nr), has_qual((size_t)nr), has_seq((size_t)nr);
		// exact-size heap blocks: a read past the end of an arena is an AddressSanitizer report
		std::vector<mm355_hit_t> hits((size_t)nh); std::vector<mm355_tags_t> tags((size_t)nh); std::vector<uint32_t> cig((size_t)nc); std::vector<char> str((size_t)ns);
		std::vector<char> cb((size_t)hd[6]), qb((size_t)hd[7]), sq((size_t)hd[8]), ql((size_t)hd[9]);
		if (!rd(f, hit_off.data(), hit_off.size() * 8) || !rd(f, status.data(), (size_t)nr * 4) || !rd(f, qlens.data(), (size_t)nr * 4) || !rd(f, rep.data(), (size_t)nr * 4) ||
		    !rd(f, has_name.data(), (size_t)nr) || !rd(f, has_qual.data(), (size_t)nr) || !rd(f, has_seq.data(), (size_t)nr) ||
		    !rd(f, hits.data(), (size_t)nh * sizeof(mm355_hit_t)) || !rd(f, tags.data(), (size_t)nh * sizeof(mm355_tags_t)) || !rd(f, cig.data(), (size_t)nc * 4) ||
		    !rd(f, str.data(), (size_t)ns) || !rd(f, cb.data(), cb.size()) || !rd(f, qb.data(), qb.size()) || !rd(f, sq.data(), sq.size()) || !rd(f, ql.data(), ql.size())) return 3;
		std::vector<std::string> contigs;
		for (size_t a = 0; a < cb.size(); a += strlen(&cb[a]) + 1) contigs.emplace_back(&cb[a]);
		if ((int64_t)contigs.size() != hd[5]) return 4;
		std::vector<const char*> qn((size_t)nr, (const char*)0), sp((size_t)nr, (const char*)0), qp((size_t)nr, (const char*)0);
		std::vector<std::vector<char>> own;      // every read and quality string in a heap block of its own size
		size_t a = 0, sa = 0, qa = 0;
		for (int64_t i = 0; i < nr; ++i) {
			if (has_name[i]) { qn[i] = &qb[a]; a += strlen(&qb[a]) + 1; }
			size_t l = qlens[i] > 0? (size_t)qlens[i] : 0;
			if (check_only && l > sq.size() - sa) l = sq.size() - sa;   // (a set for the check may claim a longer read than it brings: the check reads lengths, never bases)
			own.emplace_back(sq.begin() + (long)sa, sq.begin() + (long)(sa + l)); sa += l;
			if (has_seq[i]) sp[i] = own.back().empty()? "" : own.back().data();
			if (has_qual[i]) { const size_t m = l < ql.size() - qa? l : ql.size() - qa; own.emplace_back(ql.begin() + (long)qa, ql.begin() + (long)(qa + m)); qa += m; qp[i] = own.back().empty()? "" : own.back().data(); }
		}
		mm355_hits_t H; memset(&H, 0, sizeof(H));
		H.n_reads = nr; H.hit_off = hit_off.data(); H.status = status.data(); H.hits = hits.data(); H.cigar = cig.data(); H.str = str.data();
		H.n_hits = nh; H.n_cigar = nc; H.n_str = ns; H.tags = tags.data();
		static mm355_tags_t no_tags;
		if (nh == 0) H.tags = &no_tags;   // (an empty vector has no address, and a result without the tags array is refused)
		const PafNames nm = { contigs.data(), (uint32_t)contigs.size() };
		int rc = mm355_bam_check(&H, nm.n_seq, has_cigar, qn.data(), sp.data(), qlens.data(), rep.data(), sam_flags);
		if (check_only) { printf("rc %d\n", rc); ++n_sets; continue; }
		if (rc) { printf("set %ld: check %d\n", n_sets, rc); return 5; }
		mm355_text_t *T = 0;
		rc = mm355_bam_format_host(&H, qn.data(), sp.data(), qlens.data(), qp.data(), rep.data(), nm, sam_flags, &T);
		if (rc) { printf("set %ld: format %d\n", n_sets, rc); return 6; }
		// the counting sink against line_off, read by read; the totals
		const SamNames snm(nm);
		int64_t at = 0, n_rec = 0;
		for (int64_t i = 0; i < nr; ++i) {
			if (T->line_off[i] != at) { printf("set %ld: line_off[%lld]\n", n_sets, (long long)i); return 7; }
			const int64_t nl = mm355_sam_n_lines(&H, qlens.data(), sam_flags, i);
			if (nl == 0) continue;
			const SamRead R = mm355_sam_read_of(&H, i, qn.data(), sp.data(), qlens.data(), qp.data(), rep.data(), snm, sam_flags);
			for (int64_t j = 0; j < nl; ++j, ++n_rec) {
				BamCountSink c;
				bam_emit_record(c, SamLine{ &R, R.n_rows? (int32_t)j : -1 }, R.n_rows? mm355_bam_reflen(&H, R.rows[j]) : 0, 0);
				at += c.n;
			}
		}
		if (T->line_off[nr] != at || bgzf_size(at) != T->n_text || T->n_lines != n_rec || T->n_reads != nr) { printf("set %ld: totals\n", n_sets); return 9; }
		fwrite(&T->n_text, 8, 1, o); fwrite(&T->n_lines, 8, 1, o); fwrite(T->line_off, 8, (size_t)nr + 1, o); fwrite(T->text, 1, (size_t)T->n_text, o);
		mm355_free_text_host(T);
		++n_sets;
	}
	fclose(f); if (o) fclose(o);
	printf("sets %ld\n", n_sets);
	return 0;
}

static int run_wrap(const char *in, const char *outp)
{
	bool ok;
	const std::vector<char> v = slurp(in, &ok);
	FILE *o = fopen(outp, "wb");
	if (!ok || !o) return 2;
	mm355_text_t *T = 0;
	const std::vector<char> exact(v);                     // (a heap block of the input's size)
	if (mm355_bgzf_wrap_host(exact.empty()? 0 : exact.data(), (int64_t)exact.size(), &T)) return 3;
	if (T->n_text != bgzf_size((int64_t)v.size()) || T->n_lines != bgzf_blocks((int64_t)v.size())) return 4;
	fwrite(T->text, 1, (size_t)T->n_text, o);
	fclose(o);
	printf("wrap %lld\n", (long long)T->n_text);
	mm355_free_text_host(T);
	return 0;
}

static int run_crc(const char *in)
{
	bool ok;
	const std::vector<char> v = slurp(in, &ok);
	if (!ok) return 2;
	uint32_t tab[256], x_pow[8];
	for (uint32_t i = 0; i < 256; ++i) tab[i] = crc32_tab_entry(i);
	for (int l = 0; l < 8; ++l) x_pow[l] = crc32_x2n(11 + l);
	long n = 0;
	for (size_t at = 0; at < v.size(); at += BGZF_PAYLOAD, ++n) {
		const uint32_t len = (uint32_t)(v.size() - at < BGZF_PAYLOAD? v.size() - at : BGZF_PAYLOAD);
		const std::vector<unsigned char> piece(v.begin() + (long)at, v.begin() + (long)(at + len));
		uint32_t reg[BGZF_LANES];
		for (int lane = 0; lane < BGZF_LANES; ++lane) reg[lane] = bgzf_lane_crc(piece.data(), len, lane, tab);
		for (int l = 0; l < 8; ++l)
			for (int lane = 0; lane < BGZF_LANES; lane += 2 << l) reg[lane] = bgzf_crc_level(reg, lane, l, x_pow[l]);
		const uint32_t want = (uint32_t)crc32(crc32(0L, Z_NULL, 0), piece.data(), len);
		const uint32_t got = ~bgzf_tail_crc(piece.data(), len, reg[0], tab);
		if (got != want) { printf("piece %ld: %08x, zlib %08x\n", n, got, want); return 1; }
	}
	printf("crc %ld\n", n);
	return 0;
}

int main(int argc, char **argv)
{
	if (argc == 2 && !strcmp(argv[1], "codes")) return run_codes();
	if (argc == 4 && !strcmp(argv[1], "sets")) return run_sets(argv[2], argv[3], false);
	if (argc == 3 && !strcmp(argv[1], "check")) return run_sets(argv[2], 0, true);
	if (argc == 4 && !strcmp(argv[1], "wrap")) return run_wrap(argv[2], argv[3]);
	if (argc == 3 && !strcmp(argv[1], "crc")) return run_crc(argv[2]);
	fprintf(stderr, "usage: bam_host codes | sets <in> <out> | check <in> | wrap <in> <out> | crc <in>\n");
	return 64;
}
