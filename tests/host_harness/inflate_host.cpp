// inflate_host.cpp -- the host side of the BGZF inflate stage as a stand-alone program (g++ alone, AddressSanitizer + UBSan;
// tests/test_inflate_host.py):
//   cases <in> <out>     <in>: cases of (uint32 n_in, uint32 isize, uint32 crc, n_in bytes of cdata); each through inf_member_host of
//                        mm355_inflate.h with cdata and the output in heap blocks of exactly their sizes (an access past either span is a
//                        report); prints one status per line and writes the payloads of the accepted cases to <out>, back to back
//   unwrap <in> <out>    a file of BGZF members: bgzf_walk of mm355_bgzfwalk.h, then every member; prints "members <n> bytes <m>", or "rc <code>"
//   walk <in> <first> <eof> [max_out]   bgzf_walk alone: "rc <code> used <bytes> out <bytes>", then per member "<c_off> <c_len> <isize> <crc> <o_off>"
//   bam <in> <chunk>     <in>: the INFLATED bytes of a BAM file, handed to the record loop of mm355_bamread.h <chunk> bytes at a time; per read
//                        "<name> <bases> <quality or *>", then "rc <0 or code>"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../mappy-rs_amd/csrc/mm355_inflate.h"
#include "../../mappy-rs_amd/csrc/mm355_bgzfwalk.h"
#include "../../mappy-rs_amd/csrc/mm355_bamread.h"

static bool slurp(const char *path, std::vector<unsigned char> &v)
{
	FILE *f = fopen(path, "rb");
	if (!f) return false;
	unsigned char buf[1 << 16]; size_t k;
	while ((k = fread(buf, 1, sizeof(buf), f)) > 0) v.insert(v.end(), buf, buf + k);
	fclose(f);
	return true;
}
static uint32_t le32(const unsigned char *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

static int run_cases(const char *in, const char *outp)
{
	std::vector<unsigned char> v;
	if (!slurp(in, v)) return 2;
	FILE *o = fopen(outp, "wb");
	if (!o) return 2;
	std::vector<InfHost> S(1);
	for (size_t at = 0; at + 12 <= v.size(); ) {
		const uint32_t n_in = le32(&v[at]), isize = le32(&v[at + 4]), crc = le32(&v[at + 8]);
		if (at + 12 + n_in > v.size()) return 3;
		const std::vector<unsigned char> cdata(v.begin() + (long)at + 12, v.begin() + (long)(at + 12 + n_in));   // (exactly n_in bytes)
		std::vector<unsigned char> out(isize <= INF_MAX_ISIZE? isize : 0);
		const uint32_t st = inf_member_host(cdata.data(), n_in, isize, crc, out.data(), S[0]);
		printf("%u\n", st);
		if (st == 0 && isize) fwrite(out.data(), 1, isize, o);
		at += 12 + n_in;
	}
	fclose(o);
	return 0;
}

static int run_unwrap(const char *in, const char *outp)
{
	std::vector<unsigned char> v;
	if (!slurp(in, v)) return 2;
	const std::vector<unsigned char> exact(v);
	std::vector<BgzfMember> mem;
	int64_t used = 0, n_out = 0;
	const int rc = bgzf_walk(exact.data(), (int64_t)exact.size(), true, true, mem, &used, &n_out);
	if (rc) { printf("rc %d\n", rc); return 0; }
	std::vector<unsigned char> out((size_t)n_out);
	std::vector<InfHost> S(1);
	for (const BgzfMember &m : mem) {
		const std::vector<unsigned char> cdata(exact.begin() + m.c_off, exact.begin() + m.c_off + m.c_len);
		std::vector<unsigned char> pay(m.isize);
		if (inf_member_host(cdata.data(), m.c_len, m.isize, m.crc, pay.data(), S[0])) { printf("rc %d\n", MM355_EIO); return 0; }
		if (m.isize) memcpy(&out[(size_t)m.o_off], pay.data(), m.isize);
	}
	FILE *o = fopen(outp, "wb");
	if (!o) return 2;
	if (n_out) fwrite(out.data(), 1, (size_t)n_out, o);
	fclose(o);
	printf("members %zu bytes %lld\n", mem.size(), (long long)n_out);
	return 0;
}

static int run_walk(const char *in, int first, int eof, long long max_out)
{
	std::vector<unsigned char> v;
	if (!slurp(in, v)) return 2;
	const std::vector<unsigned char> exact(v);
	std::vector<BgzfMember> mem;
	int64_t used = 0, n_out = 0;
	const int rc = bgzf_walk(exact.data(), (int64_t)exact.size(), first != 0, eof != 0, mem, &used, &n_out, max_out);
	printf("rc %d used %lld out %lld\n", rc, (long long)used, (long long)n_out);
	for (const BgzfMember &m : mem) printf("%lld %u %u %u %lld\n", (long long)m.c_off, m.c_len, m.isize, m.crc, (long long)m.o_off);
	return 0;
}

// the stream from memory, at most `chunk` bytes per step, every step through a heap block of its own size
struct MemTake {
	const std::vector<unsigned char> &v; size_t pos, chunk;
	int64_t take(void *dst, size_t n)
	{
		size_t got = 0;
		while (got < n && pos < v.size()) {
			size_t k = n - got < chunk? n - got : chunk;
			if (k > v.size() - pos) k = v.size() - pos;
			const std::vector<unsigned char> piece(v.begin() + (long)pos, v.begin() + (long)(pos + k));
			if (dst) memcpy((char*)dst + got, piece.data(), k);
			pos += k; got += k;
		}
		return (int64_t)got;
	}
	int err() const { return 0; }
};

static int run_bam(const char *in, size_t chunk)
{
	std::vector<unsigned char> v;
	if (!slurp(in, v) || chunk < 1) return 2;
	MemTake t = { v, 0, chunk };
	int rc = bam_read_header(t);
	std::string name, seq, qual; bool has_qual = false;
	while (rc == 0) {
		seq.assign("xx");                                  // (the bases are appended behind what is there)
		const int r = bam_read_record(t, name, seq, qual, &has_qual);
		if (r != 1) { rc = r; break; }
		printf("%s %s %s\n", name.c_str(), seq.c_str() + 2, has_qual? qual.c_str() : "*");
	}
	printf("rc %d\n", rc);
	return 0;
}

int main(int argc, char **argv)
{
	if (argc == 4 && !strcmp(argv[1], "cases")) return run_cases(argv[2], argv[3]);
	if (argc == 4 && !strcmp(argv[1], "unwrap")) return run_unwrap(argv[2], argv[3]);
	if ((argc == 5 || argc == 6) && !strcmp(argv[1], "walk")) return run_walk(argv[2], atoi(argv[3]), atoi(argv[4]), argc == 6? atoll(argv[5]) : 0);
	if (argc == 4 && !strcmp(argv[1], "bam")) return run_bam(argv[2], (size_t)atoll(argv[3]));
	fprintf(stderr, "usage: inflate_host cases <in> <out> | unwrap <in> <out> | walk <in> <first> <eof> [max_out] | bam <in> <chunk>\n");
	return 64;
}
