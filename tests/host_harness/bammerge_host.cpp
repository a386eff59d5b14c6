// bammerge_host.cpp -- one step of the merge of compressed runs on the host as a stand-alone program (g++ alone, AddressSanitizer + UBSan;
// tests/test_bammerge_host.py).  Every input array and the spool are heap blocks of their exact size: a byte read past an end is a report.
//   step <in> <out>   cases written by the test -- int64 base_len, n_slice, n_rec, n_carry, n_carry_bytes, final, level; slice_at, slice_bytes,
//                     slice_raw_at (int64 x n_slice each); rec_slice (int32 x n_rec), rec_at, rec_len (int64 x n_rec each); n_carry_bytes bytes
//                     of carry; base_len bytes of spool (none where base_len < 0) -- through bam_merge_plan and, where it passes,
//                     bam_merge_step_host (mm355_bammerge.h): per case int32 rc, int64 n_text, n_blocks, n_left, the blocks, the leftover.
//                     After a refusal nothing has been returned and the leftover buffer is untouched.
//   pack <in> <out>   the file's bytes as the records of a run through bam_run_pack_host: int64 n_bytes, n_blk, blk_off[n_blk + 1], the members
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <memory>
#include <vector>
#include "../../mappy-rs_amd/csrc/mm355_bammerge.h"

static bool rd(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
template <typename T> static std::unique_ptr<T[]> arr(FILE *f, int64_t n, bool *ok)
{
	std::unique_ptr<T[]> a(new T[(size_t)(n > 0? n : 0)]);
	if (!rd(f, a.get(), (size_t)(n > 0? n : 0) * sizeof(T))) *ok = false;
	return a;
}

static int run_step(FILE *f, FILE *o)
{
	long n_cases = 0;
	for (;; ++n_cases) {
		int64_t hd[7];
		if (fread(hd, 8, 7, f) != 7) break;
		const int64_t base_len = hd[0], n_slice = hd[1], n_rec = hd[2], n_carry = hd[3], n_cb = hd[4];
		bool ok = true;
		auto s_at = arr<int64_t>(f, n_slice, &ok), s_bytes = arr<int64_t>(f, n_slice, &ok), s_raw = arr<int64_t>(f, n_slice, &ok);
		auto r_slice = arr<int32_t>(f, n_rec, &ok);
		auto r_at = arr<int64_t>(f, n_rec, &ok), r_len = arr<int64_t>(f, n_rec, &ok);
		auto carry = arr<char>(f, n_cb, &ok), base = arr<char>(f, base_len, &ok);
		if (!ok) return 3;
		const BamMergeIn a = { base.get(), base_len, s_at.get(), s_bytes.get(), s_raw.get(), n_slice, r_slice.get(), r_at.get(), r_len.get(), n_rec,
		                       carry.get(), n_carry, (int)hd[5], (int)hd[6] };
		std::unique_ptr<char[]> left(new char[BGZF_PAYLOAD]);
		memset(left.get(), 0x5a, BGZF_PAYLOAD);
		int64_t n_left = -1;
		mm355_text_t *T = 0;
		BamMergePlan p;
		int32_t rc = bam_merge_plan(a, p);
		if (rc == 0) rc = bam_merge_step_host(a, p, &T, left.get(), &n_left);
		if (rc) {
			if (T != 0 || n_left != -1) return 4;
			for (int i = 0; i < BGZF_PAYLOAD; ++i) if (left[(size_t)i] != 0x5a) return 4;
			n_left = 0;
		}
		const int64_t n_text = T? T->n_text : 0, n_blocks = T? T->n_lines : 0;
		fwrite(&rc, 4, 1, o); fwrite(&n_text, 8, 1, o); fwrite(&n_blocks, 8, 1, o); fwrite(&n_left, 8, 1, o);
		if (T) fwrite(T->text, 1, (size_t)n_text, o);
		fwrite(left.get(), 1, (size_t)n_left, o);
		mm355_free_text_host(T);
	}
	printf("step %ld\n", n_cases);
	return 0;
}

static int run_pack(FILE *f, FILE *o)
{
	std::vector<char> v; char buf[1 << 16]; size_t k;
	while ((k = fread(buf, 1, sizeof(buf), f)) > 0) v.insert(v.end(), buf, buf + k);
	mm355_run_t *R = mm355_run_alloc(0, (int64_t)v.size());
	if (R == 0) return 3;
	if (!v.empty()) memcpy(R->rec, v.data(), v.size());
	if (bam_run_pack_host(R)) return 4;
	if (R->packed != 1 || R->blk_off[R->n_blk] != R->n_bytes) return 4;
	fwrite(&R->n_bytes, 8, 1, o); fwrite(&R->n_blk, 8, 1, o); fwrite(R->blk_off, 8, (size_t)R->n_blk + 1, o); fwrite(R->rec, 1, (size_t)R->n_bytes, o);
	printf("pack %lld\n", (long long)R->n_blk);
	mm355_free_run_host(R);
	return 0;
}

int main(int argc, char **argv)
{
	if (argc != 4) return 2;
	FILE *f = fopen(argv[2], "rb"), *o = fopen(argv[3], "wb");
	if (!f || !o) return 2;
	int rc = 2;
	if (!strcmp(argv[1], "step")) rc = run_step(f, o);
	else if (!strcmp(argv[1], "pack")) rc = run_pack(f, o);
	fclose(f); fclose(o);
	return rc;
}
