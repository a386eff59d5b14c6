// mm355_bgzfdev.h -- what the kernels that write and read BGZF blocks share (mm355_bam.hip: k_bgzf_frame, k_bgzf_deflate, k_bgzf_compact;
// mm355_inflate.hip: k_bgzf_inflate): a span copied by a workgroup in aligned 16-byte stores, and a payload's CRC-32 by its lanes
#pragma once
#include "mm355_recdev.h"
#include "mm355_bam.h"
#include "mm355_bgzfwalk.h"

// mm355_inflate.hip: k_bgzf_inflate on a caller's stream (the merge step of mm355_bam.hip launches it between its own kernels)
int bgzf_inflate_launch(int dev, hipStream_t st, const unsigned char *d_in, const BgzfMember *d_mem, int64_t n_mem, char *d_out, int32_t *d_status);

// len bytes from src to dst by the block's threads: a thread owns an aligned 16-byte piece of the destination, the ragged ends are byte
// stores; src is readable for 8 bytes more (whole dwords are read around a span)
__device__ __forceinline__ void bgzf_copy(const char *src, char *dst, uint32_t len, int tid)
{
	const uintptr_t d0 = (uintptr_t)dst, d1 = d0 + len;
	for (uintptr_t c = (d0 & ~(uintptr_t)15) + 16 * (uintptr_t)tid; c < d1; c += 16 * BGZF_LANES) {
		if (c >= d0 && c + 16 <= d1) {
			uint32_t v[4];
			sam_load16(src, (int64_t)(c - d0), v);
			*(uint4*)c = make_uint4(v[0], v[1], v[2], v[3]);
		} else {
			const uintptr_t e = c + 16 < d1? c + 16 : d1;
			for (uintptr_t a = c > d0? c : d0; a < e; ++a) *(char*)a = src[a - d0];
		}
	}
}
// the CRC-32 of a payload by the block's lanes; thread 0 has it.  tab and x_pow are filled and a barrier has passed since
__device__ __forceinline__ uint32_t bgzf_block_crc(const char *src, uint32_t len, const uint32_t *tab, uint32_t *reg, const uint32_t *x_pow, int tid)
{
	reg[tid] = bgzf_lane_crc((const unsigned char*)src, len, tid, tab);
	__syncthreads();
	for (int level = 0; level < 8; ++level) {
		uint32_t x = 0;
		const bool mine = (tid & ((2 << level) - 1)) == 0;
		if (mine) x = bgzf_crc_level(reg, tid, level, x_pow[level]);
		__syncthreads();
		if (mine) reg[tid] = x;
		__syncthreads();
	}
	return tid == 0? ~bgzf_tail_crc((const unsigned char*)src, len, reg[0], tab) : 0u;
}
