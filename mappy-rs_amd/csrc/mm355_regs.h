// mm355_regs.h -- minimap2's region logic, stated once: U:hit.c::mm_gen_regs, mm_reg_set_coor, mm_set_parent, mm_sync_regs / mm_set_sam_pri,
// mm_select_sub, mm_filter_strand_retained, mm_set_mapq, U:esterr.c::mm_est_err and the two hashes, as templates over the region type R:
//   Mm355Reg (below)        the chain-only tail of a read (mapping without MM_F_CIGAR): k_regs of mm355_regs.hip runs mm355_regs_read on the
//                           device, a lane per read; tests/host_harness/regs_host.cpp compiles the same instantiation with g++
//   Reg (mm355_glue.h)      the host tail: mm355_glue.cpp calls the steps before and after extension, and for the chain-only reads the device
//                           leaves to the host; tests/host_harness/regs_finish_host.cpp holds this instantiation against the oracle
// What extension adds to a region is reached through three overloads found by the region type: mm355r_extra(r) (the record with dp_max /
// dp_max2, or null), mm355r_inv(r) and mm355r_drop(r) (release a region select_sub leaves out).  For Mm355Reg they are the constants below.
// A fourth, mm355r_sort_for, picks the caller's sort.
//
// One read, sequential, on caller-provided scratch (Mm355RegsScratch).
//
// Two library calls do not agree between the device and glibc bit for bit.  The host's are the truth (Mm355Libm: logf and pow are called and
// nothing is deferred); the device never decides with its own (Mm355LogTab):
//   logf  (mm_set_mapq): the arguments are integers (chain score, n_sub + 1); the values come from a table filled with the host's logf.
//         An argument beyond the table sends the read to the host.
//   pow   (mm_est_err): the result only reaches the records through filter_strand_retained's comparisons.  A region whose float divergence
//         could change under a few ulp of error in pow is marked; a read whose comparisons read a marked divergence goes to the host.
//         With tags rows requested (MM355_OUT_TAGS) the divergence itself is reported: then a read goes to the host as soon as any region
//         that survives to a hit row is marked.
#pragma once
#include "../../include/mm355.h"
#include "mm355_core.h"
#include <math.h>

#define MM355_PARENT_UNSET   (-1)
#define MM355_PARENT_TMP_PRI (-2)

struct Mm355Reg {           // the fields of U:minimap.h::mm_reg1_t the chain-only tail reads or writes
	int32_t id, parent, cnt, rid, score, score0;
	int32_t qs, qe, rs, re, as, mlen, blen, subsc, n_sub;
	uint32_t hash, rev, strand_retained;
	uint16_t div_unsure, sam_pri;
	float div;
};

struct Mm355RegsOpt {       // from mm355_mapopt_t + the index
	int64_t flag;
	float mask_level, pri_ratio;
	int32_t mask_len, best_n, min_diff, min_strand_sc, min_chain_score, seed;
};

inline Mm355RegsOpt mm355_regs_opt(const mm355_mapopt_t *mo, int k)
{
	Mm355RegsOpt o;
	memset(&o, 0, sizeof(o));
	o.flag = mo->flag; o.mask_level = mo->mask_level; o.pri_ratio = mo->pri_ratio; o.mask_len = mo->mask_len; o.best_n = mo->best_n;
	o.min_diff = k * 2; o.min_strand_sc = (int)(mo->max_gap * 0.8); o.min_chain_score = mo->min_chain_score; o.seed = mo->seed;
	return o;
}

struct Mm355RegsScratch {   // n_u entries each (r: the device's regions; the host keeps its own in ReadState)
	Mm355Reg *r;
	mm128 *z;
	uint64_t *cov;
	int32_t *w, *tmp;
};

// a chain-only region has no extension record, is no inversion and owns nothing
struct Mm355NoExtra { int32_t dp_max, dp_max2; };
MM_HD Mm355NoExtra *mm355r_extra(const Mm355Reg*) { return nullptr; }
MM_HD uint32_t mm355r_inv(const Mm355Reg*) { return 0; }
MM_HD void mm355r_drop(Mm355Reg*) {}

// what a read hands back when the device may not decide it
#define MM355_REGS_DEFER_LOG  1
#define MM355_REGS_DEFER_POW  2

// the numerics of a caller: logf of a positive integer (false: the read is deferred), and whether its pow decides
struct Mm355Libm {};
struct Mm355LogTab { const float *t; int32_t n; };   // t[x] = the host's logf(x) for 1 <= x < n
MM_HD bool mm355r_logf(Mm355Libm, int64_t x, float *out) { *out = logf((float)x); return true; }
MM_HD bool mm355r_logf(const Mm355LogTab &m, int64_t x, float *out)
{
	if (x < 1 || x >= m.n) return false;
	*out = m.t[x];
	return true;
}
MM_HD bool mm355r_pow_decides(Mm355Libm) { return true; }
MM_HD bool mm355r_pow_decides(const Mm355LogTab&) { return false; }

MM_HD uint32_t mm355r_wang32(uint32_t key)
{
	key += ~(key << 15); key ^= (key >> 10); key += (key << 3); key ^= (key >> 6); key += ~(key << 11); key ^= (key >> 16);
	return key;
}
MM_HD uint64_t mm355r_hash64(uint64_t key)
{
	key = (~key + (key << 21)); key = key ^ key >> 24; key = ((key + (key << 3)) + (key << 8)); key = key ^ key >> 14;
	key = ((key + (key << 2)) + (key << 4)); key = key ^ key >> 28; key = (key + (key << 31));
	return key;
}
// U:map.c::mm_map_frag: the read hash; name_hash = X31(qname), 0 for a read without a name or under MM_F_NO_HASH_NAME
MM_HD uint32_t mm355r_read_hash(int32_t qlen, int32_t seed, uint32_t name_hash = 0)
{
	uint32_t h = name_hash;
	h ^= mm355r_wang32((uint32_t)qlen) + mm355r_wang32((uint32_t)seed);
	return mm355r_wang32(h);
}

// in-place heap sort (the keys sorted here are unique as a whole, so any sort gives the radix sorts' order)
MM_HD bool mm355r_lt(const mm128 &a, const mm128 &b) { return a.x < b.x || (a.x == b.x && a.y < b.y); }
MM_HD bool mm355r_lt(uint64_t a, uint64_t b) { return a < b; }
template <typename T>
MM_HD void mm355r_sift(T *v, int i, int n)
{
	for (;;) {
		int c = 2 * i + 1;
		if (c >= n) return;
		if (c + 1 < n && mm355r_lt(v[c], v[c + 1])) ++c;
		if (!mm355r_lt(v[i], v[c])) return;
		T t = v[i]; v[i] = v[c]; v[c] = t;
		i = c;
	}
}
template <typename T>
MM_HD void mm355r_sort(T *v, int n)
{
	for (int i = n / 2 - 1; i >= 0; --i) mm355r_sift(v, i, n);
	for (int e = n - 1; e > 0; --e) { T t = v[0]; v[0] = v[e]; v[e] = t; mm355r_sift(v, 0, e); }
}

// which sort a caller runs, by its region type: the device's needs no bucket arrays; the host keeps mm_radix_sort (mm355_glue.h), U:ksort.h's
// own procedure, because the heap sort showed in its CPU time per read.  The two can differ only in the order of equal gen_regs keys (chains
// with one score, count and first anchor) among more than 64 regions, where the radix sort is not stable.
template <typename T>
MM_HD void mm355r_sort_for(const Mm355Reg*, T *v, int n) { mm355r_sort(v, n); }

template <typename R>
MM_HD void mm355r_set_coor(R *r, int32_t qlen, const mm128 *a)
{   // U:hit.c::mm_reg_set_coor + reg_fuzzy_len
	int32_t k = r->as, q_span = (int32_t)(a[k].y >> 32 & 0xff);
	r->rev = (uint32_t)(a[k].x >> 63);
	r->rid = (int32_t)(a[k].x << 1 >> 33);
	r->rs = (int32_t)a[k].x + 1 > q_span? (int32_t)a[k].x + 1 - q_span : 0;
	r->re = (int32_t)a[k + r->cnt - 1].x + 1;
	if (!r->rev) {
		r->qs = (int32_t)a[k].y + 1 - q_span;
		r->qe = (int32_t)a[k + r->cnt - 1].y + 1;
	} else {
		r->qs = qlen - ((int32_t)a[k + r->cnt - 1].y + 1);
		r->qe = qlen - ((int32_t)a[k].y + 1 - q_span);
	}
	r->mlen = r->blen = 0;
	if (r->cnt <= 0) return;
	r->mlen = r->blen = (int32_t)(a[r->as].y >> 32 & 0xff);
	for (int i = r->as + 1; i < r->as + r->cnt; ++i) {
		int span = (int)(a[i].y >> 32 & 0xff);
		int tl = (int32_t)a[i].x - (int32_t)a[i-1].x;
		int ql = (int32_t)a[i].y - (int32_t)a[i-1].y;
		r->blen += tl > ql? tl : ql;
		r->mlen += tl > span && ql > span? span : tl < ql? tl : ql;
	}
}

// U:hit.c::mm_gen_regs: radix_sort_128x on x (stable) then a reversal = x descending, equal x in descending index order.  z.y's high word
// (the first anchor) grows with the index, so an ascending (x, y) sort followed by the same reversal gives that order.
template <typename R>
MM_HD int mm355r_gen_regs(uint32_t hash, int32_t qlen, int n_u, const uint64_t *u, const mm128 *a, mm128 *z, R *r)
{
	int k = 0;
	for (int i = 0; i < n_u; ++i) {
		uint32_t h = (uint32_t)mm355r_hash64((mm355r_hash64(a[k].x) + mm355r_hash64(a[k].y)) ^ hash);
		z[i].x = u[i] ^ h;
		z[i].y = (uint64_t)k << 32 | (uint32_t)(int32_t)u[i];
		k += (int32_t)u[i];
	}
	mm355r_sort_for(r, z, n_u);
	for (int i = 0; i < n_u; ++i) {
		const mm128 zi = z[n_u - 1 - i];
		R *ri = &r[i];
		*ri = R();
		ri->id = i;
		ri->parent = MM355_PARENT_UNSET;
		ri->score = ri->score0 = (int32_t)(zi.x >> 32);
		ri->hash = (uint32_t)zi.x;
		ri->cnt = (int32_t)zi.y;
		ri->as = (int32_t)(zi.y >> 32);
		ri->div = -1.0f;
		mm355r_set_coor(ri, qlen, a);
	}
	return n_u;
}

// U:hit.c::mm_set_parent; sub_diff is read only where both regions have an extension record, so the calls before extension leave it out
template <typename R>
MM_HD void mm355r_set_parent(float mask_level, int mask_len, int n, R *r, int hard_mask_level, uint64_t *cov, int32_t *w, int sub_diff = 0)
{
	if (n <= 0) return;
	for (int i = 0; i < n; ++i) r[i].id = i;
	int k = 1, j;
	w[0] = 0, r[0].parent = 0;
	for (int i = 1; i < n; ++i) {
		R *ri = &r[i];
		int si = ri->qs, ei = ri->qe, n_cov = 0, uncov_len = 0;
		if (!hard_mask_level) {
			for (j = 0; j < k; ++j) {
				const R *rp = &r[w[j]];
				int sj = rp->qs, ej = rp->qe;
				if (ej <= si || sj >= ei) continue;
				if (sj < si) sj = si;
				if (ej > ei) ej = ei;
				cov[n_cov++] = (uint64_t)sj << 32 | (uint32_t)ej;
			}
			if (n_cov == 0) {
				w[k++] = i, ri->parent = i, ri->n_sub = 0;
				continue;
			}
			int x = si;
			mm355r_sort_for(r, cov, n_cov);
			for (int jj = 0; jj < n_cov; ++jj) {
				if ((int)(cov[jj] >> 32) > x) uncov_len += (int)(cov[jj] >> 32) - x;
				x = (int32_t)cov[jj] > x? (int32_t)cov[jj] : x;
			}
			if (ei > x) uncov_len += ei - x;
		}
		for (j = 0; j < k; ++j) {
			R *rp = &r[w[j]];
			int sj = rp->qs, ej = rp->qe, min, max, ol;
			if (ej <= si || sj >= ei) continue;
			min = ej - sj < ei - si? ej - sj : ei - si;
			max = ej - sj > ei - si? ej - sj : ei - si;
			ol = si < sj? (ei < sj? 0 : ei < ej? ei - sj : ej - sj) : (ej < si? 0 : ej < ei? ej - si : ei - si);
			if ((float)ol / min - (float)uncov_len / max > mask_level && uncov_len <= mask_len) {
				const int sci = ri->score;
				int cnt_sub = ri->cnt >= rp->cnt;
				ri->parent = rp->parent;
				rp->subsc = rp->subsc > sci? rp->subsc : sci;
				const auto pp = mm355r_extra(rp), pi = mm355r_extra(ri);
				if (pp && pi && (rp->rid != ri->rid || rp->rs != ri->rs || rp->re != ri->re || ol != min)) {   // (ol != min: not the same hit after DP)
					pp->dp_max2 = pp->dp_max2 > pi->dp_max? pp->dp_max2 : pi->dp_max;
					if (pp->dp_max - pi->dp_max <= sub_diff) cnt_sub = 1;
				}
				if (cnt_sub) ++rp->n_sub;
				break;
			}
		}
		if (j == k) w[k++] = i, ri->parent = i, ri->n_sub = 0;
	}
}

// U:hit.c::mm_set_sam_pri: the first primary gets sam_pri (one region's step, so that sync_regs can take it in its own pass)
template <typename R>
MM_HD void mm355r_sam_pri_step(R *ri, int *n_pri) { ri->sam_pri = ri->id == ri->parent && ++*n_pri == 1; }
template <typename R>
MM_HD void mm355r_set_sam_pri(int n, R *r)
{
	int n_pri = 0;
	for (int i = 0; i < n; ++i) mm355r_sam_pri_step(&r[i], &n_pri);
}

// U:hit.c::mm_sync_regs with its closing mm_set_sam_pri.  tmp has n_tmp entries, one per id that can occur: select_sub is the only caller and
// runs on what set_parent numbered 0 .. n_tmp - 1.  Chain-only mapping has no other call of mm_set_sam_pri, so a read whose select_sub drops
// nothing keeps sam_pri = 0 everywhere.
template <typename R>
MM_HD void mm355r_sync_regs(int n, R *r, int32_t *tmp, int n_tmp)
{
	if (n <= 0) return;
	for (int i = 0; i < n_tmp; ++i) tmp[i] = -1;
	for (int i = 0; i < n; ++i) if (r[i].id >= 0 && r[i].id < n_tmp) tmp[r[i].id] = i;
	int n_pri = 0;
	for (int i = 0; i < n; ++i) {
		R *ri = &r[i];
		ri->id = i;
		if (ri->parent == MM355_PARENT_TMP_PRI) ri->parent = i;
		else if (ri->parent >= 0 && ri->parent < n_tmp && tmp[ri->parent] >= 0) ri->parent = tmp[ri->parent];
		else ri->parent = MM355_PARENT_UNSET;
		mm355r_sam_pri_step(ri, &n_pri);
	}
}

// U:hit.c::mm_select_sub (check_strand: 1 before extension, 0 after); tmp: n entries
template <typename R>
MM_HD int mm355r_select_sub(float pri_ratio, int min_diff, int best_n, int min_strand_sc, int n, R *r, int32_t *tmp, int check_strand = 1)
{
	if (!(pri_ratio > 0.0f && n > 0)) return n;
	int k = 0, n_2nd = 0;
	for (int i = 0; i < n; ++i) {
		const int p = r[i].parent;
		if (p == i || mm355r_inv(&r[i])) {
			r[k++] = r[i];
		} else if ((r[i].score >= r[p].score * pri_ratio || r[i].score + min_diff >= r[p].score) && n_2nd < best_n) {
			if (!(r[i].qs == r[p].qs && r[i].qe == r[p].qe && r[i].rid == r[p].rid && r[i].rs == r[p].rs && r[i].re == r[p].re))
				r[k++] = r[i], ++n_2nd;
			else mm355r_drop(&r[i]);
		} else if (check_strand && n_2nd < best_n && r[i].score > min_strand_sc && r[p].rev != r[i].rev) {
			r[i].strand_retained = 1;
			r[k++] = r[i], ++n_2nd;
		} else mm355r_drop(&r[i]);
	}
	if (k != n) mm355r_sync_regs(k, r, tmp, n);
	return k;
}

MM_HD int32_t mm355r_for_qpos(int32_t qlen, const mm128 *a)
{
	int32_t x = (int32_t)a->y, q_span = (int32_t)(a->y >> 32 & 0xff);
	if (a->x >> 63) x = qlen - 1 - (x + 1 - q_span);
	return x;
}

// U:esterr.c::mm_est_err; div_unsure marks a divergence that a few ulp of error in pow() could move to another float
template <typename R>
MM_HD void mm355r_est_err(const uint32_t *seq_len, int32_t qlen, int n, R *r, const mm128 *a, int32_t n_mini, const uint64_t *mini_pos)
{
	uint64_t sum_k = 0;
	if (n_mini == 0) return;
	for (int i = 0; i < n_mini; ++i) sum_k += mini_pos[i] >> 32 & 0xff;
	const float avg_k = (float)sum_k / n_mini;
	for (int i = 0; i < n; ++i) {
		R *ri = &r[i];
		int32_t st, en, j, k, n_match, n_tot, l_ref;
		ri->div = -1.0f;
		if (ri->cnt == 0) continue;
		{   // get_mini_idx
			int32_t x = mm355r_for_qpos(qlen, ri->rev? &a[ri->as + ri->cnt - 1] : &a[ri->as]), lo = 0, hi = n_mini - 1;
			st = -1;
			while (lo <= hi) {
				int32_t m = (int32_t)(((uint64_t)lo + hi) >> 1), y = (int32_t)mini_pos[m];
				if (y < x) lo = m + 1; else if (y > x) hi = m - 1; else { st = m; break; }
			}
		}
		en = st;
		if (st < 0) continue;
		l_ref = (int32_t)seq_len[ri->rid];
		for (k = 1, j = st + 1, n_match = 1; j < n_mini && k < ri->cnt; ++j) {
			int32_t x = mm355r_for_qpos(qlen, ri->rev? &a[ri->as + ri->cnt - 1 - k] : &a[ri->as + k]);
			if (x == (int32_t)mini_pos[j]) ++k, en = j, ++n_match;
		}
		n_tot = en - st + 1;
		if (ri->qs > avg_k && ri->rs > avg_k) ++n_tot;
		if (qlen - ri->qs > avg_k && l_ref - ri->re > avg_k) ++n_tot;
		if (n_match >= n_tot) { ri->div = 0.0f; continue; }
		const double pw = pow((double)n_match / n_tot, 1.0 / avg_k);
		ri->div = (float)(1.0 - pw);
		// pw lies in (0, 1): 1.0 - pw is exact for pw >= 0.5 and loses at most an ulp below; a relative error of 2^-48 in pw covers any
		// correctly-rounded-within-a-few-ulp pow on either side
		const float lo = (float)(1.0 - pw * (1.0 + 0x1p-48)), hi = (float)(1.0 - pw * (1.0 - 0x1p-48));
		ri->div_unsure = lo != hi;
	}
}

// U:hit.c::mm_filter_strand_retained; returns -1 when a comparison reads an unsure divergence and the caller's pow does not decide
template <typename R>
MM_HD int mm355r_filter_strand_retained(int n, R *r, bool pow_decides)
{
	if (!pow_decides)
		for (int i = 0; i < n; ++i)
			if (r[i].strand_retained && (r[i].div_unsure || r[r[i].parent].div_unsure)) return -1;
	int k = 0;
	for (int i = 0; i < n; ++i) {
		const int p = r[i].parent;
		if (!r[i].strand_retained || r[i].div < r[p].div * 5.0f || r[i].div < 0.01f) {
			if (k < i) r[k++] = r[i]; else ++k;
		}
	}
	return k;
}

// U:hit.c::mm_set_mapq up to its closing mm_set_inv_mapq (the caller's: only extension makes inversions); false: an argument of logf is
// beyond the table.  match_sc is read only where a region has an extension record.
template <typename R, typename M>
MM_HD bool mm355r_set_mapq(int n, const R *r, int min_chain_sc, int match_sc, int rep_len, const M &m, uint32_t *mapq)
{
	const float q_coef = 40.0f;
	int64_t sum_sc = 0;
	if (n == 0) return true;
	for (int i = 0; i < n; ++i) if (r[i].parent == r[i].id) sum_sc += r[i].score;
	const float uniq_ratio = (float)sum_sc / (sum_sc + rep_len);
	for (int i = 0; i < n; ++i) {
		const R *ri = &r[i];
		const auto p = mm355r_extra(ri);
		if (mm355r_inv(ri)) {
			mapq[i] = 0;
		} else if (ri->parent == ri->id) {
			int q, subsc;
			float pen_s1 = (ri->score > 100? 1.0f : 0.01f * ri->score) * uniq_ratio;
			float pen_cm = ri->cnt > 10? 1.0f : 0.1f * ri->cnt;
			pen_cm = pen_s1 < pen_cm? pen_s1 : pen_cm;
			subsc = ri->subsc > min_chain_sc? ri->subsc : min_chain_sc;
			float ls, ln;
			if (!mm355r_logf(m, (int64_t)ri->n_sub + 1, &ln)) return false;
			if (p && p->dp_max2 > 0 && p->dp_max > 0) {
				const float identity = (float)ri->mlen / ri->blen;
				const float x = (float)p->dp_max2 * subsc / p->dp_max / ri->score0;
				q = (int)(identity * pen_cm * q_coef * (1.0f - x * x) * logf((float)p->dp_max / match_sc));
				const int q_alt = (int)(6.02f * identity * identity * (p->dp_max - p->dp_max2) / match_sc + .499f);   // BWA-MEM like
				q = q < q_alt? q : q_alt;
			} else {
				const float x = (float)subsc / ri->score0;
				if (p) {
					const float identity = (float)ri->mlen / ri->blen;
					q = (int)(identity * pen_cm * q_coef * (1.0f - x) * logf((float)p->dp_max / match_sc));
				} else {
					if (!mm355r_logf(m, ri->score, &ls)) return false;
					q = (int)(pen_cm * q_coef * (1.0f - x) * ls);
				}
			}
			q -= (int)(4.343f * ln + .499f);
			q = q > 0? q : 0;
			mapq[i] = q < 60? q : 60;
			if (p && p->dp_max > p->dp_max2 && mapq[i] == 0) mapq[i] = 1;
		} else mapq[i] = 0;
	}
	return true;
}

// The row writers of every path.  The CIGAR path adds its Extra fields and the inv / split bits on top.
template <typename R>
MM_HD void mm355r_hit(const R *r, uint32_t mapq, const uint32_t *seq_len, mm355_hit_t *h)
{
	memset(h, 0, sizeof(*h));
	h->query_start = r->qs; h->query_end = r->qe; h->strand = r->rev? -1 : 1; h->rid = r->rid;
	h->target_len = (int32_t)seq_len[r->rid]; h->target_start = r->rs; h->target_end = r->re;
	h->match_len = r->mlen; h->block_len = r->blen; h->mapq = mapq; h->is_primary = r->parent == r->id;
	h->cs_len = h->md_len = -1;
	h->score0 = r->score0; h->cnt = r->cnt; h->n_sub = r->n_sub; h->subsc = r->subsc;
}

// the tags row of a chain-only hit (MM355_OUT_TAGS): no CIGAR, so no n_ambi / gap counts; no inversion or split regions before extension
template <typename R>
MM_HD void mm355r_tags(const R *r, int32_t rep_len, mm355_tags_t *t)
{
	memset(t, 0, sizeof(*t));
	t->score = r->score; t->div = r->div; t->rep_len = rep_len;
	t->flags = r->sam_pri? MM355_TAG_SAM_PRI : 0u;
}

// the first half of the tail: the chains of a read -> regions, primary / secondary selection, divergence estimate.  No region has an
// extension record yet, so set_parent's sub_diff is not read.
template <typename R>
MM_HD int mm355r_regions(const Mm355RegsOpt &o, const uint32_t *seq_len, int32_t qlen, int n_u, const uint64_t *u, const mm128 *a, int32_t n_mini,
                         const uint64_t *mini_pos, uint32_t name_hash, const Mm355RegsScratch &s, R *r)
{
	int n = mm355r_gen_regs(mm355r_read_hash(qlen, o.seed, name_hash), qlen, n_u, u, a, s.z, r);
	if (!(o.flag & MMF_ALL_CHAINS)) {
		mm355r_set_parent(o.mask_level, o.mask_len, n, r, (int)(o.flag & MMF_HARD_MLEVEL), s.cov, s.w);
		n = mm355r_select_sub(o.pri_ratio, o.min_diff, o.best_n, o.min_strand_sc, n, r, s.tmp, 1);
	}
	mm355r_est_err(seq_len, qlen, n, r, a, n_mini, mini_pos);
	return n;
}

// the second half of the chain-only tail, on the regions est_err left: filter_strand_retained, the pow rules, MAPQ (no extension record: no
// match_sc), the rows (and the tags rows)
template <typename R, typename M>
MM_HD int mm355r_finish(const Mm355RegsOpt &o, const uint32_t *seq_len, int32_t rep_len, int n, R *r, const M &m, uint32_t *mapq, mm355_hit_t *out,
                        mm355_tags_t *tags)
{
	n = mm355r_filter_strand_retained(n, r, mm355r_pow_decides(m));
	if (n < 0) return -MM355_REGS_DEFER_POW;
	if (tags && !mm355r_pow_decides(m)) for (int i = 0; i < n; ++i) if (r[i].div_unsure) return -MM355_REGS_DEFER_POW;   // the divergence itself is reported
	if (!mm355r_set_mapq(n, r, o.min_chain_score, 0, rep_len, m, mapq)) return -MM355_REGS_DEFER_LOG;
	for (int i = 0; i < n; ++i) mm355r_hit(&r[i], mapq[i], seq_len, &out[i]);
	if (tags) for (int i = 0; i < n; ++i) mm355r_tags(&r[i], rep_len, &tags[i]);
	return n;
}

// the device's form of the second half: decided with the host-filled logf table
MM_HD int mm355r_finish(const Mm355RegsOpt &o, const uint32_t *seq_len, int32_t rep_len, int n, Mm355Reg *r, const float *logt, int32_t n_logt,
                        uint32_t *mapq, mm355_hit_t *out, mm355_tags_t *tags)
{
	return mm355r_finish(o, seq_len, rep_len, n, r, Mm355LogTab{logt, n_logt}, mapq, out, tags);
}

// the whole tail of one read, decided with the host's logf table.  Returns the number of hit rows written to `out` (at most n_u), or
// -MM355_REGS_DEFER_* when the read must take the host path.  `mapq` is scratch of n_u words.  tags != 0: one tags row per hit row, and the
// stricter pow rule (a reported divergence must not depend on the device's pow).
MM_HD int mm355_regs_read(const Mm355RegsOpt &o, const uint32_t *seq_len, int32_t qlen, int32_t rep_len, int n_u, const uint64_t *u, const mm128 *a,
                          int32_t n_mini, const uint64_t *mini_pos, const float *logt, int32_t n_logt, const Mm355RegsScratch &s, uint32_t *mapq,
                          mm355_hit_t *out, mm355_tags_t *tags = nullptr, uint32_t name_hash = 0)
{
	if (n_u <= 0 || qlen <= 0) return 0;
	const int n = mm355r_regions(o, seq_len, qlen, n_u, u, a, n_mini, mini_pos, name_hash, s, s.r);
	return mm355r_finish(o, seq_len, rep_len, n, s.r, logt, n_logt, mapq, out, tags);
}
