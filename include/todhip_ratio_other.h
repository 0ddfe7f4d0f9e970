/* The ratio test against another object: four calls of libtodhip.so's C ABI, a part of include/todhip.h kept in a file of its own.
 * todhip.h includes this header at its end, and this header includes todhip.h, so either one brings all of the ABI. Plain C99. */
#ifndef TODHIP_RATIO_OTHER_H_
#define TODHIP_RATIO_OTHER_H_
#include "todhip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Lowe's ratio test against ANOTHER OBJECT. todhip_set_ratio_test compares a query's two nearest rows of the whole DB. A TOD model DB
 * holds a surface point once per training view (todhip_model_add_observation[s_device]), so for a correct match both rows are the same
 * point of the same object, d1 / d2 is about 1 and the classic test drops it. Lowe's paper takes the second neighbour from the closest
 * row known to come from a different object; these calls do. For a binary DB (desc_bytes 32 or 64), d = the Hamming distance over the
 * DB's width, NONE = 0xFFFFFFFF.
 * Definition (exact, deterministic):
 *   searched rows   what todhip_match_radius_device searches on the context: the resident shard under the current selection
 *                   (todhip_db_select_objects: "other objects" are the other SELECTED objects).
 *   other(q, o)     = the minimum of d(q, r) over the searched rows r that do not belong to object o; NONE when there is no such row (a
 *                   single-object DB, a selection of one object, a shard that holds only o's rows). With o = NONE, or an o that is no
 *                   object of the DB, no row is excluded.
 *   the predicate   a query with at least one kept match has its nearest match m0 in slot 0 of its row of the fixed-stride output,
 *                   d1 = m0.distance, o1 = m0.imgIdx. It survives iff other == NONE || (float)d1 < ratio * (float)other, other =
 *                   other(q, o1): todhip_set_ratio_test's comparison in binary32, 0 < ratio <= 1.
 *   A query that fails gets counts[q] = 0; its slots are unspecified afterwards, and slots at or behind the old counts[q] are not
 *   written. A query with counts[q] == 0 is left alone. The matches and their xyz are not touched at all.
 *   The radius cut and the classic ratio test have acted before this filter; it is independent of todhip_set_ratio_test, and both may
 *   be on. The LSH mode does not enter: the other-object search is exact over the searched rows. todhip_set_db_bit_order is
 *   honoured: the queries are permuted as every form permutes them, the result does not change.
 * todhip_other_object_min_device, the primitive: d_min[q] = min(other(q, d_excl_obj[q]), d_limit[q], limit_cap) as unsigned integers.
 *   EVERY word of d_min is written. d_limit == NULL: no per-query limit; limit_cap = NONE: no cap (the exact minimum). A shard or
 *   selection without rows gives min(limit, cap). A limit lets the search stop early: a query whose bound has reached its limit is
 *   never looked at again, and one with limit 0 never at all. It runs on any context, also on one shard of several: a sharded caller
 *   runs it on every rank and takes the element-wise minimum over the ranks, which is the primitive's result on the whole DB.
 * todhip_ratio_other_apply_device: the predicate on a fixed-stride output and the d_other_min the caller brings. It reads slot 0 of
 *   each row and nothing of the context but its stream, so any rank's context will do.
 * todhip_ratio_other_device: the whole filter on an unsharded context, in place on what todhip_match_device,
 *   todhip_merge_shards_device[_on], todhip_match_radius_device and todhip_merge_radius_shards_device[_on] leave (stride = k or
 *   max_per_query): per query the limit L = the least integer with (float)d1 < ratio * (float)L -- any other >= L passes, so the
 *   search need not look further; a query with counts[q] == 0 gets limit 0 --, the primitive with d_excl_obj = slot 0's imgIdx and
 *   limit_cap = the limit of the largest possible d1, then the predicate.
 * All three are asynchronous on the context's stream. One DB pass on the matrix cores that keeps distances only -- a threshold and the
 * excluded object's row interval per lane, no lists -- between a per-query setup kernel and the predicate's.
 * TODHIP_EINVAL: a null context or pointer (d_limit may be NULL), nq == 0, ratio outside (0, 1], stride == 0 or > 1024, a float DB;
 * todhip_ratio_other_device on a context whose resident shard is not the whole DB (loaded with shard_count > 1: such a caller uses
 * the two calls above). TODHIP_ENODB without a DB. */
int todhip_other_object_min_device(todhip_ctx*, const void* d_q_desc, uint32_t nq, const void* d_excl_obj /*[nq] u32*/,
                                   const void* d_limit /*[nq] u32, may be NULL*/, uint32_t limit_cap, void* d_min /*[nq] u32 out*/);
int todhip_ratio_other_apply_device(todhip_ctx*, float ratio, uint32_t nq, uint32_t stride, const void* d_other_min /*[nq] u32*/,
                                    void* d_counts /*[nq] u32*/, const void* d_matches /*[nq*stride]*/);
int todhip_ratio_other_device(todhip_ctx*, const void* d_q_desc, uint32_t nq, float ratio, uint32_t stride, void* d_counts /*[nq] u32*/,
                              void* d_matches /*[nq*stride]*/);
/* Switches the filter on for todhip_match and todhip_match_device: while ratio > 0 those two calls run
 * todhip_ratio_other_device(ratio, stride = k) behind their finalize step -- behind the radius cut and todhip_set_ratio_test's test --
 * and in front of the cross-check (todhip_set_cross_check); the host form packs its CSR from the filtered counts. 0 = off, the
 * default: no launch is added and every output is what it was. The sharded, the radius and the float entry points ignore the
 * setting, as they ignore todhip_set_cross_check: a caller filters their device outputs with the calls above.
 * TODHIP_EINVAL, and the setting does not change: a ratio outside [0, 1]; ratio > 0 on a context whose DB is float or is one shard of
 * several. */
int todhip_set_ratio_test_other(todhip_ctx*, float ratio /* 0 = off, the default */);

#ifdef __cplusplus
}
#endif
#endif /* TODHIP_RATIO_OTHER_H_ */
