/*
 * todhip.h -- C ABI of the MI355X-native textured-object-detection hot path.
 *
 * This is the drop-in boundary for wg-perception/tod's detection cells: a thin C++ adapter
 * (adapter/ecto_cells.hpp) keeps the ecto cell, parameter and tendril names of
 * src/detection/DescriptorMatcher.cpp and src/detection/GuessGenerator.cpp and converts the
 * tendril types to the flat buffers below. Citations are file:line in the reference tree.
 *
 * Conventions: every function returns a todhip_status (0 = ok, negative = error); nothing throws,
 * nothing prints; all buffers are caller-owned with explicit sizes; one call in flight per
 * context; a context is bound to one HIP device and one HIP stream. Pointers named d_* are device
 * pointers on the context's device, everything else is host memory.
 */
#ifndef TODHIP_H_
#define TODHIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TODHIP_VERSION 1

typedef enum {
  TODHIP_OK = 0,
  TODHIP_EINVAL = -1,      /* bad argument (null pointer, k == 0, radius == 0, unsupported descriptor size ...) */
  TODHIP_ENODB = -2,       /* no descriptors loaded: DescriptorMatcher.cpp:204-208 logs and returns            */
  TODHIP_EHIP = -3,        /* a HIP runtime call failed; todhip_last_hip_error() has the code                   */
  TODHIP_ECAPACITY = -4,   /* caller-provided output capacity too small                                         */
  TODHIP_ERANGE = -5,      /* keypoint outside the cloud / imgIdx outside the object table                      */
  TODHIP_ENOMEM = -6,
  TODHIP_ESCRATCH = -7,    /* verifier scratch budget exceeded (never silently wrong)                           */
  TODHIP_EBUSY = -8,       /* pipeline: every ring slot holds a ticket that was not waited for yet / tickets outstanding   */
  TODHIP_ETIMEOUT = -9     /* pipeline: the ticket was not finished within timeout_ms; it stays waitable                   */
} todhip_status;

typedef struct todhip_ctx todhip_ctx;

/* One trained object as the DB hands it over (DescriptorMatcher.cpp:72-86):
 * `descriptors` attachment = n x desc_bytes CV_8U, `points` attachment = n x 3 f32 (object frame). */
typedef struct { const uint8_t* desc; const float* pts_xyz; uint32_t n; } todhip_object;

/* Same layout as cv::DMatch: the adapter reinterprets, no conversion. */
typedef struct { int32_t queryIdx, trainIdx, imgIdx; float distance; } todhip_dmatch;

/* glibc rand() state (random_r TYPE_3). The reference calls the process-global, never-seeded
 * rand() (sac_model_registration_graph.h:111, sac.h:71); here the stream is explicit (decision D4). */
typedef struct { uint32_t s[31]; uint32_t f, b; uint64_t draws; } todhip_rng;

/* GuessGenerator parameters, GuessGenerator.cpp:71-81 (defaults 15 / 1000 / 0.01). */
typedef struct { uint32_t min_inliers, n_ransac_iterations; float sensor_error; } todhip_verify_params;

/* One PoseResult (GuessGenerator.cpp:223-230): R row-major, pose maps object -> camera frame. */
typedef struct { uint32_t object; float R[9]; float t[3]; uint32_t inlier_begin, inlier_end; } todhip_pose;

/* Counters a cell would have printed to stdout (DescriptorMatcher.cpp:68-122, GuessGenerator.cpp:177-243). */
typedef struct {
  uint64_t db_rows, db_objects;
  uint32_t last_nq, last_k, last_matches;
  uint32_t last_objects_verified, last_rounds, last_hypotheses, last_gate_calls, last_poses;
  double   last_match_kernel_ms;      /* HIP-event time of the dominant matcher kernel (if timing enabled) */
  double   sum_match_kernel_ms;
  uint64_t n_match_kernel_launches;
  uint32_t last_sprint_launches;      /* verifier: launches of the single-wave small-object kernel in the last call ... */
  uint32_t last_sprint_rounds;        /* ... and the Ransac rounds (adjacency_ransac.cpp:234-309) it ran without the host */
  uint32_t last_verify_ticks;         /* host round trips (launch + synchronize) of the last verify call */
  uint32_t last_block_split;          /* matrix-core matcher: the block form of the last launch (4 = whole, 2 / 3: todhip_set_matcher_block_split) */
  /* matrix-core matcher, launches with split blocks (partial-distance elimination): accumulator blocks started as
   * parts, and those that went on to their second part -- cumulative over the context's life, as of the last report read */
  uint64_t k4x_half_blocks, k4x_half_blocks_completed;
  uint32_t last_fp4_rows;             /* matrix-core matcher: 1 if the last launch read the rows from their resident fp4 copy */
  uint32_t fp4_rows_builds;           /* ... and how often this context has built that copy (once per change of the searched rows) */
} todhip_counters;

/* ---- lifetime ---------------------------------------------------------------------------------- */
int  todhip_version(void);
/* stream == NULL: the context creates and owns a non-blocking stream. */
int  todhip_create(int device, void* hip_stream, todhip_ctx** out);
void todhip_destroy(todhip_ctx*);
void* todhip_stream(todhip_ctx*);
int  todhip_last_hip_error(const todhip_ctx*);
int  todhip_synchronize(todhip_ctx*);
int  todhip_get_counters(todhip_ctx*, todhip_counters* out);
/* Streams for contexts that run side by side (a pipeline: ORB, matcher and verifier contexts, each on a stream of its own, as
 * bench.py and tod_amd/pipeline.py drive them). todhip_set_cu_partition(n) reserves the device's last n compute units for
 * TODHIP_STREAM_LATENCY streams (the short, latency-bound kernels of ORB and of the verifier -- a single wave for hundreds of
 * microseconds -- which otherwise share every SIMD with the matcher's chip-filling DB pass); TODHIP_STREAM_THROUGHPUT streams get
 * the other compute units. n = 0 (the default, or the environment's TODHIP_LATENCY_CUS): no partition, latency streams are plain
 * high-priority streams. Process-wide; applies to streams created afterwards (the verifier's own side streams -- the lanes its
 * single-wave launch groups run on: sprints, clique gates, growth -- are latency streams and are re-created on their next use).
 * A multiple of 8 takes the same share of every XCD. Measured: a pipeline whose matcher is the bound loses with any
 * partition; a verifier-bound one (frames of ~190 objects) gains 15 % with the matcher alone confined to 160 of 256 CUs. */
enum { TODHIP_STREAM_THROUGHPUT = 0, TODHIP_STREAM_LATENCY = 1 };
int  todhip_set_cu_partition(uint32_t latency_cus);
int  todhip_stream_create(int device, int kind, void** stream_out);
int  todhip_stream_destroy(void* stream);
int  todhip_set_kernel_timing(todhip_ctx*, int enable);   /* bracket the matcher kernel with HIP events */
/* The exact Hamming search of todhip_match* exists twice, with identical results: on the vector ALU (xor + popcount,
 * partial-distance elimination: data dependent) and on the matrix cores (bits as +-1 MX-fp4 values, dot = 256 - 2 d:
 * data independent). AUTO picks by launch shape. */
enum { TODHIP_ENGINE_AUTO = 0, TODHIP_ENGINE_VALU = 1, TODHIP_ENGINE_MFMA = 2 };
int  todhip_set_matcher_engine(todhip_ctx*, int engine);
/* The matrix-core engine's partial-distance elimination: a 32 x 32 block's 256 bit positions are 4 matrix instructions, and the
 * block may stop after the first `split` of them when no partial sum can still reach a threshold (exact for any data). Which split
 * pays depends on the data, so the default (-1) adapts per context from the launches' own statistics; 0 = whole blocks, 2 / 3 = always
 * that split where the radius allows it (2: radius < 64, 3: radius < 96). Identical results in every setting. */
int  todhip_set_matcher_block_split(todhip_ctx*, int split);

/* ---- stage B: DescriptorMatcher ---------------------------------------------------------------- */
/* Replaces DescriptorMatcher::parameter_callback (DescriptorMatcher.cpp:60-129): ingest every object,
 * compute spans (:104-121), build the device-resident DB. With shard_count > 1 the descriptor rows are
 * split into object-aligned contiguous shards and only shard `shard_rank` is kept on this device; model
 * points and the object table are always complete. spans_out (n_objs floats) may be NULL. */
int todhip_db_load(todhip_ctx*, const todhip_object* objs, uint32_t n_objs, uint32_t desc_bytes,
                   uint32_t shard_rank, uint32_t shard_count, float* spans_out);
/* The same ingest from attachments that are already in this device's memory (objs[i].desc / .pts_xyz are device pointers, e.g.
 * todhip_model_device's): device-to-device copies, the spans computed there (identical values), n_objs floats come back. */
int todhip_db_load_device(todhip_ctx*, const todhip_object* objs, uint32_t n_objs, uint32_t desc_bytes,
                          uint32_t shard_rank, uint32_t shard_count, float* spans_out);
int todhip_db_info(const todhip_ctx*, uint64_t* total_rows, uint64_t* shard_first_row, uint64_t* shard_rows,
                   uint32_t* n_objs);
/* The desc_bytes of the resident DB (0 before the first load): what a query row of todhip_match* must measure. */
int todhip_db_desc_bytes(const todhip_ctx*, uint32_t* desc_bytes);

/* Descriptor widths. desc_bytes == 32: 256-bit binary rows (ORB / rBRIEF), Hamming. desc_bytes == 512: 128 x f32, L2
 * (todhip_match_l2*, one device). desc_bytes == 64: 512-bit binary rows -- BRISK, FREAK, BRIEF-64 -- Hamming, any shard_count, host
 * or device source. desc_bytes == 256: 64 x f32, L2, the second float width (see todhip_match_l2). Anything else: TODHIP_EINVAL. A narrower binary descriptor (AKAZE's 61 bytes) is used by zero-padding rows AND
 * queries to 64 bytes: the padding adds nothing to any distance.
 * On a DB loaded with desc_bytes == 64, todhip_match, todhip_match_device and todhip_match_shard_device with
 * todhip_merge_shards_device[_on] perform the same exact search as on a 32-byte DB, definition unchanged: Hamming distance over all
 * 512 bits; the k <= 8 nearest rows in the order (distance ascending, global row ascending), truncated at the first
 * distance > radius; (imgIdx, trainIdx) and the 3D point resolved as before; `distance` is the integer as a float, 0 ... 512;
 * queries are nq x 64 bytes. radius >= 512 cuts nothing (pass >= 512 to todhip_match_shard_device for the plain top-k),
 * radius == 0 stays TODHIP_EINVAL. todhip_set_ratio_test applies unchanged (the true two nearest rows, however far),
 * todhip_db_select_objects too (the view then takes 64 bytes per selected row). The definition is oracle/tod_oracle.cpp
 * orc_match_ratio(desc_bytes = 64).
 * One engine serves every launch size at this width (the matrix cores, 8 instructions per 32 x 32 block, dot = 512 - 2 d, whole
 * blocks): todhip_set_matcher_engine and todhip_set_matcher_block_split are accepted and have no effect, last_block_split reports
 * 4, todhip_set_kernel_timing brackets the DB pass as on a 32-byte DB.
 * What a 64-byte DB refuses or ignores:
 *   todhip_match_radius[_device], todhip_match_l2[_device]   TODHIP_EINVAL.
 *   todhip_match_l2_radius[_device]                          TODHIP_EINVAL.
 *   todhip_match_radius_shard_device,
 *   todhip_merge_radius_shards_device[_on]                   TODHIP_EINVAL.
 *   the match calls while todhip_set_lsh is enabled          TODHIP_EINVAL before any device work (no index is built at this width).
 *   todhip_set_db_bit_order                                  the mode may be set; the rows stay in identity order and the results
 *                                                            are those of the definition.
 *   todhip_pipeline_db_load[_device]                         TODHIP_EINVAL (the pipeline's ORB stage emits 32 bytes).
 *   todhip_model_*                                           trained models stay 32 bytes per row. */

/* Restrict every later match on this context to the rows of the listed objects (indices into the objs[] of the last
 * todhip_db_load[_device]); ids == NULL: all objects again (the state after a load). The list may be in any order and may
 * repeat an index; an index >= n_objs: TODHIP_EINVAL and the previous selection stays. n_ids == 0 with ids != NULL selects
 * nothing: every query then comes back with count 0. A new todhip_db_load[_device] resets the selection to all.
 * The reference's detector is told which objects to find (json_object_ids, detector.py:53-60, conf/detection.ork:22) and
 * DescriptorMatcher::parameter_callback builds its matcher from those alone. Definition: with S the ascending list of the distinct
 * selected indices, todhip_match, todhip_match_device, todhip_match_shard_device and todhip_merge_shards_device[_on] return what a
 * context loaded with only objs[S[0]], objs[S[1]], ... (same shard arguments) would return, except that imgIdx is S[imgIdx'], the
 * index in the full DB, and the u64 keys of the sharded form carry rows of the full DB -- so ranks that hold different parts of S
 * merge as before. The ratio test sees the two nearest SELECTED rows, the LSH mode indexes the selected rows, a bit order
 * (todhip_set_db_bit_order) stays the one the load computed. Spans, todhip_db_info, the model points and the verifier's
 * span-by-object-index input do not change. The selected rows of this context's shard are copied into a second buffer (desc_bytes per
 * row beside the full DB; none while all objects are selected).
 * Binary DBs only (desc_bytes == 32 or 64): on a float DB (desc_bytes == 512) TODHIP_EINVAL. Without a DB TODHIP_ENODB. Synchronizes the context's
 * stream, as todhip_db_load does; after TODHIP_EHIP all objects are selected. */
int todhip_db_select_objects(todhip_ctx*, const uint32_t* ids, uint32_t n_ids);
/* what is selected now: number of distinct selected objects, their rows in the whole DB and in this context's shard (any pointer
 * may be NULL) */
int todhip_db_selection(const todhip_ctx*, uint32_t* n_selected_objs, uint64_t* selected_rows, uint64_t* selected_shard_rows);

/* Replaces DescriptorMatcher::process (DescriptorMatcher.cpp:195-252): exact Hamming k-NN (decision D1,
 * instead of FLANN-LSH knnMatch(k=5) at :211), radius truncation (:212-220; radius is the reference's
 * `unsigned int radius_`, 0 is rejected because the reference then indexes an empty vector at :237) and
 * the match -> 3D gather (:231-244). Outputs in CSR form: row_ptr[nq+1], matches/matches_xyz capacity nq*k. */
int todhip_match(todhip_ctx*, const uint8_t* q_desc, uint32_t nq, uint32_t k, uint32_t radius,
                 uint32_t* row_ptr, todhip_dmatch* matches, float* matches_xyz);

/* Lowe's ratio test, the step the reference announces and leaves empty (DescriptorMatcher.cpp:223-227; its shipped configs
 * ask for ratio 0.8, conf/detection.ork:39, which its `unsigned int ratio_` turns into 0 = off). Off by default; when set
 * (0 < ratio <= 1), every todhip_match* form drops all matches of a query whose two nearest DB rows (d1 <= d2, exact, over
 * the whole DB whatever the radius) do not satisfy (float)d1 < ratio * (float)d2; a one-row DB passes. The radius cut then
 * applies to the survivors. The sharded forms need k >= 2 while it is on. Definition = oracle/tod_oracle.cpp
 * orc_match_ratio (there is no reference behaviour to be identical to). */
int todhip_set_ratio_test(todhip_ctx*, float ratio);

/* Optional LSH-approximate mode (SURVEY 8(f) N4 c). The reference's matcher is cv::FlannBasedMatcher over
 * cv::flann::LshIndexParams(n_tables, key_size, multi_probe_level) (DescriptorMatcher.cpp:175-180; conf/detection.ork:32-38:
 * 10 tables, 16-bit keys, level 1); this library answers that configuration with the EXACT search by default (a superset of
 * what any LSH index returns). With n_tables > 0 every todhip_match* form on 32-byte descriptors ranks, instead of the whole
 * shard, only the rows an index of FLANN's published scheme turns up: per table a key of key_size descriptor bits (table t uses
 * the first key_size entries of a Fisher-Yates shuffle of 0..255 driven by a 32-bit mix of (t, step): FLANN draws them from
 * rand(), which cannot be reproduced -- parity unpinned, the CPU checker is oracle/lsh_oracle.c); a query's candidates are the
 * rows whose key differs from its own in at most multi_probe_level bits in at least one table; the k nearest of those by exact
 * distance, ties by row. Radius cut, ratio test (on the candidates' two nearest) and the sharded forms work as before.
 * n_tables = 0 switches back to the exact search. Limits: n_tables <= 32, key_size <= 24, multi_probe_level <= 3.
 * May be called before or after todhip_db_load (the index is built for the resident shard either way). */
int todhip_set_lsh(todhip_ctx*, uint32_t n_tables, uint32_t key_size, uint32_t multi_probe_level);

/* Optional exact bit order of the resident Hamming DB. The matrix-core engine's partial-distance elimination
 * (todhip_set_matcher_block_split) only fires when the bit positions a block evaluates first are informative; descriptors whose
 * leading positions are biased or correlated (rBRIEF patterns trained elsewhere, cv::ORB) make nearly every block go on. With
 * TODHIP_BIT_ORDER_INFORMATIVE_FIRST the todhip_db_load[_device] calls that follow permute the bit positions of the shard's rows, and
 * every todhip_match* form permutes its queries the same way into a workspace of the context (the caller's buffer is never written):
 * Hamming distance does not depend on the order, so row indices, distances and everything behind them are those of the unordered DB,
 * and the LSH mode reads its key bits through the inverse map (same keys, same candidates). Off by default; desc_bytes == 32 only
 * (a 512-byte float DB ignores it). The order belongs to the context and its resident shard: every shard of a sharded DB computes
 * its own. A later load in mode TODHIP_BIT_ORDER_NONE restores the identity.
 * Bit i of a descriptor is bit i % 8 (LSB first) of byte i / 8 = bit i % 32 of little-endian dword i / 32.
 * Definition (exact integers, deterministic). Sample: S = min(shard_rows, 65536), sample row i = row floor(i * shard_rows / S);
 * ones[b] = sample rows with bit b set, both[a][b] = with bits a and b set. v[b] = ones[b] (S - ones[b]). Candidates: v descending,
 * ties by ascending b. Walking them once, b is accepted iff v[b] > 0 and 4 c(a, b)^2 < v[a] v[b] for every a accepted before it,
 * c(a, b) = |S both[a][b] - ones[a] ones[b]| (|correlation| < 1/2: the ORB paper's greedy step with one fixed threshold). Ranks:
 * the accepted bits, then the rejected ones (constant bits, copies of earlier bits), each in candidate order. Rank r is stored at
 * position 32 E[r / 32] + r % 32, E = {0, 4, 1, 5, 2, 6, 3, 7}: a matrix instruction of a block covers dwords s and s + 4 of a row,
 * so ranks 0-63 are what a block sees first, 0-127 what a 2-split sees. The layout serves the matrix-core engine; the vector-ALU
 * engine tests after dwords 0-2, 0-3 and 0-5 and so sees ranks 0-31, 64-95 and 128-159 first -- exact all the same, but not the
 * best order for that engine. Any other mode, or a null pointer: TODHIP_EINVAL. */
enum { TODHIP_BIT_ORDER_NONE = 0, TODHIP_BIT_ORDER_INFORMATIVE_FIRST = 1 };
int todhip_set_db_bit_order(todhip_ctx*, int mode);
/* The order of the resident DB: stored position p holds original bit src_of[p]. The identity while the option is off or nothing
 * is loaded. */
int todhip_db_bit_order(const todhip_ctx*, uint8_t src_of[256]);

/* Device-resident form of the same call (inputs already in HBM, outputs stay in HBM):
 * d_counts[nq] (matches kept per query), d_matches[nq*k], d_matches_xyz[nq*k*3], fixed stride k. */
int todhip_match_device(todhip_ctx*, const void* d_q_desc, uint32_t nq, uint32_t k, uint32_t radius,
                        void* d_counts, void* d_matches, void* d_matches_xyz);

/* Float descriptors (BASELINE.json configs[3]; not a reference feature -- the reference's matcher throws for anything
 * but FLANN-LSH on binary descriptors, DescriptorMatcher.cpp:154-188): a DB loaded with desc_bytes == 512 (128 x f32 per
 * row, one device) is searched by exact L2 k-NN, k <= 8. Result shape as todhip_match[_device] (DescriptorMatcher.cpp:
 * 195-252): order (distance asc, global row asc), truncated at the first distance > radius; DMatch.distance =
 * sqrtf(d2), d2 = sum over i = 0..127 in index order of (q[i] - r[i])^2 in IEEE binary32 without fused multiply-add
 * (the CPU checker of this definition is oracle/l2_oracle.c). The candidates come from a
 * bf16 MFMA GEMM whose distance from d2 is bounded by eps(q) = 2^-6 (1 + 2^-6) |q| Rmax + 2^-14 (|q| + Rmax)^2 (derived in
 * tod_amd/csrc/l2_bound.h, held against binary64 on worst-case inputs by tests/l2_bound_host_test.cpp and on the GPU by
 * tests/test_l2_numerics_gpu.py), the final order from the exact distances.
 * Domain (this call and todhip_match_l2_radius): every component of the DB and of the queries is finite, and every squared norm
 * |q|^2, |r|^2 is zero or lies in [2^-64, 2^64], so that no square, product or sum of the search leaves the normal range of
 * binary32 (a score stays far below the 3e38 that marks a padding row, and no bf16 product underflows). The bound is relative: it
 * says nothing about a DB or a query whose norms underflow, and outside the domain the result is not defined.
 * Batch form: the nq queries may be those of F frames (F x Q rows, frame f's query q at row f Q + q, which is also its
 * queryIdx): they share ONE pass over the DB, and every query's matches are those of a call that carried its frame alone
 * (16 frames of 1000 queries against 500k rows under the first, too narrow eps: 0.12 ms per frame instead of 0.19; under the
 * corrected one a 16-frame call has too few private candidate slots per query and is slower per frame than single calls, 0.75 ms
 * against 0.24: DESIGN 6b, "The bound").
 * Two widths: dim = desc_bytes / 4 ∈ {64, 128}. A DB loaded with desc_bytes == 256 is a float DB of 64 x f32 rows
 * (SURF's and KAZE's default width) and every float call of this header serves it -- todhip_db_load[_device] with any shard_count,
 * todhip_match_l2[_device], todhip_match_l2_radius[_device], the shard and merge pairs, todhip_set_l2_ratio_test,
 * todhip_cross_check_l2_device and todhip_set_l2_cross_check -- with the definitions given for desc_bytes == 512 and 127 read as
 * dim - 1: d2 = sum over i = 0..dim-1 in index order, distance = sqrtf(d2), order (d2, row), key = bits(d2) << 32 | row; queries are
 * nq x dim f32; the same eps(q) bounds the filter (tests/l2_dim64_bound_host_test.cpp). What a float DB refuses (the Hamming calls,
 * selections, LSH, the pipeline) it refuses at either width; any other desc_bytes is TODHIP_EINVAL at the load. */
int todhip_match_l2(todhip_ctx*, const float* q_desc, uint32_t nq, uint32_t k, float radius, uint32_t* row_ptr,
                    todhip_dmatch* matches, float* matches_xyz);
int todhip_match_l2_device(todhip_ctx*, const void* d_q_desc, uint32_t nq, uint32_t k, float radius, void* d_counts,
                           void* d_matches, void* d_matches_xyz);

/* The true L2 radius search over a float DB (desc_bytes == 512): every row within `radius` of a query, not the k <= 8 nearest cut at
 * the radius -- cv::DescriptorMatcher::radiusMatch for float descriptors, what todhip_match_radius is for 32-byte binary ones, and
 * for the same reason: a surface point is one row per training view, and k <= 8 hands the verifier a handful of those rows without
 * saying that the list was cut.
 * Definition (exact, deterministic):
 *   d2(q, r)     = sum over i = 0..127 in index order of (q[i] - r[i])^2 in IEEE binary32 without fused multiply-add, and
 *                  distance = sqrtf(d2): those of todhip_match_l2.
 *   R(q)         = the DB rows whose distance is NOT > radius (inclusive, the cut of todhip_match_l2). Descriptors are finite, as
 *                  todhip_match_l2 assumes; a d2 that overflows to +Inf is outside every radius.
 *   in_radius[q] = |R(q)|, exact, never truncated.
 *   matches of q = R(q) in the order (d2 ascending, global row ascending), cut after the first max_per_query <= 1024;
 *                  counts[q] = min(|R(q)|, max_per_query). queryIdx, trainIdx, imgIdx, distance and the gathered model point of a row
 *                  are exactly what todhip_match_l2 writes for it, so with max_per_query = k <= 8 the two calls agree bit for bit.
 *   The ratio test and the LSH mode do not apply. Batch form as todhip_match_l2: the nq queries may be those of F frames and share
 *   ONE pass over the DB.
 * Host form: CSR with todhip_match_radius's capacity rule. *n_matches: capacity of matches / matches_xyz (in matches) in, row_ptr[nq]
 * out; when it is too small: TODHIP_ECAPACITY with the needed count in *n_matches, row_ptr and in_radius filled, matches untouched.
 * in_radius may be NULL.
 * Device form: fixed stride max_per_query -- d_counts[nq] u32, d_matches[nq * max_per_query], d_matches_xyz[nq * max_per_query * 3],
 * d_in_radius[nq] u32 (may be NULL); the slots behind counts[q] are not written.
 * TODHIP_EINVAL: a null context, query or output pointer, nq == 0, max_per_query == 0 or > 1024, a radius that is not > 0 or not
 * finite, a DB that is not float (or is sharded). TODHIP_ENODB without a DB. todhip_get_counters: last_nq, last_k = max_per_query,
 * last_matches (host form); todhip_set_kernel_timing brackets the pass over the DB.
 * How: one pass of the k-NN call's bf16 GEMM with a threshold derived from the radius and the GEMM's error bound eps(q), the exact
 * distance of every candidate, a sort. A query whose candidate lists overflow (more than about 2000 candidates) is answered by a
 * second, ordered pass over the f32 rows for that query (same result). Workspace: the k-NN call's, with
 * nq * max_per_query * 8 bytes of keys. */
int todhip_match_l2_radius(todhip_ctx*, const float* q_desc, uint32_t nq, float radius, uint32_t max_per_query,
                           uint32_t* row_ptr /*[nq+1]*/, todhip_dmatch* matches, float* matches_xyz,
                           uint32_t* n_matches /* capacity in, count out */, uint32_t* in_radius /*[nq], may be NULL*/);
int todhip_match_l2_radius_device(todhip_ctx*, const void* d_q_desc, uint32_t nq, float radius, uint32_t max_per_query,
                                  void* d_counts /*[nq] u32*/, void* d_matches /*[nq*max_per_query]*/,
                                  void* d_matches_xyz /*[nq*max_per_query*3]*/, void* d_in_radius /*[nq] u32, may be NULL*/);

/* The float searches over a sharded DB, merged on the device: what todhip_match_shard_device + todhip_merge_shards_device[_on] and
 * todhip_match_radius_shard_device + todhip_merge_radius_shards_device[_on] (below) are to the Hamming searches. A float DB
 * (desc_bytes == 512) loads with any shard_count: the shard's rows alone are resident and prepared (their bf16 image, norms and
 * Rmax), model points and the object table are complete, an empty shard is legal. todhip_match_l2* and todhip_match_l2_radius* stay
 * TODHIP_EINVAL on a context that holds one shard of several; these six calls serve it (and an unsharded context, as one shard).
 * Definition (exact, deterministic):
 *   key          = (IEEE binary32 bits of d2) << 32 | row of the full DB, d2 the defining sequential f32 sum of todhip_match_l2.
 *                  d2 >= 0, so the order of the bits is the order of the values; row < 2^32, so the row cannot carry into the distance.
 *   k-NN, step 1 (todhip_match_l2_shard_device), on every rank: row q of d_keys, nq x k u64, holds the shard's min(k, shard rows)
 *                  nearest rows in key order, UINT64_MAX behind them. The plain top-k: the call takes no radius. EVERY slot is
 *                  written (the buffer goes through a collective as it is); a shard without rows writes padding only.
 *   k-NN, step 2 (todhip_merge_l2_shards_device[_on]), on the rank that owns the queries: d_keys_all is [n_shards][nq][k], step 1's
 *                  outputs. Per query the k smallest of the n_shards x k keys, cut at the first sqrtf(d2) > radius, each resolved as
 *                  todhip_match_l2_device resolves it (imgIdx, trainIdx, distance = sqrtf(d2), the gathered model point); fixed
 *                  stride k, slots behind counts[q] not written.
 *   radius, step 1 (todhip_match_l2_radius_shard_device): row q of d_keys, nq x (max_per_query + 1) u64, holds the first
 *                  min(|R_s(q)|, max_per_query) keys of R_s(q) -- the rows of R(q) in this shard -- ascending, UINT64_MAX behind
 *                  them, and |R_s(q)| as a u64 in slot max_per_query: the row todhip_match_radius_shard_device writes. Every slot
 *                  is written; a shard without rows writes padding and count 0.
 *   radius, step 2 (todhip_merge_l2_radius_shards_device[_on]): in_radius[q] = the sum of the shards' counts, counts[q] =
 *                  min(in_radius[q], max_per_query), the matches the first counts[q] keys of the union in key order, resolved as
 *                  todhip_match_l2_radius_device resolves them; fixed stride max_per_query, slots behind counts[q] not written.
 *   Result: the merged outputs (counts, the kept slots of matches and xyz, in_radius) are byte for byte what todhip_match_l2_device
 *   or todhip_match_l2_radius_device leaves on a context that holds the whole DB. Why: every shard's answer is its EXACT top-k or its
 *   exact radius set -- the bf16 filter with the shard's own Rmax and eps(q), and whichever path the shard's row count selects (seed
 *   and two GEMMs, one GEMM, the exact scan), only decide how the rows are found; the keys come from the defining d2 of each row --
 *   a key among the first n of the union is among the first n of its own shard's list, and keys are unique over the shards because the
 *   row is part of the key. The merge compares integers.
 *   The merges read only the context's object table and model points (every rank holds the full DB's), so any rank's context will do,
 *   and the _on forms may run on a stream of the caller's beside a shard call that is in flight on the context's own, as
 *   todhip_merge_shards_device_on does; the caller orders that stream against the producer of d_keys_all and the consumers.
 *   The ratio test, LSH, selections and the cross-check do not apply to float DBs, sharded or not.
 * TODHIP_EINVAL: a null pointer other than d_in_radius, nq == 0, k == 0 or > 8, max_per_query == 0 or > 1024, n_shards == 0 or > 64,
 * a radius that is not > 0 (or, for the radius pair's step 1, not finite), a DB that is not float. TODHIP_ENODB without a DB.
 * todhip_get_counters: step 1 sets last_nq and last_k (k, or max_per_query); todhip_set_kernel_timing brackets step 1's DB pass as
 * in the unsharded calls. The exchange carries world * nq * k * 8 or world * nq * (max_per_query + 1) * 8 bytes per rank and step
 * (DESIGN 6n). */
int todhip_match_l2_shard_device(todhip_ctx*, const void* d_q_desc, uint32_t nq, uint32_t k, void* d_keys /*[nq*k] u64*/);
int todhip_merge_l2_shards_device(todhip_ctx*, const void* d_keys_all, uint32_t n_shards, uint32_t nq, uint32_t k, float radius,
                                  void* d_counts /*[nq] u32*/, void* d_matches /*[nq*k]*/, void* d_matches_xyz /*[nq*k*3]*/);
int todhip_merge_l2_shards_device_on(todhip_ctx*, void* hip_stream, const void* d_keys_all, uint32_t n_shards, uint32_t nq, uint32_t k,
                                     float radius, void* d_counts, void* d_matches, void* d_matches_xyz);
int todhip_match_l2_radius_shard_device(todhip_ctx*, const void* d_q_desc, uint32_t nq, float radius, uint32_t max_per_query,
                                        void* d_keys /*[nq*(max_per_query+1)] u64*/);
int todhip_merge_l2_radius_shards_device(todhip_ctx*, const void* d_keys_all, uint32_t n_shards, uint32_t nq, uint32_t max_per_query,
                                         void* d_counts /*[nq] u32*/, void* d_matches /*[nq*max_per_query]*/,
                                         void* d_matches_xyz /*[nq*max_per_query*3]*/, void* d_in_radius /*[nq] u32, may be NULL*/);
int todhip_merge_l2_radius_shards_device_on(todhip_ctx*, void* hip_stream, const void* d_keys_all, uint32_t n_shards, uint32_t nq,
                                            uint32_t max_per_query, void* d_counts, void* d_matches, void* d_matches_xyz,
                                            void* d_in_radius /*may be NULL*/);

/* Sharded form, step 1: this shard's top-k per query as keys (distance << 32 | global_row), ascending,
 * UINT64_MAX padded; d_keys[nq*k]. The ranks exchange these with one RCCL all-gather. `radius` is the radius of
 * step 2: rows farther away never survive the truncation of DescriptorMatcher.cpp:212-220, so the search is
 * allowed to leave them out of the keys (it is not obliged to); pass >= 256 to get the plain top-k. */
int todhip_match_shard_device(todhip_ctx*, const void* d_q_desc, uint32_t nq, uint32_t k, uint32_t radius, void* d_keys);
/* Sharded form, step 2: merge n_shards key sets (layout [shard][nq][k]) with the total order
 * (distance asc, global row asc), apply the radius cut, resolve (imgIdx, trainIdx), gather 3D. */
int todhip_merge_shards_device(todhip_ctx*, const void* d_keys_all, uint32_t n_shards, uint32_t nq, uint32_t k,
                               uint32_t radius, void* d_counts, void* d_matches, void* d_matches_xyz);

/* The same merge launched on a stream of the caller's instead of the context's: it only READS the context's immutable
 * object table and model points, so it may run beside a todhip_match_shard_device call that is in flight on the context's
 * own stream (the multi-GPU step puts collectives + merge on a second stream, tod_amd/sharded.py). The caller orders the
 * stream against the producer of d_keys_all and the consumers of the outputs. */
int todhip_merge_shards_device_on(todhip_ctx*, void* hip_stream, const void* d_keys_all, uint32_t n_shards, uint32_t nq,
                                  uint32_t k, uint32_t radius, void* d_counts, void* d_matches, void* d_matches_xyz);

/* The true radius search: every searched row within `radius` bits of a query, not the k <= 8 nearest cut at the radius. The
 * reference documents `radius` as "for epsilon nearest neighbor search" (DescriptorMatcher.cpp:137) and falls back to knnMatch(5)
 * plus a cut only because "this does not work for LSH on OpenCV 2.4" (:201-220); this is cv::DescriptorMatcher::radiusMatch, the
 * third member of match / knnMatch / radiusMatch. On self-similar texture a query has hundreds of model rows inside the radius (a
 * surface point is one row per training view) and k = 5 hands the verifier five of them without saying so.
 * Definition (exact, deterministic):
 *   d(q, r)      = popcount of the xor of the two 32-byte descriptors.
 *   R(q)         = the searched rows with d(q, r) <= radius (inclusive, as the cut of todhip_match drops distance > radius);
 *                  radius >= 256 puts every searched row in R(q).
 *   in_radius[q] = |R(q)|, exact, never truncated.
 *   matches of q = R(q) in the library's total order (distance ascending, then row of the full DB ascending), cut after the first
 *                  max_per_query; counts[q] = min(|R(q)|, max_per_query). queryIdx, trainIdx, imgIdx, distance and the gathered model
 *                  point of a row are exactly what todhip_match writes for it.
 *   searched rows = what todhip_match* searches on this context: the resident shard, in the numbering of the full DB. On a context
 *                  loaded with shard_count > 1 each rank answers for its own rows; the ranks' answers are merged on the device by
 *                  todhip_match_radius_shard_device + todhip_merge_radius_shards_device[_on] below. todhip_db_select_objects
 *                  is honoured: the result is that of a context loaded with the selected objects alone, imgIdx in the full DB's
 *                  numbering; an empty selection gives all counts 0. todhip_set_db_bit_order is honoured: the queries are permuted as
 *                  the other forms permute them, the results do not change.
 *   The ratio test and the LSH mode do NOT apply: this is the exact search over all searched rows whatever todhip_set_ratio_test and
 *   todhip_set_lsh say.
 * Host form: CSR like todhip_match. *n_matches: capacity of matches / matches_xyz (in matches) in, row_ptr[nq] out; when it is too
 * small: TODHIP_ECAPACITY with the needed count in *n_matches, row_ptr and in_radius filled, matches untouched. in_radius may be NULL.
 * Device form: fixed stride max_per_query like todhip_match_device's stride k -- d_counts[nq] u32, d_matches[nq * max_per_query],
 * d_matches_xyz[nq * max_per_query * 3], d_in_radius[nq] u32 (may be NULL); the slots behind counts[q] are not written, as
 * todhip_match_device leaves them.
 * TODHIP_EINVAL: a null context, query or output pointer, nq == 0, radius == 0, max_per_query == 0 or > 1024, a float DB
 * (desc_bytes == 512) or a 64-byte binary one. TODHIP_ENODB without a DB. todhip_get_counters: last_nq, last_k = max_per_query, last_matches (host form);
 * todhip_set_kernel_timing brackets the DB pass.
 * Workspace: a candidate buffer of nq * C * 8 bytes, C = 2 * max_per_query rounded up to a power of two, at least 64, plus
 * nq * (min(radius, 256) + 2) * 4 bytes of counters. A query with at most C rows inside the radius is answered from the one DB pass;
 * one with more is answered by a second, ordered pass over the rows for that query (same result). */
int todhip_match_radius(todhip_ctx*, const uint8_t* q_desc, uint32_t nq, uint32_t radius, uint32_t max_per_query,
                        uint32_t* row_ptr /*[nq+1]*/, todhip_dmatch* matches, float* matches_xyz,
                        uint32_t* n_matches /* capacity in, count out */, uint32_t* in_radius /*[nq], may be NULL*/);
int todhip_match_radius_device(todhip_ctx*, const void* d_q_desc, uint32_t nq, uint32_t radius, uint32_t max_per_query,
                               void* d_counts /*[nq] u32*/, void* d_matches /*[nq*max_per_query]*/,
                               void* d_matches_xyz /*[nq*max_per_query*3]*/, void* d_in_radius /*[nq] u32, may be NULL*/);

/* The radius search over a sharded DB, merged on the device: what todhip_match_shard_device + todhip_merge_shards_device[_on] are to
 * todhip_match_device. R_s(q): the rows of R(q) that this context searches (its shard, under its selection).
 * Step 1, on every rank. Row q of d_keys, nq x (max_per_query + 1) u64:
 *   slots [0, max_per_query)   the min(|R_s(q)|, max_per_query) nearest rows of R_s(q) as keys distance << 32 | row of the full DB,
 *                              ascending; UINT64_MAX behind them.
 *   slot max_per_query         |R_s(q)| as a u64, exact, never truncated.
 *   EVERY slot of the buffer is written: it goes through a collective as it is. The searched rows, selections (keys in the full DB's
 *   numbering), the bit order and "the ratio test and LSH do not apply" are those of todhip_match_radius_device on this context; a
 *   shard or selection without rows writes all-padding rows with count 0. Refusals: those of todhip_match_radius_device.
 * Step 2, on the rank that owns the queries. d_keys_all: [n_shards][nq][max_per_query + 1] u64, step 1's outputs. Per query:
 *   in_radius[q] = the sum of the shards' counts; counts[q] = min(in_radius[q], max_per_query); the matches are the first counts[q]
 *   keys of the union of the shards' keys in key order, resolved and gathered as todhip_match_radius_device does, fixed stride
 *   max_per_query, slots behind counts[q] not written: byte for byte what todhip_match_radius_device leaves for an unsharded context
 *   on the same DB. Why: a key among the first max_per_query of the union of all R_s(q) is preceded by fewer than max_per_query keys
 *   of its own shard, so it is among that shard's first max_per_query -- the global first max_per_query lie inside the union of the
 *   per-shard first max_per_query -- and the keys (distance, row) are unique over the shards.
 *   The merge reads only the context's object table and model points (every rank holds the full DB's), so any rank's context will
 *   do, and the _on form may run on a stream of the caller's beside a DB pass on the context's own, as
 *   todhip_merge_shards_device_on does; the caller orders that stream against the producer of d_keys_all and the consumers.
 *   TODHIP_EINVAL: a null pointer other than d_in_radius, nq == 0, n_shards == 0 or > 64, max_per_query == 0 or > 1024, a DB that
 *   is not 32-byte binary. TODHIP_ENODB without a DB.
 * The exchange carries world * nq * (max_per_query + 1) * 8 bytes per rank and step. */
int todhip_match_radius_shard_device(todhip_ctx*, const void* d_q_desc, uint32_t nq, uint32_t radius, uint32_t max_per_query,
                                     void* d_keys /*[nq*(max_per_query+1)] u64*/);
int todhip_merge_radius_shards_device(todhip_ctx*, const void* d_keys_all, uint32_t n_shards, uint32_t nq, uint32_t max_per_query,
                                      void* d_counts /*[nq] u32*/, void* d_matches /*[nq*max_per_query]*/,
                                      void* d_matches_xyz /*[nq*max_per_query*3]*/, void* d_in_radius /*[nq] u32, may be NULL*/);
int todhip_merge_radius_shards_device_on(todhip_ctx*, void* hip_stream, const void* d_keys_all, uint32_t n_shards, uint32_t nq,
                                         uint32_t max_per_query, void* d_counts, void* d_matches, void* d_matches_xyz,
                                         void* d_in_radius /*may be NULL*/);

/* The cross-check, cv::BFMatcher(normType, crossCheck = true): a match stays only where its query is the nearest query of its frame
 * to the DB row it names. The ratio test judges a query's list in isolation; this filter sees that many keypoints of a frame claim
 * the same model row and keeps the one that is nearest to it.
 * Inputs: a match output in the fixed-stride device layout -- d_counts[nq] u32, d_matches[nq * stride], d_matches_xyz[nq * stride * 3],
 * what todhip_match_device, todhip_merge_shards_device[_on], todhip_match_radius_device and todhip_merge_radius_shards_device[_on]
 * leave, stride = k or max_per_query --, the nq query descriptors that produced it (d_q_desc, rows of the DB's width), a frame size
 * frame_queries = Q >= 1 and optionally the host array frame_nq[n_frames], n_frames = ceil(nq / Q).
 * Definition (exact, deterministic):
 *   frame f      owns query rows f Q ... min((f + 1) Q, nq) - 1. Its valid queries V(f) are the first min(frame_nq[f], rows of f) of
 *                those rows; all of them when frame_nq is NULL.
 *   g(m)         = the row of the full DB that match m names: obj_off[imgIdx] + trainIdx.
 *   d(q, g)      = the Hamming distance over the DB's width (256 or 512 bits).
 *   A kept match m of query q in frame f survives iff q is in V(f) and no q' in V(f) has (d(q', g), q') < (d(q, g), q)
 *   lexicographically: q is the nearest valid query of its frame to row g, ties to the lower query index. With stride 1 this is
 *   BFMatcher's cross-check with ties to the first index.
 *   Survivors of a query keep their order and move to the front of the query's slots, each xyz beside its match; counts[q] becomes
 *   their number. Slots in [new counts[q], old counts[q]) are unspecified afterwards, slots at or behind the old counts[q] are not
 *   written. A query outside V(f) ends with counts[q] = 0. (A slot that names no row of the DB -- nothing a match call leaves -- is
 *   dropped.)
 *   The predicate depends on (q, g, V(f)) only, not on a query's list and not on other frames; the filter is idempotent. Behind the
 *   ratio test and the radius cut it filters what those two left. Selections (todhip_db_select_objects) and the LSH mode do not
 *   enter: the reverse search runs over the frame's queries, not over DB rows, and reads row g from the resident full DB. A bit
 *   order (todhip_set_db_bit_order) is honoured: the queries are permuted as every match form permutes them, the result does not
 *   change.
 * In place, asynchronous on the context's stream; frame_nq is copied before the call returns. Two kernels: the test (a lane per kept
 * match holds its DB row in registers, the frame's valid queries pass through LDS) and an order-preserving compaction per query
 * (DESIGN 6m).
 * TODHIP_EINVAL: a null context, query or output pointer, nq == 0, frame_queries == 0, stride == 0 or > 1024 (or nq * stride >=
 * 2^31), a float DB (desc_bytes == 512), a context whose resident shard is not the whole DB (loaded with shard_count > 1: the rows a
 * match names are then not all resident -- filter a sharded DB's merged output on a context that holds the whole DB).
 * TODHIP_ENODB without a DB. */
int todhip_cross_check_device(todhip_ctx*, const void* d_q_desc, uint32_t nq, uint32_t frame_queries,
                              const uint32_t* frame_nq /* host, [ceil(nq / frame_queries)], may be NULL */,
                              uint32_t stride, void* d_counts, void* d_matches, void* d_matches_xyz);
/* Switches the cross-check on for todhip_match and todhip_match_device: while frame_queries = Q > 0, those two calls run
 * todhip_cross_check_device(Q, frame_nq = NULL, stride = k) behind their finalize step (the host form packs its CSR from the
 * filtered counts). 0 = off, the default: no launch is added and every output is what it was. The sharded and the radius entry points
 * (todhip_match_shard_device, todhip_merge_shards_device[_on], todhip_match_radius*, todhip_merge_radius_shards_device[_on]) and the
 * float forms ignore the setting: a caller filters their device outputs with todhip_cross_check_device itself.
 * TODHIP_EINVAL, and the setting does not change: Q > 0 on a context whose DB is float or is one shard of several. */
int todhip_set_cross_check(todhip_ctx*, uint32_t frame_queries /* 0 = off, the default */);

/* Lowe's ratio test against ANOTHER OBJECT than the nearest match's -- todhip_other_object_min_device, todhip_ratio_other_apply_device,
 * todhip_ratio_other_device, todhip_set_ratio_test_other -- is declared and defined in todhip_ratio_other.h, which this header
 * includes at its end: a host that includes todhip.h has those four calls. */

/* The two filters of the float forms (a DB of desc_bytes == 512). todhip_set_ratio_test and todhip_set_cross_check do not apply to the
 * float forms, whatever the comments above say about "every todhip_match* form": they keep their behaviour on every context (a host
 * that set them on a shared context keeps its results), and the float forms have setters of their own -- todhip_set_l2_ratio_test,
 * todhip_set_l2_cross_check -- and a filter of their own, todhip_cross_check_l2_device. With all of them off every float call leaves
 * byte for byte what it left before they existed.
 *
 * Lowe's ratio test on L2 distances, the descriptors the criterion was defined for. ratio: 0 = off, the default; 0 < ratio <= 1 = on;
 * anything else, NaN included, is TODHIP_EINVAL and leaves the setting unchanged. It may be called with any DB or none.
 * Definition: while on, every query of todhip_match_l2, todhip_match_l2_device and todhip_merge_l2_shards_device[_on] is tested on its
 *   two nearest rows over the whole DB (the union of the shards), whatever the radius: the two smallest keys in the library's order
 *   (d2, row), d2 the exact defining sum. With dist = sqrtf(d2) in binary32 the query keeps its matches iff dist1 < ratio * dist2 --
 *   one binary32 product, nothing fused -- and otherwise all of its matches are dropped (counts[q] = 0). A DB, or a union of shards,
 *   with one row passes. Two rows at equal distance fail even at ratio 1, as they do for the Hamming forms. The radius cut applies
 *   to the survivors. k == 1 searches two rows internally and returns one. todhip_match_l2_shard_device and the k-NN merge return
 *   TODHIP_EINVAL for k < 2 while it is on (the merge needs every shard's second nearest row; it reads the setting of the context it
 *   is called on). todhip_match_l2_radius* and their merges ignore it, as the Hamming radius forms ignore todhip_set_ratio_test.
 *   The predicate is stated once, in tod_amd/csrc/l2_filters.h (l2_ratio_passes). It adds no launch. */
int todhip_set_l2_ratio_test(todhip_ctx*, float ratio /* 0 = off, the default */);

/* The cross-check over a float DB, cv::BFMatcher(NORM_L2, crossCheck = true): todhip_cross_check_device's definition word for word --
 * frames, V(f), g(m), in place, survivors keep their order and move to the front with their xyz, slots in [new counts[q], old
 * counts[q]) unspecified, nothing written at or behind the old counts[q], a query outside V(f) ends with counts[q] = 0, idempotent,
 * frame_nq is copied before the call returns -- and only the distance differs:
 *   d(q, g)      = the IEEE binary32 bits of d2(q, row g), the defining sequential sum of todhip_match_l2 without fused multiply-add,
 *                  compared as unsigned integers (d2 >= 0, so the order of the bits is the order of the values). The query's own
 *                  d(q, g) is computed again from the descriptors, not taken from DMatch.distance.
 * d_q_desc: the nq query rows of 128 f32 that produced the output. It accepts any fixed-stride float output, stride 1 ... 1024: what
 * todhip_match_l2_device, todhip_match_l2_radius_device, todhip_merge_l2_shards_device[_on] and
 * todhip_merge_l2_radius_shards_device[_on] leave.
 * Two kernels: the test (a lane per kept match holds its DB row in 128 registers; a frame's valid queries are cut into chunks over
 * workgroups, pass through LDS, four at a time per lane; exact early exit on the partial sums) and todhip_cross_check_device's
 * compaction.
 * TODHIP_EINVAL: a null context, query or output pointer, nq == 0, frame_queries == 0, stride == 0 or > 1024 (or nq * stride >=
 * 2^31), a DB that is not float, a context that does not hold the whole DB (filter a sharded DB's merged output on a context that
 * does). TODHIP_ENODB without a DB. */
int todhip_cross_check_l2_device(todhip_ctx*, const void* d_q_desc, uint32_t nq, uint32_t frame_queries,
                                 const uint32_t* frame_nq /* host, [ceil(nq / frame_queries)], may be NULL */,
                                 uint32_t stride, void* d_counts, void* d_matches, void* d_matches_xyz);
/* Switches it on for todhip_match_l2 and todhip_match_l2_device: while frame_queries = Q > 0, those two calls run
 * todhip_cross_check_l2_device(Q, frame_nq = NULL, stride = k) behind their finalize step, that is behind the ratio test and the
 * radius cut (the host form packs its CSR from the filtered counts). 0 = off, the default: no launch is added. The shard, merge and
 * radius entry points of the float forms ignore it.
 * TODHIP_EINVAL, and the setting does not change: Q > 0 on a context whose resident DB is binary or is one shard of several. */
int todhip_set_l2_cross_check(todhip_ctx*, uint32_t frame_queries /* 0 = off, the default */);

/* ---- stage C: GuessGenerator ------------------------------------------------------------------- */
void todhip_rng_seed(todhip_rng*, uint32_t seed);   /* srand(seed); the reference never seeds => seed 1 */
/* Replaces GuessGenerator::process (GuessGenerator.cpp:127-250) and everything under src/common.
 * kp_xy: nq x 2 keypoint pixels (cv::KeyPoint::pt); cloud_xyz: H x W x 3 f32 organised cloud (NaN = no depth);
 * matches in CSR form as produced by todhip_match; spans: per object index (imgIdx).
 * poses: capacity *n_poses in, count out. inlier_kp: capacity *n_inlier_kp in, count out.
 * Range of the pose solve: R comes from a float 3x3 SVD of the inliers' correlation matrix H = sum (train - c_train)(query - c_query)^T.
 * Supported: every H whose entries, rounded to float, are finite -- any rank (planar and collinear inliers included), any ratio of
 * its singular values. R is then a rotation to 8 * 2^-23 and lies within 16 kappa 2^-23 of the float64 Kabsch solution,
 * kappa = s1 / (s2 +- s3). Data in metres gives entries of about 1e-6 .. 1e3. Between 2^-32 and 2^40 the SVD works on H as it is;
 * the one place where that alone would leave the float range (the product of two squared column norms, from s1 s2 = 1.8e19 on) takes
 * its root factor by factor. An H whose largest entry lies outside is first scaled by a power of two, because the squares of its
 * entries would overflow (beyond 1.8e19) or, for the rounding residue that stands in for a zero singular value, go denormal (a
 * largest entry below 1e-12). tests/test_verify_pose_gpu.py pins this through todhip_test_kabsch at the scales 1e-30, 1e-12,
 * 1e-8 .. 1e12, 1e30, a largest entry of 0.9 FLT_MAX, and on both sides of s1 s2 = 1.8e19. An H with an infinite or NaN entry
 * gives NaN. */
int todhip_verify(todhip_ctx*, const float* kp_xy, uint32_t nq, const float* cloud_xyz, uint32_t H, uint32_t W,
                  const uint32_t* row_ptr, const todhip_dmatch* matches, const float* matches_xyz,
                  const float* spans, uint32_t n_objs, const todhip_verify_params*, todhip_rng* rng,
                  todhip_pose* poses, uint32_t* n_poses, uint32_t* inlier_kp, uint32_t* n_inlier_kp);

/* Device-resident form: d_kp_xy[nq*2] f32, d_cloud_xyz[H*W*3] f32 and the matcher's fixed-stride outputs
 * (d_counts[nq] u32, d_matches[nq*k], d_matches_xyz[nq*k*3], exactly what todhip_match_device produced) are in
 * HBM already; ClusterPerObject (adjacency_ransac.cpp:176-205) runs as kernels. Poses come back to the host. */
int todhip_verify_device(todhip_ctx*, const void* d_kp_xy, uint32_t nq, const void* d_cloud_xyz, uint32_t H, uint32_t W,
                         const void* d_counts, const void* d_matches, const void* d_matches_xyz, uint32_t k,
                         const float* spans, uint32_t n_objs, const todhip_verify_params*, todhip_rng* rng,
                         todhip_pose* poses, uint32_t* n_poses, uint32_t* inlier_kp, uint32_t* n_inlier_kp);

/* Same, but the query points are back-projected from the registered depth image instead of being read from a
 * materialised H x W x 3 cloud (replaces RescaledRegisteredDepth -> DepthTo3d ->
 * GuessGenerator's cloud lookup, detector.py:26,62,66-69 + adjacency_ransac.cpp:184-185). d_depth: H x W, float
 * metres (NaN = no depth) or, with depth_is_u16, uint16 millimetres (0 = no depth). K9: row-major 3x3 intrinsics. */
int todhip_verify_device_depth(todhip_ctx*, const void* d_kp_xy, uint32_t nq, const void* d_depth, int depth_is_u16,
                               uint32_t H, uint32_t W, const float* K9, const void* d_counts, const void* d_matches,
                               const void* d_matches_xyz, uint32_t k, const float* spans, uint32_t n_objs,
                               const todhip_verify_params*, todhip_rng* rng, todhip_pose* poses, uint32_t* n_poses,
                               uint32_t* inlier_kp, uint32_t* n_inlier_kp);

/* A batch of n_frames frames through GuessGenerator::process in the launches and host round trips of one frame.
 * Inputs are the per-frame arrays of todhip_verify_device[_depth] back to back (frame f at f times the per-frame size:
 * d_kp_xy[n_frames*nq*2], cloud [n_frames*H*W*3] or depth [n_frames*H*W], d_counts[n_frames*nq], d_matches[n_frames*nq*k],
 * d_matches_xyz[n_frames*nq*k*3] -- what todhip_match_device yields for n_frames*nq queries); a frame with fewer
 * than nq keypoints pads with counts 0. rng[n_frames]: one generator per frame (decision D4), each advanced as
 * the single-frame call would. Poses of frame f: poses[pose_ptr[f] .. pose_ptr[f+1]) (pose_ptr[n_frames+1]);
 * inlier_begin/end index the shared inlier_kp array. Each frame's result equals the single-frame call's.
 * Frames of a batch that are out of step have their heavy phases (clique gate, growth of objects with >= 96 matches) launched on
 * up to two process-wide side streams (TODHIP_VERIFY_FLIGHTS, 0 = none); the call returns when everything has finished. */
int todhip_verify_batch_device(todhip_ctx*, uint32_t n_frames, const void* d_kp_xy, uint32_t nq, const void* d_cloud_xyz,
                               uint32_t H, uint32_t W, const void* d_counts, const void* d_matches, const void* d_matches_xyz,
                               uint32_t k, const float* spans, uint32_t n_objs, const todhip_verify_params*, todhip_rng* rng,
                               todhip_pose* poses, uint32_t* n_poses, uint32_t* pose_ptr, uint32_t* inlier_kp,
                               uint32_t* n_inlier_kp);
int todhip_verify_batch_device_depth(todhip_ctx*, uint32_t n_frames, const void* d_kp_xy, uint32_t nq, const void* d_depth,
                                     int depth_is_u16, uint32_t H, uint32_t W, const float* K9, const void* d_counts,
                                     const void* d_matches, const void* d_matches_xyz, uint32_t k, const float* spans,
                                     uint32_t n_objs, const todhip_verify_params*, todhip_rng* rng, todhip_pose* poses,
                                     uint32_t* n_poses, uint32_t* pose_ptr, uint32_t* inlier_kp, uint32_t* n_inlier_kp);

/* The depth image at the sensor's own size, dH x dW, in front of todhip_verify[_batch]_device_depth (RescaledRegisteredDepth in front
 * of DepthTo3d, detector.py:26,66-67; the arithmetic of Trainer.cpp:62-81). Definition: the result -- poses, their order, R and t bit
 * for bit, inlier lists, the generator's final state -- is that of todhip_rescale_depth_device(d_depth, depth_is_u16, dH, dW -> H, W,
 * nearest) on each frame followed by todhip_verify[_batch]_device_depth on the float result with depth_is_u16 = 0. No H x W image is
 * made: the rescaled pixel is computed from its taps at each keypoint's pixel, inside the kernel that looks the keypoints' 3D points
 * up. H, W and K9 are the IMAGE's (keypoints are image pixels). A keypoint in the NaN band below the resized rows, or on a NaN / 0 tap,
 * has no 3D point, exactly as after a rescale. The batch form reads frame f's depth at f * dH * dW values. A geometry that
 * todhip_rescale_depth refuses (the resized rows would not fit into H): TODHIP_EINVAL before any device work. dH == H and dW == W:
 * todhip_verify[_batch]_device_depth. */
int todhip_verify_device_depth_rescaled(todhip_ctx*, const void* d_kp_xy, uint32_t nq, const void* d_depth, int depth_is_u16,
                                        uint32_t dH, uint32_t dW, int nearest, uint32_t H, uint32_t W, const float* K9,
                                        const void* d_counts, const void* d_matches, const void* d_matches_xyz, uint32_t k,
                                        const float* spans, uint32_t n_objs, const todhip_verify_params*, todhip_rng* rng,
                                        todhip_pose* poses, uint32_t* n_poses, uint32_t* inlier_kp, uint32_t* n_inlier_kp);
int todhip_verify_batch_device_depth_rescaled(todhip_ctx*, uint32_t n_frames, const void* d_kp_xy, uint32_t nq, const void* d_depth,
                                              int depth_is_u16, uint32_t dH, uint32_t dW, int nearest, uint32_t H, uint32_t W,
                                              const float* K9, const void* d_counts, const void* d_matches, const void* d_matches_xyz,
                                              uint32_t k, const float* spans, uint32_t n_objs, const todhip_verify_params*,
                                              todhip_rng* rng, todhip_pose* poses, uint32_t* n_poses, uint32_t* pose_ptr,
                                              uint32_t* inlier_kp, uint32_t* n_inlier_kp);

/* ---- stage A: ORB features (ecto_opencv FeatureDescriptor -> cv::ORB; detector.py:10,27) --------- */
/* gray: H x W u8, row stride `stride` >= W: (H - 1) * stride + W bytes, nothing behind the last row's pixels is read (a region of
 * a larger image). A pyramid level that rounds to fewer than 63 pixels either way yields nothing; an image without any other level
 * returns 0 keypoints. Outputs up to n_features keypoints: kp_xy (x,y level-0 pixels),
 * kp_aux (size, angle_deg, response, octave) and 32-byte rBRIEF descriptors. *n_out: capacity in, count out.
 * pattern: 256 x 4 int8 (x0,y0,x1,y1) test pairs, or NULL for the built-in seeded pattern. Domain: every point (x0,y0) and (x1,y1)
 * has x^2 + y^2 <= 900. A keypoint lies at least 31 pixels inside its level and a steered point keeps its distance from the centre, so
 * this is the largest disc whose rotated, rounded points all read pixels of the keypoint's own level; it contains the 31 x 31 patch
 * (|x|, |y| <= 15) of cv::ORB patterns and the learner's candidates (x^2 + y^2 <= 169). A pattern with a point outside it:
 * TODHIP_EINVAL before any device work, from every form that takes a `pattern` -- the todhip_orb* forms below,
 * todhip_model_add_observation[s_device] and todhip_pipeline_set_pattern (at that call, the pipeline's pattern stays as it was). */
int todhip_orb(todhip_ctx*, const uint8_t* gray, uint32_t H, uint32_t W, uint32_t stride, uint32_t n_features,
               uint32_t n_levels, float scale_factor, const int8_t* pattern, float* kp_xy, float* kp_aux,
               uint8_t* desc, uint32_t* n_out);

/* The same with the cell's `mask` input (detector.py:41 forwards it to FeatureDescriptor; cv::ORB's second argument): only
 * pixels with mask != 0 (H x W u8, row stride `stride`, level 0) can become keypoints. mask == NULL: todhip_orb. */
int todhip_orb_masked(todhip_ctx*, const uint8_t* gray, const uint8_t* mask, uint32_t H, uint32_t W, uint32_t stride,
                      uint32_t n_features, uint32_t n_levels, float scale_factor, const int8_t* pattern, float* kp_xy,
                      float* kp_aux, uint8_t* desc, uint32_t* n_out);

/* Device-resident form: d_gray (H x W u8, row stride `stride`) is in HBM, keypoints and descriptors stay in HBM
 * (d_kp_xy[cap*2] f32, d_kp_aux[cap*4] f32, d_desc[cap*32] u8); only the count comes back. *n_out: capacity in. */
int todhip_orb_device(todhip_ctx*, const void* d_gray, uint32_t H, uint32_t W, uint32_t stride, uint32_t n_features,
                      uint32_t n_levels, float scale_factor, const int8_t* pattern, void* d_kp_xy, void* d_kp_aux,
                      void* d_desc, uint32_t* n_out);

/* A batch of n_frames device-resident frames (frame f at d_gray + f * frame_stride bytes) in the launches of one:
 * frame f's keypoints land at row f * cap of d_kp_xy[n_frames*cap*2], d_kp_aux[n_frames*cap*4], d_desc[n_frames*cap*32];
 * n_out[n_frames] comes back. Each frame's result equals todhip_orb_device's on that frame. */
int todhip_orb_batch_device(todhip_ctx*, const void* d_gray, uint32_t n_frames, uint64_t frame_stride, uint32_t H, uint32_t W,
                            uint32_t stride, uint32_t n_features, uint32_t n_levels, float scale_factor, const int8_t* pattern,
                            void* d_kp_xy, void* d_kp_aux, void* d_desc, uint32_t cap, uint32_t* n_out);

/* The batch with a mask per frame (todhip_orb_masked's `mask`, in HBM): d_mask is n_frames x H x W u8, packed (frame f's mask at
 * d_mask + f * H * W, row pitch W, whatever stride and frame_stride are). Frame f's result equals todhip_orb_masked's on frame f with
 * mask f. d_mask == NULL: todhip_orb_batch_device. */
int todhip_orb_batch_device_masked(todhip_ctx*, const void* d_gray, const void* d_mask, uint32_t n_frames, uint64_t frame_stride,
                                   uint32_t H, uint32_t W, uint32_t stride, uint32_t n_features, uint32_t n_levels, float scale_factor,
                                   const int8_t* pattern, void* d_kp_xy, void* d_kp_aux, void* d_desc, uint32_t cap, uint32_t* n_out);

/* ---- stage C without depth (SURVEY 8(f) row N4 b) -------------------------------------------------------- */
/* The branch GuessGenerator::process leaves empty when `points3d` is empty (GuessGenerator.cpp:147-152 "Only use 2d to 3d
 * matching // TODO"; doc/source/index.rst:36-46: a PnP problem the reference never plugged in). NOT a reference result:
 * defined here, checked bit for bit by the tests' CPU definition (oracle/pnp_oracle.c), parity unpinned by construction.
 *   inputs   kp_xy nq x 2 keypoint pixels; K9 the camera matrix, row-major; matches in CSR form as produced by todhip_match
 *            (matches_xyz = the model point of each match); spans per object index. prm->sensor_error is the reprojection
 *            threshold in PIXELS here, prm->n_ransac_iterations the (fixed) number of hypotheses per object.
 *   per object (ascending index, matches clustered in CSR order, at least max(3, min_inliers) of them):
 *     hypothesis h = 0 .. n - 1: a sample of three matches, pairwise with keypoints > 20 px apart and distinct model points
 *       within the object's span, picked by a counter-based hash of (seed, object, h, attempt <= 16); Grunert's P3P in f64 on
 *       it (up to 4 poses); consensus set of a pose = matches whose model point reprojects within the threshold, in front of
 *       the camera. The largest consensus set wins, the first (h, root) on ties; it must reach min_inliers.
 *     the winner is refined by 5 Gauss-Newton steps on its consensus set and the consensus set recomputed; the pose is
 *       reported if that still reaches min_inliers. ONE pose per object, by design: the 3D branch finds further instances by
 *       taking a pose's inlier keypoints out and trying the object again (GuessGenerator.cpp:192-231), guarded by its clique
 *       gate; reprojection alone is too weak a constraint for that -- at the reference's min_inliers of 8 a second round
 *       assembles chance poses from the leftovers of repeating texture (measured: 7 poses instead of 1 on the rendered-view
 *       test). A caller that expects several instances of an object supplies depth.
 *   rng: ONE draw per call supplies the seed (hypotheses do not walk the stream, which is what lets them run side by side).
 *   outputs as todhip_verify: poses (object -> camera), inlier_kp = keypoint indices of each pose's consensus set, ascending. */
int todhip_verify_2d(todhip_ctx*, const float* kp_xy, uint32_t nq, const float* K9, const uint32_t* row_ptr,
                     const todhip_dmatch* matches, const float* matches_xyz, const float* spans, uint32_t n_objs,
                     const todhip_verify_params*, todhip_rng* rng, todhip_pose* poses, uint32_t* n_poses, uint32_t* inlier_kp,
                     uint32_t* n_inlier_kp);

/* The same with the keypoints and the matcher's fixed-stride outputs in HBM (what todhip_match_device / todhip_merge_shards_device
 * left there): d_kp_xy[nq*2] f32, d_counts[nq] u32, d_matches[nq*k], d_matches_xyz[nq*k*3]. Same result as the call above. The
 * matches never come to the host: ClusterPerObject runs on the device, the host reads the number of objects worth a RANSAC
 * (one word) and, at the end, the poses and their consensus flags. */
int todhip_verify_2d_device(todhip_ctx*, const void* d_kp_xy, uint32_t nq, const float* K9, const void* d_counts, const void* d_matches,
                            const void* d_matches_xyz, uint32_t k, const float* spans, uint32_t n_objs, const todhip_verify_params*,
                            todhip_rng* rng, todhip_pose* poses, uint32_t* n_poses, uint32_t* inlier_kp, uint32_t* n_inlier_kp);

/* A batch of n_frames frames in the launches of one (the layout of todhip_verify_batch_device: per-frame arrays back to back,
 * rng[n_frames], poses of frame f at poses[pose_ptr[f] .. pose_ptr[f+1]), inlier_kp frame-local). Each frame's result equals the
 * single-frame call's. */
int todhip_verify_2d_batch_device(todhip_ctx*, uint32_t n_frames, const void* d_kp_xy, uint32_t nq, const float* K9, const void* d_counts,
                                  const void* d_matches, const void* d_matches_xyz, uint32_t k, const float* spans, uint32_t n_objs,
                                  const todhip_verify_params*, todhip_rng* rng, todhip_pose* poses, uint32_t* n_poses,
                                  uint32_t* pose_ptr, uint32_t* inlier_kp, uint32_t* n_inlier_kp);

/* ---- the detection pipeline: stages A -> B -> C on batches of frames, overlapped ------------------------------ */
/* One object that owns what a host otherwise has to assemble around the three batched stage calls: a matcher context on a
 * TODHIP_STREAM_THROUGHPUT stream, orb_workers ORB contexts and verify_workers verifier contexts on TODHIP_STREAM_LATENCY streams
 * (created as todhip_stream_create creates them, so todhip_set_cu_partition, called before, keeps its meaning), one host thread per
 * context, and a ring of ring_depth sets of device buffers. A step of up to frames_per_step frames is submitted, gets a ticket, and
 * runs todhip_orb_batch_device -> todhip_match_device (one DB pass for the step) -> todhip_verify_batch_device_depth; step i uses ORB
 * worker i % orb_workers and verifier worker i % verify_workers, the matcher issues the steps in ticket order, and the verifier's
 * stream waits for an event recorded behind the matcher's work of the step. So the matcher of one step runs beside ORB of later steps
 * and the verifier of earlier ones (tod_amd/pipeline.py and bench.py's data-chained run have the same structure in Python).
 * Result: frame f of a step yields exactly what the single-frame device chain yields on that frame alone against the same DB --
 * todhip_orb_device (capacity n_features) -> todhip_match_device on its n_kp descriptors -> todhip_verify_device_depth with a
 * generator seeded rng_seed: keypoints, poses and their order, R and t bit for bit, inlier lists. A frame with fewer than n_features
 * keypoints is padded with match counts 0 on the device.
 * The detector's two further inputs (detector.py:26,41,66-67) extend that chain and leave it as it is when unused: with masks
 * (todhip_pipeline_submit_masked[_device]) its first link is masked ORB -- todhip_orb_masked's result on frame f with mask f, in the
 * device form -- and with a depth size of its own (todhip_pipeline_set_depth_size) todhip_rescale_depth_device stands between the
 * matcher and todhip_verify_device_depth: masked ORB -> todhip_match_device -> todhip_rescale_depth_device -> todhip_verify_device_depth.
 * Inside, the steps run todhip_orb_batch_device_masked and todhip_verify_batch_device_depth_rescaled.
 * Threading: submit, wait and get_stats may be called from any threads, also concurrently; each ticket is waited for once.
 * The pipeline uses 1 + orb_workers + verify_workers streams plus the verifier's two process-wide side streams; see INTEGRATION.md
 * for the number of hardware queues a host should allow before HIP initialises. */
typedef struct todhip_pipeline todhip_pipeline;
enum { TODHIP_FRAME_GRAY8 = 0, TODHIP_FRAME_BGR8 = 1, TODHIP_FRAME_BGRA8 = 2 };
typedef struct {
  uint32_t struct_size;                /* sizeof(todhip_pipeline_params), as todhip_pipeline_default_params sets it */
  uint32_t frames_per_step;            /* B: 1..64 frames per submit */
  uint32_t H, W;                       /* every frame; the depth image has the same size unless todhip_pipeline_set_depth_size says otherwise */
  int      frame_format;               /* TODHIP_FRAME_* */
  int      depth_is_u16;               /* uint16 mm (0 = none) or float m (NaN = none) */
  float    K9[9];                      /* camera matrix, row-major */
  uint32_t n_features, n_levels; float scale_factor;   /* ORB; n_features is also the per-frame query capacity */
  uint32_t k, radius;                  /* matcher: 1..8, > 0 */
  todhip_verify_params verify;
  uint32_t rng_seed;                   /* every frame's generator starts from this srand seed (decision D4); 0 -> 1 */
  uint32_t orb_workers, verify_workers, ring_depth;    /* 0 -> 1, 2, verify_workers + 2; ring_depth > verify_workers; workers <= 8, ring <= 16 */
  uint32_t max_poses_per_frame;        /* 0 -> 64 */
} todhip_pipeline_params;
/* Cumulative since creation. The *_s fields are host seconds inside the stage calls, summed over the workers of a stage (orb_s
 * includes the uploads and the colour conversion, match_issue_s only issues work, verify_s starts once the matcher's event has
 * fired); the matcher-kernel fields are the matcher context's counters and stay 0 unless
 * todhip_set_kernel_timing(todhip_pipeline_matcher(p), 1) was called. Steps that ended in an error are not counted. */
typedef struct {
  uint64_t steps, frames, keypoints, poses;
  double   orb_s, match_issue_s, verify_s;
  double   sum_match_kernel_ms;
  uint64_t n_match_kernel_launches;
} todhip_pipeline_stats;

/* Zeroes *out, sets struct_size and the defaults: 32 frames of 480 x 640 GRAY8, float depth, 1000 features / 3 levels / 1.2,
 * k 5, radius 55, verify 15 / 1000 / 0.01, seed 1, workers 1 + 2, ring 4, 64 poses per frame. K9 is the caller's to fill. */
int  todhip_pipeline_default_params(todhip_pipeline_params* out);
/* Parameters are checked before any device work (TODHIP_EINVAL); without a usable device TODHIP_EHIP. Allocates every buffer of the
 * device form; the host form's pinned staging and upload buffers are allocated by a slot's first todhip_pipeline_submit. */
int  todhip_pipeline_create(int device, const todhip_pipeline_params*, todhip_pipeline** out);
void todhip_pipeline_destroy(todhip_pipeline*);          /* drains what is in flight, joins its threads */
/* The matcher context, for todhip_set_ratio_test / _set_ratio_test_other / _set_lsh / _set_matcher_engine / _set_kernel_timing /
 * _set_db_bit_order: only while no ticket is outstanding. todhip_set_ratio_test_other reaches every step's todhip_match_device this
 * way, with no setter of the pipeline's own; the rows behind a frame's n_kp are padded away behind the filter as behind the search. It is the pipeline's: do not call the match functions on it and do not destroy it.
 * todhip_set_db_bit_order(todhip_pipeline_matcher(p), 1) before todhip_pipeline_db_load[_device] orders the pipeline's DB. */
todhip_ctx* todhip_pipeline_matcher(todhip_pipeline*);
/* todhip_db_load[_device] into the matcher context (one device, desc_bytes == 32); the spans are kept for the verifier workers.
 * TODHIP_EBUSY while a ticket is outstanding. */
int  todhip_pipeline_db_load(todhip_pipeline*, const todhip_object*, uint32_t n_objs, uint32_t desc_bytes);
int  todhip_pipeline_db_load_device(todhip_pipeline*, const todhip_object*, uint32_t n_objs, uint32_t desc_bytes);
/* n_frames in 1..frames_per_step, frames and depth images densely packed back to back without row padding: a frame is H*W bytes
 * (GRAY8), H*W*3 (BGR8) or H*W*4 (BGRA8), a depth image H*W uint16 or float values (dH*dW after todhip_pipeline_set_depth_size). Tickets count up from 1. Never blocks on the
 * GPU: with ring_depth tickets submitted and not yet waited for it returns TODHIP_EBUSY (wait for one, then submit again).
 * Host form: copies into pinned staging owned by the ring slot and returns; the caller may reuse its buffers at once.
 * Device form: no copy -- the stages READ THE CALLER'S DEVICE BUFFERS UNTIL THAT TICKET'S todhip_pipeline_wait HAS RETURNED the
 * results (or an error other than TODHIP_ETIMEOUT / TODHIP_ECAPACITY); they must be complete when submit is called. */
int  todhip_pipeline_submit(todhip_pipeline*, const uint8_t* frames, const void* depth, uint32_t n_frames, uint64_t* ticket);
int  todhip_pipeline_submit_device(todhip_pipeline*, const void* d_frames, const void* d_depth, uint32_t n_frames, uint64_t* ticket);
/* Results of one ticket, in any order of tickets, each ticket once (a second wait, or an unknown ticket: TODHIP_EINVAL).
 * timeout_ms == 0 waits without limit; otherwise TODHIP_ETIMEOUT leaves the ticket waitable. n_kp[n_frames]; kp_xy (may be NULL)
 * [n_frames * n_features * 2], frame f's keypoints at row f * n_features, rows behind n_kp[f] zero; poses of frame f are
 * poses[pose_ptr[f] .. pose_ptr[f+1]), inlier_begin/end index inlier_kp, whose entries are frame-local keypoint indices (as
 * todhip_verify_batch_device). *n_poses / *n_inlier_kp: capacity in, count out; when one is too small: TODHIP_ECAPACITY with the
 * needed counts written, and the ticket stays waitable. A stage's error (TODHIP_ENODB when no DB was loaded ...) is returned here and
 * ends the ticket. After TODHIP_EHIP the pipeline issues no further GPU work: every later submit and wait returns TODHIP_EHIP. */
int  todhip_pipeline_wait(todhip_pipeline*, uint64_t ticket, uint32_t timeout_ms,
                          uint32_t* n_kp /*[n_frames]*/, float* kp_xy /*[n_frames*n_features*2], may be NULL*/,
                          todhip_pose* poses, uint32_t* n_poses /*cap in, count out*/, uint32_t* pose_ptr /*[n_frames+1]*/,
                          uint32_t* inlier_kp, uint32_t* n_inlier_kp /*cap in, count out*/);
int  todhip_pipeline_get_stats(todhip_pipeline*, todhip_pipeline_stats* out);
/* The ORB pattern of the pipeline's ORB workers (256 x 4 int8, copied; NULL = the built-in one), from the next submit on: how a
 * pattern learned by todhip_pattern_learn_* reaches the batched path. The DB must hold descriptors of the same pattern.
 * TODHIP_EBUSY while a ticket is outstanding. A pattern outside the domain stated at todhip_orb (a point with x^2 + y^2 > 900):
 * TODHIP_EINVAL here, not at the next submit, and the workers' pattern stays what it was. */
int  todhip_pipeline_set_pattern(todhip_pipeline*, const int8_t* pattern /* 256 x 4; NULL = built-in */);
/* The size of a depth image, from the next submit on: dH x dW values (uint16 or float as depth_is_u16 says), rescaled to the image
 * as todhip_rescale_depth does (nearest != 0: its nearest mode) -- see the definition above and todhip_verify_device_depth_rescaled.
 * (0, 0): the image's size again. The host form's staging and upload buffers follow. TODHIP_EINVAL where todhip_rescale_depth refuses
 * the geometry (nothing changes), TODHIP_EBUSY while a ticket is outstanding. */
int  todhip_pipeline_set_depth_size(todhip_pipeline*, uint32_t dH, uint32_t dW, int nearest);
/* todhip_pipeline_submit[_device] with a mask per frame: masks is n_frames x H x W u8, packed, one channel whatever frame_format is;
 * only pixels with mask != 0 can become keypoints (todhip_orb_masked). masks == NULL: todhip_pipeline_submit[_device]. Host form: the
 * masks are copied into pinned staging of the slot and go up on the ORB worker's stream, as the frames do. Device form: d_masks is
 * read under the frames' lifetime rule. A step's masks apply to that step only. */
int  todhip_pipeline_submit_masked(todhip_pipeline*, const uint8_t* frames, const uint8_t* masks, const void* depth, uint32_t n_frames,
                                   uint64_t* ticket);
int  todhip_pipeline_submit_masked_device(todhip_pipeline*, const void* d_frames, const void* d_masks, const void* d_depth,
                                          uint32_t n_frames, uint64_t* ticket);
/* todhip_db_select_objects on the pipeline's matcher context, from the next submit on; the verifier workers keep the spans of every
 * object (poses name objects of the full DB). TODHIP_EBUSY while a ticket is outstanding. */
int  todhip_pipeline_select_objects(todhip_pipeline*, const uint32_t* ids, uint32_t n_ids);
/* The cross-check (todhip_cross_check_device) behind each step's matcher call, from the next submit on: on the matcher's stream, in
 * front of the event the verifier waits on, with frame_queries = n_features and frame_nq = the step's n_kp -- the rows behind n_kp[f]
 * hold an earlier step's descriptors and do not compete. Frame f of a step then yields what the chain todhip_orb_device ->
 * todhip_match_device -> todhip_cross_check_device(frame_nq = {n_kp}) -> todhip_verify_device_depth yields on that frame alone.
 * enable 0 (the default): the steps are those of a pipeline that never called this. TODHIP_EBUSY while a ticket is outstanding. */
int  todhip_pipeline_set_cross_check(todhip_pipeline*, int enable);
/* One device-resident BGR8 / BGRA8 image (channels 3 | 4, row stride src_stride bytes) -> gray (row stride gray_stride bytes), the
 * conversion the pipeline runs in front of ORB: Y = (1868 B + 9617 G + 4899 R + 8192) >> 14, what adapter/ecto_cells.hpp computes on
 * the host. Asynchronous on the context's stream. */
int  todhip_bgr_to_gray_device(todhip_ctx*, const void* d_src, uint32_t channels /*3|4*/, uint32_t H, uint32_t W,
                               uint32_t src_stride, void* d_gray, uint32_t gray_stride);

/* ---- training ----------------------------------------------------------------- */
/* Per-observation arithmetic of the reference's Trainer cell (src/training/Trainer.cpp:121-187, training.cpp:57-195):
 * ORB on the masked view (the reference uses cv::ORB defaults: 500 features, 8 levels, scale 1.2 -- :148-149),
 * validateKeyPoints (mask eroded 4x, +-2 pixel rescue, depth validity), depthTo3dSparse, cameraToWorld, mergePoints.
 * A model is accumulated on the device; its rows are what todhip_db_load ingests (ModelFiller.cpp:23-24). */
typedef struct todhip_model todhip_model;
int  todhip_model_begin(todhip_ctx*, uint32_t capacity_rows, todhip_model** out);
/* gray/mask: H x W u8 (mask != 0 = object); depth: H x W float metres (NaN = none) or uint16 millimetres (0 = none),
 * of the image size (other sizes: todhip_rescale_depth first, as Trainer.cpp:142-143 does); K9, R9 row-major; T3.
 * pattern: as at todhip_orb, its domain included (outside it: TODHIP_EINVAL, the model unchanged; the batch form below likewise). */
int  todhip_model_add_observation(todhip_ctx*, todhip_model*, const uint8_t* gray, const uint8_t* mask, const void* depth,
                                  int depth_is_u16, uint32_t H, uint32_t W, const float* K9, const float* R9, const float* T3,
                                  uint32_t n_features, uint32_t n_levels, float scale_factor, const int8_t* pattern,
                                  uint32_t* n_added);
/* rescale_depth (Trainer.cpp:62-81; on the detection side ecto_opencv's RescaledRegisteredDepth cell, detector.py:26,62):
 * depth_in dH x dW, float metres or uint16 millimetres -> depth_out H x W float metres (NaN = none). Equal sizes: the
 * unit conversion only (:68-71). Otherwise a resize into the top int(dH * (W / dW)) rows, NaN below (:73-80):
 * nearest == 0 is what the reference executes -- its cv::resize call passes CV_INTER_NN in the `fx` position (:78), so
 * cv::resize's default bilinear interpolation runs; nearest != 0 is the nearest-neighbour resize its comment intends.
 * TODHIP_EINVAL where the reference's rowRange/resize would throw (that row count is 0 or exceeds H). The output feeds
 * todhip_model_add_observation / todhip_verify_device_depth (depth_is_u16 = 0). */
int  todhip_rescale_depth(todhip_ctx*, const void* depth_in, int depth_is_u16, uint32_t dH, uint32_t dW, float* depth_out,
                          uint32_t H, uint32_t W, int nearest);
int  todhip_rescale_depth_device(todhip_ctx*, const void* d_depth_in, int depth_is_u16, uint32_t dH, uint32_t dW,
                                 void* d_depth_out, uint32_t H, uint32_t W, int nearest);
/* A batch of device-resident views in one call: what a host that renders or captures an object's views on the device (tens to
 * hundreds per object, Trainer.cpp:121-187 loops over them) does instead of n_views host-buffer calls. View v's gray image is at
 * d_gray + v * frame_stride with row pitch stride >= W; its mask at d_mask + v * H * W (packed, != 0 = object); its depth image at
 * d_depth + v * dH * dW elements (packed; float metres or uint16 millimetres), at the sensor's own size dH x dW, or of the image's
 * size when dH == dW == 0. K9, R9 and T3 are HOST arrays of n_views x 9, n_views x 9 and n_views x 3 floats.
 * Definition: the model afterwards is byte for byte the model after this sequence, for v = 0 .. n_views - 1 in order:
 *   - if the depth size differs from the image's: todhip_rescale_depth(view v's depth, depth_is_u16, dH, dW -> H, W, nearest);
 *   - then todhip_model_add_observation(view v's packed gray, mask v, that depth, ..., K9 + 9 v, R9 + 9 v, T3 + 3 v, n_features,
 *     n_levels, scale_factor, pattern, &n_added[v]); the depth is float after a rescale, otherwise it is used as it is.
 * The bytes are the descriptors, the points, the row count, and n_added[v] per view (n_added may be NULL). That includes the capacity
 * cut (the view that reaches capacity_rows stores its first rows that still fit, every later view adds 0), views that yield no
 * keypoint (they add 0), and rows the model already held -- from todhip_model_add_observation, _add_rows, _compact or an earlier batch.
 * (Points: equal bytes where they are not NaN, NaN in the same places.) Neither an eroded mask nor a rescaled depth image is made:
 * the arithmetic of both is evaluated at the keypoints (tod_amd/csrc/train_validate.h, depth_rescale.h).
 * TODHIP_EINVAL, checked before any device work, the model untouched: whatever todhip_model_add_observation refuses (a null pointer,
 * H or W below 8, n_features == 0, n_levels == 0 or above 16, scale_factor <= 1); d_mask == NULL; n_views == 0 or > 64 (the caller
 * loops over larger sets); stride < W; n_views > 1 with frame_stride < H * stride; exactly one of dH, dW zero; a depth geometry
 * todhip_rescale_depth refuses. Synchronizes the context's stream once, at its end, as todhip_model_add_observation does: the
 * caller's buffers may be reused on return. All views of a batch share the image size and the ORB settings. */
int  todhip_model_add_observations_device(todhip_ctx*, todhip_model*,
                                          const void* d_gray, uint64_t frame_stride, uint32_t stride,
                                          const void* d_mask,
                                          const void* d_depth, int depth_is_u16, uint32_t dH, uint32_t dW, int nearest,
                                          uint32_t n_views, uint32_t H, uint32_t W,
                                          const float* K9, const float* R9, const float* T3,
                                          uint32_t n_features, uint32_t n_levels, float scale_factor, const int8_t* pattern,
                                          uint32_t* n_added);
/* *n: capacity in rows in, rows out. desc: rows x 32, pts_xyz: rows x 3 (object/world frame). */
int  todhip_model_finish(todhip_ctx*, todhip_model*, uint8_t* desc, float* pts_xyz, uint32_t* n);
/* The model where it is: device pointers of its descriptors (n x 32 u8) and points (n x 3 f32), valid until todhip_model_free.
 * With todhip_db_load_device a freshly trained model reaches the matcher without visiting the host (the reference writes it to
 * CouchDB, ModelFiller.cpp:23-24, and DescriptorMatcher::parameter_callback reads it back, DescriptorMatcher.cpp:60-129). */
int  todhip_model_device(todhip_ctx*, todhip_model*, const void** d_desc, const void** d_pts_xyz, uint32_t* n);
/* Append n already-trained rows (host memory; desc n x 32, pts_xyz n x 3) behind the model's rows, as many as still fit below its
 * capacity: *n_added (may be NULL). How a stored model (ModelFiller.cpp:23-24) is taken up again before further observations, and how
 * rows of any origin reach todhip_model_compact. n == 0 is allowed (the pointers may then be NULL). Synchronizes the context's stream. */
int  todhip_model_add_rows(todhip_ctx*, todhip_model*, const uint8_t* desc, const float* pts_xyz, uint32_t n, uint32_t* n_added);
/* Merge near-duplicate rows of the model in place. A model is the concatenation of its views' rows (mergePoints, training.cpp:147-173),
 * so a surface point seen in v views is v rows; this keeps one of them. Off unless called, and without a counterpart in the reference.
 * Definition (exact, deterministic), rows in model order 0 .. n-1:
 *   ham(i, j) = popcount of the xor of the two 32-byte descriptors.
 *   d2(i, j)  = (dx*dx + dy*dy) + dz*dz with dx = x_i - x_j (dy, dz alike), every operation in IEEE binary32, rounded once, no fused
 *               multiply-add: exactly symmetric in i and j. r2 = merge_dist * merge_dist in binary32.
 *   conflict(i, j) <=> ham(i, j) <= max_hamming and d2(i, j) <= r2, both bounds inclusive. A NaN in either point makes the float
 *               comparison false: such a row conflicts with nothing and is always kept.
 *   Row i is kept iff no KEPT row j < i has conflict(i, j) (greedy in row order, not transitive: if A conflicts with B, B with C and A
 *               not with C, then A and C are kept and B goes).
 *   The kept rows move stably to the front: descriptors and points unchanged, relative order unchanged; the model's row count
 *               becomes their number.
 *   support[r] (optional) of the r-th kept row = 1 + the dropped rows whose lowest-index conflicting kept row it is; their sum is
 *               *rows_before.
 * merge_dist == 0 merges only rows with d2 == 0: equal points (+0 == -0), or differences whose squares all underflow to 0 (below
 * 2^-75; subnormal results are kept, not flushed). max_hamming == 256 ignores the descriptors. An empty model is TODHIP_OK with 0 -> 0. Compacting again with the same arguments changes nothing (no two kept rows conflict).
 * TODHIP_EINVAL, the model untouched: merge_dist negative or not finite, max_hamming > 256, a null context or model, support without
 * n_support, or a model of more than 2^18 rows (the pair test is quadratic in the rows; device scratch is linear in them).
 * support: capacity *n_support in, *n_support = *rows_after out (n_support alone, support == NULL, just receives the count); when the
 * capacity is too small: TODHIP_ECAPACITY with *n_support = *rows_after, the model already compacted. rows_before / rows_after may be
 * NULL. Synchronizes the context's stream, as todhip_model_device does; todhip_model_add_observation, _add_rows, _device and _finish
 * then work on the compacted model. */
int  todhip_model_compact(todhip_ctx*, todhip_model*, float merge_dist, uint32_t max_hamming, uint32_t* rows_before,
                          uint32_t* rows_after, uint32_t* support /* capacity *n_support in, may be NULL */, uint32_t* n_support);
void todhip_model_free(todhip_ctx*, todhip_model*);

/* ---- training: an rBRIEF test pattern learned from training views (Rublee et al., ORB, section 4.3) ------------------ */
/* The built-in pattern of todhip_orb* is 256 seeded random tests: steered BRIEF, whose bits are biased and correlated. A learner
 * collects the keypoints of training views, evaluates every candidate test on every keypoint's steered patch, and picks 256 tests
 * whose means are near 0.5 and which are pairwise uncorrelated. The result is a `pattern` argument for every todhip_orb* form,
 * todhip_model_add_observation and todhip_pipeline_set_pattern; DB and queries must be described with the same pattern. One learner
 * call in flight per context, as everywhere. Definition (exact integers, deterministic):
 * Candidates: M tests (x0, y0, x1, y1) in int8, 256 <= M <= 65536, every point with x^2 + y^2 <= 169 (the built-in pattern's disc: a
 * rotated, rounded point stays inside the 31 x 31 patch); anything else, or capacity_keypoints of 0 or above 32768: TODHIP_EINVAL.
 * candidates == NULL (n_candidates ignored) selects the built-in set: G = the points with x and y even and x^2 + y^2 <= 169, ordered
 * by y ascending, then x ascending; the candidates are all pairs i < j of G, in lexicographic (i, j) order, at squared distance >= 16,
 * test = (G[i], G[j]).
 * Keypoints: add_view runs the detection stages of todhip_orb_masked with the same arguments (pyramid, FAST + NMS, Harris ranking,
 * blur, intensity-centroid angle; output capacity n_features) and adds that call's keypoints in its output order, as many as still
 * fit below capacity_keypoints: *n_added. Keypoint n of the learner is the n-th added overall, N their number. The device form takes
 * d_gray (row stride `stride`) and d_mask (row stride W, may be NULL) in HBM.
 * Response matrix: R[c][n] = 1 iff candidate c, steered for keypoint n exactly as a pattern row is steered for a descriptor bit,
 * reads blur[p0] < blur[p1]. So for any 256 candidates used as a `pattern`, bit b of todhip_orb_masked's descriptor of keypoint n is
 * R[that candidate][n]. Stored candidate-major: bit n % 32 of word n / 32 of row c, ceil(N / 32) words per row, padding bits zero.
 * Selection (finish; N == 0: TODHIP_EINVAL): ones[c] = popcount of row c, both[a][c] = popcount of (row a & row c),
 * v[c] = ones[c] (N - ones[c]). Candidate order: v descending, ties by ascending c. g(a, c) = |N both[a][c] - ones[a] ones[c]|.
 * Rounds 1-4 use s = 6, 4, 2, 0: a round walks the not yet accepted candidates in candidate order and accepts c iff v[c] > 0 and
 * (g(a, c)^2 << s) < v[a] v[c] for every a accepted so far, in any round (|correlation| < 1/8, 1/4, 1/2, 1: the paper's "raise the
 * threshold and go again"). Round 5: the remaining candidates with v > 0, in candidate order. Round 6: the rest, in candidate order.
 * Everything stops at 256 accepted. With N <= 2^15 every term fits an unsigned 64-bit integer (g <= 2^28, g^2 << 6 <= 2^62).
 * Outputs: chosen[r] = the candidate accepted r-th, round_of[r] in 1..6 (both may be NULL), stats (may be NULL); pattern row pos(r) =
 * candidate chosen[r], pos(r) = r for TODHIP_PATTERN_ORDER_RANK and 32 E[r / 32] + r % 32, E = {0, 4, 1, 5, 2, 6, 3, 7}, for
 * TODHIP_PATTERN_ORDER_MATCHER -- the layout todhip_set_db_bit_order documents: ranks 0-127 are what a 2-split block of the matrix-core
 * matcher sees first. Any other order: TODHIP_EINVAL. finish may be called again (another order, or after further views). */
typedef struct todhip_pattern_learner todhip_pattern_learner;
enum { TODHIP_PATTERN_ORDER_RANK = 0, TODHIP_PATTERN_ORDER_MATCHER = 1 };
typedef struct { uint32_t n_keypoints, n_candidates, accepted_in_round[6]; } todhip_pattern_stats;
int  todhip_pattern_learn_begin(todhip_ctx*, const int8_t* candidates /* M x 4, or NULL */, uint32_t n_candidates,
                                uint32_t capacity_keypoints, todhip_pattern_learner** out);
int  todhip_pattern_learn_add_view(todhip_ctx*, todhip_pattern_learner*, const uint8_t* gray, const uint8_t* mask /* may be NULL */,
                                   uint32_t H, uint32_t W, uint32_t stride, uint32_t n_features, uint32_t n_levels,
                                   float scale_factor, uint32_t* n_added);
int  todhip_pattern_learn_add_view_device(todhip_ctx*, todhip_pattern_learner*, const void* d_gray, const void* d_mask /* may be NULL */,
                                          uint32_t H, uint32_t W, uint32_t stride, uint32_t n_features, uint32_t n_levels,
                                          float scale_factor, uint32_t* n_added);
int  todhip_pattern_learn_finish(todhip_ctx*, todhip_pattern_learner*, int order, int8_t pattern[1024], uint32_t chosen[256],
                                 uint8_t round_of[256], todhip_pattern_stats*);
/* test hook: rows first .. first + count - 1 of the response matrix, count x ceil(N / 32) u32, to the host */
int  todhip_pattern_learn_responses(todhip_ctx*, todhip_pattern_learner*, uint32_t first, uint32_t count, uint32_t* words);
void todhip_pattern_learn_free(todhip_ctx*, todhip_pattern_learner*);

/* ---- diagnostics --------------------------------------------------------------------------------- */
/* Per-RANSAC-round trace of the last todhip_verify call (what GuessGenerator.cpp:202 prints, plus the
 * rand() stream position): `iterations` = iterations_ at loop exit (ransac.h:95-135). */
typedef struct {
  uint32_t object, iterations, best_iteration;
  int32_t  best_count;
  uint64_t draws_before, draws_after;
  uint32_t n_inlier_kp, accepted;
} todhip_round_trace;
int todhip_verify_trace(const todhip_ctx*, todhip_round_trace* out, uint32_t* n /* capacity in, count out */);
/* FillAdjacency (adjacency_ransac.cpp:127-172) alone: n matches (train/query n x 3, per-match keypoint pixel
 * n x 2) -> physical and sample bit matrices, n rows of ceil(n/64) u64 words each. */
int todhip_test_adjacency(todhip_ctx*, const float* train_xyz, const float* query_xyz, const float* kp_xy_per_match,
                          uint32_t n, float span, float sensor_error, uint64_t* phys, uint64_t* samp);
/* The verifier's clique search (maximum_clique.cpp:343-369, FindClique(minimal_size); 0xFFFFFFFF =
 * FindMaximumClique) on an explicit graph of m <= 1024 vertices, as the reference's own gtests call it
 * (test/test_maximum_clique.cpp:7-53). out3 = {clique size, internal error flag, search steps}. */
int todhip_test_clique(todhip_ctx*, uint32_t m, const uint32_t* edges, uint32_t n_edges, uint32_t minimal_size,
                       uint32_t* out3);
/* The depth lookup of the verifier's cluster kernel alone: z_out[i] = the depth in metres at pixel (int(kp_xy[2i]), int(kp_xy[2i+1]))
 * of rescale_depth's H x W result of the device-resident dH x dW image, computed as todhip_verify_device_depth_rescaled computes it
 * (equal sizes: the plain load of todhip_verify_device_depth). kp_xy (n x 2) and z_out (n) are host arrays. A position outside the
 * H x W image is what the verifier refuses: TODHIP_ERANGE, that z_out entry untouched, the others filled. */
int todhip_test_depth_lookup(todhip_ctx*, const void* d_depth, int depth_is_u16, uint32_t dH, uint32_t dW, int nearest, uint32_t H,
                             uint32_t W, const float* kp_xy, uint32_t n, float* z_out);
/* The same graph through the form of the search the verifier's gate runs: sac_model_registration_graph.h:260-262 only asks whether
 * the clique FindClique(minimal_size) returns is larger than minimal_size, which is decided once Q holds minimal_size vertices
 * with a common neighbour (or at the first leaf of at least that size) -- the search stops there. out3[0] = that clique's size
 * when it is <= minimal_size, a lower bound > minimal_size otherwise; out3[2] = steps actually walked. */
int todhip_test_clique_gate(todhip_ctx*, uint32_t m, const uint32_t* edges, uint32_t n_edges, uint32_t minimal_size,
                            uint32_t* out3);
/* The verifier's speculative draw table of one object alone (drawIndexSampleHelper, sac_model_registration_graph.h:102-132, started
 * at every position 0 .. S - 1 of the window_len words rnd of the rand() stream): samp = the n x W sample bit matrix, valid = W
 * words, W = ceil(n / 64), all host arrays. entries_out: S entries of six words {status (0 failed, 1 drawn, 2 the window ended
 * first), draws consumed, the three samples deepest first, 0}. form: 0 = the kernel the verifier itself would pick for this n,
 * 1 = one lane per position (n <= 512), 2 = one wave per position over 64 words (n <= 4096), 3 = over 512 words, 4 = one lane
 * per position with eight words a lane also where n <= 128 (form 1 picks the two-word kernel there); a form that cannot hold n
 * matches is TODHIP_EINVAL. */
int todhip_test_draw_table(todhip_ctx*, const uint64_t* samp, const uint64_t* valid, uint32_t n, const uint32_t* rnd,
                           uint32_t window_len, uint32_t S, uint32_t form, uint32_t* entries_out);
/* The pose solve of the verifier's refinement alone (the tail of estimateRigidTransformationSVD, sac_model_registration_graph.h:330-346),
 * one GPU lane per case: Hd = n_cases correlation matrices (9 doubles each, row-major, rounded to float as the verifier rounds its
 * double sums), C = n_cases centroid pairs {train xyz, query xyz}; R (n_cases x 9) and T (n_cases x 3) map query -> train, i.e. the
 * pose before todhip_verify inverts it. Host arrays. The range is that of todhip_verify (see there). */
int todhip_test_kabsch(todhip_ctx*, uint32_t n_cases, const double* Hd, const float* C, float* R, float* T);

/* FillAdjacency + selectWithinDistance (sac_model_registration_graph.h:171-269) for given sample triples
 * (samples_ order): counts[t] = consensus size, 0 when the clique gate rejects. stop_level 1 skips the clique
 * search (counts[t] = -|F| where it would have run). dbg (optional, dbg_stride u32 per triple): {count, |F|,
 * then (F member, its degree in the induced graph) pairs}. */
int todhip_test_consensus(todhip_ctx*, const float* train_xyz, const float* query_xyz, const float* kp_xy_per_match,
                          uint32_t n, float span, float sensor_error, const uint32_t* triples, uint32_t n_triples,
                          uint32_t stop_level, int32_t* counts, uint32_t* dbg, uint32_t dbg_stride);

#ifdef __cplusplus
}
#endif
#include "todhip_ratio_other.h"
#endif /* TODHIP_H_ */
