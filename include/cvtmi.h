/*
 * cvtmi.h -- C ABI of the MI355X-native OPQ-encode / ADC-search hot path of willard-yuan/cvt.
 *
 * This is the drop-in boundary: a C++ (or cgo / ctypes / JNI) caller that today runs the loops
 * of the reference's L1 layer on the CPU binds these entry points instead.  Each entry names the
 * reference interface it replaces (paths relative to the reference tree).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, opaque handles, no C++ / torch types.
 *   - Every function returns 0 (CVTMI_OK) or a negative cvtmi_status; the message of the last
 *     failure on the calling thread is cvtmi_last_error().  No exception crosses the boundary.
 *   - Functions without a suffix take HOST pointers (caller-owned buffers, like the reference's
 *     float** / float* arguments) and return when the result is in the caller's buffer.
 *     Functions ending in `_dev` take DEVICE pointers (HBM-resident) plus a `stream`
 *     (a hipStream_t passed as void*, NULL = the default stream) and are asynchronous.
 *   - Handles may be shared between threads and streams.  SEARCHES on one handle (cvtmi_opq_search*, cvtmi_opq_query_video*,
 *     cvtmi_flat_search*, cvtmi_hnsw_search*) are reads, as QueryThrehold / searchKnn are in the reference
 *     (opq/src/IVFOPQ.cpp:322-422, brutoforce.hpp:73-93, hnswalg.h:688-728): each call leases a scratch set from the
 *     handle's pool (tables, partial top-k lists, visited bitmaps, staging buffers; the pool grows to the number of calls
 *     in flight) and runs on its caller's stream (host-pointer entries: the set's own stream), so searches from several
 *     threads or streams proceed side by side and every one returns what a search alone would.  Calls that CHANGE a
 *     handle (add, add_codes, set_param, load, cvtmi_hnsw_add) take it exclusively: they wait for the searches in flight, and searches
 *     issued later wait for them; the result is that of some serial order.  cvtmi_hnsw_search_adc* holds its OPQ handle
 *     the way a search of that handle would.  A sharded search additionally serialises on its communicator (below).  The
 *     small accessors (ntotal, set_id_base) take no lock: do not race them with calls that change the handle.
 *   - One handle lives on the HIP device that was current when it was created.
 *   - The library has no CPU fallback: without a usable HIP device every compute entry fails
 *     with CVTMI_EHIP.
 *
 * Numerics contract (tests/ enforce it against oracle/ and the golden vectors):
 *   uint8 PQ codes, list ids, SQ8 codes, uint8-L2 distances: bit-exact.
 *   LUT entries and ADC distances: bit-exact (same fp32 operation order as the reference,
 *   separate multiply and add), which implies the 1e-4 relative bound of the north star.
 *   top-k: the k smallest (distance, id) pairs in lexicographic order, ascending.
 */
#ifndef CVTMI_H
#define CVTMI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CVTMI_VERSION 200 /* 0.2.0 */
/* Largest k of the search entries (cvtmi_opq_search*, cvtmi_flat_search*, cvtmi_topk_*): searchKnn(query, k) and
 * get_sort_results(score, num_show) of the reference take any k (brutoforce.hpp:73-93, opq/src/common.h:25-37).  k <= 128 runs on
 * every kernel; 129 .. CVTMI_K_MAX on the exact kernels (one query per workgroup, 4096-entry selection buffer) -- slower per query. */
#define CVTMI_K_MAX 2048

typedef enum cvtmi_status {
    CVTMI_OK = 0,
    CVTMI_EINVAL = -1,       /* bad argument */
    CVTMI_ENOMEM = -2,       /* host or device allocation failed */
    CVTMI_EHIP = -3,         /* HIP runtime error / no device */
    CVTMI_ESTATE = -4,       /* handle not in a state that allows the call */
    CVTMI_EUNSUPPORTED = -5, /* shape outside what the kernels are built for */
    CVTMI_ECOMM = -6,        /* RCCL not loadable / a collective failed */
    CVTMI_ESPACE = -7        /* the result does not fit the caller's arrays; lims holds the sizes (cvtmi_opq_range_search_ivf) */
} cvtmi_status;

typedef enum cvtmi_metric {
    CVTMI_METRIC_IP = 0,   /* 1 - <q,x>, fp32   : brute_force_search/src/space_ip.hpp:211-239 */
    CVTMI_METRIC_L2F = 1,  /* sum (q-x)^2, fp32  : hnsw_sifts_retrieval/hnswlib/space_l2.h:153-184 */
    CVTMI_METRIC_L2U8 = 2  /* sum (q-x)^2, uint8 -> int32 : space_l2.h:186-245 (L2SqrI / L2SpaceI) */
} cvtmi_metric;

typedef struct cvtmi_opq_s *cvtmi_opq_t;
typedef struct cvtmi_flat_s *cvtmi_flat_t;
typedef struct cvtmi_hnsw_s *cvtmi_hnsw_t;
typedef struct cvtmi_comm_s *cvtmi_comm_t;

/* ---------------------------------------------------------------- library / device ---------- */
int cvtmi_version(void);
const char *cvtmi_last_error(void);
int cvtmi_device_count(int *count);
int cvtmi_set_device(int device);
/* Library-wide tuning / measurement hooks (no effect on results).
 *   "assign_variant"  nearest-centroid assignment (coarse argmin of cvtmi_opq_encode, cvtmi_kmeans): 0 = choose (default);
 *                     1 = the reference's chain for every centroid on the VALU; 2 = bf16 matrix-core filter with exact
 *                     resolution of undecided rows wherever it applies (32 <= d <= 128, d % 16 == 0, k >= 64)
 *   "flat_variant"    exhaustive search: 0 = choose (default: large batches through the filter pipelines -- fp32: bf16 matrix-core
 *                     filter with a proven bound; uint8: exact sample, software-pipelined i8 matrix-core threshold filter, sort,
 *                     from 256 queries on >= 1 M rows; smaller uint8 batches are one stream over the rows, 128 queries per pass); 1 = exact / row-tile
 *                     kernels only; 2 = the filter pipelines wherever they apply
 *   "flat_u8_gfilter" the uint8 filter stage: 1 (default) / 3 = LDS-DMA pipelined kernel, one 8-wave workgroup per CU; 2 = two 4-wave
 *                     workgroups per CU; 4 = one wave per SIMD holding 96-128 queries (GEMM-shaped; measured equal / slower);
 *                     0 = the round-1 filter kernel (register-staged tiles)
 *   "flat_u8_dbg"     timing experiments of the filter kernel (-DCVTMI_GF_DBG builds only; EUNSUPPORTED otherwise: results are wrong)
 *   "flat_u8_mstream_min"  smallest uint8 batch that takes the streaming matrix-core kernel (default 1; 129 = never: row-per-lane / row-tile kernels)
 *   "sq8_encode_wave" 0 = SQ8 encode through the 64-row tile kernel for every width (default 1: wave-per-row kernel at d = 256 / 512)
 *   "sq8_wave_blocks" workgroups per CU of the wave-per-row SQ8 training kernel (default 3; powers of two lose 8 % to HBM channel conflicts)
 *   "flat_u8_opt"     measurement variants of the uint8 row-tile kernel (0 = shipped; 1..3 spill registers and are slower)
 *   "probe_variant"   coarse top-nk of cvtmi_opq_query_video: 0 = choose (matrix-core filter + exact distances of the candidates
 *                     from 256 query frames, 32 <= D <= 128, coarseK >= 256); 1 = exact kernels only; 2 = filter wherever it applies
 *   "flat_f32_nt"     non-temporal hint on the row loads of the fp32 stream kernels (rows a CU reads once per launch need no place in
 *                     L2 / Infinity Cache): 0 = never, 1 = choose (default: everywhere except three query blocks per wave), 2 = always
 *   "scan_seed"       1 (default) = scan variants 3 / 4 / 5 take their first filter thresholds from a histogram of the first 2048 rows of
 *                     a row split instead of starting with "every row passes" (1-4 % on 1 M rows, more on short splits); 0 = off
 *   "scan_tail_splits" adc_scan16q, query groups past the last full round of workgroups: 0 (default) = cut them into 2 / 4 / 8 row
 *                     splits while that still leaves at most one workgroup per CU (a last round is only expensive while it leaves CUs
 *                     empty: 4256 queries over 1 M rows 2.11 -> 2.79 M queries/s, 10 000 queries unchanged); -1 = never; S > 0 = S splits
 *   "ivf_part_cap_mb" cvtmi_opq_search_ivf: megabytes the partial lists of one search may take in the leased scratch set (default 256,
 *                     0 = none: one workgroup per query); a grid that needs more is cut coarser (rule 4 of cvtmi_opq_ivf_plan).
 *                     cvtmi_opq_rank_videos: the same bound on each of the ranking's two areas, the score rows of a frame chunk and
 *                     the totals of a segment group (0 = one frame per chunk, one segment per group)
 *   "scan_pad_m"      1 (default) = an OPQ index with M < 16 is searched by the M = 16 scan kernels over rows padded to 16 code bytes
 *                     with zeros (derived copies: 32 bytes per row) and per-query tables padded with all-zero tables -- M = 8 at
 *                     10 000 queries x 1 M rows: 9.8 -> 3.2 ms, and every M from 1 to 15 is searchable; 0 = the row-per-lane
 *                     kernels (M = 4 / 8 only)
 *   "scan_bigk"       1 (default) = an OPQ search (M = 16, >= 65 536 rows) with k = 129 .. 2048 runs through the filter scan: a sampled
 *                     histogram bound per query, candidate lists, one selection workgroup per query, the exact kernel behind it for the
 *                     queries it could not answer (round 6: k = 1000 at 10 000 queries x 1 M rows within 2x of k = 100); 0 = the exact
 *                     kernel for every query (one query per workgroup: 11x slower at that size)
 *   "scan_packed_m"   1 (default) = an OPQ index with M = 8 or M = 4 is scanned as it lies in memory (adc_scan16p, round 6): 16 / M rows
 *                     per 16-byte load from a pre-rotated copy of the rows (+M bytes per row, no padded copy), 16 / M copies of the M
 *                     tables in LDS so that the look-ups stay conflict-free -- no look-up is spent on a zero table; 0 = the padded
 *                     rows of "scan_pad_m" for these M as well
 *   "sq8_host_small" 1 (default) = SQ8 host-pointer calls of up to 1 MB (the reference's one vector per call) run out of a page-locked
 *                     scratch area the kernels read and write directly (512-d: 80 -> 26 us per call); 0 = allocate, copy, free
 *   "scans_max_work"  OPQ search: the small-batch form (<= 128 queries) answers while rows x query groups stays at or under this
 *                     (default 48 << 20; beyond, its per-group passes over the table lose to the persistent grid: 100 M rows,
 *                     128 queries 8.3 against 3.7 ms)
 *   "flat_u8_filter_min_nq" / "flat_u8_filter_min_rows" / "flat_u8_filter_min_work"  uint8 search: the sample + matrix-core filter pipeline
 *                     answers from this many queries (default 129), rows (524 288) and rows x width x queries in units of 1e9
 *                     (130) on; below, passes of up to 128 queries through the streaming kernel (round 5: the fitted crossover)
 *   "flat_u8_tfilter" 1 (default) = uint8 batches over >= 65 536 rows of 32 … 512 bytes in steps of 32 go through the threshold
 *                     filter of round 6 (flat_u8_tfilter.hip: exact integer scores on the i8 matrix cores, 256 queries in LDS per pass, thresholds
 *                     from 4096 sample maxima, no margins): every batch when k = 129 .. 2048 (2 M x 512-d, 1000 queries, k = 129: 139 -> 1.5 ms),
 *                     k <= 128 from "flat_u8_tfilter_min_nq" (129) queries on, k = 65 .. 128 and tables of a GB or more from "flat_u8_tfilter_min_nq_k65" (97) on and only
 *                     for k >= "flat_u8_tfilter_min_k" (1); 0 = the streaming passes / the sample + filter pipeline / the exact kernels as in
 *                     round 5.  "flat_u8_tfilter_sample": the sample pass takes one tile group in this many (0 = sqrt(8000 x GB of rows / k) within 2 .. 32);
 *                     "flat_u8_tfilter_chunks": query chunks (1 / 2 / 4, default 4) that share one pass over the rows;
 *                     "flat_u8_tfilter_min_rows" (262 144) / "flat_u8_tfilter_small_min_nq" (129): tables under _min_rows come here from that many queries on;
 *                     widths without a streaming kernel (all but 128 / 256 / 512 bytes) from two queries on
 *   "flat_u8_mstream_min_rows" smallest table the uint8 streaming kernel takes (default 4096 = its structural bound; it was 262 144 until
 *                     round 5: 65 536 x 512-d, 100 queries 0.84 -> 0.06 ms)
 *   "flat_u8_sample_passes" the uint8 filter pipeline searches its leading sample exactly through the streaming kernel while that takes at
 *                     most this many 128-query passes (default 10: batches up to 1280 queries), through the row-tile kernels beyond
 *   "flat_small_zero_copy" 1 (default) = a small host-pointer flat search (queries <= 64 KB, lists <= 768 KB: the brute_force CLI's one
 *                     searchKnn per query) sends its queries up from a page-locked staging area and lets the last kernel write the
 *                     lists into that area (1 M x 128-d, one query: 137 -> 125 us per call); 0 = three copy-engine copies
 *   "opq_host_zero_copy" 1 (default) = cvtmi_opq_search with page-locked result arrays lets the kernels write them (one launch chain);
 *                     0 = pipelined pieces through device buffers and the copy engines, as for pageable arrays
 *   "sq8_filter"      1 (default) = the wave-per-row SQ8 kernels (d = 256 / 512) decide code bytes / column extremes from a bounded
 *                     approximation and run the reference's chain (two correctly rounded divisions + the byte) only where it cannot
 *                     decide; 0 = the chain for every element.  Same codes, rows and ranges, bit for bit
 *   "sq8_flags"       bit 0 (default set) = the row-norm sums of those kernels run on DPP moves instead of the ds_bpermute butterfly
 *   "hnsw_adc_tables" HNSW over OPQ codes: 0 (default) = a query's fp32 distance tables are read from the table scratch (L2 / Infinity
 *                     Cache), 32 traversals per CU; 1 = copied into LDS first (16 KB per query: 8 traversals per CU, round 2 - 4)
 *   "comm_force_rccl" 1 = cvtmi_comm_create goes through RCCL (ncclCommInitRank, ncclAllGather) for world == 1 too, which
 *                     otherwise needs no transport (test hook for 1-GPU boxes)
 *   "comm_inject_failure" r >= 0: the local search of rank r of every sharded search fails (tests of the failure path); -1 = off
 *   "opq_host_chunk"  queries per piece of cvtmi_opq_search's pipelined form for pageable arrays (default 4096 = one full round of
 *                     workgroups; 0 = one piece)
 *   "opq_small_zero_copy" 1 (default) = host-pointer OPQ searches that take the small-batch form read their queries from and write their
 *                     lists to the handle's pinned staging area from the kernels (no copy engine in the chain); 0 = copies
 *   "host_spin_us"    microseconds a host-pointer entry polls its stream before it blocks (default 200: waking from a blocking wait costs
 *                     as much again as a small search)
 *   "scanh_balance" / "scanh_min_rows" / "scanh_tail" / "scanh_fix" / "scanh_share_hist"  planner of the persistent-grid scan (variant
 *                     6): 0 choose / 1 equal row-time shares / 2 row blocks; smallest row segment; two-region tail on / off; an item's
 *                     fixed cost in row-equivalents (160 000); one candidate histogram per query shared by its segments (1) or not
 *   "flat_f32_tfilter" fp32 searches (any width that is a multiple of 4 up to 2048-d, >= 262 144 rows, k <= 128; k up to 2048: "flat_f32_tfilter_bigk") of "flat_f32_tfilter_min" queries or more run as a
 *                     threshold filter (round 6, flat_f32_tfilter.hip): sample maxima -> per-query threshold -> queries in LDS, the rows'
 *                     bf16 operand copy in registers, no barrier, hits recorded -> per-query lists -> exact distances.  1 .. 3 = the
 *                     bf16 products per term: 1 (x1.q1), 2 ((x1 + x2).q1; both with margins from each query's own rounding residues),
 *                     3 (x1.q1 + x2.q1 + x1.q2, the stream kernels' margin); 4 (default) = one product up to "flat_f32_tfilter_one"
 *                     (default: no limit -- measured ahead at every batch size) queries, two beyond; 0 = the stream kernels for every
 *                     batch.  1 M x 128-d, top-100: 1000 queries 0.97 -> 0.69 ms, 128 queries 0.25 -> 0.16 ms, 16 queries 0.119 -> 0.107 ms
 *   "flat_f32_tfilter_min"  smallest batch that takes that pipeline; 0 (default) = choose: 65 ... 97 at the widths the stream kernels take (smaller batches
 *                     stream the operand copy, "flat_f32_packed"), 16 at the others
 *   "flat_f32_tfilter_one"  largest batch that multiplies one product under "flat_f32_tfilter" 4
 *   "flat_f32_packed" 1 (default) = fp32 searches of up to 32 queries (the stream kernels' private rings) read the bf16 operand copy the threshold
 *                     filter keeps -- one ready-made term per value, half the bytes of the fp32 rows, one product, margins from the query's
 *                     own rounding residues -- on tables that have one (>= "flat_f32_tfilter_min_rows" rows); 0 = the fp32 rows, split on the fly
 *   "flat_f32_tfilter_min_rows"  smallest table that takes that pipeline (default 262 144; >= 32 768.  Measured on 128-d: below ~130 K rows the stream
 *                     kernels are ahead for fewer than 128 queries and level beyond; 200 K rows, 1000 queries 0.42 -> 0.32 ms)
 *   "flat_f32_tfilter_sample"  the sample that sets the thresholds is about 1 / this of the row-tile groups, spread evenly over the
 *                     rows and rounded to a whole number of groups per wave (1 M x 128-d, 1000 queries, k = 100: 1/8 0.63 ms, 1/5 0.505, 1/3 0.52);
 *                     0 (default) = sqrt(1280 x GB / k) within 3 .. 32 (: 4 M x 128-d, k = 10: 1.31 -> 1.04 ms)
 *   "flat_f32_rows_copy"  narrowest fp32 row (default 4 = every width the threshold filter takes; 0 = never) that gets a row-major copy beside the
 *                     blocked rows once the filter answers on the handle: + 4 D bytes per row, the exact finish reads whole cache lines instead of 16 of
 *                     every 128 bytes (262 144 x 1024-d, 1000 queries: 1.89 -> 1.14 ms; 1 M x 128-d 0.53 -> 0.47); skipped where it does not fit
 *   "flat_f32_tfilter_wide_band"  1 (default) = rows of 256 dimensions or more: a query with more than 1024 rows inside the margin band of its k-th
 *                     score (tight, non-negative features) gets a second finish that ranks up to 4096 (262 144 x 1024-d RootSIFT-shaped rows,
 *                     k = 128: 18.6 -> 6.2 ms per 1000 queries); 0 = the exact kernels answer such a query
 *   "flat_f32_tfilter_bigk"  1 (default) = fp32 searches with k = 129 .. 2048 (every batch size, tables of "flat_f32_tfilter_min_rows" rows and more)
 *                     run through the threshold filter with 4096 sample maxima, candidate lists of 32 768 and a workgroup-wide selection
 *                     (1 M x 128-d, 1000 queries: k = 129 46.6 -> 1.3 ms, k = 1000 47.8 -> 2.4, k = 2048 53.5 -> 3.2); 0 = the exact kernels
 *   "flat_f32_tfilter_retry"  1 = a query whose candidate list ran over takes ONE second filter pass under the threshold its own stored
 *                     candidates give (it helps when the rows above the sample's threshold are many, not when the rows inside the
 *                     margin band are: measured no gain on clustered 300-d rows, three empty launches = ~10 us on every search);
 *                     0 (default) = the exact kernels at once
 *   "flat_f32_share"  fp32 stream, batches beyond one wave's queries: 0 choose, 1 the four-wave shared ring (the same form; the
 *                     eight- and twelve-wave forms, formerly 2 and 3, were removed: a sweep against the exact kernels found one query
 *                     of ~10^5 they answered wrongly -- 2 and 3 now fail with CVTMI_EINVAL)
 *   "hnsw_top_lds"    entries of an HNSW traversal's top queue kept in LDS (default 256; 0 = all)
 *   "hnsw_slots"      cap on HNSW traversals per CU (0 = what LDS allows, at most 32)
 *   "hnsw_build_frac" cvtmi_hnsw_build: a batch holds at most 1/value of the rows already inserted (default 32)
 *   "hnsw_build_cap"  cvtmi_hnsw_build with max_batch = 0: rows per batch at most (default 8192).  Unlike the other keys these
 *                     two change results: they are the schedule, and the graph depends on it (the schedule sweep of DESIGN.md 4.11)
 *   "hnsw_build_phases" 1 = time the phases of cvtmi_hnsw_build (cvtmi_hnsw_build_phases)
 *   "flat_count_redo" 1 = every flat search counts the queries its threshold filter / fp32 stream handed to the exact kernels
 *                     (cvtmi_flat_last_redo; the count is copied back and waited for inside the call); 0 (default) = not counted
 *   "scans_dbg" / "flat_f32_dbg"  measurement switches of the small-batch scan and of the fp32 stream (phases skipped: results are WRONG
 *                     when non-zero; development only) */
int cvtmi_set_tuning(const char *name, int64_t value);
/* The value a key holds now: its default, or what the last accepted cvtmi_set_tuning made of its argument (clamped, snapped).
 * A null argument or an unknown key gives CVTMI_EINVAL; no device is needed. */
int cvtmi_get_tuning(const char *name, int64_t *value);

/* ---------------------------------------------------------------- OPQ model + code index ---- */
/*
 * Replaces IVFOPQ::LoadModel's in-memory tables (opq/src/IVFOPQ.cpp:64-102):
 *   coarse [coarseK][D] fp32, books [M][K][D/M] fp32 (each sub-codebook contiguous), and the
 *   "rotation": either perm[D] (the reference's reorder_, y[i] = x[perm[i]], IVFOPQ.cpp:424-439)
 *   or a dense row-major R[D][D] (y = R x, the general OPQ rotation run as an fp32 MFMA GEMM);
 *   both NULL = identity.  K <= 256, M <= 16 (IVFelem::PQindex[16], IVFOPQ.h:28), D % M == 0.
 */
int cvtmi_opq_create(int D, int coarseK, int M, int K, const float *coarse, const float *books,
                     const float *R, const int32_t *perm, cvtmi_opq_t *out);
int cvtmi_opq_destroy(cvtmi_opq_t h);

/* IVFOPQ::reorder over n rows (IVFOPQ.cpp:424-439, :459-461).  x and y may not alias. */
int cvtmi_opq_rotate(cvtmi_opq_t h, const float *x, int64_t n, float *y);
int cvtmi_opq_rotate_dev(cvtmi_opq_t h, const float *x, int64_t n, float *y, void *stream);

/* The encode loop of IVFOPQ::Add (IVFOPQ.cpp:107-163) on already-rotated rows:
 * list_id[n] = coarse argmin (first minimum, -1 if none), codes[n][M] = per-sub-quantiser argmin
 * (255 if none).  list_id may be NULL. */
int cvtmi_opq_encode(cvtmi_opq_t h, const float *x_rot, int64_t n, int32_t *list_id, uint8_t *codes);
int cvtmi_opq_encode_dev(cvtmi_opq_t h, const float *x_rot, int64_t n, int32_t *list_id, uint8_t *codes,
                         void *stream);

/* LoadSingleFeatFile's reorder + Add's encode (IVFOPQ.cpp:459-461 + :107-163) on RAW rows in one call: what cvtmi_opq_rotate followed
 * by cvtmi_opq_encode computes, without a caller-side buffer of rotated rows (they pass through a cache-resident scratch of the
 * handle).  Same codes and list ids. */
int cvtmi_opq_rotate_encode(cvtmi_opq_t h, const float *x, int64_t n, int32_t *list_id, uint8_t *codes);
int cvtmi_opq_rotate_encode_dev(cvtmi_opq_t h, const float *x, int64_t n, int32_t *list_id, uint8_t *codes,
                                void *stream);

/* m_ivfList[vw].push_back(elem) of Add (IVFOPQ.cpp:167): append n entries to the resident index.
 * list_id NULL = list 0 (only valid when coarseK == 1); video_id NULL = one "video" per entry,
 * numbered by insertion order.  Entry ids are id_base + insertion index. */
int cvtmi_opq_add_codes(cvtmi_opq_t h, const uint8_t *codes, const int32_t *list_id,
                        const int32_t *video_id, int64_t n);
int cvtmi_opq_add_codes_dev(cvtmi_opq_t h, const uint8_t *codes, const int32_t *list_id,
                            const int32_t *video_id, int64_t n, void *stream);
int cvtmi_opq_reserve(cvtmi_opq_t h, int64_t n_total);
int cvtmi_opq_ntotal(cvtmi_opq_t h, int64_t *n);
int cvtmi_opq_reset(cvtmi_opq_t h);                      /* drop all entries, keep the model */
int cvtmi_opq_set_id_base(cvtmi_opq_t h, int64_t base);  /* first id of this row shard */
/* Copy the resident entries back in list order (the SaveIndex order, IVFOPQ.cpp:557-575).
 * list_off[coarseK+1], video_id[ntotal], codes[ntotal][M]; any may be NULL. */
int cvtmi_opq_get_entries(cvtmi_opq_t h, int64_t *list_off, int32_t *video_id, uint8_t *codes);

/* PQ_table of Query (IVFOPQ.cpp:273-291): lut[nq][M][K] for rotated queries; list_id[nq] selects
 * the coarse centroid each residual is taken against (NULL = list 0). */
int cvtmi_opq_lut(cvtmi_opq_t h, const float *q_rot, int64_t nq, const int32_t *list_id, float *lut);
int cvtmi_opq_lut_dev(cvtmi_opq_t h, const float *q_rot, int64_t nq, const int32_t *list_id, float *lut,
                      void *stream);

/* The north-star search: (optional rotation) + LUT + exhaustive ADC scan (IVFOPQ.cpp:300-306)
 * + k smallest (distance, id) (opq/src/common.h:25-37) per query, over every resident entry.
 * Requires coarseK == 1.  dist[nq][k] / ids[nq][k] ascending; rows short of k entries are padded
 * with (+inf, -1).  rotate != 0 applies cvtmi_opq_rotate to the queries first.  1 <= k <= CVTMI_K_MAX. */
int cvtmi_opq_search(cvtmi_opq_t h, const float *q, int64_t nq, int rotate, int k, float *dist,
                     int64_t *ids);
int cvtmi_opq_search_dev(cvtmi_opq_t h, const float *q, int64_t nq, int rotate, int k, float *dist,
                         int64_t *ids, void *stream);

/* IVFOPQ::Query / QueryThrehold (IVFOPQ.cpp:213-320 / :322-422): per query frame probe the nprobe
 * nearest coarse lists and keep, per video, the minimum ADC score clamped at 1.0.
 * match_score[nq][img_num].  rotate as above.  The list-ordered copy of the entries is (re)built on the device by the
 * first query after an append (a stable counting sort; ~2.5 ms per million entries); entries whose list id is outside
 * [0, coarseK) are skipped; a video id outside [0, img_num) fails the call.  nprobe > coarseK is clamped to coarseK;
 * an nprobe above 128 (after the clamp) fails with CVTMI_EUNSUPPORTED.
 * Non-finite frames score as in the reference's std::min fold: a frame holding a NaN probes lists 0 .. nprobe-1 and
 * gets NaN in every video with an entry there (1.0 elsewhere); a frame whose scores are all +inf keeps 1.0.  Frames
 * whose scores mix NaN and finite values (possible only with non-finite codebooks) depend on the reference's visiting
 * order and are not matched. */
int cvtmi_opq_query_video(cvtmi_opq_t h, const float *q, int64_t nq, int rotate, int nprobe,
                          int img_num, float *match_score);
int cvtmi_opq_query_video_dev(cvtmi_opq_t h, const float *q, int64_t nq, int rotate, int nprobe,
                              int img_num, float *match_score, void *stream);

/* The whole query of the reference's main (opq/src/multi_frame_index_test.cpp:51-84) for nseg query videos at once: Query, the sum
 * of its rows in frame order, get_sort_results -- and only the lists leave the device.
 *   Input    q holds seg_off[nseg] frames of D floats; segment s (one query video) is frames seg_off[s] .. seg_off[s + 1] - 1.
 *            seg_off is a HOST array of nseg + 1 int64 in BOTH entries, seg_off[0] == 0, never decreasing; it is read before the
 *            call returns (the host plans the chunks from it).  The _dev entry never waits for the device: q, score, video and
 *            total are device pointers there.
 *   Scores   ms[f][v] is exactly what cvtmi_opq_query_video(h, q, seg_off[nseg], rotate, nprobe, img_num, ms) writes: rotation,
 *            probing, the clamp of nprobe and its limit of 128, NaN frames and the 1.0 start value are that function's, and a
 *            video id outside [0, img_num) fails with CVTMI_EINVAL (nothing is written).
 *   Totals   total[s][v] = the fold t = +0.0f; for f ascending: t = t + ms[f][v], every step one fp32 round-to-nearest add (no
 *            fma, no reassociation).  A segment without frames has +0.0 everywhere.  total may be NULL; otherwise it is
 *            [nseg][img_num], written in full and never read.
 *   Result   score[nseg][k] / video[nseg][k]: what cvtmi_topk_select(total, nseg, img_num, k, ...) returns on those totals, bit
 *            for bit -- the k smallest (total, video) pairs ascending, ties to the smaller video id, NaN totals in that function's
 *            key order, (+inf, -1) behind the img_num-th entry.
 *   Checks   before any device work: CVTMI_EINVAL for a NULL h, seg_off, score or video, nseg < 0, seg_off[0] != 0, a decreasing
 *            seg_off, a NULL q with frames, nprobe < 1, img_num < 1, k outside 1 .. CVTMI_K_MAX; CVTMI_EUNSUPPORTED for K > 256 or
 *            more than 128 probes after the clamp.  nseg == 0 does nothing.
 *   Memory   the dense score rows exist a chunk of whole frames at a time, and with total == NULL so do the totals, a group of
 *            whole segments at a time (each group is selected before the next begins); both areas live in the leased scratch set
 *            and are bounded by "ivf_part_cap_mb" (at least one frame, one segment).  A chunk may end inside a segment: the running
 *            totals carry over and the order of the adds does not change.  The host-pointer entry stages a `total` the caller
 *            asked for in full.
 * A search like cvtmi_opq_query_video: calls on one handle run side by side.
 * cvtmi_opq_last_rank: out = { frame chunks, frames per full chunk (at most the frames there were), bytes of the score area, bytes
 * of the totals area (0 when the caller gave total) } of the handle's last ranking. */
int cvtmi_opq_rank_videos(cvtmi_opq_t h, const float *q, const int64_t *seg_off, int64_t nseg, int rotate, int nprobe, int img_num, int k,
                          float *score, int64_t *video, float *total);
int cvtmi_opq_rank_videos_dev(cvtmi_opq_t h, const float *q, const int64_t *seg_off, int64_t nseg, int rotate, int nprobe, int img_num, int k,
                              float *score, int64_t *video, float *total, void *stream);
int cvtmi_opq_last_rank(cvtmi_opq_t h, int64_t out[4]);

/* Row-level IVF search: the k nearest ENTRIES among the nprobe nearest coarse lists -- the query an index with coarseK > 1 is
 * built for, where cvtmi_opq_query_video only returns per-video minima.  Rotation and probing are cvtmi_opq_query_video's
 * (the nprobe smallest (sequential fp32 distance, list) pairs of IVFOPQ.cpp:238-260; nprobe > coarseK is clamped, more than 128
 * after the clamp fails with CVTMI_EUNSUPPORTED; a query holding a NaN probes lists 0 .. nprobe-1).  An entry of probed list l
 * scores the sum over m ascending of table[m][code[m]], the table built from the residual q - coarse[l] (IVFOPQ.cpp:273-306);
 * the score is NOT clamped at 1.0.  dist[nq][k] / ids[nq][k]: the k smallest (score, id) pairs ascending, id = id_base +
 * insertion index as cvtmi_opq_search reports it; rows short of k are padded with (+inf, -1); an entry scoring +inf is a real
 * result and precedes the padding; entries whose list id is outside [0, coarseK) never appear.  A NaN query returns NaN
 * distances and min(k, entries of its lists) distinct entries in an unspecified order.  1 <= k <= CVTMI_K_MAX, K <= 256,
 * M <= 16, fewer than 2^32 entries.  On a coarseK == 1 model the call returns what cvtmi_opq_search returns.
 * NULL pointers, nq < 0, nprobe < 1 or k out of range fail with CVTMI_EINVAL before any device work; nq == 0 does nothing.
 * The first IVF search on a handle adds a uint32 insertion-index array to the list-ordered copy (4 bytes per entry; handles
 * that only run cvtmi_opq_query_video never allocate it); like the copy it is rebuilt by the first search after an append.
 * Searches run concurrently with each other and with cvtmi_opq_query_video / cvtmi_opq_search. */
int cvtmi_opq_search_ivf(cvtmi_opq_t h, const float *q, int64_t nq, int rotate, int nprobe, int k,
                         float *dist, int64_t *ids);
int cvtmi_opq_search_ivf_dev(cvtmi_opq_t h, const float *q, int64_t nq, int rotate, int nprobe, int k,
                             float *dist, int64_t *ids, void *stream);
/* Measurement hooks.  The grid cvtmi_opq_search_ivf would run for nq queries, nprobe lists each, the longest list holding
 * longest_list rows (pure host logic: no device needed; cus = 0 assumes 256): out = { rule, probe slots per workgroup G, groups per
 * query, pieces per list, rows per piece, partial lists per query }.  rule 1 = one workgroup per query (no merge), 2 = probe slots
 * cut into groups, 3 = long lists cut into pieces as well, 4 = fewer parts than wanted because the partial lists had to fit.
 * cvtmi_opq_last_ivf_plan: the same six numbers of the handle's last IVF search, then out[6] = bytes of its partial lists and
 * out[7] = bytes the handle holds for the insertion-index array (0 until the first IVF search). */
int cvtmi_opq_ivf_plan(int64_t nq, int nprobe, int k, int64_t longest_list, int cus, int64_t out[6]);
int cvtmi_opq_last_ivf_plan(cvtmi_opq_t h, int64_t out[8]);

/* Masked IVF search: the k nearest entries of the probed lists among those a bitmap allows -- search under a filter (tenant, date
 * range, "not these videos", the ids a relational query returned) on the compressed index, the counterpart of faiss's IDSelector in
 * SearchParametersIVF and of cvtmi_flat_search_masked.  mask is uint64[mask_words].
 *   Mask     bit i & 63 of word i >> 6 allows the entry with INSERTION INDEX i -- id - id_base, the addressing of
 *            cvtmi_opq_remove_ids's remap, as removals left it.  One mask serves all nq queries of the call.
 *            mask_words >= ceil(ntotal / 64), checked under the handle's lock: fewer fails with CVTMI_EINVAL (a mask built before a
 *            cvtmi_opq_add_codes is too short, not silently wrong).  Bits at positions >= ntotal are ignored whatever they hold, and
 *            words behind ceil(ntotal / 64) are never read.  Bits of entries whose list id is outside [0, coarseK) are ignored:
 *            those entries are not in the list-ordered copy and never appear.
 *   Probing  rotation, probing and the score of an entry are cvtmi_opq_search_ivf's, bit for bit: the mask never changes which
 *            lists are probed (nprobe > coarseK is clamped, more than 128 after the clamp fails with CVTMI_EUNSUPPORTED, a query
 *            holding a NaN probes lists 0 .. nprobe-1).
 *   Result   dist[nq][k] / ids[nq][k]: the k smallest (score, id) pairs among the ALLOWED entries of the probed lists, ascending,
 *            id = id_base + insertion index, with the tie rule of cvtmi_opq_search_ivf; an allowed entry scoring +inf is a real
 *            result and precedes the padding.  With fewer than k such entries the list pads with (+inf, -1).  A NaN query returns
 *            min(k, allowed entries of its lists) distinct allowed entries with NaN distances.  An all-ones mask returns
 *            cvtmi_opq_search_ivf's lists bit for bit; an all-zero mask or an empty index pads everything.
 *   In short the result equals cvtmi_opq_search_ivf on a fresh handle of the same model that holds only the allowed entries, in
 *            their order, with the ids mapped back to the original insertion indices.
 *   Limits   those of cvtmi_opq_search_ivf: 1 <= k <= CVTMI_K_MAX, K <= 256, M <= 16, fewer than 2^32 entries.
 * Checked before any device work: what cvtmi_opq_search_ivf checks, and a NULL mask with nq > 0 or mask_words < 0 -> CVTMI_EINVAL.
 * nq == 0 does nothing.
 * Concurrency: a masked search is a search.  It takes the shared lock and a scratch set of its own -- everything derived from the
 * mask lives in that set, nothing in the handle, so threads with different masks run side by side on one handle -- and it goes
 * round again on an append between preparation and lock, as cvtmi_opq_search_ivf does.  The first masked search on a handle adds the
 * insertion-index array of the list-ordered copy like the first IVF search.  The _dev entry enqueues on `stream` and never waits for
 * the device; mask, q and the outputs are device pointers there.
 * Shards: there is no collective form.  Each rank passes the mask of its own entries and the caller merges with cvtmi_topk_merge.
 * The work: one launch brings the mask into the order of the list-ordered copy (one bit per entry, in the leased set); the scan of
 * cvtmi_opq_search_ivf then leaves a probed list BEFORE it builds the list's residual table when no row of the list is allowed --
 * under a selective mask that is most lists, and the tables are what the unmasked search spends its time on.  The grid is planned for
 * the unmasked worst case; the host never learns the mask's population. */
int cvtmi_opq_search_ivf_masked(cvtmi_opq_t h, const float *q, int64_t nq, int rotate, int nprobe, int k,
                                const uint64_t *mask, int64_t mask_words, float *dist, int64_t *ids);
int cvtmi_opq_search_ivf_masked_dev(cvtmi_opq_t h, const float *q, int64_t nq, int rotate, int nprobe, int k,
                                    const uint64_t *mask, int64_t mask_words, float *dist, int64_t *ids, void *stream);
/* The mask of a set of videos: writes all mask_words words -- the bit of every entry whose video id (the id it was added with, or its
 * insertion index where none was given) is in video_ids[nv] is set, every other bit is cleared, those at positions >= ntotal
 * included.  The set follows the rules of cvtmi_opq_remove_videos: unsorted, duplicates, foreign ids and any int32 are fine.
 * nv == 0 clears the mask.  mask_words >= ceil(ntotal / 64), else CVTMI_EINVAL; NULL h, a negative count, a NULL set with nv > 0 or a
 * NULL mask with mask_words > 0 -> CVTMI_EINVAL before any device work.
 * Non-mutating: the shared lock and a leased scratch set, like a search; the work is the mark step of cvtmi_opq_remove_videos.  The
 * _dev entry (set and mask are device pointers) runs on `stream` and waits, like cvtmi_opq_remove_videos_dev, for its set to reach
 * the host, where it is sorted (4 bytes per id), and for the sorted table to have left host memory again.
 * The caller inverts or combines masks with plain word operations.  There is no mask_ids: the caller sets bit id - id_base itself. */
int cvtmi_opq_mask_videos(cvtmi_opq_t h, const int32_t *video_ids, int64_t nv, uint64_t *mask, int64_t mask_words);
int cvtmi_opq_mask_videos_dev(cvtmi_opq_t h, const int32_t *video_ids, int64_t nv, uint64_t *mask, int64_t mask_words,
                              void *stream);
/* The handle's last masked IVF search: out = the six numbers of cvtmi_opq_ivf_plan, then out[6] = bytes of its partial lists and
 * out[7] = bytes of the mask in list order (both in the leased scratch set). */
int cvtmi_opq_last_ivf_masked(cvtmi_opq_t h, int64_t out[8]);
/* The handle's last PROFILED search ("profile" 1) that took the "scan_mfma" route: out[0] = its queries, out[1] = how many of them the
 * filter could not answer and the exact scan answered instead.  Zeros while there has been none, and after a profiled search that did not take the route.  Waits for the device. */
int cvtmi_opq_last_mfma(cvtmi_opq_t h, int64_t out[2]);
/* How a batch of nq queries would go through that route (nothing touches a device): out[0] = queries per piece, out[1] = pieces (any
 * number: they follow each other on the stream), out[2] = bytes of scratch.  A piece's lists and record regions stay within 1 GB. */
int cvtmi_opq_mfma_plan(int D, int64_t n_rows, int64_t nq, int k, int list_cap, int sample, int64_t out[3]);

/* Range search over the probed lists: for every query, EVERY entry of its nprobe nearest coarse lists whose score is under
 * `radius` -- the threshold test IVFOPQ::Query / QueryThrehold make (their cells start at 1.0 and fold with min(score, cell):
 * IVFOPQ.cpp:5, :262, :308), reported per entry where cvtmi_opq_query_video reports per video.  Probing, rotation and the score
 * of an entry are cvtmi_opq_search_ivf's (same clamp of nprobe, same limit of 128, a query holding a NaN probes lists
 * 0 .. nprobe-1; no clamp of the score).
 *   Hit      score < radius as an fp32 comparison, strict.  NaN scores never hit; a +inf score (a code byte >= K) never hits, not
 *            even for radius = +inf, which returns every entry with a finite score.  radius <= 0 is valid and yields no hits; a
 *            NaN radius fails with CVTMI_EINVAL.
 *   Order    the hits of a query come in the order of the list-ordered copy (cvtmi_opq_get_entries): list id ascending, insertion
 *            order inside a list -- whatever the probe order, the grid, the stream or the run.
 *   Outputs  lims[nq + 1] (int64): lims[0] = 0, lims[f + 1] - lims[f] = hits of query f.  For hit i of the batch dist[i] = its
 *            score, ids[i] = id_base + insertion index (the ids cvtmi_opq_search / cvtmi_opq_search_ivf report), and, where video is
 *            not NULL, video[i] = the video id the entry was added with (its insertion index where none was given).  Entries whose
 *            list id is outside [0, coarseK) never appear.  A coarseK == 1 model is one list holding everything.
 *   Capacity cap = hits the caller's arrays hold.  lims is always written in full and exactly; dist / ids / video are written only
 *            if lims[nq] <= cap and are left untouched otherwise.  cap == 0 with NULL dist / ids / video is the count-only call.
 * Host entry: CVTMI_OK after writing the results (a count-only call: after writing lims), or CVTMI_ESPACE with lims valid and the
 * arrays untouched.  Device entry: enqueues on `stream` and never waits for the device; the fill is predicated ON the device on
 * lims[nq] <= cap, the call returns CVTMI_OK and the caller reads lims[nq] after synchronising.
 * Checked before any device work: NULL h / q / lims, nq < 0, nprobe < 1, cap < 0, NULL dist or ids with cap > 0 -> CVTMI_EINVAL;
 * K > 256, M > 16 or >= 2^32 entries -> CVTMI_EUNSUPPORTED.  nq == 0 writes lims[0] = 0 and nothing else.
 * Concurrency, the list-ordered copy and its insertion indices are as for cvtmi_opq_search_ivf.
 * cvtmi_set_tuning("ivf_range_spill", C) (default 4096; no effect on results): hits a workgroup may park in the leased scratch set
 * while the sizes are not known yet; a workgroup that meets more walks its rows a second time once they are.  0 = every
 * workgroup with a hit does, a huge value = none (the area is bounded by "ivf_part_cap_mb": C shrinks to fit). */
int cvtmi_opq_range_search_ivf(cvtmi_opq_t h, const float *q, int64_t nq, int rotate, int nprobe, float radius,
                               int64_t cap, int64_t *lims, float *dist, int64_t *ids, int32_t *video);
int cvtmi_opq_range_search_ivf_dev(cvtmi_opq_t h, const float *q, int64_t nq, int rotate, int nprobe, float radius,
                                   int64_t cap, int64_t *lims, float *dist, int64_t *ids, int32_t *video, void *stream);
/* The grid of the handle's last range search: out = { rule, probe slots per workgroup G, groups per query, pieces per list, rows per
 * piece, parts (workgroups) per query, spill records per part, spill bytes }.  Rules 1-3 as cvtmi_opq_ivf_plan, except that lists are
 * cut into pieces only where G == 1; rule 4 = the spill records per part were cut down to fit "ivf_part_cap_mb". */
int cvtmi_opq_last_range_plan(cvtmi_opq_t h, int64_t out[8]);

/* Removal: drop entries from the resident index on the device (faiss remove_ids; the reference itself can only rebuild).
 *   Set      cvtmi_opq_remove_videos drops every entry whose video id is in video_ids[nv] -- the id it was added with, or its
 *            insertion index where none was ever given.  cvtmi_opq_remove_ids drops every entry whose id is in ids[n_ids] -- id_base +
 *            insertion index, what cvtmi_opq_search / _search_ivf / _range_search_ivf report.  Both sets may be unsorted, may hold
 *            duplicates and may name ids that are not in the index (ignored); any int32 is a valid video id, negative values and
 *            both extremes included.  The result never depends on the order or multiplicity of the set.
 *   Result   The kept entries close up in insertion order: kept entry number j (counting from 0 in the old order) has insertion
 *            index j afterwards and reports id_base + j.  Codes, list ids and video ids move together; entries whose list id is
 *            outside [0, coarseK) move like any other.  *removed (may be NULL) = entries dropped.  remap (may be NULL) has room for
 *            the OLD cvtmi_opq_ntotal: remap[i] = new insertion index of old entry i, or -1 if it was dropped.  cvtmi_opq_ntotal
 *            reports the new count, a later cvtmi_opq_add_codes appends behind the kept entries.
 *   renumber == 0: kept entries keep their video ids.  On a handle whose video ids were implicit the call first makes them an
 *            array (as cvtmi_opq_add_codes does for the first explicit id), so an entry keeps its old number although its
 *            insertion index changed.  renumber != 0: a kept video id v becomes v - (number of DISTINCT ids in video_ids that are
 *            smaller than v) -- the numbering IVFOPQ::IndexDatabase would have produced had the removed files never been in its
 *            list; ids of the set count whether or not they occur in the index.  cvtmi_opq_remove_ids never touches video ids,
 *            apart from making implicit ones an array when at least one entry is dropped.
 *   Equivalence  Afterwards every entry of the handle (cvtmi_opq_search, _search_sharded, _query_video, _search_ivf,
 *            _range_search_ivf, _get_entries, cvtmi_hnsw_search_adc* over it) answers exactly as a new handle of the same model and
 *            id_base would that had been given only the kept entries in their order, with the video ids as described: bit for bit,
 *            distances, ids, lims, order of the hits and list_off.  The derived copies of the rows (rotated / padded rows, the
 *            list-ordered copy) are rebuilt by the first search that needs them, as after an append.  A call that drops nothing
 *            leaves the handle, those copies included, as it was (*removed = 0, remap the identity) -- unless renumber lowers video
 *            ids, which are then rewritten in place.  A call that drops everything leaves an empty, usable index.
 *   Calling  Mutating and exclusive, like cvtmi_opq_add_codes.  NULL handle, a negative count, a NULL set with a positive count ->
 *            CVTMI_EINVAL before any device work.  All scratch is reserved before the first row moves: on CVTMI_ENOMEM the index is
 *            unchanged.  Memory is not given back; cvtmi_opq_reserve keeps its meaning.  The host entries return when the index is
 *            in its new state.  The _dev entries (set and remap are device pointers) run on `stream` and WAIT on it once for the
 *            8-byte kept count the host needs for cvtmi_opq_ntotal; cvtmi_opq_remove_videos_dev also waits for its set to reach
 *            the host, where it is sorted (4 bytes per id).
 *   Shards   On a row shard (cvtmi_opq_set_id_base) each rank removes from its own handle; id_base stays, so afterwards the ids
 *            are no longer contiguous across ranks.  There is no collective form.
 * The work is a mark (4 bytes per entry), a scan of per-tile counts and a move in chunks of "remove_chunk" rows
 * (cvtmi_opq_set_param; scratch of one chunk, never a second copy of an array); rows before the first dropped entry are not moved. */
int cvtmi_opq_remove_videos(cvtmi_opq_t h, const int32_t *video_ids, int64_t nv, int renumber, int64_t *removed, int64_t *remap);
int cvtmi_opq_remove_videos_dev(cvtmi_opq_t h, const int32_t *video_ids, int64_t nv, int renumber, int64_t *removed, int64_t *remap,
                                void *stream);
int cvtmi_opq_remove_ids(cvtmi_opq_t h, const int64_t *ids, int64_t n_ids, int64_t *removed, int64_t *remap);
int cvtmi_opq_remove_ids_dev(cvtmi_opq_t h, const int64_t *ids, int64_t n_ids, int64_t *removed, int64_t *remap, void *stream);

/* Tuning / measurement hooks (no effect on results).
 *   "splits"   row splits per query group of the scan (0 = automatic)
 *   "qtile"    queries sharing one pass over the codes: 1, 2, 4 or 8 (0 = automatic)
 *   "profile"  1 = bracket the scan kernel with HIP events on its stream
 *   "encode_variant"  PQ encode kernel: 0 = choose (default); 1 = every centroid through the reference's sub / mul / add
 *                 chain on the VALU; 2 = fp32 matrix-core filter, exact chain only for pairs it cannot separate
 *                 (K = 256, step 8 or 16, M <= 9 at step 16, 16-byte aligned rows; chosen automatically at every row count).
 *                 Same codes either way.
 *   "scan_variant"  M = 16 kernel choice: 0 row-per-lane; 1 / 2 skewed fp32 tables (512 / 1024 threads);
 *                   3 / 4 skewed 15-bit lower-bound tables, 8 queries per pass (1024 / 512 threads; 3 = default);
 *                   5 = variant 3 without checkpoints: one wave of the workgroup compacts beside the 15 that scan
 *                   (adc_scan16a; measured 7-10 % slower than 3 on 1 M rows, kept for comparison)
 *                   6 = adc_scan16h: the tables of variant 3, quantised once per query group by a preparation kernel; a
 *                   persistent grid (two workgroups per CU) walks a host-built item table (cvtmi_opq_scan_plan); candidates go
 *                   to per-workgroup areas in HBM and are selected once per (row segment, query), the filter bounds come from
 *                   a histogram of the candidates' integer sums -- ONE histogram per query for all the row segments its group
 *                   is cut into, so a segment's bound comes from the rows all of them have seen; takes any number of queries
 *                   7 = (default) the library's choice: 6 where it measured ahead (100 ... 3200 queries on a cache-resident
 *                   index: wherever the planner cuts a query group into row segments), 3 elsewhere
 *   "prerotate"   1 (default) = variants 3 / 4 stream a copy of the code rows in which row r is rotated by r & 15
 *                 bytes (the lane skew of the conflict-free table reads), kept next to the rows: +16 bytes of HBM
 *                 per row, 12 VALU instructions fewer per row in the VALU-bound scan loop; 0 = rotate in registers
 *   "tail_split"  1 (default) = with automatic splits, the query groups of the last, partly filled round of
 *                 workgroups may be split finer than the others (variants 3 / 4); 0 = one split count for all
 *   "scan_lazy"   1 (default) = variants 3 / 4 select on their integer lower bounds between checkpoints and compute exact
 *                 reference-order sums once, for the rows still held at the end; 0 = exact sums at every checkpoint
 *   "scan_share"  1 (default) = the row splits of a query publish their filter thresholds to each other (variants 3 / 4)
 *   "scan_small"  1 (default) = batches of 1 .. 128 queries (M = 16, >= 65 536 rows, k <= 128, "scan_variant" 7) take the small-batch
 *                 path: per group of 8 queries a histogram pass over a quarter of the rows fixes one global bound per query, a second
 *                 pass collects the rows below it into per-workgroup lists, one workgroup per query selects (exact fall-back inside the
 *                 kernel when a list overflows) -- four launches, rotation included, no partial lists and no merge
 *   "groups_a", "splits_b"  force that two-region shape: the first groups_a query groups use "splits" row
 *                 splits, the others splits_b (> splits); 0 = planner's choice
 *   "remove_chunk"  rows cvtmi_opq_remove_* moves at a time (0 = default, 4 194 304): the scratch of a removal holds one chunk.
 *                 Rounded UP to whole tiles of 256 rows (1 .. 256 give one tile); negative values fail with CVTMI_EINVAL
 *   "scan_mfma"   1 (default) = large batches (M = 16, K = 256, D a multiple of 32 up to 256, coarseK = 1, k <= 128, "scan_variant" 7, no forced
 *                 "qtile" / "splits") take the int8 matrix-core bound filter over a decoded copy of the rows (D + 4 bytes per row, built by
 *                 the first such search and extended after appends) and re-sum the survivors exactly; queries it cannot answer go through the
 *                 exact scan in the same call, so the results are the scan's, bit for bit; 0 = the scan
 *   "scan_mfma_min_nq", "scan_mfma_min_rows"  the smallest batch (default 512) and index (default 1 000 000 rows) that take it (>= 1)
 *   "scan_mfma_max_rows"  the largest index that takes it; negative (default) = while the copy stays within 1 GB
 *   "scan_mfma_cap"  candidate rows per query the selection accepts, 1 .. 4096 (default 4096); a query with more goes to the exact scan
 *   "scan_mfma_sample"  the threshold comes from a sample of one tile group in this many, 1 .. 3 (default 2) */
int cvtmi_opq_set_param(cvtmi_opq_t h, const char *name, int64_t value);
/* With "profile" on: MEAN duration of the scan-kernel launches recorded since the previous call
 * (the 64 most recent are kept) and the algorithmic code bytes ONE launch reads
 * (passes x rows x M, passes = ceil(nq / qtile)).  Synchronises on the profiling events only. */
int cvtmi_opq_last_scan(cvtmi_opq_t h, float *ms, int64_t *code_bytes, int *qtile, int *splits);
/* The item table "scan_variant" 6 would walk for n_rows code rows and nq queries (pure host logic: no device needed; the
 * number of workgroup slots is taken as 2 x `cus`, 0 = the current device's CU count or 256 without one).  splits > 0 forces
 * (query group, row split) blocks, 0 lets the planner choose (equal shares of the flat group x row space when the code matrix
 * is cache-resident and there are at least as many query groups as slots).  items: up to cap entries of 6 ints {query group, first
 * row / 64, rows, partial-list index inside the group, partial lists of the group (0 = unused entry), first 64-row chunk of the
 * wrap-around walk over the segment}, item i of workgroup w at [i * grid + w].  Returns the number of
 * entries (rounds * grid; nothing is written past cap) or a negative status. */
int64_t cvtmi_opq_scan_plan(int64_t n_rows, int64_t nq, int splits, int cus, int64_t *items, int64_t cap, int *grid, int *rounds,
                            int *stride);

/* Which scan form a search of nq queries (top k) over n_rows code rows of a D-dimensional model with M sub-quantisers of K codewords
 * would take under the default settings (pure host logic: no device needed; 256 CUs are assumed without one).  out[0] = 1: the
 * small-batch form (up to 128 queries); otherwise out[1] = scan variant (3 / 4 = adc_scan16q, 5 = adc_scan16a, 6 = persistent grid,
 * 0 .. 2 = the row-per-lane / fp32-table kernels), out[2] = queries per pass, out[3] = row splits, out[4] / out[5] = groups of the first
 * region and row splits of the second of a two-region plan (0 0: one region), out[6] = M when the M = 16 kernels run over padded rows
 * (M < 16), else 0.  What tests/test_scan_plan.py pins the dispatch rules of round 5 with. */
int cvtmi_opq_describe_dispatch(int D, int M, int K, int64_t n_rows, int64_t nq, int k, int out[7]);

/* The same for a flat search (metric: CVTMI_METRIC_*; pure host logic): out[0] = 1 the fp32 one-stream kernels / 2 the fp32 threshold filter
 * (round 6: any width that is a multiple of 4 up to 2048-d, >= 262 144 rows, batches from "flat_f32_tfilter_min" queries on), out[1] = the fp32 sample + matrix-core filter
 * pipeline is eligible behind them, out[2] = the uint8 sample + filter pipeline, out[3] = uint8 streaming passes of up
 * to 128 queries; all zero: the exact / row-tile kernels. */
int cvtmi_flat_describe_dispatch(int metric, int D, int64_t n_rows, int64_t nq, int k, int out[4]);

/* The status every kernel launch of the library gives a grid of x * y * z workgroups before it launches (pure host logic, nothing is
 * launched): CVTMI_OK for 1 <= x <= 0x7fffffff and 1 <= y, z <= 65535, else CVTMI_EUNSUPPORTED with the offending count in
 * cvtmi_last_error().  What tests/test_launch.py pins the rule with. */
int cvtmi_describe_launch_grid(int64_t x, int64_t y, int64_t z);

/* How the selection behind the uint8 streaming kernel would be cut for ONE pass of nq queries (1 .. 128) over n_rows rows (pure host
 * logic): out[0] = slices per query (8, 16, 32 or 64), out[1] = the most rounds of wave minima one slice spans, out[2] = the rounds the
 * kernel's per-slice tables hold.  out[1] <= out[2] wherever cvtmi_flat_describe_dispatch reports the stream (out[3]); the slice count
 * is never lowered to one that would break it.  What tests/test_flat_u8_stream_plan.py pins the rule with. */
int cvtmi_flat_describe_stream_finish(int64_t n_rows, int64_t nq, int out[3]);

/* The launch log, a debugging and testing aid: which kernels a call launched.  Per thread and off by default; while it is off a launch
 * pays one test of a thread-local pointer.  cvtmi_debug_launch_log_begin() turns the calling thread's log on and returns the number of
 * records it holds -- 0 for an outermost begin, which also empties it; begins nest, and a nested one returns the mark at which its own
 * records start.  cvtmi_debug_launch_log_end() closes the innermost begin and returns the number of records (CVTMI_EINVAL, negative,
 * without an open begin); after the outermost end the log is off and keeps its records until the thread's next begin.
 * cvtmi_debug_launch_log_read() copies records first .. first + cap - 1 (those that exist) to out and returns the number of records in
 * the log, whatever cap is.  A record: the kernel's name as the sources spell it (template arguments are not part of it), the grid, the
 * block's x and the dynamic LDS bytes of a launch that passed the grid rule, in launch order; cvtmi_describe_launch_grid notes a grid
 * it accepts the same way (block 1, no LDS).  None of the three touches a device or a stream, and other threads' launches are never
 * seen. */
typedef struct cvtmi_launch_record {
    char name[64];
    int64_t grid[3];
    int64_t block;
    int64_t lds;
} cvtmi_launch_record;
int64_t cvtmi_debug_launch_log_begin(void);
int64_t cvtmi_debug_launch_log_end(void);
int64_t cvtmi_debug_launch_log_read(int64_t first, int64_t cap, cvtmi_launch_record *out);

/* Page-locked host memory.  The host-pointer entries move their arrays through pinned staging areas (one extra host copy each way);
 * arrays that already ARE page-locked -- from here, or the caller's own hipHostMalloc / hipHostRegister -- need none: page-locked
 * queries go to the copy engine as they are, and page-locked RESULT arrays of cvtmi_opq_search are written by the kernels themselves
 * (device-visible host memory: no device copy of the lists, no copy back, the batch is not cut into pieces; tuning key
 * "opq_host_zero_copy", default 1).  10 000 queries x top-100 over 1 M rows: pageable arrays in pipelined pieces 2.7 M queries/s,
 * page-locked arrays 3.1 M, device pointers 3.3 M (round 5, profiles/r05_host_api_sweep.txt). */
int cvtmi_host_alloc(size_t bytes, void **p);
int cvtmi_host_free(void *p);

/* ---------------------------------------------------------------- top-k merge ---------------- */
/* Exchange step of a row-sharded search: merge L sorted (distance, id) lists per query
 * (in_dist / in_ids [nq][L][k], id < 0 = padding, lists ordered by ascending id range) into the
 * k smallest pairs.  Same shape as FLANN-MPI's ResultsMerger
 * (retrieval/vlindex/lib/FLANN/mpi/index.h:74-108).
 * Order of cvtmi_topk_merge, cvtmi_topk_select and cvtmi_shard_merge_topk_dev: (distance, position) with -0.0 == +0.0,
 * as std::pair<float, uint> orders them; the distances returned are the input's bits (a -0.0 stays -0.0).  NaN, which that
 * order leaves out, is ranked by its bits: sign-bit NaNs before -inf, +NaNs after +inf (0x7fffffff ties with 0x7ffffffe),
 * ties by position.  Padding: (+inf, -1). */
int cvtmi_topk_merge(const float *in_dist, const int64_t *in_ids, int64_t nq, int L, int k,
                     float *dist, int64_t *ids);
int cvtmi_topk_merge_dev(const float *in_dist, const int64_t *in_ids, int64_t nq, int L, int k,
                         float *dist, int64_t *ids, void *stream);

/* ---------------------------------------------------------------- row-sharded search --------- */
/* The north-star multi-GPU layout: the code rows are split into contiguous blocks, one per GPU, one
 * process per GPU; a search scans the local block, then ONE RCCL all-gather (xGMI) of the per-shard top-k lists and a
 * k-way merge on every rank.  The reference tree's only distributed search has this shape: FLANN-MPI's
 * mpi::Index::knnSearch (retrieval/vlindex/lib/FLANN/mpi/index.h:196-226: local knnSearch, indices += offset_,
 * boost::mpi reduce with ResultsMerger :74-108).
 *
 * A communicator spans `world` ranks, this process being `rank` on the HIP device current at creation:
 *   cvtmi_comm_unique_id   rank 0 draws the job's id (ncclGetUniqueId) and hands its CVTMI_COMM_ID_BYTES bytes to the
 *                          other ranks by any means (env, file, MPI, torch.distributed ...);
 *   cvtmi_comm_create      every rank calls it at the same time (ncclCommInitRank).  world == 1 needs no id and no RCCL;
 *   cvtmi_comm_create_custom  the same exchange over a caller-supplied all-gather instead of RCCL (an MPI job like the
 *                          reference's, or several ranks sharing one GPU in tests): fn must gather `bytes` bytes from
 *                          every rank into recv_dev in rank order, IN PLACE (send_dev == recv_dev + rank * bytes), ordered
 *                          after the work already enqueued on `stream` and complete, or enqueued on `stream`, on return;
 *                          0 = success.  All pointers are device pointers.
 * Collectives must be entered by all ranks in the same order.  A rank whose LOCAL search fails still enters the
 * all-gather, with its error code in its slot's status word, so nobody is left waiting.  What the other ranks do with the
 * status words is cvtmi_set_tuning("comm_check_status", v):
 *   2 (default)  checked on the device, behind the merge, without synchronising the stream: if any rank failed, the results
 *                of that search are overwritten with the padding pattern (+inf, -1) on EVERY rank, and every rank gets
 *                CVTMI_ECOMM from its next call on the communicator, from cvtmi_comm_status, or -- host-pointer entries,
 *                which synchronise for their copy anyway -- from the failing call itself;
 *   1            read back inside the call (one stream synchronisation per sharded search): every rank returns
 *                CVTMI_ECOMM from the failing call itself, `_dev` entries included;
 *   0            ignored: only the rank that failed returns an error.
 * Calls on one communicator are serialised like calls that change a handle (the communicator's lock is taken before the
 * handle's): drive one communicator from one thread, or issue the searches that share it in the same order on every rank. */
#define CVTMI_COMM_ID_BYTES 128
typedef int (*cvtmi_allgather_fn)(void *ctx, const void *send_dev, void *recv_dev, size_t bytes, void *stream);
int cvtmi_comm_unique_id(void *id /* [CVTMI_COMM_ID_BYTES] */);
int cvtmi_comm_create(const void *id, int rank, int world, cvtmi_comm_t *out);
/* CVTMI_ECOMM (once) if a search since the last report failed on some rank under the deferred status check, else CVTMI_OK.
 * Does not synchronise: call it after the stream of the searches in question has been synchronised. */
int cvtmi_comm_status(cvtmi_comm_t c);
int cvtmi_comm_create_custom(cvtmi_allgather_fn fn, void *ctx, int rank, int world, cvtmi_comm_t *out);
/* ONE process driving every GPU (the reference's callers are single processes: opq/src/multi_frame_index_test.cpp:32-91):
 * ncclCommInitAll over `ndev` devices (devices == NULL: 0 .. ndev - 1); comms[d] is rank d of ndev on devices[d].  Use with
 * the *_sharded_all searches below (their all-gathers leave as one ncclGroupStart / ncclGroupEnd group); each communicator is
 * destroyed with cvtmi_comm_destroy. */
int cvtmi_comm_create_all(int ndev, const int *devices, cvtmi_comm_t *comms /* [ndev] */);
int cvtmi_comm_destroy(cvtmi_comm_t c);
/* rank / world; transport: 0 none (world == 1), 1 RCCL, 2 caller-supplied; all-gathers issued so far and the bytes
 * each rank contributed to the last one.  Any pointer may be NULL. */
int cvtmi_comm_info(cvtmi_comm_t c, int *rank, int *world, int *transport, int64_t *collectives, int64_t *bytes_per_rank);
/* Bytes one rank contributes to the all-gather of an [nq][k] result (status word + fp32 + int64 fields, 16-byte aligned): the
 * size a caller-supplied transport has to stage per rank. */
int cvtmi_comm_slot_bytes(int64_t nq, int k, size_t *bytes);
/* Allocates the communicator's gather buffer (world x slot bytes) for results of up to [nq][k] ahead of the searches.  A sharded
 * search whose LOCAL part fails still enters the all-gather and fails on every rank (the status word travels in the slot); the one
 * failure that cannot be signalled that way is running out of device memory for this buffer inside a search -- the rank returns
 * CVTMI_ENOMEM before the collective and its peers wait in theirs.  Reserving up front moves that failure to a point where the
 * caller can still tell the other ranks. */
int cvtmi_comm_reserve(cvtmi_comm_t c, int64_t nq, int k);
/* Row block of `rank`: [begin, end) of n_total rows, the first n_total % world ranks own one row more. */
int cvtmi_shard_range(int64_t n_total, int rank, int world, int64_t *begin, int64_t *end);
/* cvtmi_opq_search on a row shard: `h` holds this rank's block of rows (cvtmi_opq_set_id_base = its first row), every
 * rank passes the same queries; dist / ids [nq][k] = the global result, identical on every rank and identical to a
 * single handle holding all rows. */
int cvtmi_opq_search_sharded(cvtmi_opq_t h, cvtmi_comm_t c, const float *q, int64_t nq, int rotate, int k, float *dist,
                             int64_t *ids);
int cvtmi_opq_search_sharded_dev(cvtmi_opq_t h, cvtmi_comm_t c, const float *q, int64_t nq, int rotate, int k,
                                 float *dist, int64_t *ids, void *stream);
/* The same on one process: handles[d] = the row block of device d, comms from cvtmi_comm_create_all; host pointers. */
int cvtmi_opq_search_sharded_all(cvtmi_opq_t *handles, cvtmi_comm_t *comms, int ndev, const float *q, int64_t nq, int rotate,
                                 int k, float *dist, int64_t *ids);
/* The exchange step alone, for per-shard lists produced by any search: local_dist / local_ids [nq][k] ascending
 * (distance, id) with GLOBAL ids (id < 0 = padding), ranks holding ascending id ranges.  Distances are 4-byte fields: fp32,
 * or non-negative int32 (the uint8 metric) passed as their bit patterns -- they order the same way. */
int cvtmi_shard_merge_topk_dev(cvtmi_comm_t c, const float *local_dist, const int64_t *local_ids, int64_t nq, int k,
                               float *dist, int64_t *ids, void *stream);

/* get_sort_results (opq/src/common.h:25-37): the k smallest (score, index) pairs of scores[nq][n],
 * ascending; rows short of k entries are padded with (+inf, -1).  1 <= k <= CVTMI_K_MAX.  Order as cvtmi_topk_merge above
 * (-0.0 == +0.0, NaN by its bits).  The reference returns k pairs with (0, 0) past n, and its order of NaN scores depends on
 * std::partial_sort_copy's heap: the host mirror (cvt_amd/host/IVFOPQ.cpp) asks for min(k, n) entries and runs rows that
 * hold a NaN, and k > CVTMI_K_MAX, through the reference's own operation on the host. */
int cvtmi_topk_select(const float *scores, int64_t nq, int64_t n, int k, float *dist, int64_t *ids);
int cvtmi_topk_select_dev(const float *scores, int64_t nq, int64_t n, int k, float *dist, int64_t *ids,
                          void *stream);

/* ---------------------------------------------------------------- exhaustive (flat) search -- */
/* hnswlib::BruteforceSearch<dist_t> + SpaceInterface (brute_force_search/src/brutoforce.hpp:9-136,
 * hnswlib.hpp:34-58).  Rows are D fp32 (IP, L2F) or D uint8 (L2U8). */
int cvtmi_flat_create(int metric, int D, cvtmi_flat_t *out);
int cvtmi_flat_destroy(cvtmi_flat_t h);
/* addPoint (brutoforce.hpp:43-56) for n rows; labels NULL = row numbers continuing from ntotal.
 * Labels must be unique and ascending in insertion order for the (distance, label) tie rule to
 * hold on device; the C++ BruteforceSearch mirror re-orders rows by label when they are not. */
int cvtmi_flat_add(cvtmi_flat_t h, const void *x, const int64_t *labels, int64_t n);
int cvtmi_flat_add_dev(cvtmi_flat_t h, const void *x, const int64_t *labels, int64_t n, void *stream);
int cvtmi_flat_ntotal(cvtmi_flat_t h, int64_t *n);
int cvtmi_flat_reset(cvtmi_flat_t h);
/* Removal: drop rows from the resident index on the device (BruteforceSearch::removePoint, brutoforce.hpp:58-70, for a whole set).
 *   Set      A row is dropped when the label it reports in cvtmi_flat_search is in labels[n_labels]: id_base + row on a handle with
 *            implicit labels, otherwise the label the row was added with.  The set may be unsorted, may hold duplicates and may
 *            name labels that are not in the index (ignored); any int64 is a valid label.  If several rows carry the same explicit
 *            label, all of them go.  The result never depends on the order or multiplicity of the set.
 *   Result   The kept rows close up in their old order (a stable compaction), so the device's tie rule (distance, then row) keeps
 *            meaning what it meant.  Kept rows keep their labels: on a handle with implicit labels the first call that drops
 *            something first makes the labels an array holding id_base + old row (as cvtmi_flat_add does for the first explicit
 *            label, but honouring id_base).  *removed (may be NULL) = rows dropped.  remap (may be NULL) has room for the OLD
 *            cvtmi_flat_ntotal: remap[i] = new row of old row i, or -1 if it was dropped.  cvtmi_flat_ntotal reports the new count.
 *            A later cvtmi_flat_add appends behind the kept rows; without labels it numbers its rows by position (the new row
 *            number, id_base not added), as it does on any handle with explicit labels.
 *   Equivalence  Afterwards cvtmi_flat_search, _search_dev and _search_sharded* answer bit for bit (distances and labels) as a new
 *            handle of the same metric and width would that had been given only the kept rows, in their order, with their labels,
 *            on every route a search can take.  Norms move with the rows; the score bias and the row statistics of the fp32 stream
 *            are recomputed for the kept rows (a handle whose only non-finite row was removed takes the stream / threshold-filter
 *            routes again); the operand copies of the filter routes are rebuilt by the first search that needs them.  A call that
 *            drops nothing leaves the handle as it was, those copies and the implicit labels included (*removed = 0, remap the
 *            identity).  A call that drops everything leaves an empty, usable index.
 *   Calling  Mutating and exclusive, like cvtmi_flat_add.  NULL handle, a negative count, a NULL set with a positive count ->
 *            CVTMI_EINVAL before any device work.  All scratch is reserved before the first row moves: on CVTMI_ENOMEM the index is
 *            unchanged.  Memory is not given back.  The host entry returns when the index is in its new state.  The _dev entry (set
 *            and remap are device pointers) runs on `stream` and WAITS on it once for the 8-byte kept count; on a handle with
 *            explicit labels it also waits for its set to reach the host, where it is sorted (8 bytes per label).
 *   Shards   On a row shard (cvtmi_flat_set_id_base) each rank removes from its own handle.  There is no collective form.
 * The work is a mark (a bitmap of the dropped rows), a scan of per-tile counts and a move in chunks of "remove_chunk" rows
 * (cvtmi_flat_set_param; scratch of one chunk, never a second copy of the rows); rows before the first dropped row are not moved. */
int cvtmi_flat_remove_labels(cvtmi_flat_t h, const int64_t *labels, int64_t n_labels, int64_t *removed, int64_t *remap);
int cvtmi_flat_remove_labels_dev(cvtmi_flat_t h, const int64_t *labels, int64_t n_labels, int64_t *removed, int64_t *remap, void *stream);
/* Per-handle parameters (no effect on results).
 *   "remove_chunk"     rows the move of cvtmi_flat_remove_labels works on at a time, rounded up to whole 256-row tiles;
 *                      0 (default) = the rows of 64 MB.
 *   "range_part_rows"  rows a workgroup of cvtmi_flat_range_search walks, rounded up to whole 256-row tiles; 0 (default) = the
 *                      parts that fill the device once.
 *   "range_spill"      hits C a (query, part) of cvtmi_flat_range_search may park in the leased scratch set while the sizes are not
 *                      known yet; a part that meets more walks its rows a second time once they are.  0 = every part with a hit
 *                      does; a huge value = none: C is cut down to the rows of a part and so that the area, nq x parts x C x 8
 *                      bytes, stays within 256 MB.  -1 (default) = 512.
 *   "rerank_rows_copy" 0 (default) / 1: whether cvtmi_flat_rerank may build a row-major copy of blocked fp32 rows -- a second copy
 *                      of the table in device memory against eight times the gather traffic (see cvtmi_flat_rerank).
 *   "masked_parts"     workgroups per query group of cvtmi_flat_search_masked, each walking an equal share of the allowed rows:
 *                      0 (default) = the plan for a mask that allows every row, 1 .. 1024 = that many parts. */
int cvtmi_flat_set_param(cvtmi_flat_t h, const char *name, int64_t value);
/* searchKnn (brutoforce.hpp:73-93) for nq queries: k smallest (distance, label), ascending.
 * dist is float[nq][k] for IP / L2F and int32_t[nq][k] for L2U8.  1 <= k <= CVTMI_K_MAX.  An index with fewer than k rows pads:
 * label -1, distance field 0x7f800000 -- +inf as a float, and for L2U8 the same bit pattern read as int32 (2139095040: larger than
 * any real distance, which is what lets the padded lists of row shards merge like all others).
 * Floats compare as in cvtmi_topk_select: -0.0 == +0.0, NaN by its key.  A NaN distance is a real candidate, ordered by its key: a
 * query holding a NaN returns min(k, rows) distinct rows, all with NaN distances.  (The key of a NaN with the sign bit is below -inf's,
 * and the subtractions q - x and 1 - sum negate their second operand, a NaN included: for a finite query a row holding a +NaN leads
 * the list.) */
int cvtmi_flat_search(cvtmi_flat_t h, const void *q, int64_t nq, int k, void *dist, int64_t *labels);
int cvtmi_flat_search_dev(cvtmi_flat_t h, const void *q, int64_t nq, int k, void *dist, int64_t *labels,
                          void *stream);
/* Range search: for every query, EVERY row of the index whose distance is under `radius` -- the test the reference's retrieval loop
 * makes behind a top-5 (hnsw_sifts_retrieval/makeSearch.cpp:52-61), without the 5.  q holds nq rows of the index's own type.
 *   Distance the one cvtmi_flat_search reports for that (query, row), bit for bit: IP is 1 - sum in the 4-lane order; L2F sums in 8
 *            lanes for D % 16 == 0, in 4 lanes for D % 4 == 0 and in the scalar loop otherwise; L2U8 is the exact int32 sum over
 *            D / 4 * 4 bytes (the D % 4 tail is dropped, as L2SqrI does).  dist holds 4-byte fields: float for IP and L2F, int32 for
 *            L2U8.
 *   Hit      distance < radius as real numbers, strict.  radius is a double, so that an integer radius above 2^24 is exact for L2U8.
 *            fp32 metrics: the host turns radius into the smallest float t >= radius and the kernels test d < t in fp32 -- the same
 *            predicate.  L2U8: the host turns radius into T = ceil(radius) clamped to [0, 2^31-1] (2^31 or more: every row) and the
 *            kernels test d < T in integers.  NaN distances never hit; a +inf distance never hits, not even for radius = +inf.
 *            radius = -inf or radius <= 0 yields no hit for the L2 metrics; for IP it yields whatever is below it (IP distances
 *            can be negative, -inf included).  A NaN radius fails with CVTMI_EINVAL.
 *   Order    the hits of a query come in ascending row order -- insertion order, as left by removals -- whatever the grid, the
 *            stream or the run: no atomic decides where a hit lands.
 *   Labels   each hit carries the label cvtmi_flat_search would report: id_base + row while labels are implicit, otherwise the
 *            stored label.  Duplicate explicit labels simply repeat.
 *   Outputs  lims[nq + 1] (int64): lims[0] = 0, lims[f + 1] - lims[f] = hits of query f.  For hit i of the batch dist[i] = its
 *            distance and labels[i] = its label.
 *   Capacity cap = hits the caller's arrays hold.  lims is always written in full and exactly; dist / labels are written only if
 *            lims[nq] <= cap and are left untouched otherwise.  cap == 0 with NULL dist / labels is the count-only call.
 * Host entry: CVTMI_OK after writing the results (a count-only call: after writing lims), or CVTMI_ESPACE with lims valid and the
 * arrays untouched.  Device entry: enqueues on `stream` and never waits for the device; the fill is predicated ON the device on
 * lims[nq] <= cap, the call returns CVTMI_OK and the caller reads lims[nq] after synchronising.
 * Checked before any device work: NULL h / q / lims, nq < 0, cap < 0, NULL dist or labels with cap > 0, a NaN radius ->
 * CVTMI_EINVAL; nq > INT32_MAX -> CVTMI_EUNSUPPORTED.  nq == 0 writes lims[0] = 0 and nothing else; an empty index writes all-zero
 * lims.
 * Concurrency: a range search is a search.  It runs side by side with the other searches of the handle, each on a scratch set of its
 * own, and waits behind cvtmi_flat_add / _remove_labels / _reset like them.
 * Shards: there is no sharded form.  Each rank answers for its own rows, and cvtmi_flat_set_id_base makes the labels global; the
 * caller concatenates.
 * The rows are read once as the handle holds them (no second copy): one workgroup per (group of queries, part of the rows) counts
 * the hits and parks up to C per (query, part) ("range_spill"), two scans turn the counts into lims, and a fill places the parked
 * hits; only parts with more than C hits are walked a second time ("range_part_rows", "range_spill": cvtmi_flat_set_param). */
int cvtmi_flat_range_search(cvtmi_flat_t h, const void *q, int64_t nq, double radius, int64_t cap,
                            int64_t *lims, void *dist, int64_t *labels);
int cvtmi_flat_range_search_dev(cvtmi_flat_t h, const void *q, int64_t nq, double radius, int64_t cap,
                                int64_t *lims, void *dist, int64_t *labels, void *stream);
/* The plan of the handle's last range search: out = { queries per workgroup QT, parts per query group, rows per part, spill records
 * per (query, part) C, spill bytes, kernel form }.  Forms: 0 fp32 row-major rows, queries in LDS; 1 fp32 blocked rows, queries in
 * SGPRs; 2 uint8 single bytes; 3 uint8 16-byte pieces; 4 uint8 16-byte pieces with the handle's norms.  A count-only call plans C = 0. */
int cvtmi_flat_last_range_plan(cvtmi_flat_t h, int64_t out[6]);
/* Rerank: the exact top k among the candidate rows the caller names -- the exact finish behind any candidate generator (the IVF or
 * exhaustive ADC searches, HNSW-ADC, the lists of a shard, a metadata filter), the counterpart of faiss's IndexRefineFlat.  q holds nq
 * rows of the index's own type, cand is int64[nq][R].
 *   Candidates  entry j of query f names row cand[f][j] - cand_base; it is valid when cand_base <= cand[f][j] < cand_base + ntotal,
 *            evaluated without signed overflow (INT64_MIN, INT64_MAX and any cand_base are safe).  Everything else is skipped
 *            silently: the -1 padding of the searches, ids another shard owns.  A row named several times counts once; the result
 *            never depends on the order or the multiplicity of a query's candidates.
 *   Distance the one cvtmi_flat_search reports for that (query, row), bit for bit: IP is 1 - sum in the 4-lane order; L2F sums in 8
 *            lanes for D % 16 == 0, in 4 lanes for D % 4 == 0 and in the scalar loop otherwise; L2U8 is the exact int32 sum over
 *            D / 4 * 4 bytes.  dist holds 4-byte fields: float for IP and L2F, int32 for L2U8.
 *   Order    ascending (distance, row), the device tie rule of cvtmi_flat_search.  Floats compare as in cvtmi_topk_select:
 *            -0.0 == +0.0, NaN by its key.  A NaN distance is a real candidate: a query holding a NaN returns min(k, distinct valid
 *            rows) distinct rows, all with NaN distances, in an unspecified order.  Short lists pad with label -1 and distance field
 *            0x7f800000, as cvtmi_flat_search pads.
 *   Labels   what cvtmi_flat_search would report for the row: id_base + row while labels are implicit, otherwise the stored label.
 *   In short for NaN-free data, query f gets exactly what cvtmi_flat_search(k) returns on a fresh handle that holds only f's distinct
 *            valid rows, in ascending row order, with the labels they report.
 *   Limits   1 <= k <= CVTMI_K_MAX, 1 <= R <= CVTMI_RERANK_MAX; k may exceed R (the list then pads).  ntotal >= 2^32 fails with
 *            CVTMI_EUNSUPPORTED.
 * Checked before any device work: NULL h, or NULL q / cand / dist / labels with nq > 0, nq < 0, k or R out of range -> CVTMI_EINVAL.
 * nq == 0 does nothing; an empty index pads everything.
 * Concurrency: a rerank is a search.  It takes the shared lock and a scratch set of its own, runs beside the other searches of the
 * handle and waits behind cvtmi_flat_add / _remove_labels / _reset like them.  The `_dev` entry enqueues on `stream` and never waits
 * for the device (but for the one call that builds the copy below).
 * One launch: a workgroup per query scores the valid candidates out of LDS tiles of their rows, sorts the (distance, row) pairs in LDS,
 * drops equal neighbours and writes k of them; no [nq][R] array passes through device memory.
 * Row source.  fp32 rows with D % 4 == 0 live in 64-row blocks: a gathered row costs EIGHT times its bytes there (16 useful bytes of
 * every 128-byte line).  cvtmi_flat_set_param(h, "rerank_rows_copy", v):
 *   0 (default)  read the row-major copy of the rows only if the handle already has a current one (the fp32 threshold filter builds
 *                it: "flat_f32_rows_copy"); otherwise gather from the blocked rows;
 *   1            the first rerank that needs it builds or extends that copy, under the exclusive lock, before it takes its shared
 *                lock.  The price is a SECOND copy of the table in device memory, against eight times the gather traffic without
 *                it.  If the allocation fails the blocked rows are read.
 * Every source gives the same bits.  No effect on uint8 rows or on fp32 rows with D % 4 != 0: those are row-major as they are. */
#define CVTMI_RERANK_MAX 4096
int cvtmi_flat_rerank(cvtmi_flat_t h, const void *q, int64_t nq, const int64_t *cand, int R, int64_t cand_base,
                      int k, void *dist, int64_t *labels);
int cvtmi_flat_rerank_dev(cvtmi_flat_t h, const void *q, int64_t nq, const int64_t *cand, int R, int64_t cand_base,
                          int k, void *dist, int64_t *labels, void *stream);
/* The handle's last rerank: out = { row source, lanes per distance (1 / 4 / 8; 0 for uint8), workgroups, LDS bytes per workgroup }.
 * Row source: 0 = row-major primary rows (uint8, or fp32 with D % 4 != 0), 1 = blocked rows, 2 = the row-major copy. */
int cvtmi_flat_last_rerank(cvtmi_flat_t h, int64_t out[4]);
/* ADC candidates, exact finish: R candidates per query from the OPQ index -- what cvtmi_opq_search_ivf(nprobe, R) returns for
 * nprobe >= 1, what cvtmi_opq_search(R) returns for nprobe == 0 (which needs coarseK == 1) -- reranked against `flat` as
 * cvtmi_flat_rerank does, with cand_base = the OPQ handle's id_base and the RAW queries (rotate only steers the scan).  dist and
 * labels receive the exact distances and the FLAT index's labels: the result equals that composition of the two public calls, bit for
 * bit.  The padding of a short scan list is never a candidate (with an OPQ id_base in [-ntotal, -1] the entry whose id is -1 reads as
 * padding).  The candidate lists stay in the scratch set the OPQ handle leases and never reach the host.
 * Requirements, checked before any device work, else CVTMI_EINVAL: flat is IP or L2F, its D is the model's, both hold the same number
 * of rows and live on the same device, 1 <= k <= R <= CVTMI_K_MAX, nprobe >= 0, nprobe == 0 only with coarseK == 1, no NULL handle,
 * nq >= 0, and no NULL q / dist / labels with nq > 0.  nq == 0 does nothing.
 * The call holds the OPQ handle's shared lock first and takes the flat handle's inside it. */
int cvtmi_opq_search_refine(cvtmi_opq_t h, cvtmi_flat_t flat, const float *q, int64_t nq, int rotate, int nprobe,
                            int k, int R, float *dist, int64_t *labels);
int cvtmi_opq_search_refine_dev(cvtmi_opq_t h, cvtmi_flat_t flat, const float *q, int64_t nq, int rotate, int nprobe,
                                int k, int R, float *dist, int64_t *labels, void *stream);
/* Masked search: the k nearest rows among those a bitmap allows -- search under a filter (tenant, date range, not yet seen, the ids a
 * relational query returned), the counterpart of faiss's IDSelector and of hnswlib's searchKnn(query, k, BaseFilterFunctor *).  q holds
 * nq rows of the index's own type, mask is uint64[mask_words].
 *   Mask     bit r & 63 of word r >> 6 allows ROW r.  A row is a position, in insertion order, as removals left it -- the addressing of
 *            cvtmi_flat_rerank's candidates with cand_base = 0.  One mask serves all nq queries of the call.
 *            mask_words >= ceil(ntotal / 64), checked under the handle's lock: fewer fails with CVTMI_EINVAL (a mask built before a
 *            cvtmi_flat_add is too short, not silently wrong).  Bits at positions >= ntotal are ignored whatever they hold, and words
 *            behind ceil(ntotal / 64) are never read: a caller may pass all-ones words.
 *   Distance the one cvtmi_flat_search reports for that (query, row), bit for bit: IP is 1 - sum in the 4-lane order; L2F sums in 8
 *            lanes for D % 16 == 0, in 4 lanes for D % 4 == 0 and in the scalar loop otherwise; L2U8 is the exact int32 sum over
 *            D / 4 * 4 bytes.  dist holds 4-byte fields: float for IP and L2F, int32 for L2U8.
 *   Order    ascending (distance, row), the device tie rule of cvtmi_flat_search.  Floats compare as in cvtmi_topk_select:
 *            -0.0 == +0.0, NaN by its key.  A NaN distance is a real candidate, ordered by its key: a query holding a NaN returns
 *            min(k, allowed rows) distinct allowed rows, all with NaN distances.  With fewer than k allowed rows the list pads with
 *            label -1 and distance field 0x7f800000, as cvtmi_flat_search pads.
 *   Labels   what cvtmi_flat_search would report for the row: id_base + row while labels are implicit, otherwise the stored label.
 *   In short for NaN-free data the result equals cvtmi_flat_search(k) on a fresh handle that holds only the allowed rows, in their
 *            order, with the labels they report.
 *   Limits   1 <= k <= CVTMI_K_MAX; nq <= INT32_MAX (more fails with CVTMI_EUNSUPPORTED); ntotal < 2^32.
 * Checked before any device work: NULL h, or NULL q / mask / dist / labels with nq > 0, nq < 0, mask_words < 0, k out of range ->
 * CVTMI_EINVAL.  nq == 0 does nothing; an empty index or an all-zero mask pads everything.
 * Concurrency: a masked search is a search.  It takes the shared lock and a scratch set of its own, runs beside the other searches of
 * the handle and waits behind cvtmi_flat_add / _remove_labels / _reset like them.  The `_dev` entry enqueues on `stream` and never waits
 * for the device; mask, queries and outputs are device pointers there.
 * Shards: there is no collective form.  Each rank passes the mask of its own rows (cvtmi_flat_set_id_base makes the labels global)
 * and the caller merges the lists with cvtmi_topk_merge.
 * One form for every density: the mask is compacted on the device into an ascending list of the allowed rows (per-tile popcounts, a
 * scan, no atomics; 4 bytes per row at most, in the leased scratch set; the host never learns its length), and the exact kernels of
 * cvtmi_flat_search walk the LIST, one lane per allowed row.  The parts of a query group divide the list, not the rows, so the work
 * is even however the mask clusters; the grid is planned for the worst case ("masked_parts": cvtmi_flat_set_param).  An all-ones
 * mask reads what the exact search reads plus 4 bytes per row; a sparse mask reads the allowed rows only. */
int cvtmi_flat_search_masked(cvtmi_flat_t h, const void *q, int64_t nq, int k, const uint64_t *mask, int64_t mask_words,
                             void *dist, int64_t *labels);
int cvtmi_flat_search_masked_dev(cvtmi_flat_t h, const void *q, int64_t nq, int k, const uint64_t *mask, int64_t mask_words,
                                 void *dist, int64_t *labels, void *stream);
/* The mask of a label set: writes all mask_words words -- the bit of every row whose reported label (id_base + row while labels are
 * implicit, the stored label otherwise) is in labels[n_labels] is set, every other bit is cleared, those at positions >= ntotal
 * included.  The set follows the rules of cvtmi_flat_remove_labels: unsorted, duplicates, foreign labels and any int64 are fine, and
 * several rows sharing a label are all set.  n_labels == 0 clears the mask.  mask_words >= ceil(ntotal / 64), else CVTMI_EINVAL; NULL
 * h, a negative count, a NULL set with n_labels > 0 or a NULL mask with mask_words > 0 -> CVTMI_EINVAL before any device work.
 * Non-mutating: the shared lock and a leased scratch set, like a search; the work is the mark step of cvtmi_flat_remove_labels.  The
 * _dev entry (set and mask are device pointers) runs on `stream`; on a handle with explicit labels it waits for its set to reach the
 * host, where it is sorted (8 bytes per label).  The caller inverts or combines masks with plain word operations. */
int cvtmi_flat_mask_labels(cvtmi_flat_t h, const int64_t *labels, int64_t n_labels, uint64_t *mask, int64_t mask_words);
int cvtmi_flat_mask_labels_dev(cvtmi_flat_t h, const int64_t *labels, int64_t n_labels, uint64_t *mask, int64_t mask_words,
                               void *stream);
/* The handle's last masked search: out = { queries per workgroup, parts per query group, bytes of the row list, kernel form }.
 * Forms: 0 fp32 row-major rows with queries in LDS; 1 fp32 blocked rows with queries in SGPRs; 2 uint8 single bytes; 3 uint8 16-byte
 * pieces. */
int cvtmi_flat_last_masked(cvtmi_flat_t h, int64_t out[4]);
/* Measurement hook: how the last search was answered -- *filtered = 0 the exact kernels; 1 the sample + matrix-core filter
 * pipeline (fp32 metrics, 32 <= D <= 128, D % 16 == 0, >= 131072 rows: exact search of a leading sample, bf16 matrix-core
 * products decide which other rows need an exact distance); 2 the fp32 stream (D in {32, 64, 96, 128, 192, 256}, >= 32768 rows:
 * one pass over the rows scores them on the bf16 matrix cores, the k-and-a-few candidates get exact distances; queries its
 * error bound does not cover are re-run by the exact kernels inside the same call) -- same results every way -- and the largest
 * candidate list of the pipeline.  cvtmi_set_tuning("flat_variant", 1) allows the exact kernels only, 2 prefers the pipeline;
 * cvtmi_set_tuning("flat_f32_stream", 0 / 1 / 2) = never / choose / wherever it applies. */
int cvtmi_flat_last_search(cvtmi_flat_t h, int *filtered, int64_t *max_candidates);
/* Measurement hook: *redone = how many queries of the last search on h the exact kernels answered because the fp32 threshold
 * filter, the uint8 threshold filter or the fp32 stream flagged them (bound not covering the query, sample not filled, lists over);
 * 0 for a search those paths answered whole or did not take; -1 when cvtmi_set_tuning("flat_count_redo", 1) was not in force. */
int cvtmi_flat_last_redo(cvtmi_flat_t h, int64_t *redone);
/* Row shards of an exhaustive index (BruteforceSearch<dist_t>::searchKnn over rows split across GPUs: config 3's 5 GB of
 * uint8 rows shard like config 4's codes).  Rows added without labels report label = id_base + row; the sharded searches
 * return the global k best -- float distances, or the int32 distances of the uint8 metric (same 4-byte fields) -- identical
 * on every rank and to one handle holding all rows.  See cvtmi_opq_search_sharded* for the communicator rules. */
int cvtmi_flat_set_id_base(cvtmi_flat_t h, int64_t base);
int cvtmi_flat_search_sharded(cvtmi_flat_t h, cvtmi_comm_t c, const void *q, int64_t nq, int k, void *dist, int64_t *labels);
int cvtmi_flat_search_sharded_dev(cvtmi_flat_t h, cvtmi_comm_t c, const void *q, int64_t nq, int k, void *dist, int64_t *labels,
                                  void *stream);
int cvtmi_flat_search_sharded_all(cvtmi_flat_t *handles, cvtmi_comm_t *comms, int ndev, const void *q, int64_t nq, int k,
                                  void *dist, int64_t *labels);

/* ---------------------------------------------------------------- int8 scalar quantisation -- */
/* Per-dimension min / (max - min) over (optionally L2-normalised) rows: what
 * faiss::IndexScalarQuantizer(d, QT_8bit).train leaves in sq.trained
 * (scalar_quantization/train/src/sq_train.cpp:84-103).  x is not modified. */
int cvtmi_sq8_train(const float *x, int64_t n, int d, int l2norm, float *vmin, float *vdiff);
int cvtmi_sq8_train_dev(const float *x, int64_t n, int d, int l2norm, float *vmin, float *vdiff,
                        void *stream);
/* Int8Quan::Int8Encode arithmetic (scalar_quantization/scalar_quantization/int8_quan.cc:72-94)
 * over n rows; with l2norm == 1 each row of x is L2-normalised IN PLACE first (:46-56), as the
 * reference does to its caller's buffer; l2norm == 2 encodes the normalised rows but leaves x as it
 * was (same codes, 4 d bytes of write traffic per row less: for callers that do not read x again). */
int cvtmi_sq8_encode(const float *vmin, const float *vdiff, int d, float *x, int64_t n, int l2norm,
                     uint8_t *codes);
int cvtmi_sq8_encode_dev(const float *vmin, const float *vdiff, int d, float *x, int64_t n, int l2norm,
                         uint8_t *codes, void *stream);
/* Int8Quan::Int8Decode(std::string&) arithmetic (int8_quan.cc:117-132) over n rows. */
int cvtmi_sq8_decode(const float *vmin, const float *vdiff, int d, const uint8_t *codes, int64_t n,
                     float *x);
int cvtmi_sq8_decode_dev(const float *vmin, const float *vdiff, int d, const uint8_t *codes, int64_t n,
                         float *x, void *stream);
/* Int8Quan::Int8Decode(uint8_t*) and Int8DecodeFaiss (int8_quan.cc:96-115) do NOT use the formula above: they call
 * faiss::ScalarQuantizer::decode.  faiss is a dependency that is not vendored in the reference (pinned 1.5.3 by its build notes);
 * its published QT_8bit codec is fp32 throughout: xi = (code + 0.5f) / 255.0f, x = vmin + xi * vdiff, product and sum rounded
 * separately (a faiss built with FMA contraction could fuse the two; this is the ISO evaluation).  About a third of the floats
 * differ from cvtmi_sq8_decode's by one ulp. */
int cvtmi_sq8_decode_faiss(const float *vmin, const float *vdiff, int d, const uint8_t *codes, int64_t n,
                           float *x);
int cvtmi_sq8_decode_faiss_dev(const float *vmin, const float *vdiff, int d, const uint8_t *codes, int64_t n,
                               float *x, void *stream);

/* ---------------------------------------------------------------- PCA projection ------------- */
/* cvtk::PCAUtils::reduceDim (pca_train_project/pca_online/pca_utils.cc:25-35; same arithmetic in
 * project/pca_dimension.h:47-58): y = cv::PCA::project(x) = (x - mean) * vectors^T, then with l2norm != 0 every
 * row divided by float(max(1e-12, sqrt(y . y))).  mean [din], vectors [dout][din] row-major (the "mean" and
 * "vectors" matrices of the model file), x [n][din], y [n][dout].  din % 4 == 0, dout <= 256.
 * cv::PCA::project is OpenCV (3.2 / 3.3 per the reference's comments), absent here: PARITY UNPINNED.  The
 * projection is evaluated as the k-ascending fp32 fused multiply-add chain of (x[k] - mean[k]) * vectors[j][k]
 * (OpenCV's own gemm accumulates in double or calls a BLAS, depending on its build); tests hold it within
 * 2e-6 absolute of the double-accumulated value on unit-norm outputs. */
int cvtmi_pca_project(const float *mean, const float *vectors, int din, int dout, const float *x, int64_t n,
                      int l2norm, float *y);
int cvtmi_pca_project_dev(const float *mean, const float *vectors, int din, int dout, const float *x,
                          int64_t n, int l2norm, float *y, void *stream);

/* ---------------------------------------------------------------- PCA training --------------- */
/* The reference trains its models with cv::PCA(data, noArray(), DATA_AS_ROW, dout) (pca_train_project/train/src/
 * train.cpp, opencv_utils.hpp:27-39).  OpenCV is absent here: PARITY UNPINNED.  What runs is this arithmetic:
 *   1. mean[j] = float(sum_r (double)x[r][j] / n): column sums in double over a fixed partition of the rows,
 *      the partials combined in a fixed order (no atomics);
 *   2. d[r][j] = x[r][j] - mean[j], rounded to fp32 (OpenCV centres a CV_32F matrix in fp32);
 *   3. cov[i][j] = (sum_r (double)d[r][i] * (double)d[r][j]) / n  (OpenCV's COVAR_NORMAL | COVAR_ROWS | COVAR_SCALE:
 *      divided by n, not n - 1).  Every product of two floats is exact in double; only the double additions round.
 *      Only the tiles on and below the diagonal are computed and mirrored, so cov is bitwise symmetric; rows are
 *      split into blocks that depend on (n, din) alone and the partials are summed in block order, so the same
 *      input gives the same bits on every call, host entry and device entry alike.  Two passes: the mean first,
 *      then the centred product (the one-pass X^T X - n mu mu^T loses (|mu| / sigma)^2 of its relative accuracy);
 *   4. eigendecomposition of cov in double on the device by rocSOLVER's dsyevd, loaded at run time (librocsolver.so.0:
 *      processes that never train never load it; CVTMI_EUNSUPPORTED if it cannot be loaded); a solve that does
 *      not converge is CVTMI_EHIP;
 *   5. the dout largest eigenvalues in descending order; each eigenvector's sign makes its largest-magnitude
 *      component positive, the lowest index winning ties (OpenCV's signs are arbitrary); values = float(lambda),
 *      vectors = float(v).
 * Limits: din % 4 == 0, 4 <= din <= 2048, 1 <= dout <= min(din, n); anything else is CVTMI_EINVAL.  OpenCV quietly
 * shortens the model when n < din (its "scrambled" covariance); these entries reject that instead.
 * Host entries copy x to the device once: CVTMI_ENOMEM when x, the partial sums, the covariance and the solver's
 * workspace do not fit in the device's free memory.  _dev entries take device pointers and return after the
 * work on `stream` is complete. */
/* mean [din] fp32; cov [din][din] float64, exactly symmetric */
int cvtmi_pca_covariance(const float *x, int64_t n, int din, float *mean, double *cov);
int cvtmi_pca_covariance_dev(const float *x, int64_t n, int din, float *mean, double *cov, void *stream);
/* mean [din], vectors [dout][din], values [dout]: the three matrices of the model file ("mean" 1 x din,
 * "vectors" dout x din, "values" dout x 1) */
int cvtmi_pca_train(const float *x, int64_t n, int din, int dout, float *mean, float *vectors, float *values);
int cvtmi_pca_train_dev(const float *x, int64_t n, int din, int dout, float *mean, float *vectors, float *values,
                        void *stream);

/* ---------------------------------------------------------------- codebook training ---------- */
/* TrainPQ::CoarseQuan / ProdQuan (opq/train_codebook/train_PQ_codebook.cpp:150-244).  The reference calls
 * yael's kmeans(d, n, k, niter = 0, v, nt, seed = 1, redo = 1, ...), which is not vendored: PARITY UNPINNED.
 * What runs here is a fully specified Lloyd iteration (the tests hold it bit-exact against the CPU checker):
 * k distinct seed rows drawn with splitmix64(seed); nearest-centroid assignment with the arithmetic of
 * IVFOPQ::Add (sequential fp32 distance, strict '<'); centroid = float(double sum in ascending row order /
 * count), empty clusters keep their centroid; stops when a pass changes no assignment or after niter updates
 * (niter = 0: until convergence, at most 100).  x: [n] rows, ld floats apart, d <= 512 columns used.
 * centroids [k][d]; assign [n] may be NULL; iters_done may be NULL. */
int cvtmi_kmeans(const float *x, int64_t n, int d, int k, int niter, uint64_t seed, float *centroids,
                 int32_t *assign, int *iters_done);
int cvtmi_kmeans_dev(const float *x, int64_t ld, int64_t n, int d, int k, int niter, uint64_t seed,
                     float *centroids, int32_t *assign, int *iters_done, void *stream);
/* TrainPQ::IFVPQ (:144-148) on already permuted rows (LoadFeatureSample :77-82): coarse k-means on the whole
 * vectors, residuals x - coarse[assign] (:190-197), one k-means per sub-space on the residual columns
 * (:214-233), every k-means with the same seed as in the reference.  coarse [coarseK][D], books [M][K][D/M]
 * = the SaveCodebook / LoadModel layout (:283-287, IVFOPQ.cpp:75-95). */
int cvtmi_opq_train(const float *x, int64_t n, int D, int coarseK, int M, int K, int niter, uint64_t seed,
                    float *coarse, float *books);
int cvtmi_opq_train_dev(const float *x, int64_t n, int D, int coarseK, int M, int K, int niter, uint64_t seed,
                        float *coarse, float *books, void *stream);
/* OPQ rotation learning (optional): the dense D x D rotation the a-R GEMM applies, learned from a sample instead of
 * handed in.  NOT in the reference (opq/ only permutes dimensions, reorder_ IVFOPQ.cpp:424-439, and reads the permutation from a
 * file): self-specified, held bit for bit to the oracle's orc_opq_learn_rotation.  Non-parametric alternation (Ge et al. 2013):
 * R = I; `outer` times { Xr = X R^T (the fp32 MFMA GEMM); per sub-space k-means of Xr (cvtmi_kmeans: K centroids, niter, seed);
 * Y = the rows' reconstructions; C = X^T Y in double (rows in blocks of 1024, ascending); R = V U^T for C = U S V^T (orthogonal
 * Procrustes, one-sided Jacobi on the host) }; books = the k-means of the final Xr.  outer = 0 returns the identity and plain PQ
 * codebooks.  R [D][D] row-major and books [M][K][D/M] feed cvtmi_opq_create (coarseK = 1, a zero centroid: the exhaustive
 * configuration).  D in {32, 64, 96, 128}. */
int cvtmi_opq_learn_rotation(const float *x, int64_t n, int D, int M, int K, int outer, int niter, uint64_t seed, float *R,
                             float *books);
int cvtmi_opq_learn_rotation_dev(const float *x, int64_t n, int D, int M, int K, int outer, int niter, uint64_t seed, float *R,
                                 float *books, void *stream);

/* ---------------------------------------------------------------- HNSW search ---------------- */
/* hnswlib::HierarchicalNSW<float> (hnsw_sifts_retrieval/hnswlib/hnswalg.h), search side.
 * cvtmi_hnsw_load  = loadIndex (:522-581): takes the bytes of a file written by the reference's saveIndex
 *   (:491-519) for D-dimensional fp32 vectors and moves vectors, level-0 links, upper-level links and labels
 *   to HBM.  metric: CVTMI_METRIC_IP (InnerProductSpace) or CVTMI_METRIC_L2F (L2Space).
 * cvtmi_hnsw_search = setEf(ef) + searchKnn(query, k) (:688-729) for nq queries at once, one wave per query:
 *   dist / labels [nq][k] in ascending (distance, label) order -- the order the reference's result queue
 *   yields back to front --, padded with (0, -1) when the graph returns fewer than k.  Distances use the
 *   summation order of the reference's distance functions and both priority queues replay libstdc++'s
 *   push_heap / pop_heap (the reference compares by distance only, so heap mechanics decide ties): labels
 *   and distances are bit-identical to the reference's on the same graph.  k, ef <= 1024.
 * Graphs are loaded from the reference's files or built on the GPU (cvtmi_hnsw_build, below), and grow on the GPU
 * (cvtmi_hnsw_add). */
int cvtmi_hnsw_load(const void *file, int64_t bytes, int metric, int D, cvtmi_hnsw_t *out);
int cvtmi_hnsw_destroy(cvtmi_hnsw_t h);
int64_t cvtmi_hnsw_ntotal(cvtmi_hnsw_t h);
int cvtmi_hnsw_search(cvtmi_hnsw_t h, const float *q, int64_t nq, int k, int ef, float *dist, int64_t *labels);
int cvtmi_hnsw_search_dev(cvtmi_hnsw_t h, const float *q, int64_t nq, int k, int ef, float *dist, int64_t *labels,
                          void *stream);
/* Graph construction on the GPU, batch-synchronous.  Rows x [n][D] fp32 get internal ids 0 .. n-1 and the labels
 * `labels` [n] (NULL = the row number).  The graph is the reference's HierarchicalNSW(space, n, M, ef_construction) after one
 * addPoint per row (hnswalg.h:584-684), except for one rule: rows are inserted in BATCHES of consecutive rows, every row of a
 * batch searches the graph as the earlier batches left it (rows of one batch do not see each other), and then the batch's back
 * links are applied, for each target node in increasing source id, each exactly as mutuallyConnectNewElement applies it.
 *   - header as the reference's constructor sets it: max_elements = n, maxM = M, maxM0 = 2 M, mult = 1 / ln M,
 *     ef_construction = max(ef_construction, M); the level of row i is the i-th draw of std::default_random_engine(100)
 *     through getRandomLevel (:143-148), so levels equal those of every sequential build of the same n rows;
 *   - batches: at most max_batch rows (max_batch = 1: the reference's sequential insertion, and the file cvtmi_hnsw_save
 *     writes is byte-identical to the reference's saveIndex), and at most 1/32 of the rows already inserted (at least one);
 *     max_batch = 0 caps batches at 8192 rows.  A row whose level exceeds the current top level ends its batch;
 *   - distances and queue mechanics as in cvtmi_hnsw_search: the graph is a pure function of (rows, labels, metric, M,
 *     ef_construction, max_batch), whatever the stream, device or timing.  Rows must be finite.
 * The result is an ordinary handle: every cvtmi_hnsw_search* entry works on it.  Arguments are checked before any device work;
 * invalid ones (n < 1, D < 1, unknown metric, M < 2, ef_construction < 1, max_batch < 0, NULL x / out, and M > 32: a level-0
 * list of 2 M links is one wave) return CVTMI_EINVAL with *out = NULL; max(ef_construction, M) > 1024 or D > 4096:
 * CVTMI_EUNSUPPORTED.  cvtmi_hnsw_build_dev takes device rows and labels, runs on `stream` and returns when the graph is
 * complete. */
int cvtmi_hnsw_build(const float *x, int64_t n, int D, int metric, int M, int ef_construction, const uint64_t *labels, int max_batch,
                     cvtmi_hnsw_t *out);
int cvtmi_hnsw_build_dev(const float *x, int64_t n, int D, int metric, int M, int ef_construction, const uint64_t *labels,
                         int max_batch, cvtmi_hnsw_t *out, void *stream);
/* saveIndex (:491-519) of a built or loaded graph into buf[cap]; *bytes = the file's size (buf = NULL: only the size).  Slots
 * between cur_element_count and max_elements (a loaded file's spare capacity) are written as zeros, where the reference writes
 * whatever its allocation held: load -> save reproduces a file with max_elements == cur_element_count byte for byte. */
int cvtmi_hnsw_save(cvtmi_hnsw_t h, void *buf, int64_t cap, int64_t *bytes);
/* measurement hook: with cvtmi_set_tuning("hnsw_build_phases", 1), ms[5] = device milliseconds of the last build spent in
 * traversal, selection and back links (bucketing included), its batch count, and host milliseconds (level draw, schedule) */
int cvtmi_hnsw_build_phases(double *ms);
/* Incremental insertion: HierarchicalNSW(space, location) + addPoint, the way a saved index is grown.  Appends
 * the rows x [m][D] as internal ids ntotal .. ntotal + m - 1 with the labels `labels` [m] (NULL = the internal id), on any handle,
 * built or loaded.  The result is the graph after one reference addPoint per row (hnswalg.h:584-684) except for the batch rule of
 * cvtmi_hnsw_build: batches of consecutive rows, a row sees the graph as the batches before its own left it, back links per target
 * in increasing (level, source).
 *   Schedule   the build's, continued: the first batch of a call starts at the current ntotal; a batch holds
 *              clamp(rows in the graph / "hnsw_build_frac", 1, cap) rows, cap = max_batch, or "hnsw_build_cap" for max_batch = 0; a
 *              row that raises the top level ends its batch; on an empty graph (a loaded file with cur_element_count == 0) row 0
 *              seeds alone.  max_batch = 1 is the reference's sequential addPoint.  cvtmi_hnsw_build(x[:n0], b) followed by
 *              cvtmi_hnsw_add(x[n0:], b) gives the bytes of cvtmi_hnsw_build(x, b) whenever n0 is a batch boundary of the latter.
 *   Parameters M, maxM, maxM0, mult and ef_construction are the header's (a loaded file may have maxM0 != 2 M).  maxM0 > 64,
 *              maxM > maxM0, M outside 1..maxM, ef_construction outside 1..1024, D > 4096, mult outside 0..16 or
 *              ntotal + m > 2^31 - 1: CVTMI_EUNSUPPORTED before any device work.
 *   Levels     the handle owns the level stream: std::default_random_engine(100) and the number of draws taken from it.  After
 *              cvtmi_hnsw_build of n rows that number is n, so build + add draws what a longer build draws.  After cvtmi_hnsw_load
 *              it is 0: the reference's loadIndex leaves level_generator_ at its initialiser, rows added after a load repeat the
 *              draws from the start, and so do ours -- load + add writes the reference's file.  cvtmi_hnsw_level_draws reads the
 *              number, cvtmi_hnsw_set_level_draws repositions the stream (re-seed, then that many draws: O(draws) on the host).
 *   Capacity   the header's max_elements becomes max(max_elements, ntotal + m); cvtmi_hnsw_reserve raises it and never lowers it;
 *              cvtmi_hnsw_save keeps writing zeros for the unused slots.  Device storage follows the rows, not that number: it
 *              grows geometrically and keeps its contents.
 *   Cost       per call, beyond the insertions: two arrays of ntotal + m words and one memset of them, and the copy of whatever
 *              buffer had to grow.
 *   Calling    mutating and exclusive, like cvtmi_flat_add: it waits for the searches in flight on the handle, searches issued later
 *              wait for it and plan their scratch (visited bits, the ntotal-entry queues of a masked search) for the grown graph.
 *              m == 0 does nothing.  NULL h, NULL x with m > 0, m < 0, max_batch < 0 -> CVTMI_EINVAL before any device work.  Rows
 *              must be finite.  All storage is reserved before the graph changes: on CVTMI_ENOMEM the handle is unchanged.  If the
 *              kernels report a candidate-queue overflow (or a launch fails) mid-call some link lists are already rewritten: the
 *              handle is marked broken and every entry but cvtmi_hnsw_destroy fails with a message from then on.  The `_dev` entry
 *              takes device rows and labels, runs on `stream` and returns when the graph is complete.
 *   Deleted    on a handle with deleted nodes (cvtmi_hnsw_mark_deleted, below) the new rows are linked to live nodes only, by
 *              current hnswlib's rule; the new rows arrive live and the marks are kept.
 *   Not here   replacing the vector of an existing label (a repeated label gets a second node, as in the reference), reusing the
 *              slot of a deleted node; the PQ codes cvtmi_hnsw_search_adc needs -- append them with cvtmi_opq_add_codes; until then the ADC
 *              entries answer CVTMI_EINVAL for the row-count mismatch.
 * cvtmi_hnsw_last_add: out = { first internal id of the last call that added rows, its batches (a seed row counts as one), its
 * largest batch, max_elements afterwards }. */
int cvtmi_hnsw_add(cvtmi_hnsw_t h, const float *x, int64_t m, const uint64_t *labels, int max_batch);
int cvtmi_hnsw_add_dev(cvtmi_hnsw_t h, const float *x, int64_t m, const uint64_t *labels, int max_batch, void *stream);
int cvtmi_hnsw_reserve(cvtmi_hnsw_t h, int64_t max_elements);
int cvtmi_hnsw_level_draws(cvtmi_hnsw_t h, int64_t *draws);
int cvtmi_hnsw_set_level_draws(cvtmi_hnsw_t h, int64_t draws);
int cvtmi_hnsw_last_add(cvtmi_hnsw_t h, int64_t out[4]);
/* HNSW over OPQ-compressed vectors (BASELINE config 5; not in the reference, whose HNSW holds fp32 vectors):
 * the same traversal over the same graph, but a node's distance is the ADC sum of the query's tables over the
 * node's PQ code (IVFOPQ.cpp:273-291 tables, :302-306 sum) -- M bytes gathered per neighbour instead of 4 D.
 * `opq` must hold exactly one code row per graph node, appended in the graph's internal-id order (the order
 * the vectors were added to the graph), with a coarseK == 1 model of the graph's dimension; rotate as in
 * cvtmi_opq_search.  Output as cvtmi_hnsw_search, distances = ADC distances. */
int cvtmi_hnsw_search_adc(cvtmi_hnsw_t h, cvtmi_opq_t opq, const float *q, int64_t nq, int rotate, int k, int ef,
                          float *dist, int64_t *labels);
int cvtmi_hnsw_search_adc_dev(cvtmi_hnsw_t h, cvtmi_opq_t opq, const float *q, int64_t nq, int rotate, int k, int ef,
                              float *dist, int64_t *labels, void *stream);
/* cvtmi_hnsw_search_adc followed by an exact re-rank: the ADC traversal returns its `rerank` best nodes (k <= rerank <= 1024), their
 * fp32 distances to the RAW query are computed from the graph's own vectors in the summation order of the reference's distance
 * functions, and the k smallest come back (k <= CVTMI_K_MAX); nodes with equal exact distances keep their ADC order.  16-byte codes steer
 * the traversal, full vectors are only touched for `rerank` nodes per query: the recall of the fp32 graph at a fraction of its
 * gather traffic. */
int cvtmi_hnsw_search_adc_rerank(cvtmi_hnsw_t h, cvtmi_opq_t opq, const float *q, int64_t nq, int rotate, int k, int ef,
                                 int rerank, float *dist, int64_t *labels);
int cvtmi_hnsw_search_adc_rerank_dev(cvtmi_hnsw_t h, cvtmi_opq_t opq, const float *q, int64_t nq, int rotate, int k, int ef,
                                     int rerank, float *dist, int64_t *labels, void *stream);
/* Masked search: the graph traversal of the entry of the same name, with a bitmap deciding which nodes may be RESULTS -- search under
 * a filter (tenant, date range, the ids a relational query returned), hnswlib's searchKnn(query, k, BaseFilterFunctor *), the
 * counterpart of cvtmi_flat_search_masked and cvtmi_opq_search_ivf_masked.  mask is uint64[mask_words].
 *   Mask     bit i & 63 of word i >> 6 allows NODE i.  A node is an internal id: the insertion order, the row order of
 *            cvtmi_hnsw_build, the order in which cvtmi_hnsw_search_adc expects code rows.  One mask serves all nq queries of the call.
 *            mask_words >= ceil(ntotal / 64), fewer fails with CVTMI_EINVAL.  Bits at positions >= ntotal are ignored whatever they
 *            hold, and words behind ceil(ntotal / 64) are never read: a caller may pass all-ones words.
 *   Rule     hnswlib's searchBaseLayerST with isIdAllowed: the mask decides what enters the result queue, never what is traversed.
 *            The greedy descent through the upper levels ignores it.  On level 0 every accepted neighbour joins the candidate queue,
 *            allowed or not; only allowed ones join the result queue; and the walk stops on "the nearest candidate is farther than
 *            the worst result" only once the result queue holds ef = max(ef, k) entries -- until then it ends on an empty candidate
 *            queue alone.  Distances, heap tie mechanics, result order, NaN handling, label reporting and the k, ef <= 1024 limits
 *            are those of the unmasked entry: it is the same kernel.
 *   Results  an all-ones mask returns what the unmasked entry returns, bit for bit.  With ef >= the number of allowed nodes reachable
 *            from the node the descent ends on, the result is exactly those nodes in ascending (distance, label).  With fewer than k
 *            allowed nodes found the list pads with (0, -1), as cvtmi_hnsw_search pads on a graph smaller than k; an all-zero mask
 *            pads everything (after walking the whole component: sparse masks cost a long walk).
 *   Scratch  the candidate queue of a masked traversal is not bounded by ef: every slot gets room for ntotal entries, so it cannot
 *            overflow, and the number of concurrent traversals is lowered until the scratch stays under 8 GiB (at least one).
 * Checked before any device work: NULL h, or NULL q / mask / dist / labels with nq > 0, nq < 0, mask_words < 0, a short mask ->
 * CVTMI_EINVAL; k / ef / rerank out of range answer as in the unmasked entry.  nq == 0 does nothing.
 * Concurrency: a search like the others -- a leased scratch set (the host-pointer entries stage the mask through it beside the
 * queries), concurrent with every other search on the handle.  The `_dev` entries take device q / mask / outputs and enqueue on
 * `stream`. */
int cvtmi_hnsw_search_masked(cvtmi_hnsw_t h, const float *q, int64_t nq, int k, int ef, const uint64_t *mask, int64_t mask_words,
                             float *dist, int64_t *labels);
int cvtmi_hnsw_search_masked_dev(cvtmi_hnsw_t h, const float *q, int64_t nq, int k, int ef, const uint64_t *mask, int64_t mask_words,
                                 float *dist, int64_t *labels, void *stream);
int cvtmi_hnsw_search_adc_masked(cvtmi_hnsw_t h, cvtmi_opq_t opq, const float *q, int64_t nq, int rotate, int k, int ef,
                                 const uint64_t *mask, int64_t mask_words, float *dist, int64_t *labels);
int cvtmi_hnsw_search_adc_masked_dev(cvtmi_hnsw_t h, cvtmi_opq_t opq, const float *q, int64_t nq, int rotate, int k, int ef,
                                     const uint64_t *mask, int64_t mask_words, float *dist, int64_t *labels, void *stream);
/* the ADC traversal runs under the mask with a result list of `rerank` nodes; the re-rank sees allowed nodes only */
int cvtmi_hnsw_search_adc_rerank_masked(cvtmi_hnsw_t h, cvtmi_opq_t opq, const float *q, int64_t nq, int rotate, int k, int ef,
                                        int rerank, const uint64_t *mask, int64_t mask_words, float *dist, int64_t *labels);
int cvtmi_hnsw_search_adc_rerank_masked_dev(cvtmi_hnsw_t h, cvtmi_opq_t opq, const float *q, int64_t nq, int rotate, int k, int ef,
                                            int rerank, const uint64_t *mask, int64_t mask_words, float *dist, int64_t *labels,
                                            void *stream);
/* The mask of a label set: writes all mask_words words -- the bit of every node whose label is in labels[n_labels] is set, every
 * other bit is cleared, those at positions >= ntotal included.  The set follows the rules of cvtmi_flat_mask_labels: unsorted,
 * duplicates and foreign labels are fine, labels compare as 64-bit patterns, nodes sharing a label are all set; n_labels == 0 clears
 * the mask.  mask_words >= ceil(ntotal / 64), else CVTMI_EINVAL; NULL h, a negative count, a NULL set with n_labels > 0 or a NULL
 * mask with mask_words > 0 -> CVTMI_EINVAL before any device work.  The work is the mark step of cvtmi_flat_remove_labels over the
 * graph's labels, on a leased scratch set.  The _dev entry (set and mask are device pointers) runs on `stream` and waits for its set
 * to reach the host, where it is sorted (8 bytes per label). */
int cvtmi_hnsw_mask_labels(cvtmi_hnsw_t h, const int64_t *labels, int64_t n_labels, uint64_t *mask, int64_t mask_words);
int cvtmi_hnsw_mask_labels_dev(cvtmi_hnsw_t h, const int64_t *labels, int64_t n_labels, uint64_t *mask, int64_t mask_words,
                               void *stream);
/* The handle's last masked search: out = { slots (concurrent traversals), candidate-queue capacity per slot in entries (LDS + HBM),
 * scratch bytes reserved (visited bits + queues), form: 0 fp32, 1 ADC with tables in the scratch, 2 ADC with tables in LDS }. */
int cvtmi_hnsw_last_masked(cvtmi_hnsw_t h, int64_t out[4]);
/* Deletion: current hnswlib's markDelete / unmarkDelete over a label set.  A deleted node stays in the graph and is
 * still walked through, but it is never a result and no new row links to it; its slot, vector and (in an OPQ index beside the graph)
 * code row stay where they are.  The state is a bitmap of ceil(ntotal / 64) words on the device beside the labels.
 *   Set      every node that carries one of labels[n_labels] is marked (unmarked).  The set follows cvtmi_hnsw_mask_labels: unsorted,
 *            duplicates and foreign labels are fine, labels compare as 64-bit patterns, nodes sharing a label all change.  `changed`
 *            (may be NULL; host memory in both forms) receives the number of nodes whose state actually changed: marking a marked
 *            node changes nothing.  n_labels == 0 does nothing.
 *   Search   with at least one deleted node, EVERY search entry of the handle runs the masked kernel under "not deleted" (the unmasked
 *            entries) or "allowed and not deleted" (the _masked entries; the caller's mask is only read), with the scratch plan of a
 *            masked search -- a candidate queue of ntotal entries per traversal, see cvtmi_hnsw_search_masked -- and
 *            cvtmi_hnsw_last_masked reports it.  The result is, bit for bit, that of the _masked entry on the unmarked graph under that
 *            mask.  With no deleted node (none marked yet, or all unmarked again) the handle answers through the unmasked kernels.
 *   Add      cvtmi_hnsw_add on a handle with deleted nodes: the greedy descent walks deleted nodes like live ones; on a level every
 *            accepted neighbour is traversed and only live ones enter the result queue, the walk stops on "nearest candidate farther
 *            than the worst result" only on a full result queue, and a deleted entry point is pushed into each level's result queue
 *            after the walk (hnswlib's addPoint).  Selection and back links are unchanged.
 *   File     cvtmi_hnsw_save writes hnswlib's mark: bit 16 of the node's level-0 count word (DELETE_MARK 0x01 in byte 2, the count in
 *            the low 16 bits); cvtmi_hnsw_load reads it, and refuses a count word with any higher bit.  A graph without deleted nodes
 *            writes and reads the bytes it always did.
 *   Calling  mark / unmark are mutating and exclusive, like cvtmi_hnsw_add.  NULL h, n_labels < 0, NULL labels with n_labels > 0 ->
 *            CVTMI_EINVAL before any device work, the handle stays usable.  The _dev forms take a device label set (it comes down to
 *            be sorted, as in cvtmi_hnsw_mask_labels_dev) and run on `stream`; they return when the state has changed.
 * cvtmi_hnsw_deleted_count: the deleted nodes.  cvtmi_hnsw_get_deleted: the bitmap into mask[mask_words], bit i & 63 of word i >> 6 =
 * node i is deleted, every bit at a position >= ntotal zero; mask_words >= ceil(ntotal / 64), else CVTMI_EINVAL (the checks of
 * cvtmi_hnsw_mask_labels); the _dev form writes device memory on `stream`.
 * Not here: reusing a deleted node's slot (hnswlib's replace_deleted / updatePoint), compacting the graph, sharded forms. */
int cvtmi_hnsw_mark_deleted(cvtmi_hnsw_t h, const int64_t *labels, int64_t n_labels, int64_t *changed);
int cvtmi_hnsw_mark_deleted_dev(cvtmi_hnsw_t h, const int64_t *labels, int64_t n_labels, int64_t *changed, void *stream);
int cvtmi_hnsw_unmark_deleted(cvtmi_hnsw_t h, const int64_t *labels, int64_t n_labels, int64_t *changed);
int cvtmi_hnsw_unmark_deleted_dev(cvtmi_hnsw_t h, const int64_t *labels, int64_t n_labels, int64_t *changed, void *stream);
int cvtmi_hnsw_deleted_count(cvtmi_hnsw_t h, int64_t *count);
int cvtmi_hnsw_get_deleted(cvtmi_hnsw_t h, uint64_t *mask, int64_t mask_words);
int cvtmi_hnsw_get_deleted_dev(cvtmi_hnsw_t h, uint64_t *mask, int64_t mask_words, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CVTMI_H */
