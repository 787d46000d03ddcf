/*
 * lmi_hip.h — C-ABI of liblmi_hip.so, the MI355X (gfx950) implementation of the
 * LMI search hot path of TerkaSlan/sisap23-laion-challenge-learned-index.
 *
 * The reference has no native code and no FFI: its hot path is Python calling
 * torch / sklearn / numpy.  Each entry point below replaces
 * one piece of that Python path; the reference file:line it stands in for is
 * cited per function.  The ctypes binding a maintainer adds on the reference
 * side is in INTEGRATION.md; this repo's own binding is li/_lib.py.
 *
 * Conventions (all entry points):
 *   - plain pointers and sizes only; "device" pointers are HIP device memory
 *     owned by the caller; "host" pointers are ordinary host memory;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream);
 *     device entry points are asynchronous on that stream, never allocate and
 *     never synchronise (workspace is passed in), so they can be captured in
 *     a hipGraph;
 *   - return 0 (LMI_OK) or an LMI_E_* code; lmi_last_error() gives text
 *     (thread-local).  No C++ exception crosses the ABI.
 *   - results are deterministic: no float atomics in any reduction; every
 *     top-k list is ordered by (distance, position) ascending, which is the
 *     reference's order on tie-free inputs (LearnedIndex.py:170, :91).
 */
#ifndef LMI_HIP_H
#define LMI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LMI_ABI_VERSION 13

/* ---- status codes ---------------------------------------------------- */
#define LMI_OK 0
#define LMI_E_INVALID 1001     /* bad argument (shape, null pointer, range) */
#define LMI_E_UNSUPPORTED 1002 /* valid request this build does not implement */
#define LMI_E_WORKSPACE 1003   /* workspace too small */
#define LMI_E_HIP 1004         /* a HIP runtime call failed */

/* bits of the device status word written by lmi_bucket_topk */
#define LMI_STATUS_QUERY_NOT_F16 1 /* qmode=LMI_Q_F16 but a query is not fp16-exact */
#define LMI_STATUS_INTERNAL 2      /* a list entry held an out-of-range row (a scan bug): the
                                      entry was dropped instead of read out of bounds */

/* ---- element types / modes ------------------------------------------ */
#define LMI_F32 0
#define LMI_F16 1
/* 8-bit storage (an addition: LMI_ABI_VERSION does not change): corpus is
 * [n_rows][d_pad] int8 codes and inv_norm the codes' own 1/sqrt(sum c^2)
 * (lmi_quantize_rows_i8 writes both).  Lossy: the lists are the exact top-k of
 * the quantised distances.  Only lmi_bucket_topk and lmi_bucket_topk_masked /
 * _tagged take it, with qmode LMI_Q_I8, 1 <= k <= LMI_MAX_K and d_pad <= 992. */
#define LMI_I8 2

#define LMI_ROUTER_TOPR 0   /* softmax + classes sorted by probability (predict_proba) */
#define LMI_ROUTER_ARGMAX 1 /* argmax of logits (predict)                               */

#define LMI_Q_F16 0 /* queries are fp16-representable: exact fp16 MFMA path        */
#define LMI_Q_F32 1 /* general queries: exact-fp32 MFMA path (16x the MFMA time)   */
/* The queries of an LMI_I8 index: quantised inside the call by the rule of
 * lmi_quantize_rows_i8, int8 x int8 products summed exactly in int32
 * (v_mfma_i32_32x32x32_i8).  LMI_I8 and LMI_Q_I8 come together: one without the
 * other is LMI_E_INVALID. */
#define LMI_Q_I8 2
/* ABI 6, a flag OR-ed into qmode (lmi_bucket_topk / lmi_bucket_topk_f64*, k <=
 * LMI_MAX_K): the lists of probes r >= 1 are needed only below the pair's
 * round-0 k-th distance -- the reference's thresholded rounds compare every
 * later-round object with the running k-th distance, which is never larger
 * than round 0's (LearnedIndex.py:71-75, utils.py:23; the merges only lower
 * it, :86-97) -- so the scan starts every (q, r >= 1) pair with the bound of
 * pair (q, 0) (plus 2 eps in the float64 mode) and its list holds the top-k of
 * the objects at or under that bound.  Only for the replay with thresholds
 * (use_threshold); the lists of r = 0 are unchanged. */
#define LMI_Q_SEED_ROUND0 0x100
/* ABI 7, flags OR-ed into qmode (lmi_bucket_topk / lmi_bucket_topk_f64*, k <=
 * LMI_MAX_K): run only some phases of the call, so that a caller can overlap
 * one batch's plan with another batch's scan (a stream of batches, each with
 * its own workspace, lists and status word).  The phases, in order: PLAN (the
 * queries' fragments and norms, the output prefill, the tile plan, the seed
 * map, the tail split, the bound reset), SCAN (the scan kernel), MERGE (the
 * chunk merge; in lmi_bucket_topk_f64* also the float64 refinement).  No phase
 * flag = all three.  The phase calls of one batch take the same arguments and
 * run in phase order on streams that order them. */
#define LMI_Q_PHASE_PLAN 0x200
#define LMI_Q_PHASE_SCAN 0x400
#define LMI_Q_PHASE_MERGE 0x800
/* ABI 10 (lmi_bucket_topk_f64g only): the float64 refinement as a phase of
 * its own, after the ranks' k-th distances were exchanged. */
#define LMI_Q_PHASE_REFINE 0x1000
/* The scan in two launches over one tile queue (lmi_scan_set_join_workgroups,
 * j > 0): extra workgroups of the SCAN phase's kernel, launched on their own
 * -- on any stream, before, beside or after the SCAN phase's launch, after the
 * PLAN phase and before the MERGE phase.  The scan's workgroups never wait for
 * one another and share only the queue counters and the pairs' bounds, so the
 * late workers take whatever tiles are left and the merged lists are those of
 * one launch.  Not part of "no phase flag = all three"; a no-op with j = 0. */
#define LMI_Q_PHASE_SCAN_JOIN 0x2000

#define LMI_MAX_LAYERS 8
#define LMI_MAX_K 16          /* largest k of one scan pass (and of K3 / the float32 ABI 1 lists) */
#define LMI_MAX_K_PASSES 1024 /* lmi_bucket_topk: k > LMI_MAX_K lists (the wide path, below) */
#define LMI_MAX_K_F64 240     /* lmi_bucket_topk_f64: k + 5 guard entries in <= 256-entry lists */

/* ---- router ----------------------------------------------------------- */
/* A torch nn.Sequential of nn.Linear layers with ReLU between consecutive
 * layers (reference model.py:18-83, class Model; the CLI's default 'MLP' is
 * 96->128->ReLU->C, README/north_star's 'MLP-5' is 96->256->128->C). */
typedef struct lmi_mlp_desc {
    int32_t n_layers;                 /* number of nn.Linear layers, 1..LMI_MAX_LAYERS */
    int32_t dims[LMI_MAX_LAYERS + 1]; /* dims[0]=input width ... dims[n_layers]=n_classes */
    const float* W[LMI_MAX_LAYERS];   /* device, torch layout [out][in] row-major (y = x W^T + b) */
    const float* b[LMI_MAX_LAYERS];   /* device, [out] */
} lmi_mlp_desc;

/* Widest layer (input, hidden or classes) lmi_router evaluates; it equals
 * LMI_TRAIN_MAX_DIM, so every stack lmi_mlp_train_steps trains also routes. */
#define LMI_ROUTER_MAX_DIM 1024

/* Router inference on nq rows of x (device, [nq][dims[0]] f32, row stride ldx).
 * Any Linear/ReLU stack of 1..LMI_MAX_LAYERS layers whose widths lie in
 * 1..LMI_ROUTER_MAX_DIM, whatever the alignment of its weights (an MFMA kernel
 * when the input and hidden widths are multiples of 16 and the weights 16-B
 * aligned, an FMA-chain kernel otherwise).  A wider layer returns
 * LMI_E_UNSUPPORTED before any device call.
 * mode LMI_ROUTER_TOPR — replaces NeuralNetwork.predict_proba
 *   (reference model.py:214-229 = softmax(dim=1) then topk(C)):
 *   classes_out (device, [nq][R] int32) = classes by descending probability,
 *   ties by ascending class index; probs_out (device, [nq][R] f32, nullable) =
 *   the matching softmax probabilities.  1 <= R <= n_classes.
 * mode LMI_ROUTER_ARGMAX — replaces NeuralNetwork.predict (model.py:201-212,
 *   used for object labels at LearnedIndex.py:240): R must be 1,
 *   classes_out[q] = argmax of logits (lowest index on ties); probs_out unused. */
int lmi_router(const float* x, int32_t nq, int32_t ldx, const lmi_mlp_desc* mlp,
               int32_t R, int32_t mode, int32_t* classes_out, float* probs_out,
               void* stream);

/* Adaptive probing: LMI_ROUTER_TOPR followed by a probability-mass stop rule,
 * in the same launch (an addition: LMI_ABI_VERSION does not change).
 *   p_r   = the float32 softmax probability of pick r (what probs_out receives)
 *   S_0   = 0,  S_{r+1} = fl32(S_r + p_r), summed in ascending r
 *   probe r is kept  <=>  r < min_probes  or  S_r < stop_mass
 * The kept probes are a prefix of the R picks.  classes_out[q][r] is the TOPR
 * class where kept and LMI_PROBE_NONE where dropped; every consumer of the
 * classes (the scan's plan, both replays) treats a class outside [0, C) as a
 * probe with no bucket: its list is (+inf, -1) and its round merges nothing.
 * probs_out (nullable) holds the TOPR probabilities of every r, kept or not,
 * so a caller can recompute the rule exactly; n_probes_out (device, [nq]
 * int32, nullable) the number of probes kept.
 * 0 < stop_mass <= 1 (a NaN is invalid); 1 <= min_probes, a value above R
 * means R; everything else as for lmi_router.  stop_mass = 1 with
 * min_probes = R keeps every probe.  Asynchronous, no allocation, capturable. */
#define LMI_PROBE_NONE (-1)   /* class of a probe the stop rule dropped */
int lmi_router_stop(const float* x, int32_t nq, int32_t ldx, const lmi_mlp_desc* mlp,
                    int32_t R, float stop_mass, int32_t min_probes,
                    int32_t* classes_out, float* probs_out /*nullable*/,
                    int32_t* n_probes_out /*nullable, [nq]*/, void* stream);

/* ---- bucket-sorted corpus (one shard) -------------------------------- */
/* Rows of the search corpus (reference: data_search, clip768 'emb',
 * search.py:79-84) ordered by bucket label, stable in row order, i.e. the
 * order in which DataFrame.groupby('category') visits them
 * (LearnedIndex.py:143-145).  A shard of a G-GPU index holds a contiguous
 * slice of every bucket; `gpos` maps a local row to its global position in
 * the unsharded order (the tie-break key; within a bucket it is monotone in
 * the reference's g.index order).  Inside a bucket the rows may be grouped by
 * sub-cluster as long as the rows of each chunk are in ascending gpos. */
typedef struct lmi_index_desc {
    const void* corpus;        /* device, [n_rows][d_pad] of dtype, zero-padded past d */
    int32_t dtype;             /* LMI_F16 (values fp16-exact) or LMI_F32 */
    int32_t d;                 /* logical vector width (768 for clip768) */
    int32_t d_pad;             /* row stride in elements, multiple of 32 */
    int64_t n_rows;            /* rows held by this shard */
    const float* inv_norm;     /* device [n_rows]: 1/||y|| with sklearn's zero rule */
    const int32_t* gpos;       /* device [n_rows]: global position of each row */
    int32_t n_buckets;         /* C (classes of the router) */
    const int64_t* bucket_off; /* device [C+1]: rows of bucket c are [off[c], off[c+1]) */
    int32_t chunk_rows;        /* rows per scan chunk (work unit along the corpus) */
    const int32_t* chunk_first;/* device [C+1]: prefix of ceil(n_c/chunk_rows) (lmi_plan_chunks) */
    int32_t n_chunks;          /* chunk_first[C] */
    int32_t max_chunks;        /* max_c ceil(n_c/chunk_rows) */
    /* ABI 2: optional (NULL = none) device [n_chunks][d_pad] f32, the unit
     * centroid of each chunk.  When a bucket's rows are laid out by
     * sub-cluster (every chunk one sub-cluster; rows inside a chunk still in
     * ascending gpos), the scan visits each (query, probe)'s nearest chunk
     * first, so its pruning bound starts near the final k-th distance.
     * Results do not depend on it. */
    const float* chunk_centroid;
    /* ABI 6: optional (NULL = none) device [n_rows][d_pad] float64: the rows
     * as the caller gave them when they are float64 (a float64 data_search
     * DataFrame).  The scan still reads `corpus` (the rows rounded to
     * float32); the float64 mode (lmi_bucket_topk_f64*) recomputes its band
     * and fallback distances from these rows, i.e. on the values sklearn sees
     * (utils.py:11, :19).  Results of the float32 mode do not depend on it. */
    const double* corpus64;
    /* ABI 9: optional (NULL = none) device [n_rows][d_pad] float32: the rows
     * as the caller gave them when they are float32 but NOT fp16-exact.
     * `corpus` then holds each row L2-normalised and rounded to fp16 (dtype
     * LMI_F16, inv_norm = 1/||that fp16 row||), and the search is exact in two
     * steps (lmi_bucket_topk, _f64, _f64q, k <= LMI_MAX_K; queries as given,
     * float32, rounded inside the call the same way):
     *   1. an fp16 scan on the rounded rows and queries gives each (query,
     *      probe) an upper bound B of its approximate k-th distance d~_k (the
     *      k-th of a per-bucket sample -- each bucket's first chunk_rows rows
     *      -- for k <= 10, the 15th of sampled chunk lists for k <= 15, the
     *      k-th of a whole scan for k = 16); every row's rounded distance
     *      lies within eps_x of its exact one, eps_x = lmi_split_eps(d)
     *      (1.0e-3 at d = 768), so the exact top-k lies within d~_k + 2 eps_x;
     *   2. a collect scan gathers every row under B + 2 eps_x; of those (they
     *      hold the k smallest d~, hence d~_k), the rows within d~_k + 2 eps_x
     *      get their exact distances in float64 from these rows (or from
     *      corpus64 when set, for the float64 mode) and the query, sorted by
     *      (distance, position) -- rounded to float32 first for the float32
     *      mode -- and the first k kept; a pair with more candidates than the
     *      collect buffer holds is scanned whole in float64.
     * Needs d_pad == 768 (the fp16 scan's width).  ABI 11: k <= 10 takes the
     * phase flags (LMI_Q_PHASE_PLAN: the rounded queries and both scans'
     * plans; SCAN: the sample scan, the bound and the collect scan; MERGE:
     * step 3), so a stream of batches runs one batch's re-score beside the
     * next one's scans; other k, no phase flags.
     * ABI 10: the float32 arithmetic re-scores in the reference's own float32
     * operation order -- sklearn's normalize (numpy einsum row norms, a
     * division) and OpenBLAS sgemm's summation order for the (round, bucket)
     * group's shape (oracle blas32_*: numpy 2.2 / OpenBLAS 0.3.29 SkylakeX,
     * the libraries the reference runs on in the build container) -- so its
     * float32 distances are the reference's bit for bit; shapes whose BLAS
     * path is not restated (a group of one query or one row, groups of at
     * most 3 x 3) keep the exact value rounded to float32 (ABI 11: the
     * whole-shard fallback follows the reference's order too). */
    const float* corpus32;
    /* ABI 10: optional (NULL = this shard's own) device [n_buckets] int64: the
     * rows of every bucket in the whole index (a G-GPU index's shards hold
     * slices): the shape of the reference's per-bucket product. */
    const int64_t* bucket_rows;
    /* ABI 11: optional (NULL = normalised per candidate inside the call)
     * device [n_rows][d_pad] float32: corpus32's rows divided by their
     * float32 norms as sklearn's normalize computes them (numpy einsum row
     * norms, zero rule, IEEE division; lmi_split_normalize fills it).  The
     * normalised row depends on the row alone, so the float32 re-score then
     * runs only the product's summation chains per candidate.  Same float32
     * distances, bit for bit, with or without it. */
    const float* corpus32n;
} lmi_index_desc;

/* Host helper: fills chunk_first_out[C+1] from host bucket offsets and returns
 * max chunks per bucket (>= 0) or a negative LMI_E_* code. */
int32_t lmi_plan_chunks(const int64_t* bucket_off_host, int32_t n_buckets,
                        int32_t chunk_rows, int32_t* chunk_first_out);

/* Bytes of workspace lmi_bucket_topk needs for this shard and batch. */
size_t lmi_scan_workspace_bytes(const lmi_index_desc* idx, int32_t nq, int32_t R,
                                int32_t k, int32_t qmode);

/* Per-(query, probe) exact top-k inside the probed bucket — the build contract
 * K2 of SURVEY.md §8(a) A4.  Replaces, for every probe r < R of every query,
 * utils.py:10-11 pairwise_cosine (sklearn normalize + BLAS GEMM), the full-row
 * argsort at LearnedIndex.py:170-172 and the pandas .loc gathers at :152-153,
 * :168.  Distances are 1 - cos(q, y) in fp32.
 *   q        device [nq][ldq] f32, raw query rows (normalised inside, sklearn rule)
 *   classes  device [nq][R] int32 bucket of probe r (router output)
 *   out_d    device [nq][R][k] f32 ascending, +inf past the bucket's size
 *   out_pos  device [nq][R][k] int32 global row positions, -1 past the end
 *   status   device int32, OR-ed with LMI_STATUS_* bits (caller zeroes it)
 * 1 <= k <= LMI_MAX_K_PASSES.  k > LMI_MAX_K (the reference takes any k on its
 * R == 1 path, search.py:134-140 -> LearnedIndex.py:103-111, and in
 * Baseline.py:14-19) returns the first kw = 15 * ceil(k/15) entries of the
 * (distance, position) order.  On the fp16 scan (fp16 corpus, fp16-exact
 * queries, d = 768): a bound scan (every bucket cut into 2 kw/15 lists, each
 * the top-15 of a sample of its rows: the kw-th smallest of those entries
 * bounds the pair's kw-th distance), a collect scan (every row within the
 * bound) and a sort -- two scans whatever k; buckets of fewer than ~2 kw rows
 * are collected whole, pairs whose candidates overflow take lower-bound passes
 * (ceil(k/15) scans, each keeping the next 15 entries after the previous
 * pass's last), as does every pair off the fp16 scan.  Bitwise the same lists
 * either way (LMI_WIDE_PASSES=1: the passes alone).  Same workspace contract
 * (lmi_scan_workspace_bytes). */
int lmi_bucket_topk(const lmi_index_desc* idx, const float* q, int32_t nq, int32_t ldq,
                    const int32_t* classes, int32_t R, int32_t k, int32_t qmode,
                    float* out_d, int32_t* out_pos, int32_t* status,
                    void* workspace, size_t ws_bytes, void* stream);

/* K2 tagged: lmi_bucket_topk with a predicate tested inside the scan.  Every
 * stored row carries a 32-bit tag word, every query a 32-bit want word; a row
 * is eligible for a query iff (tag & want) == want (all-of; want == 0 accepts
 * every row).  A (query, probe) list is the exact top-k, by (distance, global
 * position), of the eligible rows of the probed bucket, padded (+inf, -1) like
 * a short bucket: the list lmi_bucket_topk gives on an index built from the
 * eligible rows alone, bitwise in its distances.  A row that fails the
 * predicate never enters a list and never tightens a pair's bound.
 *   tags     device [n_rows] uint32, row order of idx->corpus
 *   want     device [nq] uint32
 * Every other argument, the outputs, the status bits and the workspace contract
 * (lmi_scan_tagged_workspace_bytes) are lmi_bucket_topk's.  1 <= k <= LMI_MAX_K.
 * The plan is lmi_bucket_topk's but that the 4-wave ring's shapes and the
 * 8-wave ring's 15-entry lists go to the general kernel: the 8-wave ring
 * (scan3_kernel MODE 4) for d_pad == 768, an fp16 corpus, LMI_Q_F16 and
 * k <= 10, the general kernel (scan_kernel TAG) for everything else; the
 * workspace has lmi_bucket_topk's size wherever both plans pick the same
 * kernel family.
 * LMI_E_INVALID (lmi_last_error says which) before any launch, device or no
 * device, for: null tags or want; k > LMI_MAX_K; idx->corpus32 or corpus64 (the
 * split mode); idx->chunk_centroid (sub-cluster layouts); any flag in qmode --
 * the phases, the join and LMI_Q_SEED_ROUND0: the tagged scan is never seeded
 * (its kernel has no scalar register left for the seed's pointer), and with
 * join workgroups set on the calling thread the call is refused.
 * Additions: LMI_ABI_VERSION does not change. */
size_t lmi_scan_tagged_workspace_bytes(const lmi_index_desc* idx, int32_t nq, int32_t R,
                                       int32_t k, int32_t qmode);
int lmi_bucket_topk_tagged(const lmi_index_desc* idx, const uint32_t* tags, const uint32_t* want,
                           const float* q, int32_t nq, int32_t ldq, const int32_t* classes,
                           int32_t R, int32_t k, int32_t qmode, float* out_d, int32_t* out_pos,
                           int32_t* status, void* workspace, size_t ws_bytes, void* stream);

/* K2 masked: the tagged scan with all-of and none-of bits in one predicate.  A
 * row is eligible for a query iff (tag & mask) == value, with
 *   value = want            the bits the row must have
 *   mask  = want | avoid    those and the bits it must not have
 * so (tag & want) == want and (tag & avoid) == 0.  lmi_bucket_topk_tagged is
 * this call with mask = want.  The kernels, the plan, the lists, the workspace
 * (lmi_scan_tagged_workspace_bytes) and every refusal are lmi_bucket_topk_tagged's.
 *   value, mask            device [nq] uint32 each
 *   host_value, host_mask  host [nq] copies of the two, or both null.  Where
 *                          they are given, a query with (value & ~mask) != 0 --
 *                          a bit both wanted and avoided, which the test would
 *                          read as wanted -- is LMI_E_INVALID before any launch,
 *                          device or no device; null: the caller has checked.
 * lmi_bucket_range_masked is lmi_bucket_range with the same two words and the
 * same host copies (tags, value and mask: all or none; untagged calls take
 * lmi_bucket_range).
 * Additions: LMI_ABI_VERSION does not change. */
int lmi_bucket_topk_masked(const lmi_index_desc* idx, const uint32_t* tags, const uint32_t* value,
                           const uint32_t* mask, const uint32_t* host_value, const uint32_t* host_mask,
                           const float* q, int32_t nq, int32_t ldq, const int32_t* classes, int32_t R,
                           int32_t k, int32_t qmode, float* out_d, int32_t* out_pos, int32_t* status,
                           void* workspace, size_t ws_bytes, void* stream);
int lmi_bucket_range_masked(const lmi_index_desc* idx, const uint32_t* tags, const uint32_t* value,
                            const uint32_t* mask, const uint32_t* host_value, const uint32_t* host_mask,
                            const float* q, int32_t nq, int32_t ldq, const int32_t* classes, int32_t R,
                            int32_t qmode, const float* bound, int32_t pair_cap, uint64_t* cand,
                            uint32_t* count, int32_t* status, void* workspace, size_t ws_bytes,
                            void* stream);

/* Tag edits in place: tags[rows[i]] = (tags[rows[i]] & ~clear[i]) | set[i] for
 * i < n, on the device tag words of a tagged index (the array the tagged scans
 * read), in stream order.  One launch of a grid-stride kernel; no atomics: the
 * rows of one call must be distinct (the caller guarantees it).
 *   tags             device [n_rows] uint32
 *   rows             device [n] int64 shard-local rows
 *   clear, set       device [n] uint32
 * A rows[i] outside [0, n_rows) writes nothing for that entry and raises
 * LMI_STATUS_INTERNAL in *status (device int32).  n == 0 is a no-op.
 * LMI_E_INVALID before any launch: n or n_rows < 0, a null pointer with n > 0.
 * The recipe for deletes by tombstone: set one reserved bit on the rows to hide
 * (a 4-byte scatter each), pass that bit as `avoid` (mask) to every search, and
 * compact the marked rows later in one batch.
 * Additions: LMI_ABI_VERSION does not change. */
int lmi_index_edit_tags(uint32_t* tags, int64_t n_rows, const int64_t* rows, const uint32_t* clear,
                        const uint32_t* set, int64_t n, int32_t* status, void* stream);

/* K11 range search: every row of the probed buckets within a per-query bound.
 *
 * lmi_bucket_range is the collect scan.  For pair p = q * R + r it writes
 *   count[p]                 uint32: the rows of bucket classes[p] with
 *                            d(q, row) <= bound[q] (inclusive), and with
 *                            (tag & want[q]) == want[q] when tags / want are
 *                            given (both or neither; null: untagged).  Exact
 *                            whatever pair_cap is.
 *   cand[p * pair_cap + i]   uint64, i < min(count[p], pair_cap): hits as
 *                            (distance ordinal << 32 | shard-local row), the
 *                            ordinal the order-preserving image of the float32
 *                            distance; in the scan's arrival order (unsorted).
 *                            A pair with count[p] > pair_cap holds pair_cap of
 *                            its hits, which ones is not defined: scan it
 *                            again with a larger pair_cap.
 * d is the float32 distance the top-k lists of the same kernel family hold for
 * that (query, row).  classes entries outside [0, n_buckets) probe nothing; a
 * bucket named twice in one query's row answers twice.  bound: device [nq]
 * float (-inf or any negative value: nothing).  qmode: LMI_Q_F16 or LMI_Q_F32
 * alone.  An fp16 corpus with LMI_Q_F16 and d_pad 768, untagged, runs the
 * 8-wave ring's collect scan (scan3_kernel MODE 2); every other call the
 * general kernel's collect form (range_scan_kernel).  Refused before any
 * launch, with a message: the split mode (corpus32 / corpus64), sub-cluster
 * layouts (chunk_centroid), phase / join / seed flags, join workgroups set on
 * the calling thread, pair_cap outside [1, 2^24], and on the general kernel a
 * d_pad whose query tile exceeds a workgroup's LDS (d_pad > 1248;
 * LMI_E_UNSUPPORTED).  lmi_range_workspace_bytes gives the workspace (0 for
 * what the call refuses, that width included; tagged != 0: the call has tags).
 *
 * lmi_range_rescore_f64: float64 distances of the stored candidates, in the
 * arithmetic and with the bits of lmi_bucket_topk_f64: d64[p * pair_cap + i]
 * for i < count[p], and kept[p] = how many have d64 <= radius64[q].  Pairs
 * with count[p] > pair_cap get kept[p] = 0 and no d64.  q: the float32 queries.
 *
 * lmi_range_pack: every pair with count[p] <= pair_cap writes its stored
 * candidates to entries off[p] .. of out_d (float64), out_pos (global
 * position) and out_q (query), unsorted; off: device [nq * R] int64, the
 * exclusive prefix of the entries each pair writes.  With d64 / radius64 (both
 * or neither) only candidates with d64 <= radius64[q] are written, d64 as the
 * distance (off: the prefix of kept); else the float32 distance, widened.
 * Pairs with count[p] > pair_cap write nothing: the second scan's call fills
 * their entries.
 * Additions: LMI_ABI_VERSION does not change. */
size_t lmi_range_workspace_bytes(const lmi_index_desc* idx, int32_t nq, int32_t R, int32_t qmode,
                                 int32_t tagged, int32_t pair_cap);
int lmi_bucket_range(const lmi_index_desc* idx, const uint32_t* tags, const uint32_t* want,
                     const float* q, int32_t nq, int32_t ldq, const int32_t* classes, int32_t R,
                     int32_t qmode, const float* bound, int32_t pair_cap, uint64_t* cand,
                     uint32_t* count, int32_t* status, void* workspace, size_t ws_bytes,
                     void* stream);
int lmi_range_rescore_f64(const lmi_index_desc* idx, const float* q, int32_t nq, int32_t ldq,
                          int32_t R, const double* radius64, int32_t pair_cap, const uint64_t* cand,
                          const uint32_t* count, double* d64, uint32_t* kept, void* stream);
int lmi_range_pack(const lmi_index_desc* idx, int32_t nq, int32_t R, int32_t pair_cap,
                   const uint64_t* cand, const uint32_t* count, const int64_t* off,
                   const double* d64, const double* radius64, double* out_d, int32_t* out_pos,
                   int32_t* out_q, void* stream);

/* ---- re-rank of short candidate lists from kept fp16 rows -------------------- */
/* The 8-bit storage's lists are approximate.  A caller that also
 * holds the index's fp16 rows scans longer lists (k_in entries a (query,
 * probe)) and re-scores them here: for every pair, the k smallest of its live
 * candidates by (d64, position), padded with (+inf, -1); d64 = the float64
 * distance of (query, row) in the arithmetic and with the bits of
 * lmi_bucket_topk_f64, computed from the stored fp16 row.
 *   rows   : the descriptor of the fp16 rows (LMI_F16) in the plain bucket
 *            layout of one GPU: position == row (gpos is the identity), no
 *            corpus32 / corpus64 / chunk_centroid, d <= 1024; only corpus, d,
 *            d_pad and n_rows are read
 *   q      : device float32 [nq][ldq], the queries as given
 *   in_pos : device int32 [nq][R][k_in] positions, -1 = empty, anywhere in a list
 *   out_d  : device float64 [nq][R][k]; out_pos: device int32 [nq][R][k]
 * 1 <= k <= k_in <= LMI_MAX_K.  A position >= n_rows is skipped and raises
 * LMI_STATUS_INTERNAL in *status (device int32, OR-ed into).  A position listed
 * twice in a pair is scored and written twice: nothing is de-duplicated.
 * LMI_E_INVALID, before any launch, for what the above excludes.  nq == 0 is a
 * no-op.  Additions: LMI_ABI_VERSION does not change. */
int lmi_rerank_f64(const lmi_index_desc* rows, const float* q, int32_t nq, int32_t ldq, int32_t R,
                   const int32_t* in_pos, int32_t k_in, int32_t k, double* out_d, int32_t* out_pos,
                   int32_t* status, void* stream);

/* Merge G per-shard lists of the same rows (K3): in
 * device [G][rows][k] (d f32, pos int32, -1 = empty), out device [rows][k] =
 * the k smallest by (d, pos).  Used after the RCCL all-gather of a G-GPU index.
 * 1 <= k <= LMI_MAX_K_PASSES (ABI 6; k > LMI_MAX_K merges by rank: the wide
 * lists of k > 16 at G > 1, search_single(k) / Baseline(k) on the R == 1 path,
 * LearnedIndex.py:103-111, Baseline.py:14-19).  The same range for
 * lmi_merge_topk_f64 and lmi_merge_topk_packed. */
int lmi_merge_topk(const float* d_in, const int32_t* pos_in, int32_t G, int64_t rows,
                   int32_t k, float* out_d, int32_t* out_pos, void* stream);

/* ---- float64 distances (ABI 4) ---------------------------------------- */
/* The reference computes 1 - cosine_similarity in float32 only when BOTH
 * operands are float32; otherwise — the real data: clip768 'emb' is float16 —
 * sklearn promotes to float64 (utils.py:11, :19; check_pairwise_arrays) and
 * the threshold test (utils.py:23) and the merges (LearnedIndex.py:86-97) see
 * float64 values.  lmi_bucket_topk_f64 returns those float64 lists:
 *   - the fp32 scan keeps 15 entries per (query, probe) for k <= 10 (round 5,
 *     fp16 scan: the union of 10-entry lane lists with the filter widened by
 *     2*eps, plus a bound below which no unlisted row lies; otherwise the
 *     top-KL, KL >= k + 5);
 *   - every list entry within 2*eps of the fp32 k-th distance is recomputed
 *     in float64 from the stored row (sklearn normalize + dot; exact fp16
 *     inputs; idx->corpus64 when set), sorted by (d64, position); when no
 *     unlisted row can lie in that band the result is the exact float64
 *     top-k whenever eps bounds the fp32 error |d32 - d64| for every row: the
 *     host passes a bound derived from d_pad and the MFMA accumulation depth
 *     (li.index.refine_eps; 2^-16 for the fp16 path at d 768);
 *   - other pairs are recomputed in float64 over their whole bucket shard
 *     (exact, rare: ties or near-ties of many objects).
 * With LMI_Q_SEED_ROUND0 the lists of rounds r >= 1 are exact below round 0's
 * threshold only (what the thresholded replay reads; k = k_round lists).
 * Same arguments and layout as lmi_bucket_topk; out_d is float64 [nq][R][k]
 * (+inf past the bucket's size), out_pos global positions (-1 past it).
 * 1 <= k <= LMI_MAX_K_F64, d <= 1024; k > 10 lists come from lower-bound
 * passes (as lmi_bucket_topk's) of at least k + 5 entries. */
#define LMI_REFINE_EPS 1.52587890625e-05 /* 2^-16 */
size_t lmi_scan_f64_workspace_bytes(const lmi_index_desc* idx, int32_t nq, int32_t R,
                                    int32_t k, int32_t qmode);
int lmi_bucket_topk_f64(const lmi_index_desc* idx, const float* q, int32_t nq, int32_t ldq,
                        const int32_t* classes, int32_t R, int32_t k, int32_t qmode, double eps,
                        double* out_d, int32_t* out_pos, int32_t* status, void* workspace,
                        size_t ws_bytes, void* stream);
/* ABI 6: as lmi_bucket_topk_f64, with float64 query rows q64 (device,
 * [nq][ldq64], nullable) for the float64 recomputation: the reference's
 * arithmetic on float64 queries (utils.py:11, :19).  q (float32) is what the
 * scan reads -- q64 rounded to float32.  Together with idx->corpus64 this is
 * the float64-input path; eps must then also cover the float32 rounding of
 * the inputs (8u more; li.index.refine_eps). */
int lmi_bucket_topk_f64q(const lmi_index_desc* idx, const float* q, int32_t nq, int32_t ldq,
                         const double* q64, int32_t ldq64, const int32_t* classes, int32_t R,
                         int32_t k, int32_t qmode, double eps, double* out_d, int32_t* out_pos,
                         int32_t* status, void* workspace, size_t ws_bytes, void* stream);
/* ABI 10: lmi_bucket_topk_f64q for a stripe of a G-rank index, with the band
 * decided over every rank's lists (replaces, for the striped
 * float64 search, the per-rank refinement of the same reference lines:
 * utils.py:10-11 in float64 and LearnedIndex.py:170-172).  The float64 top-k
 * of a pair lies in d32 <= T + 2 eps with T the k-th smallest d32 over ALL
 * ranks' rows; T is never above a rank's own k-th, so a rank that knows T
 * refines only its own rows of that merged band (about 1/G of them) instead
 * of the band of its own list.  Phases:
 *   PLAN, SCAN   as lmi_bucket_topk_f64q;
 *   MERGE        the chunk merge, then kth_send (device [nq*R][k] f32) = each
 *                pair's k smallest d32 of this rank (+inf past its list);
 *   (the caller all-gathers kth_send: block g of G at kth_all + g * kth_stride)
 *   REFINE       per pair T from the G blocks, then the refinement of this
 *                rank's listed rows with d32 <= T + 2 eps (and the whole-shard
 *                fallback of a pair whose band may hold unlisted rows): out_d
 *                / out_pos hold this rank's part of the pair's float64 top-k,
 *                ascending by (d64, position), (+inf, -1) past it.
 * No phase flag = all four on one rank (kth_all == kth_send, G == 1).  K3
 * (lmi_merge_topk_f64 / _packed) over the ranks' outputs then gives exactly
 * the one-GPU float64 lists.  Needs the band lists (k <= 10 on the fp16
 * scan): lmi_f64_global_band returns 1 when a call of these arguments has
 * them, 0 otherwise (then lmi_bucket_topk_f64q per rank). */
int lmi_f64_global_band(const lmi_index_desc* idx, int32_t nq, int32_t R, int32_t k, int32_t qmode);
int lmi_bucket_topk_f64g(const lmi_index_desc* idx, const float* q, int32_t nq, int32_t ldq,
                         const double* q64, int32_t ldq64, const int32_t* classes, int32_t R,
                         int32_t k, int32_t qmode, double eps, float* kth_send,
                         const float* kth_all, int32_t G, int64_t kth_stride, double* out_d,
                         int32_t* out_pos, int32_t* status, void* workspace, size_t ws_bytes,
                         void* stream);
/* ABI 9: the split mode's bound eps_x on |d~ - d| (lmi_index_desc.corpus32),
 * for rows of d_pad elements; a host function (≈ 9.9e-4 at d_pad = 768).  In the
 * split mode the eps argument of lmi_bucket_topk_f64* is ignored (this one
 * is used), and so is the fp16 / fp32 class of qmode (the queries are
 * normalised and rounded inside the call). */
double lmi_split_eps(int32_t d_pad);
/* ABI 11: lmi_index_desc.corpus32n from corpus32 (device [n][d_pad] float32
 * in and out, out's padding zeroed; a wave per row, index build, not the hot
 * path).  Replaces, per row, the normalize(Y) of the reference's
 * cosine_distances (utils.py:10-11; sklearn normalize: numpy einsum norms). */
int lmi_split_normalize(const float* rows, int64_t n, int32_t d, int32_t d_pad, float* out,
                        void* stream);
/* Diagnostic (synchronises `stream`): how many (query, probe) pairs of the
 * last lmi_bucket_topk_f64 call on this workspace took the whole-bucket path
 * (the split mode: also of lmi_bucket_topk, whose workspace has the same layout). */
int lmi_refine_fallback_count(const void* workspace, const lmi_index_desc* idx, int32_t nq,
                              int32_t R, int32_t k, int32_t qmode, int32_t* count_out,
                              void* stream);
/* ABI 13, diagnostic (synchronises `stream`): the split mode (k <= 10) collects
 * the rest of every bucket whose sample is at most a quarter of it and takes the
 * sample's rows from the sample scan's own list; how many pairs of the last call
 * on this workspace had a band reaching that list's k-th and were scored over
 * their sample rows and candidates instead (x_fallback_kernel). */
int lmi_split_sample_fallback_count(const void* workspace, const lmi_index_desc* idx, int32_t nq,
                                    int32_t R, int32_t k, int32_t* count_out, void* stream);
/* K3 on float64 lists: order (d64, pos). */
int lmi_merge_topk_f64(const double* d_in, const int32_t* pos_in, int32_t G, int64_t rows,
                       int32_t k, double* out_d, int32_t* out_pos, void* stream);

/* ---- K3 over the all-gathered buffer, in place (ABI 5) ------------------ */
/* A G-GPU search all-gathers one packed int32 buffer per rank instead of
 * separate lists (li/dist.py): rank g's words start at gathered + g *
 * rank_words and hold [distances: rows*k f32, or rows*k f64 as 2 words each]
 * [positions: rows*k int32][the rank's lmi_bucket_topk status word], padded
 * to rank_words (even, >= lmi_packed_rank_words; the buffer 8-byte aligned).
 * lmi_merge_topk_packed merges the G lists as lmi_merge_topk(_f64) does and
 * writes the OR of the G status words to out_status (device int32), so every
 * rank sees every rank's bits; out_d is f32 or f64 [rows][k] by dist_f64.
 * One launch replaces the unpacking copies and the per-rank status ORs. */
int64_t lmi_packed_rank_words(int64_t rows, int32_t k, int32_t dist_f64);
int lmi_merge_topk_packed(const int32_t* gathered, int32_t G, int64_t rank_words, int64_t rows,
                          int32_t k, int32_t dist_f64, void* out_d, int32_t* out_pos,
                          int32_t* out_status, void* stream);

/* ---- host replay of the reference's multi-round merge ----------------- */
/* Reproduces LearnedIndex.search (LearnedIndex.py:22-101) and search_single
 * (:103-195) — thresholds, per-category groups, the <k padding quirk
 * (:174-193), the 10000 fillers (utils.py:35-42) and the stable merge
 * (:86-97) — from the per-(query, probe) lists of lmi_bucket_topk
 * (SURVEY.md §8(a) A5).  All pointers are host memory.
 *   classes   [nq][R] int32;  lists_d / lists_pos [nq][R][k_list] (from device)
 *   k_round   length of one round's result: search_single's k.  search()
 *             never passes its k down (LearnedIndex.py:75-81), so it is 10
 *             there; search.py:134-140 passes k for the R == 1 path.
 *   k_final   search()'s k: columns kept by every merge (LearnedIndex.py:91)
 *   bucket_size [C] int64 objects per category (0 = category absent from
 *               data_navigation, so groupby never visits it)
 *   pos_to_id [n_total] int64  DataFrame index label of each global position
 *   use_threshold  0/1 as the reference's argument (search.py:127 passes True)
 *   thr_round0 [nq] float64 or NULL: search_single's threshold_dist argument
 *             (LearnedIndex.py:110, :149-163) for a direct R == 1 call
 *   dists_out [nq][w] float64, anns_out [nq][w] uint32 with w = k_round if
 *             R == 1 else k_final (*w_out receives w).
 * Returns LMI_E_INVALID where the reference's own assert (LearnedIndex.py:99)
 * would fail (k_final larger than the merged width). */
int lmi_replay(const int32_t* classes, int32_t nq, int32_t R, int32_t k_list,
               const float* lists_d, const int32_t* lists_pos, int32_t k_round,
               int32_t k_final, const int64_t* bucket_size, int32_t n_buckets,
               const int64_t* pos_to_id, int64_t n_total, int32_t use_threshold,
               const double* thr_round0, double* dists_out, uint32_t* anns_out,
               int32_t* w_out);
/* ABI 4: the same replay of float64 lists (lmi_bucket_topk_f64). */
int lmi_replay_f64(const int32_t* classes, int32_t nq, int32_t R, int32_t k_list,
                   const double* lists_d, const int32_t* lists_pos, int32_t k_round,
                   int32_t k_final, const int64_t* bucket_size, int32_t n_buckets,
                   const int64_t* pos_to_id, int64_t n_total, int32_t use_threshold,
                   const double* thr_round0, double* dists_out, uint32_t* anns_out,
                   int32_t* w_out);

/* The same replay on the device (ABI 2): identical results to lmi_replay
 * (checked bit for bit by tests/test_gpu_replay.py), no host round trip.
 * classes, lists_d, lists_pos, bucket_size, pos_to_id, thr_round0 (nullable),
 * dists_out, anns_out are device pointers; status (device int32, caller
 * zeroes it) is OR-ed with nonzero bits on an internal inconsistency (1, 2: a
 * list shorter than its bucket; 4: a position out of range; 8: a round's group
 * never completed in the one-launch replay, which then drains instead of
 * waiting forever).  k_list >= k_round,
 * k_round <= 32, k_final <= 64.  Asynchronous on `stream`; workspace of
 * lmi_replay_device_workspace_bytes bytes. */
size_t lmi_replay_device_workspace_bytes(int32_t nq, int32_t R, int32_t k_list, int32_t k_round,
                                         int32_t k_final, int32_t n_buckets);
int lmi_replay_device(const int32_t* classes, int32_t nq, int32_t R, int32_t k_list,
                      const float* lists_d, const int32_t* lists_pos, int32_t k_round,
                      int32_t k_final, const int64_t* bucket_size, int32_t n_buckets,
                      const int64_t* pos_to_id, int64_t n_total, int32_t use_threshold,
                      const double* thr_round0, double* dists_out, uint32_t* anns_out,
                      int32_t* status, void* workspace, size_t ws_bytes, void* stream);
/* ABI 4: the same device replay of float64 lists (lmi_bucket_topk_f64). */
int lmi_replay_device_f64(const int32_t* classes, int32_t nq, int32_t R, int32_t k_list,
                          const double* lists_d, const int32_t* lists_pos, int32_t k_round,
                          int32_t k_final, const int64_t* bucket_size, int32_t n_buckets,
                          const int64_t* pos_to_id, int64_t n_total, int32_t use_threshold,
                          const double* thr_round0, double* dists_out, uint32_t* anns_out,
                          int32_t* status, void* workspace, size_t ws_bytes, void* stream);

/* ABI 9: the device replay in two phases, so that a stream of batches runs the
 * part that depends on the classes only beside the scan:
 *   LMI_REPLAY_PHASE_GROUPS  every round's groups (queries by category, in
 *                            ascending q) and round 0's prologue; zeroes
 *                            *status (the phased call owns the word);
 *   LMI_REPLAY_PHASE_ROUNDS  the rounds and the answer (lists needed).
 * Both = lmi_replay_device / _f64 (the caller zeroes *status then).  Calls of
 * one replay take the same arguments and workspace, GROUPS first (lists_d /
 * lists_pos / pos_to_id / dists_out / anns_out may be NULL in a GROUPS call);
 * lists_f64 selects float64 lists. */
#define LMI_REPLAY_PHASE_GROUPS 1
#define LMI_REPLAY_PHASE_ROUNDS 2
int lmi_replay_device_phase(int32_t phases, int32_t lists_f64, const int32_t* classes, int32_t nq,
                            int32_t R, int32_t k_list, const void* lists_d, const int32_t* lists_pos,
                            int32_t k_round, int32_t k_final, const int64_t* bucket_size,
                            int32_t n_buckets, const int64_t* pos_to_id, int64_t n_total,
                            int32_t use_threshold, const double* thr_round0, double* dists_out,
                            uint32_t* anns_out, int32_t* status, void* workspace, size_t ws_bytes,
                            void* stream);

/* ---- k-means for the index build (ABI 3) -------------- */
/* Replaces faiss.Kmeans(d, k, seed=2023).train(X) and
 * kmeans.index.search(X, 1) (LearnedIndex.py:242-282); the Lloyd loop, the
 * training subsample and the empty-cluster split run on the host
 * (li/kmeans.py).  All pointers are device memory; asynchronous on `stream`.
 *
 * lmi_kmeans_assign: labels_out[i] = argmin_j Σ_e (x[i][e] - cent[j][e])²
 *   (squared L2 in fp32, e ascending, no FMA contraction; ties -> lower j);
 *   dist_out (nullable) receives the minimum.  x [n][d], cent [k][d] f32,
 *   1 <= d <= LMI_KMEANS_MAX_D (d <= 128: a row in registers; wider rows, e.g.
 *   the 768-d navigation, through a kernel that tiles the centroids instead;
 *   the same arithmetic and the same bits).
 * lmi_kmeans_update: cent_out[c] = mean of the points labelled c (fp64 sums
 *   in a fixed order, rounded once), counts_out[c] = their number; rows of
 *   empty clusters are left untouched.  A label outside [0, k) ORs 1 into
 *   *status (device int32) and is skipped.  Deterministic. */
#define LMI_KMEANS_MAX_D 1024
int lmi_kmeans_assign(const float* x, int64_t n, int32_t d, const float* cent, int32_t k,
                      int32_t* labels_out, float* dist_out, void* stream);
size_t lmi_kmeans_workspace_bytes(int64_t n, int32_t d, int32_t k);
int lmi_kmeans_update(const float* x, int64_t n, int32_t d, const int32_t* labels, int32_t k,
                      float* cent_out, int64_t* counts_out, int32_t* status, void* workspace,
                      size_t ws_bytes, void* stream);

/* ---- router training on every minibatch (K6) ------------ */
/* One optimizer step per minibatch of a Linear/ReLU stack under mean
 * cross-entropy and torch.optim.Adam's defaults (no weight decay, no amsgrad):
 * what the reference's NeuralNetwork.train does per step (model.py:150-172:
 * forward, CrossEntropyLoss, backward, Adam.step), taken on every minibatch of
 * a pass instead of train_batch's one step per epoch (model.py:174-199).
 * Additions of this section do not change LMI_ABI_VERSION: nothing existing
 * moves.
 *
 * The descriptor holds, per layer, the parameters and Adam's moments, all
 * device float32, updated in place: W / W_exp_avg / W_exp_avg_sq [out][in]
 * row-major (torch layout), b / b_exp_avg / b_exp_avg_sq [out].  Any width in
 * 1..LMI_TRAIN_MAX_DIM, for the input, hidden layers and classes alike. */
#define LMI_TRAIN_MAX_DIM 1024
typedef struct lmi_mlp_train_desc {
    int32_t n_layers;                 /* 1..LMI_MAX_LAYERS */
    int32_t dims[LMI_MAX_LAYERS + 1]; /* dims[0]=input width ... dims[n_layers]=n_classes */
    float* W[LMI_MAX_LAYERS];
    float* b[LMI_MAX_LAYERS];
    float* W_exp_avg[LMI_MAX_LAYERS];
    float* W_exp_avg_sq[LMI_MAX_LAYERS];
    float* b_exp_avg[LMI_MAX_LAYERS];
    float* b_exp_avg_sq[LMI_MAX_LAYERS];
} lmi_mlp_train_desc;
/* Bytes of workspace for minibatches of up to `batch` rows (0 for an invalid
 * descriptor or batch < 1).  The workspace needs no initialisation. */
size_t lmi_mlp_train_workspace_bytes(const lmi_mlp_train_desc* desc, int32_t batch);
/* Enqueues steps first_step .. first_step + n_steps - 1 of one pass on
 * `stream`, two kernels per step, no host synchronisation.  Step s trains on
 * the rows x[order[s*batch + i]], i < B_s = min(batch, n_order - s*batch) (the
 * pass's last step may be short, down to one row; the loss is the mean over
 * B_s, as DataLoader(drop_last=False) + CrossEntropyLoss() give), with Adam
 * step count adam_t0 + (s - first_step) + 1:
 *   m = beta1 m + (1-beta1) g;  v = beta2 v + (1-beta2) g^2;
 *   p -= (lr / (1-beta1^t)) * m / (sqrt(v) / sqrt(1-beta2^t) + eps).
 *   x        device [n][ldx] f32 rows;  y  device [n] int32 labels in [0, classes)
 *   order    device [n_order] int64 row indices in [0, n) (an entry outside is
 *            treated as a zero row without a label, never read)
 *   loss_out device [n_steps] f32: the mean loss of step first_step + i at [i]
 * Gradients and losses are reduced in a fixed order (no float atomics): equal
 * inputs give bitwise equal results, and a call of n steps equals n calls of
 * one step.  LMI_E_INVALID for a null pointer, batch < 1, n_layers or a dim out
 * of range, ldx < dims[0], first_step*batch >= n_order or steps past the end
 * of order; LMI_E_WORKSPACE for a workspace smaller than
 * lmi_mlp_train_workspace_bytes(desc, batch) or not 16-byte aligned.  All of
 * these are checked before any device call. */
int lmi_mlp_train_steps(const lmi_mlp_train_desc* desc, const float* x, int64_t n, int32_t ldx,
                        const int32_t* y, const int64_t* order, int64_t n_order, int32_t batch,
                        int64_t first_step, int64_t n_steps, int64_t adam_t0, double lr,
                        double beta1, double beta2, double eps, float* loss_out, void* workspace,
                        size_t ws_bytes, void* stream);

/* ---- index update (K7): add and remove rows without a rebuild -------------- */
/* An update of a one-GPU fp16 index writes a new bucket-sorted corpus beside
 * the old one: in every bucket the surviving rows keep their order and the
 * bucket's new rows follow in batch order -- the layout a construction from
 * scratch over the updated row sequence gives (the reference's groupby visit
 * order over the concatenated frame, LearnedIndex.py:143-145).  The host
 * prepares the offsets (li.index.BucketLayout.updated); these two calls move
 * the rows, asynchronously on `stream`, into caller-owned buffers.  Both OR
 * bits into the device word `status` (zeroed by the caller) and never write
 * outside dst_corpus [n_new][d_pad] / dst_inv_norm [n_new]: a destination row
 * outside [0, n_new) is skipped and LMI_STATUS_INTERNAL raised.  Additions:
 * LMI_ABI_VERSION does not change. */
#define LMI_STATUS_ROWS_NOT_F16 4 /* lmi_index_ingest_rows: a float32 value is not fp16-exact */
#define LMI_STATUS_ROWS_LOW_NORM 16 /* lmi_index_ingest_rows: a stored row's norm lies in
                                     * [10 eps(float64), 10 eps(float32)): a note, not an error --
                                     * the float64 mode scores it with its true 1/||y||
                                     * (li.index.DeviceIndex.inv_norm64) */
/* Old row i of bucket c (old_off[c] <= i < old_off[c+1]) goes to
 *   new_off[c] + (i - old_off[c]) - #{dropped rows of bucket c before i},
 * its 1/||y|| with it; a dropped row goes nowhere.
 *   src_corpus / dst_corpus  device fp16 [n][d_pad], 16-byte aligned, distinct
 *   old_off, new_off         device int64 [n_buckets + 1]; new_off[c] is where
 *                            bucket c starts in the new corpus
 *   dropped                  device int64 [n_dropped], ascending, distinct old
 *                            rows (NULL when n_dropped == 0)
 *   drop_before              device int64 [n_buckets + 1]: #{dropped < old_off[c]}
 *                            (NULL when n_dropped == 0)
 * One read and one write of the surviving rows, 16 bytes per lane. */
int lmi_index_move_rows(const void* src_corpus, const float* src_inv_norm, int64_t n_old,
                        int32_t d_pad, const int64_t* old_off, const int64_t* new_off,
                        int32_t n_buckets, const int64_t* dropped, int64_t n_dropped,
                        const int64_t* drop_before, void* dst_corpus, float* dst_inv_norm,
                        int64_t n_new, int32_t* status, void* stream);
/* Batch row j (device, `dtype` LMI_F16 or LMI_F32, m rows of d values, row
 * stride ld elements) is stored at row new_dst[j] (device int64 [m]) as fp16
 * with zeros in columns d..d_pad, and dst_inv_norm[new_dst[j]] = 1/||y|| of
 * the STORED values: the norm in float64, norms below 10 eps(float32) taken
 * as 1, one rounding to float32 (li.index._inv_norm).  A float32 value that
 * does not round-trip through fp16 raises LMI_STATUS_ROWS_NOT_F16 (the
 * rounded value is stored; the caller discards the buffers).  A stored row
 * whose norm is below 10 eps(float32) but not below 10 eps(float64) raises
 * LMI_STATUS_ROWS_LOW_NORM (the row and its 1/||y|| = 1 are stored as usual). */
int lmi_index_ingest_rows(const void* rows, int32_t dtype, int64_t m, int64_t ld, int32_t d,
                          int32_t d_pad, const int64_t* new_dst, void* dst_corpus,
                          float* dst_inv_norm, int64_t n_new, int32_t* status, void* stream);

/* ---- 8-bit storage: the quantiser (an addition: LMI_ABI_VERSION stays) ------- */
/* Row i of `rows` (device, `dtype` LMI_F16 or LMI_F32, m rows of d values, row
 * stride ld elements) becomes the int8 codes of slot dst_rows[i] (device int64
 * [m]; NULL: slot i) of `codes` ([slots][d_pad] int8), and inv_norm[slot] the
 * codes' 1/||c||.  With v the row's values as float32 (fp16 converts exactly):
 *   m = max_j |v_j|; if !(m >= 2^-100) (a zero, tiny or NaN row) every code is 0;
 *   else s = m / 127.0f and c_j = clamp(rintf(v_j / s), -127, 127) -- both
 *   divisions IEEE float32, rintf round-half-to-even, nothing contracted;
 *   columns d..d_pad are 0; ss = sum c_j^2 (an exact integer);
 *   inv_norm = ss == 0 ? 1.0f : (float)(1.0 / sqrt((double)ss)).
 * The scale s is not stored (the cosine does not need it).  All d_pad columns
 * of every slot touched are written; slots are the caller's to keep in range.
 * lmi_bucket_topk quantises its queries by the same device function.
 * LMI_E_INVALID before any launch: a dtype other than LMI_F16 / LMI_F32, m < 0,
 * d < 1, d_pad not d rounded up to a multiple of 32, ld < d, a null pointer
 * (m > 0), codes not 4-byte aligned. */
int lmi_quantize_rows_i8(const void* rows, int32_t dtype /*LMI_F16|LMI_F32*/, int64_t m, int64_t ld,
                         int32_t d, int32_t d_pad, const int64_t* dst_rows /*nullable*/,
                         int8_t* codes, float* inv_norm, void* stream);

/* ---- index update in place (K9): add / remove inside one buffer ------------- */
/* lmi_index_move_rows with source and destination in the SAME store of
 * `capacity` rows (li.index.DeviceIndex.add / remove with inplace=True): an add
 * (direction LMI_INPLACE_ADD: n_dropped == 0, n_new >= n_old) shifts every old
 * row right, a remove (LMI_INPLACE_REMOVE: n_new == n_old - n_dropped) shifts
 * every survivor left, both by an amount that does not decrease along the
 * corpus.  The host cuts the rows that move into slabs
 * (li.index.BucketLayout.inplace_slabs):
 *   slabs   HOST int64 [n_slabs][3] = (a, b, staged): old rows [a, b) inside
 *           [0, n_old), disjoint, in processing order -- an add from the end of
 *           the corpus backwards (every b <= the a before it), a remove from
 *           the front forwards (every a >= the b before it)
 *   staged = 0  the slab's destinations are disjoint from [a, b): one launch
 *               reads the store and writes the store
 *   staged = 1  the slab (at most stage_rows rows) is first copied to
 *               stage_corpus [stage_rows][d_pad] / stage_inv_norm [stage_rows],
 *               then written from there in a second launch
 * The whole chain is enqueued on `stream` by this one call; the order between
 * slabs is stream order alone (no grid barrier, no flag, no cooperative
 * launch), and inside one launch no workgroup writes a row another reads.
 * flags: LMI_INPLACE_MEMCPY copies a staged slab with hipMemcpyAsync instead
 * of the copy kernel (measurement).  The tables are lmi_index_move_rows'.
 * LMI_E_INVALID before any device call: a null or misaligned pointer, n_old
 * or n_new above capacity, counts that contradict the direction, a slab
 * outside [0, n_old), overlapping or out of the direction's order, a staged
 * slab longer than stage_rows.  In the kernel, before every write: the
 * destination lies in [0, n_new), outside [a, b) for a direct slab, and on
 * the direction's side of the source row; a row that fails is skipped and
 * LMI_STATUS_INTERNAL raised (the store's content is then undefined).
 * Additions: LMI_ABI_VERSION does not change. */
#define LMI_INPLACE_ADD 1
#define LMI_INPLACE_REMOVE (-1)
#define LMI_INPLACE_MEMCPY 1
int lmi_index_move_rows_inplace(void* corpus, float* inv_norm, int64_t n_old, int64_t n_new,
                                int64_t capacity, int32_t d_pad, const int64_t* old_off,
                                const int64_t* new_off, int32_t n_buckets, const int64_t* dropped,
                                int64_t n_dropped, const int64_t* drop_before, int32_t direction,
                                const int64_t* slabs, int64_t n_slabs, void* stage_corpus,
                                float* stage_inv_norm, int64_t stage_rows, int32_t flags,
                                int32_t* status, void* stream);

/* ---- index re-bucket (K8): new bucket labels without a rebuild -------------- */
/* A relabel of a one-GPU fp16 index gives every row of its row sequence a new
 * bucket; the new index is a permutation of the old one, made inside HBM
 * (li.index.DeviceIndex.relabel).  Both calls run asynchronously on `stream`,
 * write caller-owned buffers only and OR bits into the device word `status`
 * (zeroed by the caller).  Additions: LMI_ABI_VERSION does not change. */
#define LMI_STATUS_BAD_LABEL 8 /* lmi_bucket_sort_labels: a label outside [0, n_buckets) */
#define LMI_REBUCKET_MAX_BUCKETS 1024 /* the sort keeps one LDS cursor per bucket and wave */
#define LMI_REBUCKET_MAX_WAVES 4096   /* the sort's waves: longer intervals beyond */
#define LMI_GATHER_MAX_GRID 2048      /* lmi_index_gather_rows: workgroups (grid-strided beyond) */
#define LMI_GATHER_TILE_ROWS 32       /* destination rows of a workgroup per pass */
/* The stable bucket sort of n labels (device, int32 or int64: label_bytes 4 or
 * 8; labels[s] = bucket of sequence row s):
 *   bucket_off  device int64 [n_buckets + 1]: prefix sums of the bucket sizes
 *   order       device int64 [n]: the sequence row of every sorted position,
 *               rows of one bucket in sequence order
 * -- numpy's argsort(labels, kind="stable") and cumsum(bincount(labels)), bit
 * for bit.  A counting sort in four launches: every wave owns one interval of
 * the sequence (at most LMI_REBUCKET_MAX_WAVES waves), so ranks follow from
 * (wave, group of 64, lane) and no atomic hands one out.  A label outside
 * [0, n_buckets) raises LMI_STATUS_BAD_LABEL and nothing is written for its
 * row (order then has unwritten entries: the caller discards it).
 * LMI_E_INVALID: label_bytes, n < 0, n_buckets < 1, a null pointer;
 * LMI_E_UNSUPPORTED: n_buckets > LMI_REBUCKET_MAX_BUCKETS; LMI_E_WORKSPACE: a
 * workspace smaller than lmi_bucket_sort_labels_ws_bytes(n, n_buckets) (0 for
 * n = 0 or arguments the sort refuses) or not 8-byte aligned -- all checked
 * before any device call.  The workspace needs no initialisation. */
size_t lmi_bucket_sort_labels_ws_bytes(int64_t n, int32_t n_buckets);
int lmi_bucket_sort_labels(const void* labels, int32_t label_bytes, int64_t n, int32_t n_buckets,
                           int64_t* bucket_off, int64_t* order, int32_t* status, void* workspace,
                           size_t ws_bytes, void* stream);
/* dst_corpus[p] = src_corpus[src_pos[p]] and dst_inv_norm[p] =
 * src_inv_norm[src_pos[p]] for every p < n_dst:
 *   src_corpus / dst_corpus  device fp16 [n][d_pad], 16-byte aligned, distinct
 *   src_pos                  device int64 [n_dst], every entry in [0, n_src)
 * Destination-major: a wave writes consecutive destination rows as one
 * contiguous stream, 16 bytes per lane, every offset 64-bit.  A src_pos
 * outside [0, n_src) is checked before the read: the row is skipped and
 * LMI_STATUS_INTERNAL raised. */
int lmi_index_gather_rows(const void* src_corpus, const float* src_inv_norm, int64_t n_src,
                          int32_t d_pad, const int64_t* src_pos, void* dst_corpus,
                          float* dst_inv_norm, int64_t n_dst, int32_t* status, void* stream);

/* ---- index re-bucket in place (K10): the gather as two passes of row swaps ---- */
/* relabel's gather new[p] = old[src_pos[p]] inside ONE store
 * (li.index.DeviceIndex.relabel(inplace=True)): every permutation is the
 * product of two involutions, and an involution is a set of disjoint row swaps.
 * Both calls run asynchronously on `stream`, write caller-owned buffers only
 * and OR bits into the device word `status` (zeroed by the caller).
 * Additions: LMI_ABI_VERSION does not change. */
#define LMI_STATUS_BAD_PERM 32 /* lmi_perm_involutions: src_pos is no permutation of [0, n) */
/* The plan of src_pos (device int64 [n]; sigma below):
 *   partner1, partner2  device int64 [n], both involutions; swapping row j with
 *                       row partner1[j] for every j, then with partner2[j],
 *                       gives the gather by sigma
 * The plan is fixed: the leader L of a cycle of sigma is its smallest
 * position, e_0 = L, e_(t+1) = sigma(e_t), m the cycle's length;
 * partner1[e_t] = e_((m - t) mod m) and partner2[e_t] = e_(m - 1 - t).  A fixed
 * point of sigma is its own partner twice; a 2-cycle swaps in pass 2 only.
 * Pointer doubling over sigma on ping-pong buffers, ceil(log2 n) rounds for
 * the leaders and as many for the ranks, always all of them: nothing is read
 * back by the host, and 2 ceil(log2 n) + 9 launches are enqueued.  src_pos is
 * validated first (every entry in [0, n), every value hit once); when it is no
 * permutation LMI_STATUS_BAD_PERM is raised, the partners are unspecified and
 * no access leaves the buffers.  LMI_E_INVALID: n < 0, a null or misaligned
 * pointer, two of src_pos / partner1 / partner2 the same buffer;
 * LMI_E_WORKSPACE: a workspace smaller than lmi_perm_involutions_ws_bytes(n)
 * (40 bytes a row and 8 per 2048 rows; 0 for n <= 0) or not 16-byte aligned --
 * all checked before any device call.  The workspace needs no initialisation.
 * n = 0: nothing is enqueued. */
size_t lmi_perm_involutions_ws_bytes(int64_t n);
int lmi_perm_involutions(const int64_t* src_pos, int64_t n, int64_t* partner1, int64_t* partner2,
                         int32_t* status, void* workspace, size_t ws_bytes, void* stream);
/* One pass: for every j < n with partner[j] > j, rows j and partner[j] of
 * corpus (device fp16 [n][d_pad], 16-byte aligned, d_pad a multiple of 8) and
 * the two inv_norm entries change places.  Every pair is checked before its
 * first write: partner[j] lies in [0, n) and partner[partner[j]] == j; a pair
 * that fails is skipped and LMI_STATUS_INTERNAL raised (the store's content is
 * then undefined for the caller's purpose; every valid pair is swapped).  The
 * pairs of one launch are disjoint, so no workgroup writes a row another
 * reads; between two passes the order is stream order alone (no grid barrier,
 * no flag, no cooperative launch).  The grid is capped at LMI_GATHER_MAX_GRID
 * workgroups of LMI_GATHER_TILE_ROWS rows a pass and grid-strided beyond;
 * every offset is 64-bit.  LMI_E_INVALID before any device call: n < 0, d_pad,
 * a null or misaligned pointer.  n = 0: nothing is enqueued. */
int lmi_index_swap_rows(void* corpus, float* inv_norm, int64_t n, int32_t d_pad,
                        const int64_t* partner, int32_t* status, void* stream);

/* ---- kernel timing (measurement only) -------------------------------------- */
/* While enabled, lmi_bucket_topk records a HIP event pair on its stream around
 * its scan kernel (the roofline kernel).  lmi_timing_read waits for the pairs
 * recorded so far, writes up to max_n durations (ms) and clears the record;
 * it returns the number written or a negative LMI_E_* code.  Not for use
 * under graph capture (events recorded into a hipGraph cannot be timed). */
int lmi_timing_enable(int32_t on);
int32_t lmi_timing_read(float* ms_out, int32_t max_n);

/* ---- host utilities (ABI 6) ---------------------------------------------- */
/* 64-bit content hash of n_bytes of HOST memory on `threads` OpenMP threads
 * (<= 0: all), independent of the thread count; not cryptographic.  Keys the
 * drop-in's HBM index cache (li.LearnedIndex): a cached bucket-sorted corpus
 * is served only for byte-identical data_search / labels / ids, where the
 * reference re-gathers every bucket from the DataFrame on every call
 * (LearnedIndex.py:152-153, :168). */
uint64_t lmi_host_hash64(const void* data, uint64_t n_bytes, int32_t threads);

/* ---- staging a host query batch (ABI 8) ------------------------------------ */
/* The reference's queries are host arrays (search.py:49, :85-87); the batch
 * stream (li.stream.StreamedSearch.stage) writes each new batch into pinned
 * staging memory with these, on `threads` OpenMP threads (<= 0: all).
 * lmi_host_stage_f16: n float32 values -> fp16 (IEEE binary16, round to
 * nearest even) in dst; returns 1 when every value round-trips exactly
 * (numpy's array_equal(src.astype(f16).astype(f32), src): the fp16 MFMA
 * scan's precondition), 0 when some value does not (dst then holds rounded
 * values that no fp16-exact path may use), -LMI_E_INVALID on null pointers.
 * lmi_host_copy: a memcpy of n_bytes cut over the threads. */
int32_t lmi_host_stage_f16(const float* src, uint64_t n, uint16_t* dst, int32_t threads);
int lmi_host_copy(void* dst, const void* src, uint64_t n_bytes, int32_t threads);

/* ---- misc --------------------------------------------------------------- */
const char* lmi_last_error(void);
int32_t lmi_abi_version(void);
/* The LMI_* environment switches (diagnostic variants and tuning knobs; results
 * never depend on them) are read once, at the first launch.  Diagnostics that
 * change them inside one process call this to re-read them; not for use while
 * another thread launches.  The scan's workspace layout depends on the tail
 * split knobs (LMI_SCAN_SPLIT, LMI_SCAN_SPLIT_PARTS, LMI_SCAN_NO_PREF): after a
 * reload, size the workspaces again (lmi_scan_workspace_bytes /
 * lmi_scan_f64_workspace_bytes) -- a workspace sized under the old knobs may
 * be refused with LMI_E_WORKSPACE, never overrun. */
int lmi_config_reload(void);
/* The persistent scan's grid (ABI 12): the number of workgroups (one per CU)
 * the scan kernels of lmi_bucket_topk[_f64*] launch from this thread, so a
 * caller can leave CUs to work that runs beside the scan on other streams
 * (li.stream.StreamedSearch: the finish chain of the previous batch).  0: one
 * per CU (or LMI_SCAN_WGS).  Thread-local, read at launch (a captured graph
 * keeps the grid it was captured with); results never depend on it.  Returns
 * the previous setting. */
int32_t lmi_scan_set_workgroups(int32_t wgs);
/* The late-joining scan (see LMI_Q_PHASE_SCAN_JOIN): the number j of the
 * scan's workgroups that the SCAN phase leaves to the SCAN_JOIN phase.  With
 * j > 0 the SCAN phase of lmi_bucket_topk[_f64*] launches its kernel with j
 * workgroups fewer than the grid above (at least one stays), and the
 * SCAN_JOIN phase launches the same kernel with j workgroups on the workspace
 * as the plan left it.  The plan never depends on j.  0 (the default): the
 * SCAN phase launches the whole grid and the SCAN_JOIN phase does nothing.
 * Only the scans of the 8-wave ring with 10- or 15-entry lists or band lists
 * take j > 0 (lmi_scan_joinable / lmi_scan_f64_joinable); every other scan
 * (the split mode, k > LMI_MAX_K, the general kernel and the 4-wave ring)
 * refuses a SCAN or SCAN_JOIN phase while j > 0 with LMI_E_INVALID and
 * launches nothing.  Thread-local, read at launch like the grid; results
 * never depend on it.  Returns the previous setting. */
int32_t lmi_scan_set_join_workgroups(int32_t j);
/* The 8-bit storage's 16-entry lists on its ring (an addition: LMI_ABI_VERSION
 * does not change).  By default lmi_bucket_topk[_masked] on LMI_I8 at d_pad ==
 * 768 runs k = 11..16 on scan_i8_kernel, as it always has.  With on != 0 the
 * plan of this thread sends them to the 8-wave ring (scan3_i8_kernel with
 * 16-entry lists: the over-fetch that lmi_rerank_f64 re-scores), about a fifth
 * of the time.  The lists are the same bits either way; the workspace layout
 * differs, so size the workspace (lmi_scan_workspace_bytes /
 * lmi_scan_tagged_workspace_bytes) and ask lmi_scan_family under the setting the
 * call runs with.  Thread-local, read when the plan is made (every call).
 * LMI_SCAN_V1 still forces scan_i8_kernel.  Returns the previous setting. */
int32_t lmi_scan_set_i8_lists16(int32_t on);
/* 1 when lmi_bucket_topk (lmi_scan_joinable) or lmi_bucket_topk_f64* (the
 * _f64 form) of these arguments runs a scan that takes j > 0, else 0. */
int lmi_scan_joinable(const lmi_index_desc* idx, int32_t nq, int32_t R, int32_t k, int32_t qmode);
/* The kernel family that lmi_bucket_topk (tagged != 0: lmi_bucket_topk_tagged /
 * _masked) of these arguments scans with, read from the plan the launch itself
 * uses: 0 the general kernel (on LMI_I8: scan_i8_kernel), 1 the 4-wave ring,
 * 2 the 8-wave ring, 3 the 8-wave ring of the 8-bit storage (LMI_I8 with
 * LMI_Q_I8 at d_pad == 768: k <= 10, and k = 11..16 on a thread that set
 * lmi_scan_set_i8_lists16).  The diagnostic switches LMI_SCAN_V1 /
 * LMI_SCAN_V2 show in the answer (after lmi_config_reload).  A combination the
 * scan refuses -- LMI_I8 without LMI_Q_I8 or with LMI_Q_SEED_ROUND0, k outside
 * [1, LMI_MAX_K], a qmode that is no query class -- is a negative LMI_E_* code
 * (lmi_last_error says which).  Host only: no launch, no device. */
int32_t lmi_scan_family(const lmi_index_desc* idx, int32_t k, int32_t qmode, int32_t tagged);
int lmi_scan_f64_joinable(const lmi_index_desc* idx, int32_t nq, int32_t R, int32_t k,
                          int32_t qmode);

#ifdef __cplusplus
}
#endif
#endif /* LMI_HIP_H */
