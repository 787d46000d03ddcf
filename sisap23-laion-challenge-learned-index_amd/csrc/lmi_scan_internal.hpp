// Internal declarations shared by the K2 scan translation units
// (lmi_scan.hip: prep / plan / scan v3 / chunk merge / the scan's plan and
// its one host entry, bucket_topk_impl; lmi_scan_wide.hip: k > 16;
// lmi_scan_split.hip: the split mode's driver; lmi_scan_v12.hip: the round-1
// and round-2 scan kernels, kept as fallbacks for shapes scan v3 does not take
// and as A/B baselines; lmi_range.hip: K11 range search, the general kernel's
// collect form and its driver) and with lmi_refine.hip, their one outside caller.
// Not an ABI.
#pragma once
#include "lmi_common.hpp"

#include <mutex>
#include <utility>
#include <vector>

namespace lmi {

using half8 = _Float16 __attribute__((ext_vector_type(8)));
using half4 = _Float16 __attribute__((ext_vector_type(4)));
using f32x16 = float __attribute__((ext_vector_type(16)));
using f32x4 = float __attribute__((ext_vector_type(4)));
using u32x4 = uint32_t __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;  // 4 waves
constexpr int kWaves = 4;
constexpr int kQCap = 16;      // queue entries per lane (= candidates of one 32x32 tile)

struct Tile {
    int32_t c;        // bucket
    int32_t pp0;      // first pair position (into the bucket-grouped pair list)
    int32_t np;       // pairs in this tile (<= QB)
    int32_t chunk;    // chunk index inside the bucket
};

struct ScanArgs {
    const void* corpus;
    int32_t d_pad;
    const float* inv_norm;
    const int64_t* bucket_off;
    int32_t chunk_rows;
    int32_t max_chunks;
    const void* qbuf;       // [nq][d_pad] f16 or f32
    const float* invq;      // [nq]
    const int32_t* pair_q;  // [P] pair id p = q*R + r, grouped by bucket
    int32_t R;
    const Tile* tiles;
    const int32_t* meta;    // tile groups (plan_fill_kernel)
    int32_t* work;          // dequeue counters
    uint64_t* partial;      // [P][max_chunks][KL]
    const int32_t* gpos;    // [n_rows] global positions (LO: ties at the lower bound)
    const unsigned long long* lo_g;  // [nq*R] LO: keep only keys above (d, gpos) of the pair
    const uint32_t* tags;   // TAG: [n_rows] tag word of every row (row order of corpus)
    // TAG: [nq] triples (1/|q|, value, mask) of every query (want_pack_kernel);
    // value = the wanted bits, mask = wanted | avoided; row eligible iff
    // (tag & mask) == value
    const uint32_t* want;
};


// tail split: at most this many tiles per queue are halved (tail_split_kernel)
constexpr int kSplitMaxK = 256;
constexpr int kSplitMaxParts = 8;
// row parts of a tail-split tile (LMI_SCAN_SPLIT_PARTS, clamped to [2, kSplitMaxParts])
int split_parts();
// tile groups of the persistent scans' dequeue (XCD round-robin, see
// plan_fill_kernel in lmi_scan.hip)
constexpr int kGroups = 8;

// The next tile for a workgroup of group `gx`: its own group first, then steal.
__device__ inline int dequeue_tile(const int32_t* meta, int32_t* work, int gx, int ng) {
    for (int k = 0; k < ng; ++k) {
        const int g = (gx + k) & (ng - 1);
        const int sz = meta[kGroups + g];
        if (__hip_atomic_load(&work[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= sz) continue;
        const int v = atomicAdd(&work[g], 1);
        if (v < sz) return meta[g] + v;
    }
    return -1;
}

// ---------------------------------------------------------------------------
// scan v2 (fp16 corpus, fp16-exact queries, d_pad == 768): queries in
// registers, object rows staged once per workgroup through an LDS ring by
// global_load_lds DMA, shared by the 4 waves (128 queries per staged row).
//
//   per wave : 32 queries; their 48 MFMA B fragments (K = 768) live in VGPRs
//              for the whole tile (192 registers)
//   per stage: 32 object rows x 256 k (16 KiB) + each wave's copy of the 32
//              rows' 1/||y||; 7-slot ring, 4 stages in flight, one raw
//              s_barrier per stage (never __syncthreads inside the ring: its
//              vmcnt(0) would drain the DMA, guide §5 "Pipelining")
//   LDS image: row r, 16-B chunk c stored at chunk c ^ (r & 15) (the XOR
//              is applied to the DMA *source* address, LDS stays lane-linear),
//              so the 32-row A-fragment ds_read_b128 is bank-conflict free
//   per block of 32 rows: 48 x v_mfma_f32_32x32x16_f16 per wave, then the
//              top-k epilogue of v1 with 1/||y|| read from LDS
// A per-pair threshold in global memory (min over the k-th keys published
// by finished tiles of the same pair) seeds every tile's filter.
// ---------------------------------------------------------------------------
namespace v2 {
constexpr int D = 768;
constexpr int KSEG = 256;
constexpr int NST = D / KSEG;          // stages per 32-row block
constexpr int ROWB = KSEG * 2;         // bytes of one row in one stage
constexpr int TRAIL = 4 * 256;         // per-wave copies of the 32 norms
constexpr int STAGE = 32 * ROWB + TRAIL;
constexpr int NSLOT = 7;
constexpr int QB = 128;
constexpr int NQF = D / 16;            // B fragments per lane

template <int KL>
constexpr size_t lds_bytes() {
    return (size_t)NSLOT * STAGE + (size_t)kWaves * 64 * 16 * 8 + 16;
}
}  // namespace v2

// the float64 mode's band lists (scan3_kernel MODE 3): 15 entries + a bound
// per (pair, chunk part)
constexpr int kBandSlot = 16;

struct Scan2Args {
    const _Float16* corpus;
    const float* inv_norm;
    const int64_t* bucket_off;
    int32_t chunk_rows;
    int32_t max_chunks;
    const _Float16* qbuf;
    const float* invq;
    const int32_t* pair_q;
    int32_t R;
    const Tile* tiles;
    const int32_t* meta;
    int32_t* work;
    uint64_t* partial;
    unsigned long long* thr_g;  // [P] per-pair bound, EMPTY at start
    int32_t ng;                 // tile groups (power of two <= kGroups)
    int32_t lag;                // extra ring stages waited for (tuning knob, 0)
    const int32_t* gpos;        // LO: global positions of the rows
    const unsigned long long* lo_g;  // LO: [nq*R] lower-bound key (d, gpos) per pair id
    const int32_t* pair_pos;    // LMI_Q_SEED_ROUND0: [P] grouped position of the pair's (q, 0), -1 if none; else null
    float seed_margin;          //   (distance added to the seed: 2 eps in the float64 mode)
    float band;                 // MODE 3 (the float64 mode's band lists): distance added to the filter bound
    unsigned long long* dbg;    // diagnostic counters of the ABL != 0 variants (lmi_scan_abl.hip); null
    // collect mode (k > 16, scan3_kernel MODE 2): every row of a pair within
    // its fixed bound goes to cand[pp * cap + i], i from ccount[pp] (grouped
    // position pp; a count past cap means the pair overflowed)
    uint64_t* cand;
    uint32_t* ccount;
    int32_t cap;
    // chunk-list mode (MODE 1): nbins distance ordinals per grouped pair, bin
    // j = the smallest 15th entry of the pair's finished chunk lists j mod
    // nbins; their maximum bounds nbins * 15 >= kw entries, so entries above
    // it cannot change the kw-th smallest of the lists (the bound)
    uint32_t* bins;
    int32_t nbins;
    const int32_t* sub_rows;  // MODE 1: [C] rows per list of each bucket (its chunks)
    const int32_t* sub_take;  //   and the rows scanned from the start of each (a sample)
    // MODE 4 (lmi_bucket_topk_tagged): the rows' tag words ([n_rows], row order
    // of corpus); a row is a candidate of a pair only if (tag & mask) == value.
    // The queries' two words come beside 1/|q|: invq is then [nq] triples
    // (1/|q|, value, mask) (want_pack_kernel) -- no pointer more in scalar
    // registers, of which the kernel has none to spare
    const uint32_t* tags;
};

// s_waitcnt immediates (gfx9 encoding: vmcnt[3:0] + vmcnt[5:4] at [15:14],
// expcnt [6:4], lgkmcnt [11:8]); other counters left at their maximum.
// The builtin (not inline asm) keeps hipcc's wait-count scoreboard in sync,
// so it does not add its own conservative vmcnt waits later in the loop.
constexpr int waitcnt_vm(int n) { return (n & 15) | ((n >> 4) << 14) | (7 << 4) | (15 << 8); }

// The same value from the partner lane (lane ^ 32): both halves of a 32x32
// accumulator column hold one query.  v_permlane32_swap is a VALU op, so no
// LDS write happens inside the DMA ring (hipcc would drain the LDS-DMA with a
// vmcnt(0) before any LDS write it cannot prove disjoint from the ring).
__device__ __forceinline__ uint32_t partner_u32(uint32_t x, int h) {
    const auto r = __builtin_amdgcn_permlane32_swap(x, x, false, false);
    return h ? r[0] : r[1];
}
__device__ __forceinline__ uint64_t partner_u64(uint64_t x, int h) {
    const uint32_t lo = partner_u32((uint32_t)x, h);
    const uint32_t hi = partner_u32((uint32_t)(x >> 32), h);
    return ((uint64_t)hi << 32) | lo;
}

// LDS destination of the buffer_load ... lds DMA builtins
typedef __attribute__((address_space(3))) void* lds_t;

// Raw LDS accesses at a byte address (no implicit waits beyond the read's own).
__device__ __forceinline__ void lds_put_u64(uint32_t addr, uint64_t v) {
    asm volatile("ds_write_b64 %0, %1" ::"v"(addr), "v"(v) : "memory");
}
__device__ __forceinline__ uint64_t lds_get_u64(uint32_t addr) {
    uint64_t v;
    asm volatile("ds_read_b64 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(addr) : "memory");
    return v;
}

// ---- host side shared by the scan launchers ---------------------------------
int num_cus();

// optional event timing of the scan kernels (lmi_timing_enable / _read)
struct Timing {
    std::mutex mu;
    bool on = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending, pool;
};
Timing& timing();
int timing_record(hipStream_t s, bool start, std::pair<hipEvent_t, hipEvent_t>& pr);

// lmi_scan_v12.hip (explicitly instantiated there for the shapes the host
// dispatch in lmi_scan.hip uses)
template <int KL, bool F16MATH, typename TC, bool LO = false, bool TAG = false>
int launch_scan(const ScanArgs& a, int d_pad, hipStream_t s);
template <int KL>
int launch_scan2(const Scan2Args& b, hipStream_t s);
// scan_i8_kernel (8-bit storage: int8 corpus, int8 qbuf; KL 10 / 16, plain or TAG)
template <int KL, bool TAG>
int launch_scan_i8(const ScanArgs& a, int d_pad, hipStream_t s);
// the widest row of the 8-bit scan
constexpr int kI8MaxDPad = 992;
// scan3_i8_kernel (lmi_scan_ring_i8.hip: the 8-wave ring on the 8-bit storage,
// d_pad == 768, lists of KL = 10 or 16 entries, plain or TAG)
template <int KL, bool TAG>
int launch_scan3_i8(const Scan2Args& b, hipStream_t s);

// ---- the scan's plan (lmi_scan.hip) -----------------------------------------
// Every choice a scan of (idx, nq, R, k, qmode, lo) makes, made once: the
// kernel family, the list length, the tile width, the tail split's parts and
// where each array lies in the caller's workspace.  bucket_topk_impl reads it;
// so do the workspace sizes and the drivers that look into a scan's region
// afterwards (the grouped pairs, the partial lists).  lo: a lower-bound pass.
// General: scan_kernel (8-bit storage: scan_i8_kernel); Ring4: scan2_kernel
// (4 waves); Ring8: scan3_kernel; Ring8I8: scan3_i8_kernel (the 8-bit storage at
// d_pad == 768 and k <= 16: the 8-wave ring's tiles, one part, none of its
// other paths).  The values are lmi_scan_family's.
enum class ScanKernel { General = 0, Ring4 = 1, Ring8 = 2, Ring8I8 = 3 };
struct ScanPlan {
    ScanKernel family;
    // list length of the scan: 10 (k <= 10), 15 (k <= 15 on the 8-wave ring:
    // the float64 mode's 10 + 5 guard entries), else 16
    int32_t kl, qb;  // (qb: queries per tile)
    // fp16 corpus and fp16-exact queries; the nearest-chunk-first plan (8-wave
    // ring, chunk centroids)
    bool f16math, nearest_first;
    // the 8-bit storage (LMI_I8 with LMI_Q_I8): scan_i8_kernel of the general
    // family or the Ring8I8 family, qbuf holds int8 rows
    bool i8;
    int32_t split_s;     // row parts of a tail-split chunk (1: the tail split is off)
    int32_t list_stride;  // partial-list slots per pair: split_s * max(max_chunks, 1)
    int32_t max_tiles;
    // offsets into the workspace (pair_pos, seed_pos: LMI_Q_SEED_ROUND0, the
    // grouped position of every pair id and of every grouped pair's (q, 0))
    size_t qbuf, invq, counts, pair_q, pair_bucket, tiles, ntiles, work, partial, ext_off,
        split_mask, thr_g, pref, pref_tmp, pref_tmp2, n_seed, pair_pos, seed_pos, total;
};
// tagged: the plan of lmi_bucket_topk_tagged -- the untagged plan but that the
// 4-wave ring's and the 8-wave ring's 15-entry shapes go to the general kernel
ScanPlan scan_plan(const lmi_index_desc* idx, int nq, int R, int k, int qmode, bool lo = false,
                   bool tagged = false);
// The 8-bit storage's refusals, before any launch and with no device.
// i8_gate: a call of lmi_bucket_topk / _masked with `qmode` as the caller gave
// it (flags included) -- LMI_OK off the 8-bit storage, else LMI_I8 and LMI_Q_I8
// together, k <= LMI_MAX_K, no seed, no join phase, no corpus32 / corpus64 /
// chunk_centroid, d_pad <= kI8MaxDPad.  i8_refuse: every other entry point.
int i8_gate(const char* fn, const lmi_index_desc* idx, int32_t k, int32_t qmode);
int i8_refuse(const char* fn, const lmi_index_desc* idx);
// the 8-wave ring serves this index and query class (the float64 mode's band lists)
bool band_capable(const lmi_index_desc* idx, int qmode);
size_t scan_workspace_bytes(const lmi_index_desc* idx, int32_t nq, int32_t R, int32_t k,
                            int32_t qmode, bool lo = false);

// phases of bucket_topk_impl (LMI_Q_PHASE_* of the ABI, shifted to bits 0..2;
// kPhaseJoin: LMI_Q_PHASE_SCAN_JOIN, not one of "all")
constexpr int kPhasePlan = 1, kPhaseScan = 2, kPhaseMerge = 4, kPhaseAll = 7, kPhaseJoin = 8;
// LMI_Q_PHASE_* bits of a qmode -> kPhase* (none set = all); strips them from qmode
inline int take_phases(int32_t& qmode) {
    const int p = ((qmode >> 9) & 7) | ((qmode & LMI_Q_PHASE_SCAN_JOIN) ? kPhaseJoin : 0);
    qmode &= ~((7 << 9) | LMI_Q_PHASE_SCAN_JOIN);
    return p ? p : kPhaseAll;
}
// The late-joining scan (lmi_scan_set_join_workgroups): j of this thread, and
// the gate every entry point passes its phases through before it launches
// anything: with j = 0 the join phase is dropped (*done: nothing is left to
// do); with j > 0 a call with a SCAN or SCAN_JOIN phase whose scan does not
// take the join (`joinable` false) is refused with LMI_E_INVALID
int join_wgs();
int join_gate(int& phases, bool joinable, bool* done);
// the grid of the scan launch under way: scan_grid() is num_cus() but inside a
// ScanGrid scope (the main and the join launch of bucket_topk_impl)
int scan_grid();
struct ScanGrid {
    explicit ScanGrid(int wgs);
    ~ScanGrid();
    ScanGrid(const ScanGrid&) = delete;
    ScanGrid& operator=(const ScanGrid&) = delete;
};
// The scans of the wide path (k > 16, bucket_topk_wide): mode 1 writes every
// (pair, chunk part) list as that part's own top-15 (no global bound); mode 2
// collects every row within the pair's bound bound_ord[pair id] (a distance
// ordinal; 0 = none) into cand[grouped pair * cap + i] (ccount: slots taken).
struct WideScan {
    int mode;
    const uint32_t* bound_ord;
    uint64_t* cand;
    uint32_t* ccount;
    int32_t cap;
    uint32_t* bins;  // mode 1: [P][nbins], all ones at the start (Scan2Args::bins)
    int32_t nbins;
    const int32_t* sub_rows;  // mode 1: Scan2Args::sub_rows / sub_take
    const int32_t* sub_take;
    // mode 2: a pair whose (odd) bucket b has rows skipped in front of it
    // (bucket b - 1 of the descriptor not empty: the split mode's sample,
    // x_collect_desc) starts with its app_k (distance, row) entries app_d /
    // app_row [pair id][app_k] as candidates (-1 rows skipped); null: none
    const float* app_d;
    const int32_t* app_row;
    int32_t app_k;
};
// The general kernel's collect form (K11 range search, lmi_range.hip): every
// row of a pair with d <= bound[q] (and (tag & mask) == value when tagged) goes
// to cand[pair id * cap + i] as make_key(d, row), i from ccount[pair id], which
// counts every hit (slots past cap are counted, not stored).  No lists, no merge.
struct RangeScan {
    const float* bound;  // [nq] one bound per query (-inf: nothing)
    uint64_t* cand;      // [nq*R][cap]
    uint32_t* ccount;    // [nq*R], zeroed by the call's prep
    int32_t cap;
};
struct RangeArgs {
    ScanArgs s;
    const float* bound;
    uint64_t* cand;
    uint32_t* ccount;
    int32_t cap;
};
// range_scan_kernel for fp16 math / an fp16 or fp32 corpus / tags (a.s.tags)
int launch_range_scan(const RangeArgs& a, bool f16math, bool corpus_f16, hipStream_t s);

// One call of K2 up to the merged per-pair lists (bucket_topk_impl, lmi_scan.hip):
// lmi_bucket_topk's arguments, a third output (out_row: the shard-local row of
// every entry, -1 = empty; nullable), and the options below.
struct ScanCall {
    const lmi_index_desc* idx;
    const float* q;
    int32_t nq, ldq;
    const int32_t* classes;
    int32_t R, k, qmode;
    float* out_d;
    int32_t *out_pos, *out_row, *status;
    void* workspace;
    size_t ws_bytes;
    hipStream_t stream;
    // device [nq*R] or null: keep only objects after the (distance, global
    // position) key of their pair (the passes of k > 16)
    const unsigned long long* lo_g = nullptr;
    int32_t ldo = 0;      // entries per pair in the outputs (0: k)
    bool prefill = true;  // write (+inf, -1) over all R*ldo entries first (the first pass)
    // LMI_Q_SEED_ROUND0: pairs r >= 1 start from the bound of pair (q, 0),
    // + seed_margin in distance
    bool seed_r0 = false;
    float seed_margin = 0.0f;
    int phases = kPhaseAll;
    const WideScan* wide = nullptr;
    // [nq*R] float or null (k <= 15 on the 8-wave ring, kl = 15): the float64
    // mode's band lists -- the scan's filter widened by seed_margin (2 eps),
    // every pair's first 15 entries, and out_bound[pair] a distance such that
    // each row of the shard the list does not hold failed the widened filter
    // or has d32 >= it (chunk_merge_band_kernel)
    float* out_bound = nullptr;
    // with out_bound, or null: each pair's first kth_k list distances also
    // written to kth_out[pair * kth_k] (the float64 global band's kth_send, ABI 10)
    float* kth_out = nullptr;
    int32_t kth_k = 0;
    // scan_plan() of this call where the caller holds it (it reads the scan's
    // region afterwards); null: built here
    const ScanPlan* plan = nullptr;
    // lmi_bucket_topk_masked: device [n_rows] tag words and [nq] value and mask
    // words (all or none); only rows with (tag & mask) == value are listed
    // (lmi_bucket_topk_tagged: mask = want)
    const uint32_t* tags = nullptr;
    const uint32_t* want = nullptr;  // the value words
    const uint32_t* mask = nullptr;
    // K11 range search: the general kernel's collect form in place of the list
    // scan (a plan of the general family, phases plan + scan, no prefill)
    const RangeScan* range = nullptr;
};
int bucket_topk_impl(const ScanCall& c);
// the masked entries' host copies of their words (both or neither; null: not
// checked): every value word inside its mask word, else LMI_E_INVALID
int masked_words_check(const char* fn, const uint32_t* host_value, const uint32_t* host_mask, int32_t nq);

// ---- k > LMI_MAX_K (lmi_scan_wide.hip) ---------------------------------------
// passes_of() passes of kp-entry lists; bucket_topk_passes fills [nq*R][ldo]
// lists (ldo >= passes * kp) with (d32, global position[, local row]).
int passes_of(const lmi_index_desc* idx, int qmode, int k, int* kp_out);
size_t passes_ws_bytes(const lmi_index_desc* idx, int nq, int R, int k, int qmode);
int bucket_topk_passes(const ScanCall& c);
// The same lists as bucket_topk_passes from two scans (the 8-wave ring):
// chunk lists -> per-pair bound (the kw-th smallest of the pair's chunk-list
// distances, kw = passes * kp) -> collect the rows within it -> sort; pairs
// without a bound (too few chunk-list entries) or whose candidates overflow
// go through bucket_topk_passes restricted to them.  Off the 8-wave ring (or
// under LMI_WIDE_PASSES) it is bucket_topk_passes.
size_t wide_ws_bytes(const lmi_index_desc* idx, int nq, int R, int k, int qmode, int ldo);
int bucket_topk_wide(const ScanCall& c);
// lmi_bucket_topk at k > LMI_MAX_K: bucket_topk_wide into lists at the head of
// the workspace, their first k to the caller's [nq*R][k] outputs
int bucket_topk_wide_k(const ScanCall& c);
// The sampled bound of the wide path and of the split mode: every bucket cut
// into at most `lists` lists (bound_lists_kernel -> sub_first / sub_rows /
// sub_take), each list's first part scanned in MODE 1 with nbins pruning bins
// per pair, and bound[pair id] = the kw-th smallest distance ordinal of the
// pair's lists (kth_bound_kernel; no bound: all ones where the bucket fits cap
// slots, else fix[pair id] = 1).  scan: the call of the MODE 1 scan but for
// idx, k, prefill, phases and wide; wide_init_kernel pads its outputs
// [nq*R][pad_ldo] (pad_ldo 0: none) and clears bound and fix.
struct BoundScan {
    int lists, nbins, kw, cap;
    int32_t *sub_first, *sub_rows, *sub_take;
    uint32_t *bins, *bound;
    int32_t* fix;
    float* pad_d;
    int32_t *pad_pos, *pad_row;
    int32_t pad_ldo;
};
int sampled_bound(const ScanCall& scan, const BoundScan& b);
// the bound scan's index: idx with every bucket cut into at most `lists` lists
lmi_index_desc bound_desc(const lmi_index_desc* idx, int lists, const int32_t* sub_first);

// ---- the split mode (lmi_scan_split.hip; ABI 9, idx->corpus32) ---------------
// Its exact step (lmi_refine.hip): per grouped pair of the collect scan, the
// exact distances of its candidates, sorted, the first k; overflowed pairs
// scanned whole.
struct XArgs {
    const float* rows32;   // [n_rows][d_pad] the caller's float32 rows
    const double* rows64;  // [n_rows][d_pad] float64 rows (idx->corpus64) or null
    int32_t d, d_pad;
    const int32_t* gpos;
    const int64_t* bucket_off;
    int64_t n_rows;
    const float* q;        // [nq][ldq] float32 queries
    int32_t ldq;
    const double* q64;     // float64 queries or null
    int32_t ldq64;
    const int32_t* classes;
    int32_t nq, R, k;
    const int32_t* pair_q;       // grouped pair -> pair id (the collect scan's plan)
    const int32_t* pair_bucket;  // grouped pair -> bucket (-1: none)
    const uint64_t* cand;        // [grouped pair][cap] (ord(d~) << 32 | row)
    const uint32_t* ccount;
    int32_t cap;
    void* out_d;                 // [nq*R][k] float (out_f64 = 0) or double
    int32_t out_f64;
    int32_t* out_pos;
    int32_t* failed;
    int32_t* n_failed;
    int32_t* status;
    // > 0: the candidates are every row under a sampled bound + two_eps; only
    // those within the k-th smallest d~ + two_eps are re-scored
    double two_eps;
    const int32_t* fix;  // [nq*R] pairs without a sampled bound (whole shard), or null
    // ABI 10, the float32 output only: the reference's float32 operation order
    // (oracle blas32_*; lmi_index_desc.corpus32): qn32 [nq][d_pad] the queries
    // normalised as sklearn does in float32 (null: the exact value rounded),
    // grp [R][C] queries of each (round, bucket) group, nrows_c [C] rows of
    // each bucket in the whole index (null: this shard's)
    const float* qn32;
    const int32_t* grp;
    const int64_t* nrows_c;
    int32_t C;
    // (the small kernel's corner block: tailq[pair] = the query is among the
    // last M mod 4 of its group; goff [C+1] the buckets' global offsets)
    const uint8_t* tailq;
    const int64_t* goff;
    const int32_t* plan_counts;  // [C] pairs per bucket (the collect scan's plan)
    // ABI 11: rows32 normalised as sklearn does in float32 (idx->corpus32n) or
    // null (then normalised per candidate)
    const float* rows32n;
    // the grouped pairs x_select_wave_kernel leaves to x_select_kernel (more
    // candidates, overflowed, unbounded), appended by the wave kernel, and
    // their count (null: x_select_kernel walks every grouped pair)
    int32_t* wgl;
    int32_t* n_wgl;
    // the collect scan skipped each split bucket's sample rows (x_collect_desc):
    // soff [2C+1] (bucket c's sample rows [soff[2c], soff[2c+1]), empty where the
    // bucket was collected whole) and skth [nq*R][k] the sample's own lists (the
    // pair's k-th at k - 1); a pair whose band reaches its sample's k-th goes to
    // sfailed (grouped pair ids, count n_sfailed) and x_fallback_kernel scores
    // its sample rows and its candidates exactly.  null: none skipped.  plan_cm:
    // plan_counts has plan_cm entries per bucket, the pairs of bucket c at
    // plan_cm c + plan_cm - 1
    const int64_t* soff;
    const float* skth;
    int32_t* sfailed;
    int32_t* n_sfailed;
    double* spd;     // the sliced sfailed pairs' slice lists (x_fallback_slice_kernel)
    int32_t* spg;
    int32_t plan_cm;
};
// the sliced sample fallback (x_fallback_slice_kernel): the first
// kXSlicedPairs sfailed pairs, kXSlices slices each (XArgs::spd / spg hold
// kXSlicedPairs x kXSlices x k entries)
constexpr int kXSlices = 32;
constexpr int kXSlicedPairs = 256;
int launch_x_refine(const XArgs& a, int64_t P, hipStream_t s);
double split_eps(int d_pad);
size_t x_ws_bytes(const lmi_index_desc* idx, int nq, int R, int k);
size_t x_nfailed_offset(const lmi_index_desc* idx, int nq, int R, int k);
int bucket_topk_x(const lmi_index_desc* idx, const float* q, int32_t nq, int32_t ldq, const double* q64,
                  int32_t ldq64, const int32_t* classes, int32_t R, int32_t k, void* out_d, int out_f64,
                  int32_t* out_pos, int32_t* status, void* workspace, size_t ws_bytes, hipStream_t s,
                  int phases = kPhaseAll);

}  // namespace lmi
