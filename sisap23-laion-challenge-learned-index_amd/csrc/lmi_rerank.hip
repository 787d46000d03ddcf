// lmi_rerank_f64: exact float64 distances for short candidate lists (gfx950).
//
// The 8-bit storage's scan (lmi_scan_ring_i8.hip, scan_i8_kernel) is fast and
// lossy.  A caller that also holds the fp16 rows over-fetches from it (k_in <=
// LMI_MAX_K candidates a (query, probe)) and re-scores them here: rerank_kernel,
// one wave per pair, computes every live candidate's float64 distance from its
// fp16 row -- row_dist64's bits, the ones lmi_bucket_topk_f64 gives that
// (query, row) -- and writes the k smallest by (d64, position).
//
// The work per pair is one query (q^ in registers) and up to 16 scattered rows
// of 2 d bytes: kRrB rows' loads are issued before the first is used
// (rows_dist64_f16), the k_in distances stay one per lane and are ranked by
// k_in shuffles.  No second kernel, no LDS.
#include "lmi_dist64.hpp"

namespace lmi {
namespace {

constexpr int kRrT = 256;  // 4 waves, one pair each
constexpr int kRrB = 8;    // rows in flight per wave (two batches cover 16 candidates)

struct RerankArgs {
    const _Float16* rows;
    int32_t d, d_pad;
    int64_t n_rows;
    const float* q;
    int32_t ldq;
    int64_t P;  // nq * R
    int32_t R, k_in, k;
    const int32_t* in_pos;  // [P][k_in], -1 = empty
    double* out_d;          // [P][k]
    int32_t* out_pos;
    int32_t* status;
};

// NP: pieces of 4 per lane held for the query (3: d <= 768; 4: d <= 1024)
template <int NP>
__global__ __launch_bounds__(kRrT) void rerank_kernel(RerankArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * (kRrT / 64) + (threadIdx.x >> 6);
    if (p >= a.P) return;  // (wave-uniform)
    const int k = a.k, k_in = a.k_in;
    // lane l < k_in holds candidate l, wherever the empty entries lie
    const int32_t pos = lane < k_in ? a.in_pos[(size_t)p * k_in + lane] : -1;
    if (pos >= 0 && (int64_t)pos >= a.n_rows) atomicOr(a.status, LMI_STATUS_INTERNAL);
    const bool live = pos >= 0 && (int64_t)pos < a.n_rows;
    const uint64_t lmask = __ballot(live);
    double* od = a.out_d + (size_t)p * k;
    int32_t* op = a.out_pos + (size_t)p * k;
    const int m = __popcll(lmask);
    if (m == 0) {
        if (lane < k) {
            od[lane] = __builtin_inf();
            op[lane] = -1;
        }
        return;
    }
    const int nps = (a.d + 255) / 256;
    double qh[NP][4];
    query_hat<float, NP>(a.q + (size_t)(p / a.R) * a.ldq, a.d, nps, qh);
    double mine = __builtin_inf();
    if (a.d % 4 == 0) {
        for (uint64_t rest = lmask; rest != 0ull;) {
            int32_t r[kRrB];
            int src[kRrB];
#pragma unroll
            for (int b = 0; b < kRrB; ++b) {
                src[b] = rest != 0ull ? (int)__builtin_ctzll(rest) : -1;
                rest &= rest - 1ull;  // (0 stays 0)
                const int32_t x = __shfl(pos, src[b] < 0 ? 0 : src[b]);
                r[b] = src[b] < 0 ? -1 : x;
            }
            double dv[kRrB];
            rows_dist64_f16<NP, kRrB>(a.rows, (size_t)a.d_pad, r, a.d, nps, qh, dv);
#pragma unroll
            for (int b = 0; b < kRrB; ++b) mine = lane == src[b] ? dv[b] : mine;
        }
    } else {
        // (a width that is no multiple of 4: whole pieces cannot be loaded; a row at a time)
        for (uint64_t rest = lmask; rest != 0ull; rest &= rest - 1ull) {
            const int src = (int)__builtin_ctzll(rest);
            const int32_t r = __shfl(pos, src);
            const double dv = row_dist64<_Float16, NP>(a.rows + (size_t)r * a.d_pad, a.d, nps, qh);
            mine = lane == src ? dv : mine;
        }
    }
    // rank of every live candidate by (d64, position, list index): equal
    // (distance, position) entries -- a row listed twice -- keep their order
    int rank = 0;
    for (int i = 0; i < k_in; ++i) {
        const double di = __shfl(mine, i);
        const int32_t gi = __shfl(pos, i);
        const bool li = (lmask >> i) & 1ull;
        rank += (li && (lt_dp(di, gi, mine, pos) || (di == mine && gi == pos && i < lane))) ? 1 : 0;
    }
    if (live && rank < k) {
        od[rank] = mine;
        op[rank] = pos;
    }
    if (lane >= m && lane < k) {
        od[lane] = __builtin_inf();
        op[lane] = -1;
    }
}

}  // namespace
}  // namespace lmi

extern "C" int lmi_rerank_f64(const lmi_index_desc* rows, const float* q, int32_t nq, int32_t ldq, int32_t R,
                              const int32_t* in_pos, int32_t k_in, int32_t k, double* out_d, int32_t* out_pos,
                              int32_t* status, void* stream) {
    using namespace lmi;
    LMI_CHECK_ARG(rows != nullptr, "lmi_rerank_f64: null rows descriptor");
    LMI_CHECK_ARG(rows->dtype == LMI_F16, "lmi_rerank_f64: the rows are fp16 (LMI_F16), not dtype %d", rows->dtype);
    LMI_CHECK_ARG(!rows->corpus32 && !rows->corpus64,
                  "lmi_rerank_f64: the split mode (corpus32 / corpus64) is not re-ranked");
    LMI_CHECK_ARG(!rows->chunk_centroid, "lmi_rerank_f64: takes no sub-cluster layout (chunk_centroid)");
    LMI_CHECK_ARG(rows->d >= 1 && rows->d <= 256 * kMaxPieces && rows->d_pad >= rows->d && rows->d_pad % 4 == 0,
                  "lmi_rerank_f64: d=%d outside [1, %d] or d_pad=%d", rows->d, 256 * kMaxPieces, rows->d_pad);
    LMI_CHECK_ARG(rows->n_rows >= 0 && rows->n_rows <= INT32_MAX, "lmi_rerank_f64: bad n_rows");
    LMI_CHECK_ARG(nq >= 0 && R >= 1 && (int64_t)nq * R < INT32_MAX, "lmi_rerank_f64: bad nq/R");
    LMI_CHECK_ARG(k >= 1 && k <= k_in && k_in <= LMI_MAX_K, "lmi_rerank_f64: need 1 <= k <= k_in <= %d, not k=%d k_in=%d",
                  LMI_MAX_K, k, k_in);
    LMI_CHECK_ARG(ldq >= rows->d, "lmi_rerank_f64: ldq < d");
    if (nq == 0) return LMI_OK;
    LMI_CHECK_ARG(q && in_pos && out_d && out_pos && status, "lmi_rerank_f64: null pointer");
    LMI_CHECK_ARG(rows->n_rows == 0 || rows->corpus, "lmi_rerank_f64: null corpus");
    RerankArgs a{};
    a.rows = reinterpret_cast<const _Float16*>(rows->corpus);
    a.d = rows->d;
    a.d_pad = rows->d_pad;
    a.n_rows = rows->n_rows;
    a.q = q;
    a.ldq = ldq;
    a.P = (int64_t)nq * R;
    a.R = R;
    a.k_in = k_in;
    a.k = k;
    a.in_pos = in_pos;
    a.out_d = out_d;
    a.out_pos = out_pos;
    a.status = status;
    const dim3 grid((unsigned)((a.P + kRrT / 64 - 1) / (kRrT / 64)));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (rows->d <= 768)
        hipLaunchKernelGGL(rerank_kernel<3>, grid, dim3(kRrT), 0, s, a);
    else
        hipLaunchKernelGGL(rerank_kernel<4>, grid, dim3(kRrT), 0, s, a);
    LMI_LAUNCH_CHECK("rerank_kernel");
    return LMI_OK;
}
