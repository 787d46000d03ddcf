// K6 — router training that steps on every minibatch (lmi_mlp_train_steps).
//
// One step of a Linear/ReLU stack under mean cross-entropy and torch's default
// Adam (what NeuralNetwork.train / train_batch do per optimizer step,
// reference search/li/model.py:150-199), as two kernels on one stream:
//
//   mlp_train_rows_kernel    one workgroup (kRW waves) per 16 rows of the
//       minibatch: gathers the rows x[order[i]], runs every layer on the exact
//       f32 MFMA (v_mfma_f32_16x16x4_f32; A = weights from L2, B = the tile's
//       activations in LDS, as K1's MFMA form), forms softmax, the per-row
//       loss and delta_L = (softmax - onehot) / B_s, and walks back
//       delta_l = (W_l^T delta_{l+1}) * [a_l > 0].  Activations and deltas go
//       to the workspace, zero-padded to 16 columns and 16 rows.
//   mlp_train_update_kernel  one wave per 16x16 tile of some layer's W (plus
//       one per 16 outputs of a bias): dW = delta^T a over the batch rows on
//       the MFMA in a fixed order (four interleaved ascending chains, then a
//       tree), then Adam on that tile of W, exp_avg and exp_avg_sq in place;
//       every weight is owned by one wave.  One more wave sums the per-row
//       losses in a fixed order.
//
// No float atomics, no cross-workgroup waiting: phases and steps are ordered by
// kernel boundaries alone.  Every workspace word a step reads was written by
// the same step's rows kernel, so the workspace needs no initialisation (and
// no memset node under graph capture).  Widths need not be multiples of
// anything: every width is padded to 16 in LDS and in the workspace, and
// weight elements past a row's end are read as zero.
#include "lmi_common.hpp"

#include <cmath>
#include <mutex>

namespace lmi {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kRW = 16;  // waves per workgroup of the rows kernel: they split a layer's 16-wide tiles
constexpr int kTB = 8;   // float4 weight loads a lane has in flight per block of a tile's chain
constexpr int kUB = 8;   // 16-row groups whose operands the update kernel loads at once
constexpr int kTR = 16;  // batch rows per workgroup (the N side of the MFMA)
constexpr int kUW = 4;   // waves (tiles) per workgroup of the update kernel

struct TrainArgs {
    const float* x;
    int64_t n;
    int32_t ldx;
    const int32_t* y;
    const int64_t* order;  // this step's first entry
    int32_t bs;            // rows of this step
    int32_t n_layers;
    int32_t dims[LMI_MAX_LAYERS + 1];
    int32_t pd[LMI_MAX_LAYERS + 1];  // dims rounded up to 16
    float* W[LMI_MAX_LAYERS];
    float* b[LMI_MAX_LAYERS];
    float* mW[LMI_MAX_LAYERS];
    float* vW[LMI_MAX_LAYERS];
    float* mb[LMI_MAX_LAYERS];
    float* vb[LMI_MAX_LAYERS];
    float* act[LMI_MAX_LAYERS];      // act[l] [rows16][pd[l]]: layer l's input (act[0] = the gathered rows)
    float* dlt[LMI_MAX_LAYERS + 1];  // dlt[l] [rows16][pd[l]], l = 1..n_layers: dLoss/d(pre-activation l)
    float* rowloss;                  // [rows16]
    float* loss_out;                 // this step's entry
    int32_t S;                       // LDS row pitch, floats
    int32_t tile_end[LMI_MAX_LAYERS];  // update tiles: running total after layer l
    int32_t n_tiles;
    float inv_bs;
    // Adam (torch's single-tensor form): m += (g - m) * omb1; v = v * beta2 + omb2 * g * g;
    // p -= step_size * (m / (sqrt(v) / bc2_sqrt + eps))
    float omb1, beta2, omb2, step_size, bc2_sqrt, eps;
};

__device__ inline float wave_max(float v) {
#pragma unroll
    for (int x = 32; x >= 1; x >>= 1) v = fmaxf(v, __shfl_xor(v, x));
    return v;
}
// fixed xor tree: the same order in every run (and the same value in every lane)
__device__ inline float wave_sum(float v) {
#pragma unroll
    for (int x = 32; x >= 1; x >>= 1) v += __shfl_xor(v, x);
    return v;
}

// One 16x16 output tile of the rows kernel: c0 + sum over the lane group's k
// quarter [0, kq) of A * B, A = ld(kb) (the lane's four weights at quarter
// offsets kb .. kb + 3, zero past the matrix), B = the tile's activations in LDS.
// A minibatch has few rows (16 workgroups at 256), so the kernel is bound by
// the latency of its weight loads -- the update kernel has just rewritten W on
// other XCDs, so they come from beyond L2 -- not by their bandwidth: a lane
// issues kTB float4 loads before the MFMAs that use them.  The blocks alternate
// between two accumulators, added at the end: a fixed order with dependent
// chains half as long.
template <class LoadA>
__device__ inline f32x4 tile_chain(f32x4 c0, const float* hin, int kq, LoadA ld) {
    f32x4 acc0 = c0, acc1 = {0.f, 0.f, 0.f, 0.f};
    for (int kb0 = 0; kb0 < kq; kb0 += 4 * kTB) {
        float4 a4[kTB];
#pragma unroll
        for (int u = 0; u < kTB; ++u) a4[u] = ld(min(kb0 + 4 * u, kq - 4));  // (clamped: unused past kq)
#pragma unroll
        for (int u = 0; u < kTB; ++u) {
            if (kb0 + 4 * u < kq) {  // wave-uniform
                const float4 b4 = *reinterpret_cast<const float4*>(hin + kb0 + 4 * u);
                f32x4 c = (u & 1) ? acc1 : acc0;
                c = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[u].x, b4.x, c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[u].y, b4.y, c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[u].z, b4.z, c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[u].w, b4.w, c, 0, 0, 0);
                if (u & 1) acc1 = c; else acc0 = c;
            }
        }
    }
    return acc0 + acc1;
}

__global__ __launch_bounds__(64 * kRW) void mlp_train_rows_kernel(TrainArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ int64_t s_idx[kTR];
    __shared__ int32_t s_lab[kTR];
    const int S = a.S;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int ql = lane & 15;  // row of the tile (B / D column)
    const int g = lane >> 4;   // k quarter (A / B) and D row group
    const int r0 = blockIdx.x * kTR;
    const int L = a.n_layers;

    if (tid < kTR) {
        int64_t idx = -1;
        if (r0 + tid < a.bs) {
            idx = a.order[r0 + tid];
            if (idx < 0 || idx >= a.n) idx = -1;  // never read outside x
        }
        s_idx[tid] = idx;
        s_lab[tid] = idx >= 0 ? a.y[idx] : -1;
    }
    __syncthreads();

    // gather the tile's rows, zero-padded to pd[0] columns and kTR rows
    {
        const int din0 = a.dims[0], P0 = a.pd[0];
        for (int e = tid; e < kTR * P0; e += 64 * kRW) {
            const int r = e / P0, c = e - r * P0;
            const int64_t idx = s_idx[r];
            const float v = (idx >= 0 && c < din0) ? a.x[(size_t)idx * a.ldx + c] : 0.0f;
            smem[r * S + c] = v;
            a.act[0][(size_t)(r0 + r) * P0 + c] = v;
        }
    }
    __syncthreads();
    const bool row_ok = r0 + ql < a.bs;

    // ---- forward: a_{j+1} = relu(W_j a_j + b_j); the logits without relu ----
    int cur = 0;
    for (int j = 0; j < L; ++j) {
        const int din = a.dims[j], dout = a.dims[j + 1];
        const int kq = a.pd[j] >> 2;  // k quarter of lane group g: a multiple of 4
        const int Pout = a.pd[j + 1];
        const float* __restrict__ W = a.W[j];
        const float* __restrict__ bias = a.b[j];
        const bool vec = !(din & 3) && !((uintptr_t)W & 15);
        const float* hin = smem + cur * kTR * S + ql * S + g * kq;
        float* hout = smem + (cur ^ 1) * kTR * S + ql * S;
        const bool relu = j + 1 < L;
        for (int t = wave; t < (Pout >> 4); t += kRW) {
            const int orow = 16 * t + ql;  // A row of this lane
            const bool o_ok = orow < dout;
            const float* wr = W + (size_t)(o_ok ? orow : 0) * din;
            f32x4 acc;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int o = 16 * t + 4 * g + v;  // D row of this lane
                acc[v] = o < dout ? bias[o] : 0.0f;
            }
            // loads are unconditional from clamped (in-bounds) addresses, then zeroed past the row
            const auto ld_vec = [&](int kb) {
                const int k = g * kq + kb;
                const float4 w4 = *reinterpret_cast<const float4*>(wr + min(k, din - 4));
                return (o_ok && k < din) ? w4 : make_float4(0.f, 0.f, 0.f, 0.f);
            };
            const auto ld_any = [&](int kb) {
                const int k = g * kq + kb;
                float4 w4;
                w4.x = wr[min(k, din - 1)];
                w4.y = wr[min(k + 1, din - 1)];
                w4.z = wr[min(k + 2, din - 1)];
                w4.w = wr[min(k + 3, din - 1)];
                w4.x = (o_ok && k < din) ? w4.x : 0.0f;
                w4.y = (o_ok && k + 1 < din) ? w4.y : 0.0f;
                w4.z = (o_ok && k + 2 < din) ? w4.z : 0.0f;
                w4.w = (o_ok && k + 3 < din) ? w4.w : 0.0f;
                return w4;
            };
            acc = vec ? tile_chain(acc, hin, kq, ld_vec) : tile_chain(acc, hin, kq, ld_any);
            // outputs past dout are exactly 0 (zero bias, zero A rows): the padding
            float4 o4;
            o4.x = row_ok ? (relu ? fmaxf(acc[0], 0.0f) : acc[0]) : 0.0f;
            o4.y = row_ok ? (relu ? fmaxf(acc[1], 0.0f) : acc[1]) : 0.0f;
            o4.z = row_ok ? (relu ? fmaxf(acc[2], 0.0f) : acc[2]) : 0.0f;
            o4.w = row_ok ? (relu ? fmaxf(acc[3], 0.0f) : acc[3]) : 0.0f;
            *reinterpret_cast<float4*>(hout + 16 * t + 4 * g) = o4;
            if (relu)
                *reinterpret_cast<float4*>(a.act[j + 1] + (size_t)(r0 + ql) * Pout + 16 * t + 4 * g) = o4;
        }
        __syncthreads();
        cur ^= 1;
    }

    // ---- softmax, loss, delta_L (one wave per row, in place over the logits) ----
    {
        const int C = a.dims[L], PC = a.pd[L];
        for (int qq = wave; qq < kTR; qq += kRW) {
            float* zr = smem + cur * kTR * S + qq * S;
            const int row = r0 + qq;
            const bool ok = row < a.bs;
            const int yv = s_lab[qq];
            float m = -__builtin_inff();
            for (int i = lane; i < C; i += 64) m = fmaxf(m, zr[i]);
            m = wave_max(m);
            float sum = 0.0f;
            for (int i = lane; i < C; i += 64) sum += expf(zr[i] - m);
            sum = wave_sum(sum);
            const float zy = (yv >= 0 && yv < C) ? zr[yv] : m;
            const float loss = logf(sum) - (zy - m);
            __builtin_amdgcn_wave_barrier();
            for (int i = lane; i < PC; i += 64) {
                float d = 0.0f;
                if (ok && i < C) d = (expf(zr[i] - m) / sum - (i == yv ? 1.0f : 0.0f)) * a.inv_bs;
                zr[i] = d;
                a.dlt[L][(size_t)row * PC + i] = d;
            }
            if (lane == 0) a.rowloss[row] = (ok && yv >= 0 && yv < C) ? loss : 0.0f;
        }
    }
    __syncthreads();

    // ---- backward: delta_j = (W_j^T delta_{j+1}) * [a_j > 0], j = L-1 .. 1 ----
    for (int j = L - 1; j >= 1; --j) {
        const int din = a.dims[j], dout = a.dims[j + 1];
        const int oq = a.pd[j + 1] >> 2;  // quarter of the summed (output) index
        const int Pi = a.pd[j];
        const float* __restrict__ W = a.W[j];
        const float* hin = smem + cur * kTR * S + ql * S + g * oq;
        float* hout = smem + (cur ^ 1) * kTR * S + ql * S;
        for (int t = wave; t < (Pi >> 4); t += kRW) {
            const int i = 16 * t + ql;  // A row of this lane: an input neuron of layer j
            const bool i_ok = i < din;
            const float* wc = W + (i_ok ? i : 0);
            const auto ld = [&](int kb) {
                const int o = g * oq + kb;
                float4 w4;
                w4.x = wc[(size_t)min(o, dout - 1) * din];
                w4.y = wc[(size_t)min(o + 1, dout - 1) * din];
                w4.z = wc[(size_t)min(o + 2, dout - 1) * din];
                w4.w = wc[(size_t)min(o + 3, dout - 1) * din];
                w4.x = (i_ok && o < dout) ? w4.x : 0.0f;
                w4.y = (i_ok && o + 1 < dout) ? w4.y : 0.0f;
                w4.z = (i_ok && o + 2 < dout) ? w4.z : 0.0f;
                w4.w = (i_ok && o + 3 < dout) ? w4.w : 0.0f;
                return w4;
            };
            const f32x4 acc = tile_chain(f32x4{0.f, 0.f, 0.f, 0.f}, hin, oq, ld);
            // the mask: a_j as this same lane stored it in the forward pass
            // (same tile-to-wave and D layout), zero in the padding
            const size_t off = (size_t)(r0 + ql) * Pi + 16 * t + 4 * g;
            const float4 h4 = *reinterpret_cast<const float4*>(a.act[j] + off);
            float4 o4;
            o4.x = h4.x > 0.0f ? acc[0] : 0.0f;
            o4.y = h4.y > 0.0f ? acc[1] : 0.0f;
            o4.z = h4.z > 0.0f ? acc[2] : 0.0f;
            o4.w = h4.w > 0.0f ? acc[3] : 0.0f;
            *reinterpret_cast<float4*>(hout + 16 * t + 4 * g) = o4;
            *reinterpret_cast<float4*>(a.dlt[j] + off) = o4;
        }
        __syncthreads();
        cur ^= 1;
    }
}

__device__ inline void adam(const TrainArgs& a, float* p, float* m, float* v, float gr) {
    const float m1 = *m + (gr - *m) * a.omb1;
    const float v1 = *v * a.beta2 + a.omb2 * gr * gr;
    *m = m1;
    *v = v1;
    *p = *p + (-a.step_size * m1) / (sqrtf(v1) / a.bc2_sqrt + a.eps);
}

__global__ __launch_bounds__(64 * kUW) void mlp_train_update_kernel(TrainArgs a) {
    const int wid = blockIdx.x * kUW + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (wid > a.n_tiles) return;
    if (wid == a.n_tiles) {
        // the step's loss: lane partials over rows lane, lane + 64, ... then the xor tree
        float s = 0.0f;
        for (int r = lane; r < a.bs; r += 64) s += a.rowloss[r];
        s = wave_sum(s);
        if (lane == 0) *a.loss_out = s / (float)a.bs;
        return;
    }
    int j = 0;
    while (wid >= a.tile_end[j]) ++j;
    const int local = wid - (j ? a.tile_end[j - 1] : 0);
    const int din = a.dims[j], dout = a.dims[j + 1];
    const int Pi = a.pd[j], Po = a.pd[j + 1];
    const int nti = (Pi >> 4) + 1;  // the last "column tile" is the bias
    const int to = local / nti, ti = local - to * nti;
    const bool is_bias = ti == (Pi >> 4);
    const int ql = lane & 15, g = lane >> 4;
    const float* __restrict__ dl = a.dlt[j + 1] + 16 * to + ql;        // A[o][k = row]
    const float* __restrict__ ac = a.act[j] + (is_bias ? 0 : 16 * ti + ql);  // B[k = row][i]
    const int K = (a.bs + 15) & ~15;  // rows past bs hold zero deltas
    // four independent chains (rows 4u + g of every 16, u = 0..3), each in
    // ascending row order, then a fixed tree: shorter dependent chains for the
    // MFMA pipe and a smaller rounding error than one chain of B_s terms
    f32x4 part[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) part[u] = f32x4{0.f, 0.f, 0.f, 0.f};
    // kUB groups of 16 rows per block, every load of a block in flight before
    // its MFMAs (the operands were written by the rows kernel on other CUs:
    // latency again); rows are clamped below K, groups past K skipped
    for (int kk = 0; kk < K; kk += 16 * kUB) {
        float av[kUB][4], bv[kUB][4];
#pragma unroll
        for (int w = 0; w < kUB; ++w)
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const size_t r = min(kk + 16 * w + 4 * u + g, K - 1);
                av[w][u] = dl[r * Po];
                bv[w][u] = is_bias ? 1.0f : ac[r * Pi];
            }
#pragma unroll
        for (int w = 0; w < kUB; ++w)
            if (kk + 16 * w < K)  // wave-uniform
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    part[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[w][u], bv[w][u], part[u], 0, 0, 0);
    }
    const f32x4 acc = (part[0] + part[1]) + (part[2] + part[3]);
    const int i = 16 * ti + ql;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        const int o = 16 * to + 4 * g + v;
        if (o >= dout) continue;
        if (is_bias) {
            if (ql == 0) adam(a, a.b[j] + o, a.mb[j] + o, a.vb[j] + o, acc[v]);
        } else if (i < din) {
            const size_t e = (size_t)o * din + i;
            adam(a, a.W[j] + e, a.mW[j] + e, a.vW[j] + e, acc[v]);
        }
    }
}

inline int pad16(int v) { return (v + 15) & ~15; }

// floats of workspace for minibatches of `batch` rows; offsets filled when asked
size_t train_ws_floats(const lmi_mlp_train_desc* d, int64_t batch, size_t* act_off, size_t* dlt_off,
                       size_t* loss_off) {
    const size_t rows = (size_t)((batch + 15) / 16 * 16);
    size_t off = 0;
    for (int l = 0; l < d->n_layers; ++l) {
        if (act_off) act_off[l] = off;
        off += rows * pad16(d->dims[l]);
    }
    for (int l = 1; l <= d->n_layers; ++l) {
        if (dlt_off) dlt_off[l] = off;
        off += rows * pad16(d->dims[l]);
    }
    if (loss_off) *loss_off = off;
    off += rows;
    return off;
}

int check_desc(const lmi_mlp_train_desc* d) {
    LMI_CHECK_ARG(d != nullptr, "null descriptor");
    LMI_CHECK_ARG(d->n_layers >= 1 && d->n_layers <= LMI_MAX_LAYERS, "n_layers out of range");
    for (int l = 0; l <= d->n_layers; ++l)
        LMI_CHECK_ARG(d->dims[l] >= 1 && d->dims[l] <= LMI_TRAIN_MAX_DIM,
                      "dims[%d] = %d outside 1..%d", l, d->dims[l], LMI_TRAIN_MAX_DIM);
    return LMI_OK;
}

}  // namespace
}  // namespace lmi

extern "C" size_t lmi_mlp_train_workspace_bytes(const lmi_mlp_train_desc* desc, int32_t batch) {
    using namespace lmi;
    if (check_desc(desc) != LMI_OK || batch < 1) return 0;
    return align_up(train_ws_floats(desc, batch, nullptr, nullptr, nullptr) * sizeof(float), 256);
}

extern "C" int lmi_mlp_train_steps(const lmi_mlp_train_desc* desc, const float* x, int64_t n,
                                   int32_t ldx, const int32_t* y, const int64_t* order,
                                   int64_t n_order, int32_t batch, int64_t first_step,
                                   int64_t n_steps, int64_t adam_t0, double lr, double beta1,
                                   double beta2, double eps, float* loss_out, void* workspace,
                                   size_t ws_bytes, void* stream) {
    using namespace lmi;
    LMI_TRY(check_desc(desc));
    LMI_CHECK_ARG(x && y && order && loss_out && workspace, "null pointer");
    const int L = desc->n_layers;
    for (int l = 0; l < L; ++l)
        LMI_CHECK_ARG(desc->W[l] && desc->b[l] && desc->W_exp_avg[l] && desc->W_exp_avg_sq[l] &&
                          desc->b_exp_avg[l] && desc->b_exp_avg_sq[l],
                      "null parameter or moment pointer of layer %d", l);
    LMI_CHECK_ARG(batch >= 1, "batch < 1");
    LMI_CHECK_ARG(n >= 1 && n_order >= 1, "n < 1 or n_order < 1");
    LMI_CHECK_ARG(ldx >= desc->dims[0], "ldx < input width");
    LMI_CHECK_ARG(first_step >= 0 && n_steps >= 0 && adam_t0 >= 0, "negative step count");
    LMI_CHECK_ARG(first_step <= n_order / batch && first_step * (int64_t)batch < n_order,
                  "first_step * batch >= n_order");
    const int64_t steps_total = (n_order + batch - 1) / batch;
    LMI_CHECK_ARG(n_steps <= steps_total - first_step, "steps past the end of order");
    LMI_CHECK_ARG(lr >= 0.0 && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 &&
                      eps >= 0.0, "bad Adam hyperparameter");
    if (((uintptr_t)workspace & 15) != 0) {
        set_error("workspace not 16-byte aligned");
        return LMI_E_WORKSPACE;
    }
    const size_t need = lmi_mlp_train_workspace_bytes(desc, batch);
    if (ws_bytes < need) {
        set_error("train workspace too small (%zu < %zu bytes)", ws_bytes, need);
        return LMI_E_WORKSPACE;
    }
    if (n_steps == 0) return LMI_OK;

    TrainArgs a{};
    a.x = x;
    a.n = n;
    a.ldx = ldx;
    a.y = y;
    a.n_layers = L;
    size_t act_off[LMI_MAX_LAYERS], dlt_off[LMI_MAX_LAYERS + 1], loss_off;
    train_ws_floats(desc, batch, act_off, dlt_off, &loss_off);
    float* ws = static_cast<float*>(workspace);
    int maxp = 0, tiles = 0;
    for (int l = 0; l <= L; ++l) {
        a.dims[l] = desc->dims[l];
        a.pd[l] = pad16(desc->dims[l]);
        maxp = maxp > a.pd[l] ? maxp : a.pd[l];
    }
    for (int l = 0; l < L; ++l) {
        a.W[l] = desc->W[l];
        a.b[l] = desc->b[l];
        a.mW[l] = desc->W_exp_avg[l];
        a.vW[l] = desc->W_exp_avg_sq[l];
        a.mb[l] = desc->b_exp_avg[l];
        a.vb[l] = desc->b_exp_avg_sq[l];
        a.act[l] = ws + act_off[l];
        a.dlt[l + 1] = ws + dlt_off[l + 1];
        tiles += (a.pd[l + 1] / 16) * (a.pd[l] / 16 + 1);
        a.tile_end[l] = tiles;
    }
    a.rowloss = ws + loss_off;
    a.n_tiles = tiles;
    // rows 16-B aligned at a pitch of 4 mod 64 floats (K1's pitch: float4 reads
    // of 16 lanes cover all banks once)
    a.S = (maxp + 63) / 64 * 64 + 4;
    const size_t lds = (size_t)2 * kTR * a.S * sizeof(float);  // <= 136 KiB at width 1024
    static std::once_flag once;
    static hipError_t attr_err = hipSuccess;
    std::call_once(once, [] {
        attr_err = hipFuncSetAttribute((const void*)mlp_train_rows_kernel,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024);
    });
    LMI_HIP_TRY(attr_err);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    a.omb1 = (float)(1.0 - beta1);
    a.beta2 = (float)beta2;
    a.omb2 = (float)(1.0 - beta2);
    a.eps = (float)eps;
    for (int64_t i = 0; i < n_steps; ++i) {
        const int64_t st = first_step + i;
        const int64_t left = n_order - st * batch;
        a.order = order + st * batch;
        a.bs = (int32_t)(left < batch ? left : batch);
        a.inv_bs = 1.0f / (float)a.bs;
        a.loss_out = loss_out + i;
        // torch.optim.Adam (single tensor): the bias corrections in double
        const double t = (double)(adam_t0 + i + 1);
        const double bc1 = 1.0 - std::pow(beta1, t);
        const double bc2 = 1.0 - std::pow(beta2, t);
        a.step_size = (float)(lr / bc1);
        a.bc2_sqrt = (float)std::sqrt(bc2);
        hipLaunchKernelGGL(mlp_train_rows_kernel, dim3((a.bs + kTR - 1) / kTR), dim3(64 * kRW), lds,
                           s, a);
        LMI_LAUNCH_CHECK("mlp_train_rows_kernel");
        hipLaunchKernelGGL(mlp_train_update_kernel, dim3((tiles + 1 + kUW - 1) / kUW),
                           dim3(64 * kUW), 0, s, a);
        LMI_LAUNCH_CHECK("mlp_train_update_kernel");
    }
    return LMI_OK;
}
