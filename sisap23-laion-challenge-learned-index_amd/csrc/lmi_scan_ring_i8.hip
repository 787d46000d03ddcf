// scan3_i8_kernel: the 8-wave ring (scan3_kernel, lmi_scan3.hpp) on the int8
// codes of the 8-bit storage (LMI_I8 / LMI_Q_I8), d_pad == 768, k <= 16 (lists
// of 10 or 16 entries), plain and tagged.  The family ScanKernel::Ring8I8 of
// the scan's plan; every other 8-bit shape stays on scan_i8_kernel
// (lmi_scan_v12.hip), which LMI_SCAN_V1=1 also forces here.  The lists are
// scan_i8_kernel's bit for bit: the integer sums are exact and the distance
// expression is the same one.
#include "lmi_scan3.hpp"

#include <algorithm>
#include <mutex>
#include <utility>

namespace lmi {
namespace {

using i32x4 = int __attribute__((ext_vector_type(4)));
using i32x16 = int __attribute__((ext_vector_type(16)));

// ---------------------------------------------------------------------------
// The fp16 ring's structure (header comment of lmi_scan3.hpp) with these
// differences:
//
//   per wave : 32 queries, their int8 codes in 96 VGPRs for the whole tile (24
//              B fragments of 16 bytes a lane); v_mfma_i32_32x32x32_i8 through
//              the builtin (96 query registers leave room for accumulators
//              wherever the compiler puts them, and it places the hazard
//              waits itself), 24 per 32-row block
//   k map    : scan_i8_kernel's -- MFMA t = 4 kb + s of a block, lane half h:
//              k = 128 kb + 64 h + 16 s + [0, 16), for A and B alike
//   ring     : two 32-row blocks of three stages (32 rows x 256 k bytes); a
//              stage is 8 pieces (one 1-KiB DMA each) of four rows, wave w
//              brings piece w of every stage (rows 4w .. 4w+3 whole), their 4
//              norms and, tagged, their 4 tag words; one s_barrier per block
//   lists    : KL = 10 or 16 entries a lane in LDS (k <= 10, k = 11..16: the
//              over-fetch of a re-rank), lane-interleaved, as in the fp16 ring;
//              the tagged form keeps the pair's value and mask words in
//              registers (there is room here) and reads the row's tag from LDS
//   not here : seeds, join workgroups, the tail split, nearest-chunk-first,
//              lower bounds, the wide / collect / band modes, ABL variants
// ---------------------------------------------------------------------------
namespace r8 {
constexpr int D = 768;                 // bytes of a row
constexpr int KST = 256;               // k bytes of a row in one stage
constexpr int NST = D / KST;           // stages per 32-row block
// LDS image of a piece: four rows interleaved at 16-B granularity (row 4p+x,
// 16-B chunk c of the stage at 64c + 16x), pieces at a 1088-B pitch.  Row r
// chunk c then sits at (r>>2)*1088 + 16(r&3) + 64c, affine in c (one base
// register + immediate offsets), and its 16-B bank slot is
// (68(r>>2) + (r&3) + 4c) mod 16 = (r + 4c) mod 16: every lane of a half reads
// the same c, and each 16-lane group of ds_read_b128 ({0-3,12-15,20-27},
// {4-11,16-19,28-31} of a half) holds 16 rows that differ mod 16, so the 16
// lanes of a group fall on the 16 slots of the 256-B bank row: no conflict.
// (Without the 64-B pad the slot would be (r&3) + 4c: four-way.)
constexpr int PIECEP = 4 * KST + 64;   // piece pitch
constexpr int STAGE = 8 * PIECEP;
constexpr int BLOCK = NST * STAGE;
constexpr int NORM_OFF = 2 * BLOCK;          // the 32 norms of each of the three blocks in flight
constexpr int TAG_OFF = NORM_OFF + 3 * 128;  // their 32 tag words (tagged form)
constexpr int LIST_OFF = TAG_OFF + 3 * 128;
constexpr int NW = 8;
constexpr int QB = NW * 32;
constexpr int NQF = D / 32;            // B fragments (and MFMAs per block)
// KL entries a lane: 94 016 bytes for KL = 10, 118 592 for KL = 16 (one
// 512-thread workgroup a CU either way)
template <int KL>
constexpr size_t kLds = (size_t)LIST_OFF + (size_t)NW * 64 * KL * 8 + 64;
static_assert(kLds<16> <= 160 * 1024, "LDS budget");
static_assert(QB == v3::QB, "the plan's tile width");
}  // namespace r8

// TAG (lmi_bucket_topk_tagged / _masked): MODE 4's rule -- a row is a candidate
// of a pair only if (tag & mask) == value; invq holds (1/|q|, value, mask)
// triples; the test runs before the list is touched.
template <int KL, bool TAG>
__global__ __launch_bounds__(512, 1) void scan3_i8_kernel(Scan2Args a) {
    static_assert(KL == 10 || KL == 16, "10- or 16-entry lists");
    using namespace r8;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* ring = smem;
    // entry i of lane l of wave w at LIST_OFF + w * 512 KL + i * 512 + l * 8
    uint64_t* lists = reinterpret_cast<uint64_t*>(smem + LIST_OFF);
    int* wtab = reinterpret_cast<int*>(lists + NW * 64 * KL);  // [NW] SIMD ids, [NW] tile
    int& s_tile = wtab[NW];
    const int8_t* corpus = reinterpret_cast<const int8_t*>(a.corpus);
    const int8_t* qbuf = reinterpret_cast<const int8_t*>(a.qbuf);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ng = a.ng;

    // SIMD-balanced slot of this wave: order waves by (rank on their SIMD, SIMD)
    int simd, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID, 4, 2)" : "=s"(simd));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID, 0, 4)" : "=s"(xcc));
    if (lane == 0) wtab[wave] = simd;
    __syncthreads();
    int slot = 0;
    {
        int key_me = simd;
        for (int w = 0; w < wave; ++w) key_me += (wtab[w] == simd) ? 4 : 0;  // + rank * 4
        for (int w = 0; w < NW; ++w) {
            int kw = wtab[w];
            for (int v = 0; v < w; ++v) kw += (wtab[v] == wtab[w]) ? 4 : 0;
            slot += (kw < key_me || (kw == key_me && w < wave)) ? 1 : 0;
        }
        slot = __builtin_amdgcn_readfirstlane(slot);
    }
    const int gx = xcc & (ng - 1);
    const bool late = slot >= NW / 2;
    const uint32_t lbase = (uint32_t)(uintptr_t)(lists + wave * 64 * KL) + (uint32_t)lane * 8u;  // this lane's list

    for (;;) {
        if (tid == 0) s_tile = dequeue_tile(a.meta, a.work, gx, ng);
        __syncthreads();
        const int t = __builtin_amdgcn_readfirstlane(s_tile);
        if (t < 0) break;
        const Tile tile = a.tiles[t];
        const int64_t row0 = a.bucket_off[tile.c] + (int64_t)tile.chunk * a.chunk_rows;
        const int nrows = __builtin_amdgcn_readfirstlane(
            (int)std::min<int64_t>(a.chunk_rows, a.bucket_off[tile.c + 1] - row0));
        const uint32_t r0lo = __builtin_amdgcn_readfirstlane((uint32_t)row0);
        const uint32_t r0hi = __builtin_amdgcn_readfirstlane((uint32_t)(row0 >> 32));
        const int64_t row0u = (int64_t)(((uint64_t)r0hi << 32) | r0lo);
        const int np = __builtin_amdgcn_readfirstlane(tile.np);
        const bool wave_live = 32 * slot < np;
        const int h = opaque(lane) >> 5;
        const int col = lane & 31;
        const bool live = 32 * slot + col < np;
        const int pp = tile.pp0 + 32 * slot + col;

        // the descriptors' sizes are the chunk's real bytes: rows past its end
        // read as zeros (norms and tag words too) and are masked by the row count
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
            (void*)(corpus + row0u * D), (short)0, nrows * D, 0x00020000);
        const __amdgpu_buffer_rsrc_t rn = __builtin_amdgcn_make_buffer_rsrc(
            (void*)(a.inv_norm + row0u), (short)0, nrows * 4, 0x00020000);
        const __amdgpu_buffer_rsrc_t rt = __builtin_amdgcn_make_buffer_rsrc(
            TAG ? (void*)(a.tags + row0u) : (void*)(a.inv_norm + row0u), (short)0, nrows * 4, 0x00020000);

        const int nblk = (nrows + 31) / 32;
        // This wave's share of block b, into the slots of block b & 1: piece
        // `wave` of every stage (lane l: row 4w + (l & 3), chunk l >> 2 of the
        // stage, to LDS slot l of the piece), the 4 norms and the 4 tag words
        // (area b % 3: the late waves read block b's during block b + 1).
        auto dma_block = [&](int b) {
            unsigned char* dst = ring + (b & 1) * BLOCK + wave * PIECEP;
            const uint32_t vo = (uint32_t)((4 * wave + (lane & 3)) * D + (lane >> 2) * 16);
#pragma unroll
            for (int j = 0; j < NST; ++j)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_t)(dst + j * STAGE), 16, vo,
                                                         b * (32 * D) + j * KST, 0, 0);
            if (lane < 4) {
                const uint32_t v4 = (uint32_t)((4 * wave + opaque(lane)) * 4);
                const int area = (b % 3) * 128 + 16 * wave;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rn, (lds_t)(ring + NORM_OFF + area), 4, v4, b * 128, 0, 0);
                if constexpr (TAG)
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rt, (lds_t)(ring + TAG_OFF + area), 4, v4, b * 128, 0, 0);
            }
        };
        // Block 0's DMA goes out before the query fragments are loaded (the
        // ring is free: the previous tile drained it before its closing barrier)
        dma_block(0);

        i32x4 qf[NQF];
        // the lane's bound: only rows with ord(d) <= thr can enter the pair's
        // top-KL (a distance word: the bound may come from another chunk, so
        // ties at it survive to the chunk merge)
        uint32_t thr = 0u;
        float my_invq = 0.0f;
        uint32_t want = 0u, tmask = 0u;
        int cnt = 0;  // entries in this lane's list; < KL: an unsorted append buffer
        if (wave_live) {
            const int q = live ? a.pair_q[pp] / a.R : 0;
            const i32x4* qrow = reinterpret_cast<const i32x4*>(qbuf + (size_t)q * D) + 4 * h;
            // dead columns of a partial wave multiply zeros
            const i32x4 z{};
#pragma unroll
            for (int s = 0; s < NQF; ++s) qf[s] = live ? qrow[8 * (s >> 2) + (s & 3)] : z;
            thr = live ? (uint32_t)(a.thr_g[pp] >> 32) : 0u;  // dead slots reject everything
            if constexpr (TAG) {
                const uint32_t* iw = reinterpret_cast<const uint32_t*>(a.invq) + 3 * (size_t)q;
                my_invq = live ? __uint_as_float(iw[0]) : 0.0f;
                want = live ? iw[1] : 0u;
                tmask = live ? iw[2] : 0u;
            } else {
                my_invq = live ? a.invq[q] : 0.0f;
            }
        }
        {
            uint64_t E[KL];
            list_clear<KL>(E);
            list_store<KL>(opaque_u(lbase), E);
        }
        __builtin_amdgcn_s_waitcnt(waitcnt_vm(0));
        __syncthreads();

        // a lane's A-fragment base inside a block (row col, half h: + 64 h k bytes)
        const uint32_t lane_off = (uint32_t)((col >> 2) * PIECEP + (col & 3) * 16 + h * 256);

        i32x16 acc{};
        uint32_t xg_carry = 0xffffffffu;  // global bound fetched, not yet applied
        // ---- epilogue of block eb (the sums of its 24 MFMAs in acc) ----------
        auto epilogue = [&](int eb) {
            const int ln = opaque(lane);
            const int hh = ln >> 5;
            const unsigned char* nb = ring + NORM_OFF + (eb % 3) * 128 + hh * 16;
            const int vr = nrows - eb * 32 - 4 * hh;  // valid rows past this lane's offset
            thr = std::min(thr, xg_carry);
            xg_carry = 0xffffffffu;
            const float bound = key_dist_bound((uint64_t)thr << 32);
            // |acc| <= 768 * 127^2 < 2^24: the conversion is exact
            f32x16 accf;
#pragma unroll
            for (int i = 0; i < 16; ++i) accf[i] = (float)acc[i];
            // the filter: a candidate mask, one bit per register, register 0
            // in bit 15; only the chunk's last block checks the row count
            uint32_t mask = 0;
            auto filter = [&]<bool TAIL>() {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 n4 = *reinterpret_cast<const f32x4*>(nb + 32 * g);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float d = fmaf(-accf[4 * g + e], my_invq * n4[e], 1.0f);
                        bool ok = d <= bound;
                        if (TAIL) ok = ok && e + 8 * g < vr;
                        mask = mask + mask + (ok ? 1u : 0u);
                    }
                }
            };
            if (eb + 1 < nblk)
                filter.template operator()<false>();
            else
                filter.template operator()<true>();
            if (__any(mask != 0)) {
                const uint32_t rb = (uint32_t)(row0u + eb * 32 + 4 * hh);
                // every lane walks its own candidates, lowest register first
                // (rows ascending: a list ordered by distance with equal
                // distances in arrival order is ordered by key)
                uint32_t m = mask;
                const uint32_t la = opaque_u(lbase);
#pragma unroll 1
                while (__any(m != 0)) {
                    if (m != 0) {
                        const int hb = 31 - __builtin_clz(m);
                        m ^= 1u << hb;
                        const int rg = 15 - hb;
                        const int i = (rg & 3) + 8 * (rg >> 2);
                        const float n1 = *reinterpret_cast<const float*>(nb + i * 4);
                        const float d = fmaf(-select16(accf, rg), my_invq * n1, 1.0f);
                        const uint64_t key = make_key(d, rb + (uint32_t)i);
                        bool tag_ok = true;
                        if constexpr (TAG) {
                            const uint32_t tg = lds_get_u32((uint32_t)(uintptr_t)(ring + TAG_OFF) +
                                                            (uint32_t)((eb % 3) * 128 + hh * 16 + i * 4));
                            tag_ok = (tg & tmask) == want;
                        }
                        if (!tag_ok) {
                            // the row lacks a wanted bit or has an avoided one: not a candidate
                        } else if (cnt < KL) {
                            // append mode: the first KL candidates are stored
                            // unsorted; a full buffer is sorted once (stable)
                            lds_put_u64(la + (uint32_t)cnt * 512u, key);
                            if (++cnt == KL) {
                                uint64_t L[KL];
                                list_load<KL>(la, L);
                                list_sort_hi<KL>(L);
                                list_store<KL>(la, L);
                                thr = std::min(thr, (uint32_t)(L[KL - 1] >> 32));
                            }
                        } else {
                            uint64_t L[KL];
                            list_load<KL>(la, L);
                            if ((uint32_t)(key >> 32) < (uint32_t)(L[KL - 1] >> 32)) {
                                list_insert_hi<KL>(L, key);
                                list_store<KL>(la, L);
                            }
                            thr = std::min(thr, (uint32_t)(L[KL - 1] >> 32));
                        }
                    }
                }
                // every bound is an upper bound of the pair's k-th key: share it
                thr = std::min(thr, partner_u32(thr, hh));
            }
        };
        // The two waves of a SIMD are staggered as in the fp16 ring: the early
        // wave (slots 0-3) runs block b's MFMAs and then its epilogue; the late
        // wave (slots 4-7) runs block b-1's epilogue first (its sums carried
        // across the barrier) and then block b's MFMAs.
        const bool defer = late && wave_live;
        for (int blk = 0; blk < nblk; ++blk) {
            const bool more = blk + 1 < nblk;
            // one barrier per block: this wave's DMA of block blk has landed
            // (nothing newer is in flight yet) and, past the barrier, every
            // wave's has, and every wave is done with block blk-1's slots
            __builtin_amdgcn_s_waitcnt(waitcnt_vm(0));
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            // block blk+1's DMA (its slots are block blk-1's, free past the
            // barrier): the early wave ahead of its MFMAs, the late wave right
            // after its deferred epilogue
            if (more && !late) dma_block(blk + 1);
            if (defer && blk > 0) epilogue(blk - 1);
            if (more && late) dma_block(blk + 1);
            // every 32 blocks: publish this lane's bound to the pair's global
            // bound and take the global one back (tiles of the same pair on
            // other chunks run concurrently); consumed in the next epilogue
            if ((blk & 31) == 31 && live)
                xg_carry = std::min(xg_carry, (uint32_t)(atomicMin(&a.thr_g[pp], ((unsigned long long)thr << 32) | 0xffffffffull) >> 32));
            if (!wave_live) continue;
            {
                const unsigned char* rp = ring + (blk & 1) * BLOCK + opaque_u(lane_off);
                // MFMA tt = 4 kb + s: stage kb >> 1, chunk 8 (kb & 1) + 4 h + s
#define LMI_A8(tt) (*reinterpret_cast<const i32x4*>(rp + ((tt) >> 3) * STAGE + (((tt) >> 2) & 1) * 512 + ((tt) & 3) * 64))
                i32x4 af[NQF];
#pragma unroll
                for (int tt = 0; tt < 3; ++tt) af[tt] = LMI_A8(tt);
#pragma unroll
                for (int tt = 0; tt < NQF; ++tt) {
                    if (tt + 3 < NQF) af[tt + 3] = LMI_A8(tt + 3);
                    acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[tt], qf[tt], tt == 0 ? i32x16{} : acc, 0, 0, 0);
                    // keep the A-fragment reads 3 MFMAs ahead, no further
                    __builtin_amdgcn_sched_barrier(0);
                }
#undef LMI_A8
            }
            if (defer) continue;
            epilogue(blk);
        }
        if (defer && nblk > 0) epilogue(nblk - 1);
        // lanes still in append mode hold an unsorted (EMPTY-padded) buffer
        if (__any(cnt < KL)) {
            if (cnt < KL) {
                uint64_t L[KL];
                list_load<KL>(lbase, L);
                list_sort<KL>(L);
                list_store<KL>(lbase, L);
            }
        }
        __syncthreads();  // every wave's DMA drained (the tail waited vmcnt(0))

        // ---- merge the two partial lists of each query (lanes col, col+32) ----
        if (h == 0 && live) {
            uint64_t L[KL], P[KL];
            list_load<KL, 0>(lbase, L);
            list_load<KL, 32 * 8>(lbase, P);
#pragma unroll
            for (int i = 0; i < KL; ++i) {
                if (P[i] >= L[KL - 1]) break;
                list_insert<KL>(L, P[i]);
            }
            uint64_t* out = a.partial + ((size_t)pp * a.max_chunks + tile.chunk) * KL;
#pragma unroll
            for (int i = 0; i < KL; ++i) out[i] = L[i];
            if (L[KL - 1] != kEmptyKey) atomicMin(&a.thr_g[pp], (unsigned long long)L[KL - 1]);
        }
    }
}

}  // namespace

// one launch of the persistent grid (one workgroup per CU, dynamic LDS); HIP
// events around it while lmi_timing_enable is on
template <int KL, bool TAG>
int launch_scan3_i8(const Scan2Args& b, hipStream_t s) {
    static std::once_flag once;
    static hipError_t attr_err = hipSuccess;
    std::call_once(once, [] {
        attr_err = hipFuncSetAttribute((const void*)scan3_i8_kernel<KL, TAG>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)r8::kLds<KL>);
    });
    LMI_HIP_TRY(attr_err);
    const bool timed = timing().on;
    std::pair<hipEvent_t, hipEvent_t> ev{};
    if (timed) {
        const int rc = timing_record(s, true, ev);
        if (rc != LMI_OK) return rc;
    }
    hipLaunchKernelGGL((scan3_i8_kernel<KL, TAG>), dim3(scan_grid()), dim3(r8::NW * 64), r8::kLds<KL>, s, b);
    LMI_LAUNCH_CHECK("scan3_i8_kernel");
    if (timed) return timing_record(s, false, ev);
    return LMI_OK;
}

template int launch_scan3_i8<10, false>(const Scan2Args&, hipStream_t);
template int launch_scan3_i8<10, true>(const Scan2Args&, hipStream_t);
template int launch_scan3_i8<16, false>(const Scan2Args&, hipStream_t);
template int launch_scan3_i8<16, true>(const Scan2Args&, hipStream_t);

}  // namespace lmi
